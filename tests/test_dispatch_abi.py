"""The stepper launcher table (csrc/stepper_variants.hpp -> trpl_api.hip: find_launcher): over every grid size x {default,
STRICT, KERNEL_PAIR, KERNEL_SINGLE} x {no sink, MOMENTS, WEIGHTED, CUT} x PREDICT, a combination the launch checks accept
names a kernel that the library holds, and one they refuse carries the code it carried before the table replaced the
hand-written dispatch (tests/golden/dispatch_codes.txt, recorded from the library built at that commit).  No GPU needed."""
import ctypes as C
import itertools
import os
import re

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_accepted_combination_names_a_built_kernel_and_every_refusal_keeps_its_code(trpl):
    A = trpl._abi
    lib = A.lib()
    have = set(re.findall(r"(trpl::(?:\w+::)*stepper(?:_pair)?_kernel<[^>]*>)", H.demangled()))
    want = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "dispatch_codes.txt")):
        if not line.startswith("#"):
            L, flags, code = line.split()
            want[(int(L), int(flags, 0))] = int(code)
    buf = C.create_string_buffer(256)
    swept = accepted = 0
    for L, kern, sink, predict in itertools.product((4, 8, 16, 32, 64, 128, 256, 512),
                                                    (0, A.FLAG_STRICT, A.FLAG_KERNEL_PAIR, A.FLAG_KERNEL_SINGLE),
                                                    (0, A.FLAG_MOMENTS, A.FLAG_WEIGHTED, A.FLAG_CUT), (0, A.FLAG_PREDICT)):
        flags = kern | sink | predict
        rc = lib.trpl_kernel_name(10 ** 6, L, 8000, flags, 0, C.addressof(buf), 256)
        assert rc == want[(L, flags)], (L, hex(flags), rc, lib.trpl_last_error())
        swept += 1
        if rc == A.OK:
            name = buf.value.decode()
            assert name in have, (L, hex(flags), name)
            ns = {0: "", A.FLAG_MOMENTS: "moments::", A.FLAG_WEIGHTED: "weighted::", A.FLAG_CUT: "cut::"}[sink]
            assert name.startswith("trpl::" + ns + ("predict::" if predict else "")), (L, hex(flags), name)
            accepted += 1
        else:
            assert buf.value == b"", (L, hex(flags))
    assert swept == len(want) == 8 * 4 * 4 * 2 and accepted == 184
