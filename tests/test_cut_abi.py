"""TRPL_FLAG_CUT and trpl_loglik_cut[_dev] (include/trpl.h: the early stop of systems whose running squared error has
passed the caller's level): header, binding and library agree; the flag is one free bit; the shared object holds exactly
the 20 trpl::cut:: steppers and every one of them is reachable by name; the refusals carry the codes the header states,
with no device present; the flag on any other entry point is TRPL_ERR_ARG before a device is touched; every cut
instantiation has no scratch and its counterpart's occupancy.  No GPU needed."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_loglik_cut", "trpl_loglik_cut_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    hdr = open(os.path.join(ROOT, "include", "trpl.h")).read()          # with its comments: the sentences below
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        n_args = len(H.params(name))
        assert n_args == len(A.SIGNATURES[name]), (name, n_args)
    # the arguments of the moments calls without esum, plus sse_cut and cut_col
    assert len(A.SIGNATURES["trpl_loglik_cut"]) == len(A.SIGNATURES["trpl_loglik_moments"]) + 1
    assert len(A.SIGNATURES["trpl_loglik_cut_dev"]) == len(A.SIGNATURES["trpl_loglik_moments_dev"]) + 1
    proto = ", ".join(H.params("trpl_loglik_cut"))
    assert "double sse_cut" in proto and "int32_t *cut_col" in proto and "esum" not in proto
    defs = H.defines()
    assert defs["TRPL_FLAG_CUT"] == A.FLAG_CUT == 0x800000
    assert defs["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version()          # additive: the version stays
    others = [v for k, v in defs.items() if k.startswith("TRPL_FLAG_") and k != "TRPL_FLAG_CUT"]
    assert A.FLAG_CUT & (A.FLAG_CUT - 1) == 0
    assert not any(A.FLAG_CUT & o for o in others) and not A.FLAG_CUT & (0xF00 | (7 << 14))
    # the sentences the header owes its readers
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "Adding a non-negative term in floating point never decreases a sum, so cut_col >= 0 holds exactly when the plain call's final sse > sse_cut" in flat
    assert "only iters_total <= the plain full call's is promised" in flat
    assert "probs.py:5-18" in hdr and "probs.py:34-35" in hdr
    assert "loglik_cut_device" in dir(trpl.device)


def test_every_cut_kernel_name_exists_in_the_library(trpl):
    A = trpl._abi
    filt = H.demangled()
    have = set(re.findall(r"(trpl::cut::(?:predict::)?(?:pair::)?stepper(?:_pair)?_kernel<[^>]*>)", filt))
    # the one-system FAST kernel at the 8 grids, the paired kernel in both seam forms; each with and without PREDICT
    assert len(have) == 20, sorted(have)
    assert not re.findall(r"cut::moments|moments::cut|cut::weighted|weighted::cut", filt)
    named = set()
    for L, kern, predict, seam in itertools.product((4, 8, 16, 32, 64, 128, 256, 512), (0, A.FLAG_KERNEL_PAIR, A.FLAG_KERNEL_SINGLE),
                                                    (0, A.FLAG_PREDICT), (0, A.FLAG_PAIR_ALWAYS_SEAM)):
        flags = A.FLAG_CUT | kern | predict | seam
        if kern == A.FLAG_KERNEL_PAIR and L != 128:
            with pytest.raises(A.TrplError) as e:
                A.kernel_name(10 ** 6, L, 8000, flags)
            assert e.value.code == A.ERR_ARG
            continue
        name = A.kernel_name(10 ** 6, L, 8000, flags)
        assert name in have and name.startswith("trpl::cut::"), (name, L, hex(flags))
        assert ("predict::" in name) == bool(predict) and ("stepper_pair_kernel" in name) == (
            A.lib().trpl_kernel_variant(10 ** 6, L, 8000, flags) == A.KERNEL_FAST_PAIR)
        # the same classification as without the flag, in the other namespace; no snapshot or STRICT forms
        assert name.replace("cut::", "") == A.kernel_name(10 ** 6, L, 8000, flags & ~A.FLAG_CUT)
        assert "stepper_kernel<%d, false, false, false, false, false>" % L in name or "stepper_pair_kernel<true, false, " in name
        named.add(name)
    assert named == have                                         # nothing is built that no call can reach


def _cut(lib, p, n, flags=0, sse_cut=1.0, L=16, S=1, dev=False, hi=None, dx=None, h=None, plT=1):
    if dev:
        return lib.trpl_loglik_cut_dev(p, S, 1, p, 1.0, L, 10, plT, 7, 100, p, p, hi, dx, h, 1, n, sse_cut, p, p, None, None, None,
                                       None, flags, None)
    return lib.trpl_loglik_cut(p, S, 1, p, 1.0, L, 10, plT, 7, 100, p, p, hi, dx, h, 1, n, sse_cut, p, p, None, None, None, None,
                               flags, 0, None)


def test_refusals_carry_the_stated_codes_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.zeros(64)
    p, n = z.ctypes.data, np.ones(1, dtype=np.int64).ctypes.data
    unsupported = (A.FLAG_STRICT, A.FLAG_FP32, A.FLAG_MIXED, A.FLAG_HIST32, A.flag_bundle(2, 16), A.FLAG_STRICT | A.flag_bundle(3, 16))
    for dev in (False, True):
        for extra in unsupported:
            assert _cut(lib, p, n, flags=extra, dev=dev) == A.ERR_UNSUPPORTED, (dev, hex(extra), lib.trpl_last_error())
            assert b"TRPL_FLAG_CUT" in lib.trpl_last_error()
        for extra, word in ((A.FLAG_MOMENTS, b"TRPL_FLAG_MOMENTS"), (A.FLAG_WEIGHTED, b"TRPL_FLAG_WEIGHTED")):
            assert _cut(lib, p, n, flags=extra, dev=dev) == A.ERR_ARG, (dev, hex(extra))
            assert word in lib.trpl_last_error()
        for bad in (float("nan"), -1.0, -0.5, -float("inf")):
            assert _cut(lib, p, n, sse_cut=bad, dev=dev) == A.ERR_ARG, (dev, bad)
            assert b"sse_cut" in lib.trpl_last_error()
        # validated like its counterparts
        assert _cut(lib, p, n, L=12, dev=dev) == A.ERR_ARG and b"power of two" in lib.trpl_last_error()
        assert _cut(lib, p, n, hi=p, dev=dev) == A.ERR_ARG and b"go together" in lib.trpl_last_error()
        assert _cut(lib, p, n, hi=p, dx=p, h=p, plT=2, dev=dev) == A.ERR_ARG and b"plT = 1" in lib.trpl_last_error()
        assert _cut(lib, None, None, S=0, dev=dev) == 0                       # S == 0: nothing to do
    for ok in (0.0, 1.0, float("inf")):                                       # accepted levels get as far as the device
        assert _cut(lib, p, n, sse_cut=ok) in (A.ERR_NODEVICE, A.OK)
    # the same refusals where a launch is named
    for extra, L in ((A.FLAG_STRICT, 128), (A.FLAG_FP32, 128), (A.FLAG_MIXED, 128), (A.FLAG_HIST32, 256), (A.flag_bundle(2, 128), 128)):
        with pytest.raises(A.TrplError) as e:
            A.kernel_name(1000, L, 100, A.FLAG_CUT | extra)
        assert e.value.code == A.ERR_UNSUPPORTED, (hex(extra), str(e.value))
    with pytest.raises(A.TrplError) as e:
        A.kernel_name(1000, 128, 100, A.FLAG_CUT, snapshots=True)
    assert e.value.code == A.ERR_UNSUPPORTED
    for extra in (A.FLAG_MOMENTS, A.FLAG_WEIGHTED):
        with pytest.raises(A.TrplError) as e:
            A.kernel_name(1000, 128, 100, A.FLAG_CUT | extra)
        assert e.value.code == A.ERR_ARG


def test_the_flag_on_any_other_entry_point_is_an_argument_error_before_a_device_is_touched(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.zeros(64)
    zi = np.zeros(8, dtype=np.int64)
    n1 = np.ones(1, dtype=np.int64)
    F = A.FLAG_CUT
    p = z.ctypes.data
    n = n1.ctypes.data
    calls = {
        "trpl_loglik": lambda: lib.trpl_loglik(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, 1, n, p, p, None, None, None, F, 0, None),
        "trpl_loglik_dev": lambda: lib.trpl_loglik_dev(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, 1, n, p, p, None, None, None, F, None),
        "trpl_loglik_obs": lambda: lib.trpl_loglik_obs(p, 1, 1, p, 1.0, 16, 10, 7, 100, p, p, p, p, p, 1, n, p, p, None, None, None, F, 0, None),
        "trpl_loglik_obs_dev": lambda: lib.trpl_loglik_obs_dev(p, 1, 1, p, 1.0, 16, 10, 7, 100, p, p, p, p, p, 1, n, p, p, None, None, None, F, None),
        "trpl_loglik_moments": lambda: lib.trpl_loglik_moments(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, None, None, None, 1, n, p, p, p, None, None, None, F, 0, None),
        "trpl_loglik_moments_dev": lambda: lib.trpl_loglik_moments_dev(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, None, None, None, 1, n, p, p, p, None, None, None, F, None),
        "trpl_loglik_weighted": lambda: lib.trpl_loglik_weighted(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, p, None, None, None, 1, n, p, p, p, None, None, None, F, 0, None),
        "trpl_loglik_weighted_dev": lambda: lib.trpl_loglik_weighted_dev(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, p, None, None, None, 1, n, p, p, p, None, None, None, F, None),
        "trpl_solve_pl": lambda: lib.trpl_solve_pl(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, F, 0, None),
        "trpl_solve_pl_dev": lambda: lib.trpl_solve_pl_dev(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, F, None),
        "trpl_solve_pl_snap": lambda: lib.trpl_solve_pl_snap(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, zi.ctypes.data, 1, p, None, None, F, 0, None),
        "trpl_solve_pl_resume": lambda: lib.trpl_solve_pl_resume(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, 4, p, p, p, p, 8, 11, None, None, None, 0, None, None, None, F, 0, None),
        "trpl_loglik_from_pl_dev": lambda: lib.trpl_loglik_from_pl_dev(p, 8, 1, 11, 11, p, None, None, None, 5, p, None, p, None, F, None),
        "trpl_loglik_moments_from_pl_dev": lambda: lib.trpl_loglik_moments_from_pl_dev(p, 8, 1, 11, 11, p, None, None, None, 5, p, None, p, None, p, F, None),
        "trpl_loglik_weighted_from_pl_dev": lambda: lib.trpl_loglik_weighted_from_pl_dev(p, 8, 1, 11, 11, p, p, None, None, None, 5, p, None, p, None, None, F, None),
        "trpl_loglik_multi": lambda: lib.trpl_loglik_multi(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, None, None, None, 1, n, p, None, None, None, None, F, None, 0, None),
    }
    for name, call in calls.items():
        assert call() == A.ERR_ARG, name
        assert b"TRPL_FLAG_CUT" in lib.trpl_last_error(), (name, lib.trpl_last_error())


def test_cut_instantiations_keep_their_counterparts_resources():
    """The condition of the feature, checked on the cross-compiled objects (tools/kernel_resources.py; no GPU): every cut
    instantiation has 0 bytes of scratch and its counterpart's occupancy -- 2 waves for the four paired kernels; one-system
    kernels 3 waves (or more) up to L = 128, 2 at L = 256, 1 at L = 512 (figures in DESIGN.md section 12)."""
    units = ("cut_fast", "cut_predict_fast", "cut_pair", "cut_predict_pair")
    counterparts = ("fast", "predict_fast", "pair", "predict_pair")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")] + list(units + counterparts),
                         capture_output=True, text=True, check=True).stdout
    rows = [ln for ln in out.splitlines() if ln.strip()]
    occ_of = {}
    for ln in rows:                                               # (the table cuts a kernel's name at 78 characters)
        unit = ln.split()[0]
        pair = re.search(r"stepper_pair_kernel<([^>]*)>", ln)
        if pair:
            kern = pair.group(1)
        else:
            one = re.search(r"stepper_kernel<(\d+), ([a-z, ]*)", ln)
            if not one:                                           # another kernel of a counterpart's unit
                continue
            L, rest = one.groups()
            if "true" in rest:                                    # STRICT / SNAP / bundle forms of the counterpart units
                continue
            kern = int(L)
        assert (unit, kern) not in occ_of, ln
        occ_of[(unit, kern)] = (int(re.search(r"scratch +(\d+)", ln).group(1)), int(re.search(r"occ (\d+)", ln).group(1)))
    cut_rows = {k: v for k, v in occ_of.items() if k[0] in units}
    assert len(cut_rows) == 2 * 8 + 2 * 2, out
    for (unit, kern), (scratch, occ) in cut_rows.items():
        assert scratch == 0, (unit, kern)
        base_scratch, base_occ = occ_of[(unit.replace("cut_", ""), kern)]     # the same template arguments, without the cut
        assert occ >= base_occ and base_scratch == 0, (unit, kern, occ, base_occ)       # never below its counterpart
        if unit.endswith("pair"):
            assert occ == 2, (unit, kern)
        else:
            assert (occ >= 3) if kern <= 128 else occ == (2 if kern == 256 else 1), (unit, kern, occ)
    assert all("trpl::cut::" in ln for ln in rows if ln.split()[0] in units)
