"""TRPL_FLAG_MOMENTS and the magnitude-offset entry points (include/trpl.h: trpl_loglik_moments, trpl_mag_grid,
trpl_mag_profile -- the mag_grid loop of the reference's probs.lnP, probs.py:5-18, from one solve): header, binding and
library agree; the flag is one free bit; every kernel name the library returns for it exists among the shared object's
kernels, in namespace trpl::moments; the refusals carry the codes the header states; the flag on any other entry point is
TRPL_ERR_ARG before a device is touched.  No GPU needed."""
import itertools
import os
import re

import numpy as np
import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_loglik_moments", "trpl_loglik_moments_dev", "trpl_loglik_moments_from_pl_dev", "trpl_mag_grid",
       "trpl_mag_grid_dev", "trpl_mag_profile", "trpl_mag_profile_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    hdr = open(os.path.join(ROOT, "include", "trpl.h")).read()
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        n_args = len(H.params(name))
        assert n_args == len(A.SIGNATURES[name]), (name, n_args)
    defs = H.defines()
    assert defs["TRPL_FLAG_MOMENTS"] == A.FLAG_MOMENTS == 0x200000
    assert defs["TRPL_MAG_PER_CURVE"] == A.MAG_PER_CURVE
    assert defs["TRPL_MAG_MAX_CURVES"] == A.MAG_MAX_CURVES
    assert defs["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version()          # additive: the version stays
    # one free bit: no other flag of the solver entry points, nor the bundle / BDF-order fields, holds it
    others = [v for k, v in defs.items() if k.startswith("TRPL_FLAG_") and k != "TRPL_FLAG_MOMENTS"]
    assert A.FLAG_MOMENTS & (A.FLAG_MOMENTS - 1) == 0
    assert not any(A.FLAG_MOMENTS & o for o in others) and not A.FLAG_MOMENTS & (0xF00 | (7 << 14))
    assert "probs.py:5-18" in hdr and "trpl_loglik_multi* has no moments form" in hdr


def test_every_moments_kernel_name_exists_in_the_library(trpl):
    A = trpl._abi
    have = set(re.findall(r"(trpl::moments::(?:predict::)?(?:pair::)?stepper(?:_pair)?_kernel<[^>]*>)", H.demangled()))
    # one-system FAST and STRICT at the 8 grids, the paired kernel in both seam forms; each with and without PREDICT
    assert len(have) == 2 * (8 * 2 + 2), sorted(have)
    named = set()
    for L, strict, kern, predict, seam in itertools.product(
            (4, 8, 16, 32, 64, 128, 256, 512), (0, A.FLAG_STRICT), (0, A.FLAG_KERNEL_PAIR, A.FLAG_KERNEL_SINGLE),
            (0, A.FLAG_PREDICT), (0, A.FLAG_PAIR_ALWAYS_SEAM)):
        flags = A.FLAG_MOMENTS | strict | kern | predict | seam
        if kern == A.FLAG_KERNEL_PAIR and (L != 128 or strict):
            with pytest.raises(A.TrplError) as e:
                A.kernel_name(10 ** 6, L, 8000, flags)
            assert e.value.code == A.ERR_ARG
            continue
        name = A.kernel_name(10 ** 6, L, 8000, flags)
        assert name in have and "moments::" in name, (name, L, hex(flags))
        assert ("predict::" in name) == bool(predict) and ("stepper_pair_kernel" in name) == (
            A.lib().trpl_kernel_variant(10 ** 6, L, 8000, flags) == A.KERNEL_FAST_PAIR)
        # the same classification as without the flag, in the other namespace
        assert name.replace("moments::", "") == A.kernel_name(10 ** 6, L, 8000, flags & ~A.FLAG_MOMENTS)
        named.add(name)
    assert named == have                                         # nothing is built that no call can reach


def test_refusals_carry_the_stated_codes(trpl):
    A = trpl._abi
    for extra, L, steps in ((A.FLAG_FP32, 128, 100), (A.FLAG_MIXED, 128, 100), (A.FLAG_HIST32, 256, 100),
                            (A.flag_bundle(2, 128), 128, 100), (A.FLAG_STRICT | A.flag_bundle(3, 64), 64, 100)):
        with pytest.raises(A.TrplError) as e:
            A.kernel_name(1000, L, steps, A.FLAG_MOMENTS | extra)
        assert e.value.code == A.ERR_UNSUPPORTED, (hex(extra), str(e.value))
    with pytest.raises(A.TrplError) as e:                        # no snapshot / resume forms
        A.kernel_name(1000, 128, 100, A.FLAG_MOMENTS, snapshots=True)
    assert e.value.code == A.ERR_UNSUPPORTED


def test_the_flag_on_any_other_entry_point_is_an_argument_error_before_a_device_is_touched(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.zeros(64)
    zi = np.zeros(8, dtype=np.int64)
    n1 = np.ones(1, dtype=np.int64)
    F = A.FLAG_MOMENTS
    p = z.ctypes.data
    calls = {
        "trpl_loglik": lambda: lib.trpl_loglik(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, 1, n1.ctypes.data, p, p, None, None, None, F, 0, None),
        "trpl_loglik_dev": lambda: lib.trpl_loglik_dev(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, 1, n1.ctypes.data, p, p, None, None, None, F, None),
        "trpl_loglik_obs": lambda: lib.trpl_loglik_obs(p, 1, 1, p, 1.0, 16, 10, 7, 100, p, p, p, p, p, 1, n1.ctypes.data, p, p, None, None, None, F, 0, None),
        "trpl_loglik_obs_dev": lambda: lib.trpl_loglik_obs_dev(p, 1, 1, p, 1.0, 16, 10, 7, 100, p, p, p, p, p, 1, n1.ctypes.data, p, p, None, None, None, F, None),
        "trpl_solve_pl": lambda: lib.trpl_solve_pl(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, F, 0, None),
        "trpl_solve_pl_dev": lambda: lib.trpl_solve_pl_dev(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, F, None),
        "trpl_solve_pl_snap": lambda: lib.trpl_solve_pl_snap(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, zi.ctypes.data, 1, p, None, None, F, 0, None),
        "trpl_solve_pl_resume": lambda: lib.trpl_solve_pl_resume(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, 4, p, p, p, p, 8, 11, None, None, None, 0, None, None, None, F, 0, None),
        "trpl_loglik_from_pl_dev": lambda: lib.trpl_loglik_from_pl_dev(p, 8, 1, 11, 11, p, None, None, None, 5, p, None, p, None, F, None),
        "trpl_loglik_multi": lambda: lib.trpl_loglik_multi(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, None, None, None, 1, n1.ctypes.data, p, None, None, None, None, F, None, 0, None),
    }
    for name, call in calls.items():
        assert call() == A.ERR_ARG, name
        assert b"TRPL_FLAG_MOMENTS" in lib.trpl_last_error(), (name, lib.trpl_last_error())
    # the moments entry points validate like their counterparts, without a device
    assert lib.trpl_loglik_moments(p, 1, 1, p, 1.0, 12, 10, 1, 7, 100, p, p, None, None, None, 1, n1.ctypes.data, p, p, p, None, None, None, 0, 0, None) == A.ERR_ARG
    assert b"power of two" in lib.trpl_last_error()
    assert lib.trpl_loglik_moments(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, None, None, None, 1, n1.ctypes.data, p, p, None, None, None, None, 0, 0, None) == A.ERR_ARG
    assert b"esum" in lib.trpl_last_error()
    assert lib.trpl_loglik_moments(None, 0, 1, None, 1.0, 16, 10, 1, 7, 100, None, None, None, None, None, 1, None, None, None, None, None, None, None, 0, 0, None) == 0
    assert lib.trpl_mag_grid_dev(p, p, n1.ctypes.data, 4, A.MAG_MAX_CURVES + 1, p, 1, p, None) == A.ERR_ARG
    assert lib.trpl_mag_profile_dev(p, p, n1.ctypes.data, 4, 1, 0x2, p, p, None) == A.ERR_ARG
