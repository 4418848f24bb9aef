"""TRPL_FLAG_WEIGHTED and the uncertainty-weighted entry points (include/trpl.h: trpl_loglik_weighted,
trpl_loglik_weighted_from_pl_dev, trpl_sse_accumulate_w, trpl_mag_grid_w, trpl_mag_profile_w -- the weighting line the
reference has commented out, probs.py:40): header, binding and library agree; the flag is one free bit; the shared object
holds exactly the 36 trpl::weighted:: steppers and every one of them is reachable by name; the refusals carry the codes the
header states; the flag on any other entry point is TRPL_ERR_ARG before a device is touched; the host call checks its
weights without a device.  No GPU needed."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_loglik_weighted", "trpl_loglik_weighted_dev", "trpl_loglik_weighted_from_pl_dev", "trpl_sse_accumulate_w",
       "trpl_sse_accumulate_w_dev", "trpl_mag_grid_w", "trpl_mag_grid_w_dev", "trpl_mag_profile_w", "trpl_mag_profile_w_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    hdr = open(os.path.join(ROOT, "include", "trpl.h")).read()
    assert len(NEW) == 9
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        n_args = len(H.params(name))
        assert n_args == len(A.SIGNATURES[name]), (name, n_args)
    # the arguments of the moments calls plus the weights
    for name, base in (("trpl_loglik_weighted", "trpl_loglik_moments"), ("trpl_loglik_weighted_dev", "trpl_loglik_moments_dev"),
                       ("trpl_loglik_weighted_from_pl_dev", "trpl_loglik_moments_from_pl_dev"),
                       ("trpl_sse_accumulate_w", "trpl_sse_accumulate"), ("trpl_sse_accumulate_w_dev", "trpl_sse_accumulate_dev")):
        assert len(A.SIGNATURES[name]) == len(A.SIGNATURES[base]) + 1, name
    for name in ("trpl_mag_grid", "trpl_mag_grid_dev", "trpl_mag_profile", "trpl_mag_profile_dev"):
        assert len(A.SIGNATURES[name.replace("trpl_mag_grid", "trpl_mag_grid_w").replace("trpl_mag_profile", "trpl_mag_profile_w")]) \
            == len(A.SIGNATURES[name])
    defs = H.defines()
    assert defs["TRPL_FLAG_WEIGHTED"] == A.FLAG_WEIGHTED == 0x400000
    assert defs["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version()          # additive: the version stays
    # one free bit: no other flag of the solver entry points, nor the bundle / BDF-order fields, holds it
    others = [v for k, v in defs.items() if k.startswith("TRPL_FLAG_") and k != "TRPL_FLAG_WEIGHTED"]
    assert A.FLAG_WEIGHTED & (A.FLAG_WEIGHTED - 1) == 0
    assert not any(A.FLAG_WEIGHTED & o for o in others) and not A.FLAG_WEIGHTED & (0xF00 | (7 << 14))
    assert "probs.py:20-62" in hdr and "probs.py:40" in hdr and "bayes_io.py:75-76" in hdr
    assert "trpl_loglik_multi* has no weighted form" in hdr


def test_every_weighted_kernel_name_exists_in_the_library(trpl):
    A = trpl._abi
    filt = H.demangled()
    have = set(re.findall(r"(trpl::weighted::(?:predict::)?(?:pair::)?stepper(?:_pair)?_kernel<[^>]*>)", filt))
    # one-system FAST and STRICT at the 8 grids, the paired kernel in both seam forms; each with and without PREDICT
    assert len(have) == 36, sorted(have)
    assert not re.findall(r"moments::weighted|weighted::moments", filt)
    named = set()
    for L, strict, kern, predict, seam in itertools.product(
            (4, 8, 16, 32, 64, 128, 256, 512), (0, A.FLAG_STRICT), (0, A.FLAG_KERNEL_PAIR, A.FLAG_KERNEL_SINGLE),
            (0, A.FLAG_PREDICT), (0, A.FLAG_PAIR_ALWAYS_SEAM)):
        flags = A.FLAG_WEIGHTED | strict | kern | predict | seam
        if kern == A.FLAG_KERNEL_PAIR and (L != 128 or strict):
            with pytest.raises(A.TrplError) as e:
                A.kernel_name(10 ** 6, L, 8000, flags)
            assert e.value.code == A.ERR_ARG
            continue
        name = A.kernel_name(10 ** 6, L, 8000, flags)
        assert name in have and name.startswith("trpl::weighted::"), (name, L, hex(flags))
        assert ("predict::" in name) == bool(predict) and ("stepper_pair_kernel" in name) == (
            A.lib().trpl_kernel_variant(10 ** 6, L, 8000, flags) == A.KERNEL_FAST_PAIR)
        # the same classification as without the flag, in the other namespace
        assert name.replace("weighted::", "") == A.kernel_name(10 ** 6, L, 8000, flags & ~A.FLAG_WEIGHTED)
        named.add(name)
    assert named == have                                         # nothing is built that no call can reach


def test_refusals_carry_the_stated_codes(trpl):
    A = trpl._abi
    for extra, L, steps in ((A.FLAG_FP32, 128, 100), (A.FLAG_MIXED, 128, 100), (A.FLAG_HIST32, 256, 100),
                            (A.flag_bundle(2, 128), 128, 100), (A.FLAG_STRICT | A.flag_bundle(3, 64), 64, 100)):
        with pytest.raises(A.TrplError) as e:
            A.kernel_name(1000, L, steps, A.FLAG_WEIGHTED | extra)
        assert e.value.code == A.ERR_UNSUPPORTED, (hex(extra), str(e.value))
    with pytest.raises(A.TrplError) as e:                        # no snapshot / resume forms
        A.kernel_name(1000, 128, 100, A.FLAG_WEIGHTED, snapshots=True)
    assert e.value.code == A.ERR_UNSUPPORTED
    with pytest.raises(A.TrplError) as e:                        # the weighted sink already emits both sums
        A.kernel_name(1000, 128, 100, A.FLAG_WEIGHTED | A.FLAG_MOMENTS)
    assert e.value.code == A.ERR_ARG and "TRPL_FLAG_MOMENTS" in str(e.value)


def test_the_flag_on_any_other_entry_point_is_an_argument_error_before_a_device_is_touched(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.zeros(64)
    zi = np.zeros(8, dtype=np.int64)
    n1 = np.ones(1, dtype=np.int64)
    F = A.FLAG_WEIGHTED
    p = z.ctypes.data
    n = n1.ctypes.data
    calls = {
        "trpl_loglik": lambda: lib.trpl_loglik(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, 1, n, p, p, None, None, None, F, 0, None),
        "trpl_loglik_dev": lambda: lib.trpl_loglik_dev(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, 1, n, p, p, None, None, None, F, None),
        "trpl_loglik_obs": lambda: lib.trpl_loglik_obs(p, 1, 1, p, 1.0, 16, 10, 7, 100, p, p, p, p, p, 1, n, p, p, None, None, None, F, 0, None),
        "trpl_loglik_obs_dev": lambda: lib.trpl_loglik_obs_dev(p, 1, 1, p, 1.0, 16, 10, 7, 100, p, p, p, p, p, 1, n, p, p, None, None, None, F, None),
        "trpl_loglik_moments": lambda: lib.trpl_loglik_moments(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, None, None, None, 1, n, p, p, p, None, None, None, F, 0, None),
        "trpl_loglik_moments_dev": lambda: lib.trpl_loglik_moments_dev(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, None, None, None, 1, n, p, p, p, None, None, None, F, None),
        "trpl_solve_pl": lambda: lib.trpl_solve_pl(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, F, 0, None),
        "trpl_solve_pl_dev": lambda: lib.trpl_solve_pl_dev(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, F, None),
        "trpl_solve_pl_snap": lambda: lib.trpl_solve_pl_snap(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, p, p, 8, 11, None, None, zi.ctypes.data, 1, p, None, None, F, 0, None),
        "trpl_solve_pl_resume": lambda: lib.trpl_solve_pl_resume(p, 1, 100.0, 1.0, 16, 10, 1, 7, 100, 4, p, p, p, p, 8, 11, None, None, None, 0, None, None, None, F, 0, None),
        "trpl_loglik_from_pl_dev": lambda: lib.trpl_loglik_from_pl_dev(p, 8, 1, 11, 11, p, None, None, None, 5, p, None, p, None, F, None),
        "trpl_loglik_moments_from_pl_dev": lambda: lib.trpl_loglik_moments_from_pl_dev(p, 8, 1, 11, 11, p, None, None, None, 5, p, None, p, None, p, F, None),
        "trpl_loglik_multi": lambda: lib.trpl_loglik_multi(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, None, None, None, 1, n, p, None, None, None, None, F, None, 0, None),
    }
    for name, call in calls.items():
        assert call() == A.ERR_ARG, name
        assert b"TRPL_FLAG_WEIGHTED" in lib.trpl_last_error(), (name, lib.trpl_last_error())

    def weighted(X=p, S=1, L=16, wts=p, esum=p, flags=0, n_obs=n, obs_ld=1, C=1):
        return lib.trpl_loglik_weighted(X, S, C, p, 1.0, L, 10, 1, 7, 100, p, p, wts, None, None, None, obs_ld, n_obs, p, p,
                                        esum, None, None, None, flags, 0, None)

    # together with TRPL_FLAG_MOMENTS: the weighted sink already emits both sums
    assert weighted(flags=A.FLAG_MOMENTS) == A.ERR_ARG and b"TRPL_FLAG_MOMENTS" in lib.trpl_last_error()
    assert lib.trpl_loglik_weighted_dev(p, 1, 1, p, 1.0, 16, 10, 1, 7, 100, p, p, p, None, None, None, 1, n, p, p, p, None,
                                        None, None, A.FLAG_MOMENTS, None) == A.ERR_ARG
    assert b"TRPL_FLAG_MOMENTS" in lib.trpl_last_error()
    # the weighted entry points validate like their counterparts, without a device
    assert weighted(L=12) == A.ERR_ARG and b"power of two" in lib.trpl_last_error()
    assert weighted(esum=None) == A.ERR_ARG and b"esum" in lib.trpl_last_error()
    assert weighted(wts=None) == A.ERR_ARG and b"wts" in lib.trpl_last_error()
    assert lib.trpl_loglik_weighted(None, 0, 1, None, 1.0, 16, 10, 1, 7, 100, None, None, None, None, None, None, 1, None,
                                    None, None, None, None, None, None, 0, 0, None) == 0                     # S == 0
    assert lib.trpl_loglik_weighted_dev(None, 0, 1, None, 1.0, 16, 10, 1, 7, 100, None, None, None, None, None, None, 1, None,
                                        None, None, None, None, None, None, 0, None) == 0
    # a negative, NaN or infinite weight: TRPL_ERR_ARG naming curve and index, no device needed
    n3 = np.array([5, 3, 4], dtype=np.int64)
    for bad in (-1.0, float("nan"), float("inf"), -0.5):
        w = np.ones((3, 5))
        w[1, 2] = bad
        w[1, 4] = -7.0                                           # beyond n_obs[1] = 3: never read
        assert weighted(S=2, C=3, wts=w.ctypes.data, n_obs=n3.ctypes.data, obs_ld=5) == A.ERR_ARG, bad
        msg = lib.trpl_last_error()
        assert b"curve 1" in msg and b"index 2" in msg, msg
    w = np.ones(5)
    w[3] = float("nan")
    assert lib.trpl_sse_accumulate_w(p, p, 8, 2, 5, 5, p, w.ctypes.data, p, 0, None) == A.ERR_ARG
    assert b"index 3" in lib.trpl_last_error()
    assert lib.trpl_sse_accumulate_w(p, p, 8, 0, 5, 5, p, p, p, 0, None) == 0
    assert lib.trpl_sse_accumulate_w_dev(p, p, 3, 1, 5, 5, p, p, p, None) == A.ERR_ARG
    assert lib.trpl_loglik_weighted_from_pl_dev(p, 8, 1, 11, 11, p, None, None, None, None, 5, p, None, p, None, None, 0, None) == A.ERR_ARG
    assert b"wts" in lib.trpl_last_error()
    assert lib.trpl_loglik_weighted_from_pl_dev(p, 8, 0, 11, 11, p, p, None, None, None, 5, p, None, p, None, None, 0, None) == 0
    one = np.ones(1)
    assert lib.trpl_mag_grid_w_dev(p, p, one.ctypes.data, 4, A.MAG_MAX_CURVES + 1, p, 1, p, None) == A.ERR_ARG
    assert lib.trpl_mag_profile_w_dev(p, p, one.ctypes.data, 4, 1, 0x2, p, p, None) == A.ERR_ARG
    neg = np.array([-1.0])
    assert lib.trpl_mag_grid_w(p, p, neg.ctypes.data, 4, 1, p, 1, p) == A.ERR_ARG and b"wsum" in lib.trpl_last_error()


def test_weighted_instantiations_keep_their_moments_counterparts_resources():
    """The condition of the feature, checked on the cross-compiled objects (tools/kernel_resources.py; no GPU): every FAST
    weighted instantiation has 0 bytes of scratch and its moments counterpart's occupancy -- 2 waves for the four paired
    kernels; one-system kernels 3 waves up to L = 128, 2 at L = 256, 1 at L = 512.  STRICT at L >= 128 already spills in the
    moments form: no gate there (figures in DESIGN.md section 11)."""
    import sys
    units = ("weighted_fast", "weighted_predict_fast", "weighted_pair", "weighted_predict_pair")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")] + list(units),
                         capture_output=True, text=True, check=True).stdout
    rows = [ln for ln in out.splitlines() if ln.strip()]
    assert len(rows) == 2 * 8 + 2 * 2, out
    seen = set()
    for ln in rows:
        unit = ln.split()[0]
        scratch, occ = int(re.search(r"scratch +(\d+)", ln).group(1)), int(re.search(r"occ (\d+)", ln).group(1))
        assert "trpl::weighted::" in ln, ln
        assert scratch == 0, ln
        if unit.endswith("pair"):
            assert occ == 2, ln
            seen.add((unit, re.search(r"stepper_pair_kernel<([^>]*)>", ln).group(1)))
        else:
            L = int(re.search(r"stepper_kernel<(\d+),", ln).group(1))
            assert occ == (3 if L <= 128 else 2 if L == 256 else 1), ln
            seen.add((unit, L))
    assert len(seen) == len(rows)
