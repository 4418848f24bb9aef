"""trpl_loglik_cut_budget[_dev] (include/trpl.h: the early stop on a sample's total, a budget carried across the curves): header,
binding and library agree on the two symbols; the new kernel is in the library and its unit is built uncontracted; the refusals
carry the codes the header states, with no device present; the ABI version stays 5 and the shared object still holds exactly the 20
trpl::cut:: steppers.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_loglik_cut_budget", "trpl_loglik_cut_budget_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    hdr = open(os.path.join(ROOT, "include", "trpl.h")).read()          # with its comments: the sentences below
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        n_args = len(H.params(name))
        assert n_args == len(A.SIGNATURES[name]), (name, n_args)
    # the arguments of trpl_loglik_cut_levels: budget where cut_level is, curves_per_launch after it, cut_level before P
    for dev in ("", "_dev"):
        bd, lv = A.SIGNATURES["trpl_loglik_cut_budget" + dev], A.SIGNATURES["trpl_loglik_cut_levels" + dev]
        assert len(bd) == len(lv) + 2
        assert bd[:18] == lv[:18] and bd[18] is A.C.c_int32 and bd[19] is A.C.c_void_p and bd[20:] == lv[18:]
        proto = ", ".join(H.params("trpl_loglik_cut_budget" + dev))
        names = [a.split()[-1].lstrip("*") for a in proto.split(",")]
        assert names[16:22] == ["n_obs", "budget", "curves_per_launch", "cut_level", "P", "sse"] and names[22] == "cut_col", names
        assert "const double *budget" in proto and "int32_t curves_per_launch" in proto and ", double *cut_level" in proto
        assert "sse_cut" not in proto
    assert H.defines()["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version()          # additive: the version stays
    assert not any("trpl_loglik_multi" in n and "budget" in n for n in A.SIGNATURES)  # there is no multi form
    # the sentences the header owes its readers: the rule, the proof, the refusals
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "the first l with fl(R + l) >= B is the level; if none verifies, +inf" in flat
    assert "Floating-point addition of non-negative terms is monotone" in flat
    assert "a sample with any cut_col >= 0 has a plain total >= budget[s]" in flat
    assert "curves_per_launch outside [1, TRPL_MAX_CURVES]" in flat
    assert "loglik_cut_budget_device" in dir(trpl.device)


def test_the_kernel_is_in_the_library_and_its_unit_is_built_uncontracted(trpl):
    filt = H.demangled()
    assert "trpl::budget::level_kernel" in filt
    have = set(re.findall(r"(trpl::cut::(?:predict::)?(?:pair::)?stepper(?:_pair)?_kernel<[^>]*>)", filt))
    assert len(have) == 20, sorted(have)                                              # no stepper was added
    mk = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "Makefile")).read()
    rule = re.search(r"^\$\(OBJ\)/cut_budget\.o:[^\n]*\n\t([^\n]*)\n", mk, flags=re.M)
    assert rule and "-ffp-contract=off" in rule.group(1) and "$(FASTFP)" not in rule.group(1)
    assert "$(OBJ)/cut_budget.o" in mk.split("$(LIB):")[1]
    src = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "csrc", "cut_budget.hip")).read()
    assert "namespace budget" in src and "namespace cut" not in src and src.count("__global__") == 1 and "atomic" not in src.lower().replace("no atomics", "")


def _budget(lib, p, n, bd, lv, g=1, flags=0, L=16, S=1, C=1, dev=False, hi=None, dx=None, h=None, plT=1):
    if dev:
        return lib.trpl_loglik_cut_budget_dev(p, S, C, p, 1.0, L, 10, plT, 7, 100, p, p, hi, dx, h, 1, n, bd, g, lv, p, p, None, None,
                                              None, None, flags, None)
    return lib.trpl_loglik_cut_budget(p, S, C, p, 1.0, L, 10, plT, 7, 100, p, p, hi, dx, h, 1, n, bd, g, lv, p, p, None, None, None,
                                      None, flags, 0, None)


def test_refusals_carry_the_stated_codes_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.ones(256)                                                              # every array the calls below read fits
    p, n = z.ctypes.data, np.ones(4, dtype=np.int64).ctypes.data
    bd, lv = np.zeros(64).ctypes.data, np.zeros(64).ctypes.data
    unsupported = (A.FLAG_STRICT, A.FLAG_FP32, A.FLAG_MIXED, A.FLAG_HIST32, A.flag_bundle(2, 16), A.FLAG_STRICT | A.flag_bundle(3, 16))
    for dev in (False, True):
        # every flag refusal of trpl_loglik_cut (tests/test_cut_abi.py)
        for extra in unsupported:
            assert _budget(lib, p, n, bd, lv, flags=extra, dev=dev) == A.ERR_UNSUPPORTED, (dev, hex(extra), lib.trpl_last_error())
            assert b"TRPL_FLAG_CUT" in lib.trpl_last_error()
        for extra, word in ((A.FLAG_MOMENTS, b"TRPL_FLAG_MOMENTS"), (A.FLAG_WEIGHTED, b"TRPL_FLAG_WEIGHTED")):
            assert _budget(lib, p, n, bd, lv, flags=extra, dev=dev) == A.ERR_ARG, (dev, hex(extra))
            assert word in lib.trpl_last_error()
        # the refusals of its own
        assert _budget(lib, p, n, None, lv, dev=dev) == A.ERR_ARG and b"budget" in lib.trpl_last_error()
        assert _budget(lib, p, n, bd, None, dev=dev) == A.ERR_ARG and b"cut_level" in lib.trpl_last_error()
        for g in (0, -1, 17, 1 << 20):
            assert _budget(lib, p, n, bd, lv, g=g, dev=dev) == A.ERR_ARG, (dev, g)
            assert b"curves_per_launch" in lib.trpl_last_error()
        assert _budget(lib, p, n, bd, lv, L=12, dev=dev) == A.ERR_ARG and b"power of two" in lib.trpl_last_error()
        assert _budget(lib, p, n, bd, lv, hi=p, dev=dev) == A.ERR_ARG and b"go together" in lib.trpl_last_error()
        assert _budget(lib, p, n, bd, lv, hi=p, dx=p, h=p, plT=2, dev=dev) == A.ERR_ARG and b"plT = 1" in lib.trpl_last_error()
        assert _budget(lib, None, None, None, None, S=0, dev=dev) == 0            # S == 0: nothing to do
        assert _budget(lib, None, None, None, None, S=0, g=0, dev=dev) == A.ERR_ARG
    # the host form looks at every budget before it touches a device; the message names the sample
    S, C = 5, 3
    out = np.zeros((C, S))
    for bad in (float("nan"), -1.0, -float("inf")):
        for s in (0, 3, 4):
            arr = np.full(S, np.inf)
            arr[1] = 0.0
            arr[s] = bad
            assert _budget(lib, p, n, arr.ctypes.data, out.ctypes.data, S=S, C=C) == A.ERR_ARG, (bad, s)
            msg = lib.trpl_last_error()
            assert b"budget[s=%d]" % s in msg, msg
    for good in (0.0, 1.0, float("inf")):                                        # accepted budgets get as far as the device
        arr = np.full(S, good)
        for g in (1, 2, 3, 16):
            assert _budget(lib, p, n, arr.ctypes.data, out.ctypes.data, S=S, C=C, g=g) in (A.ERR_NODEVICE, A.OK)
    # a bad budget does not hide a refusal that needs no look at the data
    arr = np.full(S, -1.0)
    assert _budget(lib, p, n, arr.ctypes.data, out.ctypes.data, S=S, C=C, flags=A.FLAG_STRICT) == A.ERR_UNSUPPORTED
    assert _budget(lib, p, n, arr.ctypes.data, out.ctypes.data, S=S, C=0) == A.ERR_ARG and b"budget" not in lib.trpl_last_error()


def _loglik_args():
    rng = np.random.default_rng(1)
    S, C, L, T = 4, 2, 16, 20
    return (rng.uniform(0.5, 2.0, (S, 13)), rng.uniform(1.0, 2.0, (C, L)), 2000.0, 1.0, L, T, [np.zeros(5), np.zeros(7)]), S, C


def test_loglik_refusals(trpl):
    args, S, C = _loglik_args()
    call = lambda **kw: trpl.driver.loglik(*args, **kw)
    ok = np.full(S, 3.0)
    for other in (dict(sse_cut=1.0), dict(cut_levels=ok)):
        with pytest.raises(ValueError, match="exclude each other"):
            call(cut_budget=ok, **other)
    # refused with what sse_cut and cut_levels are refused with
    for word, kw in (("mag_grid", dict(mag_grid=[0.0])), ("mag_profile", dict(mag_profile=True)),
                     ("weights", dict(weights=[np.ones(5), np.ones(7)])), ("devices", dict(devices=[0])), ("bundle", dict(bundle=2))):
        with pytest.raises(ValueError, match="cut_budget: not available with %s" % word):
            call(cut_budget=ok, **kw)
    for shape in ((S + 1,), (C, S), (1, S), ()):
        with pytest.raises(ValueError, match="shape"):
            call(cut_budget=np.ones(shape))
    for bad in (np.nan, -1.0, -np.inf):
        arr = ok.copy()
        arr[2] = bad
        with pytest.raises(ValueError, match=">= 0"):
            call(cut_budget=arr)
    for g in (0, 17, -2):
        with pytest.raises(ValueError, match="curves_per_launch"):
            call(cut_budget=ok, curves_per_launch=g)
    with pytest.raises(ValueError, match="curves_per_launch goes with cut_budget"):
        call(curves_per_launch=2)
    with pytest.raises(ValueError, match="curves_per_launch goes with cut_budget"):
        call(cut_levels=ok, curves_per_launch=2)


def test_run_and_run_tempered_refuse_any_other_early_reject(trpl):
    import inspect
    M = trpl.mcmc
    X0, LL0 = np.full((4, 2), 0.5), np.zeros(4)
    box = (np.zeros(2), np.ones(2), np.zeros(2, dtype=bool))

    def never(*a, **k):
        raise AssertionError("nothing may be solved")
    for bad in ("system", "Sample", 1, 0, None, 2.0, "True"):
        with pytest.raises(ValueError, match="early_reject"):
            M.run(never, X0, LL0, *box, sweeps=1, early_reject=bad)
        with pytest.raises(ValueError, match="early_reject"):
            M.run_tempered(never, X0, LL0, *box, [1.0, 2.0], sweeps=1, early_reject=bad)
    sig = inspect.signature(M.run)
    assert sig.parameters["early_reject"].default is False and list(sig.parameters)[-1] == "early_reject"
    assert inspect.signature(M.run_tempered).parameters["early_reject"].default is False
    lk = inspect.signature(trpl.driver.loglik).parameters
    assert lk["cut_budget"].default is None and lk["curves_per_launch"].default == 1


def test_simulate_refuses_a_budget_without_a_margin(trpl):
    sim_flags = {"log_pl": True, "self_normalize": False}
    gpu_info = {"sims_per_gpu": 4, "num_gpus": 1, "fused": True, "cut_budget": True}
    X = np.ones((4, 13))
    e_data = [([np.linspace(0.0, 1.0, 5)], [np.zeros(5)], [np.ones(5)])]
    args = (None, e_data, np.zeros((1, 4)), X, None, None, 1, [2000.0, 1.0, 16, 20, 1, None, 7, 100], np.ones((1, 16)), sim_flags)
    with pytest.raises(ValueError, match="cut_budget.*needs.*cut_margin"):
        trpl.driver.simulate(*args, gpu_info, 0, [0.0], [0.0], [0.0])
    with pytest.raises(ValueError, match="curves_per_launch.*goes with.*cut_budget"):
        trpl.driver.simulate(*args, {"sims_per_gpu": 4, "num_gpus": 1, "fused": True, "curves_per_launch": 2}, 0, [0.0], [0.0], [0.0])
    # the combination refusals of cut_margin apply
    with pytest.raises(ValueError, match="cut_margin.*does not combine with weighted"):
        trpl.driver.simulate(*args, dict(gpu_info, cut_margin=10.0, weighted=True), 0, [0.0], [0.0], [0.0])
    with pytest.raises(ValueError, match="cut_margin.*does not combine with mag_grid"):
        trpl.driver.simulate(*args, dict(gpu_info, cut_margin=10.0, mag_grid=[0.0]), 0, [0.0], [0.0], [0.0])
