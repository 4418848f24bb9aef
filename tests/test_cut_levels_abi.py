"""trpl_loglik_cut_levels[_dev] and trpl_mcmc_levels[_dev] (include/trpl.h: the early stop with a level per system, and the levels
of a Metropolis step): header, binding and library agree on the four symbols; the refusals carry the codes the header states, with
no device present; the ABI version stays 5 and the shared object still holds exactly the 20 trpl::cut:: steppers.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_loglik_cut_levels", "trpl_loglik_cut_levels_dev", "trpl_mcmc_levels", "trpl_mcmc_levels_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    hdr = open(os.path.join(ROOT, "include", "trpl.h")).read()          # with its comments: the sentences below
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        n_args = len(H.params(name))
        assert n_args == len(A.SIGNATURES[name]), (name, n_args)
    # the cut calls' arguments, a pointer where sse_cut is
    for dev in ("", "_dev"):
        lv, cut = A.SIGNATURES["trpl_loglik_cut_levels" + dev], A.SIGNATURES["trpl_loglik_cut" + dev]
        assert len(lv) == len(cut)
        diff = [k for k in range(len(cut)) if lv[k] is not cut[k]]
        assert diff == [17] and cut[17] is A.C.c_double and lv[17] is A.C.c_void_p
        proto = ", ".join(H.params("trpl_loglik_cut_levels" + dev))
        assert "const double *cut_level" in proto and "sse_cut" not in proto and "int32_t *cut_col" in proto
        assert proto.index("n_obs") < proto.index("cut_level") < proto.index("double *P")
    assert len(A.SIGNATURES["trpl_mcmc_levels"]) == 9 and len(A.SIGNATURES["trpl_mcmc_levels_dev"]) == 8
    assert H.defines()["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version()          # additive: the version stays
    assert not any("trpl_loglik_multi" in n and "level" in n for n in A.SIGNATURES)  # there is no multi form
    # the sentences the header owes its readers
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "Every output of a system is what trpl_loglik_cut returns for it at sse_cut = cut_level[c][s], bit for bit" in flat
    assert "there a NaN level never cuts, and a negative level cuts after the first batch" in flat
    assert "Subtraction and division by tf > 0 are monotone under round-to-nearest" in flat
    assert "the likelihood starts P from +0.0, so that LL = -sum sse" in flat
    for name in ("loglik_cut_levels_device", "mcmc_levels_device"):
        assert name in dir(trpl.device)
    assert "reject_levels" in dir(trpl.mcmc)


def test_the_library_still_holds_exactly_the_twenty_cut_steppers(trpl):
    filt = H.demangled()
    have = set(re.findall(r"(trpl::cut::(?:predict::)?(?:pair::)?stepper(?:_pair)?_kernel<[^>]*>)", filt))
    assert len(have) == 20, sorted(have)
    assert "trpl::mcmc::levels_kernel" in filt


def _levels(lib, p, n, lv, flags=0, L=16, S=1, C=1, dev=False, hi=None, dx=None, h=None, plT=1):
    if dev:
        return lib.trpl_loglik_cut_levels_dev(p, S, C, p, 1.0, L, 10, plT, 7, 100, p, p, hi, dx, h, 1, n, lv, p, p, None, None, None,
                                              None, flags, None)
    return lib.trpl_loglik_cut_levels(p, S, C, p, 1.0, L, 10, plT, 7, 100, p, p, hi, dx, h, 1, n, lv, p, p, None, None, None, None,
                                      flags, 0, None)


def test_loglik_refusals_carry_the_stated_codes_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.ones(256)                                                              # every array the calls below read fits
    p, n = z.ctypes.data, np.ones(4, dtype=np.int64).ctypes.data
    ok = np.zeros(64)
    lv = ok.ctypes.data
    # every flag refusal of trpl_loglik_cut (tests/test_cut_abi.py), in both forms
    unsupported = (A.FLAG_STRICT, A.FLAG_FP32, A.FLAG_MIXED, A.FLAG_HIST32, A.flag_bundle(2, 16), A.FLAG_STRICT | A.flag_bundle(3, 16))
    for dev in (False, True):
        for extra in unsupported:
            assert _levels(lib, p, n, lv, flags=extra, dev=dev) == A.ERR_UNSUPPORTED, (dev, hex(extra), lib.trpl_last_error())
            assert b"TRPL_FLAG_CUT" in lib.trpl_last_error()
        for extra, word in ((A.FLAG_MOMENTS, b"TRPL_FLAG_MOMENTS"), (A.FLAG_WEIGHTED, b"TRPL_FLAG_WEIGHTED")):
            assert _levels(lib, p, n, lv, flags=extra, dev=dev) == A.ERR_ARG, (dev, hex(extra))
            assert word in lib.trpl_last_error()
        assert _levels(lib, p, n, None, dev=dev) == A.ERR_ARG and b"cut_level" in lib.trpl_last_error()      # NULL cut_level
        assert _levels(lib, p, n, lv, L=12, dev=dev) == A.ERR_ARG and b"power of two" in lib.trpl_last_error()
        assert _levels(lib, p, n, lv, hi=p, dev=dev) == A.ERR_ARG and b"go together" in lib.trpl_last_error()
        assert _levels(lib, p, n, lv, hi=p, dx=p, h=p, plT=2, dev=dev) == A.ERR_ARG and b"plT = 1" in lib.trpl_last_error()
        assert _levels(lib, None, None, None, S=0, dev=dev) == 0                  # S == 0: nothing to do
    # the host form looks at every level before it touches a device; the message names the curve and the sample
    S, C = 5, 3
    for bad in (float("nan"), -1.0, -float("inf")):
        for c, s in ((0, 0), (1, 3), (2, 4)):
            arr = np.full((C, S), np.inf)
            arr[0, 1] = 0.0
            arr[c, s] = bad
            assert _levels(lib, p, n, arr.ctypes.data, S=S, C=C) == A.ERR_ARG, (bad, c, s)
            msg = lib.trpl_last_error()
            assert b"cut_level" in msg and b"c=%d]" % c in msg and b"s=%d]" % s in msg, msg
    for good in (0.0, 1.0, float("inf")):                                        # accepted levels get as far as the device
        arr = np.full((C, S), good)
        assert _levels(lib, p, n, arr.ctypes.data, S=S, C=C) in (A.ERR_NODEVICE, A.OK)
    # a bad level does not hide a refusal that needs no look at the data
    arr = np.full((C, S), -1.0)
    assert _levels(lib, p, n, arr.ctypes.data, S=S, C=C, flags=A.FLAG_STRICT) == A.ERR_UNSUPPORTED
    assert _levels(lib, p, n, arr.ctypes.data, S=S, C=0) == A.ERR_ARG and b"cut_level" not in lib.trpl_last_error()


def test_mcmc_levels_refusals(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.zeros(8)
    p = z.ctypes.data
    for dev in (False, True):
        def call(LL=p, count=4, tf=1.0, chain0=0, level=p):
            if dev:
                return lib.trpl_mcmc_levels_dev(LL, count, tf, chain0, 7, 0, level, None)
            return lib.trpl_mcmc_levels(LL, count, tf, chain0, 7, 0, level, 0, None)
        for kw, word in ((dict(count=0), b"count"), (dict(count=-3), b"count"), (dict(count=1 << 40), b"count"),
                         (dict(tf=0.0), b"tf"), (dict(tf=-1.0), b"tf"), (dict(tf=float("inf")), b"tf"), (dict(tf=float("nan")), b"tf"),
                         (dict(chain0=-1), b"chain0"), (dict(LL=None), b"LL is NULL"), (dict(level=None), b"level is NULL")):
            assert call(**kw) == A.ERR_ARG, (dev, kw)
            assert word in lib.trpl_last_error(), (kw, lib.trpl_last_error())
    assert lib.trpl_mcmc_levels(p, 4, 1.0, 0, 7, 0, p, 0, None) in (A.ERR_NODEVICE, A.OK)


def test_python_refusals(trpl):
    with pytest.raises(ValueError):
        trpl.mcmc.reject_levels(np.zeros((2, 2)), 1.0, 0, 1, 0)
    with pytest.raises(trpl._abi.TrplError) as e:
        trpl.mcmc.reject_levels(np.zeros(4), 0.0, 0, 1, 0)
    assert e.value.code == trpl._abi.ERR_ARG
