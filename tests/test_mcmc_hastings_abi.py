"""trpl_mcmc_propose_stretch*, trpl_mcmc_accept_h*, trpl_mcmc_levels_h*, trpl_mcmc_prior_term* (include/trpl.h, Metropolis-Hastings):
header, binding and library agree; the kernels are in the library for every A and their unit is compiled without contraction; every
refusal the header states is TRPL_ERR_ARG with a message naming the argument, decided with no device present; the Python refusals of
run and run_tempered with kind="stretch" and prior=.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_mcmc_propose_stretch", "trpl_mcmc_propose_stretch_dev", "trpl_mcmc_accept_h", "trpl_mcmc_accept_h_dev",
       "trpl_mcmc_levels_h", "trpl_mcmc_levels_h_dev", "trpl_mcmc_prior_term", "trpl_mcmc_prior_term_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]), name
    for form in ("", "_dev"):                                    # h beside the arguments of the *_rungs calls
        assert len(A.SIGNATURES["trpl_mcmc_accept_h" + form]) == len(A.SIGNATURES["trpl_mcmc_accept_rungs" + form]) + 1
        assert len(A.SIGNATURES["trpl_mcmc_levels_h" + form]) == len(A.SIGNATURES["trpl_mcmc_levels_rungs" + form]) + 1
    assert len(A.SIGNATURES["trpl_mcmc_propose_stretch"]) == 22 and len(A.SIGNATURES["trpl_mcmc_prior_term"]) == 10
    assert H.defines()["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version() == A.ABI_VERSION          # additive: the version stays
    for fn in ("propose_stretch", "accept_h", "reject_levels_h", "prior_term", "gaussian_prior"):
        assert callable(getattr(trpl.mcmc, fn)), fn
    for fn in ("mcmc_propose_stretch_device", "mcmc_accept_h_device", "mcmc_levels_h_device", "mcmc_prior_term_device"):
        assert callable(getattr(trpl.device, fn)), fn
    for fn in (trpl.mcmc.run, trpl.mcmc.run_tempered):
        sig = inspect.signature(fn).parameters
        assert sig["stretch_a"].default == 2.0 and sig["prior"].default is None and sig["kind"].default == "de"


def test_the_library_holds_the_kernels_and_their_unit_is_uncontracted(trpl):
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    filt = H.demangled()
    for kernel in ("stretch_kernel", "hastings_accept_kernel", "prior_term_kernel"):
        have = {int(n) for n in re.findall(r"trpl::mcmc::__device_stub__%s<(\d+)>" % kernel, filt)}
        assert have == set(range(1, 17)), (kernel, sorted(have))
    assert "trpl::mcmc::__device_stub__hastings_levels_kernel" in filt
    mk = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "Makefile")).read()
    rule = re.search(r"\$\(OBJ\)/mcmc_hastings\.o:([^\n]*)\n\t([^\n]*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(2) and "refine_common.hpp" in rule.group(1)
    assert "$(OBJ)/mcmc_hastings.o" in mk.split("$(LIB):")[1]
    rule = re.search(r"\$\(OBJ\)/mcmc\.o:([^\n]*)\n\t([^\n]*)", mk)              # hastings_accept_kernel and hastings_levels_kernel are its
    assert rule and "-ffp-contract=off" in rule.group(2) and "mcmc.hip" in rule.group(1)


def _args():
    z = np.zeros(4096)
    p = z.ctypes.data
    lo, hi = np.zeros(4), np.array([1.0, 0.0, 3.0, 5.0])         # three active columns, one fixed
    lg = np.zeros(4, dtype=np.int32)
    tf = np.array([1.0, 2.5, 2.5, 0.5])
    mean, sd = np.array([0.5, 0.0, -3.0]), np.array([0.1, np.inf, 2.0])
    keep = (z, lo, hi, lg, tf, mean, sd)
    base = dict(U=p, partners=p, count=8, P=8, group=2, K=4, A=3, a=2.0, chain0=0, seed=7, step=2, ncol=4, lo=lo.ctypes.data,
                hi=hi.ctypes.data, do_log=lg.ctypes.data, flags=0, Up=p, Xp=p, inside=p, z=p, lnq=p, X=p, LL=p, LLp=p, h=p, tf=tf.ctypes.data,
                accepted=p, level=p, mean=mean.ctypes.data, sd=sd.ctypes.data, h_in=p, h_out=p)
    return keep, base


def _call(lib, form, a):
    dev = form.endswith("_dev")
    tail = [None] if dev else [0, None]
    if form.startswith("stretch"):
        fn = lib.trpl_mcmc_propose_stretch_dev if dev else lib.trpl_mcmc_propose_stretch
        return fn(a["U"], a["partners"], a["count"], a["P"], a["group"], a["A"], a["a"], a["chain0"], a["seed"], a["step"], a["ncol"], a["lo"],
                  a["hi"], a["do_log"], a["flags"], a["Up"], a["Xp"], a["inside"], a["z"], a["lnq"], *tail)
    if form.startswith("accept"):
        fn = lib.trpl_mcmc_accept_h_dev if dev else lib.trpl_mcmc_accept_h
        return fn(a["U"], a["X"], a["LL"], a["Up"], a["Xp"], a["LLp"], a["inside"], a["h"], a["count"], a["A"], a["ncol"], a["K"], a["group"],
                  a["tf"], a["chain0"], a["seed"], a["step"], a["accepted"], *tail)
    if form.startswith("levels"):
        fn = lib.trpl_mcmc_levels_h_dev if dev else lib.trpl_mcmc_levels_h
        return fn(a["LL"], a["h"], a["count"], a["K"], a["group"], a["tf"], a["chain0"], a["seed"], a["step"], a["level"], *tail)
    fn = lib.trpl_mcmc_prior_term_dev if dev else lib.trpl_mcmc_prior_term
    return fn(a["U"], a["Up"], a["count"], a["A"], a["mean"], a["sd"], a["h_in"], a["h_out"], *tail)


def test_every_refusal_is_err_arg_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    keep, base = _args()

    def refused(word, forms, **kw):
        for form in forms:
            a = dict(base)
            a.update(kw)
            assert _call(lib, form, a) == A.ERR_ARG, (word, form, kw)
            assert word in lib.trpl_last_error(), (word, form, lib.trpl_last_error())

    st, acc, lev, pr = ("stretch", "stretch_dev"), ("accept", "accept_dev"), ("levels", "levels_dev"), ("prior", "prior_dev")
    ladder = acc + lev
    for arg in ("U", "partners", "Up", "Xp", "inside", "z", "lnq", "lo", "hi", "do_log"):
        refused(arg.encode() + b" is NULL", st, **{arg: None})
    for arg in ("U", "X", "LL", "Up", "Xp", "LLp", "inside", "h", "accepted", "tf"):
        refused(arg.encode() + b" is NULL", acc, **{arg: None})
    for arg in ("LL", "h", "level", "tf"):
        refused(arg.encode() + b" is NULL", lev, **{arg: None})
    for arg in ("U", "Up", "mean", "sd", "h_out"):
        refused(arg.encode() + b" is NULL", pr, **{arg: None})
    # the stretch's own
    for a in (np.nan, np.inf, -np.inf, 1.0, 0.5, 0.0, -2.0):
        refused(b"a=", st, a=a)
    for P in (0, -1, -(1 << 40)):
        refused(b"P=%d" % P, st, P=P, count=1)
    for group in (0, -1, -(1 << 40)):
        refused(b"group=%d" % group, st + ladder, group=group)
    for P, group in ((8, 3), (9, 2), (2, 4)):
        refused(b"P=%d" % P, st, P=P, group=group, count=2)
    refused(b"count=10 must be <= P=8", st, count=10)
    refused(b"TRPL_MCMC_FOLD", st, flags=A.MCMC_FOLD)
    refused(b"TRPL_MCMC_FOLD", st, flags=A.MCMC_FOLD | 1)
    refused(b"flags=0x8", st, flags=8)
    refused(b"A=2, but the box has 3 active", st, A=2)
    refused(b"column 2: lo must be <= hi", st, hi=np.array([1.0, 0.0, -3.0, 5.0]).ctypes.data)
    refused(b"column 0: log-uniform needs lo > 0", st, do_log=np.array([1, 0, 0, 0], dtype=np.int32).ctypes.data)
    # the prior's own
    for bad in (np.nan, 0.0, -0.0, -1.0, -np.inf):
        refused(b"sd[2]=", pr, sd=np.array([0.1, np.inf, bad]).ctypes.data)
    for bad in (np.nan, np.inf, -np.inf):
        refused(b"mean[1]=", pr, mean=np.array([0.5, bad, -3.0]).ctypes.data)
    # the refusals of the *_rungs counterparts
    for K in (0, -1, 65, 1 << 20):
        refused(b"K=%d" % K, ladder, K=K)
    refused(b"blocks", ladder, group=(1 << 31) * 256)
    for count in (7, 9, 4, 16):
        refused(b"count=%d must be K * group" % count, ladder, count=count)
    for count in (0, -1, -(1 << 40)):
        refused(b"count=%d" % count, st + pr, count=count)
    refused(b"blocks", st + pr, count=(1 << 31) * 256, P=(1 << 31) * 256)
    for bad in (np.nan, np.inf, -np.inf, 0.0, -0.0, -2.0):
        for k in range(4):
            tf = np.array([1.0, 2.5, 2.5, 0.5])
            tf[k] = bad
            refused(b"tf[%d]=" % k, ladder, tf=tf.ctypes.data)
    for n in (0, -1, 17, 1000):
        refused(b"A=%d" % n, st + acc + pr, A=n)
    for c0 in (-1, -(1 << 40)):
        refused(b"chain0=%d" % c0, st + ladder, chain0=c0)
    for ncol in (0, -1, 17):
        refused(b"ncol=%d" % ncol, st + acc, ncol=ncol)
    # no refusal: these go as far as the device
    one = np.array([3.0])
    for form, kw in (("stretch", {}), ("stretch", dict(group=8)), ("stretch", dict(group=1)), ("stretch", dict(count=3)),
                     ("stretch", dict(P=64, group=4, count=64, chain0=(1 << 32) + 5, a=1.0 + 2.0 ** -52)), ("accept", {}),
                     ("accept", dict(K=1, group=8, tf=one.ctypes.data)), ("levels", {}), ("levels", dict(K=8, group=1, tf=np.full(8, 2.0).ctypes.data)),
                     ("prior", {}), ("prior", dict(h_in=None)), ("prior", dict(sd=np.full(3, np.inf).ctypes.data))):
        for suffix in ("", "_dev"):
            assert _call(lib, form + suffix, dict(base, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (form, kw, lib.trpl_last_error())
    del keep, one


def test_python_refusals(trpl):
    M = trpl.mcmc
    lo, hi, lg = np.zeros(3), np.ones(3), np.zeros(3, dtype=np.int32)
    X0, LL0 = np.full((4, 3), 0.5), np.zeros(4)

    def never(X):
        raise AssertionError("the likelihood was called")

    def both(**kw):
        yield lambda: M.run(never, X0, LL0, lo, hi, lg, sweeps=2, **kw)
        yield lambda: M.run_tempered(never, X0, LL0, lo, hi, lg, [1.0, 2.0], sweeps=2, **kw)

    for kw in (dict(gamma=0.5), dict(scale=1e-3), dict(jump_every=10)):
        for call in both(kind="stretch", **kw):
            with pytest.raises(ValueError, match="gamma, scale or jump_every"):
                call()
    for call in both(kind="stretch", bounds="fold"):
        with pytest.raises(ValueError, match="bounds='reject'"):
            call()
    for a in (1.0, 0.5, np.nan, np.inf, -2.0):
        for call in both(kind="stretch", stretch_a=a):
            with pytest.raises(ValueError, match="stretch_a"):
                call()
    for call in both(kind="snooker"):
        with pytest.raises(ValueError, match="kind"):
            call()
    for prior in ((np.zeros(2), np.ones(2)), (np.zeros(3), np.ones((1, 3))), (np.zeros(4), np.ones(4))):
        for call in both(prior=prior):
            with pytest.raises(ValueError, match="prior must be"):
                call()
    for prior in ((np.zeros(3), np.array([1.0, 0.0, 1.0])), (np.zeros(3), np.array([1.0, -1.0, 1.0])), (np.zeros(3), np.array([1.0, np.nan, 1.0])),
                  (np.array([0.0, np.inf, 0.0]), np.ones(3)), (np.array([np.nan, 0.0, 0.0]), np.ones(3))):
        for call in both(prior=prior):
            with pytest.raises(ValueError, match="prior:"):
                call()
    with pytest.raises(ValueError, match="partners must be"):
        M.propose_stretch(np.zeros((4, 3)), np.zeros((2, 2)), None, 2.0, 0, 1, 0, lo, hi, lg)
    with pytest.raises(ValueError, match="h must be"):
        M.accept_h(np.zeros((4, 2)), np.zeros((4, 3)), np.zeros(4), np.zeros((4, 2)), np.zeros((4, 3)), np.zeros(4), np.ones(4), np.zeros(3),
                   1.0, 0, 1, 0)
    with pytest.raises(ValueError, match="h must be"):
        M.reject_levels_h(np.zeros(4), np.zeros(5), 1.0, 0, 1, 0)
    with pytest.raises(ValueError, match="mean and sd must be"):
        M.prior_term(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(2), np.ones(3))


def test_gaussian_prior_is_in_unit_coordinates_of_the_active_columns(trpl):
    M = trpl.mcmc
    lo, hi = np.array([2.0, 1e-3, 7.0, -1.0]), np.array([5.0, 1e1, 7.0, 1.0])       # linear, log (4 decades), fixed, linear
    lg = np.array([0, 1, 0, 0], dtype=np.int32)
    mean, sd = M.gaussian_prior([3.5, 1e-1, 7.0, 0.0], [0.6, 0.5, 1.0, np.inf], lo, hi, lg)
    assert mean.shape == sd.shape == (3,)
    assert np.allclose(mean, [0.5, 0.5, 0.5], rtol=1e-15, atol=0) and np.allclose(sd[:2], [0.2, 0.125], rtol=1e-15, atol=0)
    assert sd[2] == np.inf
    mean, sd = M.gaussian_prior([2.0, 1e1, 0.0, 1.0], np.inf, lo, hi, lg)            # all flat: whatever the centre is
    assert np.all(sd == np.inf) and np.all(np.isfinite(mean))
    for c, w in (([3.5, -1.0, 7.0, 0.0], 0.5), ([3.5, 1e-1, 7.0, 0.0], 0.0), ([3.5, 1e-1, 7.0, 0.0], [0.1, -1.0, 1.0, 1.0]),
                 ([np.nan, 1e-1, 7.0, 0.0], 0.5)):
        with pytest.raises(ValueError, match="column"):
            M.gaussian_prior(c, w, lo, hi, lg)
