"""trpl_mcmc_propose*, trpl_mcmc_accept*, trpl_mcmc_chain_stats* (include/trpl.h): header, binding and library agree; the kernels
are in the library and their unit is compiled without contraction; every refusal the header states is TRPL_ERR_ARG with a message
naming the argument, decided with no device present; the Python layer's own refusals.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_mcmc_propose", "trpl_mcmc_propose_dev", "trpl_mcmc_accept", "trpl_mcmc_accept_dev", "trpl_mcmc_chain_stats",
       "trpl_mcmc_chain_stats_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]), name
    assert H.defines()["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version() == A.ABI_VERSION          # additive: the version stays
    for fn in ("propose", "accept", "chain_stats", "start", "run", "Chains"):
        assert callable(getattr(trpl.mcmc, fn)), fn
    for fn in ("mcmc_propose_device", "mcmc_accept_device", "mcmc_chain_stats_device"):
        assert callable(getattr(trpl.device, fn)), fn


def test_the_library_exports_the_symbols_and_holds_the_kernels(trpl):
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    filt = H.demangled()
    for kernel in ("propose_kernel", "accept_kernel"):
        have = {int(n) for n in re.findall(r"trpl::mcmc::__device_stub__%s<(\d+)>" % kernel, filt)}
        assert have == set(range(1, 17)), (kernel, sorted(have))
    assert "trpl::mcmc::__device_stub__chain_stats_kernel" in filt
    mk = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "Makefile")).read()
    rule = re.search(r"\$\(OBJ\)/mcmc\.o:([^\n]*)\n\t([^\n]*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(2) and "refine_common.hpp" in rule.group(1)
    assert "$(OBJ)/mcmc.o" in mk.split("$(LIB):")[1]


def _args():
    z = np.zeros(1024)
    p = z.ctypes.data
    scale = np.array([0.1, 0.0, 0.3])                            # a scale of 0 is allowed
    lo, hi = np.zeros(4), np.array([1.0, 0.0, 3.0, 5.0])         # three active columns, one fixed
    lg = np.zeros(4, dtype=np.int32)
    keep = (z, scale, lo, hi, lg)
    base = dict(U=p, partners=p, count=8, P=4, A=3, gamma=0.7, scale=scale.ctypes.data, chain0=0, seed=7, step=2, ncol=4,
                lo=lo.ctypes.data, hi=hi.ctypes.data, do_log=lg.ctypes.data, flags=0, Up=p, Xp=p, inside=p, X=p, LL=p, LLp=p, tf=1.0,
                accepted=p, H=p, n=8, ldh=5, Q=4, t0=1, t1=7, mean=p, m2=p)
    return keep, base


def _call(lib, form, a):
    if form.startswith("propose"):
        args = [a["U"], a["partners"], a["count"], a["P"], a["A"], a["gamma"], a["scale"], a["chain0"], a["seed"], a["step"], a["ncol"],
                a["lo"], a["hi"], a["do_log"], a["flags"], a["Up"], a["Xp"], a["inside"]]
        return lib.trpl_mcmc_propose_dev(*(args + [None])) if form.endswith("_dev") else lib.trpl_mcmc_propose(*(args + [0, None]))
    if form.startswith("accept"):
        args = [a["U"], a["X"], a["LL"], a["Up"], a["Xp"], a["LLp"], a["inside"], a["count"], a["A"], a["ncol"], a["tf"], a["chain0"],
                a["seed"], a["step"], a["accepted"]]
        return lib.trpl_mcmc_accept_dev(*(args + [None])) if form.endswith("_dev") else lib.trpl_mcmc_accept(*(args + [0, None]))
    args = [a["H"], a["n"], a["ldh"], a["Q"], a["t0"], a["t1"], a["mean"], a["m2"]]
    return lib.trpl_mcmc_chain_stats_dev(*(args + [None])) if form.endswith("_dev") else lib.trpl_mcmc_chain_stats(*(args + [0, None]))


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

    prop, acc, st = ("propose", "propose_dev"), ("accept", "accept_dev"), ("stats", "stats_dev")
    for arg in ("U", "scale", "Up", "Xp", "inside", "lo", "hi", "do_log"):
        refused(arg.encode() + b" is NULL", prop, **{arg: None})
    for arg in ("U", "X", "LL", "Up", "Xp", "LLp", "inside", "accepted"):
        refused(arg.encode() + b" is NULL", acc, **{arg: None})
    for arg in ("H", "mean", "m2"):
        refused(arg.encode() + b" is NULL", st, **{arg: None})
    for count in (0, -1, -(1 << 40)):
        refused(b"count=%d" % count, prop + acc, count=count)
    refused(b"blocks", prop + acc, count=(1 << 31) * 256)        # 2^31 blocks of 256 chains
    for n in (0, -1, 17, 1000):
        refused(b"A=%d" % n, prop + acc, A=n)
    refused(b"A=2, but the box has 3 active", prop, A=2)
    for P in (1, -1, -(1 << 40)):
        refused(b"P=%d" % P, prop, P=P)
    refused(b"partners is NULL", prop, partners=None)
    for bad in (np.nan, np.inf, -np.inf):
        refused(b"gamma=", prop, gamma=bad)
        refused(b"scale[1]=", prop, scale=np.array([0.1, bad, 0.3]).ctypes.data)
        refused(b"tf=", acc, tf=bad)
    refused(b"scale[2]=", prop, scale=np.array([0.1, 0.2, -1e-300]).ctypes.data)
    for tf in (0.0, -0.0, -2.0):
        refused(b"tf=", acc, tf=tf)
    for c0 in (-1, -(1 << 40)):
        refused(b"chain0=%d" % c0, prop + acc, chain0=c0)
    for ncol in (0, -1, 17):
        refused(b"ncol=%d" % ncol, prop + acc, ncol=ncol)
    # the box refusals of the refinement draw
    refused(b"flags=0x8", prop, flags=8)
    refused(b"column 2: lo must be <= hi", prop, hi=np.array([1.0, 0.0, -3.0, 5.0]).ctypes.data)
    refused(b"column 0: log-uniform needs lo > 0", prop, do_log=np.array([1, 0, 0, 0], dtype=np.int32).ctypes.data)
    # the history and its range
    for n in (0, -1):
        refused(b"n=%d" % n, st, n=n)
    for Q in (0, -1):
        refused(b"Q=%d" % Q, st, Q=Q)
    refused(b"ldh=3", st, ldh=3)
    for t0, t1 in ((-1, 7), (3, 3), (5, 4), (1, 9), (8, 9)):
        refused(b"t0=%d, t1=%d" % (t0, t1), st, t0=t0, t1=t1)
    # no refusal: these go as far as the device
    for form, kw in (("propose", {}), ("propose", dict(P=0, partners=None)), ("propose", dict(gamma=0.0, chain0=(1 << 32) + 5)),
                     ("accept", {}), ("accept", dict(tf=37.5, ncol=16)), ("stats", {}), ("stats", dict(t0=0, t1=8, Q=5)),
                     ("stats", dict(t0=7, t1=8))):
        assert _call(lib, form, dict(base, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (form, kw, lib.trpl_last_error())
    del keep


def test_python_refusals(trpl):
    M = trpl.mcmc
    lo, hi, lg = np.zeros(3), np.ones(3), np.zeros(3, dtype=np.int32)

    def never(X):
        raise AssertionError("the likelihood was called")

    for C in (5, 7, 2, 3, 0):
        with pytest.raises(ValueError, match="even number of chains, at least 4"):
            M.run(never, np.full((C, 3), 0.5), np.zeros(C), lo, hi, lg, sweeps=2)
    with pytest.raises(ValueError, match="needs scale"):
        M.run(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, sweeps=2, kind="rw")
    with pytest.raises(ValueError, match="kind"):
        M.run(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, sweeps=2, kind="snooker")
    # 10 kept sweeps x 4 chains x ((3 + 3 + 1) * 8 + 1) bytes = 2280
    with pytest.raises(ValueError, match="needs 2280 bytes, more than max_history_bytes = 2279"):
        M.run(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, sweeps=10, max_history_bytes=2279)
    with pytest.raises(ValueError, match="needs 1140 bytes"):                    # burn and keep_every count: sweeps 2, 4, 6, 8, 10
        M.run(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, sweeps=11, burn=2, keep_every=2, max_history_bytes=1139)
    with pytest.raises(ValueError, match="U0 must be"):
        M.run(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, sweeps=2, U0=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="X0 must be"):
        M.run(never, np.full((4, 2), 0.5), np.zeros(4), lo, hi, lg, sweeps=2)
    ch = M.Chains(np.zeros((3, 4, 2)), np.zeros((3, 4, 5)), np.zeros((3, 4)), np.zeros((3, 4), dtype=bool))
    with pytest.raises(ValueError, match="split-R-hat"):
        ch.rhat()
    ch = M.Chains(np.zeros((8, 4, 2)), np.zeros((8, 4, 5)), np.zeros((8, 4)), np.zeros((8, 4), dtype=bool))
    with pytest.raises(ValueError, match="split-R-hat"):
        ch.rhat(burn=5)
    X, W = ch.samples(burn=2, thin=3)                            # sweeps 2 and 5 of the four chains
    assert X.shape == (8, 5) and W.shape == (8,) and np.all(W == 1.0)
    with pytest.raises(ValueError, match="in place"):
        M.accept(np.zeros((4, 2), dtype=np.float32), np.zeros((4, 3)), np.zeros(4), np.zeros((4, 2)), np.zeros((4, 3)), np.zeros(4),
                 np.ones(4), 1.0, 0, 1, 0)
    with pytest.raises(ValueError, match="partners must be"):
        M.propose(np.zeros((4, 3)), np.zeros((2, 2)), 0.5, 0.1, 0, 1, 0, lo, hi, lg)
