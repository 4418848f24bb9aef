"""trpl_mcmc_propose_rungs*, trpl_mcmc_accept_rungs*, trpl_mcmc_levels_rungs*, trpl_mcmc_swap* (include/trpl.h, parallel tempering):
header, binding and library agree; the kernels are in the library for every A; every refusal the header states is TRPL_ERR_ARG with
a message naming the argument, decided with no device present; the Python refusals of run_tempered.  No GPU needed."""
import re

import numpy as np
import pytest

import abi_header as H

NEW = ("trpl_mcmc_propose_rungs", "trpl_mcmc_propose_rungs_dev", "trpl_mcmc_accept_rungs", "trpl_mcmc_accept_rungs_dev",
       "trpl_mcmc_levels_rungs", "trpl_mcmc_levels_rungs_dev", "trpl_mcmc_swap", "trpl_mcmc_swap_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]), name
    # group beside trpl_mcmc_propose's arguments; K, group and the ladder where the scalar tf was
    for form in ("", "_dev"):
        assert len(A.SIGNATURES["trpl_mcmc_propose_rungs" + form]) == len(A.SIGNATURES["trpl_mcmc_propose" + form]) + 1
        assert len(A.SIGNATURES["trpl_mcmc_accept_rungs" + form]) == len(A.SIGNATURES["trpl_mcmc_accept" + form]) + 2
        assert len(A.SIGNATURES["trpl_mcmc_levels_rungs" + form]) == len(A.SIGNATURES["trpl_mcmc_levels" + form]) + 2
    assert len(A.SIGNATURES["trpl_mcmc_swap"]) == 15 and len(A.SIGNATURES["trpl_mcmc_swap_dev"]) == 14
    defs = H.defines()
    assert defs["TRPL_MCMC_MAX_RUNGS"] == A.MCMC_MAX_RUNGS == 64
    assert defs["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version() == A.ABI_VERSION          # additive: the version stays
    for fn in ("propose_rungs", "accept_rungs", "reject_levels_rungs", "swap", "geometric_ladder", "run_tempered", "Tempered"):
        assert callable(getattr(trpl.mcmc, fn)), fn
    for fn in ("mcmc_propose_rungs_device", "mcmc_accept_rungs_device", "mcmc_levels_rungs_device", "mcmc_swap_device"):
        assert callable(getattr(trpl.device, fn)), fn


def test_the_library_exports_the_symbols_and_holds_the_kernels(trpl):
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    filt = H.demangled()
    for kernel in ("propose_rungs_kernel", "propose_rungs_fold_kernel", "accept_rungs_kernel", "swap_kernel"):
        have = {int(n) for n in re.findall(r"trpl::mcmc::__device_stub__%s<(\d+)>" % kernel, filt)}
        assert have == set(range(1, 17)), (kernel, sorted(have))
    assert "trpl::mcmc::__device_stub__levels_rungs_kernel" in filt
    # the kernels the sampler had keep their names and instantiations
    for kernel in ("propose_kernel", "propose_fold_kernel", "accept_kernel"):
        have = {int(n) for n in re.findall(r"trpl::mcmc::__device_stub__%s<(\d+)>" % kernel, filt)}
        assert have == set(range(1, 17)), (kernel, sorted(have))


def _args():
    z = np.zeros(4096)
    p = z.ctypes.data
    scale = np.array([0.1, 0.0, 0.3])
    lo, hi = np.zeros(4), np.array([1.0, 0.0, 3.0, 5.0])         # three active columns, one fixed
    lg = np.zeros(4, dtype=np.int32)
    tf = np.array([1.0, 2.5, 2.5, 0.5])                          # unsorted, two equal
    keep = (z, scale, lo, hi, lg, tf)
    base = dict(U=p, partners=p, count=8, P=8, group=2, K=4, A=3, gamma=0.7, scale=scale.ctypes.data, chain0=0, seed=7, step=2, ncol=4,
                lo=lo.ctypes.data, hi=hi.ctypes.data, do_log=lg.ctypes.data, flags=0, Up=p, Xp=p, inside=p, X=p, LL=p, LLp=p,
                tf=tf.ctypes.data, accepted=p, level=p, parity=0, swapped=p)
    return keep, base


def _call(lib, form, a):
    dev = form.endswith("_dev")
    tail = [None] if dev else [0, None]
    if form.startswith("propose"):
        fn = lib.trpl_mcmc_propose_rungs_dev if dev else lib.trpl_mcmc_propose_rungs
        return fn(a["U"], a["partners"], a["count"], a["P"], a["group"], a["A"], a["gamma"], a["scale"], a["chain0"], a["seed"], a["step"],
                  a["ncol"], a["lo"], a["hi"], a["do_log"], a["flags"], a["Up"], a["Xp"], a["inside"], *tail)
    if form.startswith("accept"):
        fn = lib.trpl_mcmc_accept_rungs_dev if dev else lib.trpl_mcmc_accept_rungs
        return fn(a["U"], a["X"], a["LL"], a["Up"], a["Xp"], a["LLp"], a["inside"], a["count"], a["A"], a["ncol"], a["K"], a["group"],
                  a["tf"], a["chain0"], a["seed"], a["step"], a["accepted"], *tail)
    if form.startswith("levels"):
        fn = lib.trpl_mcmc_levels_rungs_dev if dev else lib.trpl_mcmc_levels_rungs
        return fn(a["LL"], a["count"], a["K"], a["group"], a["tf"], a["chain0"], a["seed"], a["step"], a["level"], *tail)
    fn = lib.trpl_mcmc_swap_dev if dev else lib.trpl_mcmc_swap
    return fn(a["U"], a["X"], a["LL"], a["K"], a["group"], a["A"], a["ncol"], a["tf"], a["parity"], a["chain0"], a["seed"], a["step"],
              a["swapped"], *tail)


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

    prop, acc, lev, sw = ("propose", "propose_dev"), ("accept", "accept_dev"), ("levels", "levels_dev"), ("swap", "swap_dev")
    ladder = acc + lev + sw
    for arg in ("U", "partners", "scale", "Up", "Xp", "inside", "lo", "hi", "do_log"):
        refused(arg.encode() + b" is NULL", prop, **{arg: None})
    for arg in ("U", "X", "LL", "Up", "Xp", "LLp", "inside", "accepted", "tf"):
        refused(arg.encode() + b" is NULL", acc, **{arg: None})
    for arg in ("LL", "level", "tf"):
        refused(arg.encode() + b" is NULL", lev, **{arg: None})
    for arg in ("U", "X", "LL", "swapped", "tf"):
        refused(arg.encode() + b" is NULL", sw, **{arg: None})
    for K in (0, -1, 65, 1 << 20):
        refused(b"K=%d" % K, ladder, K=K)
    for group in (0, -1, -(1 << 40)):
        refused(b"group=%d" % group, prop + ladder, group=group)
    refused(b"group=1", prop, group=1, P=8)                      # a rung of one chain has no two partners
    refused(b"blocks", ladder, group=(1 << 31) * 256)
    for count in (7, 9, 4, 16):
        refused(b"count=%d must be K * group" % count, acc + lev, count=count)
    for count in (0, -1):
        refused(b"count=%d" % count, prop, count=count)
    refused(b"count=10 must be <= P=8", prop, count=10)
    for P, group in ((8, 3), (9, 2), (2, 4), (0, 2)):
        refused(b"P=%d" % P, prop, P=P, group=group, count=2)
    for bad in (np.nan, np.inf, -np.inf, 0.0, -0.0, -2.0):
        for k in range(4):
            tf = np.array([1.0, 2.5, 2.5, 0.5])
            tf[k] = bad
            refused(b"tf[%d]=" % k, ladder, tf=tf.ctypes.data)
    refused(b"tf[0]=", ladder, K=1, group=8, tf=np.array([np.nan]).ctypes.data)
    for parity in (-1, 2, 7):
        refused(b"parity=%d" % parity, sw, parity=parity)
    # the checks of the calls they extend
    for n in (0, -1, 17, 1000):
        refused(b"A=%d" % n, prop + acc + sw, A=n)
    refused(b"A=2, but the box has 3 active", prop, A=2)
    for c0 in (-1, -(1 << 40)):
        refused(b"chain0=%d" % c0, prop + ladder, chain0=c0)
    for ncol in (0, -1, 17):
        refused(b"ncol=%d" % ncol, prop + acc + sw, ncol=ncol)
    for bad in (np.nan, np.inf):
        refused(b"gamma=", prop, gamma=bad)
        refused(b"scale[1]=", prop, scale=np.array([0.1, bad, 0.3]).ctypes.data)
    refused(b"flags=0x8", prop, flags=8)
    refused(b"column 2: lo must be <= hi", prop, hi=np.array([1.0, 0.0, -3.0, 5.0]).ctypes.data)
    # no refusal: these go as far as the device
    one = np.array([3.0])
    for form, kw in (("propose", {}), ("propose", dict(flags=A.MCMC_FOLD)), ("propose", dict(count=3)), ("propose", dict(group=8)),
                     ("propose", dict(P=64, group=4, count=64, chain0=(1 << 32) + 5)), ("accept", {}),
                     ("accept", dict(K=1, group=8, tf=one.ctypes.data)), ("accept", dict(K=8, group=1, tf=np.full(8, 2.0).ctypes.data)),
                     ("levels", {}), ("levels", dict(K=1, group=8, tf=one.ctypes.data)), ("swap", {}), ("swap", dict(parity=1)),
                     ("swap", dict(K=1, group=8, tf=one.ctypes.data)), ("swap", dict(K=1, group=1, tf=one.ctypes.data, parity=1)),
                     ("swap", dict(K=64, group=1, tf=np.linspace(1.0, 64.0, 64).ctypes.data, ncol=16))):
        for suffix in ("", "_dev"):
            assert _call(lib, form + suffix, dict(base, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (form, kw, lib.trpl_last_error())
    del keep, one


def test_python_refusals(trpl):
    M = trpl.mcmc
    lo, hi, lg = np.zeros(3), np.ones(3), np.zeros(3, dtype=np.int32)

    def never(X):
        raise AssertionError("the likelihood was called")

    for C in (5, 7, 2, 3):
        with pytest.raises(ValueError, match="even number of chains, at least 4"):
            M.run_tempered(never, np.full((C, 3), 0.5), np.zeros(C), lo, hi, lg, [1.0, 2.0], sweeps=2)
    for ladder in ([], [[1.0, 2.0]], 1.0, np.ones(65)):
        with pytest.raises(ValueError, match="ladder must be"):
            M.run_tempered(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, ladder, sweeps=2)
    for ladder in ([1.0, 0.0], [np.nan], [1.0, -2.0], [np.inf, 1.0]):
        with pytest.raises(ValueError, match="finite and > 0"):
            M.run_tempered(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, ladder, sweeps=2)
    with pytest.raises(ValueError, match="X0 must be"):                          # two rungs of states for a ladder of three
        M.run_tempered(never, np.full((2, 4, 3), 0.5), np.zeros((2, 4)), lo, hi, lg, [1.0, 2.0, 4.0], sweeps=2)
    with pytest.raises(ValueError, match="X0 must be"):
        M.run_tempered(never, np.full((3, 4, 3), 0.5), np.zeros(4), lo, hi, lg, [1.0, 2.0, 4.0], sweeps=2)
    with pytest.raises(ValueError, match="U0 must be"):
        M.run_tempered(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, [1.0, 2.0], sweeps=2, U0=np.zeros((3, 4, 3)))
    with pytest.raises(ValueError, match="swap_every"):
        M.run_tempered(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, [1.0, 2.0], sweeps=2, swap_every=0)
    with pytest.raises(ValueError, match="needs scale"):
        M.run_tempered(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, [1.0, 2.0], sweeps=2, kind="rw")
    with pytest.raises(ValueError, match="kind"):
        M.run_tempered(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, [1.0, 2.0], sweeps=2, kind="snooker")
    # 10 kept sweeps x 3 rungs x 4 chains x ((3 + 3 + 1) * 8 + 1) bytes = 6840
    with pytest.raises(ValueError, match="10 sweeps x 3 rungs x 4 chains needs 6840 bytes, more than max_history_bytes = 6839"):
        M.run_tempered(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, [1.0, 2.0, 4.0], sweeps=10, max_history_bytes=6839)
    with pytest.raises(ValueError, match="needs 3420 bytes"):                    # burn and keep_every count: sweeps 2, 4, 6, 8, 10
        M.run_tempered(never, np.full((4, 3), 0.5), np.zeros(4), lo, hi, lg, [1.0, 2.0, 4.0], sweeps=11, burn=2, keep_every=2,
                       max_history_bytes=3419)
    lad = M.geometric_ladder(1.0, 64.0, 7)
    assert lad.shape == (7,) and lad[0] == 1.0 and lad[-1] == 64.0 and np.allclose(lad[1:] / lad[:-1], 2.0, rtol=1e-14, atol=0)
    assert np.array_equal(M.geometric_ladder(37.5, 1e3, 1), [37.5])
    for bad in ((0.0, 2.0, 3), (1.0, np.inf, 3), (1.0, 2.0, 0), (1.0, 2.0, 65)):
        with pytest.raises(ValueError):
            M.geometric_ladder(*bad)
    with pytest.raises(ValueError, match="in place"):
        M.swap(np.zeros((4, 2), dtype=np.float32), np.zeros((4, 3)), np.zeros(4), [1.0, 2.0], 0, 0, 1, 0)
    with pytest.raises(ValueError, match="no multiple"):
        M.swap(np.zeros((5, 2)), np.zeros((5, 3)), np.zeros(5), [1.0, 2.0], 0, 0, 1, 0)
    t = M.Tempered(lad, [M.Chains(np.zeros((8, 4, 2)), np.full((8, 4, 5), float(k)), np.zeros((8, 4)), np.zeros((8, 4), dtype=bool))
                         for k in range(7)], np.zeros(6))
    X, W = t.samples(burn=2, thin=3)                             # rung 0: ladder[0] is the caller's temperature
    assert X.shape == (8, 5) and np.all(X == 0.0) and np.all(W == 1.0) and np.all(t.rung(3).X == 3.0)
