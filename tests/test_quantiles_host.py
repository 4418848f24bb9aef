"""The weighted quantiles without a device: the extended-precision reference (tests/quantiles_ref.py) is the reference's
credible_interval on tie-free inputs, every input family of the -m gpu tests stays within the ambiguity cap, header, binding
and library agree, and every refusal comes before a device is touched."""
import numpy as np
import pytest

import abi_header as H
import quantiles_ref as qr

SYMBOLS = ("trpl_quantiles_stage_rows", "trpl_weighted_quantiles_dev", "trpl_weighted_quantiles", "trpl_predictive_gather_dev")


def _shapes(trpl):
    return qr.shape_list(trpl._abi.Q_BLOCK, int(trpl._abi.lib().trpl_quantiles_stage_rows()))


def test_reference_is_credible_interval_on_tie_free_inputs():
    for seed, n in enumerate((200, 1000, 4097)):
        rng = np.random.default_rng(seed)
        X = rng.permutation(n) + rng.random(n) * 0.5                   # tie-free
        P = rng.random(n) + 1e-3
        P /= P.sum()
        ref = qr.reference(X[None, :], P, [0.025, 0.975], [qr.LAST_BELOW, qr.FIRST_ABOVE])
        assert not ref["ambiguous"].any()
        assert (ref["want"][0, 0], ref["want"][1, 0]) == qr.credible_interval_literal(X, P)
    # where the reference raises IndexError (no point below 2.5 %) LAST_BELOW is NaN
    X, P = np.array([1.0, 2.0, 3.0]), np.array([0.5, 0.25, 0.25])
    with pytest.raises(IndexError):
        qr.credible_interval_literal(X, P)
    ref = qr.reference(X[None, :], P, [0.025, 0.975], [qr.LAST_BELOW, qr.FIRST_ABOVE])
    assert np.isnan(ref["want"][0, 0]) and ref["want"][1, 0] == 3.0


def test_reference_edge_cases():
    FA, LB = qr.FIRST_ABOVE, qr.LAST_BELOW
    Y = np.array([[3.0, 1.0, 2.0, 2.0, np.nan], [5.0, 5.0, 5.0, 5.0, 0.0], [np.nan, 0.0, -0.0, np.inf, -np.inf], [-0.0, 0.0, 1.0, 1.0, 9.0]])
    W = np.array([0.25, 0.25, 0.25, 0.25, 0.0])                        # row 4 is unused: its keys are not looked at
    r = qr.reference(Y, W, [0.5, 0.5, 0.3, 0.8], [FA, LB, LB, FA])
    # column 0: keys 1, 2 (a tie group of weight 0.5), 3 with cumulative weights 0.25, 0.75, 1
    assert list(r["want"][:, 0]) == [2.0, 1.0, 1.0, 3.0]
    # a constant column: FIRST_ABOVE is the constant, LAST_BELOW has no key below
    assert r["want"][0, 1] == 5.0 and np.isnan(r["want"][1, 1]) and r["want"][3, 1] == 5.0
    assert np.isnan(r["want"][:, 2]).all()                             # a NaN in a used row
    assert r["want"][0, 3] == 1.0 and np.isnan(r["want"][1, 3])        # -0.0 and +0.0 are one point of weight 0.5 ...
    assert r["ambiguous"][0, 3] and r["ambiguous"][1, 3]               # ... whose cumulative weight IS q sw: either neighbour
    assert (r["below"][0, 3], r["above"][1, 3]) == (0.0, 0.0) and r["above"][0, 3] == 1.0 and np.isnan(r["below"][1, 3])
    assert not r["ambiguous"][2:, 3].any() and not qr.within_cap(r)
    inf = qr.reference(np.array([[np.inf, -np.inf, 0.0, 1.0]]), np.array([0.1, 0.2, 0.3, 0.4]), [0.1, 0.95], [FA, FA])
    assert inf["want"][0, 0] == -np.inf and inf["want"][1, 0] == np.inf
    none = qr.reference(Y, np.array([0.0, -1.0, np.nan, np.inf, -0.0]), [0.5], [FA])
    assert np.isnan(none["want"]).all() and not none["ambiguous"].any()
    assert list(qr.used_rows([1.0, 0.0, np.nan, np.inf, -1.0, 1e-300])) == [True, False, False, False, False, True]
    # mismatches() applies the rule: equality where unambiguous, either neighbour where ambiguous
    ok = qr.reference(Y[:1], W, [0.3, 0.8], [LB, FA])
    assert qr.mismatches(ok["want"], ok) == [] and qr.mismatches(ok["want"] + [[0.0], [1.0]], ok) == [(1, 0, 4.0, 3.0)]


def test_every_input_family_of_the_gpu_tests_meets_the_ambiguity_cap(trpl):
    seen = set()
    for n in _shapes(trpl):
        for args in qr.shape_cases(n):
            Y, W, q, rule, ref = qr.case(*args)
            assert qr.within_cap(ref), (args, ref["ambiguous"].mean())
            assert qr.used_rows(W).any() and Y.shape == (args[1], n + args[2])
            seen |= {("K", args[3]), ("w", args[4])}
    assert seen == {("K", k) for k in qr.REQUESTS} | {("w", w) for w in qr.WEIGHTS}
    for args in qr.family_cases(trpl._abi.Q_BLOCK):
        Y, W, q, rule, ref = qr.case(*args)
        assert qr.within_cap(ref), (args, ref["ambiguous"].mean())
        wk, kk = args[4], args[5]
        if kk == "nan_used":
            assert np.isnan(ref["want"][:, 0]).all() and np.isnan(ref["want"][:, -1]).all() and np.isfinite(ref["want"][:, 1]).any()
        elif kk == "constant":
            lb = np.array(rule) == qr.LAST_BELOW
            assert np.isnan(ref["want"][lb]).all() and np.array_equal(ref["want"][~lb], np.tile(np.arange(3) - 0.5, (int((~lb).sum()), 1)))
        elif kk == "nan_unused":
            assert np.isnan(Y[:, :W.size]).any() and not np.isnan(ref["want"][np.array(rule) == qr.FIRST_ABOVE]).any()
        if wk == "sparse":
            assert 0.8 < np.mean(W == 0.0) < 0.97
        if wk == "decades":
            assert np.log10(W[W > 0].max() / W[W > 0].min()) > 15
        if wk == "unused":
            assert np.isnan(W).any() and (W < 0).any() and np.isinf(W).any()
        if wk == "one_row" and kk != "nan_unused":
            assert qr.used_rows(W).sum() == 1


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    want = {"TRPL_Q_MAX": A.Q_MAX, "TRPL_Q_BLOCK": A.Q_BLOCK, "TRPL_Q_FIRST_ABOVE": A.Q_FIRST_ABOVE, "TRPL_Q_LAST_BELOW": A.Q_LAST_BELOW,
            "TRPL_Q_FORCE_STREAM": A.Q_FORCE_STREAM}
    assert {k: v for k, v in H.defines().items() if k.startswith("TRPL_Q_")} == want
    assert (qr.FIRST_ABOVE, qr.LAST_BELOW) == (A.Q_FIRST_ABOVE, A.Q_LAST_BELOW) and max(qr.REQUESTS) == A.Q_MAX
    assert A.Q_BLOCK % 64 == 0 and A.Q_FIRST_ABOVE != A.Q_LAST_BELOW and 0 not in (A.Q_FIRST_ABOVE, A.Q_LAST_BELOW)
    lib = A.lib()
    for name in SYMBOLS:
        assert name in A.SIGNATURES and hasattr(lib, name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]), name
    assert A.ABI_VERSION == 5 == lib.trpl_abi_version()                    # new symbols only
    # two workgroups of staged rows (a 64-bit key image and a weight each) fit the 160 KiB of LDS of a compute unit
    stage = lib.trpl_quantiles_stage_rows()
    assert stage > 2 * A.Q_BLOCK and 2 * 16 * stage <= 160 << 10
    assert trpl.posterior.quantiles and trpl.posterior.credible_intervals and trpl.predictive.band_quantiles
    assert "Quantiles do not merge" in trpl.predictive.merge.__doc__


def test_refusals_need_no_device(trpl):
    lib, A = trpl._abi.lib(), trpl._abi
    E = A.ERR_ARG
    Y, Wq, out = np.ones((3, 10)), np.ones(8), np.zeros((2, 3))
    q, rule = np.array([0.025, 0.975]), np.array([A.Q_LAST_BELOW, A.Q_FIRST_ABOVE], dtype=np.int32)
    base = dict(Y=Y.ctypes.data, ncols=3, n=8, ldy=10, Wq=Wq.ctypes.data, q=q.ctypes.data, rule=rule.ctypes.data, K=2, flags=0,
                out=out.ctypes.data)
    keep = []                                                          # the arrays behind the addresses below stay alive

    def f64(*v):
        keep.append(np.array(v, dtype=np.float64))
        return keep[-1].ctypes.data

    def i32(*v):
        keep.append(np.array(v, dtype=np.int32))
        return keep[-1].ctypes.data

    bad = [(dict(Y=None), b"Y is NULL"), (dict(Wq=None), b"Wq is NULL"), (dict(q=None), b"q is NULL"), (dict(rule=None), b"rule is NULL"),
           (dict(out=None), b"out is NULL"), (dict(ncols=0), b"ncols"), (dict(n=0), b"n="), (dict(ldy=7), b"ldy"), (dict(K=0), b"K="),
           (dict(K=9, q=f64(*[0.5] * 9), rule=i32(*[A.Q_FIRST_ABOVE] * 9)), b"K="),
           (dict(q=f64(0.5, 0.0)), b"q[1]"), (dict(q=f64(1.0, 0.5)), b"q[0]"),
           (dict(q=f64(0.5, np.nan)), b"q[1]"), (dict(q=f64(-0.1, 0.5)), b"q[0]"),
           (dict(rule=i32(A.Q_LAST_BELOW, 0)), b"rule[1]"),
           (dict(rule=i32(3, A.Q_LAST_BELOW)), b"rule[0]"),
           (dict(flags=2), b"flags"), (dict(flags=A.FLAG_NORMALIZE), b"flags")]
    for kw, word in bad:
        a = dict(base, **kw)
        args = (a["Y"], a["ncols"], a["n"], a["ldy"], a["Wq"], a["q"], a["rule"], a["K"], a["flags"], a["out"])
        assert lib.trpl_weighted_quantiles(*args, 0, None) == E and word in lib.trpl_last_error(), (kw, lib.trpl_last_error())
        assert lib.trpl_weighted_quantiles_dev(*args, None) == E and word in lib.trpl_last_error(), (kw, lib.trpl_last_error())
    assert not out.any()

    pl, W, store, wq = np.ones((4, 7)), np.ones(4), np.zeros((6, 9)), np.zeros(9)
    g = dict(pl=pl.ctypes.data, elem=8, rows=4, ncol=6, ld=7, W=W.ctypes.data, flags=0, Y=store.ctypes.data, ldy=9, row0=5, Wq=wq.ctypes.data)
    bad = [(dict(pl=None), b"plI"), (dict(W=None), b"W is NULL"), (dict(Y=None), b"Y is NULL"), (dict(Wq=None), b"Wq is NULL"),
           (dict(elem=2), b"elem_bytes"), (dict(elem=16), b"elem_bytes"), (dict(rows=0), b"rows"), (dict(ncol=0), b"ncol"),
           (dict(ld=5), b"ld="), (dict(row0=-1), b"row0"), (dict(row0=6), b"row0"), (dict(ldy=3, row0=0), b"row0"),
           (dict(flags=A.FLAG_STRICT), b"flags"), (dict(flags=A.FLAG_NORMALIZE | A.FLAG_PREDICT), b"flags")]
    for kw, word in bad:
        a = dict(g, **kw)
        rc = lib.trpl_predictive_gather_dev(a["pl"], a["elem"], a["rows"], a["ncol"], a["ld"], None, a["W"], None, a["flags"], a["Y"],
                                            a["ldy"], a["row0"], a["Wq"], None)
        assert rc == E and word in lib.trpl_last_error(), (kw, lib.trpl_last_error())
    assert not store.any() and not wq.any()
    # the Python layer refuses what it can see itself
    with pytest.raises(ValueError):
        trpl.posterior.quantiles(np.ones((2, 5)), np.ones(4), 0.5)
    with pytest.raises(trpl.TrplError) as e:
        trpl.posterior.quantiles(np.ones((2, 5)), np.ones(5), 1.5)
    assert e.value.code == E
    q, rule = trpl.device.quantile_requests([0.025, 0.5, 0.975])
    assert list(rule) == [A.Q_LAST_BELOW, A.Q_FIRST_ABOVE, A.Q_FIRST_ABOVE] and q.dtype == np.float64 and rule.dtype == np.int32


def test_the_store_limit_of_posterior_predictive_fires_before_any_device_call(trpl):
    """80 001 columns x 1000 weighted samples are 640 008 000 bytes: the refusal states them, and comes before a device is
    looked for (this test runs where there is none) and before anything is solved."""
    w = trpl.workloads
    L, T = 128, 80000
    ini, lens = w.power_scan(L)
    X = w.samples(1200)
    W = np.zeros(1200)
    W[:1000] = 1e-3
    sim = [list(lens), T * 0.025, L, T, 1]
    with pytest.raises(ValueError, match="640008000 bytes"):
        trpl.predictive.posterior_predictive(X, W, ini, sim, quantiles=(0.025, 0.5, 0.975), max_store_bytes=640008000 - 1)
    with pytest.raises(ValueError, match="640008000 bytes"):
        trpl.posterior_predictive(X, W, ini, sim, quantiles=(0.5,), max_store_bytes=1 << 20)
    for bad in ((), (0.0,), (0.5, 1.0), tuple([0.5] * 9)):
        with pytest.raises(ValueError, match="quantiles"):
            trpl.predictive.posterior_predictive(X, W, ini, sim, quantiles=bad)
