"""The log-ratio front end without a device: the longdouble reference of tests/tf_scan_lr_ref.py against tests/highprec.py and its
own invariances; the grid rule of posterior.tf_for_ess on injected objectives; refine.run with and without the temperature ladder,
its device calls replaced by the numpy restatements of tests/refine_ref.py (the product has no CPU fallback: the stubs live here)."""
import numpy as np
import pytest

import highprec as hp
import refine_ref as rr
import tf_scan_lr_ref as lr

LD = np.longdouble


def _inputs(S, seed=0):
    rng = np.random.default_rng(seed)
    LL = -1e3 * rng.random(S)
    LL[rng.random(S) < 0.05] = -np.inf
    LL[0] = -3.0
    return LL, rng.uniform(-3.0, 30.0, S)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("tf", (1e-3, 1.0, 37.0, 1e6))
def test_the_reference_without_a_ratio_is_highprec_weights(tf):
    LL, _ = _inputs(777)
    LL[5] = np.nan
    for zero in (0.0, -0.0):
        a, b = lr.weights(LL, np.full(LL.size, zero), tf), hp.weights(LL, tf)
        assert a.dtype == LD and np.array_equal(a, b, equal_nan=True)
    assert np.isnan(a[5]) and abs(np.nansum(a) - 1) < 1e-17


def test_a_constant_added_to_the_ratio_leaves_the_weights():
    LL, lnr = _inputs(500, 1)
    for tf in (0.5, 20.0):
        W = lr.weights(LL, lnr, tf)
        for c in (-7.25, 0.5, 100.0):
            # the constant leaves with the maximum; what remains is the rounding of lnr + c in fp64 (1e-14 at |lnr + c| < 130)
            assert np.allclose((lr.weights(LL, lnr + c, tf)[W > 0] / W[W > 0]).astype(np.float64), 1.0, rtol=1e-13, atol=0)
            assert np.array_equal(lr.weights(LL, lnr + c, tf) == 0, W == 0)


def test_the_reference_follows_the_nan_and_infinity_rules_and_the_leader_changes():
    LL, lnr = np.array([0.0, -10.0, np.nan, -1.0, -2.0]), np.array([20.0, 0.0, 1.0, np.nan, np.inf])
    r = lr.scan(LL, lnr, [1.0, 0.1])
    assert np.array_equal(r["stats"][:, 0].astype(np.float64), [-10.0, -20.0]) and np.all(r["stats"][:, 4] == 3)
    W1, W2 = lr.weights(LL, lnr, 1.0), lr.weights(LL, lnr, 0.1)
    assert np.array_equal(np.isnan(W1), [False, False, True, True, False]) and W1[4] == 0 and W2[4] == 0
    assert W1[1] > 0.999 and W2[0] > 0.999                        # exp(-20) against 1, then exp(-100 + 20) against 1
    # the effective sample size is that of refine_ref.ess on the same weights
    LL, lnr = _inputs(300, 2)
    assert abs(lr.ess_at(LL, lnr, 3.0) / rr.ess(lr.weights64(LL, lnr, 3.0)) - 1) < 1e-14
    assert abs(float(lr.scan(LL, lnr, [3.0])["stats"][0, 5]) / lr.ess_at(LL, lnr, 3.0) - 1) < 1e-13


# ------------------------------------------------------------------ the grid rule of tf_for_ess
def _search(trpl, f, target, lo, hi, rtol=1e-6, k=64):
    calls = []

    def objective(tfs):
        calls.append(np.array(tfs))
        return f(np.asarray(tfs))

    tf, ess, info = trpl.posterior._ess_search(objective, target, lo, hi, k, rtol)
    want = lr.tf_for_ess(f, target, lo, hi, k, rtol)
    assert (tf, info["at_edge"], info["scans"]) == (want[0], want[2], want[3]) and info["scans"] == len(calls)
    assert ess == want[1] or (ess != ess and want[1] != want[1])
    for t in calls:                                               # every grid: k points, geometric, both ends, inside the outer bracket
        assert t.shape == (k,) and np.all(np.diff(t) > 0) and t[0] >= lo and t[-1] <= hi
        assert np.allclose(np.diff(np.log(t)), np.log(t[-1] / t[0]) / (k - 1), rtol=1e-6, atol=1e-12)
    assert calls[0][0] == lo and calls[0][-1] == hi
    return tf, ess, info


def test_tf_for_ess_on_a_monotone_objective(trpl):
    f = lambda t: 1.0 + 10.0 * np.log(t)                          # reaches 50 at exp(4.9)
    tf, ess, info = _search(trpl, f, 50.0, 1.0, 1e4)
    assert info["at_edge"] is None and info["lo"] < np.exp(4.9) <= info["hi"] == tf and info["hi"] / info["lo"] - 1 <= 1e-6
    assert ess == f(tf) >= 50.0 and info["scans"] == 4            # ceil(ln(ln(1e4) / ln(1 + 1e-6)) / ln 63)
    assert _search(trpl, f, 50.0, 1.0, 1e4, rtol=1e-2)[2]["scans"] == 2


def test_tf_for_ess_takes_the_smallest_of_two_crossings(trpl):
    # up through 30 at tf = 3, down again at tf = 12, up for good at tf = 400: the grid sees the first crossing (it is 12 points wide)
    f = lambda t: np.where(t < 12.0, 10.0 * t, np.where(t < 400.0, 5.0, 100.0))
    tf, ess, info = _search(trpl, f, 30.0, 1.0, 1e4)
    assert info["at_edge"] is None and abs(tf / 3.0 - 1) <= 1e-6 and tf >= 3.0 and ess >= 30.0
    # a crossing narrower than the grid's spacing is not seen: the rule is stated on the grid
    g = lambda t: np.where((t > 3.0) & (t < 3.01), 100.0, np.where(t < 400.0, 5.0, 100.0))
    tf, _, _ = _search(trpl, g, 30.0, 1.0, 1e4)
    assert abs(tf / 400.0 - 1) <= 1e-6


def test_tf_for_ess_at_the_edges(trpl):
    f = lambda t: 1.0 + np.log(t)
    tf, ess, info = _search(trpl, f, 1e3, 1.0, 1e4)
    assert (tf, info["at_edge"], info["scans"]) == (1e4, "hi", 1) and ess == f(1e4) < 1e3
    tf, ess, info = _search(trpl, f, 0.5, 1.0, 1e4)
    assert (tf, ess, info["at_edge"], info["scans"]) == (1.0, 1.0, "lo", 1)
    nan = lambda t: np.full(t.shape, np.nan)                      # a NaN never reaches a target
    assert _search(trpl, nan, 2.0, 1.0, 10.0)[2]["at_edge"] == "hi"
    for bad in (dict(lo=0.0), dict(lo=2.0, hi=2.0), dict(hi=np.inf), dict(k=3), dict(rtol=0.0), dict(target=0.0)):
        a = dict(target=5.0, lo=1.0, hi=10.0, k=64, rtol=1e-6)
        a.update(bad)
        with pytest.raises(ValueError):
            trpl.posterior._ess_search(f, a["target"], a["lo"], a["hi"], a["k"], a["rtol"])


# ------------------------------------------------------------------ refine.run on numpy stand-ins for the device calls
LO, HI, LG = np.array([2.0, 1e-3, -1.0]), np.array([5.0, 1e1, 1.0]), np.array([0, 1, 0])


@pytest.fixture
def host_refine(trpl, monkeypatch):
    """trpl.refine with every device call replaced by tests/refine_ref.py; returns the record of the posterior calls made."""
    R, P = trpl.refine, trpl.posterior
    calls = {"weights": [], "tf_scan": 0}

    def resample(W, K, offset=0.5, device=0):
        idx, _, st = rr.resample(W, K, offset)
        return idx, {"sum": st[0], "sum_sq": st[1], "ess": st[2], "seconds": 0.0}

    def draw(p, minX, maxX, do_log, sim_flags=None, device=0):
        U2 = rr.draw_unit(p.a, p.b, p.m, p.n_uniform, p.seed, p.generation)
        return rr.from_unit(U2, minX, maxX, do_log), U2

    def weights(LL, tf=1.0, device=0, info=None, **kw):
        calls["weights"].append(sorted(kw))
        lnr = kw.get("log_ratio")
        return lr.weights64(LL, np.zeros(len(LL)) if lnr is None else lnr, tf)

    def tf_scan(LL, tfs, V=None, device=0, log_ratio=None):
        calls["tf_scan"] += 1
        return {"ess": np.array([lr.ess_at(LL, log_ratio, t) for t in np.atleast_1d(tfs)])}

    monkeypatch.setattr(R, "unit_coords", lambda X, lo, hi, lg, sim_flags=None, device=0: rr.unit_coords(X, lo, hi, lg))
    monkeypatch.setattr(R, "resample", resample)
    monkeypatch.setattr(R, "bandwidth", lambda U, W, S1, device=0: rr.bandwidth(U, W, S1))
    monkeypatch.setattr(R, "draw", draw)
    monkeypatch.setattr(R, "density", lambda U, p, device=0, info=None: rr.density(U, p.a, p.b, p.inv_vol))
    monkeypatch.setattr(P, "weights", weights)
    monkeypatch.setattr(P, "tf_scan", tf_scan)
    return calls


def _toy(seed):
    loglik_unit, _ = rr.gaussian_toy(lr.LADDER_SD, lr.LADDER_A)
    U1 = np.random.default_rng(seed).random((1024, lr.LADDER_A))
    X1 = rr.from_unit(U1, LO, HI, LG)
    return loglik_unit, U1, X1, lambda X: loglik_unit(rr.unit_coords(X, LO, HI, LG)[0])


def test_run_without_a_target_takes_the_old_path(trpl, host_refine):
    loglik_unit, U1, X1, loglik = _toy(0)
    info = {}
    pop = trpl.refine.run(loglik, X1, loglik(X1), LO, HI, LG, rounds=2, K=32, m=8, n_uniform=64, seed=0, info=info)
    # the weights of LLc, never the log-ratio calls, no scan
    assert host_refine["weights"] == [[]] * 3 and host_refine["tf_scan"] == 0
    assert sorted(info) == ["ess", "nonzero"]
    ref = rr.run(loglik_unit, rr.unit_coords(X1, LO, HI, LG)[0], 2, 32, 8, 64, seed=0)
    assert np.allclose(info["ess"], ref["ess"], rtol=1e-9, atol=0)
    assert np.allclose(pop.corrected(1.0)[1], ref["LLc"], rtol=1e-12, atol=0)
    # log_ratio() is corrected()'s ratio, at any temperature
    X, LL, lnr = pop.log_ratio()
    for tf in (1.0, 7.0):
        Xc, LLc = pop.corrected(tf)
        assert np.array_equal(Xc, X) and np.array_equal(LLc, LL - tf * lnr)
    assert np.array_equal(LL, np.concatenate(pop.LL)) and lnr.shape == LL.shape


def test_run_with_a_target_is_the_reference_ladder(trpl, host_refine):
    loglik_unit, U1, X1, loglik = _toy(1)
    info = {}
    pop = trpl.refine.run(loglik, X1, loglik(X1), LO, HI, LG, rounds=2, K=32, m=8, n_uniform=64, seed=1, info=info, target_ess=16.0)
    ref = lr.run_ladder(loglik_unit, rr.unit_coords(X1, LO, HI, LG)[0], 2, 32, 8, 64, 16.0, seed=1)
    assert host_refine["weights"] == [["log_ratio"]] * 2 + [[]] and host_refine["tf_scan"] > 2
    assert len(info["tfs"]) == 2 and len(info["ess_at_tf"]) == 3 == len(info["ess"])
    assert np.allclose(info["tfs"], ref["tfs"], rtol=1e-9, atol=0) and np.allclose(info["ess"], ref["ess"], rtol=1e-9, atol=0)
    assert np.allclose(info["ess_at_tf"], ref["ess_at_tf"], rtol=1e-9, atol=0)
    assert info["tfs"][0] > 1.0 and all(t >= 1.0 for t in info["tfs"]) and info["ess"][0] >= 16.0 > info["ess_at_tf"][0]
    X, LL, lnr = pop.log_ratio()
    assert np.allclose(lnr, ref["lnr"], rtol=1e-12, atol=1e-15) and np.allclose(LL, ref["LL"], rtol=1e-9, atol=0)
    # tf_hi caps the ladder: the first generation cannot reach the target below it, the cap is used
    info2 = {}
    trpl.refine.run(loglik, X1, loglik(X1), LO, HI, LG, rounds=1, K=32, m=8, n_uniform=64, seed=1, info=info2, target_ess=16.0, tf_hi=2.0)
    assert info2["tfs"] == [2.0] and info2["ess"][0] < 16.0
