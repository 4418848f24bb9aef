"""trpl_posterior_weights_lr and trpl_posterior_tf_scan_lr on the device (include/trpl.h; csrc/posterior.hip, csrc/posterior_scan.hip): the posterior
weights and the temperature scan with a proposal log-ratio kept beside LL.

Bit contract (np.array_equal, NaN matching NaN, no tolerance): with lnr = +0.0 every shared output is that of posterior.weights /
posterior.tf_scan; with a general lnr row k of the scan is posterior.weights(LL, tfs[k], log_ratio=lnr) followed by
posterior.moments(V, W).  Against tests/tf_scan_lr_ref.py (numpy.longdouble) the tolerances are those of
tests/test_gpu_posterior_instances.py for the same quantities.  The ladder runs end to end against the reference's ladder."""
import os
import re

import numpy as np
import pytest

import highprec as hp
import refine_ref as rr
import tf_scan_lr_ref as lr

pytestmark = pytest.mark.gpu
LD = np.longdouble
TINY = np.finfo(np.float64).tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMMON = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "csrc", "posterior_common.hpp")).read()
K_THREADS, K_MAX_BLOCKS = (int(re.search(r"constexpr int %s = (\d+);" % n, _COMMON).group(1)) for n in ("kThreads", "kMaxBlocks"))
GRID = K_THREADS * K_MAX_BLOCKS                  # beyond it a thread adds more than one sample

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, GRID + 300]
TFS = np.geomspace(1e-3, 1e6, 64)                # as tests/test_gpu_tf_scan.py: from all-but-one weight underflowing to nearly equal
KS = (1, 4, 5, 64)                               # both sides of the tile of four temperatures
DS = (0, 1, 13, 16)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _inputs(S, general):
    """LL = -1e4 U with some -inf; V of 16 scaled and shifted columns.  general: lnr uniform in [-3, 30], NaN in LL and in lnr, one
    lnr = +inf (from S = 63 on: the small sizes keep every sample usable); otherwise lnr = +0.0."""
    rng = np.random.default_rng(2000 + S)
    V = np.ascontiguousarray(rng.normal(size=(16, S)) * 10.0 ** rng.integers(-3, 4, size=(16, 1)) + rng.normal(size=(16, 1)))
    LL = -1e4 * rng.random(S)
    if S >= 63:
        LL[rng.choice(S, max(1, S // 50), replace=False)] = -np.inf
    if not general:
        return LL, np.zeros(S), V
    lnr = rng.uniform(-3.0, 30.0, S)
    if S >= 63:
        LL[rng.choice(S, max(1, S // 40), replace=False)] = np.nan
        lnr[rng.choice(S, max(1, S // 40), replace=False)] = np.nan
        LL[7], lnr[7] = -50.0, np.inf
    return LL, lnr, V


@pytest.mark.parametrize("S", SIZES)
def test_a_zero_ratio_gives_the_bits_of_the_calls_without_one(gpu, S):
    P = gpu.posterior
    big = S > 100000
    LL, lnr, V = _inputs(S, False)
    assert not np.signbit(lnr).any()
    tfs = TFS[::8] if big else TFS
    for tf in (tfs[0], tfs[len(tfs) // 2], tfs[-1]):
        a, b = {}, {}
        assert _same(P.weights(LL, tf, info=a, log_ratio=lnr), P.weights(LL, tf, info=b)), (S, tf)
        assert (a["max"], a["raw_sum"]) == (b["max"], b["raw_sum"])
    for K in ((1, len(tfs)) if big else KS):
        for D in ((0, 13) if big else DS):
            got = P.tf_scan(LL, tfs[:K], V[:D] if D else None, log_ratio=lnr)
            old = P.tf_scan(LL, tfs[:K], V[:D] if D else None)
            assert got["stats"].shape == (K, 6) and _same(got["ess"], got["stats"][:, 5])
            assert _same(got["stats"][:, [0, 1, 3, 4]], old["stats"]), (S, K, D)
            assert all(_same(got[n], old[n]) for n in ("mean", "var", "Q")), (S, K, D)


@pytest.mark.parametrize("S", SIZES)
def test_scan_rows_are_the_bits_of_weights_lr_then_moments(gpu, S):
    P = gpu.posterior
    big = S > 100000
    LL, lnr, V = _inputs(S, True)
    tfs = TFS[::8] if big else TFS
    Ds = (0, 13) if big else DS
    usable = ~(np.isnan(LL) | np.isnan(lnr))
    ref = {D: dict(stats=np.zeros((len(tfs), 6)), mean=np.zeros((len(tfs), D)), var=np.zeros((len(tfs), D)), Q=np.zeros((len(tfs), D)))
           for D in Ds}
    for k, tf in enumerate(tfs):
        info = {}
        W = P.weights(LL, tf, info=info, log_ratio=lnr)
        assert np.array_equal(np.isnan(W), ~usable), (S, tf)                  # NaN exactly where LL or lnr is
        if S >= 63:
            assert W[7] == 0.0 and (W[np.isneginf(LL) & usable] == 0.0).all()   # lnr = +inf, LL = -inf: exactly 0
        assert abs(np.nansum(W.astype(LD)) - 1) <= 1e-13
        for D in Ds:
            s, c = P.moments(V[:max(D, 1)], W)
            ref[D]["stats"][k] = info["max"], info["raw_sum"], s[0], s[1], usable.sum(), s[0] * s[0] / s[1]
            if D:
                var = np.diag(c[:, :D]) / s[0]
                ref[D]["mean"][k], ref[D]["var"][k], ref[D]["Q"][k] = s[2:] / s[0], var, np.sqrt(s[1] * var)
    for K in ((1, len(tfs)) if big else KS):
        for D in Ds:
            sel = slice(0, K) if K != 5 else slice(len(tfs) - 5, len(tfs))    # five temperatures: an odd tile, the other end
            got = P.tf_scan(LL, tfs[sel], V[:D] if D else None, log_ratio=lnr)
            for name in ("stats", "mean", "var", "Q"):
                assert _same(got[name], ref[D][name][sel]), (S, K, D, name, np.argwhere(~(got[name] == ref[D][name][sel]))[:4].tolist())
            assert (got["stats"][:, 4] == usable.sum()).all()
            if S >= 63:
                assert np.isnan(got["ess"]).all() and np.isfinite(got["stats"][:, :2]).all()     # NaN weights: as posterior.moments


@pytest.mark.parametrize("S", [255, 257, GRID + 300])
def test_weights_lr_against_longdouble(gpu, S):
    """rtol 1e-13 on the finite weights (one spacing of the format added below the smallest normal double), exact 0 and NaN where
    the definition has them, the sum within 1e-13 of 1; sum W, sum W^2 and sum W v_d to rtol 1e-12 (tests/test_gpu_posterior_instances.py).
    The columns are highprec.columns()'s 0, 12 and 15, shifted by 1e3 of their deviations: every v_d has one sign, so sum |W v| =
    |sum W v| and the weights' 1e-13 each cannot grow by cancellation -- with the fp64 summation (S / 2^18 + 9 additions deep per
    partial, 1e-15) that is well inside 1e-12."""
    P = gpu.posterior
    Vall, _, _ = hp.columns()
    V = np.ascontiguousarray(Vall[[0, 12, 15], :S])
    rng = np.random.default_rng(31 + S)
    LL = hp.loglik(S, seed=23)
    lnr = rng.uniform(-3.0, 30.0, S)
    LL[3], lnr[9] = -np.inf, np.inf
    worst = 0.0
    for tf in (TFS[::9] if S > 100000 else TFS[::3]):
        W = P.weights(LL, tf, log_ratio=lnr)
        want = lr.weights(LL, lnr, tf)
        assert W[3] == 0.0 and W[9] == 0.0 and not np.isnan(W).any()
        pos = want > 0
        err = np.abs(W[pos].astype(LD) - want[pos])
        allow = 1e-13 * want[pos] + np.where(want[pos] < TINY, 2.0 ** -1074, 0.0)
        nrm = want[pos] >= TINY
        worst = max(worst, float(np.max(err[nrm] / want[pos][nrm])))
        assert (err <= allow).all(), (S, tf, float(np.max(err / allow)))
        assert (W[~pos] == 0).all() and abs(W.astype(LD).sum() - 1) <= 1e-13, (S, tf)
        got = P.tf_scan(LL, [tf], V, log_ratio=lnr)
        sw, sw2, swv = want.sum(), (want * want).sum(), (V.astype(LD) * want).sum(axis=1)
        for name, g, w in (("sum W", got["stats"][0, 2], sw), ("sum W^2", got["stats"][0, 3], sw2)):
            assert abs(LD(g) - w) <= 1e-12 * abs(w), (S, tf, name, g, w)
        g = (got["mean"][0].astype(LD) * LD(got["stats"][0, 2]))              # sums[2 + d] to one rounding of the quotient and product
        assert (np.abs(g - swv) <= 1e-12 * np.abs(swv)).all(), (S, tf, "sum W v", g, swv)
        assert abs(LD(got["ess"][0]) - sw * sw / sw2) <= 3e-12 * (sw * sw / sw2), (S, tf)      # the two sums' 1e-12 each, one doubled
    print("S=%d: largest relative error of a normal weight %.3e" % (S, worst))


def test_the_leader_changes_with_the_temperature(gpu):
    """A max phase shared across the temperatures (max(LL) / tf, as the scan without a ratio may use) fails exactly here."""
    P = gpu.posterior
    LL, lnr, tfs = np.array([0.0, -10.0]), np.array([20.0, 0.0]), np.array([1.0, 0.1])
    got = P.tf_scan(LL, tfs, log_ratio=lnr)
    assert np.array_equal(got["stats"][:, 0], [-10.0, -20.0]) and np.array_equal(got["stats"][:, 4], [2.0, 2.0])
    W1, W2 = P.weights(LL, 1.0, log_ratio=lnr), P.weights(LL, 0.1, log_ratio=lnr)
    # the largest weight sits on sample 1, then on sample 0: exp(-10) beside 1, then exp(-80) beside 1
    assert np.allclose(W1, np.array([np.exp(-10.0), 1.0]) / (1.0 + np.exp(-10.0)), rtol=1e-13, atol=0) and W1[1] > 0.9999
    assert W2[0] == 1.0 and abs(W2[1] / np.exp(-80.0) - 1) < 1e-13
    want = lr.scan(LL, lnr, tfs)
    assert np.allclose(got["stats"][:, 2:4], want["stats"][:, 2:4].astype(np.float64), rtol=1e-13, atol=0)
    # the raw sums: the leader's unnormalised weight is exp(1000 ln 2 - ln 2) at both temperatures
    assert np.allclose(got["stats"][:, 1], want["stats"][:, 1].astype(np.float64), rtol=1e-12, atol=0)
    # the same through one scan of four and of five temperatures (the tile's edge), the pair in the middle
    for pad in ([3.0], [3.0, 4.0, 5.0]):
        t = np.array(pad[:1] + [1.0, 0.1] + pad)
        assert np.array_equal(P.tf_scan(LL, t, log_ratio=lnr)["stats"][1:3], got["stats"])


def test_the_device_form_can_be_captured_in_a_hip_graph(gpu):
    """trpl_posterior_tf_scan_lr_dev allocates nothing and never synchronises: captured once on one stream, replayed on other
    likelihoods, ratios and temperatures in the same buffers, it gives the eager call's bits (and those are the host form's); so
    does the weights call next to it."""
    import torch
    dv = gpu.device
    dev = torch.device("cuda", 0)
    S, D, K = 3 * K_THREADS + 5, 13, 64
    (lla, ra, va), (llb, rb, vb) = _inputs(S, True), _inputs(S + 1, True)
    for ll, r in ((lla, ra), (llb, rb)):            # no NaN here (the sums stay finite and can be told apart); -inf and lnr = +inf stay
        ll[np.isnan(ll)] = -7.0
        r[np.isnan(r)] = 1.5
    data = {"a": (lla, ra, va, TFS), "b": (llb[:S].copy(), rb[:S].copy(), np.ascontiguousarray(vb[:, :S]), TFS[::-1].copy())}
    LL, R, W = (torch.empty(S, dtype=torch.float64, device=dev) for _ in range(3))
    V = torch.empty((D, S), dtype=torch.float64, device=dev)
    tfs = torch.empty(K, dtype=torch.float64, device=dev)
    out = {n: torch.zeros((K, 6 if n == "stats" else D), dtype=torch.float64, device=dev) for n in ("stats", "mean", "var", "Q")}
    out["wstats"] = torch.zeros(2, dtype=torch.float64, device=dev)
    ws, wsw = dv.posterior_tf_scan_lr_workspace(S, D, K), dv.posterior_workspace(1)

    def load(name):
        ll, r, v, t = data[name]
        LL.copy_(torch.from_numpy(ll)); R.copy_(torch.from_numpy(r)); V.copy_(torch.from_numpy(np.ascontiguousarray(v[:D])))
        tfs.copy_(torch.from_numpy(t))

    def step():
        dv.posterior_tf_scan_lr_device(LL, R, tfs, out["stats"], ws, V=V, mean=out["mean"], var=out["var"], Q=out["Q"])
        dv.posterior_weights_lr_device(LL, R, 37.0, W, wsw, stats=out["wstats"])

    eager = {}
    for name in data:
        load(name)
        step()
        torch.cuda.synchronize()
        eager[name] = {n: t.clone() for n, t in out.items()}
        eager[name]["W"] = W.clone()
        ll, r, v, t = data[name]
        host = gpu.posterior.tf_scan(ll, t, v[:D], log_ratio=r)
        assert all(_same(eager[name][n].cpu().numpy(), host[n]) for n in ("stats", "mean", "var", "Q")), name
        info = {}
        assert _same(eager[name]["W"].cpu().numpy(), gpu.posterior.weights(ll, 37.0, info=info, log_ratio=r))
        assert eager[name]["wstats"].cpu().tolist() == [info["max"], info["raw_sum"]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        load("a")
        step()                                      # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            step()
    for name in ("b", "a", "b"):
        load(name)
        for t in list(out.values()) + [W]:
            t.fill_(-1.0)
        torch.cuda.synchronize()
        for _ in range(2):                          # replayed twice: the same bits both times
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(out[n], eager[name][n]) or _same(out[n].cpu().numpy(), eager[name][n].cpu().numpy()) for n in out), name
            assert _same(W.cpu().numpy(), eager[name]["W"].cpu().numpy()), name
    qa, qb = eager["a"]["Q"].cpu().numpy(), eager["b"]["Q"].cpu().numpy()
    assert np.isfinite(qa).all() and np.isfinite(qb).all() and not _same(qa, qb)


# ---- find_best_tf with a ratio ----
def _search_inputs():
    """The two-sided toy of tests/test_gpu_tf_scan.py (xi uniform in [-1, 1], the likelihood peaking at |xi| = 0.8) as a refined set
    would hold it: the samples with xi > 0 were proposed four times as densely as the others (r = 1.6 against 0.4), which the ratio
    undoes.  A ratio that is not constant moves the maximum: without it the right-hand side would carry four times the weight."""
    rng = np.random.default_rng(0)
    xi = np.concatenate([rng.uniform(-1, 0, 819), rng.uniform(0, 1, 3277)])
    lnr = np.where(xi > 0, np.log(1.6), np.log(0.4))
    return xi, -2e4 * ((np.abs(xi) - 0.8) / 0.1) ** 2, lnr, 1.0


def test_find_best_tf_with_a_ratio_finds_the_dense_grids_maximum(gpu):
    """Q at the returned tf is at least the best Q of the longdouble reference on a dense grid, minus that grid's spacing effect: the
    search ends within 1e-6 of a maximiser of its bracket, the grid's best point is at most half a spacing (1.15e-3 in ln tf) from
    the true maximiser, and only rounding (1e-12) separates the device's Q from the reference's at equal tf -- so Q >= Q_grid (1 -
    1e-12) unless the search followed another local maximum, which the coarse grid over the whole bracket (161 points, verified on the
    CPU: Q rises to tf = 0.178, Q = 0.3085, and falls after it; without the ratio the maximum is at tf = 0.294) excludes."""
    xi, LL, lnr, u0 = _search_inputs()
    grid = np.geomspace(u0 * 1e-4, u0 * 1e4, 8001)
    qs = np.array([float(lr.scan(LL, lnr, [t], xi)["Q"][0, 0]) for t in grid[3000:3500]])        # tf in [0.1, 0.316]: around the coarse maximum
    coarse = np.array([float(lr.scan(LL, lnr, [t], xi)["Q"][0, 0]) for t in grid[::50]])
    best = int(np.argmax(qs))
    assert qs[best] >= coarse.max() and 0 < best < len(qs) - 1
    assert np.all(np.diff(qs[:best + 1]) > 0) and np.all(np.diff(qs[best:]) < 0)                  # one maximum
    info = {}
    tf, q = gpu.posterior.find_best_tf(xi, LL, u0, info=info, log_ratio=lnr)
    tf0, q0 = gpu.posterior.find_best_tf(xi, LL, u0)
    print("find_best_tf with the ratio: tf %.9g Q %.15g in %d scans; dense grid: tf %.9g Q %.15g; without the ratio: tf %.9g Q %.9g"
          % (tf, q, info["scans"], grid[3000 + best], qs[best], tf0, q0))
    assert not info["at_edge"] and info["hi"] / info["lo"] - 1 <= 1e-6 and info["scans"] == 5
    assert q >= qs[best] * (1 - 1e-12), (q, qs[best])
    assert abs(np.log(tf / grid[3000 + best])) <= np.log(grid[1] / grid[0])                       # the same maximum: within one spacing
    assert abs(float(lr.scan(LL, lnr, [tf], xi)["Q"][0, 0]) / q - 1) < 1e-12                      # the value is the objective's
    assert abs(tf / tf0 - 1) > 1e-3                                                               # the ratio matters here
    cols = {"a": xi, "b": xi ** 2}
    both = gpu.posterior.calc_max_uncertainty(cols, LL, 2000 * u0, log_ratio=lnr)
    assert both["a"] == (tf, q) and both["b"] == gpu.posterior.find_best_tf(cols["b"], LL, u0, log_ratio=lnr)


# ---- the ladder end to end ----
TOY_LO, TOY_HI, TOY_LG = np.array([2.0, 1e-3, -1.0]), np.array([5.0, 1e1, 1.0]), np.array([0, 1, 0])


def test_the_ladder_end_to_end_on_the_device(gpu):
    """DESIGN.md section 19's toy at deviation 0.02 (the first generation's effective sample size at tf = 1 is 2.84) through
    refine.run(target_ess=64) against the reference's ladder, to the rtol 1e-9 of section 19's own end-to-end toy (unit_coords' device
    log10 and the device's moments and weights are the unpinned steps).  Whether the ladder's final effective sample size beats the
    fixed-temperature run's is NOT gated: the reference alone does not satisfy it on seeds 0 .. 7 (2922 against 3507 on this seed;
    DESIGN.md section 21 has the eight)."""
    loglik_unit, _ = rr.gaussian_toy(lr.LADDER_SD, lr.LADDER_A)
    U1 = np.random.default_rng(0).random((lr.LADDER_S1, lr.LADDER_A))
    ref = lr.run_ladder(loglik_unit, U1, lr.LADDER_ROUNDS, lr.LADDER_K, lr.LADDER_M, lr.LADDER_NU, lr.LADDER_TARGET, seed=0)
    assert ref["ess_at_tf"][0] < 4.0 and ref["tfs"][0] > 5.0

    def loglik(X):
        return loglik_unit(rr.unit_coords(X, TOY_LO, TOY_HI, TOY_LG)[0])

    X1 = rr.from_unit(U1, TOY_LO, TOY_HI, TOY_LG)
    info = {}
    pop = gpu.refine.run(loglik, X1, loglik(X1), TOY_LO, TOY_HI, TOY_LG, rounds=lr.LADDER_ROUNDS, K=lr.LADDER_K, m=lr.LADDER_M,
                         n_uniform=lr.LADDER_NU, tf=1.0, seed=0, info=info, target_ess=lr.LADDER_TARGET)
    print("ladder: tfs %s vs %s; ess %s vs %s; ess at tf %s vs %s" % (info["tfs"], ref["tfs"], info["ess"], ref["ess"],
                                                                      info["ess_at_tf"], ref["ess_at_tf"]))
    assert np.allclose(info["tfs"], ref["tfs"], rtol=1e-9, atol=0)
    assert np.allclose(info["ess"], ref["ess"], rtol=1e-9, atol=0) and np.allclose(info["ess_at_tf"], ref["ess_at_tf"], rtol=1e-9, atol=0)
    assert all(a >= b for a, b in zip(info["tfs"], info["tfs"][1:])) and info["tfs"][-1] == 1.0
    X, LL, lnr = pop.log_ratio()
    assert LL.shape == ref["LL"].shape and np.allclose(lnr, ref["lnr"], rtol=1e-9, atol=1e-12)
    W = gpu.posterior.weights(LL, 1.0, log_ratio=lnr)
    assert abs(W.sum() - 1.0) < 1e-12
    # LLc stays valid at its own tf: the folded form gives the same weights to rounding, and Population's thin calls are the module's
    Wc = pop.weights(1.0)
    assert np.allclose(W, Wc, rtol=1e-10, atol=1e-300)
    sc = pop.tf_scan([1.0, 3.0])
    assert sc["stats"].shape == (2, 6) and abs(sc["ess"][0] / info["ess"][-1] - 1) < 1e-9
    one = {}
    tf, ess = pop.tf_for_ess(lr.LADDER_TARGET, lo=1.0, hi=1e4, info=one)
    assert (tf, one["at_edge"]) == (1.0, "lo") and ess == sc["ess"][0]
