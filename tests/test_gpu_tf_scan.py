"""trpl_posterior_tf_scan on the device: row k of the scan carries the BITS of posterior.weights(LL, tfs[k]) followed by
posterior.moments(V, W) (include/trpl.h), at every sample count where the combination of the partial sums can go wrong; the
_dev form replays from a HIP graph; find_best_tf finds at least the maximum the reference's fmin finds; calc_max_uncertainty is
one find_best_tf per column.  Equality is exact (np.array_equal, NaN matching NaN): nothing here has a tolerance but the
comparison with fmin, whose bound the test states."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMMON = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "csrc", "posterior_common.hpp")).read()
K_THREADS, K_MAX_BLOCKS, K_MAX_DIM = (int(re.search(r"constexpr int %s = (\d+);" % n, _COMMON).group(1))
                                      for n in ("kThreads", "kMaxBlocks", "kMaxDim"))
GRID = K_THREADS * K_MAX_BLOCKS                  # samples of a full partial grid: beyond it a thread adds more than one sample

# one wave and its neighbours, an odd size, a block's share and its neighbours, more than a full grid
SIZES = [1, 63, 64, 65, 1000, K_THREADS - 1, K_THREADS, K_THREADS + 1, GRID + 300]
TFS = np.geomspace(1e-3, 1e6, 64)                # from all-but-one weight underflowing to all weights (nearly) equal
KS = (1, 2, 33, 64)
DS = (0, 1, 13, K_MAX_DIM)


def _inputs(S, variant):
    rng = np.random.default_rng(1000 + S)
    V = np.ascontiguousarray(rng.normal(size=(K_MAX_DIM, S)) * 10.0 ** rng.integers(-3, 4, size=(K_MAX_DIM, 1)) + rng.normal(size=(K_MAX_DIM, 1)))
    if variant == "equal":
        return np.full(S, -123.456), V
    LL = -1e4 * rng.random(S)
    if S >= 3:
        LL[rng.choice(S, max(1, S // 50), replace=False)] = -np.inf
        if variant == "nan":
            LL[rng.choice(S, max(1, S // 40), replace=False)] = np.nan
            LL[1] = np.nan
    return LL, V


def _reference(gpu, LL, V, tfs, Ds):
    """What the existing calls give at every temperature, once per (inputs)."""
    p = gpu.posterior
    ref = {D: dict(stats=np.zeros((len(tfs), 4)), mean=np.zeros((len(tfs), D)), var=np.zeros((len(tfs), D)),
                   Q=np.zeros((len(tfs), D))) for D in Ds}
    for k, tf in enumerate(tfs):
        info = {}
        W = p.weights(LL, tf, info=info)
        for D in Ds:
            s, c = p.moments(V[:max(D, 1)], W)
            ref[D]["stats"][k] = info["max"], info["raw_sum"], s[1], np.count_nonzero(~np.isnan(LL))
            if D:
                var = np.diag(c[:, :D]) / s[0]
                ref[D]["mean"][k], ref[D]["var"][k], ref[D]["Q"][k] = s[2:] / s[0], var, np.sqrt(s[1] * var)
    return ref


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("S", SIZES)
def test_scan_rows_are_the_bits_of_weights_then_moments(gpu, S):
    big = S > 100000
    for variant in ("inf", "nan", "equal"):
        LL, V = _inputs(S, variant)
        tfs = TFS[::8] if big else TFS             # the large sizes check the combination of partials, at 8 temperatures
        Ds = (0, 13) if big else DS
        ref = _reference(gpu, LL, V, tfs, Ds)
        if variant == "inf":
            assert np.isfinite(ref[Ds[-1]]["Q"]).all() and (S < 3 or np.isneginf(LL).any())
            if S == 1000:                          # both regimes are there: one sample holds the weight / all share it
                ws = ref[Ds[-1]]["stats"][:, 2]
                assert ws[0] == 1.0 and 1.0 / np.isfinite(LL).sum() <= ws[-1] < 1.001 / np.isfinite(LL).sum()
        if variant == "nan" and S >= 3:
            assert np.isnan(ref[Ds[-1]]["Q"]).all() and np.isfinite(ref[0]["stats"][:, :2]).all()
        for K in (KS if not big else (1, len(tfs))):
            for D in Ds:
                sel = slice(0, K) if K != 33 else slice(31, 64)             # 33 temperatures: an odd tile, another range
                got = gpu.posterior.tf_scan(LL, tfs[sel], V[:D] if D else None)
                for name in ("stats", "mean", "var", "Q"):
                    assert _same(got[name], ref[D][name][sel]), (S, variant, K, D, name,
                                                                  np.argwhere(~(got[name] == ref[D][name][sel]))[:4].tolist())


def test_scan_accepts_one_column_as_a_vector_and_refuses_bad_temperatures(gpu):
    LL, V = _inputs(500, "inf")
    a, b = gpu.posterior.tf_scan(LL, [3.0, 7.0], V[2]), gpu.posterior.tf_scan(LL, [3.0, 7.0], V[2:3])
    assert all(_same(a[n], b[n]) for n in a) and a["Q"].shape == (2, 1)
    for bad in ([1.0, 0.0], [np.nan], [-2.0], [np.inf], np.ones(65)):
        with pytest.raises(gpu.TrplError) as e:
            gpu.posterior.tf_scan(LL, bad, V[:2])
        assert e.value.code == gpu._abi.ERR_ARG


def test_the_device_form_can_be_captured_in_a_hip_graph(gpu):
    """trpl_posterior_tf_scan_dev allocates nothing and never synchronises: captured once, replayed twice on other
    likelihoods and temperatures in the same buffers, it gives the eager call's bits (and those are the host form's)."""
    import torch
    dv = gpu.device
    dev = torch.device("cuda", 0)
    S, D, K = 3 * K_THREADS + 5, 13, 64
    (lla, va), (llb, vb) = _inputs(S, "inf"), _inputs(S + 1, "inf")
    data = {"a": (lla, va, TFS), "b": (llb[:S].copy(), np.ascontiguousarray(vb[:, :S]), TFS[::-1].copy())}
    LL = torch.empty(S, dtype=torch.float64, device=dev)
    V = torch.empty((D, S), dtype=torch.float64, device=dev)
    tfs = torch.empty(K, dtype=torch.float64, device=dev)
    out = {n: torch.zeros((K, 4 if n == "stats" else D), dtype=torch.float64, device=dev) for n in ("stats", "mean", "var", "Q")}
    ws = dv.posterior_tf_scan_workspace(S, D, K)

    def load(name):
        ll, v, t = data[name]
        LL.copy_(torch.from_numpy(ll)); V.copy_(torch.from_numpy(np.ascontiguousarray(v[:D]))); tfs.copy_(torch.from_numpy(t))

    def step():
        dv.posterior_tf_scan_device(LL, tfs, out["stats"], ws, V=V, mean=out["mean"], var=out["var"], Q=out["Q"])

    eager = {}
    for name in data:
        load(name)
        step()
        torch.cuda.synchronize()
        eager[name] = {n: t.clone() for n, t in out.items()}
        host = gpu.posterior.tf_scan(data[name][0], data[name][2], data[name][1][:D])
        assert all(_same(eager[name][n].cpu().numpy(), host[n]) for n in host), name
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
        for t in out.values():
            t.fill_(-1.0)
        torch.cuda.synchronize()
        for _ in range(2):                          # replayed twice: the same bits both times
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(out[n], eager[name][n]) for n in out), name
    assert not torch.equal(eager["a"]["Q"], eager["b"]["Q"])


# ---- find_best_tf against the reference's method ----
def _normalize(lnP):                                # utils.py:157-166
    lnP = np.exp(lnP - np.nanmax(lnP) + 1000 * np.log(2) - np.log(lnP.size))
    lnP /= np.nansum(lnP)
    return lnP


def _tf_driver(tf, xi, P):                          # utils.py:172-179 (w_sample_var :168-170, w_variance :202-204)
    Pt = _normalize(P / np.exp(tf))
    ws = np.sum(Pt ** 2)
    m = np.average(xi, weights=Pt)
    return -np.sqrt(ws * np.average((xi - m) ** 2, weights=Pt))


def _search_inputs():
    """S = 4096 samples of a parameter uniform in [-1, 1] whose likelihood peaks on both sides, |xi| = 0.8: the weighted
    variance is largest where few samples of both sides share the weight and falls to the prior's as tf grows, while
    sum W^2 falls too -- one maximum.  Verified on the CPU with the restatement above before these inputs were committed:
    Q on 8001 log-spaced temperatures over u0 * [1e-4, 1e4] rises strictly up to its maximum (tf = 0.649, Q = 0.39738) and
    falls strictly after it (no other local maximum), and the 44 points scipy.optimize.fmin visits from ln u0 all lie in
    tf = [0.60, 1.0003], well inside the bracket."""
    rng = np.random.default_rng(0)
    xi = rng.uniform(-1, 1, 4096)
    return xi, -2e4 * ((np.abs(xi) - 0.8) / 0.1) ** 2, 1.0


def test_find_best_tf_finds_at_least_fmins_maximum(gpu):
    from scipy.optimize import fmin
    xi, LL, u0 = _search_inputs()
    opt = fmin(_tf_driver, np.log(u0), args=(xi, LL), full_output=True, disp=False)
    tf_ref, q_ref = float(np.exp(opt[0][0])), float(-opt[1])
    info = {}
    tf, q = gpu.posterior.find_best_tf(xi, LL, u0, info=info)
    print("find_best_tf: tf %.9g Q %.15g in %d scans; fmin: tf %.9g Q %.15g" % (tf, q, info["scans"], tf_ref, q_ref))
    assert u0 * 1e-4 < tf_ref < u0 * 1e4 and not info["at_edge"]
    # the search covers a bracket that holds fmin's answer and ends 1e-6 from the maximiser: only rounding (of the
    # restatement against the device sums, ~1e-15) may leave it below fmin, which stops at xtol = 1e-4 in ln tf
    assert q >= q_ref * (1 - 1e-12), (q, q_ref)
    assert info["lo"] <= tf <= info["hi"] and info["hi"] / info["lo"] - 1 <= 1e-6
    assert info["scans"] == 5                       # ceil(ln(ln(1e8) / ln(1 + 1e-6)) / ln(63 / 2)), tests/test_tf_scan_host.py
    assert abs(tf / tf_ref - 1) < 1e-2              # the same maximum (fmin's own xtol is 1e-4 in ln tf; the peak is flat)
    near = gpu.posterior.tf_scan(LL, [tf * (1 - 1e-3), tf, tf * (1 + 1e-3)], xi)["Q"][:, 0]
    assert near[1] == q and near[1] >= near[0] and near[1] >= near[2], near
    # the value is the objective's: the restatement at the located temperature, to rounding
    assert abs(-_tf_driver(np.log(tf), xi, LL) / q - 1) < 1e-12


def test_calc_max_uncertainty_is_one_find_best_tf_per_column(gpu):
    xi, LL, u0 = _search_inputs()
    rng = np.random.default_rng(5)
    cols = {"p0": xi}
    for d in range(1, 13):                          # other parameters: shifted, scaled, correlated with xi or not at all
        cols["p%d" % d] = rng.normal(size=xi.size) * 10.0 ** (d - 6) + (d % 3) * xi ** (1 + d % 2)
    info = {}
    got = gpu.posterior.calc_max_uncertainty(cols, LL, 2000 * u0, info=info)
    single_scans = []
    for name, col in cols.items():
        one = {}
        assert got[name] == gpu.posterior.find_best_tf(col, LL, u0, info=one), name
        assert (info["lo"][name], info["hi"][name], info["at_edge"][name]) == (one["lo"], one["hi"], one["at_edge"]), name
        single_scans.append(one["scans"])
    assert list(got) == list(cols)
    assert info["scans"] == max(single_scans) == 5          # the rounds of ONE search
    print("calc_max_uncertainty: %d rounds, %d device scans; 13 separate searches: %d scans" % (
        info["scans"], info["device_scans"], sum(single_scans)))
    # the first round is one scan for all 13 columns; later rounds scan each distinct bracket once
    assert info["device_scans"] <= 1 + 13 * (info["scans"] - 1) < sum(single_scans)
