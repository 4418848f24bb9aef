"""TRPL_FLAG_CUT on the GPU (include/trpl.h, trpl_loglik_cut): the early stop of systems whose running squared error has
passed the caller's level, checked through the C ABI against the PLAIN call on the same inputs (trpl_loglik / trpl_loglik_obs,
the code every other test pins) -- never against figures of the cut kernels themselves:
  * an uncut system is the plain call's, bit for bit; cut_col >= 0 exactly where the plain call's final sse > sse_cut;
  * a cut system reports what the plain call TRUNCATED to its cut_col observations reports (sse, floor_col and, on the grid,
    iters_total), its sum is above the level and the sum one batch earlier was not;
  * outputs do not depend on pairing rule, seam form or sharding, with broken neighbours in the batch;
  * driver.bayes with gpu_info["cut_margin"] = exact_cut_margin(tf) gives the uncut run's posterior weights, bit for bit.
The level of every comparison is the median of the plain call's sse: it splits the batch by construction, and the tests
require at least a quarter of the systems on either side (conditions of the test, not measurements)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_common import DT
from test_gpu_pair_kernel import _pair_batch

pytestmark = pytest.mark.gpu

KERNELS = {
    "single": lambda A: dict(kernel="single"),
    "pair": lambda A: dict(kernel="pair"),
    "pair_always_seam": lambda A: dict(kernel="pair", extra_flags=A.FLAG_PAIR_ALWAYS_SEAM),
}
OUT = ("sse", "status", "iters_total", "floor_col")


def _workload(gpu, name):
    w = gpu.workloads
    ini, lens = w.power_scan(128) if name == "power_scan" else w.twothick(128)
    return w.samples(64 if name == "power_scan" else 32, seed=17), ini, lens


def _observations(C, T, plT, offgrid):
    """On the grid: curve c has ncol - 3 c points of a straight line in log10 (unequal counts: curves of unequal n_obs are not
    paired with each other).  Off the grid: sorted random times, 300 + 7 c of them."""
    ncol = T // plT + 1
    if not offgrid:
        return None, [18.0 - 0.2 * DT * plT * np.arange(ncol - 3 * c) for c in range(C)]
    rng = np.random.default_rng(5)
    times = [np.sort(rng.uniform(0.0, T * DT, 300 + 7 * c)) for c in range(C)]
    return times, [18.0 - 0.2 * t + 0.05 * rng.standard_normal(len(t)) for t in times]


def _run(gpu, X, ini, lens, T, obs, times, kw, sse_cut=None, upto=None, P=None, L=128):
    """One call; upto = k truncates every curve to its first min(k, n_obs) observations (the plain call a cut is compared with)."""
    if upto is not None:
        obs = [o[:upto] for o in obs]
        times = None if times is None else [t[:upto] for t in times]
    info = {}
    P = gpu.loglik(X, ini, lens, T * DT, L, T, obs, times=times, info=info, sse_cut=sse_cut,
                   P=None if P is None else P.copy(), **kw)
    info["P"] = P
    return info


def _check_against_plain(gpu, X, ini, lens, T, obs, times, kw, label, L=128):
    """L: the grid size (tests/test_gpu_stepper_grids.py runs this at every compiled one)."""
    n_obs = np.array([len(o) for o in obs])
    C, S = len(obs), len(X)
    P_in = np.linspace(-3.0, 5.0, S)
    ref = _run(gpu, X, ini, lens, T, obs, times, kw, P=P_in, L=L)
    conv = ref["status"] == 0
    level = float(np.median(ref["sse"][conv]))
    out = _run(gpu, X, ini, lens, T, obs, times, kw, sse_cut=level, P=P_in, L=L)
    cc = out["cut_col"]
    cut, uncut = cc >= 0, cc == -1
    print("%s: level %.6g, cut %d / uncut %d / flagged %d of %d; iterations cut / plain = %.4f; cut counts %s"
          % (label, level, cut.sum(), uncut.sum(), (cc == -2).sum(), cc.size,
             out["iters_total"].sum() / ref["iters_total"].sum(), sorted(set(cc[cut].tolist()))))
    assert cut.sum() * 4 >= cc.size and uncut.sum() * 4 >= cc.size
    # a non-converged system: as in the plain call, cut_col = -2
    assert np.array_equal(out["status"], ref["status"]) and np.array_equal(cc == -2, ~conv)
    # exact equivalence
    assert np.array_equal(cut, conv & (ref["sse"] > level))
    # uncut systems (and flagged ones): the plain call's bits
    for k in OUT:
        assert np.array_equal(out[k][~cut], ref[k][~cut]), k
    # cut systems against the plain call truncated to their count
    assert (out["sse"][cut] > level).all()
    for k in sorted(set(cc[cut].tolist())):
        m = cc == k
        assert (n_obs[np.nonzero(m)[0]] >= k).all()
        tr = _run(gpu, X, ini, lens, T, obs, times, kw, upto=k, L=L)
        assert np.array_equal(out["sse"][m], tr["sse"][m]), k
        assert np.array_equal(out["floor_col"][m], tr["floor_col"][m]), k
        assert not tr["status"][m].any()
        if times is None:
            assert np.array_equal(out["iters_total"][m], tr["iters_total"][m]), k
            assert ((k % 64 == 0) | (n_obs[np.nonzero(m)[0]] == k)).all(), k
            if k > 64 and k % 64 == 0:                                   # minimality: one batch earlier the sum was not above
                before = _run(gpu, X, ini, lens, T, obs, times, kw, upto=k - 64, L=L)
                assert (before["sse"][m] <= level).all(), k
    # iterations
    assert out["iters_total"].sum() < ref["iters_total"].sum()
    assert (out["iters_total"][cut] <= ref["iters_total"][cut]).all()
    # P, with a non-zero incoming P: the reported sums leave it in curve order
    acc = P_in.copy()
    for c in range(C):
        acc = acc + (0.0 - out["sse"][c])
    assert np.array_equal(out["P"], acc)
    some_cut = cut.any(axis=0)
    assert (out["P"][some_cut] >= ref["P"][some_cut]).all() and (out["P"][some_cut] <= P_in[some_cut] - level).all()
    return ref, out, level


@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("workload", ["power_scan", "twothick"])
def test_cut_systems_equal_the_truncated_plain_call_and_uncut_systems_the_full_one(gpu, workload, kernel, predict):
    X, ini, lens = _workload(gpu, workload)
    T = 330                                                   # 331 columns: five full batches and a partial one
    times, obs = _observations(len(lens), T, 1, False)
    kw = dict(KERNELS[kernel](gpu._abi), predict=predict)
    _check_against_plain(gpu, X, ini, lens, T, obs, times, kw, "%s %s predict=%s" % (workload, kernel, predict))


@pytest.mark.parametrize("workload", ["power_scan", "twothick"])
@pytest.mark.parametrize("variant", ["plT2", "pl_f32_normalize", "offgrid"])
def test_cut_with_a_pl_stride_with_f32_staging_and_off_the_grid(gpu, workload, variant):
    X, ini, lens = _workload(gpu, workload)
    A = gpu._abi
    if variant == "plT2":
        T, kw = 660, dict(kernel="pair", plT=2)
        times, obs = _observations(len(lens), T, 2, False)
    elif variant == "pl_f32_normalize":
        T, kw = 330, dict(kernel="single", pl_f32=True, normalize=True)
        times, obs = _observations(len(lens), T, 1, False)
        obs = [o - 18.0 for o in obs]                         # self-normalised PL starts at 1
    else:
        T, kw = 330, dict(kernel="pair")
        times, obs = _observations(len(lens), T, 1, True)
    assert A.FLAG_CUT == 0x800000
    _check_against_plain(gpu, X, ini, lens, T, obs, times, kw, "%s %s" % (workload, variant))


@pytest.mark.parametrize("kernel", ["single", "pair"])
def test_limit_values_of_the_level(gpu, kernel):
    X, ini, lens = _workload(gpu, "power_scan")
    T = 200
    times, obs = _observations(3, T, 1, False)
    obs[2] = obs[2][:40]                                      # a curve shorter than one batch
    kw = dict(kernel=kernel)
    ref = _run(gpu, X, ini, lens, T, obs, times, kw)
    inf = _run(gpu, X, ini, lens, T, obs, times, kw, sse_cut=float("inf"))
    for k in OUT + ("P",):
        assert np.array_equal(inf[k], ref[k]), k
    assert (inf["cut_col"] == -1).all() and inf["cut_fraction"] == 0.0
    zero = _run(gpu, X, ini, lens, T, obs, times, kw, sse_cut=0.0)
    assert not ref["status"].any() and (ref["sse"] > 0).all()
    want = np.minimum(64, np.array([len(o) for o in obs]))[:, None] * np.ones((1, len(X)), dtype=np.int64)
    assert np.array_equal(zero["cut_col"], want) and zero["cut_fraction"] == 1.0
    for bad in (float("nan"), -1.0, -float("inf")):
        with pytest.raises(ValueError):
            _run(gpu, X, ini, lens, T, obs, times, kw, sse_cut=bad)


@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
def test_outputs_do_not_depend_on_pairing_rule_seam_form_or_sharding(gpu, predict):
    """A batch with broken neighbours: the clean batch of the pair-kernel tests (their generator, imported) with the broken rows
    of test_paired_kernel_isolates_a_broken_system_from_its_partner -- a NaN lifetime, an infinite rate, a zero lifetime, a
    negative diffusivity -- and the hostile spread of test_optimistic_seam_equals_the_always_isolating_kernel_on_hostile_inputs
    on every fourth row (40 decades, one special value in eight rows), under a small iteration cap."""
    A = gpu._abi
    S, T = 600, 200
    X, ini, lens = _pair_batch(gpu, 5120, T)
    X = np.ascontiguousarray(X[:S])
    X[10, 9] = np.nan
    X[21, 4] = np.inf
    X[300, 9] = 0.0
    X[301, 2] = -1e9
    rng = np.random.RandomState(12)
    rows = np.arange(3, S, 4)
    X[rows, :12] *= 10.0 ** rng.uniform(-20, 20, size=(rows.size, 12))
    special = np.array([0.0, -1.0, np.inf, -np.inf, np.nan, 1e-310, 1e300, -1e-300])
    hit = rows[::8]
    X[hit, rng.randint(0, 12, size=hit.size)] = special[rng.randint(0, special.size, size=hit.size)]
    obs = [18.0 - 0.2 * DT * np.arange(T + 1)] * 3
    kw = dict(kernel="pair", predict=predict, MAX=1000)
    ref = _run(gpu, X, ini, lens, T, obs, None, kw)
    conv = ref["status"] == 0
    finite = conv & np.isfinite(ref["sse"])
    level = float(np.median(ref["sse"][finite]))
    base = _run(gpu, X, ini, lens, T, obs, None, kw, sse_cut=level)
    cut = base["cut_col"] >= 0
    flagged = int((~conv).sum())
    print("hostile batch predict=%s: %d systems, %d flagged, %d cut, %d NaN sums" % (predict, conv.size, flagged, cut.sum(),
                                                                                 int(np.isnan(ref["sse"]).sum())))
    assert flagged > 10 and cut.sum() * 4 >= conv.size
    # exact equivalence (the plain call's sse of a non-converged system is +inf: above every level)
    assert np.array_equal(cut[conv], (ref["sse"] > level)[conv])                # a NaN sum is never cut
    # A system the plain call flags is flagged here too (cut_col = -2, the plain call's outputs), unless its sum passed the
    # level BEFORE the step that fails: it stopped there, converged so far, and is a cut system like any other -- what the
    # plain call truncated to cut_col observations reports.  It is never reported uncut.
    cc = base["cut_col"]
    late = cut & ~conv
    print("   of the flagged systems, %d were cut before their failing step" % late.sum())
    assert np.array_equal(cc == -2, ~conv & ~late) and not (cc[~conv] == -1).any()
    assert ((cc[late] - 1) < ref["status"][late] - 1).all() and not base["status"][late].any()
    for k in sorted(set(cc[late].tolist())):
        m = late & (cc == k)
        tr = _run(gpu, X, ini, lens, T, obs, None, kw, upto=k)
        for key in OUT:
            assert np.array_equal(base[key][m], tr[key][m]), (k, key)
        assert (base["sse"][m] > level).all()
    for k in OUT:
        assert np.array_equal(base[k][~cut], ref[k][~cut], equal_nan=(k == "sse")), k
    keys = OUT + ("cut_col", "P")
    for extra in (A.FLAG_PAIR_ADJACENT, A.FLAG_PAIR_ALWAYS_SEAM, A.FLAG_PAIR_ADJACENT | A.FLAG_PAIR_ALWAYS_SEAM):
        other = _run(gpu, X, ini, lens, T, obs, None, dict(kw, extra_flags=extra), sse_cut=level)
        for k in keys:
            assert other[k].tobytes() == base[k].tobytes(), (hex(extra), k)
    for bounds in ((0, 301, S), (0, 199, 402, S)):                              # 2 and 3 shards, odd ones among them
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            part = _run(gpu, X[lo:hi], ini, lens, T, obs, None, kw, sse_cut=level)
            for k in keys:
                whole = base[k][lo:hi] if k == "P" else base[k][:, lo:hi]
                assert part[k].tobytes() == np.ascontiguousarray(whole).tobytes(), (bounds, lo, k)


@pytest.mark.parametrize("kernel", ["single", "pair"])
def test_a_flagged_system_is_as_in_the_plain_call(gpu, kernel):
    X, ini, lens = _workload(gpu, "power_scan")
    X = X[:16].copy()
    X[5, 9] = np.nan                                          # tau_n: never converges
    T = 200
    obs = [18.0 - 0.2 * DT * np.arange(T + 1)] * 3
    kw = dict(kernel=kernel, MAX=200)
    ref = _run(gpu, X, ini, lens, T, obs, None, kw)
    level = float(np.median(ref["sse"][ref["status"] == 0]))
    out = _run(gpu, X, ini, lens, T, obs, None, kw, sse_cut=level)
    assert (ref["status"][:, 5] > 0).all() and np.array_equal(out["status"], ref["status"])
    assert (out["cut_col"][:, 5] == -2).all() and np.isposinf(out["sse"][:, 5]).all() and (out["floor_col"][:, 5] == -2).all()
    assert np.isneginf(out["P"][5]) and np.array_equal(out["iters_total"][:, 5], ref["iters_total"][:, 5])
    ok = np.setdiff1d(np.arange(16), [5])
    assert (out["cut_col"][:, ok] >= -1).all() and (out["cut_col"][:, ok] >= 0).any()


def test_bayes_with_the_exact_margin_gives_the_uncut_posterior(gpu, tmp_path):
    """driver.bayes over the default box against the shipped observations, 8 sample blocks: with gpu_info["cut_margin"] =
    exact_cut_margin(tf) the posterior weights at that tf and the best sample's P are the uncut run's, bit for bit, and later
    blocks do cut.  The window is the first 50 ns of obs_balanced_full.csv.gz (2001 points per curve) rather than the 6 ns of
    obs_balanced_6ns.csv: a sample has to lie exact_cut_margin(1) = 1439 below the best one to be cut, i.e. 0.5 decades off on
    average over 3 x 2001 points against 1.4 decades over 3 x 241 -- the margin stays what the derivation gives, the window is
    what makes the condition `cut_fraction > 0` safe."""
    import gzip
    sm = gpu.sampler
    obs_csv = str(tmp_path / "Balancedhighsurf_Power_scan_Observations.csv")
    with gzip.open(os.path.join(GOLDEN, "obs_balanced_full.csv.gz"), "rb") as fh, open(obs_csv, "wb") as out:
        out.write(fh.read())
    ini = gpu.get_initpoints(os.path.join(GOLDEN, "exc_power_scan.csv"), {"select_obs_sets": None})
    flags = {"load_PL_from_file": False, "override_equal_auger": False, "override_equal_mu": False, "override_equal_s": False,
             "log_pl": True, "self_normalize": False, "random_sample": True, "num_points": 256}
    e_data = gpu.get_data([obs_csv], {"time_cutoff": 50, "select_obs_sets": None, "noise_level": None}, flags, scale_f=1e-23)
    Time, T = 50.0, 2000
    assert all(len(t) <= T + 1 for t in e_data[0][0])
    simPar = [2000.0, Time, 128, T, 1, (0,), 7, 10000]
    minX, maxX = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS
    base = dict(num_gpus=1, has_GPU=True, max_sims_per_block=1, sims_per_gpu=32, fused=True, pl_dtype=np.float64)

    def run(**kw):
        return gpu.bayes(gpu.pvSim, None, None, minX, maxX, sm.DEFAULT_DO_LOG, ini, list(simPar), e_data, dict(flags),
                         dict(base, **kw), rng=np.random.RandomState(42))
    _, P0, X0 = run()
    _, Pn, Xn = run(cut_margin=None)
    assert np.array_equal(P0, Pn) and np.array_equal(X0, Xn)
    best = int(np.nanargmax(P0[0]))
    for tf in (1.0, 4.0):
        log = []
        margin = gpu.posterior.exact_cut_margin(tf)
        _, Pc, Xc = run(cut_margin=margin, cut_log=log)
        assert np.array_equal(Xc, X0) and len(log) == 8 and log[0]["sse_cut"] == float("inf") and log[0]["cut_fraction"] == 0.0
        print("tf = %g: margin %.2f; spread of the uncut P: best %.1f, median %.1f; cut fraction per block %s; iterations of "
              "blocks 2.. = %d" % (tf, margin, P0[0, best], np.nanmedian(P0[0]),
                                         ["%.2f" % b["cut_fraction"] for b in log], sum(b["iters_total"] for b in log[1:])))
        assert all(a["sse_cut"] >= b["sse_cut"] for a, b in zip(log[:-1], log[1:]))            # the level only tightens
        W0, Wc = gpu.posterior.weights(P0[0], tf), gpu.posterior.weights(Pc[0], tf)
        assert W0.tobytes() == Wc.tobytes()
        assert Pc[0, best] == P0[0, best] and int(np.nanargmax(Pc[0])) == best
        changed = Pc[0] != P0[0]
        assert (W0[changed] == 0.0).all() and (Pc[0][changed] >= P0[0][changed]).all()
        if tf == 1.0:
            assert max(b["cut_fraction"] for b in log[1:]) > 0.0
    for bad, word in ((dict(devices=[0]), "devices"), (dict(num_gpus=2), "num_gpus"), (dict(max_sims_per_block=2), "max_sims_per_block"),
                      (dict(mag_grid=[0.0]), "mag_grid"), (dict(weighted=True), "weighted"), (dict(fused=False), "fused")):
        with pytest.raises(ValueError) as ei:
            run(cut_margin=1.0, **bad)
        assert word in str(ei.value), (word, str(ei.value))


def test_the_device_call_can_be_captured_in_a_hip_graph(gpu):
    """trpl_loglik_cut_dev allocates nothing and never synchronises: captured once, replayed on other samples (modelled on the
    capture test of trpl_loglik_dev in test_gpu_resume.py)."""
    import torch
    dv = gpu.device
    w = gpu.workloads
    dev = torch.device("cuda", 0)
    L, T, S = 128, 130, 4096 + 3
    ini, lens = w.power_scan(L)
    C = len(lens)
    Xa, Xb = w.samples(S, seed=11), w.samples(S, seed=12)
    ini_d = torch.from_numpy(ini).to(dev)
    obs = torch.from_numpy(np.ascontiguousarray(np.stack([18.0 - 0.2 * DT * np.arange(T + 1)] * C))).to(dev)
    X = torch.from_numpy(Xa).to(dev)
    P = torch.zeros(S, dtype=torch.float64, device=dev)
    sse = torch.empty((C, S), dtype=torch.float64, device=dev)
    it = torch.zeros((C, S), dtype=torch.int64, device=dev)
    cc = torch.zeros((C, S), dtype=torch.int32, device=dev)
    P.zero_()
    dv.loglik_device(X, ini_d, lens, T * DT, L, T, obs, [T + 1] * C, P, sse, iters_total=it, flags=gpu.FLAG_KERNEL_PAIR)
    torch.cuda.synchronize()
    level = float(sse.median())

    def step():
        P.zero_()
        dv.loglik_cut_device(X, ini_d, lens, T * DT, L, T, obs, [T + 1] * C, level, P, sse, cut_col=cc, iters_total=it,
                             flags=gpu.FLAG_KERNEL_PAIR)

    eager = {}
    for name, Xh in (("a", Xa), ("b", Xb)):
        X.copy_(torch.from_numpy(Xh))
        step()
        torch.cuda.synchronize()
        eager[name] = (P.clone(), it.clone(), cc.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        X.copy_(torch.from_numpy(Xa))
        step()                                      # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            step()
    for name, Xh in (("b", Xb), ("a", Xa), ("b", Xb)):
        X.copy_(torch.from_numpy(Xh))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(P, eager[name][0]) and torch.equal(it, eager[name][1]) and torch.equal(cc, eager[name][2]), name
    assert (eager["a"][2] >= 0).any() and (eager["a"][2] == -1).any() and not torch.equal(eager["a"][0], eager["b"][0])
