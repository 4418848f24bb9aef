"""TRPL_FLAG_PREDICT (include/trpl.h): every time step's iteration starts from the extrapolated history instead of U^t.
The mode is checked at solution level -- there is no CPU twin of it: the same solution as the default path to the header's
5e-5 / 3e-4 above the floor (T = 8000 / 80 000) with about half the solves, at least as close to the exact per-step solution, second-order convergence
under time-step refinement, FAST following STRICT's iteration path, independence from pairing / seam / sharding, bit-exact
resume, and the public layers reaching the same kernels."""
import numpy as np
import pytest

from gpu_common import (DT, ENVELOPE_K, ENVELOPE_K_L512, FLOOR, excess_scale, follows_iteration_path, nthreads,
                        record)

pytestmark = pytest.mark.gpu

# the header's tolerance against the default path, above TRPL_PL_FLOOR_EXCESS, by window length (steps)
REL = {8000: 5e-5, 80000: 3e-4}


def _above(pl, X, length, L=128):
    """PL points above the cancellation floor: PL >= TRPL_PL_FLOOR_EXCESS * B L n0p0."""
    return pl >= FLOOR * excess_scale(X, length, L)[:, None]


def _pl_pair(gpu, X12, length, Time, L, T, ini, **kw):
    d = gpu.solve_pl(X12, length, Time, L, T, ini, **kw)
    p = gpu.solve_pl(X12, length, Time, L, T, ini, predict=True, **kw)
    return d, p


# ------------------------------------------------------------------------------------------------------- 1
# tools/bench_predict.py's four configurations at the size of its error subset (256 samples, the default seed: the bench batch's
# first rows) on the kernel the bench times, and Power_scan on a second seed
SAME = {"power_scan_T8000": ("power_scan", 128, 8000, 42), "power_scan_T8000_seed3": ("power_scan", 128, 8000, 3),
        "twothick_T8000": ("twothick", 128, 8000, 42), "l512_T8000": ("power_scan", 512, 8000, 42),
        "power_scan_T80000": ("power_scan", 128, 80000, 42)}


@pytest.mark.parametrize("case", list(SAME))
def test_same_solution_with_about_half_the_solves(gpu, case):
    w = gpu.workloads
    workload, L, T, seed = SAME[case]
    Time = T * DT
    ini, lens = w.power_scan(L) if workload == "power_scan" else w.twothick(L)
    S = 256
    kernel = "pair" if L == 128 else "single"
    X = w.samples(S, seed=seed)
    n_obs = 2001
    mark = (w.MARKED_POINT * gpu.UNIT_CONVERSIONS)[None, :-1]
    obs, rel, ratio, resid = [], 0.0, [], np.zeros(S)
    dd = dp = 0.0                                                     # each path's distance to a tol-11 solution
    for c in range(len(lens)):
        pm = gpu.solve_pl(mark, lens[c], n_obs * DT - DT, L, n_obs - 1, ini[c])[0][0]
        obs.append(np.log10(pm))
        (pd, sd, itd, _), (pp, sp, itp, _) = _pl_pair(gpu, X[:, :12], lens[c], Time, L, T, ini[c], kernel=kernel)
        ref, sr, _, _ = gpu.solve_pl(X[:, :12], lens[c], Time, L, T, ini[c], kernel=kernel, tol=11)
        assert not sd.any() and not sp.any() and not sr.any()
        ok = _above(pd, X, lens[c], L)
        assert ok.mean() > 0.5
        rel = max(rel, float(np.max(np.abs(pp[ok] / pd[ok] - 1))))
        dd = max(dd, float(np.max(np.abs(pd[ok] / ref[ok] - 1))))
        dp = max(dp, float(np.max(np.abs(pp[ok] / ref[ok] - 1))))
        ratio.append(float(itp.sum() / itd.sum()))
        resid += np.abs(np.log10(np.maximum(pd[:, :n_obs], np.finfo(float).tiny)) + X[:, 12:13] - obs[-1]).sum(axis=1)
    record("predict_same_solution_%s_pl" % case, {"pl_rel_max": rel, "vs_tol11": {"default": dd, "predict": dp},
                                                  "iter_ratio": ratio})
    assert rel <= REL[T], rel
    assert dp <= dd, (dp, dd)                                         # at least as close to the exact step solution
    assert max(ratio) <= 0.6, ratio
    # through trpl_loglik (observations over the first 2001 columns): the same (empty) set of flagged systems, and the
    # likelihood bound that follows from the PL bound of a window of up to 8000 steps
    di, pi = {}, {}
    Pd = gpu.loglik(X, ini, lens, Time, L, T, obs, info=di)
    Pp = gpu.loglik(X, ini, lens, Time, L, T, obs, info=pi, predict=True)
    assert np.array_equal(di["status"], pi["status"]) and not di["status"].any()
    assert pi["iters_total"].sum() <= 0.6 * di["iters_total"].sum()
    free = (di["floor_col"] < 0).all(axis=0)                 # samples whose compared columns all lie above the floor
    assert free.mean() > 0.5
    delta = np.log10(1 + REL[8000])
    bound = 2 * delta * resid + len(lens) * n_obs * delta ** 2
    assert (np.abs(Pp - Pd)[free] <= bound[free]).all(), float(np.max((np.abs(Pp - Pd) / bound)[free]))
    assert not np.array_equal(Pp, Pd)                         # the flag reached the kernel


# ------------------------------------------------------------------------------------------------------- 2
def test_at_least_as_close_to_the_exact_step_solution(gpu):
    w = gpu.workloads
    T, L = 8000, 128
    Time = T * DT
    ini, lens = w.power_scan(L)
    X = w.samples(16, seed=7)
    dd, dp = 0.0, 0.0
    for c in range(3):
        ref, st, _, _ = gpu.solve_pl(X[:, :12], lens[c], Time, L, T, ini[c], tol=11)
        assert not st.any()
        (pd, _, _, _), (pp, _, _, _) = _pl_pair(gpu, X[:, :12], lens[c], Time, L, T, ini[c])
        ok = _above(ref, X, lens[c], L)
        dd = max(dd, float(np.max(np.abs(pd[ok] / ref[ok] - 1))))
        dp = max(dp, float(np.max(np.abs(pp[ok] / ref[ok] - 1))))
    assert dp <= 2 * dd and dp <= 1e-6, (dp, dd)
    record("predict_vs_tol11", {"default": dd, "predict": dp})


# ------------------------------------------------------------------------------------------------------- 3
def test_converges_at_second_order_under_refinement(gpu, golden):
    import refine_common as R
    g = golden("tester_refine")
    L, T, Time = int(g["L"]), int(g["T"]), float(g["time"])
    rec = {}
    for f in range(len(g["lengths"])):
        X, length, dN = R.film_inputs(g, f)
        ode = g["plI_odeint"][f]
        devs = {"default": {}, "predict": {}}
        for k in R.REFINE_K:
            for name, kw in (("default", {}), ("predict", dict(predict=True))):
                pl, st, _, _ = gpu.solve_pl(X[:, :-1], length, Time, L, T * k, dN, plT=k, kernel="single", **kw)
                assert not st.any()
                devs[name][k] = R.deviation(pl, ode)
        for name, d in devs.items():
            worst, end = R.check_refinement(d, label="film %d, %s" % (f, name))
            rec["film%d_%s" % (f, name)] = {"worst": worst, "end": end}
    record("predict_refine", rec)


# ------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("shape", ["pair", "single128", "single512"])
def test_fast_follows_strict_in_the_mode(gpu, shape):
    w = gpu.workloads
    L = 512 if shape == "single512" else 128
    T = 8000 if L == 128 else 2000
    Time = T * DT
    ini, lens = w.power_scan(L)
    X = w.samples(64 if L == 128 else 16, seed=9)
    kernel = "pair" if shape == "pair" else "single"
    K = ENVELOPE_K_L512 if L == 512 else ENVELOPE_K[2000.0]
    for c in range(3):
        ps, ss, its, _ = gpu.solve_pl(X[:, :12], lens[c], Time, L, T, ini[c], strict=True, predict=True)
        pf, sf, itf, _ = gpu.solve_pl(X[:, :12], lens[c], Time, L, T, ini[c], kernel=kernel, predict=True)
        assert not ss.any() and not sf.any()
        follows_iteration_path(itf, its, "%s, curve %d" % (shape, c))
        r = ps / excess_scale(X, lens[c], L)[:, None]
        ok = ps > 0
        dev = np.abs(pf[ok] / ps[ok] - 1)
        assert (dev <= 1e-9 + K / r[ok]).all(), (c, float(np.max(dev * r[ok])))


# ------------------------------------------------------------------------------------------------------- 5
def _pair_runs(gpu, X, ini, lens, Time, T, obs):
    P = gpu._abi.FLAG_PREDICT
    out = {}
    runs = (("table", 0), ("adjacent", gpu._abi.FLAG_PAIR_ADJACENT), ("seam", gpu._abi.FLAG_PAIR_ALWAYS_SEAM))
    for name, extra in runs:
        info = {}
        Pv = gpu.loglik(X, ini, lens, Time, 128, T, obs, info=info, kernel="pair", extra_flags=extra | P)
        out[name] = dict(P=Pv, sse=info["sse"], it=info["iters_total"], st=info["status"], fc=info["floor_col"])
    k = len(X) // 2 + 1                                                      # two launches, cut inside a period
    parts = []
    for sl in (slice(0, k), slice(k, None)):
        info = {}
        Pv = gpu.loglik(X[sl], ini, lens, Time, 128, T, obs, info=info, kernel="pair", extra_flags=P)
        parts.append(dict(P=Pv, sse=info["sse"], it=info["iters_total"], st=info["status"], fc=info["floor_col"]))
    out["shard"] = {n: np.concatenate([parts[0][n], parts[1][n]], axis=-1) for n in parts[0]}
    for name in ("adjacent", "seam", "shard"):
        for n in ("P", "sse", "it", "st", "fc"):
            assert out[name][n].tobytes() == out["table"][n].tobytes(), (name, n)
    return out["table"]


def test_pairing_seam_and_shard_independence(gpu):
    w = gpu.workloads
    ini, lens = w.twothick(128)
    X = w.samples(1025, seed=17)
    T = 300
    obs = [np.linspace(17.0, 14.0, T + 1)] * 6
    clean = _pair_runs(gpu, X, ini, lens, T * DT, T, obs)
    assert np.isfinite(clean["P"]).all() and not clean["st"].any()
    # PL itself: optimistic against always-voiding seam, paired against one-system-per-wave is NOT asked (rounding)
    P = gpu._abi.FLAG_PREDICT
    a = gpu.solve_pl(X[:, :12], lens[0], T * DT, 128, T, ini[0], kernel="pair", extra_flags=P)
    b = gpu.solve_pl(X[:, :12], lens[0], T * DT, 128, T, ini[0], kernel="pair", extra_flags=P | gpu._abi.FLAG_PAIR_ALWAYS_SEAM)
    c = gpu.solve_pl(X[1:, :12], lens[0], T * DT, 128, T, ini[0], kernel="pair", extra_flags=P)
    for i in range(3):
        assert a[i].tobytes() == b[i].tobytes()
        assert a[i][1:].tobytes() == c[i].tobytes()
    # the hostile batch: non-finite systems beside finite partners exercise the repeat from the extrapolated start
    bad = X.copy()
    bad[10, 9] = np.nan
    bad[21, 4] = np.inf
    bad[300, 9] = 0.0
    bad[301, 2] = -1e9
    hostile = _pair_runs(gpu, bad, ini, lens, T * DT, T, obs)
    ok = np.setdiff1d(np.arange(len(X)), [10, 21, 300, 301])
    for n in ("sse", "it", "st", "fc"):
        assert hostile[n][:, ok].tobytes() == clean[n][:, ok].tobytes(), n
    assert hostile["P"][ok].tobytes() == clean["P"][ok].tobytes()
    assert (hostile["st"][:, [10, 21]] > 0).all() and not np.isfinite(hostile["P"][[10, 21]]).any()


# ------------------------------------------------------------------------------------------------------- 6
# the LDS-ring history (FAST, L >= 128: one-system and paired kernels) and the register history (STRICT at any L, FAST below
# L = 128), each of which reloads a checkpoint in its own code block
RESUME = {"single128": (dict(kernel="single"), 128), "pair128": (dict(kernel="pair"), 128),
          "strict128": (dict(strict=True), 128), "single64": (dict(kernel="single"), 64)}


@pytest.mark.parametrize("shape", list(RESUME))
@pytest.mark.parametrize("t0", [4, 5, 517])
def test_resume_is_the_uninterrupted_run(gpu, shape, t0):
    w = gpu.workloads
    kw, L = RESUME[shape]
    ini, lens = w.twothick(L)
    X = w.samples(9, seed=5)[:, :12]
    T = 600
    dt = 2.0 ** -5
    Time = T * dt
    mode = dict(kw, predict=True)
    late = (t0, t0 + 1, T)
    fs = {}
    full = gpu.solve_pl(X, lens[0], Time, L, T, ini[0], snap_steps=list(late), snapshots=fs, **mode)
    plain = gpu.solve_pl(X, lens[0], Time, L, T, ini[0], **mode)              # the instantiation without snapshots
    assert plain[0].tobytes() == full[0].tobytes() and np.array_equal(plain[2], full[2])
    ck = {}
    pl_a, st_a, it_a, _ = gpu.solve_pl(X, lens[0], t0 * dt, L, t0, ini[0], snap_steps=gpu.checkpoint_steps(t0),
                                       snapshots=ck, snap_raw=True, **mode)
    out = np.full((len(X), T + 1), np.nan)
    out[:, :t0 + 1] = pl_a
    gs = {}
    res = (t0, ck["plN"], ck["plP"], ck["plE"])
    pl_b, st_b, it_b, _ = gpu.solve_pl(X, lens[0], Time, L, T, None, out=out, resume=res, snap_steps=list(late),
                                       snapshots=gs, **mode)
    tail = np.full((len(X), t0 + 1), np.nan)
    _, _, it_c, _ = gpu.solve_pl(X, lens[0], t0 * dt, L, t0, None, out=tail, resume=res, **mode)
    assert not full[1].any() and not st_a.any() and not st_b.any()
    assert full[0].tobytes() == pl_b.tobytes()
    assert np.array_equal(full[2], it_a + it_b - it_c)
    for k in ("plN", "plP", "plE"):
        assert fs[k].tobytes() == gs[k].tobytes(), k
    # the continuation really extrapolates from the reloaded history: a default-path continuation differs
    d = gpu.solve_pl(X, lens[0], Time, L, T, None, out=out.copy(), resume=res, **kw)
    assert not np.array_equal(d[2], it_b)


# ------------------------------------------------------------------------------------------------------- 7
def test_public_layers_reach_the_predict_kernels(gpu, golden):
    w = gpu.workloads
    P = gpu._abi.FLAG_PREDICT
    ini, lens = w.power_scan(128)
    X = w.samples(40, seed=21)
    T = 400
    Time = T * DT
    obs = [np.linspace(16.5, 15.0, T + 1)] * 3
    direct = gpu.loglik(X, ini, lens, Time, 128, T, obs, extra_flags=P)
    assert np.array_equal(gpu.loglik(X, ini, lens, Time, 128, T, obs, predict=True), direct)
    assert not np.array_equal(gpu.loglik(X, ini, lens, Time, 128, T, obs), direct)
    assert np.array_equal(gpu.loglik(X, ini, lens, Time, 128, T, obs, predict=True, devices=[0, 0]), direct)
    times = [np.linspace(0.0, Time, 57)] * 3
    obs_t = [np.linspace(16.5, 15.0, 57)] * 3
    d_t = gpu.loglik(X, ini, lens, Time, 128, T, obs_t, times=times, extra_flags=P)
    assert np.array_equal(gpu.loglik(X, ini, lens, Time, 128, T, obs_t, times=times, predict=True), d_t)
    assert np.array_equal(gpu.loglik(X, ini, lens, Time, 128, T, obs_t, times=times, predict=True, devices=[0, 0]), d_t)
    # model.pvSim
    pl = np.zeros((len(X), T + 1))
    sim = (lens[0], Time, 128, T, 1, None, 7, 10000)
    info = {}
    gpu.pvSim(pl, None, None, None, X[:, :12], sim, ini[0], None, None, 1, init_mode="points", info=info, predict=True)
    ref = gpu.solve_pl(X[:, :12], lens[0], Time, 128, T, ini[0], extra_flags=P)
    assert pl.tobytes() == ref[0].tobytes() and np.array_equal(info["iters_total"], ref[2])
    # driver.simulate, fused (one experiment: trpl_loglik per block) and unfused (pvSim per curve)
    g = golden("bayes_e2e")
    Tg, tg = int(g["T"]), g["tgrid"]
    e_data = [([tg] * 3, list(g["obs0"]), [None] * 3)]
    flags = {"load_PL_from_file": False, "log_pl": True, "self_normalize": False}
    sim_params = [float(g["length"]), float(g["time"]), 128, Tg, 1, (0,), 7, 10000]
    Xg = g["X"]
    z = np.zeros(1)
    base = {"sims_per_gpu": 4, "num_gpus": 1}

    def run(model, **gi):
        Pm = np.zeros((1, len(Xg)))
        gpu.simulate(model, e_data, Pm, Xg, [None], [None], 3, sim_params, g["ini"], flags, dict(base, **gi), 0,
                     z.copy(), z.copy(), z.copy())
        return Pm

    fused = run(gpu.pvSim, fused=True, predict=True)
    want = gpu.loglik(Xg, g["ini"], float(g["length"]), float(g["time"]), 128, Tg, list(g["obs0"]), pl_f32=True,
                      extra_flags=P)
    assert fused[0].tobytes() == want.tobytes()

    def predicting(*a, **k):
        return gpu.pvSim(*a, predict=True, **k)
    predicting.reentrant = True
    unfused = run(gpu.pvSim, predict=True)
    assert unfused.tobytes() == run(predicting).tobytes()
    assert not np.array_equal(unfused, run(gpu.pvSim))
    assert np.max(np.abs(unfused / run(gpu.pvSim) - 1)) < 1e-4
