"""TRPL_FLAG_MOMENTS on the GPU (include/trpl.h: trpl_loglik_moments, trpl_mag_grid, trpl_mag_profile): the moments steppers
return trpl_loglik[_obs]'s outputs bit for bit plus esum = sum e_i, from which the likelihood at any magnitude offset follows
(the mag_grid loop of the reference's probs.lnP, probs.py:5-18, from one solve).

Tolerances are derived (the header's paragraph), not measured.  With A(d) = sse + 2 |d esum| + n d^2, eps = 2^-52:
  * formula against a direct evaluation at offset d on the same PL:  k eps (A(d) + |d| sum|e_i|), k = the depth of the summation
    actually used + 4 for the polynomial: FAST 6 levels inside a 64-column batch + ceil(n / 64) batches added serially, STRICT the
    serial sum of n terms.  Nothing is added to it.  sum|e_i| never leaves the kernel; it is formed from the fixture's
    reference PL (which the GPU's agrees with to 1e-9).
  * against the reference's lnP on the REFERENCE PL (tests/golden/lnp_maggrid.npz): FAST adds the header's envelope
    |d lg| <= 1e-9 / ln 10 per column, i.e. 2 sqrt(n sse(d)) 4.4e-10 on sse(d); STRICT only log10's 1 ulp,
    2 sqrt(n sse(d)) eps max|lg|.
Both PL fixtures sit far above the cancellation floor: no system is left out, floor_col == -1 is asserted."""
import os

import numpy as np
import pytest

from gpu_common import DT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
OFFSETS = np.linspace(-2.5, 2.5, 21)
MODES = {"strict": dict(strict=True), "single": dict(kernel="single"), "pair": dict(kernel="pair")}


def _depth(n, strict):
    return (n if strict else 6 + -(-n // 64)) + 4


def _same_outputs(info, ref, P, Pref):
    for k in ("sse", "status", "iters_total", "floor_col"):
        assert np.array_equal(info[k], ref[k]), k
    assert np.array_equal(P, Pref)


# ------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
@pytest.mark.parametrize("mode", list(MODES))
def test_moments_call_returns_the_plain_calls_outputs_bit_for_bit(gpu, mode, predict, offgrid):
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 9, 150                                        # odd S: the paired kernel's duplicated tail; 3 batches of columns
    Time = T * DT
    X = w.samples(S, seed=11)
    rng = np.random.default_rng(5)
    if offgrid:
        times = [np.sort(rng.uniform(0.0, Time, 140 + 7 * c)) for c in range(3)]
        obs = [18.0 - 0.2 * t + 0.05 * rng.standard_normal(len(t)) for t in times]
    else:
        times = None
        obs = [18.0 - 0.2 * DT * np.arange(T + 1 - 3 * c) for c in range(3)]      # 151, 148, 145 columns
    kw = dict(MODES[mode], predict=predict, times=times)
    ref, info = {}, {}
    Pref = gpu.loglik(X, ini, lens, Time, 128, T, obs, info=ref, **kw)
    Pm = gpu.loglik(X, ini, lens, Time, 128, T, obs, info=info, mag_grid=[0.0], **kw)
    assert not ref["status"].any()
    _same_outputs(info, ref, info["P"], Pref)             # info["P"]: the P of trpl_loglik_moments itself
    acc = np.zeros(S)
    for c in range(3):
        acc = acc + np.maximum(info["sse"][c], 0.0)
    assert np.array_equal(Pm[0], 0.0 - acc)              # offset 0: the grid's expression is sse itself
    assert np.isfinite(info["esum"]).all() and (np.abs(info["esum"]) <= np.sqrt(info["sse"] * np.array([len(o) for o in obs])[:, None]) * (1 + 1e-12)).all()


@pytest.mark.parametrize("L,mode,predict", [(32, "strict", False), (32, "single", True), (512, "single", False), (512, "single", True)])
def test_moments_outputs_at_the_small_and_the_large_grid(gpu, L, mode, predict):
    w = gpu.workloads
    ini, lens = w.power_scan(L)
    S, T = 4, 100
    X = w.samples(S, seed=12)
    obs = [18.0 - 0.2 * DT * np.arange(T + 1) for _ in range(3)]
    ref, info = {}, {}
    kw = dict(MODES[mode], predict=predict)
    Pref = gpu.loglik(X, ini, lens, T * DT, L, T, obs, info=ref, **kw)
    best, Pp = gpu.loglik(X, ini, lens, T * DT, L, T, obs, info=info, mag_profile=True, **kw)
    _same_outputs(info, ref, info["P"], Pref)
    assert np.isfinite(best).all() and (Pp >= Pref).all()


# ------------------------------------------------------------------------------------------------------- 6
def _fixture_case(key, name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name))
    g = np.load(os.path.join(ROOT, "tests", "golden", "lnp_maggrid.npz"))
    assert np.array_equal(g["offsets"], OFFSETS)
    X = np.array(z["X"], dtype=np.float64)
    X[:, 12] = g["mag_" + key]
    lens = np.array(z["lengths"]) if "lengths" in z.files else float(z["length"])
    pl = np.asarray(z["plI"], dtype=np.float64)
    T, n = int(z["T"]), pl.shape[2]
    e = np.log10(pl) + X[None, :, 12, None] - g["obs_" + key][:, None, :]
    return dict(X=X, ini=np.asarray(z["ini"]), lens=lens, Time=float(z["time"]), L=int(z["L"]), T=T, plT=T // (n - 1),
                tol=int(z["tol"]), MAX=int(z["MAX"]), obs=[o for o in g["obs_" + key]], P_ref=g["P_ref_" + key], n=n,
                sum_abs_e=np.abs(e).sum(axis=2), max_lg=float(np.abs(np.log10(pl)).max()))


@pytest.mark.parametrize("key,name", [("power", "pvsim_power.npz"), ("twothick", "pvsim_twothick.npz")])
@pytest.mark.parametrize("mode", list(MODES))
def test_mag_grid_against_the_references_lnp_and_against_direct_calls(gpu, mode, key, name):
    import torch
    f = _fixture_case(key, name)
    strict = mode == "strict"
    n, C, S = f["n"], len(f["obs"]), f["X"].shape[0]
    args = (f["ini"], f["lens"], f["Time"], f["L"], f["T"], f["obs"])
    kw = dict(MODES[mode], tol=f["tol"], MAX=f["MAX"], plT=f["plT"])
    info = {}
    P = gpu.loglik(f["X"], *args, info=info, mag_grid=OFFSETS, **kw)
    assert not info["status"].any() and (info["floor_col"] == -1).all()             # no system excluded anywhere
    sse, esum = info["sse"], info["esum"]
    k = _depth(n, strict)
    print("%s %s: n = %d, summation depth + 4 = %d" % (mode, key, n, k))
    worst_ref = worst_dir = 0.0
    for m, d in enumerate(OFFSETS):
        A_d = sse + 2 * np.abs(d * esum) + n * d * d
        sse_d = np.maximum((sse + (2.0 * d) * esum) + n * (d * d), 0.0)
        first = k * EPS * (A_d + abs(d) * f["sum_abs_e"])
        # (a) the reference's lnP on the reference PL
        pl_term = 2 * np.sqrt(n * sse_d) * (EPS * f["max_lg"] if strict else 4.4e-10)
        bound = (first + pl_term).sum(axis=0)
        err = np.abs(P[m] - f["P_ref"][:, :, m].sum(axis=0))
        worst_ref = max(worst_ref, float((err / bound).max()))
        assert (err <= bound).all(), ("lnP", mode, key, d, float((err / bound).max()))
        # (b) a direct call at X[:, 12] + d: the same PL bits
        Xd = f["X"].copy()
        Xd[:, 12] = Xd[:, 12] + d
        Pd = gpu.loglik(Xd, *args, **kw)
        bound = first.sum(axis=0)                                                    # the first bound, as the header states it
        err = np.abs(P[m] - Pd)
        worst_dir = max(worst_dir, float((err / bound).max()))
        assert (err <= bound).all(), ("direct", mode, key, d, float((err / bound).max()))
    print("%s %s: worst error / bound: against lnP %.3g, against direct calls %.3g" % (mode, key, worst_ref, worst_dir))
    # the device kernels equal the plain host forms bit for bit
    from trpl_amd import device as D
    n_obs = np.full(C, n, dtype=np.int64)
    ts, te = torch.tensor(sse, device="cuda"), torch.tensor(esum, device="cuda")
    Pg = torch.zeros((len(OFFSETS), S), dtype=torch.float64, device="cuda")
    D.mag_grid_device(ts, te, n_obs, OFFSETS, Pg)
    assert np.array_equal(Pg.cpu().numpy(), P)
    for per_curve in (False, True):
        bh, Ph = gpu.loglik(f["X"], *args, mag_profile="per_curve" if per_curve else True, **kw)
        bd = torch.zeros((C, S) if per_curve else (S,), dtype=torch.float64, device="cuda")
        Pd_ = torch.zeros(S, dtype=torch.float64, device="cuda")
        D.mag_profile_device(ts, te, n_obs, bd, Pd_, per_curve=per_curve)
        assert np.array_equal(bd.cpu().numpy(), bh) and np.array_equal(Pd_.cpu().numpy(), Ph)
        assert (Ph >= P.max(axis=0) - 64 * EPS * np.abs(Ph)).all()                   # the profile dominates every grid point


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("mode,predict", [("pair", False), ("single", True), ("strict", False)])
def test_device_resident_moments_call_equals_the_device_resident_plain_call(gpu, mode, predict, offgrid):
    """trpl_loglik_moments_dev against trpl_loglik_dev / trpl_loglik_obs_dev on resident tensors: every output array_equal."""
    import torch
    from trpl_amd import device as D
    from trpl_amd.driver import bracket_times
    A = gpu._abi
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 16, 130
    Time = T * DT
    X = torch.tensor(w.samples(S, seed=4), device="cuda")
    tini = torch.tensor(np.ascontiguousarray(ini), device="cuda")
    flags = {"pair": A.FLAG_KERNEL_PAIR, "single": A.FLAG_KERNEL_SINGLE, "strict": A.FLAG_STRICT}[mode] | (A.FLAG_PREDICT if predict else 0)
    br = None
    if offgrid:
        rng = np.random.default_rng(8)
        t = np.sort(rng.uniform(0.0, Time, 120))
        hi, dx, h = bracket_times(np.linspace(0, Time, T + 1), t)
        obs = torch.tensor(np.stack([18.0 - 0.2 * t] * 3), device="cuda")
        br = [torch.tensor(np.ascontiguousarray(np.stack([a] * 3)), device="cuda") for a in (hi.astype(np.int32), dx, h)]
        n_obs = 120
    else:
        obs = torch.tensor(np.stack([18.0 - 0.2 * DT * np.arange(T + 1)] * 3), device="cuda")
        n_obs = T + 1
    out = {}
    for name in ("plain", "moments"):
        P = torch.zeros(S, dtype=torch.float64, device="cuda")
        sse = torch.zeros((3, S), dtype=torch.float64, device="cuda")
        st = torch.zeros((3, S), dtype=torch.int32, device="cuda")
        it = torch.zeros((3, S), dtype=torch.int64, device="cuda")
        fl = torch.zeros((3, S), dtype=torch.int32, device="cuda")
        if name == "plain" and offgrid:
            D.loglik_obs_device(X, tini, lens, Time, 128, T, obs, br[0], br[1], br[2], n_obs, P, sse, st, it, flags=flags, floor_col=fl)
        elif name == "plain":
            D.loglik_device(X, tini, lens, Time, 128, T, obs, n_obs, P, sse, st, it, flags=flags, floor_col=fl)
        else:
            es = torch.zeros((3, S), dtype=torch.float64, device="cuda")
            kw = dict(obs_hi=br[0], obs_dx=br[1], obs_h=br[2]) if offgrid else {}
            D.loglik_moments_device(X, tini, lens, Time, 128, T, obs, n_obs, P, sse, es, st, it, flags=flags, floor_col=fl, **kw)
            assert torch.isfinite(es).all()
        torch.cuda.synchronize()
        out[name] = [t_.cpu().numpy() for t_ in (P, sse, st, it, fl)]
    assert not out["plain"][2].any()
    for a, b in zip(out["plain"], out["moments"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_moments_from_stored_pl(gpu, dtype, offgrid):
    """trpl_loglik_moments_from_pl_dev: sse and P array_equal to trpl_loglik_from_pl_dev on the same rows; esum against the
    NumPy sum of the same errors within its reduction's bound -- the kernel sums ceil(n / 256) terms serially per thread, 6
    shuffle levels and 3 adds across the block's four wavefronts: depth ceil(n / 256) + 9, times eps sum|e_i|; a flagged row
    gets NaN (its sse +inf)."""
    import torch
    from trpl_amd import device as D
    from trpl_amd.driver import bracket_times
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 12, 300
    Time = T * DT
    X = w.samples(S, seed=9)
    tdt = torch.float32 if dtype == "float32" else torch.float64
    mat = torch.tensor(np.ascontiguousarray(X[:, :12]), device="cuda")
    mag = torch.tensor(np.ascontiguousarray(X[:, 12]), device="cuda")
    pl = torch.zeros((S, T + 1), dtype=tdt, device="cuda")
    st = torch.zeros(S, dtype=torch.int32, device="cuda")
    D.solve_pl_device(mat, lens[0], Time, 128, T, torch.tensor(np.ascontiguousarray(ini[0]), device="cuda"), pl, status=st)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    st[3] = 7                                                        # a row the solve would have flagged at step 6
    rng = np.random.default_rng(2)
    plh = pl.cpu().numpy()
    lg = np.log10(plh.astype(np.float64))
    if dtype == "float32":
        lg = lg.astype(np.float32).astype(np.float64)               # the reference's float32 buffer (bayeslib.py:137)
    if offgrid:
        t = np.sort(rng.uniform(0.0, Time, 270))
        hi, dx, h = bracket_times(np.linspace(0, Time, T + 1), t)
        obs = 18.0 - 0.2 * t
        dy = lg[:, hi] - lg[:, hi - 1]
        if dtype == "float32":
            dy = (lg[:, hi].astype(np.float32) - lg[:, hi - 1].astype(np.float32)).astype(np.float64)
        y = (dy / h) * dx + lg[:, hi - 1]
        br = dict(obs_hi=torch.tensor(hi.astype(np.int32), device="cuda"), obs_dx=torch.tensor(dx, device="cuda"),
                  obs_h=torch.tensor(h, device="cuda"))
    else:
        obs = 18.0 - 0.2 * DT * np.arange(T + 1)
        y, br = lg, {}
    e = (y + X[:, 12:13]) - obs[None, :]
    n = e.shape[1]
    tobs = torch.tensor(obs, device="cuda")
    res = {}
    for name in ("plain", "moments"):
        P = torch.full((S,), 3.0, dtype=torch.float64, device="cuda")
        sse = torch.zeros(S, dtype=torch.float64, device="cuda")
        if name == "plain":
            D.loglik_from_pl_device(pl, tobs, mag, P=P, sse=sse, status=st, **br)
        else:
            es = torch.zeros(S, dtype=torch.float64, device="cuda")
            D.loglik_moments_from_pl_device(pl, tobs, mag, P=P, sse=sse, esum=es, status=st, **br)
        torch.cuda.synchronize()
        res[name] = (P.cpu().numpy(), sse.cpu().numpy())
    assert np.array_equal(res["plain"][0], res["moments"][0]) and np.array_equal(res["plain"][1], res["moments"][1])
    es = es.cpu().numpy()
    live = np.arange(S) != 3
    assert np.isnan(es[3]) and np.isinf(res["moments"][1][3]) and res["moments"][0][3] == -np.inf
    bound = (-(-n // 256) + 9) * EPS * np.abs(e).sum(axis=1)
    if dtype == "float64":
        bound = bound + 2 * EPS * np.abs(lg).max() * n               # the device's log10 against NumPy's: 1 ulp per term
    err = np.abs(es - e.sum(axis=1))
    print("%s %s: esum worst error / bound %.3g" % (dtype, "offgrid" if offgrid else "ongrid", float((err[live] / bound[live]).max())))
    assert (err[live] <= bound[live]).all()


@pytest.mark.parametrize("mode", ["single", "pair"])
def test_a_sample_that_does_not_converge_is_nan_and_leaves_its_partner_alone(gpu, mode):
    """The ordinary flagged-system path (pvSimPCR.py:269: the iteration cap is reached): max_iter is lowered until some, not
    all, samples of an ordinary batch run into it; those get esum = NaN, sse = +inf, P = -inf at every offset, best = NaN, and
    every other system -- a flagged one's wavefront partner included (adjacent samples share a wavefront) -- keeps the bits it
    has in a batch where nothing is flagged."""
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 12, 70
    X = w.samples(S, seed=23)
    obs = [18.0 - 0.2 * DT * np.arange(T + 1) for _ in range(3)]
    kw = dict(MODES[mode], extra_flags=gpu._abi.FLAG_PAIR_ADJACENT)
    clean = {}
    gpu.loglik(X, ini, lens, T * DT, 128, T, obs, info=clean, mag_grid=OFFSETS, **kw)
    assert not clean["status"].any()
    for MAX in (8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512):
        info = {}
        P = gpu.loglik(X, ini, lens, T * DT, 128, T, obs, info=info, mag_grid=OFFSETS, MAX=MAX, **kw)
        bad = info["status"] != 0
        partner = np.zeros_like(bad)                               # adjacent samples 2p, 2p + 1 of one curve share a wavefront
        partner[:, 0::2], partner[:, 1::2] = bad[:, 1::2], bad[:, 0::2]
        if bad.any() and (partner & ~bad).any():                   # some flagged, and one of them beside a live system
            break
    else:
        pytest.fail("no iteration cap flags a system beside a live wavefront partner in this batch")
    assert np.isnan(info["esum"][bad]).all() and np.isinf(info["sse"][bad]).all()
    assert np.array_equal(info["esum"][~bad], clean["esum"][~bad]) and np.array_equal(info["sse"][~bad], clean["sse"][~bad])
    print("MAX = %d: %d of %d systems flagged, %d live wavefront partners" % (MAX, bad.sum(), bad.size, (partner & ~bad).sum()))
    dead = bad.any(axis=0)
    assert (P[:, dead] == -np.inf).all() and np.isfinite(P[:, ~dead]).all()
    best, Pp = gpu.loglik(X, ini, lens, T * DT, 128, T, obs, mag_profile=True, MAX=MAX, **kw)
    assert np.isnan(best[dead]).all() and (Pp[dead] == -np.inf).all() and np.isfinite(best[~dead]).all()


# ------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
def test_esum_bits_do_not_depend_on_the_launch_cut_or_the_pairing_rule(gpu, predict):
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 10, 130
    X = w.samples(S, seed=31)
    obs = [18.0 - 0.2 * DT * np.arange(T + 1) for _ in range(3)]
    def run(Xs, **kw):
        info = {}
        gpu.loglik(Xs, ini, lens, T * DT, 128, T, obs, info=info, mag_grid=[0.0], kernel="pair", predict=predict, **kw)
        return info["esum"], info["sse"]
    e0, s0 = run(X)
    for es, ss in (run(X, extra_flags=gpu._abi.FLAG_PAIR_ADJACENT), run(X, extra_flags=gpu._abi.FLAG_PAIR_ALWAYS_SEAM)):
        assert np.array_equal(es, e0) and np.array_equal(ss, s0)
    e_odd, s_odd = run(X[:7])                                       # odd S: the last wavefront holds one system twice
    assert np.array_equal(e_odd, e0[:, :7]) and np.array_equal(s_odd, s0[:, :7])
    e_sh, s_sh = run(X[3:8])                                        # a shard of the batch
    assert np.array_equal(e_sh, e0[:, 3:8]) and np.array_equal(s_sh, s0[:, 3:8])


# ------------------------------------------------------------------------------------------------------- 8
def _e2e(g):
    T, tg, npre = int(g["T"]), g["tgrid"], int(g["npre"])
    e_data = [([tg] * 3, list(g["obs0"]), [None] * 3), ([tg[:npre]] * 3, list(g["obs1"]), [None] * 3)]
    flags = {"load_PL_from_file": False, "override_equal_auger": False, "override_equal_mu": False, "override_equal_s": False,
             "log_pl": True, "self_normalize": False, "random_sample": True, "num_points": int(g["X"].shape[0])}
    return T, e_data, flags


@pytest.mark.parametrize("n_exp", [2, 1], ids=["resident_pl", "single_experiment"])
def test_bayes_with_a_mag_grid_equals_plain_runs_at_the_shifted_offsets(gpu, golden, n_exp):
    """driver.bayes with gpu_info["mag_grid"] on bayes_e2e.npz's inputs (two experiments: the resident-PL level; one: the
    fused single-experiment level): block m of P equals a plain run with offsets[m] added to minX / maxX[12], within the first
    bound (FAST depth; sum|e_i| from the solved PL); X is (M S, 13) in the GUI's wire format; mag_grid = None changes nothing."""
    g = golden("bayes_e2e")
    T, e_data, flags = _e2e(g)
    e_data = e_data[:n_exp]
    ini, Time = g["ini"], float(g["time"])
    simPar = [float(g["length"]), Time, 128, T, 1, (0,), 7, 10000]
    offsets = np.array([-1.25, 0.0, 0.5])
    base = dict(num_gpus=1, has_GPU=True, max_sims_per_block=1, sims_per_gpu=4, fused=True, pl_dtype=np.float64)
    def run(minX, maxX, **kw):
        return gpu.bayes(gpu.pvSim, None, None, minX, maxX, g["do_log"], ini, list(simPar), e_data, dict(flags),
                         dict(base, **kw), rng=np.random.RandomState(42))
    _, P0, X0 = run(g["minX"], g["maxX"])
    _, Pn, Xn = run(g["minX"], g["maxX"], mag_grid=None)
    assert np.array_equal(P0, Pn) and np.array_equal(X0, Xn)
    S = len(X0)
    _, Pg, Xg = run(g["minX"], g["maxX"], mag_grid=offsets)
    assert Pg.shape == (n_exp, 3 * S) and Xg.shape == (3 * S, 13)
    worst = 0.0
    for m, d in enumerate(offsets):
        lo, hi = g["minX"].copy(), g["maxX"].copy()
        lo[12] += d; hi[12] += d
        _, Pd, Xd = run(lo, hi)
        assert np.array_equal(Xd[:, :12], X0[:, :12]) and np.array_equal(Xg[m * S:(m + 1) * S, :12], X0[:, :12])
        assert np.array_equal(Xg[m * S:(m + 1) * S, 12], X0[:, 12] + d)
        for e in range(n_exp):
            bound = np.zeros(S)
            for c in range(3):
                n = len(e_data[e][1][c])
                pl = gpu.solve_pl(X0[:, :12], simPar[0], Time, 128, T, ini[c])[0][:, :n]
                err = np.log10(pl) + X0[:, 12:13] - np.asarray(e_data[e][1][c])[None, :]
                A_d = (err * err).sum(axis=1) + 2 * np.abs(d * err.sum(axis=1)) + n * d * d
                bound += (6 + -(-n // 64) + 4) * EPS * (A_d + abs(d) * np.abs(err).sum(axis=1))
            diff = np.abs(Pg[e, m * S:(m + 1) * S] - Pd[e])
            worst = max(worst, float((diff / bound).max()))
            assert (diff <= bound).all(), (e, d, float((diff / bound).max()))
    print("n_exp = %d: worst |P_grid - P_plain| / bound = %.3g" % (n_exp, worst))
    if n_exp == 2:                                  # the fixed-sample form of the golden: simulate() on g["X"], as today
        P = np.zeros((2, len(g["X"]))); z = np.zeros(1)
        gpu.simulate(gpu.pvSim, e_data, P, g["X"], [None], [None], 3, list(simPar), ini, flags,
                     {"sims_per_gpu": 4, "num_gpus": 1, "fused": True, "mag_grid": None}, 0, z.copy(), z.copy(), z.copy())
        assert np.max(np.abs(P - g["P"]) / np.abs(g["P"])) < 2e-5
    for bad, word in ((dict(devices=[0]), "devices"), (dict(fused=False), "fused"), (dict(num_gpus=2), "num_gpus")):
        with pytest.raises(ValueError) as ei:
            run(g["minX"], g["maxX"], mag_grid=offsets, **bad)
        assert word in str(ei.value)


# ------------------------------------------------------------------------------------------------------- the eight mag exports
@pytest.mark.parametrize("C", [1, 2, 64])
@pytest.mark.parametrize("S", [1, 257])
def test_mag_exports_route_counts_and_weight_sums_to_the_same_arithmetic(gpu, S, C):
    """trpl_mag_grid / trpl_mag_profile: the host form, the _dev form, and the _w forms given wsum = n_obs.astype(float64) return
    the same bits -- the grid at M = 1, 256 and 257 (the second launch starts at offset 256), the profile with and without
    TRPL_MAG_PER_CURVE.  The kernels themselves are pinned by test_gpu_likelihood_instances.py; this pins that each of the eight
    exports reaches the arithmetic of its name with the per-curve vector converted exactly."""
    import torch

    import likelihood_ref as R
    a, lib = gpu._abi, gpu._abi.lib()
    m = R.mag_moments(S, C, False)
    vec = {"": m["n"], "_w": m["n"].astype(np.float64)}
    assert m["n"].dtype == np.int64
    dsse, desum = torch.from_numpy(m["sse"]).cuda(), torch.from_numpy(m["esum"]).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def run(name, sfx, on_device, mid, outs):
        """outs: host arrays holding the start values; returns what the export leaves in them."""
        got = [o.copy() for o in outs]
        if on_device:
            dev = [torch.from_numpy(o).cuda() for o in got]
            a.check(getattr(lib, "%s%s_dev" % (name, sfx))(dsse.data_ptr(), desum.data_ptr(), a.ptr(vec[sfx]), S, C, *mid,
                                                           *[d.data_ptr() for d in dev], stream))
            torch.cuda.synchronize()
            return [d.cpu().numpy() for d in dev]
        a.check(getattr(lib, name + sfx)(a.ptr(m["sse"]), a.ptr(m["esum"]), a.ptr(vec[sfx]), S, C, *mid, *[a.ptr(o) for o in got]))
        return got

    forms = [(sfx, dev) for sfx in ("", "_w") for dev in (False, True)]
    for M in (1, 256, 257):
        offsets = R.mag_offsets(M)
        res = [run("trpl_mag_grid", sfx, dev, (a.ptr(offsets), M), [np.tile(m["P0"], (M, 1))]) for sfx, dev in forms]
        assert S == 1 or not np.array_equal(res[0][0], np.tile(m["P0"], (M, 1)))
        for r, form in zip(res[1:], forms[1:]):
            assert np.array_equal(r[0], res[0][0]), (M, form)
    for per_curve in (False, True):
        start = [np.full((C, S) if per_curve else S, 5.0), m["P0"]]
        res = [run("trpl_mag_profile", sfx, dev, (a.MAG_PER_CURVE if per_curve else 0,), start) for sfx, dev in forms]
        assert S == 1 or not np.array_equal(res[0][1], m["P0"])
        for r, form in zip(res[1:], forms[1:]):
            assert np.array_equal(r[0], res[0][0], equal_nan=True) and np.array_equal(r[1], res[0][1]), (per_curve, form)
