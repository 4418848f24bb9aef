"""TRPL_FLAG_WEIGHTED on the GPU (include/trpl.h: trpl_loglik_weighted, trpl_loglik_weighted_from_pl_dev,
trpl_sse_accumulate_w, trpl_mag_grid_w, trpl_mag_profile_w): the weighting line the reference has commented out
(probs.py:40) inside the stepper's sink -- sse = sum w e^2, esum = sum w e.

Exact statements are asserted exactly (array_equal): unit weights are the moments call, a power-of-two weight scales it, a
zero weight removes the observation, the weights never touch the solve, the bits depend neither on the launch cut nor on the
wavefront partner.  Tolerances are derived as in tests/test_gpu_moments.py's header, not measured (eps = 2^-52):
  * sums of given terms: k eps sum w e^2 (k eps sum w |e| for esum), k = the depth of the summation + 6 -- FAST 6 levels
    inside a 64-column batch + ceil(n / 64) batches added serially, STRICT the serial sum of n terms; + 6: the moments bound's
    roundings with two more for the weight;
  * where the PL the errors are formed from is not the same bits (FAST: the kernel that stores PL is another instantiation
    than the weighted likelihood kernel; the header's envelope |d lg| <= 1e-9 / ln 10 = 4.4e-10 per column holds between any
    two FAST evaluations): + 2 sqrt(wsum sse) 4.4e-10 on sse (Cauchy-Schwarz on sum 2 w |e| |d lg|) and wsum 4.4e-10 on esum;
    STRICT PL is bit-identical between instantiations and takes no such term;
  * the stored-PL kernel sums ceil(n / 256) terms serially per thread, 6 shuffle levels and 3 adds: depth ceil(n / 256) + 9.
All inputs sit far above the cancellation floor: floor_col == -1 is asserted, no system is left out of a comparison."""
import math
import os

import numpy as np
import pytest

from gpu_common import DT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
ENV = 4.4e-10
MODES = {"strict": dict(strict=True), "single": dict(kernel="single"), "pair": dict(kernel="pair")}
GRID = [pytest.param(m, p, o, id="%s-%s-%s" % (m, "predict" if p else "default", "offgrid" if o else "ongrid"))
        for m in MODES for p in (False, True) for o in (False, True)]


def _depth(n, strict):
    return (n if strict else 6 + -(-n // 64)) + 6


def _case(gpu, offgrid, S=9, T=150, seed=11):
    """Odd S (the paired kernel's duplicated tail), three 64-column batches, three curves of different n_obs."""
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    Time = T * DT
    X = w.samples(S, seed=seed)
    rng = np.random.default_rng(5)
    if offgrid:
        times = [np.sort(rng.uniform(0.0, Time, 140 + 7 * c)) for c in range(3)]
        obs = [18.0 - 0.2 * t + 0.05 * rng.standard_normal(len(t)) for t in times]
    else:
        times = None
        obs = [18.0 - 0.2 * DT * np.arange(T + 1 - 3 * c) for c in range(3)]      # 151, 148, 145 columns
    return dict(args=(X, ini, lens, Time, 128, T, obs), times=times, S=S, n=[len(o) for o in obs], rng=rng)


def _run(gpu, case, mode, predict, weights=None, **kw):
    info = {}
    if weights is None:
        gpu.loglik(*case["args"], info=info, mag_grid=[0.0], times=case["times"], predict=predict, **MODES[mode], **kw)
    else:
        P = gpu.loglik(*case["args"], info=info, weights=weights, times=case["times"], predict=predict, **MODES[mode], **kw)
        assert P is info["P"]
    return info


def _same_solve(a, b):
    for k in ("status", "iters_total", "floor_col"):
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------- 1, 2, 3
@pytest.mark.parametrize("mode,predict,offgrid", GRID)
def test_unit_weights_are_the_moments_call_and_a_power_of_two_scales_it(gpu, mode, predict, offgrid):
    case = _case(gpu, offgrid)
    mom = _run(gpu, case, mode, predict)
    assert not mom["status"].any()
    one = _run(gpu, case, mode, predict, weights=[np.ones(n) for n in case["n"]])
    for k in ("sse", "esum", "P"):
        assert np.array_equal(one[k], mom[k]), k
    _same_solve(one, mom)
    assert np.array_equal(one["wsum"], np.array(case["n"], dtype=float))
    quarter = _run(gpu, case, mode, predict, weights=[np.full(n, 0.25) for n in case["n"]])
    assert np.array_equal(quarter["sse"], 0.25 * mom["sse"]) and np.array_equal(quarter["esum"], 0.25 * mom["esum"])
    _same_solve(quarter, mom)
    # random positive weights per curve: the weights never touch the solve
    plain = {}
    gpu.loglik(*case["args"], info=plain, times=case["times"], predict=predict, **MODES[mode])
    rnd = _run(gpu, case, mode, predict, weights=[case["rng"].uniform(0.1, 10.0, n) for n in case["n"]])
    _same_solve(rnd, plain)
    assert np.isfinite(rnd["sse"]).all() and not np.array_equal(rnd["sse"], mom["sse"])


@pytest.mark.parametrize("L,mode,predict", [(32, "strict", False), (32, "single", True), (512, "single", False), (512, "single", True)])
def test_unit_weights_at_the_small_and_the_large_grid(gpu, L, mode, predict):
    w = gpu.workloads
    ini, lens = w.power_scan(L)
    S, T = 4, 100
    X = w.samples(S, seed=12)
    obs = [18.0 - 0.2 * DT * np.arange(T + 1) for _ in range(3)]
    mom, one = {}, {}
    kw = dict(MODES[mode], predict=predict)
    gpu.loglik(X, ini, lens, T * DT, L, T, obs, info=mom, mag_grid=[0.0], **kw)
    gpu.loglik(X, ini, lens, T * DT, L, T, obs, info=one, weights=[np.ones(T + 1)] * 3, **kw)
    for k in ("sse", "esum", "P", "status", "iters_total", "floor_col"):
        assert np.array_equal(one[k], mom[k]), k


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("mode,predict", [("pair", False), ("single", True), ("strict", False)])
def test_device_resident_unit_weights_equal_the_device_resident_moments_call(gpu, mode, predict, offgrid):
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
    kw = {}
    if offgrid:
        t = np.sort(np.random.default_rng(8).uniform(0.0, Time, 120))
        hi, dx, h = bracket_times(np.linspace(0, Time, T + 1), t)
        obs = torch.tensor(np.stack([18.0 - 0.2 * t] * 3), device="cuda")
        br = [torch.tensor(np.ascontiguousarray(np.stack([a] * 3)), device="cuda") for a in (hi.astype(np.int32), dx, h)]
        kw, n_obs = dict(obs_hi=br[0], obs_dx=br[1], obs_h=br[2]), 120
    else:
        obs = torch.tensor(np.stack([18.0 - 0.2 * DT * np.arange(T + 1)] * 3), device="cuda")
        n_obs = T + 1
    out = {}
    for name in ("moments", "weighted"):
        P = torch.zeros(S, dtype=torch.float64, device="cuda")
        sse, es = (torch.zeros((3, S), dtype=torch.float64, device="cuda") for _ in range(2))
        st = torch.zeros((3, S), dtype=torch.int32, device="cuda")
        it = torch.zeros((3, S), dtype=torch.int64, device="cuda")
        fl = torch.zeros((3, S), dtype=torch.int32, device="cuda")
        if name == "moments":
            D.loglik_moments_device(X, tini, lens, Time, 128, T, obs, n_obs, P, sse, es, st, it, flags=flags, floor_col=fl, **kw)
        else:
            D.loglik_weighted_device(X, tini, lens, Time, 128, T, obs, torch.ones_like(obs), n_obs, P, sse, es, st, it,
                                     flags=flags, floor_col=fl, **kw)
        torch.cuda.synchronize()
        out[name] = [t_.cpu().numpy() for t_ in (P, sse, es, st, it, fl)]
    assert not out["moments"][3].any() and np.isfinite(out["moments"][2]).all()
    for a, b in zip(out["moments"], out["weighted"]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
@pytest.mark.parametrize("mode", list(MODES))
def test_a_zero_weight_is_an_absent_observation(gpu, mode, predict):
    case = _case(gpu, False)
    X, ini, lens, Time, L, T, obs = case["args"]
    keep = [100, 64, 131]                                 # inside a batch, on a batch boundary, in the last batch
    wts = [np.where(np.arange(n) < k, 1.0, 0.0) for n, k in zip(case["n"], keep)]
    got = _run(gpu, case, mode, predict, weights=wts)
    short = dict(case, args=(X, ini, lens, Time, L, T, [o[:k] for o, k in zip(obs, keep)]))
    want = _run(gpu, short, mode, predict)
    assert not got["status"].any() and not want["status"].any()
    assert np.array_equal(got["sse"], want["sse"]) and np.array_equal(got["esum"], want["esum"])
    assert np.array_equal(got["wsum"], np.array(keep, dtype=float))


# ------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("mode,predict,offgrid", GRID)
def test_weighted_sums_against_numpy_within_the_derived_bound(gpu, mode, predict, offgrid):
    from trpl_amd.driver import bracket_times
    case = _case(gpu, offgrid, seed=17)
    X, ini, lens, Time, L, T, _ = case["args"]
    strict = mode == "strict"
    rng = np.random.default_rng(3)
    lg = []
    for c in range(3):                                    # the PL of the same systems, the same kernel pinned
        pl, st, _, _ = gpu.solve_pl(X[:, :12], lens[c], Time, L, T, ini[c], predict=predict, **MODES[mode])
        assert not st.any() and (pl > 0).all()
        lg.append(np.log10(pl))
    sim_t = np.linspace(0, Time, T + 1)
    ys, obs, times, wts = [], [], [] if offgrid else None, []
    for c, n in enumerate(case["n"]):
        if offgrid:
            t = np.sort(rng.uniform(0.0, Time, n))
            hi, dx, h = bracket_times(sim_t, t)
            y = ((lg[c][:, hi] - lg[c][:, hi - 1]) / h) * dx + lg[c][:, hi - 1]
            times.append(t)
        else:
            y = lg[c][:, :n]
        ys.append(y)
        # observations a decade below every simulated curve: errors of order 1 and more, nothing near a cancellation
        obs.append(np.min(y + X[:, 12:13], axis=0) - 1.0 + 0.1 * rng.standard_normal(n))
        wts.append(10.0 ** rng.uniform(-1.5, 1.5, n))     # three decades
    info = {}
    gpu.loglik(X, ini, lens, Time, L, T, obs, info=info, weights=wts, times=times, predict=predict, **MODES[mode])
    assert not info["status"].any() and (info["floor_col"] == -1).all()                 # no system excluded
    worst = 0.0
    for c, n in enumerate(case["n"]):
        e = (ys[c] + X[:, 12:13]) - obs[c][None, :]
        assert np.abs(e).min() > 0.1
        w = wts[c][None, :]
        sse_np = np.array([math.fsum(r) for r in (e * e) * w])
        esum_np = np.array([math.fsum(r) for r in e * w])
        k = _depth(n, strict)
        b2 = k * EPS * sse_np
        b1 = k * EPS * np.array([math.fsum(r) for r in np.abs(e) * w])
        if not strict:
            b2 = b2 + 2 * np.sqrt(info["wsum"][c] * sse_np) * ENV
            b1 = b1 + info["wsum"][c] * ENV
        d2, d1 = np.abs(info["sse"][c] - sse_np), np.abs(info["esum"][c] - esum_np)
        worst = max(worst, float((d2 / b2).max()), float((d1 / b1).max()))
        print("curve %d n %d k %d: sse err/bound %.3g (depth term alone %.3g), esum err/bound %.3g" % (
            c, n, k, float((d2 / b2).max()), float((d2 / (k * EPS * sse_np)).max()), float((d1 / b1).max())))
        assert (d2 <= b2).all() and (d1 <= b1).all(), (mode, c)
    assert np.array_equal(info["wsum"], np.array([math.fsum(w) for w in wts]))
    acc = np.zeros(case["S"])
    for c in range(3):
        acc = acc + (0.0 - info["sse"][c])
    assert np.array_equal(info["P"], acc)                 # P[s] -= sum_c sse[c][s], curves in order


# ------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
def test_bits_do_not_depend_on_the_launch_cut_or_the_pairing_rule(gpu, predict):
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 10, 130
    X = w.samples(S, seed=31)
    obs = [18.0 - 0.2 * DT * np.arange(T + 1) for _ in range(3)]
    rng = np.random.default_rng(6)
    wts = [rng.uniform(0.0, 4.0, T + 1) for _ in range(3)]                              # per-curve different weights
    def run(Xs, **kw):
        info = {}
        gpu.loglik(Xs, ini, lens, T * DT, 128, T, obs, info=info, weights=wts, kernel="pair", predict=predict, **kw)
        return info["esum"], info["sse"]
    e0, s0 = run(X)
    assert np.isfinite(e0).all() and np.isfinite(s0).all()
    for es, ss in (run(X, extra_flags=gpu._abi.FLAG_PAIR_ADJACENT), run(X, extra_flags=gpu._abi.FLAG_PAIR_ALWAYS_SEAM)):
        assert np.array_equal(es, e0) and np.array_equal(ss, s0)
    e_odd, s_odd = run(X[:7])                                       # odd S: the last wavefront holds one system twice
    assert np.array_equal(e_odd, e0[:, :7]) and np.array_equal(s_odd, s0[:, :7])
    e_sh, s_sh = run(X[3:8])                                        # a shard of the batch
    assert np.array_equal(e_sh, e0[:, 3:8]) and np.array_equal(s_sh, s0[:, 3:8])


# ------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("mode", ["single", "pair"])
def test_a_sample_that_does_not_converge_is_flagged_and_leaves_its_partner_alone(gpu, mode):
    """The ordinary flagged-system path (pvSimPCR.py:269: the iteration cap is reached), found as tests/test_gpu_moments.py
    finds it: max_iter is lowered until some, not all, samples of an ordinary batch run into it."""
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 12, 70
    X = w.samples(S, seed=23)
    obs = [18.0 - 0.2 * DT * np.arange(T + 1) for _ in range(3)]
    wts = [np.random.default_rng(c).uniform(0.5, 2.0, T + 1) for c in range(3)]
    kw = dict(MODES[mode], extra_flags=gpu._abi.FLAG_PAIR_ADJACENT, weights=wts)
    clean = {}
    gpu.loglik(X, ini, lens, T * DT, 128, T, obs, info=clean, **kw)
    assert not clean["status"].any()
    for MAX in (8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512):
        info = {}
        P = gpu.loglik(X, ini, lens, T * DT, 128, T, obs, info=info, MAX=MAX, **kw)
        bad = info["status"] != 0
        partner = np.zeros_like(bad)                               # adjacent samples 2p, 2p + 1 of one curve share a wavefront
        partner[:, 0::2], partner[:, 1::2] = bad[:, 1::2], bad[:, 0::2]
        if bad.any() and (partner & ~bad).any():
            break
    else:
        pytest.fail("no iteration cap flags a system beside a live wavefront partner in this batch")
    assert np.isnan(info["esum"][bad]).all() and (info["sse"][bad] == np.inf).all()
    assert np.array_equal(info["esum"][~bad], clean["esum"][~bad]) and np.array_equal(info["sse"][~bad], clean["sse"][~bad])
    dead = bad.any(axis=0)
    assert (P[dead] == -np.inf).all() and np.isfinite(P[~dead]).all()
    Pg = gpu.loglik(X, ini, lens, T * DT, 128, T, obs, MAX=MAX, mag_grid=[-0.5, 0.5], **kw)
    assert (Pg[:, dead] == -np.inf).all() and np.isfinite(Pg[:, ~dead]).all()


# ------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_weighted_from_stored_pl(gpu, dtype, offgrid):
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
    lg = np.log10(pl.cpu().numpy().astype(np.float64))
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
    wts = 10.0 ** rng.uniform(-1.5, 1.5, n)

    def call(weights):
        P = torch.full((S,), 3.0, dtype=torch.float64, device="cuda")
        sse, es = (torch.zeros(S, dtype=torch.float64, device="cuda") for _ in range(2))
        if weights is None:
            D.loglik_moments_from_pl_device(pl, tobs, mag, P=P, sse=sse, esum=es, status=st, **br)
        else:
            D.loglik_weighted_from_pl_device(pl, tobs, torch.tensor(weights, device="cuda"), mag, P=P, sse=sse, esum=es,
                                             status=st, **br)
        torch.cuda.synchronize()
        return P.cpu().numpy(), sse.cpu().numpy(), es.cpu().numpy()

    mom, one = call(None), call(np.ones(n))
    for a, b in zip(mom, one):                                       # unit weights: the moments form, bit for bit
        assert np.array_equal(a, b, equal_nan=True)
    P, sse, es = call(wts)
    live = np.arange(S) != 3
    assert np.isnan(es[3]) and sse[3] == np.inf and P[3] == -np.inf
    assert np.array_equal(P[live], 3.0 - sse[live])
    k = -(-n // 256) + 9 + 2
    sse_np = np.array([math.fsum(r) for r in (e * e) * wts])            # exactly rounded: the reference adds no error of its own
    b2 = k * EPS * sse_np
    b1 = k * EPS * (np.abs(e) * wts).sum(axis=1)
    if dtype == "float64":                                           # the device's log10 against NumPy's: 1 ulp per term
        b2 = b2 + 2 * np.sqrt(wts.sum() * sse_np) * EPS * np.abs(lg).max()
        b1 = b1 + wts.sum() * EPS * np.abs(lg).max()
    d2, d1 = np.abs(sse - sse_np), np.abs(es - np.array([math.fsum(r) for r in e * wts]))
    print("%s %s: sse err/bound %.3g, esum err/bound %.3g" % (dtype, "offgrid" if offgrid else "ongrid",
                                                              float((d2[live] / b2[live]).max()), float((d1[live] / b1[live]).max())))
    assert (d2[live] <= b2[live]).all() and (d1[live] <= b1[live]).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("rows", [5, 300])
def test_sse_accumulate_w_equals_the_serial_loop(gpu, dtype, rows):
    """trpl_sse_accumulate_w[_dev]: P[j] -= sum_i ((pl + mag - v)^2 * w), fp64, index order -- array_equal to the same loop in
    NumPy; through likelihood.prob(weighted=True) and through the device wrapper."""
    import torch
    from trpl_amd import device as D
    rng = np.random.default_rng(rows)
    n = 333
    pl = rng.uniform(-3.0, 3.0, (rows, n)).astype(dtype)
    v, mag, u = rng.uniform(-3.0, 3.0, n), rng.uniform(-1.0, 1.0, rows), 10.0 ** rng.uniform(-2.0, 0.0, n)
    wts = gpu.likelihood.weights_from_uncertainty(u)
    acc = np.zeros(rows)
    for i in range(n):
        e = pl[:, i].astype(np.float64) + mag
        e = e - v[i]
        acc = acc + (e * e) * wts[i]
    want = 2.0 + (0.0 - acc)
    P = np.full(rows, 2.0)
    gpu.likelihood.prob(P, pl, v, u, mag, weighted=True)
    assert np.array_equal(P, want)
    Pd = torch.full((rows,), 2.0, dtype=torch.float64, device="cuda")
    D.sse_accumulate_w_device(Pd, torch.tensor(pl, device="cuda"), torch.tensor(v, device="cuda"),
                              torch.tensor(wts, device="cuda"), torch.tensor(mag, device="cuda"))
    torch.cuda.synchronize()
    assert np.array_equal(Pd.cpu().numpy(), want)
    P1, P0 = np.full(rows, 2.0), np.full(rows, 2.0)                  # default: the uncertainty is still ignored
    gpu.likelihood.prob(P1, pl, v, u, mag)
    gpu.likelihood.prob(P0, pl, v, None, mag)
    assert np.array_equal(P1, P0) and not np.array_equal(P1, want)


# ------------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize("mode", list(MODES))
def test_weighted_mag_grid_and_profile(gpu, mode):
    import torch
    from trpl_amd import device as D
    case = _case(gpu, False, S=5)
    X = case["args"][0]
    strict = mode == "strict"
    rng = np.random.default_rng(12)
    wts = [10.0 ** rng.uniform(-1.0, 1.0, n) for n in case["n"]]
    offsets = np.linspace(-1.5, 1.5, 7)
    kw = dict(MODES[mode], weights=wts)
    info = {}
    Pg = gpu.loglik(*case["args"], info=info, mag_grid=offsets, **kw)
    assert not info["status"].any() and (info["floor_col"] == -1).all()
    sse, esum, wsum = info["sse"], info["esum"], info["wsum"]
    # sum w |e| never leaves the kernel: from the PL of the same systems (agrees with the kernel's to 1e-9)
    swe = np.zeros_like(sse)
    for c, n in enumerate(case["n"]):
        pl = gpu.solve_pl(X[:, :12], case["args"][2][c], case["args"][3], 128, case["args"][5], case["args"][1][c])[0][:, :n]
        swe[c] = (np.abs(np.log10(pl) + X[:, 12:13] - case["args"][6][c][None, :]) * wts[c]).sum(axis=1)
    worst = 0.0
    for m, d in enumerate(offsets):
        Xd = X.copy()
        Xd[:, 12] = Xd[:, 12] + d
        Pd = gpu.loglik(Xd, *case["args"][1:], **kw)                                  # a direct weighted call at the offset
        bound = np.zeros(case["S"])
        for c, n in enumerate(case["n"]):
            A_d = sse[c] + 2 * np.abs(d * esum[c]) + wsum[c] * d * d
            bound += _depth(n, strict) * EPS * (A_d + abs(d) * swe[c] * (1 + 1e-6))
        err = np.abs(Pg[m] - Pd)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (mode, d, float((err / bound).max()))
    print("%s: worst |P_grid - P_direct| / bound = %.3g" % (mode, worst))
    best, Pp = gpu.loglik(*case["args"], mag_profile=True, **kw)
    for s in range(case["S"]):                                                          # the profile IS the grid at best
        assert gpu.loglik(*case["args"], mag_grid=[best[s]], **kw)[0, s] == Pp[s]
    fine = gpu.loglik(*case["args"], mag_grid=np.linspace(-2.0, 2.0, 81), **kw)
    assert (Pp >= fine.max(axis=0) - 64 * EPS * np.abs(Pp)).all()                      # and best minimises
    E, W = np.zeros(case["S"]), 0.0
    for c in range(3):
        E, W = E + esum[c], W + wsum[c]
    assert np.array_equal(best, (0.0 - E) / W)
    ts, te = torch.tensor(sse, device="cuda"), torch.tensor(esum, device="cuda")       # the kernels equal the host forms
    Pdv = torch.zeros((len(offsets), case["S"]), dtype=torch.float64, device="cuda")
    D.mag_grid_w_device(ts, te, wsum, offsets, Pdv)
    assert np.array_equal(Pdv.cpu().numpy(), Pg)
    for per_curve in (False, True):
        bh, Ph = gpu.loglik(*case["args"], mag_profile="per_curve" if per_curve else True, **kw)
        bd = torch.zeros((3, case["S"]) if per_curve else (case["S"],), dtype=torch.float64, device="cuda")
        Pd_ = torch.zeros(case["S"], dtype=torch.float64, device="cuda")
        D.mag_profile_w_device(ts, te, wsum, bd, Pd_, per_curve=per_curve)
        assert np.array_equal(bd.cpu().numpy(), bh) and np.array_equal(Pd_.cpu().numpy(), Ph)


# ------------------------------------------------------------------------------------------------------- 10
def _e2e(g):
    """bayes_e2e.npz's two experiments with an uncertainty column: a relative sigma that grows along the decay, as a constant
    absolute sigma gives (bayes_io.py:75-76)."""
    T, tg, npre = int(g["T"]), g["tgrid"], int(g["npre"])
    u0 = [0.02 * 10.0 ** (0.03 * np.arange(len(tg)) + 0.1 * c) for c in range(3)]
    e_data = [([tg] * 3, list(g["obs0"]), u0), ([tg[:npre]] * 3, list(g["obs1"]), [1.5 * u[:npre] for u in u0])]
    flags = {"load_PL_from_file": False, "override_equal_auger": False, "override_equal_mu": False, "override_equal_s": False,
             "log_pl": True, "self_normalize": False, "random_sample": True, "num_points": int(g["X"].shape[0])}
    return T, e_data, flags


@pytest.mark.parametrize("n_exp", [1, 2], ids=["single_experiment", "resident_pl"])
def test_bayes_weighted_on_every_level(gpu, golden, n_exp):
    g = golden("bayes_e2e")
    T, e_data, flags = _e2e(g)
    e_data = e_data[:n_exp]
    ini, Time = g["ini"], float(g["time"])
    simPar = [float(g["length"]), Time, 128, T, 1, (0,), 7, 10000]
    base = dict(num_gpus=1, has_GPU=True, max_sims_per_block=1, sims_per_gpu=4, pl_dtype=np.float64)

    def run(**kw):
        return gpu.bayes(gpu.pvSim, None, None, g["minX"], g["maxX"], g["do_log"], ini, list(simPar), e_data, dict(flags),
                         dict(base, **kw), rng=np.random.RandomState(42))
    _, P0, X0 = run(fused=True)
    _, Pn, Xn = run(fused=True, weighted=False)
    assert np.array_equal(P0, Pn) and np.array_equal(X0, Xn)                            # off: nothing changes
    _, Pw, Xw = run(fused=True, weighted=True)
    _, Pu, Xu = run(fused=False, weighted=True)
    assert np.array_equal(Xw, X0) and np.array_equal(Xu, X0)
    assert np.isfinite(Pw).all() and not np.allclose(Pw, P0, rtol=1e-3)                 # another posterior
    sim_t = np.linspace(0, Time, T + 1)
    for e, exp in enumerate(e_data):
        wts = [gpu.likelihood.weights_from_uncertainty(u) for u in exp[2]]
        on_grid = gpu.driver.fused_entry_point(exp[0], sim_t, 3, False) == "trpl_loglik"
        info = {}
        Pd = gpu.loglik(X0, ini, simPar[0], Time, 128, T, exp[1], weights=wts, info=info,
                        times=None if on_grid else exp[0])
        assert not info["status"].any() and (info["floor_col"] == -1).all()
        if n_exp == 1:
            # the fused single-experiment level IS this call, in blocks of sims_per_gpu: a system's bits do not depend on the cut
            P_blocks = np.concatenate([gpu.loglik(X0[b:b + 4], ini, simPar[0], Time, 128, T, exp[1], weights=wts,
                                                  times=None if on_grid else exp[0]) for b in range(0, len(X0), 4)])
            assert np.array_equal(Pw[e], P_blocks)
        bound = np.zeros(len(X0))
        for c in range(3):
            n = len(exp[1][c])
            bound += (6 + -(-n // 64) + 6) * EPS * info["sse"][c] + 2 * np.sqrt(info["wsum"][c] * info["sse"][c]) * ENV
        for name, P in (("fused", Pw[e]), ("unfused", Pu[e])):
            err = np.abs(P - Pd)
            print("n_exp %d exp %d %s: |P - loglik(weights=)| / bound = %.3g" % (n_exp, e, name, float((err / bound).max())))
            assert (err <= bound).all(), (name, e)
    _, Pg, Xg = run(fused=True, weighted=True, mag_grid=[0.0, 0.5], predict=True)       # combines with mag_grid and predict
    assert Pg.shape == (n_exp, 2 * len(X0)) and np.isfinite(Pg).all()
    for bad, word in ((dict(devices=[0]), "devices"), (dict(max_sims_per_block=2), "max_sims_per_block")):
        with pytest.raises(ValueError) as ei:
            run(fused=True, weighted=True, **bad)
        assert word in str(ei.value) and "weighted" in str(ei.value)
    with pytest.raises(ValueError, match="devices"):
        gpu.loglik(X0, ini, simPar[0], Time, 128, T, e_data[0][1], weights=[np.ones(len(o)) for o in e_data[0][1]], devices=[0])
