"""The time-steppers (a-1 `pvSim`, a-2 `tEvol`, a-3 `iterate`; trpl_solve_pl) through the C ABI against the reference's golden
vectors and the pinned CPU oracle on the same seeded inputs -- small windows, hundreds of systems, and the window the
benchmark times (T = 8000: Power_scan x 64 x 3 and Twothick x 32 x 6), plus the two independent solvers north_star names
(Legacy/pvSim.py over whole curves with the BDF order capped at 2, Testing/PV_tester2.py + odeint).

Bars: STRICT (TRPL_FLAG_STRICT) -- state, every convergence decision and the PL quadrature bit-identical: iteration counts
EQUAL, PL(t) EQUAL in fp64.  FAST (default; both kernels) -- the oracle's iteration totals and PL inside the envelope
include/trpl.h states, |dPL / PL| <= 1e-9 + K / r (r = PL / (B L n0p0), K per film)."""
import numpy as np
import pytest

from gpu_common import (ENVELOPE_K, FLOOR, IDS, KERNELS, RTOL_FAST, RTOL_STRICT, SSE_GATE, _check_pl_against, deviation_bound, follows_iteration_path,
                        excess_scale, first_below, nthreads, record, relerr)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- pvSim
def _run(gpu, X12, length, time_ns, L, T, ini, **kw):
    pl, status, iters, sec = gpu.solve_pl(X12, length, time_ns, L, T, ini, **kw)
    assert sec > 0
    return pl, status, iters


def test_pvsim_power_scan_vs_reference_golden(gpu, golden):
    g = golden("pvsim_power")
    X, T = g["X"], int(g["T"])
    for c in range(3):
        want, want_it = g["plI"][c], g["iters"][c].sum(axis=1)
        pl, st, it = _run(gpu, X[:, :-1], 2000.0, float(g["time"]), 128, T, g["ini"][c], strict=True)
        assert not st.any() and np.array_equal(it, want_it)
        assert relerr(pl, want) <= RTOL_STRICT
        pl, st, it = _run(gpu, X[:, :-1], 2000.0, float(g["time"]), 128, T, g["ini"][c])
        assert not st.any()
        follows_iteration_path(it, want_it, "curve %d" % c)
        assert relerr(pl, want) < RTOL_FAST


def test_pvsim_twothick_vs_reference_golden(gpu, golden):
    g = golden("pvsim_twothick")
    X, T = g["X"], int(g["T"])
    for c, length in enumerate(g["lengths"]):
        want, want_it = g["plI"][c], g["iters"][c].sum(axis=1)
        pl, st, it = _run(gpu, X[:, :-1], float(length), float(g["time"]), 128, T, g["ini"][c], strict=True)
        assert not st.any() and np.array_equal(it, want_it)
        assert relerr(pl, want) <= RTOL_STRICT
        pl, st, it = _run(gpu, X[:, :-1], float(length), float(g["time"]), 128, T, g["ini"][c])
        assert not st.any()
        follows_iteration_path(it, want_it, "curve %d" % c)
        assert relerr(pl, want) < RTOL_FAST


def test_pvsim_64_random_samples_vs_oracle(gpu, oracle):
    """BASELINE configs[0] shape: Power_scan (3 excitations, 128 nodes) x 64 random parameter samples,
    here against the pinned CPU oracle: STRICT iteration counts identical and PL bit for bit, FAST PL to
    1e-9 and the oracle's iteration totals (gpu_common.follows_iteration_path)."""
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    X = w.samples(64)
    T, Time = 200, 200 * 0.025
    for c in range(3):
        r = oracle.pvsim(X[:, :-1], lens[c], Time, 128, T, ini[c], nthreads=8)
        pl, st, it, _ = gpu.solve_pl(X[:, :-1], lens[c], Time, 128, T, ini[c], strict=True)
        assert not st.any() and not r["status"].any()
        assert np.array_equal(it, r["iters_total"]) and relerr(pl, r["plI"]) <= RTOL_STRICT
        pl, st, it, _ = gpu.solve_pl(X[:, :-1], lens[c], Time, 128, T, ini[c])
        assert not st.any() and relerr(pl, r["plI"]) < RTOL_FAST
        follows_iteration_path(it, r["iters_total"], "curve %d" % c)


def test_against_legacy_pvsim_and_odeint(gpu, golden):
    """North-star parity references run by the reference itself (oracle/gen_golden.py):
    Legacy/pvSim.pvSim -- bit-level agreement on the steps where the schemes coincide (PL[0..2]), BDF
    order difference afterwards; PV_tester2.dydt + odeint -- the time-converged solution."""
    g = golden("legacy_odeint")
    X = g["X"].copy(); X[:, 7] = 0.0; X[:, 8] = 0.0
    L, T, length, Time = int(g["L"]), int(g["T"]), float(g["length"]), float(g["time"])
    sim_params = [length, Time, L, T, 1, (0,), 7, 10000]
    for strict in (True, False):
        plI = np.empty((len(X), T + 1))
        gpu.pvSim(plI, None, None, None, X[:, :-1], sim_params, (float(g["a_nm3"]), float(g["l_nm"])),
                  init_mode="exp", strict=strict)
        assert np.max(np.abs(plI[:, :3] / g["plI_legacy"][:, :3] - 1)) < 1e-12
        assert np.max(np.abs(plI / g["plI_legacy"] - 1)) < 1e-3
        assert np.max(np.abs(plI / g["plI_odeint"] - 1)) < 2e-2
        assert np.max(np.abs(plI[:, -1] / g["plI_odeint"][:, -1] - 1)) < 5e-4


def test_time_step_refinement_converges_to_pv_tester2_odeint(gpu, oracle, golden):
    """The third reference north_star names, pinned by time-step refinement.  Testing/PV_tester2.dydt (:13-49) under scipy
    odeint (:91-93, rtol 1e-10) is the time-converged solution of the spatial scheme that pvSimPCR.py:241-250 steps at fixed
    dt; tests/golden/tester_refine.npz holds it for 9 samples x (the three Power_scan excitations on a 2000 nm film + the
    strongest on a 311 nm film) over 20 ns, every 0.025 ns (oracle/gen_golden.py case_tester_refine, the reference's own
    code).  With T * k steps of dt / k and plT = k, k = 1, 2, 4, 8, 16 (the same 801 stored columns):
      * STRICT is the CPU oracle BIT FOR BIT at every k (PL bit patterns, iteration totals);
      * both FAST kernels hold the oracle's iteration totals and stay inside the header's envelope 1e-9 + K / r at every k;
      * STRICT and both FAST kernels converge to the odeint curves at SECOND order inside the bounds of
        tests/refine_common.py -- the same bounds tests/test_oracle_golden.py holds the oracle to: the film's worst
        deviation shrinks >= 2.8x, then >= 3.5x per halving of dt, to <= 1e-4 on every column and <= 3e-6 at 20 ns at
        dt / 16 (measured 5.1e-5 / 1.0e-6)."""
    import refine_common as R
    g = golden("tester_refine")
    L, T, Time = int(g["L"]), int(g["T"]), float(g["time"])
    rec = {}
    for f in range(len(g["lengths"])):
        X, length, dN = R.film_inputs(g, f)
        ode = g["plI_odeint"][f]
        scale = excess_scale(X, length, L)
        K = ENVELOPE_K[length]
        devs = {"strict": {}, "single": {}, "pair": {}}
        for k in R.REFINE_K:
            ref = oracle.pvsim(X[:, :-1], length, Time, L, T * k, dN, plT=k, nthreads=nthreads())
            assert not ref["status"].any()
            pl, st, it, _ = gpu.solve_pl(X[:, :-1], length, Time, L, T * k, dN, plT=k, strict=True)
            assert not st.any() and np.array_equal(it, ref["iters_total"]), (f, k)
            assert pl.shape == ode.shape and pl.tobytes() == ref["plI"].tobytes(), (f, k)
            devs["strict"][k] = R.deviation(pl, ode)
            r = ref["plI"] / scale[:, None]
            for kernel in ("single", "pair"):
                plf, stf, itf, _ = gpu.solve_pl(X[:, :-1], length, Time, L, T * k, dN, plT=k, kernel=kernel)
                assert not stf.any()
                follows_iteration_path(itf, ref["iters_total"], "film %d, k = %d, %s" % (f, k, kernel))
                dev = np.abs(plf / ref["plI"] - 1)
                assert (dev <= 1e-9 + K / r).all(), (f, k, kernel, float(np.max(dev * r)))
                devs[kernel][k] = R.deviation(plf, ode)
        for name, d in devs.items():
            worst, end = R.check_refinement(d, label="film %d, %s" % (f, name))
            rec["film%d_%s" % (f, name)] = {"worst": worst, "end": end}
    record("tester_refine", rec)


def test_whole_curve_parity_with_legacy_pvsim_under_the_bdf_order_cap(gpu, oracle, golden):
    """Full-curve parity with the second reference implementation north_star names.  Legacy/pvSim.pvSim (Legacy/pvSim.py:129-173:
    Euler then BDF2, Thomas solve, no Auger) ran as shipped over 2400 steps on 4 films x 9 samples (tests/golden/legacy_full.npz,
    oracle/gen_golden.py case_legacy_full); tests/test_oracle_golden.py holds the oracle with the BDF order capped at 2 to it
    within 1e-11 on every stored PL column and state snapshot.  Here, with TRPL_FLAG_BDF_ORDER(2) and CN = CP = 0:
      * STRICT is that oracle BIT FOR BIT -- PL as bit patterns, iteration totals, the N / P / E snapshots -- so the
        discretisation is pinned through an implementation that shares no code with pvSimPCR.py;
      * both FAST kernels hold the oracle's iteration totals and its PL inside the header's envelope 1e-9 + K / r
        (TRPL_PL_ENVELOPE_K_THICK on the 2000 nm films, _THIN on the 311 nm film), and the Legacy curves themselves within that
        envelope + 1e-11;
      * without the flag the same comparison stops at the BDF-order gap (2e-4 .. 5e-4): the flag is what is tested.
    The excitation goes in as "points" (Legacy's own exp profile, restated like pvSimPCR.py:347-353)."""
    g = golden("legacy_full")
    L, T, Time = int(g["L"]), int(g["T"]), float(g["time"])
    cols, pT = g["cols"], [int(v) for v in g["pT"]]
    worst = {}
    for f in range(len(g["lengths"])):
        length = float(g["lengths"][f])
        X = g["X"].copy(); X[:, 7] = 0.0; X[:, 8] = 0.0
        x = np.arange(L) + 0.5
        dN = float(g["a_nm3"][f]) * np.exp(-x / (float(g["l_nm"]) / (length / L)))
        ref = oracle.pvsim(X[:, :-1], length, Time, L, T, dN, snap_steps=pT, max_order=2, nthreads=nthreads())
        snaps = {}
        pl, st, it, _ = gpu.solve_pl(X[:, :-1], length, Time, L, T, dN, strict=True, bdf_order=2, snap_steps=pT, snapshots=snaps)
        assert not st.any() and np.array_equal(it, ref["iters_total"])
        assert pl.tobytes() == ref["plI"].tobytes()
        for k in ("plN", "plP", "plE"):
            assert snaps[k].tobytes() == ref[k].tobytes(), (f, k)
        assert np.max(np.abs(pl[:, cols] / g["plI"][f] - 1)) < 1e-11                  # hence STRICT against Legacy itself
        r = ref["plI"] / excess_scale(X, length, L)[:, None]
        K = ENVELOPE_K[length]
        for kernel in ("single", "pair"):
            plf, stf, itf, _ = gpu.solve_pl(X[:, :-1], length, Time, L, T, dN, kernel=kernel, bdf_order=2)
            assert not stf.any()
            follows_iteration_path(itf, ref["iters_total"], "film %d, %s" % (f, kernel))     # the oracle's totals
            dev = np.abs(plf / ref["plI"] - 1)
            assert (dev <= 1e-9 + K / r).all(), (f, kernel, float(np.max(dev * r)))
            devL = np.abs(plf[:, cols] / g["plI"][f] - 1)
            assert (devL <= 1e-9 + 1e-11 + K / r[:, cols]).all(), (f, kernel)
            worst[(f, kernel)] = float(dev.max())
            # the uncapped run is a different scheme: the BDF-order gap
            pl5, _, _, _ = gpu.solve_pl(X[:, :-1], length, Time, L, T, dN, kernel=kernel)
            gap = np.max(np.abs(pl5[:, cols] / g["plI"][f] - 1))
            assert 5e-5 < gap < 1e-3, gap
    record("legacy_full_parity", {"max_rel_dev_fast_vs_oracle_order2": {"film%d_%s" % k: v for k, v in worst.items()}})
    # the flag's range is checked, and the fused likelihood takes it too (same arithmetic as the PL-storing launch)
    with pytest.raises(gpu.TrplError):
        gpu.solve_pl(X[:2, :-1], length, Time, L, 8, dN, extra_flags=6 << 14)
    w = gpu.workloads
    ini, lens = w.power_scan(L)
    Xs = w.samples(64, seed=5)
    obs = [np.full(101, -3.0)] * 3
    a, b = {}, {}
    gpu.loglik(Xs, ini, lens, 2.5, L, 100, obs, info=a, kernel="pair", bdf_order=2)
    gpu.loglik(Xs, ini, lens, 2.5, L, 100, obs, info=b, kernel="pair")
    for c in range(3):
        plc, _, itc, _ = gpu.solve_pl(Xs[:, :-1], lens[c], 2.5, L, 100, ini[c], kernel="pair", bdf_order=2)
        want = np.sum((np.log10(plc) + Xs[:, -1:] - obs[c][None, :]) ** 2, axis=1)
        assert np.array_equal(a["iters_total"][c], itc) and np.max(np.abs(a["sse"][c] / want - 1)) < 1e-12
    assert not np.array_equal(a["sse"], b["sse"])


def test_pvsim_float32_buffer_matches_reference(gpu, golden):
    g = golden("pvsim_power")
    T = int(g["T32"])
    pl, st, _ = _run(gpu, g["X"][:2, :-1], 2000.0, T * 0.025, 128, T, g["ini"][2], dtype=np.float32, strict=True)
    assert pl.dtype == np.float32 and not st.any()
    # same two float32 roundings as the reference (store, then divide); the fp64 value in front
    # of them differs by ~1e-16, so allow one float32 ulp
    assert np.max(np.abs(pl - g["plI32"]) / g["plI32"]) <= 2.0 ** -23


def test_pvsim_small_grids_plT_and_nonconvergence(gpu, golden):
    """Every compiled grid size, every sink and predict against the oracle: tests/test_gpu_stepper_grids.py."""
    g = golden("pvsim_small")
    X = g["X"]
    for L in (8, 32, 64):
        for strict, tol in ((True, RTOL_STRICT), (False, RTOL_FAST)):
            pl, st, it = _run(gpu, X[:, :-1], 500.0, 30 * 0.05, L, 30, g[f"ini_L{L}"], tol=6, strict=strict)
            assert not st.any() and relerr(pl, g[f"plI_L{L}"]) <= tol
            if strict:
                assert np.array_equal(it, g[f"it_L{L}"].sum(axis=1))
    pl, st, it = _run(gpu, X[:, :-1], 500.0, 40 * 0.05, 32, 40, g["ini_L32"], tol=6, plT=4, strict=True)
    assert pl.shape == (3, 11) and relerr(pl, g["plI_plT4"]) <= RTOL_STRICT
    assert np.array_equal(it, g["it_plT4"].sum(axis=1))
    # forced non-convergence: status = 1 + step, remaining PL = NaN, other systems unaffected
    p, t, n = g["nc_log"][-1]
    Xnc = np.vstack([X[2, :-1], X[0, :-1]])
    pl, st, it = _run(gpu, Xnc, 311.0, 10 * 0.025, 32, 10, g["nc_ini"], MAX=3, strict=True)
    assert st[0] == 1 + t and np.isnan(pl[0, t:]).all()


def test_fast_mode_plT_and_midrun_nonconvergence(gpu, oracle):
    """FAST mode batches its PL output over 64 time points: check plT > 1 (columns != steps), a column
    count that is not a multiple of 64, and a non-convergence in the middle of a run -- PL before the
    failing step must be valid and everything from it on NaN -- against the oracle."""
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    X = w.samples(4)
    T, Time = 150, 150 * 0.025
    r = oracle.pvsim(X[:, :-1], lens[2], Time, 128, T, ini[2], plT=3, want_step_iters=True)
    pl, st, it, _ = gpu.solve_pl(X[:, :-1], lens[2], Time, 128, T, ini[2], plT=3)
    assert pl.shape == (4, 51) and not st.any() and relerr(pl, r["plI"]) < RTOL_FAST
    # MAX just above the iteration count of the late steps: the early (stiffer) steps pass only for some samples
    steps = oracle.pvsim(X[:, :-1], lens[2], Time, 128, T, ini[2], want_step_iters=True)["step_iters"]
    MAXc = int(np.sort(steps.max(axis=1))[1]) + 1          # at least one sample exceeds it, at least one does not
    ro = oracle.pvsim(X[:, :-1], lens[2], Time, 128, T, ini[2], MAX=MAXc)
    assert ro["status"].any() and not ro["status"].all()
    for dtype in (np.float64, np.float32):
        pl, st, it, _ = gpu.solve_pl(X[:, :-1], lens[2], Time, 128, T, ini[2], MAX=MAXc, dtype=dtype)
        assert np.array_equal(st, ro["status"])
        for s_ in range(4):
            t_fail = st[s_] - 1 if st[s_] else T + 1
            good = slice(0, t_fail)
            tol = RTOL_FAST if dtype == np.float64 else 2.0 ** -22
            assert np.all(np.abs(pl[s_, good] / ro["plI"][s_, good] - 1) < tol)
            assert np.isnan(pl[s_, t_fail:]).all()
    # likelihood mode: the failing samples get -inf, the others match the oracle
    obs = [np.log10(ro["plI"][~ro["status"].astype(bool)][0]) + 0.05]
    info = {}
    P = gpu.loglik(X, ini[2:3], lens[2:3], Time, 128, T, obs, MAX=MAXc, info=info)
    assert np.array_equal(info["status"][0], ro["status"]) and np.all(np.isneginf(P[ro["status"] != 0]))
    want = oracle.simulate_loglik(X, ini[2:3], lens[2:3], Time, 128, T, [([np.linspace(0, Time, T + 1)], obs)],
                                  pl_dtype=np.float64, MAX=MAXc)[0]
    ok = ro["status"] == 0
    assert np.max(np.abs(P[ok] - want[ok]) / np.abs(want[ok])) < 1e-8


def test_pvsim_dropin_signature(gpu, golden):
    """Called exactly the way bayeslib.simulate calls the model (bayeslib.py:144-146)."""
    g = golden("pvsim_power")
    T = 24
    sim_params = [2000, T * 0.025, 128, T, 1, (0, 1, 3, 10, 30, 100), 7, 10000]
    plI = np.empty((5, T + 1), dtype=np.float32)
    plN = np.empty((5, 2, 128)); plE = np.empty((5, 2, 129))
    sec = gpu.pvSim(plI, plN, plN.copy(), plE, g["X"][:, :-1], sim_params, g["ini"][1], (128,), 8 * 256, 1,
                    init_mode="points")
    assert isinstance(sec, float) and sec > 0
    want = g["plI"][1][:, :T + 1]
    assert np.max(np.abs(plI / want - 1)) < 2e-7
    with pytest.raises(ValueError):
        gpu.pvSim(plI, None, None, None, g["X"][:, :-1], sim_params, g["ini"][1], init_mode="continue")
    with pytest.raises(ValueError):
        gpu.pvSim(plI, None, None, None, g["X"][:, :-1], sim_params, g["ini"][1][:64], init_mode="points")


# ----------------------------------------------------------------------------- full-size properties
def test_full_size_properties(gpu):
    """At sizes the CPU oracle cannot reach: (i) FAST vs STRICT agree on thousands of random
    samples; (ii) shard invariance: a sample's likelihood does not depend on its batch;
    (iii) determinism: two runs are bit-identical; (iv) the offset identity
    P(m) = P(0) - sum_c [ n_c m^2 + 2 m r_c ] holds through the fused kernel."""
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T, Time = 65536, 24, 24 * 0.025            # BASELINE configs[1] sample count
    X = w.samples(S)
    mark = (w.MARKED_POINT * gpu.UNIT_CONVERSIONS)[None, :]
    obs = []
    for c in range(3):
        pl, st, _, _ = gpu.solve_pl(mark[:, :-1], lens[c], Time, 128, T, ini[c], strict=True)
        obs.append(np.log10(pl[0]))
    info_f, info_s = {}, {}
    Pf = gpu.loglik(X, ini, lens, Time, 128, T, obs, info=info_f)
    Ps = gpu.loglik(X, ini, lens, Time, 128, T, obs, strict=True, info=info_s)
    ok = ~(info_f["status"].any(axis=0) | info_s["status"].any(axis=0))
    assert ok.mean() > 0.99
    assert np.max(np.abs(Pf[ok] - Ps[ok]) / np.abs(Ps[ok])) < 1e-8
    assert abs(info_f["iters_total"].sum() / info_s["iters_total"].sum() - 1) < 1e-3
    Pf2 = gpu.loglik(X, ini, lens, Time, 128, T, obs)
    assert np.array_equal(Pf, Pf2)                                            # (iii)
    sub = gpu.loglik(X[60001:65300], ini, lens, Time, 128, T, obs)            # same kernel, other partners
    assert np.array_equal(sub, Pf[60001:65300])                               # (ii)
    # a launch that cannot keep the chip full runs the one-system-per-wavefront kernel, whose node sums
    # associate differently: same likelihoods to rounding
    small = gpu.loglik(X[61000:61300], ini, lens, Time, 128, T, obs)
    assert np.allclose(small, Pf[61000:61300], rtol=1e-10, atol=1e-10)
    m = 0.25
    Xm = X.copy(); Xm[:, -1] = m
    Pm = gpu.loglik(Xm, ini, lens, Time, 128, T, obs)
    # residual sums r_c from sse(m=0): sum (a+m)^2 = sum a^2 + 2 m sum a + n m^2; check via a third offset
    Xm2 = X.copy(); Xm2[:, -1] = -m
    Pm2 = gpu.loglik(Xm2, ini, lens, Time, 128, T, obs)
    n_tot = 3 * (T + 1)
    assert np.max(np.abs((Pm[ok] + Pm2[ok]) / 2 - (Pf[ok] - n_tot * m * m)) / np.abs(Pf[ok])) < 1e-9


def test_strict_mode_is_bit_identical_to_the_oracle_on_hundreds_of_systems(gpu, oracle):
    """STRICT against the pinned oracle on a wider draw than the goldens hold: 512 Power_scan samples and 128
    Twothick samples (all six curves, the stiff 311 nm ones included) x 300 steps -- PL bit for bit (compared as
    float64 bit patterns), per-system iteration totals and status equal."""
    w = gpu.workloads
    T = 300
    Time = T * 0.025
    for name, (ini, lens), S in (("power_scan", w.power_scan(128), 512), ("twothick", w.twothick(128), 128)):
        X = w.samples(S, seed=101)[:, :12]
        for c in range(len(lens)):
            r = oracle.pvsim(X, lens[c], Time, 128, T, ini[c], nthreads=nthreads())
            pl, st, it, _ = gpu.solve_pl(X, lens[c], Time, 128, T, ini[c], strict=True)
            assert np.array_equal(st, r["status"]) and np.array_equal(it, r["iters_total"]), (name, c)
            assert np.array_equal(pl.view(np.uint64), r["plI"].view(np.uint64)), (name, c)


def test_fast_kernels_vs_oracle_over_a_longer_window(gpu, oracle):
    """Both FAST steppers against the oracle over 1200 steps (30 ns: well past the stiff start, deep into the
    two-iterations-per-step regime that dominates a production run), 256 samples x 3 curves: PL to 1e-9 above the
    floor, > 99 % of the systems with exactly the oracle's iteration total, none flagged."""
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 256, 1200
    Time = T * 0.025
    X = w.samples(S, seed=111)[:, :12]
    for c in range(3):
        r = oracle.pvsim(X, lens[c], Time, 128, T, ini[c], nthreads=nthreads())
        assert not r["status"].any()
        for kernel in ("single", "pair"):
            err, same = _check_pl_against(gpu, X, lens[c], Time, 128, T, ini[c], r["plI"], r["iters_total"], kernel)
            assert same > 0.99, (c, kernel, same)


@pytest.mark.parametrize("mode", KERNELS, ids=IDS)
def test_bench_window_pl_and_iteration_totals_against_the_oracle(gpu, long_window, mode):
    g = long_window
    for c in range(3):
        want = g["ref"][c]
        assert not want["status"].any()
        pl, st, it, _ = gpu.solve_pl(g["X"][:, :12], g["lens"][c], g["Time"], g["L"], g["T"], g["ini"][c], **mode)
        assert not st.any()
        assert np.array_equal(it, want["iters_total"]), (c, int((it != want["iters_total"]).sum()))
        if mode.get("strict"):
            assert np.array_equal(pl.view(np.int64), want["plI"].view(np.int64))       # bit patterns
            continue
        dev = np.abs(pl / want["plI"] - 1)
        bound = deviation_bound(want["plI"], excess_scale(g["X"], g["lens"][c]))
        assert (dev <= bound).all(), (c, float(np.nanmax(dev / bound)))
        # the review's wording: every point >= 1e-12 of the curve's start that is also above the floor, to 2e-8
        above = (want["plI"] >= 1e-12 * want["plI"][:, :1]) & (want["plI"] >= 1e-4 * excess_scale(g["X"], g["lens"][c])[:, None])
        assert dev[above].max() < 2e-8 and above.mean() > 0.9


@pytest.mark.parametrize("mode", [dict(strict=True), dict(kernel="single"), dict(kernel="pair")], ids=["strict", "single", "pair"])
def test_twothick_bench_window_against_the_oracle(gpu, twothick_window, mode):
    g = twothick_window
    S = g["S"]
    rec = {}
    info = {}
    P = gpu.loglik(g["X"], g["ini"], g["lens"], g["Time"], g["L"], g["T"], g["obs"], info=info, **mode)
    assert not info["status"].any()
    for c in range(6):
        want = g["ref"][c]
        length = float(g["lens"][c])
        assert not want["status"].any()
        pl, st, it, _ = gpu.solve_pl(g["X"][:, :12], length, g["Time"], g["L"], g["T"], g["ini"][c], **mode)
        assert not st.any()
        scale = excess_scale(g["X"], length)
        want_col = first_below(want["plI"], FLOOR * scale)
        if mode.get("strict"):
            assert np.array_equal(it, want["iters_total"])
            assert np.array_equal(pl.view(np.int64), want["plI"].view(np.int64))       # bit patterns
            assert np.array_equal(info["iters_total"][c], want["iters_total"])
            assert np.array_equal(info["floor_col"][c], want_col)
            assert np.max(np.abs(info["sse"][c] - g["sse"][c]) / g["sse"][c]) < 1e-12
            continue
        # iteration totals: the oracle's (a knife-edge convergence decision may flip on one system of the 32, by one)
        n_differ = follows_iteration_path(it, want["iters_total"], "curve %d" % c)
        assert np.array_equal(info["iters_total"][c], it)                  # fused and PL-storing launches agree
        r = want["plI"] / scale[:, None]
        dev = np.abs(pl / want["plI"] - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            bound = 1e-9 + ENVELOPE_K[length] / r
        physical = r >= 1e-10                                              # below: rounding noise in both evaluations
        worst = float(np.max((dev / bound)[physical])) if physical.any() else 0.0
        assert worst <= 1.0, (c, length, worst)
        above = r >= FLOOR
        k_meas = float(np.max((dev * r)[physical & (r < 0.1)])) if (physical & (r < 0.1)).any() else 0.0
        # floor_col: the column the oracle's own PL gives
        assert np.array_equal(info["floor_col"][c], want_col), (c, int((info["floor_col"][c] != want_col).sum()))
        clear = want_col < 0
        gap = np.abs(info["sse"][c] - g["sse"][c]) / g["sse"][c]
        assert gap[clear].max() < SSE_GATE[length], (c, length, float(gap[clear].max()))
        rec["curve%d" % c] = dict(length=length, iteration_totals_differ=n_differ, worst_over_bound=worst,
                                  max_dev_above_floor=float(dev[above].max()), envelope_k_measured=k_meas,
                                  floor_free=int(clear.sum()), max_sse_gap_floor_free=float(gap[clear].max()))
    if not mode.get("strict"):
        record("twothick_T8000_%s" % mode["kernel"], rec)
        # the likelihood of the floor-free samples: the oracle's, to the thin film's gate
        Pw = -g["sse"].sum(axis=0)
        clear_s = (info["floor_col"] == -1).all(axis=0)
        assert clear_s.sum() >= 0.8 * S
        assert np.max(np.abs(P[clear_s] - Pw[clear_s]) / np.abs(Pw[clear_s])) < SSE_GATE[311.0]
