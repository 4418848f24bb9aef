"""The CPU oracle (oracle/trpl_oracle.c) against the golden vectors produced by the reference's
own code (oracle/gen_golden.py).  The restatement follows the reference's evaluation order and
is built without FMA contraction, so the bar is BIT-EXACT everywhere."""
import numpy as np


def test_pcreduce_and_norm2_bit_exact(oracle, golden):
    g = golden("pcr_norm")
    for N in (4, 8, 32, 128, 512):
        for s in range(g[f"d{N}"].shape[0]):
            x = oracle.pcreduce(g[f"ld{N}"][s], g[f"d{N}"][s], g[f"ud{N}"][s], g[f"B{N}"][s])
            assert np.array_equal(x, g[f"x{N}"][s])
            # reference call form: norm2(A0=upper, A1=diag, A2=lower, b, c)
            e = oracle.norm2(g[f"ud{N}"][s], g[f"d{N}"][s], g[f"ld{N}"][s], g[f"B{N}"][s], g[f"c{N}"][s])
            assert e == g[f"err{N}"][s]


def test_pcreduce_solves_the_system(oracle, golden):
    g = golden("pcr_norm")
    N = 128
    ld, d, ud, B = g[f"ld{N}"][0], g[f"d{N}"][0], g[f"ud{N}"][0], g[f"B{N}"][0]
    x = oracle.pcreduce(ld, d, ud, B)
    r = d * x
    r[1:] += ld[1:] * x[:-1]
    r[:-1] += ud[:-1] * x[1:]
    assert np.max(np.abs(r - B)) < 1e-12


def test_pvsim_power_scan_bit_exact(oracle, golden):
    g = golden("pvsim_power")
    X, T = g["X"], int(g["T"])
    for c in range(3):
        r = oracle.pvsim(X[:, :-1], float(g["length"]), float(g["time"]), int(g["L"]), T, g["ini"][c],
                         want_step_iters=True)
        assert np.array_equal(r["plI"], g["plI"][c])
        assert np.array_equal(r["step_iters"], g["iters"][c])
        assert not r["status"].any()
    r = oracle.pvsim(X[:2, :-1], 2000, int(g["T32"]) * 0.025, 128, int(g["T32"]), g["ini"][2], dtype=np.float32)
    assert r["plI"].dtype == np.float32 and np.array_equal(r["plI"], g["plI32"])


def test_pvsim_twothick_bit_exact(oracle, golden):
    g = golden("pvsim_twothick")
    X, T = g["X"], int(g["T"])
    for c in range(len(g["lengths"])):
        r = oracle.pvsim(X[:, :-1], float(g["lengths"][c]), float(g["time"]), 128, T, g["ini"][c],
                         want_step_iters=True)
        assert np.array_equal(r["plI"], g["plI"][c])
        assert np.array_equal(r["step_iters"], g["iters"][c])
    assert g["iters"].max() > 400          # the 311 nm / high power curve stresses the iteration


def test_pvsim_bundled_convergence_bit_exact(oracle, golden):
    """max_sims_per_block = 3 and 2 (pvSimPCR.py:213-216,:258-266): the bundle's systems iterate until the slowest
    has converged -- PL and the shared per-step iteration counts as the reference produced them, bundles 3+3+1 and
    2+2+2+1, on the high-power Power_scan curve and the stiff 311 nm Twothick curve."""
    g = golden("pvsim_bundle")
    X, T, Time, L = g["X"][:, :12], int(g["T"]), float(g["time"]), int(g["L"])
    for tag, ini, length in (("P", g["iniP"], float(g["lengthP"])), ("T", g["iniT"], float(g["lengthT"]))):
        for m in (3, 2):
            r = oracle.pvsim(X, length, Time, L, T, ini, mspb=m, want_step_iters=True, nthreads=2)
            assert np.array_equal(r["plI"], g["pl%s%d" % (tag, m)]), (tag, m)
            assert np.array_equal(r["step_iters"], g["it%s%d" % (tag, m)]), (tag, m)
            assert not r["status"].any()
        # and the bundles do change the answer: the unbundled run differs from the bundled one
        r1 = oracle.pvsim(X, length, Time, L, T, ini)
        assert not np.array_equal(r1["plI"], g["pl%s3" % tag]) and np.allclose(r1["plI"], g["pl%s3" % tag], rtol=1e-6)
    # a bundle that hits MAX is flagged as a whole
    cap = int(g["itT3"][3].max())                      # the second bundle's slowest step
    r = oracle.pvsim(X, float(g["lengthT"]), Time, L, T, g["iniT"], mspb=3, MAX=cap)
    assert (r["status"][3:6] == r["status"][3]).all() and r["status"][3] > 0 and np.isnan(r["plI"][3:6, -1]).all()
    assert (r["status"][:3] == r["status"][0]).all() and r["status"][6] == 0


def test_pvsim_grids_the_sizes_the_small_golden_leaves_out(oracle, golden):
    """L = 4, 16, 256 (oracle/gen_golden.py case_pvsim_grids: the reference's pvSim on pvsim_small's film, window and tolerance):
    with pvsim_small (8, 32, 64) and the L = 128 goldens the oracle is pinned at every grid size the stepper is compiled for
    but L = 512, which the reference cannot run (its shared arrays exceed the static limit); all three sizes asked for ran."""
    g = golden("pvsim_grids")
    X = g["X"]
    for L in (4, 16, 256):
        r = oracle.pvsim(X[:, :-1], 500, 30 * 0.05, L, 30, g[f"ini_L{L}"], tol=6, want_step_iters=True)
        assert not r["status"].any() and r["plI"].shape == (3, 31)
        assert np.array_equal(r["plI"], g[f"plI_L{L}"]) and np.array_equal(r["step_iters"], g[f"it_L{L}"])


def test_pvsim_small_grids_plT_and_nonconvergence(oracle, golden):
    g = golden("pvsim_small")
    X = g["X"]
    for L in (8, 32, 64):
        r = oracle.pvsim(X[:, :-1], 500, 30 * 0.05, L, 30, g[f"ini_L{L}"], tol=6, want_step_iters=True)
        assert np.array_equal(r["plI"], g[f"plI_L{L}"]) and np.array_equal(r["step_iters"], g[f"it_L{L}"])
    r = oracle.pvsim(X[:, :-1], 500, 40 * 0.05, 32, 40, g["ini_L32"], tol=6, plT=4, want_step_iters=True)
    assert r["plI"].shape == (3, 11)
    assert np.array_equal(r["plI"], g["plI_plT4"]) and np.array_equal(r["step_iters"], g["it_plT4"])
    # reference: iterate() returned MAX=3 at step 0 -> flagged, nothing written (pvSimPCR.py:269-274)
    p, t, it = g["nc_log"][-1]
    r = oracle.pvsim(X[2:3, :-1], 311, 10 * 0.025, 32, 10, g["nc_ini"], MAX=3)
    assert it == 3 and r["status"][0] == 1 + t
    assert np.isnan(r["plI"][0, t:]).all()
    assert np.all(g["nc_plI"] < 0)         # the reference never touched its (pre-filled) buffer


def test_fastlog_and_prob_bit_exact(oracle, golden):
    g = golden("probs")
    l64 = g["pl64"].copy()
    oracle.fastlog(l64, float(g["MIN"]))
    assert np.array_equal(l64, g["log64"])
    l32 = g["pl32"].copy()
    oracle.fastlog(l32, float(g["MIN"]))
    assert l32.dtype == np.float32 and np.array_equal(l32, g["log32"])
    P = g["P64_in"].copy()
    oracle.prob(P, g["log64"], g["values"], g["mag"])
    assert np.array_equal(P, g["P64"])
    P = np.zeros(len(g["mag"]))
    oracle.prob(P, g["log32"], g["values"], g["mag"])
    assert np.array_equal(P, g["P32"])


def test_fastlog_float32_clamp_is_minus_inf(oracle):
    # (float)DBL_MIN == 0.0f, so a clamped float32 entry becomes log10(0) = -inf
    x = np.array([[0.0, -1.0, 1e-3]], dtype=np.float32)
    oracle.fastlog(x)
    assert np.isneginf(x[0, 0]) and np.isneginf(x[0, 1]) and np.isclose(x[0, 2], -3)
    y = np.array([[0.0, 1e-3]])
    oracle.fastlog(y)
    assert np.isclose(y[0, 0], np.log10(np.finfo(float).tiny))


def test_simulate_end_to_end_bit_exact(oracle, golden):
    """bayeslib.bayes(pvSim, ...) -> P for two experiments (bypass and griddata paths)."""
    g = golden("bayes_e2e")
    T, tg, npre = int(g["T"]), g["tgrid"], int(g["npre"])
    e_data = [([tg] * 3, list(g["obs0"])), ([tg[:npre]] * 3, list(g["obs1"]))]
    P = oracle.simulate_loglik(g["X"], g["ini"], float(g["length"]), float(g["time"]), int(g["L"]), T, e_data,
                               sims_per_gpu=int(g["sims_per_gpu"]), nthreads=4)
    assert np.array_equal(P, g["P"])


def test_simulate_real_data_and_offgrid_times_bit_exact(oracle, golden):
    """bayes() on the reference's shipped example files (ingested by its own bayes_io): exp 0 on
    the grid, exp 1 at irregular off-grid times (per-row griddata)."""
    g = golden("bayes_realdata")
    T = int(g["T"])
    e_data = [([g[f"t_{e}_{c}"] for c in range(3)], [g[f"v_{e}_{c}"] for c in range(3)]) for e in range(2)]
    P = oracle.simulate_loglik(g["X"], g["ini"], float(g["length"]), float(g["time"]), 128, T, e_data,
                               sims_per_gpu=3, nthreads=4)
    assert np.array_equal(P, g["P"])


def test_scipy_port_matches_reference_fallback(golden):
    """oracle/scipy_mol.py (the "scipy CPU path" timing baseline) against PL(t) produced by the
    reference's pvSim_fallback.pvSim_cpu_fallback as shipped (no stand-in involved)."""
    from oracle import scipy_mol
    g = golden("fallback")
    X, T, Time = g["X"], int(g["T"]), float(g["time"])
    for c in (0, 2):
        pl = np.empty((2, T + 1))
        scipy_mol.pvsim_cpu(pl, X[:2], [float(g["length"]), Time, int(g["L"]), T], g["ini"][c])
        assert np.max(np.abs(pl / g["plI"][c][:2] - 1)) < 1e-6
    # it is a different discretisation of PL (Simpson) than the GPU path's midpoint rule: 0.03-0.04 dex at t=0
    import oracle
    mid = oracle.pvsim(X[:1, :-1], float(g["length"]), Time, 128, T, g["ini"][2])["plI"][0]
    assert 0.02 < abs(np.log10(mid[0] / g["plI"][2][0][0])) < 0.05


def _legacy_inputs(g):
    X = g["X"].copy()
    X[:, 7] = 0.0; X[:, 8] = 0.0                       # the legacy solvers have no Auger terms
    L, T, length = int(g["L"]), int(g["T"]), float(g["length"])
    x = np.arange(L) + 0.5
    dN = float(g["a_nm3"]) * np.exp(-x / (float(g["l_nm"]) / (length / L)))      # pvSimPCR.py:347-353 ("exp" init)
    return X, L, T, length, float(g["time"]), dN


def test_against_legacy_pvsim_and_odeint(oracle, golden):
    """The two independent solvers the north star names: Legacy/pvSim.py (same scheme, BDF2 only,
    Thomas solve: identical on the BDF1/BDF2 steps, ~4e-4 apart later) and PV_tester2.dydt + scipy
    odeint (the time-converged solution of the same spatial scheme: first-order error on step 1,
    ~2e-4 at the end of this 6 ns window)."""
    g = golden("legacy_odeint")
    X, L, T, length, Time, dN = _legacy_inputs(g)
    r = oracle.pvsim(X[:, :-1], length, Time, L, T, dN)
    pl = r["plI"]
    assert np.max(np.abs(pl[:, :3] / g["plI_legacy"][:, :3] - 1)) < 1e-13
    assert np.array_equal(r["iters_max"], g["iters_legacy"])            # the stiff step 0 takes the same iterations
    assert np.max(np.abs(pl / g["plI_legacy"] - 1)) < 1e-3
    assert np.max(np.abs(pl / g["plI_odeint"] - 1)) < 2e-2
    assert np.max(np.abs(pl[:, -1] / g["plI_odeint"][:, -1] - 1)) < 5e-4


def test_state_snapshots_against_legacy_pvsim(oracle, golden):
    """The oracle's plN / plP / plE (pvSimPCR.py:283-288 restated; Legacy/pvSim.py:121-126,:169-171) against
    what Legacy/pvSim.pvSim itself returned: on the steps where BDF1 / BDF2 and the BDF ramp coincide
    (t = 0, 1, 2) N and P agree to 1e-12 (Thomas vs PCR rounding) and the field -- the integral of the tiny
    charge imbalance P - N, so 1e-14 of N is 1e-7 of E -- to 1e-6 of its largest value; afterwards the
    densities stay within the BDF-order gap (< 5e-3) at the Testing/compare.py:22 sample points."""
    g = golden("legacy_odeint")
    X, L, T, length, Time, dN = _legacy_inputs(g)
    pT = [int(v) for v in g["pT"]]
    r = oracle.pvsim(X[:, :-1], length, Time, L, T, dN, snap_steps=pT)
    for k in ("plN", "plP"):
        ref = g[k + "_legacy"]
        assert r[k].shape == ref.shape
        assert np.max(np.abs(r[k][:, :3] - ref[:, :3]) / ref[:, :3]) < 1e-12
        locs = (np.array([0.1, 0.3, 0.5, 0.7, 0.9]) * L).astype(int)
        for thr in range(len(X)):
            a, b = r[k][thr][3:, locs].ravel(), ref[thr][3:, locs].ravel()
            assert np.linalg.norm(a - b) / np.linalg.norm(b) < 5e-3
    refE = g["plE_legacy"]
    assert (r["plE"][:, 0] == 0).all() and (refE[:, 0] == 0).all()           # t = 0: no field yet
    scale = np.abs(refE[:, 1:3]).max(axis=2, keepdims=True)
    assert np.max(np.abs(r["plE"][:, 1:3] - refE[:, 1:3]) / scale) < 1e-6
    assert (r["plE"][:, :, 0] == 0).all() and (r["plE"][:, :, L] == 0).all()   # E_0 = E_L = 0 (pvSimPCR.py:205)
    # the snapshot of step t is the state PL(t) is computed from: rebuild PL from it (pvSimPCR.py:276-281,:393)
    dx = length / L
    rate = X[:, 4]
    for i, t in enumerate(pT):
        pl = rate * dx * np.sum(r["plN"][:, i] * r["plP"][:, i] - (X[:, 0] * X[:, 1])[:, None], axis=1)
        assert np.max(np.abs(pl / r["plI"][:, t] - 1)) < 1e-9
    # a repeated step fills its first slot only, a step beyond T none (Legacy `pT.index(t)`)
    r2 = oracle.pvsim(X[:1, :-1], length, Time, L, 20, dN, snap_steps=[5, 5, 40, 0])
    assert (r2["plN"][0, 1] == 0).all() and (r2["plN"][0, 2] == 0).all() and (r2["plN"][0, 0] > 0).all()
    assert np.array_equal(r2["plN"][0, 3], r["plN"][0, 0])


def _legacy_full_film(g, f):
    """inputs of film f of tests/golden/legacy_full.npz as the oracle / the product take them ("points" excitation)"""
    X = g["X"].copy()
    X[:, 7] = 0.0; X[:, 8] = 0.0                       # Legacy/pvSim.py has no Auger terms
    L, length = int(g["L"]), float(g["lengths"][f])
    x = np.arange(L) + 0.5
    dN = float(g["a_nm3"][f]) * np.exp(-x / (float(g["l_nm"]) / (length / L)))     # Legacy/pvSim.py:151-156 ("exp" init)
    return X, length, dN


def test_whole_curve_against_legacy_pvsim_with_the_bdf_order_capped_at_two(oracle, golden):
    """The second solver north_star names, over WHOLE curves: Legacy/pvSim.pvSim (Euler, then BDF2; Thomas solve; sequential
    norms; no Auger; its own "exp" excitation) shares no code with pvSimPCR.py.  With the BDF ramp of pvSimPCR.py:241-250 capped
    at order 2 (oracle max_order) and CN = CP = 0 the two discretise the same equations the same way, so what is
    left between them is rounding: Thomas against parallel cyclic reduction, a serial against a tree norm, numpy's pairwise PL
    sum against the kernel's serial one.  2400 steps (60 ns) x three Power_scan excitations on a 2000 nm film + the strongest
    on a 311 nm film x 9 samples: PL on all 2401 x 36 stored columns within 1e-11 (measured 4.5e-13), N and P profiles at
    0.1 / 10 / 100 % of the window within 1e-11 (3.5e-12), the field within 5e-6 of its largest value (it is the integral of
    the charge imbalance P - N: 1e-13 of N is 1e-6 of E), the same largest iteration count on every system.  Uncapped, the
    same comparison stops at the BDF-order gap, 2e-4 .. 5e-4 (asserted: the cap is what is being tested)."""
    g = golden("legacy_full")
    L, T, Time = int(g["L"]), int(g["T"]), float(g["time"])
    cols, pT = g["cols"], [int(v) for v in g["pT"]]
    for f in range(len(g["lengths"])):
        X, length, dN = _legacy_full_film(g, f)
        r = oracle.pvsim(X[:, :-1], length, Time, L, T, dN, snap_steps=pT, max_order=2, nthreads=4)
        assert not r["status"].any()
        assert np.array_equal(r["iters_max"], g["iters_max"][f])
        assert np.max(np.abs(r["plI"][:, cols] / g["plI"][f] - 1)) < 1e-11
        for k in ("plN", "plP"):
            assert np.max(np.abs(r[k] / g[k][f] - 1)) < 1e-11, (f, k)
        scale = np.abs(g["plE"][f]).max(axis=2, keepdims=True)
        assert np.max(np.abs(r["plE"] - g["plE"][f]) / scale) < 5e-6
        full = oracle.pvsim(X[:, :-1], length, Time, L, T, dN, nthreads=4)          # the reference's ramp to order 5
        gap = np.max(np.abs(full["plI"][:, cols] / g["plI"][f] - 1))
        assert 5e-5 < gap < 1e-3, gap
    # order 1 (implicit Euler throughout) and the default are different schemes again; an order outside 1 .. 5 is ignored
    X, length, dN = _legacy_full_film(g, 0)
    e1 = oracle.pvsim(X[:1, :-1], length, 100 * 0.025, L, 100, dN, max_order=1)["plI"]
    e5 = oracle.pvsim(X[:1, :-1], length, 100 * 0.025, L, 100, dN)["plI"]
    assert np.array_equal(e1[:, :2], e5[:, :2]) and not np.array_equal(e1[:, 2:], e5[:, 2:])
    assert np.array_equal(oracle.pvsim(X[:1, :-1], length, 100 * 0.025, L, 100, dN, max_order=9)["plI"], e5)


def test_time_step_refinement_converges_to_pv_tester2_odeint(oracle, golden):
    """The THIRD solver north_star names, as a convergence target: Testing/PV_tester2.dydt (:13-49) + scipy odeint (:91-93)
    is the time-converged solution of the spatial scheme pvSimPCR.py steps at fixed dt.  tests/golden/tester_refine.npz
    (oracle/gen_golden.py case_tester_refine: the reference's dydt, rtol 1e-10; 9 samples x the three Power_scan excitations
    on a 2000 nm film + the strongest on a 311 nm film; 20 ns stored every 0.025 ns).  The oracle with T * k steps and
    plT = k, k = 1, 2, 4, 8, 16, approaches those curves at second order -- the film's worst deviation shrinks 2.9x, then
    3.8 .. 4.0x per halving of dt, to <= 1e-4 on every column (5.1e-5 measured, at step 1: the Euler start of
    pvSimPCR.py:241-242) and <= 3e-6 at 20 ns (1.0e-6) at dt / 16.  Bounds: tests/refine_common.py."""
    import refine_common as R
    g = golden("tester_refine")
    assert float(g["ode_conv"].max()) < R.ODE_CONV and not g["negative"].any()      # PV_tester2.py:101: no negative density
    L, T, Time = int(g["L"]), int(g["T"]), float(g["time"])
    for f in range(len(g["lengths"])):
        X, length, dN = R.film_inputs(g, f)
        devs = {}
        for k in R.REFINE_K:
            r = oracle.pvsim(X[:, :-1], length, Time, L, T * k, dN, plT=k, nthreads=4)
            assert not r["status"].any() and r["plI"].shape == (len(X), T + 1)
            devs[k] = R.deviation(r["plI"], g["plI_odeint"][f])
        R.check_refinement(devs, label="film %d" % f)


def test_scipy_port_matches_the_reference_cpu_path_on_configs0(golden):
    """BASELINE.json configs[0] as worded -- Power_scan (3 excitations, 128 nodes) x 64 random samples through the reference's own
    CPU path -- is the fixture tests/golden/fallback64.npz: bayeslib.bayes(pvSim_fallback.pvSim_cpu_fallback, ...) with has_GPU
    False, the shipped Balancedhighsurf observations, run as 8 SLURM-style array tasks (oracle/gen_golden.py case_fallback64;
    8 cores of the development container: 26 s at the bench window T = 8000, 121 s at the reference's T = 80 000).
    oracle/scipy_mol.py, the port that bench.py's cpu_baseline_scipy times on the GPU box, is pinned to it here on ALL 192
    curves of the bench window (SURVEY asked for rtol 1e-4; since the port's right-hand side keeps the reference's association
    it takes the integrator's very steps: the stored float32 columns to their rounding, 1.2e-7, the fp64 head columns and the
    likelihood the CPU branch forms -- bayeslib.py:158-161,:198-201: float32 staging, |PL| + MIN, no mag_offset -- to 1e-12),
    and on 4 curves of the full window."""
    import os
    from oracle import scipy_mol
    g = golden("fallback64")
    X, ini, L, length = g["X"], g["ini"], int(g["L"]), float(g["length"])
    procs = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 2))
    T, Time, dec = int(g["w8k_T"]), float(g["w8k_time"]), int(g["w8k_dec"])
    pl = scipy_mol.pl_batch(X, ini, [length] * 3, Time, L, T, procs)
    ref = g["w8k_pl32"].astype(np.float64)
    assert pl.shape == (3, 64, T + 1) and ref.shape == (3, 64, T // dec + 1)
    assert np.max(np.abs(pl[:, :, ::dec] / ref - 1)) < 1.2e-7
    assert np.max(np.abs(pl[:, :2, :401] / g["w8k_pl_head"] - 1)) < 1e-12
    P = sum(scipy_mol.cpu_branch_loglik(pl[c], g["w8k_obs_%d" % c], Time, T) for c in range(3))
    assert np.max(np.abs(P / g["w8k_P"][0] - 1)) < 1e-12
    # the reference's full window (T = 80 000, 2000 ns; its full_* arrays are stored in fallback64_full.npz): four of the 192 curves
    gf = golden("fallback64_full")
    T, Time, dec = int(gf["full_T"]), float(gf["full_time"]), int(gf["full_dec"])
    plf = scipy_mol.pl_batch(X[:2], ini[[0, 2]], [length] * 2, Time, L, T, min(procs, 4))
    reff = gf["full_pl32"][[0, 2]][:, :2].astype(np.float64)
    live = np.abs(reff) > 1e-30                                    # (a fully decayed tail is stored as float32 zeros / denormals)
    assert live.mean() > 0.5 and np.max(np.abs(plf[:, :, ::dec] / reff - 1)[live]) < 2e-7
    assert np.max(np.abs(plf[:, :, :401] / gf["full_pl_head"][[0, 2]] - 1)) < 1e-12
    # what the fixture says about the reference's own speed (the figures DESIGN.md quotes)
    assert int(g["ntasks"]) == 8 and g["w8k_model_seconds"].shape == (3, 8)
    assert 5 < float(g["w8k_wall"]) < 600 and 20 < float(gf["full_wall"]) < 3600


def test_posterior_core_restatement_matches_the_reference(golden):
    """oracle/posterior.py against the outputs of the reference's own Visualization/utils.py functions
    (normalize, w_*, covariance, credible_interval, marginalize_1D/2D; golden made by gen_golden.py)."""
    from oracle import posterior as op
    g = golden("posterior")
    X, LL = op.filter_nan(g["X"], g["LL"])
    assert len(LL) == len(g["P"]) and np.isinf(LL).any()
    P = op.weights(LL, float(g["tf"]))
    assert np.array_equal(P, g["P"])
    cols = [np.log10(X[:, i]) if lg else X[:, i] for i, lg in zip(g["col_index"], g["col_log"])]
    for k, c in enumerate(cols):
        assert op.w_mean(c, P) == g["mean"][k] and op.w_variance(c, P) == g["var"][k]
        assert op.w_sample_std(c, P) == g["sstd"][k]
        assert np.isclose(op.w_skew(c, P), g["skew"][k], rtol=1e-14) and np.isclose(op.w_kurtosis(c, P), g["kurt"][k], rtol=1e-14)
        assert op.credible_interval(c, P) == tuple(g["ci"][k])
        dens, e = op.marginalize_1D(P, *g["limits"][k], int(g["bins"]), c, correct_sampling="mu" in str(g["names"][k]))
        assert np.array_equal(e, g["edges"][k]) and np.allclose(dens, g["h1"][k], rtol=1e-11, atol=1e-15)
    cov = np.array([[op.covariance(a, b, P) for b in cols] for a in cols])
    assert np.allclose(cov, g["cov"], rtol=1e-14, atol=0)
    for (a, b), h in zip(g["pairs"], g["h2"]):
        assert np.allclose(op.marginalize_2D(P, g["limits"][a], g["limits"][b], int(g["bins"]), cols[a], cols[b]), h,
                           rtol=1e-12, atol=1e-16)


def test_two_legitimate_evaluations_of_the_reference_part_company_as_the_floor_contract_says(oracle):
    """The goldens pin the reference as CPython executes it: IEEE operations, no fused multiply-add.  A compiler that
    contracts (numba-CUDA and nvcc do by default) evaluates the SAME source to slightly different states.  The oracle
    built with -ffp-contract=fast -mfma stands for that evaluation: against the pinned build it takes the same number of
    inner iterations on every system, its PL agrees to ~1e-12 while the excess carriers are there -- and loses digits
    exactly as include/trpl.h says a second evaluation does once they have decayed: |dPL / PL| <= 1e-9 + K / r, K = 5e-13,
    r = PL / (B L n0p0).  (What `floor_col` reports is a property of the arithmetic problem, not of this library.)"""
    import trpl_amd
    w = trpl_amd.workloads
    L, T, S = 128, 1600, 12
    Time = T * 0.025
    ini, lens = w.power_scan(L)
    X = w.samples(S, seed=7)
    rng = np.random.default_rng(3)
    X[:, 9] = 10 ** rng.uniform(np.log10(0.3), np.log10(3.0), S)        # short lifetimes: the decay reaches the floor
    X[:, 10] = X[:, 9] * 10 ** rng.uniform(-0.3, 0.3, S)
    c = 1
    ref = oracle.pvsim(X[:, :12], lens[c], Time, L, T, ini[c], nthreads=4)
    with oracle.fma_variant():
        alt = oracle.pvsim(X[:, :12], lens[c], Time, L, T, ini[c], nthreads=4)
    again = oracle.pvsim(X[:, :12], lens[c], Time, L, T, ini[c], nthreads=4)
    assert np.array_equal(again["plI"], ref["plI"])                       # the pinned build is back
    assert not np.array_equal(alt["plI"], ref["plI"])                     # the contracted build really differs
    assert np.array_equal(alt["iters_total"], ref["iters_total"]) and not ref["status"].any()
    dx = lens[c] / L
    scale = X[:, 4] * L * X[:, 0] * X[:, 1] * dx                          # B L n0p0 in the units of PL
    r = ref["plI"] / scale[:, None]
    dev = np.abs(alt["plI"] / ref["plI"] - 1)
    high = r >= 1.0
    assert high.any() and dev[high].max() < 1e-10                         # excess carriers present: rounding level
    physical = r >= 1e-10
    assert (r[:, -1] < 1e-6).sum() >= S // 2                              # most of these systems get deep into the decay
    assert (dev[physical] <= 1e-9 + 5e-13 / r[physical]).all()          # TRPL_PL_ENVELOPE_K_THICK (measured here: ~5e-15 / r)
    assert dev[(r < 1e-6) & physical].max() > 1e-8                        # ... and there the two evaluations do differ
