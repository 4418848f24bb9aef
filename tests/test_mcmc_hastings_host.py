"""The restatement of the Metropolis-Hastings kernels alone (tests/mcmc_hastings_ref.py): the early-rejection level with h is safe
on the 10^5-draw set and the edge set of mcmc_levels_ref crossed with h in {0, +-1e-3, +-5, +-700}; h = 0 reproduces mcmc_ref and
mcmc_levels_ref bit for bit; the stretch move samples a 10-D Gaussian, and the same gate refuses the move without its Hastings term;
the figures the device test is gated by are this restatement's.  No GPU, no library."""
import numpy as np
import pytest

import mcmc_hastings_ref as hr
import mcmc_levels_ref as lr
import mcmc_ref as mr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _proposals_at(level):
    """For every finite level the likelihoods a cut proposal can report: -level itself, the next double below, and far below."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = -level
        return [q, np.nextafter(q, -np.inf), q - np.abs(q) * 1e-9 - 1e-300, q - 1.0, q * 2.0 - 1.0, np.full_like(q, -1e300)]


@pytest.mark.parametrize("h", hr.H_VALUES)
def test_no_proposal_at_or_below_the_level_is_accepted(h):
    LL, tf, chains, steps = lr.random_inputs()
    xi = lr.accept_uniform_at(chains, steps, lr.SEED)
    eLL, etf, exi = lr.edge_inputs()
    LL, tf, xi = np.concatenate([LL, eLL]), np.concatenate([tf, etf]), np.concatenate([xi, exi])
    with np.errstate(divide="ignore"):
        lx0 = np.log(xi)
    finite_total = 0
    for shift in (0, 1, -1, 2, -2):                              # any rounding of the logarithm within two ulp
        lx = lx0.copy()
        for _ in range(abs(shift)):
            lx = np.nextafter(lx, np.inf if shift > 0 else -np.inf)
        level = hr.levels_h_from_log(LL, tf, xi, lx, h)
        fin = np.isfinite(level)
        finite_total += int(fin.sum())
        for LLp in _proposals_at(level):
            ok = fin & (LLp <= -level)
            assert not hr.accept_take_h(LL, LLp, tf, h, lx)[ok].any()
        # +inf exactly where the rule says so, or where neither candidate verifies: never a NaN
        assert not np.isnan(level).any()
        assert np.all(np.isinf(level[np.isnan(LL) | ~(LL > -np.inf) | (xi == 0.0)]))
    # the levels are there: with h >= -1e-3 at least 98 % of the draws are given one.  (Further below zero the first candidate is often
    # negative, where the second candidate's step (|LL| + l0) 2^-40 points the wrong way: 81 % at h = -5, 65 % at -700 -- fewer
    # levels, none of them unsafe.)
    assert finite_total > (4.9 if h >= -1e-3 else 0) * lr.N_RANDOM


def test_an_h_that_is_nan_or_infinite_gives_no_level_and_h_zero_is_the_plain_rule():
    LL, tf, chains, steps = lr.random_inputs()
    xi = lr.accept_uniform_at(chains, steps, lr.SEED)
    lx = np.log(xi)
    for h in (np.nan, np.inf, -np.inf):
        assert np.all(hr.levels_h_from_log(LL, tf, xi, lx, h) == np.inf)
    eLL, etf, exi = lr.edge_inputs()
    for a, b, c in ((LL, tf, xi), (eLL, etf, exi)):
        with np.errstate(divide="ignore"):
            l = np.log(c)
        for zero in (0.0, -0.0):
            assert np.array_equal(_bits(hr.levels_h_from_log(a, b, c, l, zero)), _bits(lr.levels_from_log(a, b, c, l)))
    rng = np.random.default_rng(3)
    LLp = LL + 3.0 * tf * rng.normal(size=LL.size)
    assert np.array_equal(hr.accept_take_h(LL, LLp, tf, 0.0, lx), lr.accept_take(LL, LLp, tf, xi))
    for count, chain0 in lr.DEVICE_CASES:
        for k in (1, 2):
            if count % k == 0:
                ladder = np.array([1.0, 37.5])[:k]
                case = lr.device_case(count, chain0, 1.0)
                want = np.concatenate([lr.levels(case[r * (count // k):(r + 1) * (count // k)], ladder[r], chain0 + r * (count // k), lr.SEED, 5)
                                       for r in range(k)])
                assert np.array_equal(_bits(hr.levels_h(case, np.zeros(count), ladder, chain0, lr.SEED, 5)), _bits(want))


@pytest.mark.parametrize("count", mr.ACCEPT_COUNTS)
def test_accept_with_h_zero_is_mcmc_ref_and_the_edge_values_follow_the_rule(count):
    for tf in mr.ACCEPT_TFS:
        U, X, LL, Up, Xp, LLp, inside = mr.accept_case(count, tf)
        wU, wX, wLL, wacc, margin = mr.accept(U, X, LL, Up, Xp, LLp, inside, tf, 3, mr.ACCEPT_SEED, 1)
        gU, gX, gLL, gacc = hr.accept_h(U, X, LL, Up, Xp, LLp, inside, np.zeros(count), tf, 3, mr.ACCEPT_SEED, 1)
        same = margin > mr.MARGIN                                # mcmc_ref decides in longdouble: the float64 log agrees off the margin
        assert np.array_equal(gacc[same], wacc[same]) and same.mean() >= 0.99
        if same.all():
            for g, w in ((gU, wU), (gX, wX), (gLL, wLL)):
                assert np.array_equal(_bits(g), _bits(w)) or np.array_equal(np.isnan(g), np.isnan(w))
        plain = hr.accept_h(U, X, LL, Up, Xp, LLp, inside, np.zeros(count), tf, 3, mr.ACCEPT_SEED, 1)[3]
        valid = (inside != 0) & ~np.isnan(LLp) & (LLp > -np.inf)
        for edge in hr.H_EDGES:
            acc = hr.accept_h(U, X, LL, Up, Xp, LLp, inside, np.full(count, edge), tf, 3, mr.ACCEPT_SEED, 1)[3]
            if np.isnan(edge) or edge == -np.inf:
                assert not acc.any()
            elif edge == np.inf:                                 # d = +inf, or a NaN where (LLp - LL) / tf is -inf
                with np.errstate(invalid="ignore"):
                    d = (LLp - LL) / tf + np.inf
                assert np.array_equal(acc != 0, valid & (~(LL > -np.inf) | (d >= 0.0)))
            else:
                assert np.array_equal(acc, plain)                # -0.0 is +0.0 to every comparison


def test_the_prior_term_and_the_stretch_are_their_expressions():
    rng = np.random.default_rng(8)
    U, Up = rng.random((50, 3)), rng.random((50, 3)) * 3.0 - 1.0
    mean, sd = np.array([0.2, 0.5, -1.0]), np.array([0.1, np.inf, 2.0])
    h = hr.prior_term(U, Up, mean, sd)
    want = (-0.5 * ((Up[:, [0, 2]] - mean[[0, 2]]) / sd[[0, 2]]) ** 2).sum(axis=1) - (-0.5 * ((U[:, [0, 2]] - mean[[0, 2]]) / sd[[0, 2]]) ** 2).sum(axis=1)
    assert np.allclose(h, want, rtol=1e-12, atol=1e-13)
    flat = hr.prior_term(U, Up * np.nan, mean, np.full(3, np.inf))
    assert np.array_equal(_bits(flat), _bits(np.zeros(50)))      # exactly +0.0, whatever u is
    assert np.array_equal(_bits(hr.prior_term(U, Up, mean, sd, h=np.full(50, 1.5))), _bits(1.5 + (h - 0.0)))
    # the stretch: z in [1 / a, a), the partner inside the chain's rung, u' on the line through p and u
    partners = rng.random((60, 3))
    U = rng.random((60, 3))
    for a in (2.0, 1.5, 7.0):
        Up, inside, z, row = hr.stretch_unit(U, partners, 20, a, (1 << 32) + 1, 5, 9)
        assert np.all((z >= 1.0 / a) & (z < a)) and np.array_equal(row // 20, np.arange(60) // 20) and len(set(row)) > 20
        assert np.allclose(Up - partners[row], z[:, None] * (U - partners[row]), rtol=1e-13, atol=1e-15)
        assert np.array_equal(inside, np.all((Up >= 0) & (Up <= 1), axis=1))
    # the density of z is proportional to 1 / sqrt(z): its distribution function is (sqrt(a z) - 1) / (a - 1), uniform in xi
    _, _, z, _ = hr.stretch_unit(np.zeros((4000, 1)), np.ones((4000, 1)), None, 2.0, 0, 1, 0)
    cdf = np.sort((np.sqrt(2.0 * z) - 1.0) / (2.0 - 1.0))
    assert np.max(np.abs(cdf - (np.arange(4000) + 0.5) / 4000)) < 1.63 / np.sqrt(4000)      # Kolmogorov's 1 % point


# ------------------------------------------------------------------ the stretch move samples what it should
TEN = dict(A=10, sd=0.08, C=64, sweeps=600, seed=5, batches=10)


def _ten_d(use_lnq):
    """The ensemble means, sweep by sweep over the kept half, of u and of (u - 1/2)^2 averaged over the 64 chains and the 10
    coordinates of an isotropic Gaussian of deviation 0.08 centred in the cube; every level formed on the way is checked."""
    A, sd = TEN["A"], TEN["sd"]

    def loglik(U):
        return -0.5 * np.sum((np.asarray(U) - 0.5) ** 2, axis=1) / sd ** 2

    box = (np.zeros(A), np.ones(A), np.zeros(A, dtype=np.int32))
    U0 = 0.5 + sd * np.random.default_rng(TEN["seed"]).normal(size=(TEN["C"], A))
    res = hr.run(loglik, U0, loglik(U0), *box, sweeps=TEN["sweeps"], seed=TEN["seed"], use_lnq=use_lnq, levels_check=True)
    kept = res["U"][0, TEN["sweeps"] // 2:]
    return kept.mean(axis=(1, 2)), ((kept - 0.5) ** 2).mean(axis=(1, 2))


def _gate(series, truth):
    """(error, 5 standard errors): the standard error of the series' mean by batch means -- the kept sweeps in 10 batches of 30, far
    longer than the move's autocorrelation time in 10 dimensions, so the batch means are nearly independent and their spread
    (ddof = 1) over sqrt(10) estimates the error of the whole mean."""
    b = series.reshape(TEN["batches"], -1).mean(axis=1)
    return abs(series.mean() - truth), 5.0 * b.std(ddof=1) / np.sqrt(TEN["batches"])


def test_the_stretch_move_samples_a_ten_dimensional_gaussian_and_the_gate_sees_the_hastings_term():
    m1, m2 = _ten_d(True)
    (e1, g1), (e2, g2) = _gate(m1, 0.5), _gate(m2, TEN["sd"] ** 2)
    print("10-D stretch: mean off by %.2e (gate %.2e), variance off by %.2e (gate %.2e), deviation %.5f"
          % (e1, g1, e2, g2, np.sqrt(m2.mean())))
    assert e1 < g1 and e2 < g2
    assert g2 < 0.1 * TEN["sd"] ** 2                              # the gate is worth something: a tenth of the variance
    w1, w2 = _ten_d(False)                                        # without z^(A - 1) the ensemble collapses towards its centre
    e, g = _gate(w2, TEN["sd"] ** 2)
    print("10-D stretch without lnq: variance off by %.2e (gate %.2e), deviation %.5f" % (e, g, np.sqrt(w2.mean())))
    assert not e < g


def test_the_figures_of_the_device_test_are_the_restatement_s():
    """The first seed of the stretch toy's eight, recomputed; the gates that follow from the eight; the gate can tell the move without
    its Hastings term apart."""
    got = hr.toy_stats(hr.stretch_toy_run(hr.STRETCH_SEEDS[0]))
    assert np.allclose(got, hr.STRETCH_STATS[0], rtol=1e-9, atol=0)
    lo, hi = hr.stretch_gates()
    assert np.all(lo < np.array([0.5, mr.TOY_SD, mr.TOY_RHO])) and np.all(np.array([0.5, mr.TOY_SD, mr.TOY_RHO]) < hi)
    wrong = np.array(hr.toy_stats(hr.stretch_toy_run(hr.STRETCH_SEEDS[0], use_lnq=False)))
    assert not np.all((lo < wrong) & (wrong < hi))


def test_the_prior_toy_of_the_device_test_in_the_restatement():
    """kind="de" under a flat likelihood and the half-Gaussian prior: the two moments within the device test's gates."""
    t = hr.PRIOR_TOY
    U0 = np.random.default_rng([t["seed"], 1]).random((t["C"], 2))
    res = hr.run(hr.flat_loglik, U0, np.zeros(t["C"]), *hr.PRIOR_BOX, sweeps=t["sweeps"], seed=t["seed"], kind="de", prior=hr.PRIOR)
    kept = res["U"][0, t["sweeps"] // 2:, :, 0]
    for series, truth in ((kept.mean(axis=1), hr.PRIOR_M1), ((kept ** 2).mean(axis=1), hr.PRIOR_M2)):
        err, gate = hr.prior_gate(series, truth)
        print("prior toy: moment %.5f, truth %.5f, off by %.2e (gate %.2e)" % (series.mean(), truth, err, gate))
        assert err < gate
    flat = res["U"][0, t["sweeps"] // 2:, :, 1]                  # the flat column stays uniform
    assert abs(flat.mean() - 0.5) < 0.02
