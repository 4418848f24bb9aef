"""trpl_amd.mcmc.ess_from_sums, the estimator of the effective sample size, on sums made by the restatement (tests/mcmc_ess_ref.py).
No GPU needed: the estimator is numpy, and the sums here are the sequential loops.

The statistical case: stationary AR(1) sequences, 32 x 256 steps, 128 lags, seeds 0 .. 7.  The ratio tau / ((1 + phi) / (1 - phi)) of
the RESTATEMENT over the eight seeds has mean 0.9917, sd 0.0196 at phi = 0 and mean 0.9772, sd 0.0468 at phi = 0.5 (mcmc_ess_ref.AR1_RATIO,
made by `python tests/mcmc_ess_ref.py`); the package's value is gated at mean +- 5 sd.  No seed is truncated at either phi.

phi = 0.9: with this generator and the rule as include/trpl.h states it, NONE of the seeds 0 .. 7 is truncated at 128 lags (ratios
0.85 .. 1.20): around lag 50 the pooled autocorrelation has decayed to the size of its noise and a pair turns non-positive long
before the lags run out.  So at 128 lags the flag is asserted to be the restatement's, seed by seed, and truncated = True is asserted
where the lags do run out first: the same sequences with 16 lags, where every pair is at least rho[14] + rho[15] = 0.9^14 + 0.9^15 =
0.43 in expectation, many times the noise.  Nothing is gated on tau at phi = 0.9."""
import numpy as np
import pytest

import mcmc_ess_ref as er


def _sums_from_rho(rho, M=4, m=100):
    """(mean, m2, pooled) of M sequences of m steps that give back exactly this rho (L,) -- up to rounding: equal means (B = 0), m2 =
    m - 1 (W = 1), so var+ = (m - 1) / m and rho[l] = 1 - (1 - acov[l]) / var+."""
    rho = np.asarray(rho, dtype=np.float64)
    var_plus = (m - 1) / m
    acov = 1.0 - (1.0 - rho) * var_plus
    return np.zeros((M, 1)), np.full((M, 1), m - 1.0), (acov * M * m)[:, None]


def test_the_geyer_rule_by_hand(trpl):
    ess_from_sums = trpl.mcmc.ess_from_sums
    M, m = 4, 100
    floor = 1.0 / np.log10(M * m)
    # pairs 1.5, 0.5, -0.1: the sum stops at the first non-positive pair; tau = -1 + 2 (1.5 + 0.5) = 3
    ess, info = ess_from_sums(*_sums_from_rho([1.0, 0.5, 0.3, 0.2, -0.2, 0.1], M, m), m)
    assert info["K"][0] == 2 and not info["truncated"][0]
    assert np.allclose(info["tau"], 3.0, rtol=1e-12) and np.allclose(ess, M * m / 3.0, rtol=1e-12)
    assert np.allclose(info["rho"][:, 0], [1.0, 0.5, 0.3, 0.2, -0.2, 0.1], rtol=0, atol=1e-12)
    assert np.allclose(info["var_plus"], (m - 1) / m, rtol=1e-15)
    # pairs 1.2, 0.3, 0.5: the third may not exceed the second (running minimum); no pair fails, so the lags truncated the sum;
    # tau = -1 + 2 (1.2 + 0.3 + 0.3) = 2.6
    ess, info = ess_from_sums(*_sums_from_rho([1.0, 0.2, 0.2, 0.1, 0.3, 0.2], M, m), m)
    assert info["K"][0] == 3 and info["truncated"][0]
    assert np.allclose(info["tau"], 2.6, rtol=1e-12) and np.allclose(ess, M * m / 2.6, rtol=1e-12)
    # the first pair 1 - 0.8 = 0.2: tau = -0.6 is below the floor 1 / log10(M m); the second pair is negative
    ess, info = ess_from_sums(*_sums_from_rho([1.0, -0.8, 0.25, -0.3, 0.9, 0.9], M, m), m)
    assert info["K"][0] == 1 and not info["truncated"][0]
    assert info["tau"][0] == floor and ess[0] == M * m / floor and ess[0] > M * m
    # the first pair fails at once: K = 0, the floor again
    ess, info = ess_from_sums(*_sums_from_rho([1.0, -1.5, 0.9, 0.9, 0.9, 0.9], M, m), m)
    assert info["K"][0] == 0 and not info["truncated"][0] and info["tau"][0] == floor
    # rho[0] is 1 whatever the sums say; an odd last lag joins no pair
    mean, m2, pooled = _sums_from_rho([0.7, 0.5, 0.3, 0.2, 0.9], M, m)
    ess, info = ess_from_sums(mean, m2, pooled, m)
    assert info["rho"][0, 0] == 1.0 and info["K"][0] == 2 and info["truncated"][0] and np.allclose(info["tau"], 3.0, rtol=1e-12)
    # one lag: no pair at all
    ess, info = ess_from_sums(mean, m2, pooled[:1], m)
    assert info["K"][0] == 0 and info["truncated"][0] and info["tau"][0] == floor
    # a NaN pair fails P > 0; columns are judged one by one; the flat (M A,) layout is sequence-major
    a = _sums_from_rho([1.0, 0.5, np.nan, 0.2, 0.1, 0.1], M, m)
    b = _sums_from_rho([1.0, 0.2, 0.2, 0.1, 0.3, 0.2], M, m)
    mean, m2, pooled = (np.concatenate([x, y], axis=1) for x, y in zip(a, b))
    ess, info = ess_from_sums(mean.reshape(-1), m2.reshape(-1), pooled, m)
    assert list(info["K"]) == [1, 3] and list(info["truncated"]) == [False, True]
    assert np.allclose(info["tau"], [2.0, 2.6], rtol=1e-12)
    # the restatement's scalar rule says the same of each of these
    for rho, want in (([1.0, 0.5, 0.3, 0.2, -0.2, 0.1], (3.0, 2, False)), ([1.0, 0.2, 0.2, 0.1, 0.3, 0.2], (2.6, 3, True)),
                      ([1.0, -0.8, 0.25, -0.3, 0.9, 0.9], (floor, 1, False))):
        tau, K, trunc = er.geyer(np.array(rho), M * m)
        assert np.isclose(tau, want[0], rtol=1e-12) and (K, trunc) == want[1:]


def test_between_chain_variance_enters_var_plus(trpl):
    """Sequences of equal spread about different means: B / m = var(means, ddof 1) lifts var+ above W and every rho with it."""
    m, M = 50, 3
    x = er.ar1(0.0, m, M, 11)
    x += np.array([0.0, 2.0, 4.0])[None, :, None]
    want_ess, want = er.ess(x, 10)
    ess, info = trpl.mcmc.ess_from_sums(want["mean"], want["m2"], want["pooled"], m)
    W = np.mean(want["m2"] / (m - 1))
    assert np.allclose(info["var_plus"], (m - 1) / m * W + np.var(want["mean"], ddof=1), rtol=1e-14)
    assert info["var_plus"][0] > 4.0 and np.all(info["rho"][:, 0] > 0.7)          # the offsets dominate: nothing decorrelates
    assert np.allclose(ess, want_ess, rtol=1e-12) and info["truncated"][0] and ess[0] < M * m / 5
    one, info1 = trpl.mcmc.ess_from_sums(want["mean"][:1], want["m2"][:1], er.pool(er.autocov(x[:, 0], 0, m, 10)[1], 1, 1), m)
    assert np.isfinite(one[0]) and np.allclose(info1["var_plus"], (m - 1) / m * want["m2"][0] / (m - 1), rtol=1e-14)      # M = 1: B = 0


def test_rho_is_the_autocorrelation_of_the_definition(trpl):
    """One sequence: pooled[l] / m is the biased autocovariance np.correlate gives, and rho[l] = 1 - (W - acov[l]) / var+ with W =
    np.var(x, ddof=1) and, for M = 1 (B = 0), var+ = (m - 1) / m W = acov[0]: the textbook acov[l] / acov[0] less 1 / (m - 1), to
    1e-12."""
    m, L = 200, 60
    x = er.ar1(0.7, m, 1, 5)
    mean, s = er.autocov(x.reshape(m, 1), 0, m, L)
    e = x[:, 0, 0] - x[:, 0, 0].mean()
    acov = np.correlate(e, e, mode="full")[m - 1:m - 1 + L] / m
    assert np.allclose(s[:, 0] / m, acov, rtol=0, atol=1e-12)
    W = np.var(x[:, 0, 0], ddof=1)
    direct = 1.0 - (W - acov) / ((m - 1) / m * W)
    direct[0] = 1.0
    ess, info = trpl.mcmc.ess_from_sums(mean, s[0], er.pool(s, 1, 1), m)
    assert np.allclose(info["rho"][:, 0], direct, rtol=0, atol=1e-12)
    assert np.allclose(info["rho"][1:, 0], acov[1:] / acov[0] - 1.0 / (m - 1), rtol=0, atol=1e-12)
    want_ess, want = er.ess(x, L)
    assert np.allclose(info["rho"], want["rho"], rtol=0, atol=1e-12) and np.allclose(ess, want_ess, rtol=1e-12)


@pytest.fixture(scope="module")
def ar1_sums():
    """The restatement's sums and estimates of every (phi, seed) of the statistical case, made once."""
    S = er.AR1_SHAPE
    out = {}
    for phi in (0.0, 0.5, 0.9):
        for seed in S["seeds"]:
            out[phi, seed] = er.ess(er.ar1(phi, S["m"], S["M"], seed), S["L"])
    return out


@pytest.mark.parametrize("phi", (0.0, 0.5))
def test_ar1_tau_is_the_theory_within_the_restatements_spread(trpl, ar1_sums, phi):
    S = er.AR1_SHAPE
    theory = (1.0 + phi) / (1.0 - phi)
    ref = np.array([ar1_sums[phi, seed][1]["tau"][0] / theory for seed in S["seeds"]])
    assert np.isclose(ref.mean(), er.AR1_RATIO[phi][0], rtol=0, atol=1e-5) and np.isclose(ref.std(ddof=1), er.AR1_RATIO[phi][1], rtol=0, atol=1e-5)
    mean, sd = er.AR1_RATIO[phi]
    for seed in S["seeds"]:
        want_ess, want = ar1_sums[phi, seed]
        ess, info = trpl.mcmc.ess_from_sums(want["mean"], want["m2"], want["pooled"], S["m"])
        ratio = info["tau"][0] / theory
        print("phi=%g seed=%d: tau / theory = %.4f (gate %.4f .. %.4f), ess %.0f of %d" % (phi, seed, ratio, mean - 5 * sd, mean + 5 * sd,
                                                                                         ess[0], S["m"] * S["M"]))
        assert not info["truncated"][0] and not want["truncated"][0]
        assert mean - 5.0 * sd <= ratio <= mean + 5.0 * sd
        assert np.allclose(ess, want_ess, rtol=1e-12) and info["K"][0] == want["K"][0]
        assert np.allclose(ess * info["tau"], S["m"] * S["M"], rtol=1e-14)


def test_ar1_truncated_flag_at_phi_09(trpl, ar1_sums):
    S = er.AR1_SHAPE
    for seed in S["seeds"]:
        want_ess, want = ar1_sums[0.9, seed]
        ess, info = trpl.mcmc.ess_from_sums(want["mean"], want["m2"], want["pooled"], S["m"])
        assert info["truncated"][0] == want["truncated"][0] and info["K"][0] == want["K"][0]          # 128 lags: the restatement's flag
        assert info["K"][0] < S["L"] // 2 or info["truncated"][0]
        # 16 lags of the same sums: every pair is positive, the lags run out first
        short, sinfo = trpl.mcmc.ess_from_sums(want["mean"], want["m2"], want["pooled"][:16], S["m"])
        assert sinfo["truncated"][0] and sinfo["K"][0] == 8
        assert er.geyer(want["rho"][:16, 0], S["m"] * S["M"])[2]
        assert short[0] >= ess[0]                                # the truncated sum is an upper bound of the ESS
        print("phi=0.9 seed=%d: 128 lags K=%d truncated=%s tau=%.2f; 16 lags truncated=%s tau=%.2f" % (
            seed, info["K"][0], info["truncated"][0], info["tau"][0], sinfo["truncated"][0], sinfo["tau"][0]))
