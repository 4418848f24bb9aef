"""The estimator of the log-evidence differences (trpl_amd.mcmc.log_evidence_ratios, pure numpy) on synthetic sums, the refusals of
posterior.log_evidence, the trimming of Tempered.log_evidence, and the restatement tests/mcmc_evidence_ref.py against itself and
against its recorded figures.  No GPU needed: whatever would reach the device is refused before, or K = 1, which makes no call."""
import numpy as np
import pytest

import mcmc_evidence_ref as er


def _synthetic(rng, tf, B, n, mu, s):
    """(ext, sums) of K rungs of B blocks of n iid N(mu, s^2) values each, formed as the header states, in plain numpy sums."""
    K = tf.size
    d = er.deltas(tf)
    x = rng.normal(mu, s, size=(K, B, n))
    ext = np.stack([x.max(axis=(1, 2)), x.min(axis=(1, 2))], axis=1)
    sums = np.zeros((K, B, 6))
    sums[:, :, 0], sums[:, :, 5] = x.sum(axis=2), n
    for k in range(K):
        cu, au, cd, ad = er.coefficients(tf, ext, k)
        for c, a, slot in ((cu, au, 1), (cd, ad, 3)):
            if c is not None:
                e = np.exp(c * (x[k] - a))
                sums[k, :, slot], sums[k, :, slot + 1] = e.sum(axis=1), (e * e).sum(axis=1)
    return ext, sums


@pytest.mark.parametrize("tf", ((1.0, 1.5, 2.5, 4.0, 8.0), (4.0, 1.0, 2.0)), ids=("rising", "unsorted"))
def test_ratios_on_gaussian_sums(trpl, tf):
    """iid LL ~ N(mu, s^2) on every rung: E exp(d LL) = exp(d mu + d^2 s^2 / 2), so forward estimates d mu + d^2 s^2 / 2, reverse
    d mu - d^2 s^2 / 2 and ti d mu; each within 5 of its own jackknife errors.  The unsorted ladder has deltas of both signs."""
    tf = np.array(tf)
    mu, s, B, n = -40.0, 2.0, 16, 2000
    ext, sums = _synthetic(np.random.default_rng(3), tf, B, n, mu, s)
    r = trpl.mcmc.log_evidence_ratios(ext, sums, tf)
    d = er.deltas(tf)
    assert np.array_equal(r["delta"], d) and np.array_equal(r["N"], np.full(tf.size, B * n)) and r["blocks"] == B
    for name, want in (("forward", d * mu + d * d * s * s / 2), ("reverse", d * mu - d * d * s * s / 2), ("ti", d * mu)):
        est, se = r[name], r[name + "_se"]
        print(name, np.round((est - want) / se, 2), se)
        assert est.shape == se.shape == (tf.size - 1,) and np.all(se > 0) and np.all(se < 0.05)
        assert np.all(np.abs(est - want) < 5.0 * se), (name, est, want, se)
        assert r[name + "_total"] == sum(est.tolist(), 0.0)      # added in ascending k from 0.0
        assert r[name + "_total_se"] == pytest.approx(np.sqrt(np.sum(se ** 2)), rel=1e-14)
    # the share of the states that carry a sum: exp(-d^2 s^2) for a Gaussian; a ratio of sampled moments of a log-normal, so a
    # loose check of the formula and its order (forward, reverse), not of a distribution
    assert r["term_ess"].shape == (tf.size - 1, 2)
    assert np.allclose(r["term_ess"], np.exp(-(d * s) ** 2)[:, None], rtol=0.25)


def test_one_block_has_no_error_and_one_rung_no_ratio(trpl):
    tf = np.array([1.0, 2.0, 4.0])
    ext, sums = _synthetic(np.random.default_rng(4), tf, 1, 500, -3.0, 1.0)
    r = trpl.mcmc.log_evidence_ratios(ext, sums, tf)
    for name in ("forward", "reverse", "ti"):
        assert np.all(np.isfinite(r[name])) and np.isnan(r[name + "_se"]).all() and np.isnan(r[name + "_total_se"])
    for B in (1, 4):
        r = trpl.mcmc.log_evidence_ratios(np.zeros((1, 2)), np.ones((1, B, 6)), [3.0])
        for name in ("forward", "reverse", "ti"):
            assert r[name].shape == r[name + "_se"].shape == (0,)
            assert r[name + "_total"] == 0.0 and r[name + "_total_se"] == 0.0 and isinstance(r[name + "_total"], float)
        assert r["term_ess"].shape == (0, 2)


def test_equal_temperatures_and_shape_refusals(trpl):
    """delta = 0 between two rungs: up = down = N, the difference is exactly 0.0 whatever the centres, even an infinite one."""
    tf = np.array([2.0, 2.0])
    ext = np.array([[-1.0, -np.inf], [-2.0, -9.0]])
    sums = np.zeros((2, 3, 6))
    sums[:, :, 0], sums[:, :, 5] = -50.0, 10.0
    sums[0, :, 3:5] = sums[1, :, 1:3] = 10.0
    r = trpl.mcmc.log_evidence_ratios(ext, sums, tf)
    for name in ("forward", "reverse", "ti"):
        assert r[name][0] == 0.0 and r[name + "_se"][0] == 0.0
    assert np.array_equal(r["term_ess"], [[1.0, 1.0]])
    for bad_ext, bad_sums, lad in ((np.zeros((3, 2)), sums, tf), (ext, np.zeros((2, 3, 5)), tf), (ext, np.zeros((2, 0, 6)), tf),
                                  (ext, np.zeros((2, 6)), tf), (ext, sums, [1.0, 2.0, 3.0])):
        with pytest.raises(ValueError, match="ext must be"):
            trpl.mcmc.log_evidence_ratios(bad_ext, bad_sums, lad)
    with pytest.raises(ValueError, match="LL must be"):
        trpl.mcmc.evidence_sums(np.zeros((2, 4)), tf)
    with pytest.raises(ValueError, match="LL must be"):
        trpl.mcmc.evidence_sums(np.zeros((3, 4, 2)), tf)
    with pytest.raises(trpl.TrplError, match="B=3"):             # the library's own refusal reaches Python
        trpl.mcmc.evidence_sums(np.zeros((2, 4, 2)), tf, blocks=3)


def test_posterior_log_evidence_refuses_bad_shapes(trpl):
    P = trpl.posterior
    for LL, tf, kw in ((np.zeros((2, 3)), 1.0, {}), (np.zeros(0), 1.0, {}), (np.zeros(5), np.ones((2, 2)), {}),
                       (np.zeros(5), np.ones(P.TF_SCAN_POINTS + 1), {}), (np.zeros(5), np.ones(0), {})):
        with pytest.raises(ValueError, match="LL must be|tf must be"):
            P.log_evidence(LL, tf, **kw)
    with pytest.raises(ValueError, match="log_ratio must have one entry per sample"):
        P.log_evidence(np.zeros(5), 1.0, log_ratio=np.zeros(4))


def _tempered(trpl, K, n, C=4):
    M = trpl.mcmc
    ladder = M.geometric_ladder(1.0, 8.0, K)
    chains = [M.Chains(np.zeros((n, C, 2)), np.zeros((n, C, 5)), -np.arange(n * C, dtype=np.float64).reshape(n, C) - k,
                       np.zeros((n, C), dtype=bool)) for k in range(K)]
    return M.Tempered(ladder, chains, np.full(K - 1, np.nan))


def test_tempered_log_evidence_trims_and_reports(trpl):
    """K = 1 makes no device call, so the trimming is visible here: the oldest kept sweeps after burn go until blocks divides."""
    t = _tempered(trpl, 1, 103)
    for burn, blocks, dropped in ((0, 16, 7), (3, 10, 0), (4, 10, 9), (0, 103, 0), (100, 1, 0), (0, 1, 0)):
        r = t.log_evidence(burn=burn, blocks=blocks)
        assert (r["dropped"], r["t0"], r["t1"], r["blocks"]) == (dropped, burn + dropped, 103, blocks)
        assert r["forward_total"] == r["reverse_total"] == r["ti_total"] == 0.0 and "ln_z" not in r
    for burn, blocks in ((0, 104), (100, 4), (0, 0), (-1, 4), (103, 1)):
        with pytest.raises(ValueError, match="blocks=%d" % blocks):
            t.log_evidence(burn=burn, blocks=blocks)
    t3 = _tempered(trpl, 3, 20)
    for base in ((np.zeros(8), 7.999), (np.zeros(8), 1.0, None)):
        with pytest.raises(ValueError, match="tf_hot_check"):
            t3.log_evidence(base=base)
    with pytest.raises(ValueError, match="base must be"):
        t3.log_evidence(base=(np.zeros(8),))


def test_the_restatement_agrees_with_itself():
    """The fp64 form and the long-double form of the sums; the tree against a plain sum; the rule of -inf, zero and NaN."""
    K, C, B = 3, 257, 2
    tf = np.array([1.0, 3.0, 2.0])                               # deltas of both signs
    LL = er.case_LL(K, C, B)
    t0, t1 = er.T0, er.T0 + B * er.case_w(C)
    ext, s = er.sums(LL, tf, t0, t1, B)
    sl = er.sums_long(LL, tf, t0, t1, B)
    assert np.isfinite(s).all() and np.all(s[0, :, 1:3] == 0.0) and np.all(s[-1, :, 3:5] == 0.0)
    assert np.all(np.abs(s - sl) <= er.sums_rtol(er.case_w(C), C) * np.abs(sl))
    assert np.all(s[:, :, 1] <= s[:, :, 5]) and np.all(s[:, :, 3] <= s[:, :, 5])        # no exponent is positive
    assert s[1, :, 1].max() >= 1.0 or s[1, :, 3].max() >= 1.0                            # and the centre's own term is 1
    LL[1, t0 + 1, 3] = -np.inf
    LL[2, t0, 0] = np.nan
    ext, s = er.sums(LL, tf, t0, t1, B)
    assert np.isnan(ext[2]).all() and np.isnan(s[2]).all() and np.isfinite(ext[0]).all() and np.isfinite(s[0]).all()
    assert ext[1, 1] == -np.inf and s[1, 0, 0] == -np.inf and s[1, 0, 5] == er.case_w(C) * C - 1
    # rung 1: up has delta_0 = 1 - 1/3 > 0 (the -inf gives 0), down has -delta_1 = -(1/3 - 1/2) > 0 (it gives 0 too)
    assert np.isfinite(s[1, :, 1:5]).all()
    tf2 = np.array([3.0, 1.0, 2.0])                              # now up of rung 1 has a negative coefficient
    assert er.sums(LL, tf2, t0, t1, B)[1][1, 0, 1] == np.inf
    assert er.tree_sum(np.arange(1000.0)) == 499500.0 and er.tree_sum([]) == 0.0


def test_the_recorded_figures_are_the_restatement_and_meet_their_own_gates(trpl):
    """The first seed recomputed (2 s of numpy); every recorded figure lies within the gate the device test applies."""
    got = er.gauss_restatement(er.GA_SEEDS[0], trpl.mcmc.log_evidence_ratios)
    assert np.allclose(got, er.GA_RESTATEMENT[0], rtol=1e-12, atol=0), (got, er.GA_RESTATEMENT[0])
    gates = er.gauss_gates()
    rec = np.array(er.GA_RESTATEMENT)
    for i, name in enumerate(("forward", "reverse", "ti")):
        target, margin = gates[name]
        assert 0.0 < margin < 0.2 and np.all(np.abs(rec[:, i] - target) < margin), (name, target, margin)
        target, margin = gates["ln_z_" + name]
        assert np.all(np.abs(rec[:, i] + rec[:, 3] - target) < margin), (name, target, margin)
    # truncation at the faces is far below the gates, and ti's target is its own: the trapezoid's bias is 0.06
    stone, ti = er.gauss_targets(trpl.mcmc.geometric_ladder(1.0, er.GA_HOT, er.GA_K))
    assert abs(stone - 1.5 * np.log(1.0 / er.GA_HOT)) < 1e-4 and 0.05 < stone - ti < 0.08
