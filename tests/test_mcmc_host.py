"""The ensemble Metropolis sampler as tests/mcmc_ref.py restates it (trpl_mcmc_*, include/trpl.h), alone, with its Philox stream, on
two toys: 3-D Gaussians of deviation 0.08 centred in the cube, one isotropic and one with correlation 0.99.  256 chains, 400
sweeps, the first 200 dropped, seeds 0 .. 3.  No GPU, no library.

Measured with this stream (per coordinate, over the four seeds):
    isotropic,  de:      |mean - 1/2| <= 0.034 sd, sd ratio 0.990 .. 1.011, acceptance 0.32, R-hat <= 1.057
    isotropic,  rw 0.1:  |mean - 1/2| <= 0.022 sd, sd ratio 0.986 .. 1.010, acceptance 0.55, R-hat <= 1.079
    correlated, de:      |mean - 1/2| <= 0.021 sd, sd ratio 0.987 .. 1.006, corr 0.990, acceptance 0.32, R-hat <= 1.052
    correlated, rw 0.1:  acceptance 0.03, R-hat 2.8 .. 2.9 (it has not converged: the walk is as wide as the ridge is long)
The bounds below were set before these were taken (from a prototype on numpy's generator) and leave room."""
import numpy as np
import pytest

import mcmc_ref as mr
import refine_ref as rr

C, SWEEPS, BURN, SEEDS = 256, 400, 200, (0, 1, 2, 3)
_runs = {}


def _run(rho, kind, seed):
    """One run per (toy, proposal, seed), shared by the tests."""
    key = (rho, kind, seed)
    if key not in _runs:
        ll, cov = mr.toy(rho)
        U0 = mr.toy_start(C, seed)
        lo, hi, lg = mr.CUBE
        r = mr.run(ll, U0, ll(U0), lo, hi, lg, sweeps=SWEEPS, kind=kind, scale=0.1 if kind == "rw" else None, seed=seed)
        S = r["U"][BURN:].reshape(-1, mr.TOY_A)
        sd = np.sqrt(np.diag(cov))
        _runs[key] = dict(mean=np.abs(S.mean(axis=0) - 0.5) / sd, sd=S.std(axis=0) / sd, corr=np.corrcoef(S.T),
                          accept=float(r["accepted"][BURN:].mean()), rhat=mr.rhat(r["U"], BURN), margin=r["margin"])
    return _runs[key]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("rho", (0.0, mr.TOY_RHO))
def test_differential_evolution_samples_both_toys(rho, seed):
    r = _run(rho, "de", seed)
    print("rho %.2f seed %d: |mean - 1/2| / sd %s, sd ratio %s, acceptance %.3f, R-hat %s" % (rho, seed, r["mean"], r["sd"], r["accept"],
                                                                                             r["rhat"]))
    assert np.all(r["mean"] <= 0.15), r["mean"]
    assert np.all((r["sd"] >= 0.9) & (r["sd"] <= 1.1)), r["sd"]
    if rho:
        off = r["corr"][~np.eye(mr.TOY_A, dtype=bool)]
        assert np.all(off >= 0.98), off
    assert np.all(r["rhat"] <= 1.1), r["rhat"]
    assert 0.15 <= r["accept"] <= 0.6, r["accept"]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_walk_samples_the_isotropic_toy(seed):
    r = _run(0.0, "rw", seed)
    print("seed %d: |mean - 1/2| / sd %s, sd ratio %s, acceptance %.3f" % (seed, r["mean"], r["sd"], r["accept"]))
    assert np.all(r["mean"] <= 0.15), r["mean"]
    assert np.all((r["sd"] >= 0.9) & (r["sd"] <= 1.1)), r["sd"]


@pytest.mark.parametrize("seed", SEEDS)
def test_differential_evolution_converges_faster_on_the_ridge(seed):
    de, rw = _run(mr.TOY_RHO, "de", seed), _run(mr.TOY_RHO, "rw", seed)
    print("seed %d: worst R-hat de %.3f, rw %.3f" % (seed, de["rhat"].max(), rw["rhat"].max()))
    assert de["rhat"].max() < rw["rhat"].max()


@pytest.mark.parametrize("P", (2, 3, 1000))
def test_partner_indices_are_distinct_and_in_range(P):
    for chain0, step in ((0, 0), (5, 3), ((1 << 32) + 5, 7)):
        a, b = mr.partner_indices(4096, P, chain0, 11, step)
        assert np.all(a != b)
        assert a.min() >= 0 and a.max() < P and b.min() >= 0 and b.max() < P
        if P <= 3:                                               # every ordered pair occurs
            assert len(set(zip(a.tolist(), b.tolist()))) == P * (P - 1)


def test_the_streams_are_apart():
    """One seed, step = generation: the uniforms of the proposal, of the partner choice, of the acceptance and of the refinement
    draw share no value."""
    n, seed, step = 1000, 7, 2
    xi = mr.uniforms(n, 16, 0, seed, step)
    r = mr._philox(0, n, mr.PARTNER_CALL, seed, step)
    partner = np.stack([rr.res53(r[:, 0], r[:, 1]), rr.res53(r[:, 2], r[:, 3])], axis=1)
    acc = mr.accept_uniform(n, 0, seed, step)
    draw = rr.uniforms(n, 16, seed, step)
    sets = [set(a.ravel().tolist()) for a in (xi, partner, acc, draw)]
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            assert not sets[i] & sets[j], (i, j)
    assert not np.any(xi == draw)
    # another chain0 shifts the stream: chain n of the ensemble has one stream wherever its call starts
    assert np.array_equal(mr.uniforms(10, 3, 5, seed, step), mr.uniforms(15, 3, 0, seed, step)[5:])


def test_accept_rule_branches():
    """Every clause of the rule on hand-made inputs (the uniform only decides the last row)."""
    inf, nan = np.inf, np.nan
    #              inside LL    LLp
    rows = [(1, 0.0, 1.0),      # d > 0: taken
            (1, 0.0, 0.0),      # d == 0: taken
            (0, 0.0, 1e9),      # outside: never
            (1, 0.0, nan),      # LLp NaN: never
            (1, 0.0, -inf),     # LLp -inf: never
            (1, 0.0, inf),      # LLp +inf: taken
            (1, nan, -5.0),     # the chain stands on NaN: taken
            (1, -inf, -5.0),    # ... on -inf: taken
            (1, -inf, -inf),    # ... but not to -inf
            (1, inf, inf),      # d NaN: not taken
            (1, 0.0, -1e9)]     # hopeless
    inside, LL, LLp = (np.array(c) for c in zip(*rows))
    take, margin = mr.accept_decision(LL, LLp, inside, 1.0, 0, 3, 0)
    assert take.tolist() == [True, True, False, False, False, True, True, True, False, False, False]
    assert np.isfinite(margin[-1]) and np.all(np.isinf(margin[:-1]))


def test_chain_stats_and_rhat():
    rng = np.random.default_rng(0)
    H = rng.normal(size=(40, 6))
    mean, m2 = mr.chain_stats(H, 3, 33)
    assert np.allclose(mean, H[3:33].mean(axis=0), rtol=1e-14) and np.allclose(m2, H[3:33].var(axis=0) * 30, rtol=1e-13)
    H[5, 2] = np.nan
    mean, m2 = mr.chain_stats(H, 0, 40)
    assert np.isnan(mean[2]) and np.isnan(m2[2]) and np.all(np.isfinite(np.delete(mean, 2)))
    U = rng.normal(size=(100, 8, 2))                             # stationary, independent: R-hat close to 1
    assert np.all(np.abs(mr.rhat(U) - 1.0) < 0.05)
    U[:, :4, 0] += 3.0                                           # half the chains elsewhere in the first column
    r = mr.rhat(U)
    assert r[0] > 1.5 and abs(r[1] - 1.0) < 0.05
    with pytest.raises(ValueError):
        mr.rhat(U[:3])


def test_the_fixed_seeds_of_the_device_tests_excuse_no_decision():
    """The accept inputs and the end-to-end run that tests/test_gpu_mcmc.py uses: no decision of the restatement lies inside the
    margin within which the device's log may decide otherwise, and every branch of the rule occurs."""
    for count in mr.ACCEPT_COUNTS:
        for tf in mr.ACCEPT_TFS:
            U, X, LL, Up, Xp, LLp, inside = mr.accept_case(count, tf)
            for step in (0, 1):
                take, margin = mr.accept_decision(LL, LLp, inside, tf, 0, mr.ACCEPT_SEED, step)
                assert margin.min() > mr.MARGIN, (count, tf, step, margin.min())
            if count > 1:
                assert 0.2 < take.mean() < 0.8
                compared = np.isfinite(margin)
                assert (take & compared).any() and (~take & compared).any()        # log(xi) < d decided both ways
                same = (LLp == LL) & np.isfinite(LL)             # d of exactly 0 (not the rows where both are -inf)
                assert same.any() and np.all(take[same & (inside != 0)])
    U0, X0, LL0, ref = mr.e2e_reference()
    print("end to end: smallest margin %.3g, acceptance %.3f, outside %.4f" % (ref["margin"], ref["accepted"].mean(), ref["outside"]))
    assert ref["margin"] > mr.E2E_MARGIN
    assert 0.1 < ref["accepted"].mean() < 0.7 and ref["outside"] > 0        # some proposals leave the cube and are never solved
