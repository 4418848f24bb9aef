"""tests/mcmc_tempered_ref.py, the numpy restatement of parallel tempering, checked on its own: the exchange is a permutation of
rows with a symmetric flag; a pair and its reverse are exchanged with probabilities in the ratio exp(d) (detailed balance of the
joint state); one rung is mcmc_ref.run; the inputs of the device tests excuse no decision; and the bimodal toy, where the gate of
tests/test_gpu_mcmc_tempered.py is fixed.  No GPU, no library."""
import numpy as np
import pytest

import mcmc_ref as mr
import mcmc_tempered_ref as tr


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("K", (1, 2, 3, 4, 5))
def test_the_swap_is_a_permutation_of_rows_with_a_symmetric_flag(K):
    for group in (1, 2, 7):
        n = K * group
        rng = np.random.default_rng([K, group])
        U, X, LL = rng.random((n, 3)), rng.normal(size=(n, 4)), -5.0 * rng.random(n)
        U[:, 0] = np.arange(n)                                   # a row's name
        tf = tr.geometric_ladder(1.0, 20.0, K)
        for parity in (0, 1):
            U2, X2, LL2, swapped, _ = tr.swap(U, X, LL, K, group, tf, parity, 9, 21, 4)
            src = U2[:, 0].astype(np.int64)                      # where every row came from
            assert np.array_equal(np.sort(src), np.arange(n))
            assert _same_bits(U2, U[src]) and _same_bits(X2, X[src]) and _same_bits(LL2, LL[src])
            a, b, _ = tr.swap_pairs(K, group, parity)
            assert a.size == (max(K - parity, 0) // 2) * group
            unpaired = np.setdiff1d(np.arange(n), np.concatenate([a, b]))
            assert np.all(swapped[unpaired] == 0) and np.array_equal(src[unpaired], unpaired)
            assert np.array_equal(swapped[a], swapped[b]) and np.all(np.isin(swapped, (0, 1)))
            assert np.array_equal(src[a], np.where(swapped[a] != 0, b, a)) and np.array_equal(src[b], np.where(swapped[a] != 0, a, b))
            if K == 1:
                assert not swapped.any() and _same_bits(U2, U)
    if K >= 2:                                                   # both outcomes occur
        taken = [tr.swap_decision(-5.0 * np.random.default_rng(s).random(K * 64), K, 64, tr.geometric_ladder(1.0, 20.0, K), 0, 0, s, 0)[2]
                 for s in range(4)]
        assert 0 < np.concatenate(taken).mean() < 1


def test_a_pair_and_its_reverse_stand_in_the_ratio_exp_d():
    """min(1, e^d) / min(1, e^-d) = e^d: with the symmetric proposal 'exchange', the exact Metropolis ratio of the joint state
    L(x_a)^(1/tf_k) L(x_b)^(1/tf_k+1)."""
    rng = np.random.default_rng(2)
    la, lb = -20.0 * rng.random(1000), -20.0 * rng.random(1000)
    tfa, tfb = 10.0 ** rng.uniform(-1, 2, 1000), 10.0 ** rng.uniform(-1, 2, 1000)
    d = tr.swap_d(la, lb, tfa, tfb)
    fwd, back = tr.swap_probability(la, lb, tfa, tfb), tr.swap_probability(lb, la, tfa, tfb)
    assert np.all((fwd == 1.0) | (back == 1.0))
    assert np.allclose(fwd / back, np.exp(d), rtol=1e-13, atol=0)
    # ... and d is the log of that ratio of tempered likelihoods
    want = (lb / tfa + la / tfb) - (la / tfa + lb / tfb)
    assert np.allclose(d, want, rtol=0, atol=1e-12 * np.maximum(1.0, np.abs(want)).max())
    # the rule's special values: equal temperatures exchange every finite pair, NaN d exchanges nothing
    LL = np.array([-1.0, -np.inf, -np.inf, np.nan, -3.0, -0.5, -np.inf, -5.0, -4.0, np.inf])
    a, b, take, margin = tr.swap_decision(LL, 2, 5, np.array([2.0, 2.0]), 0, 0, 1, 0)
    assert np.array_equal(take, [True, False, False, False, False]) and np.all(np.isinf(margin))       # d = 0, then NaN: 0 * inf
    a, b, take, margin = tr.swap_decision(LL, 2, 5, np.array([1.0, 2.0]), 0, 0, 1, 0)
    assert np.array_equal(take, [True, False, True, False, True]) and np.all(np.isinf(margin))         # the better state goes down
    a, b, take, margin = tr.swap_decision(LL, 2, 5, np.array([2.0, 1.0]), 0, 0, 1, 0)
    assert not take[1:].any() and np.all(np.isinf(margin[1:])) and np.isfinite(margin[0])              # d = -inf never, d = -1/4 by xi


@pytest.mark.parametrize("kind", ("de", "rw"))
def test_one_rung_is_the_plain_run(kind):
    loglik, _ = mr.toy(0.0)
    U0 = mr.toy_start(12, 5)
    LL0 = loglik(U0)
    kw = dict(sweeps=8, kind=kind, scale=0.05, jump_every=3, seed=9)
    want = mr.run(loglik, U0, LL0, *mr.CUBE, tf=2.5, **kw)
    for swap_every in (1, 3):
        got = tr.run_tempered(loglik, U0, LL0, *mr.CUBE, [2.5], swap_every=swap_every, **kw)
        assert got["swaps"] == 0 and got["swap_rate"].shape == (0,)
        assert _same_bits(got["U"][0], want["U"]) and _same_bits(got["X"][0], want["X"]) and _same_bits(got["LL"][0], want["LL"])
        assert np.array_equal(got["accepted"][0], want["accepted"]) and got["outside"][0] == want["outside"]
        assert got["margin"] == want["margin"]


@pytest.mark.parametrize("K", tr.SWAP_KS)
def test_the_swap_cases_of_the_device_test_excuse_nothing(K):
    """The cap of tests/test_gpu_mcmc.py's accept test -- at most 1 % of the decisions within MARGIN of a tie -- is kept by the
    restatement alone with room to spare: no decision of any case is excused, so the device must equal it bit for bit."""
    tf = tr.swap_ladder(K)
    assert K < 3 or tf[0] == tf[1]
    kinds = set()
    for group, parity, A, ncol, chain0, step in tr.swap_cases(K):
        U, X, LL = tr.swap_case(K, group, A, ncol)
        a, b, take, margin = tr.swap_decision(LL, K, group, tf, parity, chain0, tr.SWAP_SEED, step)
        assert not (margin <= mr.MARGIN).any(), (K, group, parity, margin.min())
        if group >= 5:
            la, lb = LL[a], LL[b]
            for name, m in (("lower -inf", np.isneginf(la) & np.isfinite(lb)), ("upper -inf", np.isfinite(la) & np.isneginf(lb)),
                            ("both -inf", np.isneginf(la) & np.isneginf(lb)), ("nan", np.isnan(la) | np.isnan(lb)),
                            ("equal", (la == lb) & np.isfinite(la)), ("taken", take), ("refused", ~take & np.isfinite(la) & np.isfinite(lb))):
                if m.any():
                    kinds.add(name)
            assert not take[np.isnan(la) | np.isnan(lb)].any() and not take[np.isneginf(la) & np.isneginf(lb)].any()
            assert np.all(take[(la == lb) & np.isfinite(la)])
    want = {"lower -inf", "upper -inf", "both -inf", "nan", "equal", "taken", "refused"}
    if K == 2:                                                   # one pair of rungs: at parity 0 the special rows alternate with it only
        want -= {"upper -inf"}
    assert kinds >= want, want - kinds


@pytest.mark.parametrize("swap_every", (1, 3))
def test_the_end_to_end_case_of_the_device_test_decides_nothing_near_a_tie(swap_every):
    ref = tr.e2e_reference(swap_every)[3]
    assert ref["margin"] > mr.E2E_MARGIN
    assert ref["swaps"] == tr.E2E["sweeps"] // swap_every and np.all(ref["swap_rate"] > 0) and np.all(ref["swap_rate"] <= 1)
    assert 0 < ref["accepted"].mean() < 1


def test_the_gate_of_the_bimodal_toy():
    assert len(tr.BI_SHARES) == len(tr.BI_SEEDS) == 8
    assert tr.BI_MARGIN == 5.0 * np.std(tr.BI_SHARES) and 0.01 < tr.BI_MARGIN < 0.1      # a gate that can fail: far inside 0.5
    assert abs(tr.BI_SHARES[tr.BI_SEEDS.index(tr.BI_DEVICE_SEED)] - 0.5) < tr.BI_MARGIN


@pytest.mark.parametrize("i", range(len(tr.BI_SEEDS)))
def test_the_bimodal_toy_on_the_restatement(i):
    """Every chain starts in the first mode.  The tempered cold rung spends half of its time in the second one; the recorded share
    of each seed, from which the device test's margin is formed, is recomputed here."""
    seed = tr.BI_SEEDS[i]
    U0, LL0 = tr.bimodal_start(seed)
    assert tr.second_mode_share(U0) == 0.0
    lad = tr.geometric_ladder(1.0, tr.BI_HOT, tr.BI_K)
    ref = tr.run_tempered(tr.bimodal_loglik, U0, LL0, *tr.BI_BOX, lad, sweeps=tr.BI_SWEEPS, seed=seed)
    share = tr.second_mode_share(ref["U"][0, tr.BI_BURN:])
    print("seed %d: share %.9f, swap rates %s" % (seed, share, np.round(ref["swap_rate"], 3)))
    assert share == tr.BI_SHARES[i]
    assert np.all(ref["swap_rate"] > 0)
    if seed == tr.BI_DEVICE_SEED:
        assert abs(share - 0.5) < tr.BI_MARGIN
        # the single-temperature ensemble never leaves the first mode: its differences cannot span 16 deviations
        plain = mr.run(tr.bimodal_loglik, U0, LL0, *tr.BI_BOX, sweeps=tr.BI_SWEEPS, seed=seed)
        assert tr.second_mode_share(plain["U"]) == 0.0
