"""The restatement of the subspace differential-evolution proposal alone (tests/mcmc_subspace_ref.py), and trpl_amd.mcmc.run's Python
layer driven by it: the anchor (ncr = 1, one pair, e_width = 0 is mcmc_ref's rung proposal bit for bit, folded or not), the structure
of a proposal, its reversibility, the Python refusals, and the adaptation of the crossover shares.  No GPU, no library."""
import numpy as np
import pytest

import mcmc_fold_ref as fr
import mcmc_ref as mr
import mcmc_subspace_ref as sr

HI = (1 << 32) + 7                                                # a chain0 whose counter uses its high word


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _case(count, A, P, seed=0, spread=1.0):
    rng = np.random.default_rng([seed, count, A, P])
    return rng.random((count, A)), 0.5 + spread * (rng.random((P, A)) - 0.5)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("A", [1, 2, 10, 16])
def test_the_anchor_is_the_rung_proposal_bit_for_bit(A, fold):
    group, K = 5, 3
    U, partners = _case(K * group, A, K * group, spread=3.0)     # wide partners: a proposal leaves the cube, or is folded
    U, partners[:group] = 0.3 + 0.4 * U, 0.5 + 0.05 * (partners[:group] - 0.5) / 3.0      # but for rung 0, whose proposals stay inside
    scale, gamma = np.linspace(0.0, 0.05, A), 0.7
    lo, hi, lg = np.full(A, 1e-2), np.full(A, 1e2), (np.arange(A) % 2).astype(np.int32)
    got = sr.propose(U, partners, group, np.full((1, A), gamma), scale, HI, 5, 3, lo, hi, lg, ncr=1, e_width=0.0, fold=fold)
    want = [fr.propose(U[k * group:(k + 1) * group], partners[k * group:(k + 1) * group], gamma, scale, HI + k * group, 5, 3, lo, hi, lg,
                       fold=fold) for k in range(K)]              # the rung call is the plain call on each slice (mcmc_tempered_ref)
    for j in range(3):
        w = np.concatenate([x[j] for x in want])
        assert np.array_equal(_bits(got[j]), _bits(w)) if j < 2 else np.array_equal(got[j], w)
    assert np.all(got[3] == (1 << A) - 1) and np.all(got[4] == 1)
    assert set(got[2].tolist()) == ({1, 2} if fold else {0, 1})       # both codes occur


def test_the_structure_of_a_proposal():
    count, A, group, pairs, ncr = 1 << 16, 10, 64, 4, 3
    pcr = np.array([0.6, 0.1, 0.3])
    U, partners = _case(count, A, count)
    tab = sr.gamma_table(pairs, A)
    Up, inside, mask, sel, raw = sr.propose_unit(U, partners, group, tab, 1e-3, HI, 9, 4, ncr, pcr, 0.05)
    d = sr.draws(count, A, group, HI, 9, 4, pairs, ncr, pcr)
    sel_bits = (mask[:, None] >> np.arange(A)) & 1 == 1
    assert np.all(mask != 0) and np.array_equal(sel_bits, d["mask"])
    assert np.array_equal(_bits(Up)[~sel_bits], _bits(U)[~sel_bits])             # an unselected coordinate has U's bits
    assert np.all(Up[sel_bits] != U[sel_bits])
    want = d["c"] < d["cr"][:, None]
    none = ~want.any(axis=1)
    assert none.any()                                             # the fallback is exercised: (2/3)^10 of the class CR = 1/3
    assert np.array_equal(sel_bits[~none], want[~none])
    assert np.all(sel_bits[none].sum(axis=1) == 1) and np.array_equal(sel_bits[none].argmax(axis=1), d["f"][none])
    assert np.bincount(d["f"][none], minlength=A).min() > 0       # and it falls on every coordinate
    delta, m = sel & 0xFF, sel >> 8
    assert delta.min() == 1 and delta.max() == pairs and np.array_equal(delta, d["delta"]) and np.array_equal(m, d["m"])
    for freq, p in ((np.bincount(m, minlength=ncr) / count, pcr), (np.bincount(delta - 1, minlength=pairs) / count, np.full(pairs, 1.0 / pairs))):
        assert np.all(np.abs(freq - p) < 5.0 * np.sqrt(p * (1.0 - p) / count)), (freq, p)
    assert np.all(d["a"] != d["b"]) and d["a"].min() == 0 and d["a"].max() == group - 1 and d["b"].max() == group - 1
    # the rows are the chain's rung's, and D is the sum of the first delta differences
    base = (np.arange(count) // group) * group
    D = np.zeros((count, A))
    for p in range(pairs):
        D += np.where((p < delta)[:, None], partners[base + d["a"][:, p]] - partners[base + d["b"][:, p]], 0.0)
    g = tab[delta - 1, d["dsel"] - 1]
    step = Up - U - (g[:, None] * (1.0 + 0.05 * (2.0 * d["v"] - 1.0))) * D
    assert np.all(np.abs(step[sel_bits]) <= 1e-3 + 1e-12) and np.abs(step[sel_bits]).max() > 0.9e-3
    assert np.array_equal(inside, np.all(~sel_bits | ((Up >= 0.0) & (Up <= 1.0)), axis=1).astype(np.int32))
    # equal shares without pcr, and one class selects everything
    assert np.array_equal(sr.class_cdf(4), np.array([0.25, 0.5, 0.75, 1.0])) and sr.class_cdf(3, pcr)[-1] == 1.0
    assert np.all(sr.draws(64, A, 8, 0, 1, 0, 2, 1)["mask"])


@pytest.mark.parametrize("A", [1, 3, 10, 16])
def test_the_move_is_reversible_through_the_exchanged_pairs(A):
    count, group, pairs = 4096, 16, 4
    U, partners = _case(count, A, count, seed=2)
    tab, scale, e_width = sr.gamma_table(pairs, A), np.full(A, 1e-2), 0.2
    d = sr.draws(count, A, group, 3, 11, 6, pairs, 3)
    g = tab[d["delta"] - 1, d["dsel"] - 1]
    D = sr.difference(partners, group, d["a"], d["b"], d["delta"])
    Up = sr.move(U, D, g, e_width, d["v"], scale, d["xi"], d["mask"])
    back = sr.move(Up, sr.difference(partners, group, d["b"], d["a"], d["delta"]), g, e_width, d["v"], scale, d["xi"], d["mask"], sign=-1.0)
    ulp = np.spacing(np.maximum(np.abs(U), np.abs(Up)))
    assert np.all(np.abs(back - U) <= 4.0 * ulp), float(np.max(np.abs(back - U) / ulp))
    assert np.array_equal(_bits(back)[~d["mask"]], _bits(U)[~d["mask"]])
    # the exchanged draw is as likely as the draw: the ordered pair is uniform over a != b
    a, b = d["a"][:, 0], d["b"][:, 0]
    n = np.bincount(a * group + b, minlength=group * group).reshape(group, group)
    assert np.all(np.diag(n) == 0) and np.all(np.abs(n - n.T)[~np.eye(group, dtype=bool)] < 5.0 * np.sqrt(2.0 * count / (group * (group - 1))))


def test_python_refusals(trpl):
    M = trpl.mcmc
    lo, hi, lg = np.zeros(3), np.ones(3), np.zeros(3, dtype=np.int32)
    X0, LL0 = np.full((4, 3), 0.5), np.zeros(4)

    def never(X):
        raise AssertionError("the likelihood was called")

    def both(**kw):
        yield lambda: M.run(never, X0, LL0, lo, hi, lg, sweeps=2, **kw)
        yield lambda: M.run_tempered(never, X0, LL0, lo, hi, lg, [1.0, 2.0], sweeps=2, **kw)

    for kind, extra in (("de", {}), ("rw", dict(scale=0.1)), ("stretch", {})):
        for kw in (dict(pairs=2), dict(ncr=2), dict(e_width=0.1), dict(pcr=[0.2, 0.3, 0.5]), dict(adapt_cr=True, burn=1)):
            for call in both(kind=kind, **extra, **kw):
                with pytest.raises(ValueError, match="belongs to kind='subspace'"):
                    call()
    for pairs in (0, -1, 5, 2.5, None, True):
        for call in both(kind="subspace", pairs=pairs):
            with pytest.raises(ValueError, match="pairs="):
                call()
    for ncr in (0, -1, 9, 1.5, None):
        for call in both(kind="subspace", ncr=ncr):
            with pytest.raises(ValueError, match="ncr="):
                call()
    for e in (-0.1, 1.0, 2.0, np.nan, np.inf, None):
        for call in both(kind="subspace", e_width=e):
            with pytest.raises(ValueError, match="e_width="):
                call()
    for pcr in ([0.5, 0.5], [0.2, 0.3, 0.4, 0.1], [[0.2, 0.3, 0.5]]):
        for call in both(kind="subspace", pcr=pcr):
            with pytest.raises(ValueError, match="pcr must be"):
                call()
    for pcr in ([0.5, -0.1, 0.6], [0.0, 0.0, 0.0], [np.nan, 0.5, 0.5], [np.inf, 0.5, 0.5]):
        for call in both(kind="subspace", pcr=pcr):
            with pytest.raises(ValueError, match="pcr:"):
                call()
    for call in both(kind="subspace", gamma=np.nan):
        with pytest.raises(ValueError, match="gamma="):
            call()
    for kw in (dict(adapt_cr=True), dict(adapt_cr=True, burn=0)):
        for call in both(kind="subspace", **kw):
            with pytest.raises(ValueError, match="burn must be >= 1"):
                call()
    for call in both(kind="subspace", adapt_cr=1):
        with pytest.raises(ValueError, match="adapt_cr must be"):
            call()
    for call in both(kind="subspace", bounds="bounce"):
        with pytest.raises(ValueError, match="bounds"):
            call()
    with pytest.raises(ValueError, match="gamma_tab must be"):
        M.propose_subspace(np.zeros((4, 3)), np.zeros((4, 3)), None, np.zeros((2, 2)), 1e-3, 0, 1, 0, lo, hi, lg)
    with pytest.raises(ValueError, match="pcr must be"):
        M.propose_subspace(np.zeros((4, 3)), np.zeros((4, 3)), None, np.zeros((2, 3)), 1e-3, 0, 1, 0, lo, hi, lg, ncr=3, pcr=[0.5, 0.5])
    with pytest.raises(ValueError, match="partners must be"):
        M.propose_subspace(np.zeros((4, 3)), np.zeros((4, 2)), None, np.zeros((2, 3)), 1e-3, 0, 1, 0, lo, hi, lg)
    assert np.array_equal(_bits(M.subspace_gamma_table(4, 10, 0.5)), _bits(sr.gamma_table(4, 10, 0.5)))


# ---- trpl_amd.mcmc.run driven by the restatement: the module's front ends replaced by numpy, so its own sweep loop, counters and
# adaptation run with no device
TOY = dict(A=4, C=32, sweeps=40, burn=25, seed=3, sd=0.1)


def _toy_loglik(X):
    return -0.5 * np.sum((np.asarray(X) - 0.5) ** 2, axis=1) / TOY["sd"] ** 2


def _inject(monkeypatch, M):
    def propose_subspace(U, partners, group, tab, scale, chain0, seed, step, lo, hi, lg, ncr=3, pcr=None, e_width=0.05, sim_flags=None,
                         device=0, info=None, fold=False):
        return sr.propose(U, partners, group, tab, scale, chain0, seed, step, lo, hi, lg, ncr, pcr, e_width, fold=fold)

    def propose(U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, sim_flags=None, device=0, info=None, fold=False):
        return fr.propose(U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, fold=fold)

    def accept(U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step, device=0, info=None):
        U2, X2, LL2, acc, _ = mr.accept(U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step)
        U[:], X[:], LL[:] = U2, X2, LL2
        return acc

    monkeypatch.setattr(M, "propose_subspace", propose_subspace)
    monkeypatch.setattr(M, "propose", propose)
    monkeypatch.setattr(M, "accept", accept)


@pytest.mark.parametrize("adapt", [False, True])
def test_run_with_the_restatement_s_proposal_is_the_restatement_s_run(trpl, monkeypatch, adapt):
    M = trpl.mcmc
    _inject(monkeypatch, M)
    A, C = TOY["A"], TOY["C"]
    box = (np.zeros(A), np.ones(A), np.zeros(A, dtype=np.int32))
    U0 = np.random.default_rng(TOY["seed"]).random((C, A))
    kw = dict(sweeps=TOY["sweeps"], seed=TOY["seed"], bounds="fold", pairs=2, ncr=4, e_width=0.1, jump_every=7, adapt_cr=adapt)
    info = {}
    ch = M.run(_toy_loglik, U0, _toy_loglik(U0), *box, kind="subspace", U0=U0, burn=TOY["burn"], info=info, **kw)
    ref = sr.run(_toy_loglik, U0, _toy_loglik(U0), *box, burn=TOY["burn"], **kw)
    assert np.array_equal(_bits(ch.U), _bits(ref["U"][TOY["burn"]:])) and np.array_equal(ch.accept, ref["accepted"][TOY["burn"]:])
    assert info["pairs"] == 2 and info["ncr"] == 4 and info["mean_dsel"] == ref["mean_dsel"] and 1.0 <= info["mean_dsel"] <= A
    assert np.array_equal(info["pcr"], ref["pcr"]) and info["folded"] == ref["folded"]
    if not adapt:
        assert info["pcr"] == [0.25] * 4 and "pcr_trace" not in info
        return
    trace = info["pcr_trace"]
    assert trace.shape == (TOY["sweeps"], 4) and np.array_equal(trace, ref["pcr_trace"])
    assert np.allclose(trace.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    floor = 1.0 / (10 * 4)
    assert np.all(trace >= floor / (1.0 + 4 * floor) - 1e-15)      # floored at 1 / (10 ncr), then divided by a sum of at most 1.1
    assert np.all(trace[TOY["burn"]:] == trace[TOY["burn"]])       # frozen: the kept sweeps have one kernel
    assert np.array_equal(trace[TOY["burn"]], info["pcr"]) and np.all(trace[0] == 0.25)
    assert len({tuple(r) for r in trace[:TOY["burn"]]}) > 5        # and it moved while it was allowed to
    assert not np.array_equal(trace[TOY["burn"]], trace[0])


def test_adapted_pcr_is_its_rule(trpl):
    f = trpl.mcmc.adapted_pcr
    for ncr in (1, 3, 8):
        floor = 1.0 / (10 * ncr)
        rng = np.random.default_rng(ncr)
        for jump, tried in ((rng.random(ncr), rng.integers(1, 50, ncr)), (np.zeros(ncr), np.ones(ncr, dtype=np.int64)),
                            (np.zeros(ncr), np.zeros(ncr, dtype=np.int64)), (np.eye(ncr)[0] * 1e6, np.full(ncr, 10))):
            p = f(jump, tried, ncr)
            assert np.array_equal(p, sr.adapted_pcr(np.asarray(jump, dtype=np.float64), np.asarray(tried), ncr))
            assert abs(p.sum() - 1.0) < 1e-15 and np.all(p >= floor / 1.1 - 1e-15)
    p = f(np.array([4.0, 1.0, 1.0]), np.array([2, 1, 1]), 3)      # means 2, 1, 1 -> shares 1/2, 1/4, 1/4: no floor applies
    assert np.allclose(p, [0.5, 0.25, 0.25], rtol=1e-15, atol=0)
    p = f(np.array([1.0, 0.0, 0.0]), np.array([1, 1, 1]), 3)      # 1, 0, 0 -> floored to 1, 1/30, 1/30 -> over their sum
    assert np.allclose(p, np.array([1.0, 1 / 30, 1 / 30]) / (1.0 + 2 / 30), rtol=1e-15, atol=0)


def test_the_correlated_toy_of_the_device_test_in_the_restatement():
    """The gates of the device test hold the truth: the restatement alone passes at the sweep count the test uses."""
    lo, hi = sr.ten_gates()
    print("10-D toy, restatement over %d seeds: mean %s" % (len(sr.TEN_SEEDS), np.array2string(sr._ten["rows"].mean(axis=0), precision=4)))
    print("gates lo %s\ngates hi %s" % (np.array2string(lo, precision=4), np.array2string(hi, precision=4)))
    assert np.all(lo < sr.TEN_TRUTH) and np.all(sr.TEN_TRUTH < hi)
    width = hi - lo                                               # and they can tell an ensemble that is off by one deviation, or 0.1 in rho
    assert np.all(width[:20] < sr.TEN_SD) and width[20] < 0.1
