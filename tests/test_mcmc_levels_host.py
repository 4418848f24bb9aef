"""The rule of early rejection (trpl_mcmc_levels, include/trpl.h) as tests/mcmc_levels_ref.py restates it, checked on the CPU
against the restated accept predicate: whatever a cut proposal reports, the accept step rejects it; the level is tight; and the
rule does not pass by never cutting.  No GPU, no library: tests/test_gpu_cut_levels.py holds the device to this restatement."""
import numpy as np

import mcmc_levels_ref as lr
import mcmc_ref as mr


def _inputs():
    LL, tf, chains, steps = lr.random_inputs()
    xi = lr.accept_uniform_at(chains, steps, lr.SEED)
    eLL, etf, exi = lr.edge_inputs()
    return np.concatenate([LL, eLL]), np.concatenate([tf, etf]), np.concatenate([xi, exi]), LL.size


def test_the_uniform_of_any_chain_and_step_is_the_accept_steps():
    chains = np.array([0, 7, (1 << 32) + 5, (1 << 40) - 1], dtype=np.uint64)
    for step in (0, 3, 0xFFFFFFFF):
        xi = lr.accept_uniform_at(chains, step, lr.SEED)
        for k, n in enumerate(chains):
            assert xi[k] == mr.accept_uniform(1, int(n), lr.SEED, step)[0]
    LL = -np.linspace(0.5, 40.0, 300)
    assert np.array_equal(lr.levels(LL, 2.5, 11, 9, 4), lr.levels_from_xi(LL, 2.5, mr.accept_uniform(300, 11, 9, 4)))


def test_whatever_a_cut_proposal_reports_is_rejected():
    LL, tf, xi, _ = _inputs()
    lv = lr.levels_from_xi(LL, tf, xi)
    fin = np.isfinite(lv)
    assert fin.sum() > 0.99 * lv.size and (lv[fin] >= 0.0).all()
    # a system cut at `level` reports sse > level, and P = -(sum of non-negative terms) <= -sse: the largest LLp a cut proposal can
    # have is -nextafter(level, inf)
    for LLp in (-np.nextafter(lv[fin], np.inf), -2.0 * lv[fin] - 1.0, np.full(fin.sum(), -np.inf)):
        take = lr.accept_take(LL[fin], LLp, tf[fin], xi[fin])
        assert not take.any(), (LL[fin][take][:5], tf[fin][take][:5], xi[fin][take][:5])


def test_the_level_is_tight_and_infinite_only_where_the_rule_says():
    LL, tf, xi, n_random = _inputs()
    lv = lr.levels_from_xi(LL, tf, xi)
    l0 = lr.first_candidate(LL, tf, xi)
    fin = np.isfinite(lv)
    assert (lv[fin] >= l0[fin]).all()
    assert (lv[fin] <= l0[fin] + (np.abs(LL[fin]) + l0[fin]) * 2.0 ** -39).all()
    # the cap: at most 1 % of the random inputs are never cut (the rule must not pass by giving up)
    share = float(np.mean(~fin[:n_random]))
    print("random inputs without a level: %.4f %%; first candidate taken: %.2f %%" % (100 * share, 100 * np.mean(lv[fin] == l0[fin])))
    assert share <= 0.01
    # the edge inputs
    eLL, etf, exi = lr.edge_inputs()
    e = lr.levels_from_xi(eLL, etf, exi)
    for k in range(eLL.size):
        if np.isnan(eLL[k]) or not eLL[k] > -np.inf or exi[k] == 0.0 or eLL[k] == np.inf:
            assert e[k] == np.inf, (k, eLL[k], exi[k], e[k])
    zero = (eLL == 0.0) & (exi == 0.5)
    assert zero.sum() == 2 and (e[zero] == etf[zero] * -np.log(0.5)).all()           # LL = -0.0 and +0.0: the level is -tf log(xi)
    # |LL| = 1e6 at tf = 1e-3 with tf log(xi) far below an ulp of LL: the first candidate is LL itself and cannot verify (dq = 0);
    # the second one does
    lost = (eLL == -1e6) & (etf == 1e-3) & (exi > 1.0 - 2.0 ** -35)
    assert lost.sum() >= 2 and (l0[n_random:][lost] == 1e6).all() and np.isfinite(e[lost]).all() and (e[lost] > 1e6).all()
