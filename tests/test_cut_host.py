"""The host side of the early stop (TRPL_FLAG_CUT): driver.next_cut, posterior.exact_cut_margin and the option checks of
driver.loglik / driver.simulate.  No GPU needed.

exact_cut_margin is checked against the expression it is derived for -- the weights of Visualization/utils.py:157-166, which
csrc/posterior.hip restates operation by operation: w = exp(((LL / tf - max) + 1000 ln 2) - ln S), then w / nansum(w) --
(the kernel then scales w by 1 + corr, |corr| < 2^-30, a function of the sample alone that leaves a zero a zero) --
evaluated here in NumPy: samples `margin` below the best one have a weight of exactly 0.0, so the weights of the others do
not depend on how far below they are.  The bound is the derivation's (exp underflows below ln 2^-1075 = -745.14), not a
measured figure."""
import inspect
import math

import numpy as np
import pytest


def _normalize(LL, tf):
    """utils.normalize in its order of operations (csrc/posterior.hip, weights_partial)."""
    q = LL / tf
    with np.errstate(under="ignore"):
        w = np.exp(((q - np.nanmax(q)) + 1000.0 * math.log(2.0)) - math.log(float(len(LL))))
    return w / np.nansum(w)


def test_next_cut_is_a_pure_function_of_margin_and_best_total(trpl):
    nc = trpl.driver.next_cut
    assert nc(5.0, None) == float("inf") and nc(0.0, None) == float("inf")
    assert nc(5.0, 2.5) == 7.5 and nc(1439.25, 0.0) == 1439.25
    assert nc(np.float64(1.5), np.float64(2.0)) == 3.5 and isinstance(nc(1.5, 2), float)
    assert nc(3.0, 10.0) > nc(3.0, 4.0)                       # a falling minimum tightens the level
    assert list(inspect.signature(nc).parameters) == ["margin", "best_total"]


@pytest.mark.parametrize("tf", [1.0, 4.0, 903.0 * 0.25])
@pytest.mark.parametrize("S", [8, 2 ** 10, 2 ** 17])
def test_exact_cut_margin_makes_the_weight_exactly_zero(trpl, tf, S):
    margin = trpl.posterior.exact_cut_margin(tf)
    assert margin == tf * (1000.0 * math.log(2.0) + 746.0)
    assert trpl.posterior.exact_cut_margin() == trpl.posterior.exact_cut_margin(1.0)
    rng = np.random.default_rng(S)
    for best in (-3.0, -2.5e4, -7.7e5):
        LL = best - rng.uniform(0.0, 0.999, S) * margin        # the head: within the margin of the best sample
        LL[0] = best
        tail = np.arange(S) >= S // 2
        cases = [LL.copy() for _ in range(4)]
        cases[0][tail] = best - margin                         # exactly at the margin
        cases[1][tail] = best - margin * (1.0 + rng.uniform(0.0, 3.0, tail.sum()))
        cases[2][tail] = -np.inf
        cases[3][tail] = best - margin - 1e9
        W = [_normalize(c, tf) for c in cases]
        for w in W:
            assert (w[tail] == 0.0).all()
            assert w[0] > 0.0 and np.isfinite(w).all() and abs(w.sum() - 1.0) < 1e-9
        for w in W[1:]:
            assert np.array_equal(w[~tail], W[0][~tail])       # the rest: unchanged whatever the tail holds
    # the docstring keeps the derivation
    doc = trpl.posterior.exact_cut_margin.__doc__
    assert "-745.14" in doc and "1000 ln 2" in doc and "ln S" in doc


def test_loglik_refuses_the_options_the_cut_does_not_combine_with(trpl):
    loglik = trpl.driver.loglik
    assert inspect.signature(loglik).parameters["sse_cut"].default is None
    args = (np.zeros((1, 13)), np.zeros((1, 16)), 100.0, 1.0, 16, 10, [np.zeros(3)])
    for kw, word in ((dict(mag_grid=[0.0]), "mag_grid"), (dict(mag_profile=True), "mag_profile"),
                     (dict(weights=[np.ones(3)]), "weights"), (dict(devices=[0]), "devices"), (dict(bundle=2), "bundle")):
        with pytest.raises(ValueError, match=word):
            loglik(*args, sse_cut=1.0, **kw)
    for bad in (float("nan"), -1.0):
        with pytest.raises(ValueError, match="sse_cut"):
            loglik(*args, sse_cut=bad)


def test_simulate_refuses_the_options_the_cut_margin_does_not_combine_with(trpl):
    T, Time = 40, 1.0
    tg = np.linspace(0, Time, T + 1)
    one = ([tg] * 3, [np.zeros(T + 1)] * 3, [np.full(T + 1, 0.1)] * 3)
    ini = np.zeros((3, 128))
    flags = {"load_PL_from_file": False, "log_pl": True, "self_normalize": False}
    base = {"sims_per_gpu": 4, "num_gpus": 1, "fused": True, "cut_margin": 10.0}

    def run(e_data, **kw):
        P = np.zeros((len(e_data), 8)); z = np.zeros(2)
        trpl.simulate(trpl.pvSim, e_data, P, np.ones((8, 13)), [None] * 2, [None] * 2, 3, [2000.0, Time, 128, T, 1, (0,), 7, 100], ini,
                      dict(flags), dict(base, **kw), 0, z.copy(), z.copy(), z.copy())
    for e_data, kw, word in (([one, one], {}, "len(e_data) > 1"), ([one], dict(devices=[0]), "devices"),
                             ([one], dict(num_gpus=2), "num_gpus"), ([one], dict(max_sims_per_block=2), "max_sims_per_block"),
                             ([one], dict(mag_grid=[0.0]), "mag_grid"), ([one], dict(weighted=True), "weighted"),
                             ([one], dict(fused=False), "fused"), ([one], dict(cut_margin=-1.0), "cut_margin")):
        with pytest.raises(ValueError) as ei:
            run(e_data, **kw)
        assert word in str(ei.value) and "cut_margin" in str(ei.value), (word, str(ei.value))
