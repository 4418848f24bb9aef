"""Host forms of trpl_mag_grid_w / trpl_mag_profile_w (plain host code, include/trpl.h) and the Python side of the
uncertainty-weighted likelihood (likelihood.weights_from_uncertainty, prob(weighted=)).

With wsum = n_obs the weighted calls ARE the unweighted ones, bit for bit (one expression, the quadratic coefficient a
double).  With real weights -- 1 / (2 u^2) from the uncertainty column of tests/golden/obs_balanced_6ns.csv as
dataio.get_data rescales it (bayes_io.py:75-76), errors formed from the reference PL of tests/golden/lnp_maggrid.npz's
fixtures as test_mag_grid_host.py forms them -- the grid agrees with a direct evaluation of sum_i w_i (e_i + d)^2 (numpy, in
extended precision, so the reference adds no error of its own) within the header's bound, derived, not measured:
    |P_grid - P_direct| <= k eps (A_w(d) + |d| sum w_i |e_i|),   A_w(d) = sse + 2 |d esum| + wsum d^2,
    k = 6 + ceil(n / 64) + 6 with the moments summed in the FAST association (n + 6 for serial sums):
the moments bound with two more roundings, one per multiplication by the weight.  Nothing is added to it."""
import inspect
import math
import os

import numpy as np
import pytest

from test_mag_grid_host import EPS, OFFSETS, _batched_sum, _call_grid, _call_profile, _errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(trpl, n):
    """(3, n): the chi-square weights of the first n points of the three curves of obs_balanced_6ns.csv."""
    e = trpl.get_data([os.path.join(ROOT, "tests", "golden", "obs_balanced_6ns.csv")],
                      {"time_cutoff": None, "select_obs_sets": None, "noise_level": None},
                      {"log_pl": True, "self_normalize": False}, scale_f=1e-23)
    u = np.array([np.asarray(e[0][2][c], dtype=np.float64)[:n] for c in range(3)])
    assert u.shape == (3, n)
    w = trpl.likelihood.weights_from_uncertainty(u)
    assert w.max() / w.min() > 10.0                      # a real error column: the relative sigma grows along the decay
    return w


def _call_grid_w(trpl, sse, esum, wsum, offsets, P=None):
    A = trpl._abi
    C, S = sse.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.float64)
    wsum = np.ascontiguousarray(wsum, dtype=np.float64)
    P = np.zeros((len(offsets), S)) if P is None else P
    A.check(A.lib().trpl_mag_grid_w(A.ptr(sse), A.ptr(esum), A.ptr(wsum), S, C, A.ptr(offsets), len(offsets), A.ptr(P)))
    return P


def _call_profile_w(trpl, sse, esum, wsum, per_curve=False):
    A = trpl._abi
    C, S = sse.shape
    wsum = np.ascontiguousarray(wsum, dtype=np.float64)
    best = np.zeros((C, S) if per_curve else S)
    P = np.zeros(S)
    A.check(A.lib().trpl_mag_profile_w(A.ptr(sse), A.ptr(esum), A.ptr(wsum), S, C, A.MAG_PER_CURVE if per_curve else 0,
                                       A.ptr(best), A.ptr(P)))
    return best, P


def _serial_sum(v):
    total = np.zeros(v.shape[:-1])
    for i in range(v.shape[-1]):
        total = total + v[..., i]
    return total


@pytest.mark.parametrize("name,key", [("pvsim_power.npz", "power"), ("pvsim_twothick.npz", "twothick")])
def test_wsum_equal_to_n_obs_is_the_unweighted_call_bit_for_bit(trpl, name, key):
    e = _errors(name, key)
    C, S, n = e.shape
    sse = np.ascontiguousarray(_batched_sum(e * e))
    esum = np.ascontiguousarray(_batched_sum(e))
    n_obs = np.array([n, n - 7, n - 1][:C], dtype=np.int64)
    wsum = n_obs.astype(np.float64)
    assert np.array_equal(_call_grid_w(trpl, sse, esum, wsum, OFFSETS), _call_grid(trpl, sse, esum, n_obs, OFFSETS))
    P0 = np.full((3, S), 5.0)
    assert np.array_equal(_call_grid_w(trpl, sse, esum, wsum, OFFSETS[:3], P=P0.copy()),
                          _call_grid(trpl, sse, esum, n_obs, OFFSETS[:3], P=P0.copy()))
    for per_curve in (False, True):
        bw, Pw = _call_profile_w(trpl, sse, esum, wsum, per_curve)
        b, P = _call_profile(trpl, sse, esum, n_obs, per_curve)
        assert np.array_equal(bw, b) and np.array_equal(Pw, P)


@pytest.mark.parametrize("name,key", [("pvsim_power.npz", "power"), ("pvsim_twothick.npz", "twothick")])
@pytest.mark.parametrize("serial", [False, True])
def test_weighted_grid_equals_the_direct_sum_within_the_derived_bound(trpl, name, key, serial):
    e = _errors(name, key)
    C, S, n = e.shape
    w = _weights(trpl, n)[:C, None, :]                                                   # (C, 1, n)
    summed = _serial_sum if serial else _batched_sum
    sse = np.ascontiguousarray(summed((e * e) * w))                                      # the sink's products, as written
    esum = np.ascontiguousarray(summed(e * w))
    wsum = np.array([math.fsum(w[c, 0]) for c in range(C)])
    P = _call_grid_w(trpl, sse, esum, wsum, OFFSETS)
    k = (n + 6) if serial else (6 + -(-n // 64) + 6)
    el, wl = e.astype(np.longdouble), w.astype(np.longdouble)
    worst = 0.0
    for m, d in enumerate(OFFSETS):
        direct = (wl * (el + np.longdouble(d)) ** 2).sum(axis=2)                         # (C, S), extended precision
        A_d = sse + 2 * np.abs(d * esum) + wsum[:, None] * d * d
        bound = k * EPS * (A_d + abs(d) * (w * np.abs(e)).sum(axis=2))                   # the header's bound, as stated
        err = np.abs(P[m] + direct.sum(axis=0).astype(np.float64))
        tot = bound.sum(axis=0)
        worst = max(worst, float((err / tot).max()))
        assert (err <= tot).all(), (name, d, float((err / tot).max()))
        for c in range(C):                                                               # and curve by curve
            Pc = _call_grid_w(trpl, sse[c:c + 1], esum[c:c + 1], wsum[c:c + 1], [d])[0]
            assert (np.abs(Pc + direct[c].astype(np.float64)) <= bound[c]).all(), (name, c, d)
    print("%s (%s sums): n = %d, k = %d, worst error / bound = %.3f" % (name, "serial" if serial else "FAST", n, k, worst))
    # evaluated as written, the quadratic coefficient wsum_c
    P2 = _call_grid_w(trpl, sse, esum, wsum, OFFSETS[:3], P=np.full((3, S), 5.0))
    want = np.full((3, S), 5.0)
    for m, d in enumerate(OFFSETS[:3]):
        acc = np.zeros(S)
        for c in range(C):
            acc = acc + np.maximum((sse[c] + (2.0 * d) * esum[c]) + wsum[c] * (d * d), 0.0)
        want[m] = want[m] - acc
    assert np.array_equal(P2, want)


def test_weighted_profile_equals_the_grid_at_best_and_best_minimises(trpl):
    e = _errors("pvsim_power.npz", "power")
    C, S, n = e.shape
    w = _weights(trpl, n)[:C, None, :]
    sse = np.ascontiguousarray(_batched_sum((e * e) * w))
    esum = np.ascontiguousarray(_batched_sum(e * w))
    wsum = np.array([math.fsum(w[c, 0]) for c in range(C)])
    best, P = _call_profile_w(trpl, sse, esum, wsum)
    acc, W = np.zeros(S), 0.0
    for c in range(C):
        acc, W = acc + esum[c], W + wsum[c]
    assert np.array_equal(best, (0.0 - acc) / W)
    for s in range(S):                                                                   # bit for bit the grid at best[s]
        assert _call_grid_w(trpl, sse, esum, wsum, [best[s]])[0, s] == P[s]
    fine = best[None, :] + np.linspace(-0.01, 0.01, 41)[:, None]                         # best minimises over a fine grid
    for s in range(S):
        Pf = _call_grid_w(trpl, sse, esum, wsum, fine[:, s])[:, s]
        assert P[s] >= Pf.max() - 8 * EPS * abs(P[s]) and np.argmax(Pf) in (19, 20, 21)
    bc, Pc = _call_profile_w(trpl, sse, esum, wsum, per_curve=True)
    assert np.array_equal(bc, (0.0 - esum) / wsum[:, None])
    assert (Pc >= P).all()
    # a curve whose weights are all zero: no best offset of its own, and it contributes nothing
    sse0, esum0, wsum0 = sse.copy(), esum.copy(), wsum.copy()
    sse0[1], esum0[1], wsum0[1] = 0.0, 0.0, 0.0
    b0, P0 = _call_profile_w(trpl, sse0, esum0, wsum0, per_curve=True)
    keep = [0, 2]
    b2, P2 = _call_profile_w(trpl, np.ascontiguousarray(sse[keep]), np.ascontiguousarray(esum[keep]), wsum[keep], per_curve=True)
    assert np.isnan(b0[1]).all() and np.array_equal(b0[keep], b2) and np.array_equal(P0, P2)
    bs0, Ps0 = _call_profile_w(trpl, sse0, esum0, wsum0)
    bs2, Ps2 = _call_profile_w(trpl, np.ascontiguousarray(sse[keep]), np.ascontiguousarray(esum[keep]), wsum[keep])
    assert np.array_equal(bs0, bs2) and np.array_equal(Ps0, Ps2)
    assert np.array_equal(_call_grid_w(trpl, sse0, esum0, wsum0, OFFSETS),
                          _call_grid_w(trpl, np.ascontiguousarray(sse[keep]), np.ascontiguousarray(esum[keep]), wsum[keep], OFFSETS))
    z = np.zeros((1, S))                                                                 # every weight zero: nothing to fit
    bz, Pz = _call_profile_w(trpl, z, z, [0.0])
    assert np.isnan(bz).all() and (Pz == 0.0).all()
    # a flagged system stays flagged whatever the weights
    sse_f, esum_f = sse.copy(), esum.copy()
    sse_f[0, 1], esum_f[0, 1] = np.inf, np.nan
    bf, Pf = _call_profile_w(trpl, sse_f, esum_f, wsum)
    assert np.isnan(bf[1]) and Pf[1] == -np.inf and np.isfinite(np.delete(Pf, 1)).all()
    assert (_call_grid_w(trpl, sse_f, esum_f, wsum, OFFSETS)[:, 1] == -np.inf).all()


def test_weights_from_uncertainty(trpl):
    wf = trpl.likelihood.weights_from_uncertainty
    u = np.array([0.5, 1.0, 2.0, 0.1, 3e-3])
    assert np.array_equal(wf(u), 1.0 / (2.0 * u * u))
    assert np.array_equal(wf([0.5, 2.0]), [2.0, 0.125]) and wf(u.reshape(1, 5)).shape == (1, 5)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        v = u.copy()
        v[3] = bad
        with pytest.raises(ValueError, match=r"uncertainty\[3\]"):
            wf(v)


def test_prob_is_untouched_by_default_and_uses_the_uncertainty_only_when_asked(trpl):
    prob = trpl.likelihood.prob
    sig = inspect.signature(prob)
    assert list(sig.parameters)[:8] == ["P", "plI", "values", "uncertainty", "mag_grid", "TPB", "BPG", "device"]
    assert sig.parameters["weighted"].default is False
    assert inspect.signature(trpl.driver.loglik).parameters["weights"].default is None
    values = np.zeros(5)
    empty = np.zeros((0, 5), dtype=np.float32)
    # an empty batch needs no device; by default the uncertainty is not even looked at (the reference never reads it)
    assert prob(np.zeros(0), empty, values, np.full(5, np.nan), np.zeros(0)) == 0.0
    assert prob(np.zeros(0), empty, values, np.full(5, 0.1), np.zeros(0), weighted=True) == 0.0
    with pytest.raises(ValueError, match="uncertainty"):
        prob(np.zeros(0), empty, values, None, np.zeros(0), weighted=True)
    with pytest.raises(ValueError, match=r"uncertainty\[2\]"):
        prob(np.zeros(0), empty, values, [0.1, 0.1, 0.0, 0.1, 0.1], np.zeros(0), weighted=True)
    with pytest.raises(ValueError, match="shape"):
        prob(np.zeros(0), empty, values, np.full(4, 0.1), np.zeros(0), weighted=True)
    # loglik refuses the sharded form by name before anything else
    with pytest.raises(ValueError, match="weights"):
        trpl.driver.loglik(np.zeros((1, 13)), np.zeros((1, 16)), 100.0, 1.0, 16, 10, [np.zeros(3)], weights=[np.ones(3)],
                           devices=[0])
