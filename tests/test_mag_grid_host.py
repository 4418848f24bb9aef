"""Host forms of trpl_mag_grid / trpl_mag_profile (plain host code, include/trpl.h): the mag_grid loop of the reference's
probs.lnP (probs.py:5-18) from the two moments sse = sum e^2, esum = sum e.

Reference: tests/golden/lnp_maggrid.npz -- the reference's own probs.lnP on the reference PL committed in
tests/golden/pvsim_power.npz / pvsim_twothick.npz against seeded synthetic observations, per curve, with lnP's constant
n ln(pi) / 2 added back (tools/gen_golden_maggrid.py; numbers only).  Bound (include/trpl.h, derived, not measured): with
A(d) = sse + 2 |d esum| + n d^2 and eps = 2^-52,
    |P_grid - P_direct| <= k eps (A(d) + |d| sum|e_i|),
k = the depth of the summation that made the moments + 4 for the polynomial.  The moments are summed here the way the FAST
steppers sum them (_batched_sum: a binary tree inside each batch of 64 columns, the batches added serially), so
k = 6 + ceil(n / 64) + 4, the header's figure; nothing is added to the bound."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
OFFSETS = np.linspace(-2.5, 2.5, 21)


def _batched_sum(v):
    """Sum over the last axis as PlSink::flush_batch does: a 6-level tree inside each 64-column batch, batches in order."""
    n = v.shape[-1]
    total = np.zeros(v.shape[:-1])
    for b in range(0, n, 64):
        t = np.zeros(v.shape[:-1] + (64,))
        t[..., :min(64, n - b)] = v[..., b:b + 64]
        while t.shape[-1] > 1:
            t = t[..., 0::2] + t[..., 1::2]
        total = total + t[..., 0]
    return total


def _golden(key):
    g = np.load(os.path.join(ROOT, "tests", "golden", "lnp_maggrid.npz"))
    assert np.array_equal(g["offsets"], OFFSETS)
    return g["obs_" + key], g["mag_" + key], g["P_ref_" + key]


def _errors(name, key):
    """e[c][s][i] = log10 PL + mag - obs, formed like lnP forms it (probs.py:7-11), from the fixture's reference PL and the
    golden's observations and offsets."""
    pl = np.asarray(np.load(os.path.join(ROOT, "tests", "golden", name))["plI"], dtype=np.float64)       # (C, S, n)
    assert (pl > 0).all()
    obs, mag, _ = _golden(key)
    e = np.log10(pl) + mag[None, :, None]
    e -= obs[:, None, :]
    return e


def _call_grid(trpl, sse, esum, n_obs, offsets, P=None):
    A = trpl._abi
    C, S = sse.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.float64)
    P = np.zeros((len(offsets), S)) if P is None else P
    A.check(A.lib().trpl_mag_grid(A.ptr(sse), A.ptr(esum), A.ptr(n_obs), S, C, A.ptr(offsets), len(offsets), A.ptr(P)))
    return P


def _call_profile(trpl, sse, esum, n_obs, per_curve=False):
    A = trpl._abi
    C, S = sse.shape
    best = np.zeros((C, S) if per_curve else S)
    P = np.zeros(S)
    A.check(A.lib().trpl_mag_profile(A.ptr(sse), A.ptr(esum), A.ptr(n_obs), S, C, A.MAG_PER_CURVE if per_curve else 0,
                                     A.ptr(best), A.ptr(P)))
    return best, P


@pytest.mark.parametrize("name,key", [("pvsim_power.npz", "power"), ("pvsim_twothick.npz", "twothick")])
def test_grid_equals_the_references_lnp_within_the_derived_bound(trpl, name, key):
    e = _errors(name, key)
    P_ref = _golden(key)[2]                                                              # (C, S, M)
    C, S, n = e.shape
    sse = np.ascontiguousarray(_batched_sum(e * e))
    esum = np.ascontiguousarray(_batched_sum(e))
    n_obs = np.full(C, n, dtype=np.int64)
    P = _call_grid(trpl, sse, esum, n_obs, OFFSETS)
    k = 6 + -(-n // 64) + 4
    worst = 0.0
    for m, d in enumerate(OFFSETS):
        A_d = sse + 2 * np.abs(d * esum) + n * d * d
        bound = k * EPS * (A_d + abs(d) * np.abs(e).sum(axis=2))                        # the header's bound, as stated
        err = np.abs(P[m] - P_ref[:, :, m].sum(axis=0))
        worst = max(worst, float((err / bound.sum(axis=0)).max()))
        assert (err <= bound.sum(axis=0)).all(), (name, d, float((err / bound.sum(axis=0)).max()))
        for c in range(C):                                                               # and curve by curve
            Pc = _call_grid(trpl, sse[c:c + 1], esum[c:c + 1], n_obs[:1], [d])[0]
            assert (np.abs(Pc - P_ref[c, :, m]) <= bound[c]).all(), (name, c, d)
    print("%s: n = %d, k = %d, worst error / bound = %.3f" % (name, n, k, worst))
    # accumulates into P (like probs.prob), evaluated as written
    P2 = _call_grid(trpl, sse, esum, n_obs, OFFSETS[:3], P=np.full((3, S), 5.0))
    want = np.full((3, S), 5.0)
    for m, d in enumerate(OFFSETS[:3]):
        acc = np.zeros(S)
        for c in range(C):
            acc = acc + np.maximum((sse[c] + (2.0 * d) * esum[c]) + n * (d * d), 0.0)
        want[m] = want[m] - acc
    assert np.array_equal(P2, want)


def test_profile_equals_the_grid_at_best_and_best_minimises(trpl):
    e = _errors("pvsim_power.npz", "power")
    C, S, n = e.shape
    sse = np.ascontiguousarray((e * e).sum(axis=2))
    esum = np.ascontiguousarray(e.sum(axis=2))
    n_obs = np.full(C, n, dtype=np.int64)
    best, P = _call_profile(trpl, sse, esum, n_obs)
    acc = np.zeros(S)
    for c in range(C):
        acc = acc + esum[c]
    assert np.array_equal(best, (0.0 - acc) / float(C * n))
    for s in range(S):                                                                   # bit for bit the grid at best[s]
        assert _call_grid(trpl, sse, esum, n_obs, [best[s]])[0, s] == P[s]
    fine = best[None, :] + np.linspace(-0.01, 0.01, 41)[:, None]                         # best minimises over a fine grid
    for s in range(0, S, max(1, S // 8)):
        Pf = _call_grid(trpl, sse, esum, n_obs, fine[:, s])[:, s]
        assert P[s] >= Pf.max() - 8 * EPS * abs(P[s]) and np.argmax(Pf) in (19, 20, 21)
    bc, Pc = _call_profile(trpl, sse, esum, n_obs, per_curve=True)
    assert np.array_equal(bc, (0.0 - esum) / float(n))
    for s in range(0, S, max(1, S // 4)):
        acc = 0.0
        for c in range(C):
            acc = acc - _call_grid(trpl, sse[c:c + 1], esum[c:c + 1], n_obs[:1], [bc[c, s]])[0, s]
        assert Pc[s] == -acc
    assert (Pc >= P).all()                                                               # more freedom, no worse a fit


def test_flagged_systems_and_empty_calls(trpl):
    A = trpl._abi
    sse = np.array([[1.0, np.inf, 2.0, 3.0], [1.5, 0.5, 2.5, np.nan]])
    esum = np.array([[0.5, np.nan, -1.0, 1.0], [0.25, 0.1, np.inf, 1.0]])
    n_obs = np.array([10, 12], dtype=np.int64)
    P = _call_grid(trpl, sse, esum, n_obs, [-1.0, 0.0, 0.7])
    assert np.isfinite(P[:, 0]).all() and (P[:, 1:] == -np.inf).all()
    assert P[1, 0] == -(1.0 + 1.5)
    best, Pp = _call_profile(trpl, sse, esum, n_obs)
    assert np.isfinite(best[0]) and np.isnan(best[1:]).all() and (Pp[1:] == -np.inf).all() and np.isfinite(Pp[0])
    bc, Pc = _call_profile(trpl, sse, esum, n_obs, per_curve=True)
    assert np.isnan(bc[0, 1]) and np.isfinite(bc[1, 1]) and np.isnan(bc[1, 2]) and np.isnan(bc[1, 3]) and (Pc[1:] == -np.inf).all()
    # cancellation below zero is clamped: sse = n d^2 and esum = -n d exactly  ->  0, never a negative "squared error"
    # (sse a little below n d^2: the unclamped polynomial is negative -- asserted -- and P stays exactly 0)
    sse_z, d_z = 0.09 * 10 * (1 - 1e-12), 0.3
    assert (sse_z + (2.0 * d_z) * -3.0) + 10.0 * (d_z * d_z) < 0.0
    Pz = _call_grid(trpl, np.array([[sse_z]]), np.array([[-3.0]]), n_obs[:1], [d_z])
    assert Pz[0, 0] == 0.0
    # M = 0 and S = 0 are no-ops that touch nothing
    lib = A.lib()
    guard = np.full(4, 7.0)
    assert lib.trpl_mag_grid(A.ptr(sse), A.ptr(esum), A.ptr(n_obs), 4, 2, None, 0, A.ptr(guard)) == 0
    assert lib.trpl_mag_grid(None, None, A.ptr(n_obs), 0, 2, A.ptr(guard), 4, None) == 0
    assert lib.trpl_mag_profile(None, None, A.ptr(n_obs), 0, 2, 0, None, None) == 0
    assert (guard == 7.0).all()
    assert lib.trpl_mag_grid(A.ptr(sse), A.ptr(esum), A.ptr(n_obs), 4, 0, A.ptr(guard), 1, A.ptr(guard)) == A.ERR_ARG
