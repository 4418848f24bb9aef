"""tests/highprec.py on the CPU: the extended-precision references the stand-alone kernels are held to agree with the oracle and
the reference's golden within the project's tolerances, and the shared inputs leave fp64 itself a tenfold margin under every
bound of tests/test_gpu_posterior_instances.py.  No GPU needed."""
import math

import numpy as np
import pytest

import highprec as hp
from highprec import LD


def test_platform_longdouble_has_a_64_bit_mantissa():
    assert np.finfo(LD).nmant >= 63


# ------------------------------------------------------------------------------------------------ tridiagonal solve
@pytest.mark.parametrize("L", hp.PCR_SIZES)
def test_oracle_pcreduce_is_the_exact_solution_to_rounding(oracle, L):
    """oracle.pcreduce (the reference's elimination order, fp64) within 1e-14 max |x| of longdouble Thomas (measured
    <= 4.2e-16), and the longdouble solution's residual at the longdouble rounding level."""
    ld, d, ud, b = hp.pcr_family(100 + L, 67, L)
    want = hp.thomas(ld, d, ud, b)
    got = np.array([oracle.pcreduce(ld[s], d[s], ud[s], b[s]) for s in range(67)])
    assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want))
    r = d * want; r[:, 1:] += ld[:, 1:] * want[:, :-1]; r[:, :-1] += ud[:, :-1] * want[:, 1:]
    assert np.max(np.abs(r - b)) < 1e-17
    # one system against mpmath at 50 digits
    import mpmath
    mpmath.mp.dps = 50
    if L <= 64:
        A = mpmath.zeros(L)
        for i in range(L):
            A[i, i] = mpmath.mpf(float(d[0, i]))
            if i: A[i, i - 1] = mpmath.mpf(float(ld[0, i]))
            if i < L - 1: A[i, i + 1] = mpmath.mpf(float(ud[0, i]))
        x = mpmath.lu_solve(A, mpmath.matrix([mpmath.mpf(float(v)) for v in b[0]]))
        assert max(abs(x[i] - mpmath.mpf(float(want[0, i])) - mpmath.mpf(float(want[0, i] - LD(float(want[0, i])))))
                   for i in range(L)) < 1e-18


@pytest.mark.parametrize("L", hp.PCR_SIZES)
def test_plain_fp32_thomas_sets_the_fp32_bound(L):
    """On this family a float32 Thomas solve is within 1.0e-7 .. 2.3e-7 of the exact solution of the rounded system, so the
    kernels' bound, 8 x that, is at least 5 x tighter than the 2e-5 it replaces at every L."""
    f, want, plain = hp.fp32_case(*hp.pcr_family(100 + L, 67, L))
    assert all(a.dtype == np.float32 for a in f) and want.dtype == LD and plain.shape == (67,)
    assert 5e-8 < plain.max() < 4e-7 and 8 * plain.max() < 2e-5 / 5


# ------------------------------------------------------------------------------------------------ weights
def test_longdouble_weights_agree_with_the_oracle_and_the_golden(golden):
    from oracle import posterior as op
    g = golden("posterior")
    _, LL = op.filter_nan(g["X"], g["LL"])
    w = hp.weights(LL, float(g["tf"]))
    assert np.allclose(w.astype(np.float64), g["P"], rtol=1e-13, atol=0) and (w[np.isinf(LL)] == 0).all()
    assert abs(w.sum() - 1) < 1e-18
    LL = hp.loglik(1000)
    LL[7] = np.nan
    for tf in (10.0, 300.0, 1e6):
        w = hp.weights(LL, tf)
        wo = op.weights(LL, tf)
        assert np.isnan(w[7]) and np.isnan(wo[7]) and (w[np.isneginf(LL)] == 0).all() and abs(np.nansum(w) - 1) < 1e-18
        # The fp64 expression rounds the quotient, the difference and the lifted exponent (up to max(1e4 / tf, 693)): half an
        # ulp of it each, 5.7e-14 at 512 .. 1024 -- so fp64 itself is NOT within 1e-13 of the longdouble form at tf = 10
        # (measured 1.3e-13 at 262 444 samples, 6e-14 at tf >= 300).  Weights below the smallest normal double are compared
        # by the format's spacing instead (fp64 has no 1e-13 there; 6e-403 is 0).
        ulp = np.spacing(max(1e4 / tf, 1000 * math.log(2)))
        nrm = w >= np.finfo(np.float64).tiny
        assert nrm.sum() > 600 and float(np.max(np.abs(wo[nrm] / w[nrm] - 1))) < 1.5 * ulp + 1e-14, tf
        sub = np.isfinite(LL) & ~nrm
        assert sub.sum() >= 100 * (tf == 10.0) and (np.abs(wo[sub] - w[sub]) <= 1.5 * ulp * w[sub] + 2.0 ** -1074).all()


# ------------------------------------------------------------------------------------------------ moments
def test_longdouble_moments_agree_with_the_oracle_and_the_golden(golden):
    from oracle import posterior as op
    g = golden("posterior")
    X, LL = op.filter_nan(g["X"], g["LL"])
    P = g["P"]
    cols = np.stack([np.log10(X[:, i]) if lg else X[:, i] for i, lg in zip(g["col_index"], g["col_log"])])
    D = len(cols)
    s, c = hp.moments(cols, P)
    assert np.array_equal(c[:, :D], c[:, :D].T)
    f = lambda a: np.asarray(a).astype(np.float64)
    assert np.allclose(f(s[2:] / s[0]), g["mean"], rtol=1e-12) and np.isclose(float(s[1]), float(g["ws"]), rtol=1e-12)
    assert np.allclose(f(c[:, :D] / s[0]), g["cov"], rtol=1e-9, atol=1e-18)
    var = np.diag(c[:, :D]) / s[0]
    assert np.allclose(f(var), g["var"], rtol=1e-10)
    assert np.allclose(f(c[:, D] / s[0] / var ** 1.5), g["skew"], rtol=1e-9)
    assert np.allclose(f(c[:, D + 1] / s[0] / var ** 2), g["kurt"], rtol=1e-9)
    for k in range(D):
        assert np.isclose(float(var[k]), op.w_variance(cols[k], P), rtol=1e-10)
        assert np.isclose(float(c[k, (k + 1) % D] / s[0]), op.covariance(cols[k], cols[(k + 1) % D], P), rtol=1e-9, atol=1e-18)
    # about given means: the definition, term by term
    m = f(s[2:] / s[0]) + 0.25
    _, c2 = hp.moments(cols, P, mean_in=m)
    want = math.fsum(((cols[0] - m[0]) * (cols[1] - m[1]) * P).tolist())
    assert np.isclose(float(c2[0, 1]), want, rtol=1e-12)


def test_the_moment_inputs_are_what_the_issue_describes():
    V, sd, LL = hp.columns()
    assert V.shape == (16, hp.S_MAX) and hp.S_MAX == 3 * hp.GRID + 5
    off = np.abs(V.mean(axis=1)) / sd
    assert off.max() <= 1.01e3 and off[[0, 12, 15]].min() > 990
    lg = np.log10(sd)
    assert lg.min() > -3.5 and lg.max() < 4.0 and lg.max() - lg.min() > 3            # scales 1e-3 .. 1e3 (sd of M @ gamma ~ 1.5 .. 3)
    z = (V[:, :200000] - V[:, :200000].mean(axis=1, keepdims=True)) / V[:, :200000].std(axis=1, keepdims=True)
    skew, corr = (z ** 3).mean(axis=1), np.corrcoef(z)
    assert skew.max() > 0.9 and np.median(skew) > 0.3 and np.abs(corr - np.eye(16)).max() > 0.3 and ((z ** 4).mean(axis=1) > 3).all()
    assert np.isfinite(LL[0]) and 0.015 < np.isneginf(LL).mean() < 0.025 and LL[np.isfinite(LL)].min() < -9999


@pytest.mark.parametrize("D,S", hp.MOMENT_CASES + [(-D, S) for D, S in hp.MEAN_IN_CASES])
def test_fp64_has_a_tenfold_margin_under_every_moment_bound(D, S):
    """A condition on the inputs, checked without the kernel: plain numpy float64 evaluation of the moment formulae is within
    one tenth of each bound the kernels are held to (D < 0: the mean_in case of |D| columns)."""
    from oracle import posterior as op
    V, LL, sd = hp.moment_inputs(abs(D), S)
    W = op.weights(LL, hp.MOMENT_TF)
    m = hp.shifted_means(V, W, sd) if D < 0 else None
    want = hp.moments(V, W, mean_in=m)
    assert np.array_equal(want[1][:, :abs(D)], want[1][:, :abs(D)].T)
    err = hp.moment_errors(*hp.moments_fp64(V, W, mean_in=m), *want)
    assert max(err.values()) <= 0.1, err


# ------------------------------------------------------------------------------------------------ histograms
def test_last_edge_is_not_always_hi():
    """The reference's last edge lo + (hi - lo) * bins / bins: below hi for (0.2, 0.9) at every bin count, above hi for
    (0.1, 0.3) at 100 bins and (0.1, 0.9) at 3, hi itself for (0.1, 0.9) at 10 -- and numpy's rule follows the EDGE, not hi."""
    from oracle import posterior as op
    for bins in hp.HIST_BINS_1D + (3, 10, 64, 65, 100):
        assert hp.edges(0.2, 0.9, bins)[-1] == 0.8999999999999999 < 0.9
        assert np.array_equal(hp.edges(0.2, 0.9, bins), op.edges(0.2, 0.9, bins))
    assert hp.edges(0.1, 0.9, 10)[-1] == 0.9 and hp.edges(0.1, 0.9, 3)[-1] == 0.9000000000000001 > 0.9
    assert 100 in hp.HIST_BINS_1D and (3, 1025) in hp.HIST_BINS_2D          # both "above" cases reach the device
    e = hp.edges(0.1, 0.3, 100)
    assert e[-1] == 0.30000000000000004 > 0.3
    x = np.array([0.9, 0.8999999999999999])
    assert np.array_equal(hp.hist(x, None, hp.edges(0.2, 0.9, 10)), np.histogram(x, bins=hp.edges(0.2, 0.9, 10))[0])
    assert hp.hist(x, None, hp.edges(0.2, 0.9, 10)).tolist() == [0] * 9 + [1]              # 0.9 dropped, the edge kept
    x = np.array([0.3, 0.30000000000000004])
    assert hp.hist(x, None, e)[-1] == 2 == np.histogram(x, bins=e)[0][-1]                  # both kept


@pytest.mark.parametrize("lo,hi", hp.HIST_RANGES)
def test_longdouble_histogram_is_numpys_on_the_test_points(lo, hi):
    rng = np.random.default_rng(3)
    for bins in (1, 129, 1025):
        S = 3 * bins + 14 + 500
        e = hp.edges(lo, hi, bins)
        x = hp.hist_points(rng, lo, hi, bins, S)
        assert x.shape == (S,) and np.isin(e, x).all() and np.isin(np.nextafter(e, np.inf), x).all()
        assert np.isin(np.nextafter(e, -np.inf), x).all() and hi in x and np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2
        assert hp.hist_points(rng, lo, hi, bins, 1).tolist() == [hi]
        w = rng.random(S)
        ok = ~np.isnan(x)
        assert np.array_equal(hp.hist(x, None, e), np.histogram(x[ok], bins=e)[0])
        # (numpy's weighted histogram takes differences of a running sum: 1e-16 of the TOTAL per bin)
        assert np.allclose(hp.hist(x, w, e), np.histogram(x[ok], bins=e, weights=w[ok])[0], rtol=1e-11, atol=0)
        if bins <= 129:
            ey = hp.edges(-3.0, 9.0, 7)
            y = hp.hist_points(rng, -3.0, 9.0, 7, S)
            ok = ~np.isnan(x) & ~np.isnan(y)
            assert np.array_equal(hp.hist(x, None, e, y, ey), np.histogram2d(x[ok], y[ok], bins=[e, ey])[0])
            assert np.allclose(hp.hist(x, w, e, y, ey), np.histogram2d(x[ok], y[ok], bins=[e, ey], weights=w[ok])[0], rtol=1e-11, atol=0)


def test_the_golden_histograms_follow_from_the_longdouble_counts(golden):
    from oracle import posterior as op
    g = golden("posterior")
    X, _ = op.filter_nan(g["X"], g["LL"])
    P, bins = g["P"], int(g["bins"])
    cols = [np.log10(X[:, i]) if lg else X[:, i] for i, lg in zip(g["col_index"], g["col_log"])]
    for k, c in enumerate(cols):
        if "mu" in str(g["names"][k]):
            continue                                                     # corrected for sampling: another normalisation
        e = hp.edges(*g["limits"][k], bins)
        raw = hp.hist(c, P, e)
        assert np.array_equal(e, g["edges"][k]) and np.allclose(raw / (np.diff(e) * raw.sum()), g["h1"][k], rtol=1e-11, atol=1e-15)
    for (a, b), h in zip(g["pairs"], g["h2"]):
        ex, ey = hp.edges(*g["limits"][a], bins), hp.edges(*g["limits"][b], bins)
        raw = hp.hist(cols[a], P, ex, cols[b], ey)
        assert np.allclose(raw / (np.outer(np.diff(ex), np.diff(ey)) * raw.sum()), h, rtol=1e-12, atol=1e-16)
