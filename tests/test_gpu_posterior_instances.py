"""The posterior core (csrc/posterior.hip) against extended-precision references (tests/highprec.py), at every compiled size and
regime: moments2_partial<4 | 8 | 13 | 16> on both edges of each size and with one to four samples per thread (the two-deep
prefetch turns over); the weights with -inf and NaN likelihoods; hist_kernel with an edge table and with computed edges
(kMaxAxisTab = 1024), with 16 .. 1 LDS replicas and with global atomics (kLdsBins = 4096), below and above its grid cap, on
samples that sit on every edge and next to it.  tests/test_highprec_host.py proves the references and that the inputs leave
fp64 a tenfold margin under the moment bounds.  DESIGN.md section 14 lists which test covers which kernel."""
import numpy as np
import pytest

import highprec as hp
from highprec import LD

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float64).tiny


# ------------------------------------------------------------------------------------------------ moments
def check_moments(got, want, D, label):
    sums, central = got
    assert np.array_equal(central[:, :D], central[:, :D].T), label                         # exactly symmetric
    err = hp.moment_errors(sums, central, *want)
    print("%s: error / bound  sums %.3g  cov %.3g  third %.3g  fourth %.3g" % (label, err["sums"], err["cov"], err["third"],
                                                                              err["fourth"]))
    assert max(err.values()) <= 1.0, (label, err)


@pytest.mark.parametrize("D,S", hp.MOMENT_CASES)
def test_moments_at_every_compiled_size(gpu, D, S):
    """sums rtol 1e-12; covariance entries 1e-10 sd_d sd_e sums[0]; third sums 1e-9 sd^3 sums[0]; fourth sums rtol 1e-9."""
    po = gpu.posterior
    V, LL, _ = hp.moment_inputs(D, S)
    W = po.weights(LL, hp.MOMENT_TF)
    keep = V.copy(), W.copy()
    got = po.moments(V, W)
    assert np.array_equal(V, keep[0]) and np.array_equal(W, keep[1])
    check_moments(got, hp.moments(V, W), D, "D=%d S=%d" % (D, S))


@pytest.mark.parametrize("D,S", hp.MEAN_IN_CASES)
def test_moments_about_given_means(gpu, D, S):
    """mean_in: all of central about means half a standard deviation off this call's own; sums are unaffected."""
    po = gpu.posterior
    V, LL, sd = hp.moment_inputs(D, S)
    W = po.weights(LL, hp.MOMENT_TF)
    m = hp.shifted_means(V, W, sd)
    got = po.moments(V, W, mean_in=m)
    own = po.moments(V, W)
    assert np.array_equal(got[0], own[0]) and not np.array_equal(got[1], own[1])
    check_moments(got, hp.moments(V, W, mean_in=m), D, "mean_in D=%d S=%d" % (D, S))


# ------------------------------------------------------------------------------------------------ weights
def weight_case(S, variant):
    if variant == "equal":
        return np.full(S, -1234.5)
    LL = hp.loglik(S, seed=23)
    if S > 5:
        LL[3] = -np.inf
        if variant == "inf_nan":
            rng = np.random.default_rng(29)
            LL[1:][rng.random(S - 1) < 0.01] = np.nan
            LL[5] = np.nan
    return LL


@pytest.mark.parametrize("variant", ["inf", "inf_nan", "equal"])
@pytest.mark.parametrize("tf", [10.0, 300.0, 1e6])
@pytest.mark.parametrize("S", [1, 255, 257, hp.GRID + 300])
def test_weights_against_longdouble(gpu, S, tf, variant):
    """rtol 1e-13 where finite, exact 0 at -inf, NaN exactly where LL is NaN, the finite sum within 1e-13 of 1, info["max"]
    exact.  A weight below the smallest normal double has no 1e-13 in fp64: there one spacing of the format (2^-1074) is
    added to the allowance.

    The reference's expression taken operation by operation in fp64 (utils.py:164, numpy itself) does NOT meet this at tf = 10:
    it rounds LL / tf, the difference to the maximum and the lifted exponent, each by up to 5.7e-14 at magnitudes 512 .. 1024,
    and is 1.2e-13 .. 1.4e-13 off the longdouble form at S = 255 and S = GRID + 300 (tests/test_highprec_host.py).  The kernel
    puts those roundings back (posterior_common.hpp, tempered_weight); DESIGN.md section 14 has the account."""
    po = gpu.posterior
    LL = weight_case(S, variant)
    keep = LL.copy()
    info = {}
    W = po.weights(LL, tf, info=info)
    assert np.array_equal(LL, keep, equal_nan=True)
    want = hp.weights(LL, tf)
    nan, ninf = np.isnan(LL), np.isneginf(LL)
    assert np.array_equal(np.isnan(W), nan) and (W[ninf] == 0).all()
    assert info["max"] == np.nanmax(LL / tf)
    fin = ~nan & ~ninf
    err = np.abs(W[fin].astype(LD) - want[fin])
    allow = 1e-13 * want[fin] + np.where(want[fin] < TINY, 2.0 ** -1074, 0.0)
    nrm = want[fin] >= TINY
    print("S=%d tf=%g %s: max rel err %.3e over %d normal weights; sum - 1 = %.3e" % (
        S, tf, variant, float(np.max(err[nrm] / want[fin][nrm])), nrm.sum(), float(np.nansum(W.astype(LD)) - 1)))
    assert abs(np.nansum(W.astype(LD)) - 1) <= 1e-13
    assert (err <= allow).all()
    if variant == "equal":
        assert (W == W[0]).all()


# ------------------------------------------------------------------------------------------------ histograms
def check_hist(po, x, w, lo, hi, bins, y=None, ylo=0.0, yhi=1.0, ybins=1, label=""):
    e = hp.edges(lo, hi, bins)
    ey = hp.edges(ylo, yhi, ybins) if y is not None else None
    kw = dict(y=y, ylo=ylo, yhi=yhi, ybins=ybins) if y is not None else {}
    want_n, want_w = hp.hist(x, None, e, y, ey), hp.hist(x, w, e, y, ey)
    got_n, got_w = po.hist(x, None, lo, hi, bins, **kw), po.hist(x, w, lo, hi, bins, **kw)
    bad = np.argwhere(got_n != want_n)
    assert not len(bad), "%s: %d bin(s) miscounted, first %s: got %g, numpy's rule gives %g" % (
        label, len(bad), bad[0].tolist(), got_n[tuple(bad[0])], want_n[tuple(bad[0])])
    assert np.allclose(got_w, want_w, rtol=1e-12, atol=1e-15 * float(np.sum(w))), label


@pytest.mark.parametrize("lo,hi", hp.HIST_RANGES)
@pytest.mark.parametrize("S", hp.HIST_SIZES)
@pytest.mark.parametrize("bins", hp.HIST_BINS_1D)
def test_hist_1d_on_every_edge_in_every_regime(gpu, bins, S, lo, hi):
    """Counts equal numpy's rule on the reference's edge array (the LAST EDGE closes the range, not hi); weighted counts rtol
    1e-12, atol 1e-15 sum w."""
    rng = np.random.default_rng(1000 + bins)
    x = hp.hist_points(rng, lo, hi, bins, S)
    check_hist(gpu.posterior, x, rng.random(S), lo, hi, bins, label="1-D bins=%d S=%d (%g, %g)" % (bins, S, lo, hi))


@pytest.mark.parametrize("lo,hi", hp.HIST_RANGES)
@pytest.mark.parametrize("S", hp.HIST_SIZES)
@pytest.mark.parametrize("xb,yb", hp.HIST_BINS_2D)
def test_hist_2d_on_every_edge_in_every_regime(gpu, xb, yb, S, lo, hi):
    """x on (lo, hi), y on the next range of the list; 64 x 64 fills the LDS bins exactly, 64 x 65 is the first size on global
    atomics, 1025 on either axis computes that axis's edges while the other reads its table."""
    ylo, yhi = hp.HIST_RANGES[(hp.HIST_RANGES.index((lo, hi)) + 1) % len(hp.HIST_RANGES)]
    rng = np.random.default_rng(2000 + xb + 7 * yb)
    x, y = hp.hist_points(rng, lo, hi, xb, S), hp.hist_points(rng, ylo, yhi, yb, S)
    check_hist(gpu.posterior, x, rng.random(S), lo, hi, xb, y, ylo, yhi, yb,
               label="2-D %d x %d S=%d (%g, %g) x (%g, %g)" % (xb, yb, S, lo, hi, ylo, yhi))


# ------------------------------------------------------------------------------------------------ the host-buffer forms' optional pointers
@pytest.mark.parametrize("S", [1, 257])
def test_host_forms_without_their_optional_pointers(gpu, S):
    """stats NULL (weights), mean_in NULL (moments), y and W NULL (hist), one sample and one block boundary: the bits of the calls
    that pass them; the plain counts exactly numpy's."""
    A_, po = gpu._abi, gpu.posterior
    rng = np.random.default_rng(S)
    LL = -50.0 * rng.random(S)
    W = np.full(S, -7.0)
    sec = A_.C.c_double(-1.0)
    A_.check(A_.lib().trpl_posterior_weights(A_.ptr(LL), S, 10.0, A_.ptr(W), None, 0, A_.C.byref(sec)))
    assert np.array_equal(W, po.weights(LL, 10.0)) and sec.value > 0.0
    V = np.ascontiguousarray(rng.normal(size=(4, S)))
    sums, central = np.full(6, -7.0), np.full((4, 6), -7.0)
    A_.check(A_.lib().trpl_posterior_moments(A_.ptr(V), S, 4, A_.ptr(W), None, A_.ptr(sums), A_.ptr(central), 0, None))
    got = po.moments(V, W)
    assert np.array_equal(sums, got[0]) and np.array_equal(central, got[1])
    x = np.ascontiguousarray(V[0])
    out = np.full(8, -7.0)
    A_.check(A_.lib().trpl_posterior_hist(A_.ptr(x), None, None, S, -1.0, 1.0, 8, 0.0, 1.0, 1, A_.ptr(out), 0, A_.C.byref(sec)))
    assert np.array_equal(out, np.histogram(x, bins=8, range=(-1.0, 1.0))[0].astype(np.float64)) and sec.value > 0.0


def test_weights_of_no_samples_return_at_once(gpu):
    """S == 0: TRPL_OK, seconds 0, W and stats as they were."""
    A_ = gpu._abi
    W, stats = np.full(4, -7.0), np.full(2, -7.0)
    sec = A_.C.c_double(-1.0)
    A_.check(A_.lib().trpl_posterior_weights(None, 0, 10.0, A_.ptr(W), A_.ptr(stats), 0, A_.C.byref(sec)))
    assert sec.value == 0.0 and np.all(W == -7.0) and np.all(stats == -7.0)
