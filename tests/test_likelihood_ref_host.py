"""What tests/test_gpu_likelihood_instances.py assumes of tests/likelihood_ref.py, proved without a device: the serial-loop
reference is the oracle's probs.prob bit for bit; the longdouble log10 clamp agrees with the oracle's probs.fastlog within the
gates the kernels are held to; float64 log10 rounded to float32 -- what the kernel and the oracle compute -- stays within the
"differs at all" cap of the correctly rounded value on the generated inputs; the plain host forms of the mag grid accept the
sizes the device tests use, and the cancelling entry of the generated moments does reach the clamp at 0."""
import numpy as np
import pytest

import likelihood_ref as R
from likelihood_ref import LD

EPS = 2.0 ** -52


@pytest.fixture(autouse=True)
def _extended_longdouble():
    if not R.longdouble_is_extended():
        pytest.skip("numpy.longdouble has %d mantissa bits here: no extended-precision reference" % np.finfo(LD).nmant)


SHAPES = [(1, n) for n in range(1, 10)] + [(3, 171), (5, 7), (8193, 5), (2, 16390), (4, 33)]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_sse_ref_is_the_oracles_prob_bit_for_bit(oracle, dtype):
    for rows, n_obs in ((1, 1), (5, 65), (5, 577), (300, 333), (4097, 70)):
        c = R.sse_inputs(rows, n_obs, n_obs, False)
        pl = c["pl"].astype(dtype)
        P = c["P0"].copy()
        oracle.prob(P, pl, c["values"], c["mag"])
        assert np.array_equal(P, R.sse_ref(c["P0"], pl, c["values"], c["mag"])), (rows, n_obs)
        unit = R.sse_ref(c["P0"], pl, c["values"], c["mag"], np.ones(n_obs))           # unit weights change no bit
        assert np.array_equal(P, unit)
    c = R.sse_inputs(5, 577, 580, True)                                                # the NaN row and the +inf row
    pl = np.ascontiguousarray(c["pl"][:, :577]).astype(dtype)
    P = c["P0"].copy()
    oracle.prob(P, pl, c["values"], c["mag"])
    want = R.sse_ref(c["P0"], pl, c["values"], c["mag"])
    assert np.array_equal(P, want, equal_nan=True) and np.isnan(want[c["bad"][0]]) and want[c["bad"][1]] == -np.inf
    live = np.setdiff1d(np.arange(5), c["bad"])
    assert np.isfinite(want[live]).all()
    wtd = R.sse_ref(c["P0"], pl, c["values"], c["mag"], c["wts"])
    assert np.isnan(wtd[list(c["bad"])]).all() and np.isfinite(wtd[live]).all()        # 0 * inf = NaN
    assert c["wts"][577 // 3] == 0.0 and (c["wts"] == 0.25).any()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_log10_clamp_ref_agrees_with_the_oracles_fastlog_within_the_kernels_gates(oracle, dtype):
    worst = 0.0
    for mn in R.MINS[dtype]:
        for k, shape in enumerate(SHAPES):
            x = R.clamp_values(shape, dtype, mn, seed=k)
            want = R.log10_clamp_ref(x, mn)
            got = x.copy()
            oracle.fastlog(got, mn)
            assert R.same_classes(got, want), (mn, shape)
            fin = np.isfinite(want)
            if x.size > 100:
                assert np.isnan(want).any() and np.isposinf(want).any() and (want[fin] == 0.0).any()
                assert np.isneginf(want).any() == (dtype == "float32" and mn != 1e-30)     # (float)mn = 0
            u = R.ulps(got[fin], want[fin])
            worst = max(worst, float(u.max()) if u.size else 0.0)
            if dtype == "float32":
                assert (u <= 1.0).all() and np.count_nonzero(got[fin] != want[fin]) <= R.DIFFER_CAP * fin.sum(), (mn, shape)
            else:
                d = np.abs(got[fin] - want[fin])
                assert (d <= 2 * EPS * np.abs(want[fin])).all() and (d <= 4e-16 * np.abs(want[fin]).max(initial=0.0)).all(), (mn, shape)
    print("%s: the oracle's fastlog is within %.3g ulp of the longdouble reference" % (dtype, worst))


def test_float64_log10_rounded_to_float32_stays_inside_the_differ_cap():
    """The kernel's float32 result is the float32 rounding of a float64 logarithm (two roundings); the reference rounds once.
    The two differ only where the exact logarithm lies within the float64 error of a float32 rounding boundary: on the
    generated inputs, the cap-sized buffer included, far fewer than 0.01 % of the elements, and never by more than one ulp."""
    n = 256 * 8192 * 4 + 5
    for mn in R.MINS["float32"]:
        for k, shape in enumerate(SHAPES + [(1, n)]):
            x = R.clamp_values(shape, "float32", mn, seed=k)
            if x.size > 100000:
                x = x.ravel()[::64]
            want = R.log10_clamp_ref(x, mn)
            with np.errstate(under="ignore"):
                v = np.where(x.astype(np.float64) < mn, np.float32(mn), x)
            with np.errstate(divide="ignore", invalid="ignore"):
                two = np.log10(v.astype(np.float64)).astype(np.float32)
            assert R.same_classes(two, want)
            fin = np.isfinite(want)
            assert np.count_nonzero(two[fin] != want[fin]) <= R.DIFFER_CAP * fin.sum() and (R.ulps(two[fin], want[fin]) <= 1.0).all(), (mn, shape)


def test_from_pl_ref_restates_the_stored_pl_likelihood():
    """On the grid without staging the terms are log10(pl) + mag - obs; the float32 staging rounds the logarithm to float32;
    unit weights change nothing; the clamped 0 is log10(DBL_MIN) in float64 and -inf under the float32 staging (its row then
    reports sse = +inf); off the grid a time on a grid point takes that point's value."""
    c = R.pl_case(3, 257, False)
    pl = c["pl"][:, :c["ncol"]]
    r = R.from_pl_ref(pl, c["obs"], c["mag"], 0)
    live = pl[:, :257] > 0
    e = np.log10(np.where(live, pl[:, :257], R.DBL_MIN).astype(LD)) + c["mag"][:, None] - c["obs"][None, :]
    assert np.max(np.abs(r["sse"] - (e * e).sum(axis=1)) / r["sse"]) < 1e-13
    assert abs(r["lg"][1, c["zero_col"]] - np.log10(R.DBL_MIN)) < 1e-12 and np.isfinite(np.asarray(r["sse"], dtype=np.float64)).all()
    one = R.from_pl_ref(pl, c["obs"], c["mag"], 0, wts=np.ones(257))
    assert all(np.array_equal(r[k], one[k]) for k in ("sse", "esum", "abs"))
    f = R.from_pl_ref(pl, c["obs"], c["mag"], R.FLAG_PL_F32)
    assert np.array_equal(f["lg"], f["lg"].astype(np.float32).astype(np.float64)) and f["lg"][1, c["zero_col"]] == -np.inf
    assert f["sse"][1] == np.inf and np.isfinite(np.asarray(f["sse"][[0, 2]], dtype=np.float64)).all()
    assert np.array_equal(R.from_pl_ref(pl.astype(np.float32), c["obs"], c["mag"], 0)["lg"],
                          R.log_pl_ref(pl.astype(np.float32), False, True))
    nz = R.from_pl_ref(pl, c["obs"], c["mag"], R.FLAG_NORMALIZE)
    assert (nz["lg"][:, 0] == 0.0).all()
    o = R.pl_case(3, 257, True)
    hi, dx, h = o["brackets"]
    assert hi[0] == 1 and hi[-1] == o["ncol"] - 1 and dx[0] == 0.0 and dx[-1] == h[-1] and (hi == o["zero_col"]).any()
    assert (np.diff(hi) >= 0).all() and hi.min() >= 1 and hi.max() <= o["ncol"] - 1 and hi.dtype == np.int32
    opl = o["pl"][:, :o["ncol"]]
    lg = R.log_pl_ref(opl, False, False)
    first = R.from_pl_ref(opl, o["obs"][:1], o["mag"], 0, brackets=(hi[:1], dx[:1], h[:1]))
    e0 = (lg[:, 0] + o["mag"]) - o["obs"][0]
    assert np.array_equal(np.asarray(first["esum"], dtype=np.float64), e0)


def _host_grid(A, m, offsets, weighted):
    C, S = m["sse"].shape
    P = np.tile(m["P0"], (len(offsets), 1))
    fn = A.lib().trpl_mag_grid_w if weighted else A.lib().trpl_mag_grid
    A.check(fn(A.ptr(m["sse"]), A.ptr(m["esum"]), A.ptr(m["n"]), S, C, A.ptr(offsets), len(offsets), A.ptr(P)))
    return P


@pytest.mark.parametrize("weighted", [False, True], ids=["n_obs", "wsum"])
def test_host_mag_forms_accept_the_device_tests_sizes(trpl, weighted):
    """C = TRPL_MAG_MAX_CURVES and M past the 256 offsets of one device launch are ordinary sizes for the plain host forms; the
    cancelling entry is negative before the clamp and contributes exactly 0; flagged samples come out -inf, the rest finite."""
    A = trpl._abi
    assert A.MAG_MAX_CURVES == 64
    for S, C, M in ((1, 1, 1), (1000, 64, 257), (1000, 64, 300), (1000, 3, 256)):
        m = R.mag_moments(S, C, weighted)
        offsets = R.mag_offsets(M)
        nf = np.asarray(m["n"], dtype=np.float64)
        assert offsets[0] == R.CANCEL_D and R.mag_poly(m["sse"][0, 0], m["esum"][0, 0], nf[0], R.CANCEL_D) < 0.0
        P = _host_grid(A, m, offsets, weighted)
        rest = 0.0
        for c in range(1, C):
            rest = rest + max(R.mag_poly(m["sse"][c, 0], m["esum"][c, 0], nf[c], R.CANCEL_D), 0.0)
        assert P[0, 0] == m["P0"][0] - rest                                             # curve 0 added exactly 0
        dead = ~(np.isfinite(m["sse"]) & np.isfinite(m["esum"])).all(axis=0)
        assert dead.sum() == (3 if S > 8 else 0) and (P[:, dead] == -np.inf).all() and np.isfinite(P[:, ~dead]).all()
        for per_curve in (False, True):
            best, Pp = np.zeros((C, S) if per_curve else S), m["P0"].copy()
            fn = A.lib().trpl_mag_profile_w if weighted else A.lib().trpl_mag_profile
            A.check(fn(A.ptr(m["sse"]), A.ptr(m["esum"]), A.ptr(m["n"]), S, C, A.MAG_PER_CURVE if per_curve else 0, A.ptr(best),
                       A.ptr(Pp)))
            assert (Pp[dead] == -np.inf).all() and np.isfinite(Pp[~dead]).all()
            if weighted and per_curve and C > 1:
                assert np.isnan(best[C // 2]).all()                                     # the curve of weight 0 has no best offset
    m = R.mag_moments(8, 64, weighted)
    n65 = np.concatenate([np.asarray(m["n"]), np.asarray(m["n"])[:1]])
    fn = A.lib().trpl_mag_grid_w if weighted else A.lib().trpl_mag_grid
    big = np.zeros((65, 8))
    assert fn(A.ptr(big), A.ptr(big), A.ptr(n65), 8, 65, A.ptr(np.zeros(1)), 1, A.ptr(np.zeros(8))) == A.ERR_ARG
