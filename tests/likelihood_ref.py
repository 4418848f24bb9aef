"""References and seeded inputs for the stand-alone likelihood kernels of csrc/likelihood.hip (log10 clamp, squared-error
accumulation, the likelihood of stored PL rows, the mag grid): tests/test_likelihood_ref_host.py proves them on the CPU against
the oracle, tests/test_gpu_likelihood_instances.py holds every launch path of the kernels to them.  Plain helper module:
numpy.longdouble (64-bit mantissa on x86-64) where a logarithm or a sum must carry no error of its own, float64 one operation
at a time where the kernel's own roundings are restated.  Nothing here imports the product package or the oracle."""
import functools

import numpy as np

LD = np.longdouble
DBL_MIN = float(np.finfo(np.float64).tiny)
FLAG_PL_F32, FLAG_NORMALIZE = 0x2, 0x4             # TRPL_FLAG_PL_F32, TRPL_FLAG_NORMALIZE (include/trpl.h)
SENTINEL = -7.0                                    # what the padding of a leading dimension carries
MINS = {"float32": (DBL_MIN, 1e-30, 1e-300), "float64": (DBL_MIN, 1e-30)}
DIFFER_CAP = 1e-4                                  # float32: at most 0.01 % of the elements differ from the correctly rounded value


def longdouble_is_extended():
    return np.finfo(LD).nmant >= 63


# ------------------------------------------------------------------------------------------------ log10 clamp
def log10_clamp_ref(x, mn):
    """log10_clamp_one: the clamp value is stored as (T)mn first (float32: 0 for mn = DBL_MIN or 1e-300, hence -inf), NaN is
    not below anything and stays NaN; the logarithm in longdouble, rounded once to T."""
    x = np.asarray(x)
    T = x.dtype.type
    with np.errstate(under="ignore"):
        mn_t = T(mn)
    v = np.where(x.astype(np.float64) < mn, mn_t, x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log10(v.astype(LD)).astype(T)


def clamp_specials(dtype, mn):
    """0, -0.0, -1, a denormal, mn itself, the value below it, 1.0 and its two neighbours, the largest finite value, +inf, NaN."""
    T = np.dtype(dtype).type
    fi = np.finfo(T)
    with np.errstate(under="ignore"):
        mn_t = T(mn)
    return np.array([0.0, -0.0, -1.0, fi.smallest_subnormal * T(3), mn_t, np.nextafter(mn_t, T(0)), 1.0, np.nextafter(T(1), T(0)),
                     np.nextafter(T(1), T(2)), fi.max, np.inf, np.nan], dtype=T)


def clamp_values(shape, dtype, mn, seed):
    """Lognormal over 30 decades (+-3 sigma) with the special values of clamp_specials: scattered twice over a large buffer and
    once more over its last elements (the scalar tail of the flat kernel); rotating through every other element of a small one."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = np.exp(rng.normal(0.0, 30.0 * np.log(10.0) / 6.0, n)).astype(dtype)
    sp = clamp_specials(dtype, mn)
    k = len(sp)
    if n < 4 * k:
        j = np.arange(seed % 2, n, 2)
        x[j] = sp[(j // 2 + seed) % k]
    else:
        x[rng.choice(n - k, 2 * k, replace=False)] = np.tile(sp, 2)
        x[n - k + rng.permutation(k)[:k // 2]] = sp[rng.permutation(k)[:k // 2]]
    return x.reshape(shape)


def ulps(got, want):
    """|got - want| in units of the spacing of `want`'s type at want (finite elements only make sense)."""
    want = np.asarray(want)
    with np.errstate(invalid="ignore"):
        return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def same_classes(got, want):
    """-inf, +inf and NaN in the same places."""
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
            and np.array_equal(np.isneginf(got), np.isneginf(want)))


# ------------------------------------------------------------------------------------------------ squared-error accumulation
def sse_ref(P0, pl, values, mag, wts=None):
    """The serial loop of probs.py:29-44 over the columns, vectorised over the rows, float64, one rounding per operation:
    e = pl + mag; e = e - v; acc = acc + e * e  (times w[i] when weighted);  P0 + (0 - acc)."""
    pl = np.asarray(pl)
    acc = np.zeros(pl.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(pl.shape[1]):
            e = pl[:, i].astype(np.float64) + mag
            e = e - values[i]
            acc = acc + ((e * e) * wts[i] if wts is not None else e * e)
        return P0 + (0.0 - acc)


def weights(n, seed):
    """As grid_cases.weights: one exact 0, one power of two, random positive values over three decades."""
    rng = np.random.default_rng(1000 + seed)
    w = 10.0 ** rng.uniform(-1.5, 1.5, n)
    w[70 % n] = 0.25
    w[n // 3] = 0.0
    return w


@functools.lru_cache(maxsize=4)
def sse_inputs(rows, n_obs, ld, special):
    """PL rows uniform in +-3 in a [rows][ld] float64 buffer (the padding holds SENTINEL; the tests cast it), observations,
    offsets, weights and a non-zero P.  special: row 1 of the last block but one holds a NaN, the row after it a +inf in the
    column whose weight is zero (unweighted: -inf; weighted: 0 * inf = NaN)."""
    rng = np.random.default_rng(rows * 7919 + n_obs)
    pl = np.full((rows, ld), SENTINEL)
    pl[:, :n_obs] = rng.uniform(-3.0, 3.0, (rows, n_obs))
    out = dict(pl=pl, values=rng.uniform(-3.0, 3.0, n_obs), mag=rng.uniform(-1.0, 1.0, rows), P0=rng.normal(size=rows),
               wts=weights(n_obs, n_obs), bad=())
    if special:
        r = max(0, rows - 20)
        pl[r + 1, n_obs - 2] = np.nan
        pl[r + 2, n_obs // 3] = np.inf
        out["bad"] = (r + 1, r + 2)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ likelihood of stored PL rows
def log_pl_ref(pl, normalize, f32):
    """log_pl (csrc/log_pl.hpp) as float64 values: normalisation to column 0, clamp at DBL_MIN ((float)DBL_MIN = 0 under the
    float32 staging), log10 in longdouble rounded once to the staging type."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if f32:
            f = pl.astype(np.float32)
            if normalize:
                f = f / f[:, :1]
            f = np.where(f.astype(np.float64) < DBL_MIN, np.float32(0.0), f)
            return np.log10(f.astype(LD)).astype(np.float32).astype(np.float64)
        d = pl.astype(np.float64)
        if normalize:
            d = d / d[:, :1]
        d = np.where(d < DBL_MIN, DBL_MIN, d)
        return np.log10(d.astype(LD)).astype(np.float64)


def from_pl_ref(pl, obs, mag, flags, brackets=None, wts=None):
    """pl_loglik_kernel's terms restated in float64 one operation at a time -- log_pl; off the grid (dy / h) * dx + lg_lo with dy
    the float32 difference under the float32 staging; e = y + mag; e = e - obs -- and summed in longdouble.  brackets: (hi, dx, h).
    Returns dict(sse, esum, abs: sum (w) e^2, sum (w) e, sum (w) |e| per row, longdouble; lg: the log10 PL).  A row whose sum
    of squares is NaN reports what the kernel reports for it: sse = +inf, esum = NaN."""
    pl = np.asarray(pl)
    f32 = bool(flags & FLAG_PL_F32) or pl.dtype == np.float32
    lg = log_pl_ref(pl, bool(flags & FLAG_NORMALIZE), f32)
    n = len(obs)
    with np.errstate(invalid="ignore", over="ignore"):
        if brackets is None:
            y = lg[:, :n]
        else:
            hi, dx, h = brackets
            lg_hi, lg_lo = lg[:, hi], lg[:, hi - 1]
            dy = (lg_hi.astype(np.float32) - lg_lo.astype(np.float32)).astype(np.float64) if f32 else lg_hi - lg_lo
            y = (dy / h[None, :]) * dx[None, :] + lg_lo
        e = y + np.asarray(mag)[:, None]
        e = e - np.asarray(obs)[None, :]
        w = np.ones(n) if wts is None else np.asarray(wts)
        t2, t1 = ((e * e) * w[None, :]).astype(LD), (e * w[None, :]).astype(LD)
        sse, esum, mag1 = t2.sum(axis=1), t1.sum(axis=1), np.abs(t1).sum(axis=1)
    nan = np.isnan(sse)
    sse[nan], esum[nan] = np.inf, np.nan
    return dict(sse=sse, esum=esum, abs=mag1, lg=lg, n=n)


@functools.lru_cache(maxsize=None)
def pl_case(rows, n_obs, offgrid):
    """Positive lognormal PL rows [rows][ncol + 3] float64 (padding SENTINEL; ncol = max(n_obs, 2)), observations near their
    log10, offsets, weights.  With three rows, row 1 holds one 0 (the clamp at DBL_MIN) in a column every case reads.  Off the
    grid: sorted brackets that include hi = 1 and hi = ncol - 1, one time exactly on a grid point (dx = 0) and one exactly on
    the next (dx = h)."""
    rng = np.random.default_rng(31 * n_obs + rows + (7 if offgrid else 0))
    ncol = max(n_obs, 2)
    pl = np.full((rows, ncol + 3), SENTINEL)
    pl[:, :ncol] = np.exp(rng.normal(30.0, 3.0, (rows, ncol)))
    zero_col = None
    if rows == 3 and ncol > 2:
        zero_col = ncol // 2
        pl[1, zero_col] = 0.0
    out = dict(pl=pl, ncol=ncol, mag=rng.uniform(-1.0, 1.0, rows), obs=rng.normal(13.0, 1.5, n_obs), wts=weights(n_obs, n_obs + 1),
               zero_col=zero_col, brackets=None)
    if offgrid:
        hi = np.sort(rng.integers(1, ncol, n_obs)).astype(np.int32)
        hi[0], hi[-1] = 1, ncol - 1
        if zero_col is not None:
            hi[n_obs // 2] = zero_col
            hi.sort()
        h = np.full(n_obs, 0.025)
        dx = rng.uniform(0.0, 0.025, n_obs)
        dx[0] = 0.0
        dx[-1] = h[-1]
        out["brackets"] = (hi, dx, h)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ mag grid
CANCEL_D = 0.3                                     # offsets[0] of every grid: where the cancelling entry's polynomial is below 0


def mag_offsets(M):
    rng = np.random.default_rng(M)
    d = rng.uniform(-1.5, 1.5, M)
    d[0] = CANCEL_D
    return d


def mag_moments(S, C, weighted, seed=3):
    """Moments [C][S] for trpl_mag_grid[_w] / trpl_mag_profile[_w]: finite sums of squares and of errors; n_obs (int64) or wsum
    (float64, with one curve of weight 0 when C > 1); a non-zero P.  Sample 0, curve 0: sse = n d^2 (1 - 1e-12), esum = -n d
    at d = CANCEL_D, so the polynomial cancels below zero there and the clamp at 0 acts (tests/test_likelihood_ref_host.py
    asserts that it is negative).  With S > 8: flagged entries (sse = +inf, esum = NaN) in samples 3 and S // 2, an infinite esum
    under a finite sse in sample 5 (on a curve whose weight is not zero)."""
    rng = np.random.default_rng(seed + 64 * S + C)
    if weighted:
        n = 10.0 ** rng.uniform(0.0, 3.0, C)
        if C > 1:
            n[C // 2] = 0.0
    else:
        n = rng.integers(1, 400, C).astype(np.int64)
    nf = np.asarray(n, dtype=np.float64)
    e_rms = 10.0 ** rng.uniform(-2.0, 0.0, (C, S))
    sse = nf[:, None] * e_rms ** 2 * rng.uniform(1.0, 2.0, (C, S))
    esum = nf[:, None] * e_rms * rng.uniform(-1.0, 1.0, (C, S))
    if nf[0] > 0:
        sse[0, 0], esum[0, 0] = nf[0] * (CANCEL_D * CANCEL_D) * (1 - 1e-12), -nf[0] * CANCEL_D
    if S > 8:
        sse[0, 3], esum[0, 3] = np.inf, np.nan
        sse[C - 1, S // 2], esum[C - 1, S // 2] = np.inf, np.nan
        esum[(C // 2 + 1) % C, 5] = np.inf
    return dict(sse=np.ascontiguousarray(sse), esum=np.ascontiguousarray(esum), n=n, P0=rng.normal(size=S))


def mag_poly(sse, esum, n, d):
    """The unclamped polynomial as the header writes it: (sse + (2 d) esum) + n (d d), float64."""
    return (sse + (2.0 * d) * esum) + n * (d * d)
