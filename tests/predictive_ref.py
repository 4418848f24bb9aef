"""Extended-precision reference of the posterior-predictive band (trpl_predictive*, include/trpl.h) and the inputs its tests
share: tests/test_predictive_host.py proves reference, allowances and inputs on the CPU, tests/test_gpu_predictive.py holds the
kernels to them.  A helper, not a test; nothing here imports the product package.

The band of a matrix y [rows][ncol] of model values under weights W over the rows `used`, per column:
    sw = sum W,  mean = sum W y / sw,  var = sum W (y - mean)^2 / sw,  lo = min y,  hi = max y
(min / max skip a NaN).  A column with a y that is not finite in a used row has mean = var = NaN (the header's NaN rule)."""
import sys

import numpy as np

LD = np.longdouble
FIELDS = ("mean", "var", "lo", "hi", "sw")
DBL_MIN = sys.float_info.min


def _band(y, W, used, dtype):
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    W = np.asarray(W, dtype=np.float64)
    used = np.asarray(used, dtype=bool)
    ncol = y.shape[1]
    if not used.any():
        nan = np.full(ncol, np.nan, dtype=dtype)
        return {"mean": nan, "var": nan.copy(), "lo": np.full(ncol, np.inf, dtype=dtype), "hi": np.full(ncol, -np.inf, dtype=dtype),
                "sw": np.zeros(ncol, dtype=dtype), "scale": nan.copy()}
    yy, w = y[used].astype(dtype), W[used].astype(dtype)[:, None]
    bad = ~np.isfinite(yy).all(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        sw = w.sum()
        mean = (w * yy).sum(axis=0) / sw                                  # first pass
        var = (w * (yy - mean) ** 2).sum(axis=0) / sw                     # second pass, about that mean
        scale = (w * np.abs(yy)).sum(axis=0) / sw
        lo, hi = np.fmin.reduce(yy, axis=0), np.fmax.reduce(yy, axis=0)
    mean[bad] = np.nan
    var[bad] = np.nan
    return {"mean": mean, "var": var, "lo": lo, "hi": hi, "sw": np.full(ncol, sw, dtype=dtype), "scale": scale}


def band_ref(y, W, used):
    """The band in numpy.longdouble (64-bit mantissa on x86-64), two passes.  Also returns scale = sum W |y| / sw, the size
    the mean's allowance is written in."""
    return _band(y, W, used, LD)


def band_fp64(y, W, used):
    """The same two passes in plain float64: what fp64 itself delivers on the inputs."""
    return _band(y, W, used, np.float64)


def used_rows(W, status=None):
    """The header's rule: W finite and > 0, and status absent or 0."""
    W = np.asarray(W, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        u = np.isfinite(W) & (W > 0)
    return u if status is None else u & (np.asarray(status) == 0)


def errors(got, want):
    """error / allowance per field (<= 1 passes), with the figures of highprec.moment_errors: mean within
    1e-12 sum W |y| / sw, var within 1e-10 var_ref, lo, hi and sw within 1e-12 relative.  An allowance of 0 (one used row, a
    constant column: var_ref = 0) demands equality; so do infinite entries; a NaN must meet a NaN."""
    def ratio(g, w, allow):
        g, w, allow = (np.asarray(a).astype(LD) for a in (g, w, allow))
        out = np.zeros(w.shape, dtype=LD)
        fin = np.isfinite(w) & np.isfinite(g)
        with np.errstate(invalid="ignore"):
            err = np.abs(g - w)
        pos = fin & (allow > 0)
        out[pos] = err[pos] / allow[pos]
        out[fin & ~pos & (err != 0)] = np.inf
        same = (np.isnan(g) & np.isnan(w)) | (g == w)                   # what is not finite on either side must be identical
        out[~fin & ~same] = np.inf
        return float(np.max(out)) if out.size else 0.0

    with np.errstate(invalid="ignore"):
        return {"mean": ratio(got["mean"], want["mean"], 1e-12 * want["scale"]),
                "var": ratio(got["var"], want["var"], 1e-10 * want["var"]),
                "lo": ratio(got["lo"], want["lo"], 1e-12 * np.abs(want["lo"])),
                "hi": ratio(got["hi"], want["hi"], 1e-12 * np.abs(want["hi"])),
                "sw": ratio(got["sw"], want["sw"], 1e-12 * np.abs(want["sw"]))}


# ------------------------------------------------------------------------------------------------ inputs
def pl_family(seed, rows, ncol, ld, dtype):
    """PL [rows][ld] of `dtype`: log-uniform in [1e-30, 1e30] with 3 % exact zeros (never in column 0, which TRPL_FLAG_NORMALIZE
    divides by); the ld - ncol padding columns hold NaN -- nothing may read them."""
    rng = np.random.default_rng(seed)
    pl = 10.0 ** rng.uniform(-30, 30, (rows, ld))
    pl[:, 1:][rng.random((rows, ld - 1)) < 0.03] = 0.0
    pl[:, ncol:] = np.nan
    return np.ascontiguousarray(pl.astype(dtype))


def ll_family(seed, rows):
    """Log-likelihoods whose posterior weights (tf = 1) are exactly 0.0 on ~70 % of the rows (1e5 below the best: exp
    underflows), with some -inf and one NaN (weight NaN: an unused row); row 0 is always among the best."""
    rng = np.random.default_rng(seed + 7)
    LL = -50.0 * rng.random(rows)
    LL[rng.random(rows) < 0.7] -= 1e5
    LL[rng.random(rows) < 0.05] = -np.inf
    if rows > 2:
        LL[rng.integers(1, rows)] = np.nan
    LL[0] = -1.0
    return LL


def mag_family(seed, rows):
    return np.random.default_rng(seed + 13).uniform(-3, 3, rows)


def weights_np(LL):
    """normalize(LL) of Visualization/utils.py:157-166 in float64 NumPy (the host tests' stand-in for posterior.weights)."""
    LL = np.asarray(LL, dtype=np.float64)
    with np.errstate(invalid="ignore", under="ignore"):
        w = np.exp(LL - np.nanmax(LL) + 1000 * np.log(2) - np.log(LL.size))
        return w / np.nansum(w)


def y_numpy(pl, ncol, mag=None, normalize=False):
    """The model values by NumPy's log10 (the host tests' stand-in for the device function: the same value up to an ulp):
    optional division by column 0 in the buffer's dtype, the clamp at DBL_MIN cast to that dtype (0 for float32), log10 in
    fp64 rounded to the dtype, + mag in fp64."""
    v = np.array(pl[:, :ncol])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if normalize:
            v = v / v[:, :1]
        v[v.astype(np.float64) < DBL_MIN] = v.dtype.type(DBL_MIN)
        y = np.log10(v.astype(np.float64)).astype(v.dtype).astype(np.float64)
    return y if mag is None else y + np.asarray(mag, dtype=np.float64)[:, None]


def chunk_rows(chunks_of, ncol, elem):
    """The largest row count the exported rule chunks_of(rows, ncol, elem) keeps in ONE chunk (the rule's shortest chunk), and
    the smallest row count that gives at least three chunks with a shorter last one."""
    one = 1
    while chunks_of(one + 1, ncol, elem) == 1:
        one += 1
    r = 2 * one + 1
    while True:
        k = chunks_of(r, ncol, elem)
        per = -(-r // k)
        if k >= 3 and r % per:
            return one, r
        r += 1
