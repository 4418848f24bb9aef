"""Extended-precision references for the stand-alone kernels (batched tridiagonal solve, posterior core) and the inputs their
tests share (tests/test_highprec_host.py proves both on the CPU; tests/test_gpu_pcr_instances.py and
tests/test_gpu_posterior_instances.py hold the kernels to them).  Plain helper module: numpy.longdouble (64-bit mantissa on
x86-64), math.fsum where a sum of doubles must be exact.  Nothing here imports the product package."""
import math

import numpy as np

LD = np.longdouble

PCR_SIZES = (4, 8, 16, 32, 64, 128, 256, 512)     # the compiled L of pcr_batched_kernel
GRID = 256 * 1024                                 # kThreads * kMaxBlocks of csrc/posterior_common.hpp: one sample per thread
HIST_GRID = 768 * 256                             # the histogram's own grid cap (launch_posterior_hist)


# ------------------------------------------------------------------------------------------------ tridiagonal solve
def pcr_family(seed, S, L):
    """The matrix family of tests/test_gpu_pcr.py: ld, ud ~ U(-1, 1), d ~ U(2.5, 4) (diagonally dominant), b ~ N(0, 1)."""
    rng = np.random.default_rng(seed)
    ld = rng.uniform(-1, 1, (S, L)); ud = rng.uniform(-1, 1, (S, L)); d = rng.uniform(2.5, 4, (S, L))
    ld[:, 0] = 0; ud[:, -1] = 0
    b = rng.normal(size=(S, L))
    return ld, d, ud, b


def thomas(ld, d, ud, b, dtype=LD):
    """Plain Thomas elimination (one forward sweep, one back substitution) over a batch [S][L], every operation in `dtype`:
    longdouble is the reference, float32 gives the error of a plain fp32 solver on the same operands."""
    ld, d, ud, b = (np.atleast_2d(np.asarray(a)).astype(dtype) for a in (ld, d, ud, b))
    S, L = d.shape
    c = np.empty((S, L), dtype=dtype); g = np.empty((S, L), dtype=dtype)
    c[:, 0] = ud[:, 0] / d[:, 0]
    g[:, 0] = b[:, 0] / d[:, 0]
    for i in range(1, L):
        den = d[:, i] - ld[:, i] * c[:, i - 1]
        c[:, i] = ud[:, i] / den
        g[:, i] = (b[:, i] - ld[:, i] * g[:, i - 1]) / den
    x = np.empty((S, L), dtype=dtype)
    x[:, L - 1] = g[:, L - 1]
    for i in range(L - 2, -1, -1):
        x[:, i] = g[:, i] - c[:, i] * x[:, i + 1]
    return x


def fp32_case(ld, d, ud, b):
    """What the fp32 kernels are held to: the operands rounded to float32, the exact (longdouble Thomas) solution of that
    rounded system, and per system the largest error of Thomas run in float32 on the same operands.  The kernels' bound is
    8 x the largest of those over the systems solved (cyclic reduction + PCR has up to log2 L <= 9 elimination levels where
    Thomas has one sweep)."""
    f = [np.ascontiguousarray(a, dtype=np.float32) for a in (ld, d, ud, b)]
    want = thomas(*f)
    plain = np.max(np.abs(thomas(*f, dtype=np.float32).astype(LD) - want), axis=1).astype(np.float64)
    return f, want, plain


# ------------------------------------------------------------------------------------------------ posterior core
def weights(LL, tf):
    """oracle/posterior.py:normalize(LL / tf) in longdouble: NaN stays NaN (and out of max and sum), -inf gives 0."""
    LL = np.asarray(LL, dtype=np.float64).astype(LD)
    q = LL / LD(tf)
    with np.errstate(invalid="ignore"):
        w = np.exp(q - np.nanmax(q) + LD(1000) * np.log(LD(2)) - np.log(LD(LL.size)))
    return w / np.nansum(w)


def moments(V, W, mean_in=None):
    """sums[2 + D] = {sum w, sum w^2, sum w v_d} and central[D][D + 2] = {sum w (v_d - m_d)(v_e - m_e), sum w (v_d - m_d)^3,
    sum w (v_d - m_d)^4} as trpl_posterior_moments defines them (m = sums[2:] / sums[0] unless mean_in): two passes, longdouble."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64)).astype(LD)
    W = np.asarray(W, dtype=np.float64).astype(LD)
    D = V.shape[0]
    sums = np.empty(2 + D, dtype=LD)
    sums[0] = W.sum(); sums[1] = (W * W).sum(); sums[2:] = (V * W).sum(axis=1)
    mean = sums[2:] / sums[0] if mean_in is None else np.asarray(mean_in, dtype=np.float64).astype(LD)
    xc = V - mean[:, None]
    central = np.empty((D, D + 2), dtype=LD)
    for d in range(D):
        xw = xc[d] * W
        central[d, d:D] = (xc[d:] * xw).sum(axis=1)
        central[d:D, d] = central[d, d:D]
        x2 = xc[d] * xc[d]
        central[d, D] = (x2 * xw).sum()
        central[d, D + 1] = (x2 * x2 * W).sum()
    return sums, central


def moments_fp64(V, W, mean_in=None):
    """The same formulae in plain numpy float64 (pairwise sums): what fp64 itself can deliver on the inputs."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64)); W = np.asarray(W, dtype=np.float64)
    D = V.shape[0]
    sums = np.concatenate([[W.sum(), (W * W).sum()], (V * W).sum(axis=1)])
    mean = sums[2:] / sums[0] if mean_in is None else np.asarray(mean_in, dtype=np.float64)
    xc = V - mean[:, None]
    central = np.empty((D, D + 2))
    for d in range(D):
        central[d, :D] = (xc * xc[d] * W).sum(axis=1)
        central[d, D] = (xc[d] ** 3 * W).sum()
        central[d, D + 1] = (xc[d] ** 4 * W).sum()
    return sums, central


def moment_errors(sums, central, want_sums, want_central):
    """The four figures the moment bounds are written in, each as error / allowance (<= 1 passes): sums rtol 1e-12; covariance
    entries 1e-10 sd_d sd_e sums[0]; third sums 1e-9 sd^3 sums[0]; fourth sums rtol 1e-9 (sd^2 = central[d][d] / sums[0] of the
    reference).  An allowance of 0 (one sample: every central sum is exactly 0) demands equality."""
    D = len(want_sums) - 2
    sums, central = np.asarray(sums).astype(LD), np.asarray(central).astype(LD)
    sw = want_sums[0]
    sd = np.sqrt(np.diag(want_central[:, :D]) / sw)

    def ratio(err, allow):
        err, allow = np.asarray(err, dtype=LD), np.asarray(allow, dtype=LD)
        out = np.zeros(err.shape, dtype=LD)
        nz = allow > 0
        out[nz] = err[nz] / allow[nz]
        out[~nz & (err != 0)] = np.inf
        return float(np.max(out))

    return {"sums": ratio(np.abs(sums - want_sums), 1e-12 * np.abs(want_sums)),
            "cov": ratio(np.abs(central[:, :D] - want_central[:, :D]), 1e-10 * np.outer(sd, sd) * sw),
            "third": ratio(np.abs(central[:, D] - want_central[:, D]), 1e-9 * sd ** 3 * sw),
            "fourth": ratio(np.abs(central[:, D + 1] - want_central[:, D + 1]), 1e-9 * np.abs(want_central[:, D + 1]))}


def hist(x, w, e, y=None, ey=None):
    """Weighted counts (w None: plain counts) of x in the bins of the explicit edge array e -- with y and ey, [x bin][y bin] --
    by numpy.histogram's rules (oracle.posterior.bin_index), every bin an exact sum (math.fsum) rounded once."""
    from oracle.posterior import bin_index
    x = np.asarray(x, dtype=np.float64)
    k = bin_index(x, np.asarray(e, dtype=np.float64))
    shape = (len(e) - 1,)
    ok = k >= 0
    if y is not None:
        ky = bin_index(np.asarray(y, dtype=np.float64), np.asarray(ey, dtype=np.float64))
        ok &= ky >= 0
        k = k * (len(ey) - 1) + ky
        shape = (len(e) - 1, len(ey) - 1)
    n = int(np.prod(shape))
    if w is None:
        return np.bincount(k[ok], minlength=n).astype(np.float64).reshape(shape)
    k, w = k[ok], np.asarray(w, dtype=np.float64)[ok]
    order = np.argsort(k, kind="stable")
    k, w = k[order], w[order]
    out = np.zeros(n)
    first = np.flatnonzero(np.diff(k, prepend=-1))
    for a, b in zip(first, np.append(first[1:], len(k))):
        out[k[a]] = math.fsum(w[a:b].tolist())
    return out.reshape(shape)


def edges(lo, hi, bins):
    """The reference's edge array (Visualization/utils.py:243-244), in float64 as it computes it."""
    return lo + (hi - lo) * np.arange(bins + 1) / bins


# ------------------------------------------------------------------------------------------------ posterior inputs
S_MAX = 3 * GRID + 5
MOMENT_TF = 3000.0                # LL spans 1e4: weights within e^-3.3 of each other, every sample counts
_columns = {}


def loglik(S, seed=11):
    """LL = -1e4 U(0, 1) with 2 % of the samples at -inf (never the first one: a batch of one sample keeps a finite weight)."""
    rng = np.random.default_rng(seed)
    LL = -1e4 * rng.random(S)
    LL[1:][rng.random(S - 1) < 0.02] = -np.inf
    return LL


def columns():
    """16 columns of S_MAX samples, built once: M @ gamma(2, 1) with M = I + 0.3 N(0, 1) (real covariances, skew near 1.4,
    fourth moments away from 0), column d scaled by 10^k, k in [-3, 3], and shifted by up to 1e3 of its standard deviations.
    Returns (V [16][S_MAX], sd [16] of the scaled columns, LL [S_MAX])."""
    if not _columns:
        rng = np.random.default_rng(2024)
        M = np.eye(16) + 0.3 * rng.normal(size=(16, 16))
        V = M @ rng.gamma(2.0, 1.0, (16, S_MAX))
        V *= (10.0 ** rng.integers(-3, 4, 16))[:, None]
        sd = V.std(axis=1)
        shift = rng.uniform(-1e3, 1e3, 16)
        shift[[0, 12, 15]] = [1e3, -1e3, 1e3]               # the first column and the last of DM = 13 / 16 at the largest offset
        V += (shift * sd)[:, None]
        _columns.update(V=V, sd=sd, LL=loglik(S_MAX))
    return _columns["V"], _columns["sd"], _columns["LL"]


MOMENT_DIMS = (1, 4, 5, 8, 9, 13, 14, 16)                  # both edges of each compiled DM (4, 8, 13, 16)
MOMENT_SIZES = (1, 2, 255, 256, 257, 513)
MOMENT_SIZES_DEEP = (GRID + 300, 2 * GRID + 300, 3 * GRID + 5)     # two, three and four samples per thread (D = 13, 16)
MOMENT_CASES = [(D, S) for D in MOMENT_DIMS for S in MOMENT_SIZES] + [(D, S) for D in (13, 16) for S in MOMENT_SIZES_DEEP]
MEAN_IN_CASES = [(13, 257), (13, GRID + 300)]


def moment_inputs(D, S):
    V, sd, LL = columns()
    return np.ascontiguousarray(V[:D, :S]), LL[:S].copy(), sd[:D]


def shifted_means(V, W, sd):
    """The means of a sharded caller that are not this call's own: half a standard deviation off."""
    m = (V * W).sum(axis=1) / W.sum()
    return m + 0.5 * sd * np.where(np.arange(len(sd)) % 2 == 0, 1.0, -1.0)


# ------------------------------------------------------------------------------------------------ histogram inputs
HIST_RANGES = ((0.1, 0.9), (0.2, 0.9), (0.1, 0.3), (-3.0, 9.0))
HIST_BINS_1D = (1, 100, 128, 129, 1024, 1025, 2048, 4096, 4097)     # 100: the last edge of (0.1, 0.3) is above hi
HIST_BINS_2D = ((64, 64), (64, 65), (1025, 3), (3, 1025))
HIST_SIZES = (1, 1000, HIST_GRID + 77)


def hist_points(rng, lo, hi, bins, S):
    """S samples for one histogram axis.  In this order, cut to S and then shuffled: hi, the last edge and its two neighbours,
    NaN, +-inf, values outside the range, the first edge and its neighbours, every other edge with its two neighbours (a
    random order of edges), then U(lo - 0.1, hi + 0.1).  One sample is `hi` itself; S >= 3 bins + 14 holds every edge."""
    e = edges(lo, hi, bins)
    last = e[-1]
    head = [hi, last, np.nextafter(last, -np.inf), np.nextafter(last, np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
            np.nan, np.inf, -np.inf, lo - 1.0, hi + 5.0, e[0], np.nextafter(e[0], -np.inf), np.nextafter(e[0], np.inf)]
    inner = e[1:-1][rng.permutation(max(bins - 1, 0))]
    body = np.stack([inner, np.nextafter(inner, -np.inf), np.nextafter(inner, np.inf)], axis=1).ravel()
    x = np.concatenate([head, body])[:S]
    x = np.concatenate([x, rng.uniform(lo - 0.1, hi + 0.1, S - len(x))])
    return x[rng.permutation(S)]
