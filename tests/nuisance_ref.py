"""trpl_nuisance_reduce restated in NumPy (include/trpl.h): the three cell rules and both reductions with their loops in the stated
order -- responses, offsets, curves ascending, one rounded operation at a time (NumPy's elementwise operators fuse nothing) -- an
extended-precision value of the marginal from given fp64 cells, and the cells the host and the device tests share."""
import ctypes

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18                    # the x87 format: 64 bits of mantissa against the 53 under test
INF, NAN = np.inf, np.nan
FIXED, GRID, PROFILE = "fixed", "grid", "profile"


def mag_term(sse, esum, n, d):
    """likelihood.hip's mag_term: (sse + (2 d) esum) + n (d d), clamped at 0; +inf for a flagged system or NaN / inf moments."""
    with np.errstate(invalid="ignore", over="ignore"):
        t1 = (2.0 * d) * esum
        t2 = n * (d * d)
        v = (sse + t1) + t2
        bad = ~(sse < INF) | ~((esum - esum) == 0.0) | (v != v)
        return np.where(bad, INF, np.where(v < 0.0, 0.0, v))


def cells(sse, esum, wsum, mode, offsets=None):
    """v (J M, S) and the offset of each cell (J M, S), from sse, esum (C, J, S) and wsum (C,); cell i = j M + m."""
    Cn, J, S = sse.shape
    M = len(offsets) if mode == GRID else 1
    v, dm = np.empty((J * M, S)), np.empty((J * M, S))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(J):
            if mode == FIXED:
                acc = np.zeros(S)
                for c in range(Cn):
                    acc = acc + sse[c, j]
                v[j], dm[j] = 0.0 - acc, 0.0
            elif mode == PROFILE:
                E, N, ok = np.zeros(S), 0.0, np.ones(S, dtype=bool)
                for c in range(Cn):
                    E = E + esum[c, j]
                    N = N + wsum[c]
                    ok &= sse[c, j] < INF
                d = (0.0 - E) / np.float64(N)
                acc = np.zeros(S)
                for c in range(Cn):
                    acc = acc + mag_term(sse[c, j], esum[c, j], wsum[c], d)
                nothing = (N == 0.0) & ok
                v[j] = np.where(nothing, 0.0, 0.0 - acc)
                dm[j] = np.where(~nothing & ok & ((E - E) == 0.0), d, NAN)
            else:
                for m in range(M):
                    acc = np.zeros(S)
                    for c in range(Cn):
                        acc = acc + mag_term(sse[c, j], esum[c, j], wsum[c], np.float64(offsets[m]))
                    v[j * M + m], dm[j * M + m] = 0.0 - acc, offsets[m]
    return v, dm


def greatest(a, dm):
    """The greatest a[i] per sample, the first i that attains it and dm there; NaN never the greatest; all -inf or NaN: -inf, -1, NaN."""
    n, S = a.shape
    p, best, mag = np.full(S, -INF), np.full(S, -1, dtype=np.int32), np.full(S, NAN)
    for i in range(n):
        with np.errstate(invalid="ignore"):
            up = a[i] > p
        p[up], best[up], mag[up] = a[i][up], i, dm[i][up]
    return p, best, mag


def tempered(v, tf, logw):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return v / np.float64(tf) + (np.zeros(len(v)) if logw is None else np.asarray(logw, dtype=np.float64))[:, None]


def marginal(v, dm, tf, logw=None):
    """The two passes in fp64: (P, best, best_mag)."""
    a = tempered(v, tf, logw)
    mx, best, mag = greatest(a, dm)
    total = np.zeros(a.shape[1])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(len(a)):
            t = a[i] - mx
            total = total + np.where(t == t, np.exp(t), 0.0)
        P = np.where(best >= 0, np.float64(tf) * (mx + np.log(total)), -INF)
    return P, best, mag


def marginal_exact(v, tf, logw=None):
    """(R, B) per sample: R = tf (MX + ln sum_i exp(A_i - MX)) with A_i = v_i / tf + logw_i in extended precision from the fp64 cells
    (a NaN cell counts as -inf), and B = the greatest |v_i| / tf + |logw_i| over the cells with a finite A_i (0 where there is none)."""
    n, S = v.shape
    lw = np.zeros(n, dtype=LD) if logw is None else np.asarray(logw, dtype=np.float64).astype(LD)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A = v.astype(LD) / LD(tf) + lw[:, None]
        A = np.where(np.isnan(A), -INF, A)
        MX = A.max(axis=0)
        fin = np.isfinite(A)
        size = np.where(fin, np.abs(v.astype(LD)) / LD(tf) + np.abs(np.where(np.isfinite(lw), lw, 0))[:, None], 0)
        B = size.max(axis=0).astype(np.float64)
        R = np.full(S, -INF, dtype=LD)
        live = np.isfinite(MX)
        R[live] = LD(tf) * (MX[live] + np.log(np.exp(A[:, live] - MX[live]).sum(axis=0)))
    return R, B


def bound(lib, tf, B, n, R):
    """The header's TRPL_NUISANCE_BOUND per sample, from the library (trpl_nuisance_bound)."""
    return np.array([lib.trpl_nuisance_bound(float(tf), float(b), int(n), float(r)) if np.isfinite(r) else 0.0 for b, r in zip(B, R)])


def inside(P, R, bnd):
    """|P - R| <= bound wherever R is finite, and P == R = -inf elsewhere (the difference is taken in extended precision)."""
    fin = np.isfinite(R)
    return bool(np.all(np.abs(P[fin].astype(LD) - R[fin]) <= bnd[fin]) and np.all(P[~fin] == -INF) and np.all(np.isfinite(P[fin])))


def moments(Cn, J, S, seed, special=True):
    """sse, esum (C, J, S) and integer-valued wsum (C,): moments of about n_c observations with an error of a few tenths.  With special
    (where the shape has room): sample 0 holds a flagged cell (sse = +inf, esum = NaN) in response 0; sample 1 is flagged in every cell;
    sample 2 repeats response 0 in response 1 (an exact tie, the first cell wins); sample 3 has moments no curve can have (a large
    esum under a small sse), so that the quadratic is negative between its roots and takes the clamp; sample 4 holds a NaN sse."""
    rng = np.random.default_rng(seed)
    wsum = rng.integers(5, 40, Cn).astype(np.float64)
    mean = rng.normal(0.0, 0.3, (Cn, J, S))
    esum = wsum[:, None, None] * mean
    sse = wsum[:, None, None] * (mean * mean + rng.uniform(0.01, 0.2, (Cn, J, S)))
    if special:
        sse[0, 0, 0], esum[0, 0, 0] = INF, NAN
        if S > 1:
            sse[:, :, 1], esum[:, :, 1] = INF, NAN
        if S > 2 and J > 1:
            sse[:, 1, 2], esum[:, 1, 2] = sse[:, 0, 2], esum[:, 0, 2]
        if S > 3:
            sse[:, :, 3], esum[:, :, 3] = 0.01, wsum[:, None] * 0.5
        if S > 4:
            sse[Cn - 1, J - 1, 4] = NAN
    return np.ascontiguousarray(sse), np.ascontiguousarray(esum), wsum


OFFSETS = np.array([-0.5, -0.125, 0.0, 0.3, 1.0])            # -0.5 sits between the roots of sample 3's quadratic


def mode_flags(A, mode, marg):
    return {FIXED: A.NUISANCE_MAG_FIXED, GRID: A.NUISANCE_MAG_GRID, PROFILE: A.NUISANCE_MAG_PROFILE}[mode] | (A.NUISANCE_MARGINAL if marg else 0)


def host(trpl, sse, esum, wsum, mode, offsets=None, marg=False, tf=1.0, logw=None, outputs=True):
    """trpl_nuisance_reduce on host arrays -> (P, best, best_mag); canaries behind every output are checked."""
    A = trpl._abi
    Cn, J, S = sse.shape
    M = len(offsets) if mode == GRID else 1
    P, best, mag = np.full(S + 2, -7.0), np.full(S + 2, -9, dtype=np.int32), np.full(S + 2, -7.0)
    ptr = lambda a: None if a is None else a.ctypes.data
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64)
    lw = None if logw is None else np.ascontiguousarray(logw, dtype=np.float64)
    A.check(A.lib().trpl_nuisance_reduce(ptr(sse), ptr(esum), ptr(wsum), S, Cn, J, ptr(off), M, ptr(lw), ctypes.c_double(tf),
                                         mode_flags(A, mode, marg), ptr(P), ptr(best) if outputs else None, ptr(mag) if outputs else None))
    assert np.all(P[S:] == -7.0) and np.all(best[S:] == -9) and np.all(mag[S:] == -7.0)
    return (P[:S], best[:S], mag[:S]) if outputs else (P[:S], None, None)
