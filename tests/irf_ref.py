"""The NumPy restatement of trpl_convolve_irf's definition (include/trpl.h) and seeded case builders:
tests/test_irf_host.py proves the restatement on the CPU, tests/test_gpu_irf.py holds the kernel to it bit for bit.  Plain
helper module: nothing here imports the product package."""
import functools

import numpy as np

CANARY = -7.0                                      # what the padding of a leading dimension carries


def convolve_ref(pl, h, k0, ncol=None):
    """out[r][j] = sum over k ascending of h[k] * (double)pl[r][j + k0 - k], 0 <= j < ncol - k0: an fp64 accumulator from +0.0,
    one rounded product and one rounded addition per term, the terms left of column 0 skipped; the sum rounded once to pl's
    dtype.  Returns (rows, ncol - k0) in pl's dtype."""
    pl = np.asarray(pl)
    h = np.asarray(h, dtype=np.float64)
    ncol = pl.shape[1] if ncol is None else int(ncol)
    ncol_out = ncol - int(k0)
    assert 0 <= k0 < len(h) and ncol_out >= 1 and pl.dtype in (np.float32, np.float64)
    pl64 = pl[:, :ncol].astype(np.float64)
    acc = np.zeros((pl.shape[0], ncol_out))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(len(h)):
            lo = max(0, k - k0)                    # the first output whose column j + k0 - k is not negative
            if lo >= ncol_out:
                break
            acc[:, lo:] += h[k] * pl64[:, lo + k0 - k:ncol_out + k0 - k]
        return acc.astype(pl.dtype)


def taps(K, seed):
    """K taps of mixed sign and of magnitudes over 12 decades, so that a reordered or fused sum shows in the bits."""
    rng = np.random.default_rng(977 * K + seed)
    return rng.choice([-1.0, 1.0], K) * 10.0 ** rng.uniform(-6.0, 6.0, K)


@functools.lru_cache(maxsize=None)
def block(rows, ncol, dtype, seed=0):
    """PL rows [rows][ncol + 3] in `dtype`: positive lognormal values over 12 decades with a few negative ones, the padding
    holding CANARY.  Read-only: shared between the cases of a test."""
    rng = np.random.default_rng(31 * rows + 7 * ncol + seed)
    pl = np.full((rows, ncol + 3), CANARY, dtype=dtype)
    v = np.exp(rng.normal(0.0, 4.6, (rows, ncol)))
    v[rng.random((rows, ncol)) < 0.05] *= -1.0
    pl[:, :ncol] = v.astype(dtype)
    pl.setflags(write=False)
    return pl


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))
