"""Plain numpy restatement of early rejection (trpl_mcmc_levels, include/trpl.h; trpl_amd.mcmc.reject_levels): the level above which
a proposal's running squared error makes its rejection certain, and the accept predicate it is verified against -- both with log(xi)
in float64, the way the kernels form it, one rounding per operation.  Philox is mcmc_ref's (refine_ref's).  No device, no library."""
import numpy as np

import mcmc_ref as mr
import refine_ref as rr


def accept_uniform_at(chains, steps, seed):
    """xi of the accept step for every (chain, step) pair: counter (n low, n high, 0x100 + 9, step), key (seed low, seed high)."""
    n = np.asarray(chains, dtype=np.uint64)
    steps = np.broadcast_to(np.asarray(steps, dtype=np.uint64), n.shape)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    ctr = np.stack([(n & rr.MASK).astype(np.uint32), (n >> np.uint64(32)).astype(np.uint32),
                    np.full(n.shape, mr.STREAM + mr.ACCEPT_CALL, dtype=np.uint32), (steps & rr.MASK).astype(np.uint32)], axis=-1)
    r = rr.philox4x32_10(ctr, key)
    return rr.res53(r[:, 0], r[:, 1])


def accept_take(LL, LLp, tf, xi, inside=1):
    """The accept kernel's decision, its own expression: inside, LLp neither NaN nor -inf, and the chain not above -inf, or
    d = (LLp - LL) / tf >= 0, or log(xi) < d."""
    LL, LLp, tf, xi = (np.asarray(v, dtype=np.float64) for v in (LL, LLp, tf, xi))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (LLp - LL) / tf
        return (np.asarray(inside) != 0) & ~np.isnan(LLp) & (LLp > -np.inf) & (~(LL > -np.inf) | (d >= 0.0) | (np.log(xi) < d))


def _verified(l, LL, tf, lx):
    """The candidate l is safe: with q = -l the accept step's dq = (q - LL) / tf is negative and not above log(xi)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dq = (-l - LL) / tf
        return (dq < 0.0) & ~(lx < dq)


def first_candidate(LL, tf, xi):
    """l0 = -(LL + tf log(xi))"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return -(np.asarray(LL, dtype=np.float64) + np.asarray(tf, dtype=np.float64) * np.log(np.asarray(xi, dtype=np.float64)))


def levels_from_xi(LL, tf, xi):
    """level per element: l0, else l0 + (|LL| + l0) 2^-40, whichever is verified first; +inf when LL is NaN or not above -inf, when
    xi == 0, or when neither is."""
    with np.errstate(divide="ignore"):
        return levels_from_log(LL, tf, xi, np.log(np.asarray(xi, dtype=np.float64)))


def levels_from_log(LL, tf, xi, lx):
    """levels_from_xi with log(xi) given: the rule for any rounding of the logarithm."""
    LL, tf, xi, lx = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (LL, tf, xi, lx)))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l0 = -(LL + tf * lx)
        l1 = l0 + (np.abs(LL) + l0) * 2.0 ** -40
        usable = ~np.isnan(LL) & (LL > -np.inf) & (xi != 0.0)
        ok0, ok1 = _verified(l0, LL, tf, lx), _verified(l1, LL, tf, lx)
    return np.where(usable & ok0, l0, np.where(usable & ok1, l1, np.inf))


def levels(LL, tf, chain0, seed, step):
    """trpl_mcmc_levels: chain i of LL (count,) is ensemble chain chain0 + i."""
    LL = np.asarray(LL, dtype=np.float64)
    return levels_from_xi(LL, tf, mr.accept_uniform(LL.size, chain0, seed, step))


# ---- the inputs shared by the host test and the device test
SEED = 2012
N_RANDOM = 100000


def random_inputs():
    """(LL, tf, chains, steps): 10^5 draws, LL uniform in [-1e6, 0] in the log (|LL| from 1e-6 to 1e6) and tf log-uniform in
    [1e-3, 1e3]; chains up to 2^40, steps up to 2^32 - 1."""
    rng = np.random.default_rng(SEED)
    LL = -(10.0 ** rng.uniform(-6.0, 6.0, N_RANDOM))
    LL[::1000] = -rng.uniform(0.0, 1e6, LL[::1000].size)
    tf = 10.0 ** rng.uniform(-3.0, 3.0, N_RANDOM)
    chains = rng.integers(0, 1 << 40, N_RANDOM, dtype=np.uint64)
    steps = rng.integers(0, 1 << 32, N_RANDOM, dtype=np.uint64)
    return LL, tf, chains, steps


def edge_inputs():
    """(LL, tf, xi): the chain on -inf, NaN, +inf, -0.0 and +0.0; |LL| = 1e6 at tf = 1e-3 with xi so close to 1 that tf log(xi)
    vanishes against LL, and with ordinary xi; xi = 0 and the smallest and largest 53-bit uniforms."""
    tiny, big = 2.0 ** -53, 1.0 - 2.0 ** -53
    rows = [(-np.inf, 1.0, 0.5), (np.nan, 1.0, 0.5), (np.inf, 1.0, 0.5), (-0.0, 1.0, 0.5), (0.0, 1.0, 0.5), (-0.0, 1e-3, big),
            (-1e6, 1e-3, big), (-1e6, 1e-3, 1.0 - 2.0 ** -30), (-1e6, 1e-3, 0.5), (-1e6, 1e-3, tiny), (-1e6, 1e3, big),
            (-1e6, 1e-3, 0.999), (-123.456, 1.0, 0.0), (-123.456, 1.0, tiny), (-123.456, 1.0, big), (-1e-300, 1.0, 0.5),
            (-1e6, 1e-3, 1.0 - 2.0 ** -20), (-1e6, 1e-3, 1.0 - 2.0 ** -40)]
    a = np.array(rows)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


# the device test: counts around one block of 256 threads, and a chain index beyond 2^32
DEVICE_CASES = ((1, 0), (255, 3), (256, 0), (257, 1 << 20), (64, (1 << 32) + 5))
DEVICE_TFS = (1.0, 37.5)


def device_case(count, chain0, tf):
    """LL (count,): a few units of tf below zero, with the special values of the rule every fifth row from 1 on (row 0 plain)."""
    rng = np.random.default_rng([SEED, count, chain0 & 0xFFFF, int(tf * 2)])
    LL = -50.0 * tf * rng.random(count)
    special = (np.nan, -np.inf, -0.0, -1e6, np.inf)
    for k in range(1, count, 5):
        LL[k] = special[(k // 5) % len(special)]
    return LL
