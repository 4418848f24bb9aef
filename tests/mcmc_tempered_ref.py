"""Plain numpy restatement of parallel tempering (trpl_mcmc_swap, trpl_amd.mcmc.run_tempered; include/trpl.h):
the exchange between adjacent rungs with log(xi) in np.longdouble and the margin of every decision recorded as
mcmc_ref.accept_decision records it, and the driver of the tempered sweeps built from mcmc_ref's propose and accept, one rung at a
time -- which is what the *_rungs calls are, slice by slice.  No device, no library: the tests compare against this."""
import numpy as np

import mcmc_ref as mr

SWAP_CALL = 10


def geometric_ladder(tf, tf_hot, K):
    if K == 1:
        return np.array([float(tf)])
    out = tf * (tf_hot / tf) ** (np.arange(K) / float(K - 1))
    out[0], out[-1] = tf, tf_hot
    return out


def swap_pairs(K, group, parity):
    """(a, b, k), each (pairs,): the lower row, the upper row and the lower rung of every pair, k = parity, parity + 2, .. < K - 1."""
    lower = np.arange(parity, K - 1, 2)
    a = (lower[:, None] * group + np.arange(group)[None, :]).ravel().astype(np.int64)
    return a, a + group, np.repeat(lower, group)


def swap_d(LLa, LLb, tfa, tfb):
    """d = (LL[b] - LL[a]) * (1 / tf[k] - 1 / tf[k + 1]), one rounding per operation."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (np.asarray(LLb, dtype=np.float64) - np.asarray(LLa, dtype=np.float64)) * (1.0 / np.asarray(tfa, dtype=np.float64)
                                                                                         - 1.0 / np.asarray(tfb, dtype=np.float64))


def swap_probability(LLa, LLb, tfa, tfb):
    """min(1, exp(d)): the probability with which the rule exchanges a pair of finite likelihoods."""
    return np.minimum(1.0, np.exp(swap_d(LLa, LLb, tfa, tfb)))


def swap_decision(LL, K, group, tf, parity, chain0, seed, step):
    """(a, b, take, margin): the pairs, the decision of each and, where log(xi) < d decided it, |ln xi - d| / max(1, |d|) in
    np.longdouble (inf elsewhere)."""
    LL, tf = np.asarray(LL, dtype=np.float64), np.asarray(tf, dtype=np.float64)
    a, b, k = swap_pairs(K, group, parity)
    r = mr._philox(chain0, K * group, SWAP_CALL, seed, step)
    xi = mr.rr.res53(r[:, 0], r[:, 1])[a]
    la, lb = LL[a], LL[b]
    d = swap_d(la, lb, tf[k], tf[np.minimum(k + 1, K - 1)])
    with np.errstate(invalid="ignore", divide="ignore"):
        lx = np.log(xi.astype(np.longdouble))
        dl = d.astype(np.longdouble)
        valid = ~np.isnan(la) & ~np.isnan(lb)
        free = d >= 0.0
        take = valid & (free | (lx < dl))
        compared = valid & ~free & np.isfinite(d)
        margin = np.where(compared, np.abs(lx - dl) / np.maximum(1.0, np.abs(dl)), np.inf).astype(np.float64)
    return a, b, take, margin


def swap(U, X, LL, K, group, tf, parity, chain0, seed, step):
    """(U, X, LL, swapped, margin) after the exchange: new arrays; margin (K group,) is the pair's on both of its rows, inf on an
    unpaired row."""
    a, b, take, mg = swap_decision(LL, K, group, tf, parity, chain0, seed, step)
    U2, X2, LL2 = np.array(U), np.array(X), np.array(LL)
    swapped, margin = np.zeros(K * group, dtype=np.int32), np.full(K * group, np.inf)
    ta, tb = a[take], b[take]
    U2[ta], U2[tb] = np.asarray(U)[tb], np.asarray(U)[ta]
    X2[ta], X2[tb] = np.asarray(X)[tb], np.asarray(X)[ta]
    LL2[ta], LL2[tb] = np.asarray(LL)[tb], np.asarray(LL)[ta]
    swapped[ta] = swapped[tb] = 1
    margin[a] = margin[b] = mg
    return U2, X2, LL2, swapped, margin


def run_tempered(loglik, U0, LL0, lo, hi, lg, ladder, flags=0, sweeps=100, swap_every=1, kind="de", gamma=None, scale=None, jump_every=0,
                 seed=1):
    """The sweeps of trpl_amd.mcmc.run_tempered with keep_every = 1 and burn = 0.  U0 (C, A) and LL0 (C,) for every rung, or (K, C, A)
    and (K, C).  Returns dict(U (K, sweeps, C, A), X, LL, accepted (K, sweeps, C) bool, outside (K,), swap_rate (K - 1,), swaps: the
    number of swap steps, margin: the smallest margin of any decision, accept or exchange)."""
    ladder = np.asarray(ladder, dtype=np.float64)
    K = ladder.size
    U, LL = np.array(U0, dtype=np.float64), np.array(LL0, dtype=np.float64)
    if U.ndim == 2:
        U, LL = np.broadcast_to(U, (K,) + U.shape), np.broadcast_to(LL, (K,) + LL.shape)
    C, A = U.shape[1:]
    g = C // 2
    half = K * g
    U = np.array(U.reshape(K, 2, g, A).swapaxes(0, 1).reshape(2 * half, A), order="C")        # half-major, a copy of its own
    LL = np.array(LL.reshape(K, 2, g).swapaxes(0, 1).reshape(2 * half), order="C")
    X = mr.rr.from_unit(U, lo, hi, lg, flags)
    if scale is None:
        scale = 1e-3
    gamma0 = 2.38 / np.sqrt(2.0 * A) if gamma is None else float(gamma)

    def rung_major(a):
        return a.reshape((2, K, g) + a.shape[1:]).swapaxes(0, 1).reshape((K, C) + a.shape[1:])

    hU, hX, hLL = np.empty((K, sweeps, C, A)), np.empty((K, sweeps, C, X.shape[1])), np.empty((K, sweeps, C))
    hAcc = np.empty((K, sweeps, C), dtype=bool)
    outside, margin, swaps = np.zeros(K, dtype=np.int64), np.inf, 0
    tried, done = np.zeros(max(K - 1, 0), dtype=np.int64), np.zeros(max(K - 1, 0), dtype=np.int64)
    moved = np.empty(2 * half, dtype=bool)
    for t in range(sweeps):
        gm = 1.0 if jump_every > 0 and (t + 1) % jump_every == 0 else gamma0
        for h, (a, b) in enumerate(((0, half), (half, 2 * half))):
            other = U[half:] if h == 0 else U[:half]
            Up, Xp, inside = np.empty((half, A)), np.empty((half, X.shape[1])), np.empty(half, dtype=np.int32)
            for k in range(K):                                   # the slice identity: rung k is the plain call on its rows
                s = slice(k * g, (k + 1) * g)
                partners = None if kind == "rw" else other[s]
                Up[s], Xp[s], inside[s] = mr.propose(U[a:b][s], partners, gm, scale, a + k * g, seed, 2 * t + h, lo, hi, lg, flags)
            ok = inside != 0
            LLp = np.full(half, -np.inf)
            if ok.any():
                LLp[ok] = loglik(Xp[ok])                         # one call for all rungs
            outside += np.bincount(np.repeat(np.arange(K), g)[~ok], minlength=K)
            for k in range(K):
                s = slice(a + k * g, a + (k + 1) * g)
                r = slice(k * g, (k + 1) * g)
                U[s], X[s], LL[s], acc, mg = mr.accept(U[s], X[s], LL[s], Up[r], Xp[r], LLp[r], inside[r], ladder[k], a + k * g, seed,
                                                       2 * t + h)
                moved[s] = acc != 0
                margin = min(margin, float(mg.min()))
        if K > 1 and (t + 1) % swap_every == 0:
            parity = (t // swap_every) % 2
            swaps += 1
            for a, b in ((0, half), (half, 2 * half)):
                U[a:b], X[a:b], LL[a:b], sw, mg = swap(U[a:b], X[a:b], LL[a:b], K, g, ladder, parity, a, seed, t)
                lower = np.arange(parity, K - 1, 2)
                tried[lower] += g
                done[lower] += sw.reshape(K, g)[lower].sum(axis=1)
                margin = min(margin, float(mg.min()))
        hU[:, t], hX[:, t], hLL[:, t], hAcc[:, t] = rung_major(U), rung_major(X), rung_major(LL), rung_major(moved)
    with np.errstate(invalid="ignore"):
        rate = done / tried.astype(np.float64)
    return dict(U=hU, X=hX, LL=hLL, accepted=hAcc, outside=outside / float(sweeps * C), swap_rate=rate, swaps=swaps, margin=margin)


# ---- inputs shared by the host and the device tests of the swap
SWAP_KS, SWAP_GROUPS, SWAP_SEED = (2, 3, 4, 7), (1, 5, 257), 11


def swap_ladder(K):
    """Distinct unsorted temperatures; with K >= 3 the first two are equal (d = 0 * something: every finite pair exchanges, an
    infinite difference gives a NaN d and exchanges nothing)."""
    tf = np.array([1.0, 3.0, 2.0, 17.5, 6.0, 40.0, 9.0])[:K].copy()
    if K >= 3:
        tf[1] = tf[0]
    return tf


def swap_case(K, group, A, ncol):
    """(U, X, LL): K group rows with every branch among them (group permitting): -inf in the lower row, in the upper row, in both,
    NaN, equal values, +inf; everywhere else differences of a few units."""
    rng = np.random.default_rng([SWAP_SEED, K, group, A, ncol])
    n = K * group
    U, X = rng.random((n, A)), rng.normal(size=(n, ncol))
    LL = -10.0 * rng.random(n)
    special = (-np.inf, np.nan, "same", -np.inf, np.inf, "both")
    for j, c in enumerate(range(1, group, 2)):                   # every second column of the block from 1 on, the kinds in turn
        kind = special[j % len(special)]
        for k in range(K):
            row = k * group + c
            if kind == "same":
                LL[row] = LL[c]
            elif kind == "both":
                LL[row] = -np.inf
            elif (j // len(special) + k) % 2 == 0:               # alternate rungs: the special value sits in the lower or the upper row
                LL[row] = kind
    return U, X, LL


def swap_cases(K):
    """(group, parity, A, ncol, chain0, step) of every case of the device test at K rungs."""
    return [(group, parity, A, ncol, (1 << 32) + 5 if parity else 0, 3 + parity)
            for group in SWAP_GROUPS for parity in (0, 1) for A in (1, 16) for ncol in (1, 13)]


# ---- the end-to-end run of the device test: mcmc_ref's isotropic toy on its box, three rungs
E2E = dict(C=16, sweeps=10, seed=4, ladder=(1.0, 4.0, 16.0))


def e2e_reference(swap_every):
    U0 = mr.toy_start(E2E["C"], E2E["seed"])
    X0 = mr.rr.from_unit(U0, mr.E2E_LO, mr.E2E_HI, mr.E2E_LG)
    LL0 = mr.e2e_loglik(X0)
    return U0, X0, LL0, run_tempered(mr.e2e_loglik, U0, LL0, mr.E2E_LO, mr.E2E_HI, mr.E2E_LG, E2E["ladder"], sweeps=E2E["sweeps"],
                                     swap_every=swap_every, seed=E2E["seed"])


# ---- the bimodal toy: an equal mixture of two Gaussians of deviation 0.03 at (1/4, 1/4) and (3/4, 3/4) of the unit square.  Every
# chain starts in the first mode; the second is 16 deviations away along each axis.
BI_SD, BI_C, BI_SWEEPS, BI_BURN, BI_K, BI_HOT = 0.03, 64, 300, 100, 7, 64.0
BI_BOX = (np.zeros(2), np.ones(2), np.zeros(2, dtype=np.int32))
BI_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
BI_DEVICE_SEED = 1
# The cold rung's share of the second mode over the sweeps from BI_BURN on, by run_tempered of this file with
# geometric_ladder(1, BI_HOT, BI_K), for the seeds of BI_SEEDS in turn (tests/test_mcmc_tempered_host.py recomputes them).  The gate
# of the device test is 5 standard deviations (numpy.std, the narrower ddof = 0) of these about the analytic 1/2.
BI_SHARES = (0.510546875, 0.520546875, 0.506796875, 0.515546875, 0.5125, 0.4984375, 0.506171875, 0.505546875)
BI_MARGIN = 5.0 * float(np.std(BI_SHARES))                       # 0.0319


def bimodal_loglik(X):
    X = np.asarray(X)[:, :2]
    r1 = np.sum((X - 0.25) ** 2, axis=1)
    r2 = np.sum((X - 0.75) ** 2, axis=1)
    return np.logaddexp(-0.5 * r1 / BI_SD ** 2, -0.5 * r2 / BI_SD ** 2)


def bimodal_start(seed):
    U0 = 0.25 + BI_SD * np.random.default_rng([seed, 77]).normal(size=(BI_C, 2))
    return U0, bimodal_loglik(U0)


def second_mode_share(U):
    """The share of the states U (..., 2) that lie nearer the second mode: u0 + u1 > 1."""
    return float(np.mean(U[..., 0] + U[..., 1] > 1.0))
