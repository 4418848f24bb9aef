"""Plain numpy restatement of the Metropolis-Hastings half of the ensemble sampler (trpl_mcmc_propose_stretch, trpl_mcmc_accept_h,
trpl_mcmc_levels_h, trpl_mcmc_prior_term, include/trpl.h; csrc/mcmc_hastings.hip) and of a sweep loop that uses
them, in the style of mcmc_ref.py and mcmc_levels_ref.py: one rounding per operation, in the kernels' order.  The accept predicate and
the level rule take log(xi) as an argument, so they hold for any rounding of the logarithm (the device's library and numpy's differ
in the last bit for a few per cent of the uniforms).  Philox is mcmc_ref's (refine_ref's).  No device, no library."""
import numpy as np

import mcmc_levels_ref as lr
import mcmc_ref as mr
import mcmc_tempered_ref as tr
import refine_ref as rr

STRETCH_CALL = 11


def rung_tf(tf, count):
    """tf per row (count,): a scalar, or a ladder (K,) over K rungs of count / K rows."""
    tf = np.atleast_1d(np.asarray(tf, dtype=np.float64))
    assert count % tf.size == 0
    return np.repeat(tf, count // tf.size)


# ------------------------------------------------------------------ stretch
def stretch_uniforms(count, chain0, seed, step):
    """(xa, xi): the first uniform of the partner call and the first uniform of the stretch call."""
    ra, rs = mr._philox(chain0, count, mr.PARTNER_CALL, seed, step), mr._philox(chain0, count, STRETCH_CALL, seed, step)
    return rr.res53(ra[:, 0], ra[:, 1]), rr.res53(rs[:, 0], rs[:, 1])


def stretch_unit(U, partners, group, a, chain0, seed, step):
    """(Up, inside, z, row): s = (a - 1) xi + 1, z = s s / a, u' = p + z (u - p) with p the row (i // group) group + min(int(xa group),
    group - 1) of partners."""
    U, partners = np.asarray(U, dtype=np.float64), np.asarray(partners, dtype=np.float64)
    count = U.shape[0]
    group = partners.shape[0] if group is None else int(group)
    xa, xi = stretch_uniforms(count, chain0, seed, step)
    row = (np.arange(count) // group) * group + np.minimum((xa * float(group)).astype(np.int64), group - 1)
    s = (a - 1.0) * xi + 1.0
    z = s * s / a
    p = partners[row]
    Up = p + z[:, None] * (U - p)
    with np.errstate(invalid="ignore"):
        inside = np.all((Up >= 0.0) & (Up <= 1.0), axis=1).astype(np.int32)
    return Up, inside, z, row


def stretch(U, partners, group, a, chain0, seed, step, lo, hi, lg, flags=0):
    """(Up, Xp, inside, z, lnq): lnq = (A - 1) log(z) with numpy's log."""
    Up, inside, z, _ = stretch_unit(U, partners, group, a, chain0, seed, step)
    return Up, rr.from_unit(Up, lo, hi, lg, flags), inside, z, float(Up.shape[1] - 1) * np.log(z)


# ------------------------------------------------------------------ accept with h
def accept_take_h(LL, LLp, tf, h, lx, inside=1):
    """The accept kernel's decision, its own expression, with log(xi) = lx given: inside, LLp and h neither NaN nor -inf, and the
    chain not above -inf, or d = (LLp - LL) / tf + h >= 0, or lx < d."""
    LL, LLp, tf, h, lx = (np.asarray(v, dtype=np.float64) for v in (LL, LLp, tf, h, lx))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = (LLp - LL) / tf + h
        return ((np.asarray(inside) != 0) & ~np.isnan(LLp) & (LLp > -np.inf) & ~np.isnan(h) & (h > -np.inf)
                & (~(LL > -np.inf) | (d >= 0.0) | (lx < d)))


def accept_h(U, X, LL, Up, Xp, LLp, inside, h, tf, chain0, seed, step, lx=None):
    """(U, X, LL, accepted) after the step: new arrays.  tf a scalar or a ladder (K,); lx: log(xi) per row, default numpy's."""
    count = np.asarray(LL).size
    if lx is None:
        with np.errstate(divide="ignore"):
            lx = np.log(mr.accept_uniform(count, chain0, seed, step))
    take = accept_take_h(LL, LLp, rung_tf(tf, count), h, lx, inside)
    U2, X2, LL2 = np.array(U), np.array(X), np.array(LL)
    U2[take], X2[take], LL2[take] = np.asarray(Up)[take], np.asarray(Xp)[take], np.asarray(LLp)[take]
    return U2, X2, LL2, take.astype(np.int32)


# ------------------------------------------------------------------ levels with h
def _verified_h(l, LL, tf, h, lx):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dq = (-l - LL) / tf + h
        return (dq < 0.0) & ~(lx < dq)


def levels_h_from_log(LL, tf, xi, lx, h):
    """level per element: l0 = -(LL + tf (lx - h)), else l0 + (|LL| + l0) 2^-40, whichever the accept step's own dq = (-l - LL) / tf + h
    verifies first; +inf when LL is NaN or not above -inf, when xi == 0, when h is NaN or infinite, or when neither is verified."""
    LL, tf, xi, lx, h = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (LL, tf, xi, lx, h)))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l0 = -(LL + tf * (lx - h))
        l1 = l0 + (np.abs(LL) + l0) * 2.0 ** -40
        usable = ~np.isnan(LL) & (LL > -np.inf) & (xi != 0.0) & np.isfinite(h)
        ok0, ok1 = _verified_h(l0, LL, tf, h, lx), _verified_h(l1, LL, tf, h, lx)
    return np.where(usable & ok0, l0, np.where(usable & ok1, l1, np.inf))


def levels_h(LL, h, tf, chain0, seed, step, lx=None):
    """trpl_mcmc_levels_h: tf a scalar or a ladder (K,)."""
    LL = np.asarray(LL, dtype=np.float64)
    xi = mr.accept_uniform(LL.size, chain0, seed, step)
    if lx is None:
        with np.errstate(divide="ignore"):
            lx = np.log(xi)
    return levels_h_from_log(LL, rung_tf(tf, LL.size), xi, lx, h)


# ------------------------------------------------------------------ the prior term
def log_prior(U, mean, sd):
    """lnp (count,): the sum over d ascending from +0.0 of (-0.5 t) t, t = (u_d - mean_d) / sd_d; sd_d = inf adds exactly +0.0."""
    U, mean, sd = np.asarray(U, dtype=np.float64), np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    s = np.zeros(U.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(U.shape[1]):
            t = (U[:, d] - mean[d]) / sd[d]
            s = s + (0.0 if np.isposinf(sd[d]) else (-0.5 * t) * t)
    return s


def prior_term(U, Up, mean, sd, h=None):
    """h_out = h + (lnp(Up) - lnp(U)); h None is +0.0."""
    h = np.zeros(np.asarray(U).shape[0]) if h is None else np.asarray(h, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return h + (log_prior(Up, mean, sd) - log_prior(U, mean, sd))


# ------------------------------------------------------------------ the sweeps
def run(loglik, U0, LL0, lo, hi, lg, flags=0, sweeps=100, tf=1.0, ladder=None, kind="stretch", stretch_a=2.0, prior=None, gamma=None,
        scale=None, seed=1, swap_every=1, use_lnq=True, levels_check=False):
    """The sweeps of trpl_amd.mcmc.run (ladder None: U0 (C, A), LL0 (C,)) and run_tempered (ladder (K,): U0 (C, A) or (K, C, A)) with
    kind="stretch" or a prior, keep_every = 1 and burn = 0, numpy's log throughout.  kind "stretch" or "de".  use_lnq=False drops the
    Hastings term of the stretch move -- the wrong sampler the gates must be able to tell from the right one.  levels_check: also
    form every half-sweep's levels_h and assert that no accepted proposal had LLp <= -level.
    Returns dict(U (K, sweeps, C, A), X, LL, accepted (K, sweeps, C) bool, outside (K,)); K = 1 for ladder None."""
    lad = np.array([float(tf)]) if ladder is None else np.asarray(ladder, dtype=np.float64)
    K = lad.size
    U, LL = np.array(U0, dtype=np.float64), np.array(LL0, dtype=np.float64)
    if U.ndim == 2:
        U, LL = np.broadcast_to(U, (K,) + U.shape), np.broadcast_to(LL, (K,) + LL.shape)
    C, A = U.shape[1:]
    g = C // 2
    half = K * g
    U = np.array(U.reshape(K, 2, g, A).swapaxes(0, 1).reshape(2 * half, A), order="C")
    LL = np.array(LL.reshape(K, 2, g).swapaxes(0, 1).reshape(2 * half), order="C")
    X = rr.from_unit(U, lo, hi, lg, flags)
    scale = 1e-3 if scale is None else scale
    gamma0 = 2.38 / np.sqrt(2.0 * A) if gamma is None else float(gamma)

    def rung_major(a):
        return a.reshape((2, K, g) + a.shape[1:]).swapaxes(0, 1).reshape((K, C) + a.shape[1:])

    hU, hX, hLL = np.empty((K, sweeps, C, A)), np.empty((K, sweeps, C, X.shape[1])), np.empty((K, sweeps, C))
    hAcc = np.empty((K, sweeps, C), dtype=bool)
    outside, moved = np.zeros(K, dtype=np.int64), np.empty(2 * half, dtype=bool)
    for t in range(sweeps):
        for hs, (a, b) in enumerate(((0, half), (half, 2 * half))):
            step = 2 * t + hs
            other = U[half:] if hs == 0 else U[:half]
            if kind == "stretch":
                Up, Xp, inside, _, h = stretch(U[a:b], other, g, stretch_a, a, seed, step, lo, hi, lg, flags)
                if not use_lnq:
                    h = np.zeros(half)
            else:
                Up, Xp, inside = np.empty((half, A)), np.empty((half, X.shape[1])), np.empty(half, dtype=np.int32)
                for k in range(K):
                    s = slice(k * g, (k + 1) * g)
                    Up[s], Xp[s], inside[s] = mr.propose(U[a:b][s], other[s], gamma0, scale, a + k * g, seed, step, lo, hi, lg, flags)
                h = np.zeros(half)
            if prior is not None:
                h = prior_term(U[a:b], Up, prior[0], prior[1], h)
            ok = (inside != 0) & ~np.isnan(h) & (h > -np.inf)
            LLp = np.full(half, -np.inf)
            if ok.any():
                LLp[ok] = loglik(Xp[ok])
            outside += np.bincount(np.repeat(np.arange(K), g)[~ok], minlength=K)
            if levels_check:
                level = levels_h(LL[a:b], h, lad, a, seed, step)
            U[a:b], X[a:b], LL[a:b], acc = accept_h(U[a:b], X[a:b], LL[a:b], Up, Xp, LLp, inside, h, lad, a, seed, step)
            if levels_check:
                assert not (acc != 0)[LLp <= -level].any()
            moved[a:b] = acc != 0
        if K > 1 and (t + 1) % swap_every == 0:
            parity = (t // swap_every) % 2
            for a, b in ((0, half), (half, 2 * half)):
                U[a:b], X[a:b], LL[a:b], _, _ = tr.swap(U[a:b], X[a:b], LL[a:b], K, g, lad, parity, a, seed, t)
        hU[:, t], hX[:, t], hLL[:, t], hAcc[:, t] = rung_major(U), rung_major(X), rung_major(LL), rung_major(moved)
    return dict(U=hU, X=hX, LL=hLL, accepted=hAcc, outside=outside / float(sweeps * C))


# ------------------------------------------------------------------ inputs shared by the host and the device tests
H_VALUES = (0.0, 1e-3, -1e-3, 5.0, -5.0, 700.0, -700.0)          # crossed with mcmc_levels_ref's random and edge sets
H_EDGES = (np.nan, -np.inf, np.inf, -0.0)

# the shapes of the device test: (count, A, K, group, chain0); count = K group.  Counts around one block of 256 threads, the
# smallest and the largest A, rungs of 100 and 200 rows so that blocks straddle rungs, one chain index above 2^32.
DEVICE_SHAPES = ((1, 1, 1, 1, 0), (255, 2, 1, 255, 3), (256, 3, 1, 256, 0), (257, 10, 1, 257, 1 << 20), (600, 16, 3, 200, (1 << 32) + 5),
                 (300, 3, 3, 100, 7), (600, 2, 1, 600, 0))
DEVICE_LADDER = np.array([1.0, 37.5, 4.0])
DEVICE_SEED = 2010


def device_box(A):
    """(lo, hi, lg): A active columns, alternately linear and log, and -- where 16 columns leave room -- one fixed column in front of
    the last."""
    lo, hi, lg = [], [], []
    for d in range(A):
        if d == A - 1 and A < 16:
            lo.append(1.5), hi.append(1.5), lg.append(0)          # the fixed column
        if d % 2:
            lo.append(1e-3), hi.append(1e1), lg.append(1)
        else:
            lo.append(-1.0), hi.append(3.0), lg.append(0)
    return np.array(lo), np.array(hi), np.array(lg, dtype=np.int32)


def device_case(count, A, K, chain0):
    """(U, partners, X, LL, Up, Xp, LLp, inside, h): states in the middle of the cube, the accept case of mcmc_ref (every branch of the
    rule among the rows; X of min(A + 1, 16) columns) and an h of a few units with the edge values every seventh row from 2 on."""
    rng = np.random.default_rng([DEVICE_SEED, count, A, K, chain0 & 0xFFFF])
    U, partners = rng.uniform(0.2, 0.8, (count, A)), rng.uniform(0.2, 0.8, (count, A))
    _, X, LL, Up, Xp, LLp, inside = mr.accept_case(count, 1.0, A=A, ncol=min(A + 1, 16))
    h = 2.0 * rng.normal(size=count)
    h[rng.random(count) < 0.2] = 0.0
    for k in range(2, count, 7):
        h[k] = H_EDGES[(k // 7) % len(H_EDGES)]
    return U, partners, X, LL, Up, Xp, LLp, inside, h


# ---- the stretch toy of the device test: mcmc_ref's 3-D Gaussian with correlation 0.99 (deviation 0.08, centred in the cube),
# 256 chains x 400 sweeps from over-dispersed starts, the second half kept.  The figures below are this file's run() for the seeds
# STRETCH_SEEDS in turn (tests/test_mcmc_hastings_host.py recomputes the first of them): per seed the mean over the three
# coordinates of the kept states' mean, of their deviation, and of the three pairwise correlations.  The device test's gate for each
# is the mean of the eight +- 5 of their standard deviations (numpy.std, ddof = 0, the narrower).
STRETCH_TOY = dict(C=256, sweeps=400, rho=mr.TOY_RHO)
STRETCH_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
STRETCH_DEVICE_SEED = 1
STRETCH_STATS = ((0.5002040511463842, 0.07980529777824434, 0.9898955617344417), (0.49799338957972034, 0.08014301872097916, 0.9901589075224759),
                 (0.5014284247658405, 0.07935337657513906, 0.9897938669496776), (0.5020734425079327, 0.08187481925293745, 0.9906588341935718),
                 (0.5005305576524823, 0.07974571572649777, 0.9901390879521164), (0.5020251645320629, 0.07990778077625238, 0.9898662358734193),
                 (0.49456788327311785, 0.07945551147061364, 0.9897358650985999), (0.49882826864996466, 0.08097257203257298, 0.9903329401487321))


def stretch_gates():
    """(lo, hi), each (3,): mean - 5 sd and mean + 5 sd of STRETCH_STATS -- mean in (0.4879, 0.5116), deviation in (0.0762, 0.0842),
    correlation in (0.98861, 0.99154); the analytic 0.5, 0.08 and 0.99 lie inside."""
    a = np.array(STRETCH_STATS)
    return a.mean(axis=0) - 5.0 * a.std(axis=0), a.mean(axis=0) + 5.0 * a.std(axis=0)


def toy_stats(U):
    """(mean, deviation, correlation) of kept states U (n, C, 3): each averaged over the coordinates (the pairs)."""
    S = U.reshape(-1, U.shape[-1])
    c = np.corrcoef(S.T)
    return float(S.mean()), float(S.std(axis=0).mean()), float(c[np.triu_indices(S.shape[1], 1)].mean())


def stretch_toy_run(seed, use_lnq=True, sweeps=None, C=None):
    loglik, _ = mr.toy(STRETCH_TOY["rho"])
    C = STRETCH_TOY["C"] if C is None else C
    sweeps = STRETCH_TOY["sweeps"] if sweeps is None else sweeps
    U0 = mr.toy_start(C, seed)
    res = run(loglik, U0, loglik(U0), *mr.CUBE, sweeps=sweeps, seed=seed, use_lnq=use_lnq)
    return res["U"][0, sweeps // 2:]


# ---- the prior toy: a flat likelihood on the unit square, the prior N(0, 0.2^2) on the first coordinate (centred on the face u = 0)
# and flat on the second.  The posterior of u_0 is the half-Gaussian on [0, 1] (the cut at 1 = 5 sd removes 6e-7 of the mass, far
# below the gates): E u = sd sqrt(2 / pi), E u^2 = sd^2.
PRIOR_SD = 0.2
PRIOR_TOY = dict(C=256, sweeps=400, seed=3)
PRIOR = (np.array([0.0, 0.5]), np.array([PRIOR_SD, np.inf]))
PRIOR_BOX = (np.zeros(2), np.ones(2), np.zeros(2, dtype=np.int32))
PRIOR_M1, PRIOR_M2 = PRIOR_SD * np.sqrt(2.0 / np.pi), PRIOR_SD ** 2


PRIOR_BATCHES = 10


def prior_gate(series, truth):
    """(error, 5 standard errors) of the mean of a per-sweep series of ensemble means: the standard error by batch means, the kept
    200 sweeps in 10 batches of 20 -- differential evolution at gamma = 2.38 / sqrt(2 A) forgets a 2-D state within a few sweeps, so
    the batch means are nearly independent -- as their spread (ddof = 1) over sqrt(10)."""
    b = np.asarray(series).reshape(PRIOR_BATCHES, -1).mean(axis=1)
    return abs(float(np.mean(series)) - truth), 5.0 * float(b.std(ddof=1)) / np.sqrt(PRIOR_BATCHES)


def flat_loglik(X, cut_levels=None):
    return np.zeros(len(X))
