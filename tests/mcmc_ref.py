"""Plain numpy restatement of the ensemble Metropolis sampler (trpl_mcmc_*, include/trpl.h; trpl_amd.mcmc): the proposal, the
accept/reject step with log(xi) in np.longdouble, the per-column sums of chain_stats as the sequential loop, split-R-hat and the
driver of the sweeps.  Philox and the expressions of X are refine_ref's.  No device, no library: the tests compare against this."""
import numpy as np

import refine_ref as rr

STREAM, PARTNER_CALL, ACCEPT_CALL = 0x100, 8, 9
MARGIN = 1e-12                                   # a decision with |ln xi - d| <= MARGIN max(1, |d|) is excused


def _philox(chain0, count, call, seed, step):
    """The four words of counter (n low, n high, 0x100 + call, step), n = chain0 + i, under key (seed low, seed high): (count, 4)."""
    n = np.uint64(chain0) + np.arange(count, dtype=np.uint64)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    ctr = np.stack([(n & rr.MASK).astype(np.uint32), (n >> np.uint64(32)).astype(np.uint32),
                    np.full(count, STREAM + call, dtype=np.uint32), np.full(count, step & 0xFFFFFFFF, dtype=np.uint32)], axis=-1)
    return rr.philox4x32_10(ctr, key)


def uniforms(count, A, chain0, seed, step):
    """xi (count, A): call j < 8 -> dimensions 2j, 2j + 1."""
    xi = np.empty((count, A))
    for j in range((A + 1) // 2):
        r = _philox(chain0, count, j, seed, step)
        xi[:, 2 * j] = rr.res53(r[:, 0], r[:, 1])
        if 2 * j + 1 < A:
            xi[:, 2 * j + 1] = rr.res53(r[:, 2], r[:, 3])
    return xi


def partner_indices(count, P, chain0, seed, step):
    """(a, b), each (count,) int64, b != a: a = min(int(xi_a P), P - 1), b = min(int(xi_b (P - 1)), P - 2), b += (b >= a)."""
    r = _philox(chain0, count, PARTNER_CALL, seed, step)
    xa, xb = rr.res53(r[:, 0], r[:, 1]), rr.res53(r[:, 2], r[:, 3])
    a = np.minimum((xa * float(P)).astype(np.int64), P - 1)
    b = np.minimum((xb * float(P - 1)).astype(np.int64), P - 2)
    return a, b + (b >= a)


def accept_uniform(count, chain0, seed, step):
    r = _philox(chain0, count, ACCEPT_CALL, seed, step)
    return rr.res53(r[:, 0], r[:, 1])


def propose_unit(U, partners, gamma, scale, chain0, seed, step):
    """(Up, inside): u' = (u + gamma (pa - pb)) + scale (2 xi - 1), or u + scale (2 xi - 1) without partners; one rounding per
    operation, in this order."""
    U = np.asarray(U, dtype=np.float64)
    count, A = U.shape
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (A,))
    xi = uniforms(count, A, chain0, seed, step)
    base = U
    if partners is not None and partners.shape[0] >= 2:
        a, b = partner_indices(count, partners.shape[0], chain0, seed, step)
        diff = partners[a] - partners[b]
        base = U + gamma * diff
    Up = base + scale * (2.0 * xi - 1.0)
    with np.errstate(invalid="ignore"):
        inside = np.all((Up >= 0.0) & (Up <= 1.0), axis=1).astype(np.int32)
    return Up, inside


def propose(U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, flags=0):
    """(Up, Xp, inside): Xp by the sampler's expressions from u', inside or not."""
    Up, inside = propose_unit(U, partners, gamma, scale, chain0, seed, step)
    return Up, rr.from_unit(Up, lo, hi, lg, flags), inside


def accept_decision(LL, LLp, inside, tf, chain0, seed, step):
    """(take, margin): the decision of every chain and, where the comparison log(xi) < d decided it, |ln xi - d| / max(1, |d|) in
    np.longdouble (inf elsewhere)."""
    LL, LLp = np.asarray(LL, dtype=np.float64), np.asarray(LLp, dtype=np.float64)
    xi = accept_uniform(LL.size, chain0, seed, step)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (LLp - LL) / tf
        lx = np.log(xi.astype(np.longdouble))
        dl = d.astype(np.longdouble)
        valid = (np.asarray(inside) != 0) & ~np.isnan(LLp) & (LLp > -np.inf)
        free = ~(LL > -np.inf) | (d >= 0.0)
        take = valid & (free | (lx < dl))
        compared = valid & ~free & np.isfinite(d)
        margin = np.where(compared, np.abs(lx - dl) / np.maximum(1.0, np.abs(dl)), np.inf).astype(np.float64)
    return take, margin


def accept(U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step):
    """(U, X, LL, accepted, margin) after the step: new arrays, an accepted row the proposal's bits, a rejected one untouched."""
    take, margin = accept_decision(LL, LLp, inside, tf, chain0, seed, step)
    U2, X2, LL2 = np.array(U), np.array(X), np.array(LL)
    U2[take], X2[take], LL2[take] = np.asarray(Up)[take], np.asarray(Xp)[take], np.asarray(LLp)[take]
    return U2, X2, LL2, take.astype(np.int32), margin


def chain_stats(H, t0, t1, Q=None):
    """(mean, m2), each (Q,): the sums in ascending t from +0.0, the mean one division, the squares about it."""
    H = np.asarray(H, dtype=np.float64)
    Q = H.shape[1] if Q is None else Q
    s = np.zeros(Q)
    with np.errstate(invalid="ignore"):
        for t in range(t0, t1):
            s = s + H[t, :Q]
        mean = s / float(t1 - t0)
        m2 = np.zeros(Q)
        for t in range(t0, t1):
            e = H[t, :Q] - mean
            m2 = m2 + e * e
    return mean, m2


def rhat(U, burn=0):
    """Split-R-hat (A,) of a history U (n, C, A): two halves of n2 = (n - burn) // 2 kept sweeps, 2 C sequences."""
    n, C, A = U.shape
    n2 = (n - burn) // 2
    if n2 < 2:
        raise ValueError("n2 < 2")
    H = U.reshape(n, C * A)
    parts = [chain_stats(H, burn + k * n2, burn + (k + 1) * n2) for k in (0, 1)]
    mean = np.concatenate([p[0].reshape(C, A) for p in parts])
    m2 = np.concatenate([p[1].reshape(C, A) for p in parts])
    W = np.mean(m2 / (n2 - 1), axis=0)
    B = n2 * np.var(mean, axis=0, ddof=1)
    return np.sqrt(((n2 - 1) / n2 * W + B / n2) / W)


def run(loglik, U0, LL0, lo, hi, lg, flags=0, sweeps=100, tf=1.0, kind="de", gamma=None, scale=None, jump_every=0, seed=1):
    """The sweeps of trpl_amd.mcmc.run with keep_every = 1 and burn = 0, on any loglik(X) -> LL.  Returns dict(U (sweeps, C, A),
    X, LL, accepted (sweeps, C) bool, outside, margin: the smallest margin of any decision)."""
    U, LL = np.array(U0, dtype=np.float64), np.array(LL0, dtype=np.float64)
    C, A = U.shape
    X = rr.from_unit(U, lo, hi, lg, flags)
    if scale is None:
        scale = 1e-3
    gamma0 = 2.38 / np.sqrt(2.0 * A) if gamma is None else float(gamma)
    half = C // 2
    hU, hX, hLL = np.empty((sweeps, C, A)), np.empty((sweeps, C, X.shape[1])), np.empty((sweeps, C))
    hAcc = np.empty((sweeps, C), dtype=bool)
    outside, margin = 0, np.inf
    for t in range(sweeps):
        g = 1.0 if jump_every > 0 and (t + 1) % jump_every == 0 else gamma0
        for k, (a, b) in enumerate(((0, half), (half, C))):
            partners = None if kind == "rw" else (U[half:] if k == 0 else U[:half])
            Up, Xp, inside = propose(U[a:b], partners, g, scale, a, seed, 2 * t + k, lo, hi, lg, flags)
            ok = inside != 0
            LLp = np.full(b - a, -np.inf)
            if ok.any():
                LLp[ok] = loglik(Xp[ok])
            outside += int((~ok).sum())
            U[a:b], X[a:b], LL[a:b], acc, mg = accept(U[a:b], X[a:b], LL[a:b], Up, Xp, LLp, inside, tf, a, seed, 2 * t + k)
            hAcc[t, a:b] = acc != 0
            margin = min(margin, float(mg.min()))
        hU[t], hX[t], hLL[t] = U, X, LL
    return dict(U=hU, X=hX, LL=hLL, accepted=hAcc, outside=outside / float(sweeps * C), margin=margin)


# ---- the toys of the host and the device tests: 3-D Gaussians of deviation 0.08 centred in the cube, on the box [0, 1]^3 (X = U)
TOY_SD, TOY_A, TOY_RHO = 0.08, 3, 0.99
CUBE = (np.zeros(TOY_A), np.ones(TOY_A), np.zeros(TOY_A, dtype=np.int32))


def toy(rho=0.0):
    """(loglik on unit coordinates, covariance): rho = 0 the isotropic toy, else every pair of coordinates correlated by rho."""
    cov = TOY_SD ** 2 * ((1.0 - rho) * np.eye(TOY_A) + rho * np.ones((TOY_A, TOY_A)))
    prec = np.linalg.inv(cov)

    def loglik(U):
        e = np.asarray(U)[:, :TOY_A] - 0.5
        return -0.5 * np.einsum("si,ij,sj->s", e, prec, e)

    return loglik, cov


def toy_start(C, seed):
    """Over-dispersed starts: uniform in the cube."""
    return np.random.default_rng([seed, C]).random((C, TOY_A))


# ---- inputs shared by the host and the device tests of the accept step and of the end-to-end run
ACCEPT_COUNTS, ACCEPT_TFS, ACCEPT_SEED = (1, 257, 4096), (1.0, 37.5), 5


def accept_case(count, tf, A=3, ncol=5):
    """(U, X, LL, Up, Xp, LLp, inside) with every branch of the rule among the rows (count permitting): the chain on NaN and on
    -inf, LLp NaN, -inf and +inf, a proposal outside with a large LLp, d of exactly 0; everywhere else d of a few units either way."""
    rng = np.random.default_rng([ACCEPT_SEED, count, int(tf * 2)])
    U, Up = rng.random((count, A)), rng.random((count, A))
    X, Xp = rng.normal(size=(count, ncol)), rng.normal(size=(count, ncol))
    LL = -5.0 * rng.random(count) * tf
    LLp = LL + 3.0 * tf * rng.normal(size=count)
    inside = np.ones(count, dtype=np.int32)
    special = [("LL", np.nan), ("LL", -np.inf), ("LLp", np.nan), ("LLp", -np.inf), ("LLp", np.inf), ("out", 1e9), ("same", 0.0),
               ("LL", np.inf), ("both", -np.inf), ("both", np.nan), ("out", -1.0)]
    for k in range(1, count, 3):                                 # every third row from 1 on, the kinds in turn; row 0 stays plain
        kind, v = special[(k // 3) % len(special)]
        if kind == "LL":
            LL[k] = v
        elif kind == "LLp":
            LLp[k] = v
        elif kind == "both":
            LL[k] = LLp[k] = v
        elif kind == "same":
            LLp[k] = LL[k]
        else:
            inside[k] = 0
            LLp[k] = v
    return U, X, LL, Up, Xp, LLp, inside


# the end-to-end run of the device test: the isotropic toy on the box of tests/test_gpu_refine.py.  The seed is one whose smallest
# decision margin in the restatement is above E2E_MARGIN (tests/test_mcmc_host.py asserts it): the device's likelihoods differ
# from the restatement's by the distance of the device's pow to numpy's in the log column, 4 ulp of x, which moves LL by at most
# |u - 1/2| / sd^2 * 4 * 2^-52 * ln(10) * 4 decades < 3e-12 -- far inside 1e-9, so no decision can differ.
E2E = dict(C=256, sweeps=60, seed=3)
E2E_MARGIN = 1e-9
E2E_LO, E2E_HI, E2E_LG = np.array([2.0, 1e-3, -1.0]), np.array([5.0, 1e1, 1.0]), np.array([0, 1, 0], dtype=np.int32)


def e2e_loglik(X):
    return toy(0.0)[0](rr.unit_coords(np.asarray(X), E2E_LO, E2E_HI, E2E_LG)[0])


def e2e_reference():
    """(U0, X0, LL0, run): the start and the restatement's run of the end-to-end case."""
    U0 = toy_start(E2E["C"], E2E["seed"])
    X0 = rr.from_unit(U0, E2E_LO, E2E_HI, E2E_LG)
    LL0 = e2e_loglik(X0)
    return U0, X0, LL0, run(e2e_loglik, U0, LL0, E2E_LO, E2E_HI, E2E_LG, sweeps=E2E["sweeps"], seed=E2E["seed"])
