"""Plain numpy restatement of TRPL_MCMC_FOLD (include/trpl.h; trpl_amd.mcmc.run(bounds="fold")): the fold of one coordinate, the
proposal with the codes of `inside`, and the driver of the sweeps with either boundary rule.  Everything else -- Philox, the
unfolded proposal, the accept step, split-R-hat -- is tests/mcmc_ref.py's, the expressions of X tests/refine_ref.py's.  No device,
no library: the tests compare against this."""
import numpy as np

import mcmc_ref as mr
import refine_ref as rr


def fold(v):
    """v in [0, 1]: the same bits.  Otherwise r = fmod(v, 2); r < 0: r + 2; r > 1: 2 - r.  NaN and +-inf give NaN."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        keep = (v >= 0.0) & (v <= 1.0)
        r = np.fmod(v, 2.0)
        r = np.where(r < 0.0, r + 2.0, r)
        r = np.where(r > 1.0, 2.0 - r, r)
    return np.where(keep, v, r)


def propose(U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, flags=0, fold=False, rule=None):
    """(Up, Xp, inside).  fold=False: mcmc_ref.propose.  fold=True: every coordinate of the unfolded u' goes through `rule`
    (default: fold), Xp is formed from the result, and inside is the code 0 (a coordinate is not finite) / 1 (the rule changed
    nothing: every coordinate was in [0, 1]) / 2 (at least one coordinate was outside [0, 1])."""
    if not fold:
        return mr.propose(U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, flags)
    raw, _ = mr.propose_unit(U, partners, gamma, scale, chain0, seed, step)
    Up = (globals()["fold"] if rule is None else rule)(raw)
    with np.errstate(invalid="ignore"):
        out = ~((raw >= 0.0) & (raw <= 1.0))
    code = np.where(np.isnan(Up).any(axis=1), 0, np.where(out.any(axis=1), 2, 1)).astype(np.int32)
    return Up, rr.from_unit(Up, lo, hi, lg, flags), code


def run(loglik, U0, LL0, lo, hi, lg, flags=0, sweeps=100, tf=1.0, kind="de", gamma=None, scale=None, jump_every=0, seed=1,
        bounds="reject", rule=None):
    """mcmc_ref.run with the boundary rule: the same dict, and folded, the share of all proposals with code 2."""
    if bounds not in ("reject", "fold"):
        raise ValueError("bounds")
    U, LL = np.array(U0, dtype=np.float64), np.array(LL0, dtype=np.float64)
    C, A = U.shape
    X = rr.from_unit(U, lo, hi, lg, flags)
    if scale is None:
        scale = 1e-3
    gamma0 = 2.38 / np.sqrt(2.0 * A) if gamma is None else float(gamma)
    half = C // 2
    hU, hX, hLL = np.empty((sweeps, C, A)), np.empty((sweeps, C, X.shape[1])), np.empty((sweeps, C))
    hAcc = np.empty((sweeps, C), dtype=bool)
    outside, folded, margin = 0, 0, np.inf
    for t in range(sweeps):
        g = 1.0 if jump_every > 0 and (t + 1) % jump_every == 0 else gamma0
        for k, (a, b) in enumerate(((0, half), (half, C))):
            partners = None if kind == "rw" else (U[half:] if k == 0 else U[:half])
            Up, Xp, inside = propose(U[a:b], partners, g, scale, a, seed, 2 * t + k, lo, hi, lg, flags, fold=bounds == "fold", rule=rule)
            ok = inside != 0
            LLp = np.full(b - a, -np.inf)
            if ok.any():
                LLp[ok] = loglik(Xp[ok])
            outside += int((~ok).sum())
            folded += int((inside == 2).sum())
            U[a:b], X[a:b], LL[a:b], acc, mg = mr.accept(U[a:b], X[a:b], LL[a:b], Up, Xp, LLp, inside, tf, a, seed, 2 * t + k)
            hAcc[t, a:b] = acc != 0
            margin = min(margin, float(mg.min()))
        hU[t], hX[t], hLL[t] = U, X, LL
    n = float(sweeps * C)
    return dict(U=hU, X=hX, LL=hLL, accepted=hAcc, outside=outside / n, folded=folded / n, margin=margin)


# ---- the face toy: the 3-D Gaussian of deviation TOY_SD centred at (0, 0.5, 1) on the cube -- one coordinate against a lower face,
# one in the interior, one against an upper face.  The far face of a half-Gaussian is 12.5 deviations away: its cut is below e^-78.
TOY_SD, TOY_A = mr.TOY_SD, mr.TOY_A
FACE_CENTRE = np.array([0.0, 0.5, 1.0])
_HALF_MEAN, _HALF_VAR = TOY_SD * np.sqrt(2.0 / np.pi), TOY_SD ** 2 * (1.0 - 2.0 / np.pi)
FACE_MEAN = np.array([_HALF_MEAN, 0.5, 1.0 - _HALF_MEAN])
FACE_VAR = np.array([_HALF_VAR, TOY_SD ** 2, _HALF_VAR])
FACE_SECOND = FACE_VAR + FACE_MEAN ** 2                           # E[u^2] per coordinate


def toy_face():
    """(loglik on unit coordinates, analytic mean (3,), analytic variance (3,))."""

    def loglik(U):
        e = np.asarray(U)[:, :TOY_A] - FACE_CENTRE
        return -0.5 * np.sum(e * e, axis=1) / TOY_SD ** 2

    return loglik, FACE_MEAN, FACE_VAR


# ---- the end-to-end run of the device test: the face toy on the box of mcmc_ref's end-to-end case (a log column in the middle),
# bounds="fold".  The seed is one whose smallest decision margin in the restatement is above mcmc_ref.E2E_MARGIN
# (tests/test_mcmc_fold_host.py asserts it).  The argument of mcmc_ref holds here too: the device's likelihoods differ from the
# restatement's only through the log column, whose coordinate is the interior one, centred at 1/2 as there.
E2E = dict(C=256, sweeps=60, seed=0)


def e2e_loglik(X):
    return toy_face()[0](rr.unit_coords(np.asarray(X), mr.E2E_LO, mr.E2E_HI, mr.E2E_LG)[0])


_e2e = []


def e2e_reference():
    """(U0, X0, LL0, run): the start and the restatement's run of the end-to-end case, computed once."""
    if not _e2e:
        U0 = mr.toy_start(E2E["C"], E2E["seed"])
        X0 = rr.from_unit(U0, mr.E2E_LO, mr.E2E_HI, mr.E2E_LG)
        LL0 = e2e_loglik(X0)
        _e2e.append((U0, X0, LL0, run(e2e_loglik, U0, LL0, mr.E2E_LO, mr.E2E_HI, mr.E2E_LG, sweeps=E2E["sweeps"], seed=E2E["seed"],
                                      bounds="fold")))
    return _e2e[0]
