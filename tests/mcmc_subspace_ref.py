"""Plain numpy restatement of the subspace differential-evolution proposal (trpl_mcmc_propose_subspace, include/trpl.h;
trpl_amd.mcmc.run(kind="subspace")): the draws of a chain from the Philox counter alone, the move on the
selected coordinates with the kernel's expression order, the fold through mcmc_fold_ref, and the driver of the sweeps with the
adaptation of the crossover shares.  Philox, the partner expressions and the accept step are tests/mcmc_ref.py's, the expressions of X
tests/refine_ref.py's.  No device, no library: the tests compare against this."""
import numpy as np

import mcmc_fold_ref as fr
import mcmc_ref as mr
import refine_ref as rr

CROSS_CALL, JUMP_CALL, SELECT_CALL, PAIR_CALL = 12, 20, 28, 28
MAX_PAIRS, MAX_CR = 4, 8


def gamma_table(pairs, A, factor=1.0):
    """(pairs, A): factor * 2.38 / sqrt(2 delta dsel), by (delta - 1, dsel - 1)."""
    delta, dsel = np.arange(1, pairs + 1, dtype=np.float64)[:, None], np.arange(1, A + 1, dtype=np.float64)[None, :]
    return float(factor) * (2.38 / np.sqrt(2.0 * delta * dsel))


def class_cdf(ncr, pcr=None):
    """(ncr,): the cumulative shares as the host forms them: (pcr[0] + .. + pcr[m], ascending from +0.0) / (the whole sum in that
    order); without pcr (m + 1) / ncr."""
    if pcr is None:
        return np.arange(1, ncr + 1, dtype=np.float64) / float(ncr)
    c, out = 0.0, np.empty(ncr)
    for m in range(ncr):
        c = c + float(pcr[m])
        out[m] = c
    return out / c


def _pair_of_call(count, group, chain0, call, seed, step):
    """mcmc_ref.partner_indices with any call index: (a, b), b != a, both in [0, group)."""
    r = mr._philox(chain0, count, call, seed, step)
    xa, xb = rr.res53(r[:, 0], r[:, 1]), rr.res53(r[:, 2], r[:, 3])
    a = np.minimum((xa * float(group)).astype(np.int64), group - 1)
    b = np.minimum((xb * float(group - 1)).astype(np.int64), group - 2)
    return a, b + (b >= a)


def _paired_uniforms(count, A, chain0, call0, seed, step):
    """(count, A): call call0 + j -> coordinates 2j, 2j + 1, as mcmc_ref.uniforms lays out the jitter's."""
    out = np.empty((count, A))
    for j in range((A + 1) // 2):
        r = mr._philox(chain0, count, call0 + j, seed, step)
        out[:, 2 * j] = rr.res53(r[:, 0], r[:, 1])
        if 2 * j + 1 < A:
            out[:, 2 * j + 1] = rr.res53(r[:, 2], r[:, 3])
    return out


def draws(count, A, group, chain0, seed, step, pairs, ncr, pcr=None):
    """Everything a chain draws, none of it from its state: dict(m, cr, delta, f (the fallback coordinate), c (count, A) the crossover
    uniforms, mask (count, A) bool, dsel, a and b (count, pairs) the rows inside the rung, v and xi (count, A))."""
    cdf = class_cdf(ncr, pcr)
    r = mr._philox(chain0, count, SELECT_CALL, seed, step)
    xm, xs = rr.res53(r[:, 0], r[:, 1]), rr.res53(r[:, 2], r[:, 3])
    m = (~(xm[:, None] < cdf[None, :ncr - 1])).cumprod(axis=1).sum(axis=1).astype(np.int64)   # the first m with xm < cdf[m]; the
    # last class is what is left: its boundary is never read
    cr = (m + 1).astype(np.float64) / float(ncr)
    t = xs * float(pairs)
    delta = np.minimum(t.astype(np.int64), pairs - 1) + 1
    xf = t - (delta - 1).astype(np.float64)
    f = np.minimum((xf * float(A)).astype(np.int64), A - 1)
    c = _paired_uniforms(count, A, chain0, CROSS_CALL, seed, step)
    mask = c < cr[:, None]
    none = ~mask.any(axis=1)
    mask[none, f[none]] = True
    a, b = np.empty((count, pairs), dtype=np.int64), np.empty((count, pairs), dtype=np.int64)
    for p in range(pairs):
        a[:, p], b[:, p] = _pair_of_call(count, group, chain0, mr.PARTNER_CALL if p == 0 else PAIR_CALL + p, seed, step)
    return dict(m=m, cr=cr, delta=delta, f=f, c=c, mask=mask, dsel=mask.sum(axis=1), a=a, b=b,
                v=_paired_uniforms(count, A, chain0, JUMP_CALL, seed, step), xi=mr.uniforms(count, A, chain0, seed, step))


def difference(partners, group, a, b, delta):
    """D (count, A) = (pa_0 - pb_0), then + (pa_p - pb_p) for p = 1 .. delta - 1 in turn; rows inside the chain's rung."""
    count = a.shape[0]
    base = (np.arange(count) // group) * group
    D = partners[base + a[:, 0]] - partners[base + b[:, 0]]
    for p in range(1, a.shape[1]):
        more = D + (partners[base + a[:, p]] - partners[base + b[:, p]])
        D = np.where((p < delta)[:, None], more, D)
    return D


def move(U, D, g, e_width, v, scale, xi, mask, sign=1.0):
    """u' on the selected coordinates, (u + (g (1 + e_width (2 v - 1))) D) + sign (scale (2 xi - 1)), one rounding per operation;
    the others keep u's bits.  sign = -1 is the negated jitter of the reverse move (a product's negation is exact)."""
    ge = g[:, None] * (1.0 + e_width * (2.0 * v - 1.0))
    moved = (U + ge * D) + sign * (scale * (2.0 * xi - 1.0))
    return np.where(mask, moved, U)


def propose_unit(U, partners, group, tab, scale, chain0, seed, step, ncr=3, pcr=None, e_width=0.05, fold=False):
    """(Up, inside, mask, sel, raw): the proposal in unit coordinates.  inside is trpl_mcmc_propose's code over the SELECTED coordinates
    (0 / 1, with fold 0 / 1 / 2); mask (count,) int32 bit d = coordinate d selected; sel = delta | m << 8; raw the unfolded u'."""
    U, partners, tab = (np.asarray(x, dtype=np.float64) for x in (U, partners, tab))
    count, A = U.shape
    group = partners.shape[0] if group is None else int(group)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (A,))
    d = draws(count, A, group, chain0, seed, step, tab.shape[0], ncr, pcr)
    D = difference(partners, group, d["a"], d["b"], d["delta"])
    g = tab[d["delta"] - 1, d["dsel"] - 1]
    raw = move(U, D, g, e_width, d["v"], scale, d["xi"], d["mask"])
    with np.errstate(invalid="ignore"):
        out = d["mask"] & ~((raw >= 0.0) & (raw <= 1.0))
    if fold:
        Up = np.where(out, fr.fold(raw), raw)
        inside = np.where((d["mask"] & np.isnan(Up)).any(axis=1), 0, np.where(out.any(axis=1), 2, 1)).astype(np.int32)
    else:
        Up, inside = raw, (~out.any(axis=1)).astype(np.int32)
    mask = (d["mask"] * (1 << np.arange(A))).sum(axis=1).astype(np.int32)
    return Up, inside, mask, (d["delta"] | d["m"] << 8).astype(np.int32), raw


def propose(U, partners, group, tab, scale, chain0, seed, step, lo, hi, lg, ncr=3, pcr=None, e_width=0.05, flags=0, fold=False):
    """(Up, Xp, inside, mask, sel): Xp by the sampler's expressions from u', for every column."""
    Up, inside, mask, sel, _ = propose_unit(U, partners, group, tab, scale, chain0, seed, step, ncr, pcr, e_width, fold)
    return Up, rr.from_unit(Up, lo, hi, lg, flags), inside, mask, sel


def adapted_pcr(jump, tried, ncr):
    """trpl_amd.mcmc.adapted_pcr: the mean squared jump per proposal of each class, normalised, floored at 1 / (10 ncr), renormalised."""
    mean = np.full(ncr, np.nan)
    mean[tried > 0] = jump[tried > 0] / tried[tried > 0]
    mean[tried <= 0] = mean[tried > 0].mean() if np.any(tried > 0) else 1.0
    total = mean.sum()
    q = mean / total if total > 0.0 and np.isfinite(total) else np.full(ncr, 1.0 / ncr)
    q = np.maximum(q, 1.0 / (10.0 * ncr))
    return q / q.sum()


def run(loglik, U0, LL0, lo, hi, lg, flags=0, sweeps=100, tf=1.0, gamma=None, scale=None, jump_every=0, seed=1, bounds="reject", pairs=3,
        ncr=3, e_width=0.05, pcr=None, adapt_cr=False, burn=0):
    """The sweeps of trpl_amd.mcmc.run(kind="subspace") with keep_every = 1 and every sweep kept (burn only bounds the adaptation).
    Returns mcmc_fold_ref.run's dict and mean_dsel, pcr (the final shares), pcr_trace (sweeps, ncr)."""
    U, LL = np.array(U0, dtype=np.float64), np.array(LL0, dtype=np.float64)
    C, A = U.shape
    X = rr.from_unit(U, lo, hi, lg, flags)
    scale = 1e-3 if scale is None else scale
    tab = gamma_table(pairs, A, 1.0 if gamma is None else gamma)
    pcr = np.full(ncr, 1.0 / ncr) if pcr is None else np.asarray(pcr, dtype=np.float64) / np.sum(pcr)
    half, fold = C // 2, bounds == "fold"
    hU, hX, hLL = np.empty((sweeps, C, A)), np.empty((sweeps, C, X.shape[1])), np.empty((sweeps, C))
    hAcc, trace = np.empty((sweeps, C), dtype=bool), np.empty((sweeps, ncr))
    outside, folded, margin, dsel, dn = 0, 0, np.inf, 0, 0
    jump, tried = np.zeros(ncr), np.zeros(ncr, dtype=np.int64)
    for t in range(sweeps):
        jumping = jump_every > 0 and (t + 1) % jump_every == 0
        adapting = adapt_cr and t < burn and not jumping
        trace[t] = pcr
        for k, (a, b) in enumerate(((0, half), (half, C))):
            partners = U[half:] if k == 0 else U[:half]
            if jumping:
                Up, Xp, inside = fr.propose(U[a:b], partners, 1.0, scale, a, seed, 2 * t + k, lo, hi, lg, flags, fold=fold)
            else:
                Up, Xp, inside, mask, sel = propose(U[a:b], partners, half, tab, scale, a, seed, 2 * t + k, lo, hi, lg, ncr, pcr, e_width, flags,
                                                    fold)
                dsel += int(np.unpackbits(mask.view(np.uint8)).sum())
                dn += half
                sd, before = U.std(axis=0), U[a:b].copy()
            ok = inside != 0
            LLp = np.full(b - a, -np.inf)
            if ok.any():
                LLp[ok] = loglik(Xp[ok])
            outside += int((~ok).sum())
            folded += int((inside == 2).sum())
            U[a:b], X[a:b], LL[a:b], acc, mg = mr.accept(U[a:b], X[a:b], LL[a:b], Up, Xp, LLp, inside, tf, a, seed, 2 * t + k)
            hAcc[t, a:b] = acc != 0
            margin = min(margin, float(mg.min()))
            if adapting:
                with np.errstate(invalid="ignore", divide="ignore"):
                    z2 = (((U[a:b] - before) / sd) ** 2).sum(axis=1)
                jump += np.bincount(sel >> 8, weights=np.where(np.isfinite(z2), z2, 0.0), minlength=ncr)
                tried += np.bincount(sel >> 8, minlength=ncr)
        if adapting:
            pcr = adapted_pcr(jump, tried, ncr)
        hU[t], hX[t], hLL[t] = U, X, LL
    n = float(sweeps * C)
    return dict(U=hU, X=hX, LL=hLL, accepted=hAcc, outside=outside / n, folded=folded / n, margin=margin, mean_dsel=dsel / float(max(dn, 1)),
                pcr=pcr, pcr_trace=trace)


# ---- the correlated toy of the device test: a 10-D Gaussian of deviation TEN_SD centred in the cube, coordinates 0 and 1 correlated by
# TEN_RHO, the others independent.  256 chains, bounds="fold" (the far faces are 6 deviations away).
TEN_A, TEN_SD, TEN_RHO, TEN_C, TEN_SWEEPS, TEN_BURN = 10, 0.08, 0.9, 256, 80, 20
TEN_BOX = (np.zeros(TEN_A), np.ones(TEN_A), np.zeros(TEN_A, dtype=np.int32))
TEN_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
TEN_DEVICE_SEED = 1


def _ten_precision():
    cov = TEN_SD ** 2 * np.eye(TEN_A)
    cov[0, 1] = cov[1, 0] = TEN_RHO * TEN_SD ** 2
    return np.linalg.inv(cov)


_TEN_PREC = _ten_precision()


def ten_loglik(X):
    e = np.asarray(X)[:, :TEN_A] - 0.5
    return -0.5 * np.einsum("si,ij,sj->s", e, _TEN_PREC, e)


def ten_start(seed):
    """Starts drawn from the target itself, so the sweeps before TEN_BURN only have to decorrelate them: what is tested is that the
    move keeps the distribution, and a wrong move leaves it within a few sweeps."""
    z = np.random.default_rng([seed, TEN_C, 33]).normal(size=(TEN_C, TEN_A))
    U0 = 0.5 + z @ np.linalg.cholesky(np.linalg.inv(_TEN_PREC)).T
    return U0, ten_loglik(U0)


def ten_stats(U):
    """(2 A + 1,): the means, the deviations and the correlation of coordinates 0 and 1 of the kept states U (n, C, A)."""
    flat = U.reshape(-1, U.shape[-1])
    return np.concatenate([flat.mean(axis=0), flat.std(axis=0), [np.corrcoef(flat[:, 0], flat[:, 1])[0, 1]]])


TEN_TRUTH = np.concatenate([np.full(TEN_A, 0.5), np.full(TEN_A, TEN_SD), [TEN_RHO]])
_ten = {}


def ten_gates():
    """(lo, hi), each (2 A + 1,): the mean +- 5 standard deviations (ddof = 1) of ten_stats over the restatement's own runs of the
    seeds TEN_SEEDS, kept sweeps from TEN_BURN on; computed once."""
    if "gates" not in _ten:
        rows = []
        for seed in TEN_SEEDS:
            U0, LL0 = ten_start(seed)
            res = run(ten_loglik, U0, LL0, *TEN_BOX, sweeps=TEN_SWEEPS, seed=seed, bounds="fold")
            rows.append(ten_stats(res["U"][TEN_BURN:]))
        rows = np.array(rows)
        _ten["rows"] = rows
        _ten["gates"] = (rows.mean(axis=0) - 5.0 * rows.std(axis=0, ddof=1), rows.mean(axis=0) + 5.0 * rows.std(axis=0, ddof=1))
    return _ten["gates"]
