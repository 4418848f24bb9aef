"""Plain numpy restatement of the sums of the log-evidence estimates (trpl_mcmc_evidence_sums, include/trpl.h):
the extrema rule, the fp64 exponent, the term with its rule of -inf and zero, the strided partials and the halving tree in loops --
and a second form that takes the same fp64 exponents but does exp and the additions in np.longdouble, which is what the device's
four exponential sums are held to.  Then the Gaussian toy of the statistics tests with its analytic targets and the gates, which
come from the numpy restatement of run_tempered (mcmc_tempered_ref.py) and never from the code under test.  No device, no library."""
import math

import numpy as np

THREADS, NSUMS = 256, 6


def deltas(tf):
    """delta_k = 1.0 / tf[k] - 1.0 / tf[k + 1], (K - 1,): trpl_mcmc_swap's expression, one rounding per operation."""
    tf = np.asarray(tf, dtype=np.float64)
    return 1.0 / tf[:-1] - 1.0 / tf[1:]


def extrema(LL, t0, t1):
    """ext (K, 2): [maximum, minimum] of each rung over the steps [t0, t1), a zero as +0.0; both NaN when the rung has a NaN there."""
    x = np.asarray(LL, dtype=np.float64)[:, t0:t1].reshape(LL.shape[0], -1)
    ext = np.empty((x.shape[0], 2))
    for k in range(x.shape[0]):
        ext[k] = (np.nan, np.nan) if np.isnan(x[k]).any() else (x[k].max() + 0.0, x[k].min() + 0.0)
    return ext


def coefficients(tf, ext, k):
    """(cu, au, cd, ad): the coefficient and the centre of rung k's up and down terms; a coefficient is None where the sum does not
    exist (k = 0, k = K - 1)."""
    d = deltas(tf)
    K = len(tf)
    cu = d[k - 1] if k > 0 else None
    cd = -d[k] if k + 1 < K else None
    au = None if cu is None else ext[k, 0] if cu >= 0.0 else ext[k, 1]
    ad = None if cd is None else ext[k, 1] if cd <= 0.0 else ext[k, 0]
    return cu, au, cd, ad


def exponents(x, c, a):
    """c * (x - a) in fp64: a subtraction and a product, one rounding each."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float64(c) * (np.asarray(x, dtype=np.float64) - np.float64(a))


def terms(x, c, a, dtype=np.float64):
    """The term of every x: exp of the fp64 exponent, taken in `dtype`; x = -inf gives +0.0 for c >= 0 and +inf for c < 0 and is not
    put through the expression; c = +-0.0 gives 1.0 for every x above -inf."""
    x = np.asarray(x, dtype=np.float64)
    if c == 0.0:
        return np.where(x > -np.inf, 1.0, 0.0).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        e = np.exp(exponents(x, c, a).astype(dtype))
    return np.where(x == -np.inf, dtype(np.inf if c < 0.0 else 0.0), e)


def tree_sum(v):
    """The one association of a block's sum: thread j adds the elements j, j + 256, .. ascending from +0.0, then the 256 partials are
    added by the halving tree p[j] = p[j] + p[j + s], s = 128 .. 1."""
    v = np.asarray(v, dtype=np.float64).ravel()
    p = np.zeros(THREADS)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(0, v.size, THREADS):                      # round r: every thread that still has an element adds its next one
            chunk = v[r:r + THREADS]
            p[:chunk.size] = p[:chunk.size] + chunk
        s = THREADS // 2
        while s >= 1:
            for j in range(s):
                p[j] = p[j] + p[j + s]
            s //= 2
    return p[0]


def _blocks(LL, t0, t1, B):
    K = LL.shape[0]
    w = (t1 - t0) // B
    for k in range(K):
        for b in range(B):
            yield k, b, np.asarray(LL, dtype=np.float64)[k, t0 + b * w:t0 + (b + 1) * w].ravel()


def sums(LL, tf, t0, t1, B):
    """(ext (K, 2), sums (K, B, 6)) in fp64 with the device's association: [sum x, up, up2, down, down2, count above -inf].  The sum
    of x and the count are the device's bits; the exponential sums differ from the device's by exp's last bits only."""
    K = LL.shape[0]
    ext, out = extrema(LL, t0, t1), np.zeros((K, B, NSUMS))
    for k, b, x in _blocks(LL, t0, t1, B):
        if np.isnan(ext[k, 0]):
            out[k, b] = np.nan
            continue
        cu, au, cd, ad = coefficients(tf, ext, k)
        out[k, b, 0], out[k, b, 5] = tree_sum(x), tree_sum(np.where(x > -np.inf, 1.0, 0.0))
        for c, a, slot in ((cu, au, 1), (cd, ad, 3)):
            if c is not None:
                e = terms(x, c, a)
                with np.errstate(over="ignore"):
                    out[k, b, slot], out[k, b, slot + 1] = tree_sum(e), tree_sum(e * e)
    return ext, out


def sums_long(LL, tf, t0, t1, B):
    """sums (K, B, 6) in np.longdouble: the same fp64 exponents, exp and every addition in long double (the order of a long-double
    sum is below what the tolerance sees)."""
    K = LL.shape[0]
    ext, out = extrema(LL, t0, t1), np.zeros((K, B, NSUMS), dtype=np.longdouble)
    for k, b, x in _blocks(LL, t0, t1, B):
        if np.isnan(ext[k, 0]):
            out[k, b] = np.nan
            continue
        cu, au, cd, ad = coefficients(tf, ext, k)
        with np.errstate(invalid="ignore", over="ignore"):
            out[k, b, 0], out[k, b, 5] = np.sum(x.astype(np.longdouble)), np.sum(x > -np.inf)
            for c, a, slot in ((cu, au, 1), (cd, ad, 3)):
                if c is not None:
                    e = terms(x, c, a, np.longdouble)
                    out[k, b, slot], out[k, b, slot + 1] = np.sum(e), np.sum(e * e)
    return out


def sums_rtol(w, C):
    """The relative tolerance of an exponential sum of w C terms: 1e-13, the gate tests/test_gpu_posterior_instances.py holds the
    device's tempered weights to (exp of an fp64 exponent), + one rounding 2^-53 per addition on the longest path from a term to the
    result: ceil(w C / 256) additions in a thread and 8 levels of the tree.  All terms are >= 0, so the bound on a path is the
    bound on the sum."""
    return 1e-13 + (math.ceil(w * C / THREADS) + 8) * 2.0 ** -53


# ---- the device cases: K rungs, C chains, B blocks of w steps; T0 rows before and TAIL rows after the range are NaN
T0, TAIL = 2, 3
KS, CS, BS = (1, 2, 3, 64), (1, 255, 256, 257, 1000), (1, 2, 7)


def case_w(C):
    """Steps per block: w C is below 256 at C = 1 (w = 3) and C = 255 (w = 1: one partial short of a full round), exactly 256 at
    C = 256 (w = 1), above it with a ragged last round elsewhere (C = 257: w = 3; C = 1000: w = 2)."""
    return {1: 3, 255: 1, 256: 1, 257: 3, 1000: 2}[C]


def case_ladder(K):
    """Increasing temperatures with unequal ratios; K = 64 fills the kernel argument."""
    return 1.0 + np.cumsum(0.05 + 0.1 * np.random.default_rng([5, K]).random(K))


def case_LL(K, C, B, seed=0):
    """LL (K, T0 + B w + TAIL, C): log-likelihoods of a few units' spread around an offset that differs per rung, NaN outside the range."""
    w = case_w(C)
    rng = np.random.default_rng([seed, K, C, B])
    LL = np.full((K, T0 + B * w + TAIL, C), np.nan)
    LL[:, T0:T0 + B * w] = -3.0 * rng.chisquare(3, size=(K, B * w, C)) - 10.0 * np.arange(1, K + 1)[:, None, None]
    return LL


# ---- the Gaussian toy of the statistics tests: LL = -|u - 1/2|^2 / (2 sd^2) on the unit cube of GA_D dimensions
GA_SD, GA_D, GA_C, GA_SWEEPS, GA_BURN, GA_BLOCKS, GA_K, GA_HOT, GA_BASE = 0.03, 3, 64, 300, 100, 8, 7, 8.0, 4096
GA_BOX = (np.zeros(GA_D), np.ones(GA_D), np.zeros(GA_D, dtype=np.int32))
GA_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
GA_DEVICE_SEED = 1


def gauss_loglik(X):
    return -np.sum((np.asarray(X)[:, :GA_D] - 0.5) ** 2, axis=1) / (2.0 * GA_SD ** 2)


def gauss_start(seed):
    U0 = 0.5 + GA_SD * np.random.default_rng([seed, 78]).normal(size=(GA_C, GA_D))
    return U0, gauss_loglik(U0)


def gauss_base(seed):
    """The LL of GA_BASE uniform draws of the cube: the importance run that anchors the ladder at its hottest rung."""
    return gauss_loglik(np.random.default_rng([seed, 79]).random((GA_BASE, GA_D)))


def gauss_ln_z(tf):
    """ln of the integral of exp(LL / tf) over the cube: per dimension sd sqrt(2 pi tf) erf(1 / (2 sd sqrt(2 tf)))."""
    return GA_D * (math.log(GA_SD * math.sqrt(2.0 * math.pi * tf)) + math.log(math.erf(0.5 / (GA_SD * math.sqrt(2.0 * tf)))))


def gauss_mean_ll(tf):
    """E[LL] at temperature tf = d ln Z / d beta, beta = 1 / tf: per dimension -1 / (2 beta) + (erf'(z) / erf(z)) z / (2 beta), z = the
    argument of erf above."""
    beta = 1.0 / tf
    z = 0.5 * math.sqrt(beta) / (GA_SD * math.sqrt(2.0))
    return GA_D * (-0.5 / beta + 2.0 / math.sqrt(math.pi) * math.exp(-z * z) / math.erf(z) * z / (2.0 * beta))


def gauss_targets(ladder):
    """(stepping stone, ti): ln Z(ladder[0]) - ln Z(ladder[-1]), what forward and reverse estimate, and the trapezoid of the analytic
    E[LL] on the ladder, what ti estimates -- its discretisation bias is the rule's, not the sampler's."""
    d = deltas(ladder)
    mean = np.array([gauss_mean_ll(t) for t in ladder])
    return gauss_ln_z(ladder[0]) - gauss_ln_z(ladder[-1]), float(np.sum(d * (mean[:-1] + mean[1:]) / 2.0))


def gauss_restatement(seed, log_evidence_ratios):
    """[forward total, reverse total, ti total, base ln Z(GA_HOT)] of one seed, everything in numpy: run_tempered of
    mcmc_tempered_ref.py, the sums above, the estimator passed in (trpl_amd.mcmc.log_evidence_ratios, pure numpy), and the
    long-double mean of the base."""
    import mcmc_tempered_ref as tr
    ladder = tr.geometric_ladder(1.0, GA_HOT, GA_K)
    U0, LL0 = gauss_start(seed)
    lo, hi, lg = GA_BOX
    LL = tr.run_tempered(gauss_loglik, U0, LL0, lo, hi, lg, ladder, sweeps=GA_SWEEPS, seed=seed)["LL"]
    ext, s = sums(LL, ladder, GA_BURN, GA_SWEEPS, GA_BLOCKS)
    r = log_evidence_ratios(ext, s, ladder)
    base = float(np.log(np.mean(np.exp(gauss_base(seed).astype(np.longdouble) / GA_HOT))))
    return [r["forward_total"], r["reverse_total"], r["ti_total"], base]


# gauss_restatement(seed, trpl_amd.mcmc.log_evidence_ratios) for the seeds of GA_SEEDS in turn, computed on the CPU by
#     python -c "import sys; sys.path[:0] = ['.', 'tests']; import trpl_amd, mcmc_evidence_ref as e; \
#                print([e.gauss_restatement(s, trpl_amd.mcmc.log_evidence_ratios) for s in e.GA_SEEDS])"
# (tests/test_mcmc_evidence_host.py recomputes the first).  A gate of the device test is 5 standard deviations (numpy.std, the
# narrower ddof = 0) of a column of these about its analytic target; the absolute ln Z(1) adds the base to a total, so its gate is
# formed from the sum of the two columns.
GA_RESTATEMENT = (
    (-3.12852012355562, -3.134857825469556, -3.1917531338623446, -4.669295697396935),
    (-3.0826719554546216, -3.0620478456504387, -3.1356159630326372, -4.731326657450074),
    (-3.150261840572109, -3.1507525776079564, -3.2169025502869224, -4.7073185558380715),
    (-3.0967542928499237, -3.1031088558405298, -3.161712063475087, -4.733091349350216),
    (-3.1345589701289986, -3.1410981440107415, -3.2015293945072827, -4.478399708263759),
    (-3.1284276578801147, -3.1218160049917385, -3.19146799676833, -4.729403292170475),
    (-3.1130858114496966, -3.1154790698366583, -3.176429275591944, -4.5873727365062145),
    (-3.123005345588563, -3.1195781014064043, -3.1855473257420903, -4.767328994119052))
# analytic: ln Z(1) - ln Z(8) = -3.119162, the trapezoid of E[LL] -3.181980, ln Z(8) = -4.643696; the columns' means are -3.119661,
# -3.118592, -3.182620, -4.675442 and their deviations 0.0202, 0.0257, 0.0234, 0.0904


def gauss_gates():
    """dict(forward, reverse, ti, ln_z_forward, ln_z_reverse, ln_z_ti): (target, margin) of each gated figure."""
    import mcmc_tempered_ref as tr
    ladder = tr.geometric_ladder(1.0, GA_HOT, GA_K)
    r = np.array(GA_RESTATEMENT)
    stone, ti = gauss_targets(ladder)
    out = {}
    for i, (name, target) in enumerate((("forward", stone), ("reverse", stone), ("ti", ti))):
        out[name] = (target, 5.0 * float(np.std(r[:, i])))
        out["ln_z_" + name] = (target + gauss_ln_z(GA_HOT), 5.0 * float(np.std(r[:, i] + r[:, 3])))
    return out
