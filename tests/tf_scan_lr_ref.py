"""numpy.longdouble reference of the posterior core with a proposal log-ratio kept beside LL (trpl_posterior_weights_lr,
trpl_posterior_tf_scan_lr; include/trpl.h), the grid rule of posterior.tf_for_ess, and the temperature-ladder form of the
refinement driver of tests/refine_ref.py.  No device, no library: the tests compare against this.

    e_k[s] = LL[s] / tf_k - lnr[s],   m_k = nanmax_s e_k[s],   w_k[s] = exp(((e_k[s] - m_k) + 1000 ln 2) - ln S),   W_k = w_k / nansum w_k
"""
import numpy as np

import highprec as hp
import refine_ref as rr

LD = np.longdouble


def weights(LL, lnr, tf):
    """W (S,) longdouble: NaN where LL or lnr is NaN (and out of max and sum), 0 where LL = -inf or lnr = +inf."""
    LL = np.asarray(LL, dtype=np.float64).astype(LD)
    lnr = np.asarray(lnr, dtype=np.float64).astype(LD)
    with np.errstate(invalid="ignore"):
        e = LL / LD(tf) - lnr
        w = np.exp(e - np.nanmax(e) + LD(1000) * np.log(LD(2)) - np.log(LD(LL.size)))
    return w / np.nansum(w)


def scan(LL, lnr, tfs, V=None):
    """What trpl_posterior_tf_scan_lr defines, every row from weights() above and highprec.moments: dict(stats (K, 6) = [m_k, raw
    sum, sum W, sum W^2, count, ess], mean, var, Q (K, D)) in longdouble.  (m_k and the raw sum are those of the longdouble
    exponent; the raw sum carries the lift 2^1000 / S.)"""
    LL64, lnr64 = np.asarray(LL, dtype=np.float64), np.asarray(lnr, dtype=np.float64)
    tfs = np.atleast_1d(np.asarray(tfs, dtype=np.float64))
    D = 0 if V is None else np.atleast_2d(V).shape[0]
    out = dict(stats=np.zeros((tfs.size, 6), dtype=LD), mean=np.zeros((tfs.size, D), dtype=LD), var=np.zeros((tfs.size, D), dtype=LD),
               Q=np.zeros((tfs.size, D), dtype=LD))
    count = np.count_nonzero(~(np.isnan(LL64) | np.isnan(lnr64)))
    for k, tf in enumerate(tfs):
        with np.errstate(invalid="ignore"):
            e = LL64.astype(LD) / LD(tf) - lnr64.astype(LD)
            m = np.nanmax(e)
            raw = np.nansum(np.exp(e - m + LD(1000) * np.log(LD(2)) - np.log(LD(LL64.size))))
        W = weights(LL64, lnr64, tf)
        sw, sw2 = W.sum(), (W * W).sum()
        out["stats"][k] = m, raw, sw, sw2, count, sw * sw / sw2
        if D:
            s, c = hp.moments(V, W.astype(np.float64))          # the moments of the fp64 weights, as the device call is given them
            var = np.diag(c[:, :D]) / s[0]
            out["mean"][k], out["var"][k], out["Q"][k] = s[2:] / s[0], var, np.sqrt(s[1] * var)
    return out


def ess_at(LL, lnr, tf):
    """(sum W)^2 / sum W^2 at one temperature in plain float64; a NaN sample counts as weight 0."""
    with np.errstate(invalid="ignore"):
        e = np.asarray(LL, dtype=np.float64) / tf - np.asarray(lnr, dtype=np.float64)
    w = np.exp(e - np.nanmax(e))
    w = np.where(np.isnan(w), 0.0, w)
    return float(w.sum() ** 2 / np.sum(w * w))


def grid(lo, hi, k):
    """k temperatures equally spaced in ln tf over [lo, hi], the ends exactly."""
    t = np.exp(np.log(lo) + (np.log(hi) - np.log(lo)) * (np.arange(k) / (k - 1)))
    t[0], t[-1] = lo, hi
    return t


def tf_for_ess(objective, target, lo, hi, k=64, rtol=1e-6):
    """The grid rule of posterior.tf_for_ess, restated: every round lays grid(lo, hi, k), takes the SMALLEST grid temperature
    whose objective is >= target and continues on [its lower neighbour, it] until hi / lo - 1 <= rtol.  Returns (tf, ess,
    at_edge, scans): at_edge "hi" when no point of the first grid reaches the target (hi is returned), "lo" when the lowest does."""
    scans = 0
    while True:
        t = grid(lo, hi, k)
        v = np.asarray(objective(t), dtype=np.float64)
        scans += 1
        hit = [i for i in range(k) if v[i] >= target]
        if not hit:
            assert scans == 1, "a later round's upper end reached the target in the round before"
            return hi, float(v[-1]), "hi", scans
        i = hit[0]
        if i == 0:
            assert scans == 1, "a later round's lower end missed the target in the round before"
            return lo, float(v[0]), "lo", scans
        lo, hi = float(t[i - 1]), float(t[i])
        if hi / lo - 1.0 <= rtol:
            return hi, float(v[i]), None, scans


def weights64(LL, lnr, tf):
    """Weights that sum to 1 at temperature tf with the ratio beside LL, float64 (refine_ref.normalize's form)."""
    return rr.normalize(np.asarray(LL, dtype=np.float64) / tf - np.asarray(lnr, dtype=np.float64))


def run_ladder(loglik_unit, U1, rounds, K, m, n_uniform, target_ess, tf=1.0, tf_hi=None, seed=1, h=None, offset=0.5):
    """refine_ref.run with the temperature ladder: generation g's proposal is built from the union's weights at
    tf_g = max(tf, tf_for_ess(union, target_ess, lo = tf, hi = tf_hi)), tf_hi defaulting to 1e4 tf.  Returns dict(U, LL, lnr, tfs (one
    per further generation), ess (the union's at the temperature its proposal was built at, then the final union's at tf), ess_at_tf
    (the union's at tf: the first generation's, then after each further one), proposals)."""
    S1 = U1.shape[0]
    U, LL = U1, loglik_unit(U1)
    props, esses, tfs, at_tf = [], [], [], []
    tf_hi = 1e4 * tf if tf_hi is None else tf_hi
    for g in range(2, 2 + rounds):
        lnr = rr.log_ratio(U, S1, props)
        at_tf.append(ess_at(LL, lnr, tf))
        tfs.append(max(tf, tf_for_ess(lambda t: [ess_at(LL, lnr, x) for x in t], target_ess, tf, tf_hi)[0]))
        W = weights64(LL, lnr, tfs[-1])
        esses.append(rr.ess(W))
        idx, _, _ = rr.resample(W, K, offset)
        hh = rr.bandwidth(U, W, S1) if h is None else h
        a, b, iv = rr.boxes(U[idx], hh)
        props.append(dict(a=a, b=b, inv_vol=iv, m=m, n_uniform=n_uniform, seed=seed, generation=g))
        U2 = rr.draw_unit(a, b, m, n_uniform, seed, g)
        U, LL = np.concatenate([U, U2]), np.concatenate([LL, loglik_unit(U2)])
    lnr = rr.log_ratio(U, S1, props)
    esses.append(rr.ess(weights64(LL, lnr, tf)))
    at_tf.append(esses[-1])
    return dict(U=U, LL=LL, lnr=lnr, tfs=tfs, ess=esses, ess_at_tf=at_tf, proposals=props, S1=S1)


# ---- the ladder toy of the tests: DESIGN.md section 19's toy, narrowed until the first generation's effective sample size at tf = 1
# is of order 1
LADDER_SD, LADDER_A, LADDER_S1, LADDER_K, LADDER_M, LADDER_NU, LADDER_ROUNDS = 0.02, 3, 4096, 128, 32, 512, 2
LADDER_TARGET = 64.0                 # half the parents: a proposal whose K = 128 boxes sit around at least ~64 distinct samples
