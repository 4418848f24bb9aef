"""Posterior core: what consumes the likelihood vector.

Host-side mirror of the numeric functions of the reference's Visualization/utils.py, same names and
argument meaning, every reduction over the samples running on the GPU through libtrpl_hip.so
(trpl_posterior_weights / _moments / _hist; csrc/posterior.hip).  No CPU fallback: without the library
or a device these raise TrplError / ImportError.

    normalize(lnP)                               utils.py:157-166
    temper(LL, num_observations, c)              marginalization_visual.py:589-591
    w_mean, w_variance, w_sample_var, w_skew,
    w_kurtosis, covariance                       utils.py:168-170, :197-227
    marginalize_1D, marginalize_2D               utils.py:239-285
    filter_nan                                   utils.py:33-38
    summarize(...)                               LikelihoodData.stats_summarize / calc_covariance, utils.py:117-143
"""
import numpy as np

from . import _abi


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def filter_nan(X, LL):
    """Drop the samples whose likelihood is NaN (LikelihoodData.filter_nan, utils.py:33-38)."""
    LL = np.asarray(LL)
    keep = ~np.isnan(LL)
    return np.asarray(X)[keep], LL[keep]


def _log_ratio(log_ratio, S):
    lnr = _f64(log_ratio)
    if lnr.shape != (S,):
        raise ValueError("log_ratio must have one entry per sample")
    return lnr


def weights(LL, tf=1.0, device=0, info=None, log_ratio=None):
    """normalize(LL / tf): posterior weights that sum to 1 (NaN stays NaN, -inf gives 0).  log_ratio (S,): ln r(u) of a refined
    set (refine.Population.log_ratio), kept beside LL -- the weights of exp(LL / tf) / r (trpl_posterior_weights_lr); a NaN in
    either gives NaN, +inf in log_ratio gives 0; info["max"] is then the largest LL / tf - log_ratio."""
    LL = _f64(LL)
    if LL.ndim != 1:
        raise ValueError("LL must be one-dimensional")
    W = np.empty_like(LL)
    stats = np.zeros(2)
    sec = _abi.C.c_double(0.0)
    if log_ratio is None:
        _abi.check(_abi.lib().trpl_posterior_weights(_abi.ptr(LL), LL.size, float(tf), _abi.ptr(W), _abi.ptr(stats),
                                                     int(device), _abi.C.byref(sec)))
    else:
        lnr = _log_ratio(log_ratio, LL.size)
        _abi.check(_abi.lib().trpl_posterior_weights_lr(_abi.ptr(LL), _abi.ptr(lnr), LL.size, float(tf), _abi.ptr(W),
                                                        _abi.ptr(stats), int(device), _abi.C.byref(sec)))
    if info is not None:
        info.update(max=stats[0], raw_sum=stats[1], seconds=sec.value)
    return W


def exact_cut_margin(tf=1.0):
    """The margin below the best sample's likelihood from which a sample's posterior weight at tempering factor tf is
    EXACTLY 0.0 in fp64: tf * (1000 ln 2 + 746).  For driver.simulate's gpu_info["cut_margin"] / loglik(sse_cut=).

    The weight kernel (csrc/posterior.hip, weights_partial; utils.py:164) forms, in this order,
        q = LL / tf;   w = exp(((q - max q) + 1000 ln 2) - ln S).
    A sample cut at sse_cut = margin + best_total has LL <= -(margin + best_total) while max LL >= -best_total' with
    best_total' <= best_total (the running minimum only falls), so q - max q <= -margin / tf = -(1000 ln 2 + 746): the
    argument of exp is <= -746 - ln S, and ln S >= 0 is dropped conservatively.  exp underflows to 0.0 below
    ln(2^-1075) = -745.14 (half the smallest subnormal); the 0.86 in between covers the roundings of the division and the
    three additions, each below 1e-10 for |LL / tf| < 1e5.  The kernel then multiplies w by 1 + corr, |corr| < 2^-30, which
    puts those roundings back (posterior_common.hpp, tempered_weight): a w of 0.0 stays 0.0, and corr is a function of the
    sample's own LL alone.  A zero weight contributes nothing to the sum the others are divided by, so the weights of the
    uncut samples are unchanged too: the posterior equals the uncut run's."""
    import math
    return float(tf) * (1000.0 * math.log(2.0) + 746.0)


def normalize(lnP, device=0):
    """utils.py:157-166."""
    return weights(lnP, 1.0, device=device)


def temper(LL, num_observations, c, device=0):
    """P = normalize(LL / (num_observations * c)), marginalization_visual.py:589-591."""
    return weights(LL, float(num_observations) * float(c), device=device)


def moments(V, W, mean_in=None, device=0):
    """Raw weighted sums of the columns V (D, S) under weights W (S,):
    returns (sums[2+D] = [sum w, sum w^2, sum w v_d], central[D][D+2]) as trpl_posterior_moments defines them."""
    V = _f64(V)
    W = _f64(W)
    if V.ndim == 1:
        V = V[None, :]
    D, S = V.shape
    if W.shape != (S,):
        raise ValueError("W must have one weight per sample")
    sums = np.zeros(2 + D)
    central = np.zeros((D, D + 2))
    m = None if mean_in is None else _f64(mean_in)
    if m is not None and m.shape != (D,):
        raise ValueError("mean_in must have one entry per column")
    _abi.check(_abi.lib().trpl_posterior_moments(_abi.ptr(V), S, D, _abi.ptr(W), _abi.ptr(m), _abi.ptr(sums),
                                                 _abi.ptr(central), int(device), None))
    return sums, central


def w_mean(var, wts, device=0):
    """utils.py:197-199."""
    s, _ = moments(var, wts, device=device)
    return s[2] / s[0]


def w_variance(var, wts, device=0):
    """utils.py:202-204."""
    s, c = moments(var, wts, device=device)
    return c[0, 0] / s[0]


def w_sample_var(val, wts, ws, device=0):
    """utils.py:168-170 (the reference's name; it is a standard deviation): sqrt(ws * weighted variance)."""
    return np.sqrt(ws * w_variance(val, wts, device=device))


def w_skew(var, wts, device=0):
    """utils.py:207-210."""
    s, c = moments(var, wts, device=device)
    return (c[0, 1] / s[0]) / (c[0, 0] / s[0]) ** 1.5


def w_kurtosis(var, wts, device=0):
    """utils.py:212-215."""
    s, c = moments(var, wts, device=device)
    return (c[0, 2] / s[0]) / (c[0, 0] / s[0]) ** 2


def covariance(X, Y, weights, device=0):
    """utils.py:222-227."""
    s, c = moments(np.stack([_f64(X), _f64(Y)]), weights, device=device)
    return c[0, 1] / s[0]


def hist(x, W, lo, hi, bins, y=None, ylo=0.0, yhi=1.0, ybins=1, device=0):
    """Weighted counts (W None: plain counts) in `bins` equal bins of [lo, hi] (numpy.histogram's edge rules);
    with y, a (bins, ybins) array like numpy.histogram2d."""
    x = _f64(x)
    S = x.size
    yy = None if y is None else _f64(y)
    ww = None if W is None else _f64(W)
    if (yy is not None and yy.shape != x.shape) or (ww is not None and ww.shape != x.shape):
        raise ValueError("x, y and W must have the same length")
    out = np.zeros((int(bins), int(ybins)) if yy is not None else (int(bins),))
    _abi.check(_abi.lib().trpl_posterior_hist(_abi.ptr(x), _abi.ptr(yy), _abi.ptr(ww), S, float(lo), float(hi), int(bins),
                                              float(ylo), float(yhi), int(ybins), _abi.ptr(out), int(device), None))
    return out


def bin_edges(lo, hi, bins):
    """utils.py:243-244."""
    return lo + (hi - lo) * np.arange(int(bins) + 1) / int(bins)


def marginalize_1D(P, axis_overrides, bin_count, SECONDARY_PARAMS, param, X, device=0):
    """utils.py:239-262, same arguments: (density, edges); secondary parameters and mobilities are corrected
    for non-uniform sampling (each bin divided by its sample count, then renormalised to unit area)."""
    minX, maxX = axis_overrides[param]
    bins = int(bin_count)
    e = bin_edges(minX, maxX, bins)
    raw = hist(X, P, minX, maxX, bins, device=device)
    marP = raw / (np.diff(e) * raw.sum())                                  # numpy's density=True
    if SECONDARY_PARAMS[param] or "mu" in param:
        cnt = hist(X, None, minX, maxX, bins, device=device)
        corr = np.zeros_like(marP)
        nz = cnt != 0
        corr[nz] = marP[nz] / cnt[nz]
        marP = corr / np.sum(np.diff(e) * corr)
    return marP, e


def marginalize_2D(P, axis_overrides, bin_count, SECONDARY_PARAMS, param_names, X, Y, device=0):
    """utils.py:264-285, same arguments and return value (density[x bin][y bin], X_corr, Y_corr)."""
    px, py = param_names
    (minX, maxX), (minY, maxY) = axis_overrides[px], axis_overrides[py]
    bins = int(bin_count)
    ex, ey = bin_edges(minX, maxX, bins), bin_edges(minY, maxY, bins)
    raw = hist(X, P, minX, maxX, bins, y=Y, ylo=minY, yhi=maxY, ybins=bins, device=device)
    dens = raw / (np.outer(np.diff(ex), np.diff(ey)) * raw.sum())
    Y_corr, X_corr = np.meshgrid(ex, ey)                                   # :282, as the reference names them
    return dens, X_corr, Y_corr


def credible_interval(X, P):
    """utils.py:185-196 (host: one argsort, like the reference; trpl_amd.device.credible_interval_device
    does the same with torch.sort on the GPU)."""
    X = np.asarray(X)
    order = np.argsort(X)
    xs, cs = X[order], np.cumsum(np.asarray(P)[order])
    return xs[np.where(cs < 0.025)[0][-1]], xs[np.where(cs > 0.975)[0][0]]


def quantiles(V, W, q, rule=None, device=0, info=None, flags=0):
    """Weighted quantiles of the columns V (D, S) under the weights W (S,) in one device call (trpl_weighted_quantiles,
    include/trpl.h): returns (K, D) for K requests q in (0, 1).  rule: one of _abi.Q_LAST_BELOW (the largest value whose
    cumulative weight is < q sum W; NaN if there is none) / _abi.Q_FIRST_ABOVE (the smallest whose cumulative weight is
    > q sum W) per request; None takes LAST_BELOW for q < 0.5 and FIRST_ABOVE otherwise.  A sample counts iff its weight is
    finite and > 0; a NaN value among those makes that column's quantiles NaN."""
    from .device import quantile_requests
    V = _f64(V)
    W = _f64(W)
    if V.ndim == 1:
        V = V[None, :]
    if V.ndim != 2 or W.shape != (V.shape[1],):
        raise ValueError("V must be (D, S) and W (S,)")
    q, rule = quantile_requests(q, rule)
    D, S = V.shape
    out = np.empty((q.size, D))
    sec = _abi.C.c_double(0.0)
    _abi.check(_abi.lib().trpl_weighted_quantiles(_abi.ptr(V), D, S, S, _abi.ptr(W), _abi.ptr(q), _abi.ptr(rule), q.size, int(flags),
                                                  _abi.ptr(out), int(device), _abi.C.byref(sec)))
    if info is not None:
        info.update(seconds=sec.value)
    return out


def credible_intervals(columns, P, lo=0.025, hi=0.975, device=0):
    """credible_interval (utils.py:185-196) of every column in ONE device call: `columns` maps a name to its (S,) values, P
    are the weights.  Returns dict name -> (low, high): the last value whose cumulative weight is below lo * sum P and the
    first whose cumulative weight is above hi * sum P (low is NaN where the reference raises IndexError)."""
    names = list(columns)
    V = np.stack([_f64(columns[k]) for k in names])
    r = quantiles(V, P, [lo, hi], [_abi.Q_LAST_BELOW, _abi.Q_FIRST_ABOVE], device=device)
    return {k: (float(r[0, i]), float(r[1, i])) for i, k in enumerate(names)}


def summarize(columns, P, device=0):
    """stats_summarize + calc_covariance (utils.py:117-143) in one device pass: `columns` maps a name to its
    (S,) values.  Returns dict(names, mean, variance, sample_std, skew, kurtosis, covariance (D, D), w2)."""
    names = list(columns)
    V = np.stack([_f64(columns[k]) for k in names])
    s, c = moments(V, P, device=device)
    D = len(names)
    mean = s[2:] / s[0]
    cov = c[:, :D] / s[0]
    var = np.diag(cov).copy()
    return {"names": names, "mean": mean, "variance": var, "sample_std": np.sqrt(s[1] * var),
            "skew": (c[:, D] / s[0]) / var ** 1.5, "kurtosis": (c[:, D + 1] / s[0]) / var ** 2,
            "covariance": cov, "w2": s[1]}


# ---- choosing the temperature factor (utils.py:128-133, 168-183) on the device: trpl_posterior_tf_scan ----
TF_SCAN_POINTS = _abi.TF_SCAN_MAX          # temperatures per scan of the bracketed search


def tf_scan(LL, tfs, V=None, device=0, log_ratio=None):
    """The posterior at every temperature of `tfs` (at most TF_SCAN_MAX) from one scan of the samples.

    Returns dict(stats (K, 4) = [nanmax(LL / tf), raw normalising sum, sum W^2, count of non-NaN LL], mean (K, D),
    var (K, D), Q (K, D) = sqrt(sum W^2 * var), the objective of tf_driver), row k being bit for bit what
    weights(LL, tfs[k]) followed by moments(V, W) gives.  V is (D, S) or (S,); None: stats only (D = 0).

    log_ratio (S,): ln r(u) of a refined set, kept beside LL (trpl_posterior_tf_scan_lr).  Row k is then the bits of
    weights(LL, tfs[k], log_ratio=log_ratio) followed by moments(V, W), stats is (K, 6) = [max of LL / tf - log_ratio, raw
    normalising sum, sum W, sum W^2, count of samples with neither NaN, ess] and "ess" = stats[:, 5] = (sum W)^2 / sum W^2,
    the effective sample size at each temperature (NaN where a weight is NaN)."""
    LL = _f64(LL)
    tfs = np.atleast_1d(_f64(tfs))
    if LL.ndim != 1 or tfs.ndim != 1:
        raise ValueError("LL and tfs must be one-dimensional")
    if V is None:
        V = np.empty((0, LL.size))
    V = _f64(V)
    if V.ndim == 1:
        V = V[None, :]
    D, S = V.shape
    if S != LL.size:
        raise ValueError("V must have one column entry per sample")
    K = tfs.size
    out = {"stats": np.zeros((K, 4 if log_ratio is None else 6)), "mean": np.zeros((K, D)), "var": np.zeros((K, D)),
           "Q": np.zeros((K, D))}
    if log_ratio is None:
        _abi.check(_abi.lib().trpl_posterior_tf_scan(_abi.ptr(LL), S, _abi.ptr(V) if D else None, D, _abi.ptr(tfs), K,
                                                     _abi.ptr(out["stats"]), _abi.ptr(out["mean"]), _abi.ptr(out["var"]),
                                                     _abi.ptr(out["Q"]), int(device), None))
        return out
    lnr = _log_ratio(log_ratio, S)
    _abi.check(_abi.lib().trpl_posterior_tf_scan_lr(_abi.ptr(LL), _abi.ptr(lnr), S, _abi.ptr(V) if D else None, D, _abi.ptr(tfs),
                                                    K, _abi.ptr(out["stats"]), _abi.ptr(out["mean"]), _abi.ptr(out["var"]),
                                                    _abi.ptr(out["Q"]), int(device), None))
    out["ess"] = out["stats"][:, 5].copy()
    return out


def _bracket_search(objective, lo, hi, k, rtol):
    """Deterministic bracketed maximisation over ln tf, for C independent brackets at once.

    objective(tfs) takes a (k, C) array of temperatures (column c is bracket c's grid) and returns the (k, C) values.
    Every round lays k points, equally spaced in ln tf and including both ends, over each bracket [lo_c, hi_c], takes
    the FIRST largest value of each column (ties resolve to the lowest index) and shrinks that bracket to the two
    neighbours of that point (an end point keeps itself as that side).  A column is finished, and from then on frozen,
    once hi / lo - 1 <= rtol: its result does not depend on the other columns.  k >= 4.

    Rounds: a round multiplies ln(hi / lo) by 2 / (k - 1), so a column takes
        rounds = max(1, ceil(ln(ln(hi / lo) / ln(1 + rtol)) / ln((k - 1) / 2)))
    objective calls and rounds * k temperatures -- fewer only where a round's maximum is an end point of its grid (that
    round shrinks the bracket by 1 / (k - 1)).

    Returns (tf (C,), value (C,), info): info = dict(scans (rounds run), rounds (C,) per column, lo, hi (C,) the final
    brackets, at_edge (C,) bool: the maximum of the FIRST round was an end point of the outer bracket, so the maximiser
    may lie outside it)."""
    lo = np.atleast_1d(np.asarray(lo, dtype=np.float64)).copy()
    hi = np.atleast_1d(np.asarray(hi, dtype=np.float64)).copy()
    if lo.shape != hi.shape or lo.ndim != 1 or not (np.all(lo > 0) and np.all(hi > lo) and np.all(np.isfinite(hi))):
        raise ValueError("brackets need 0 < lo < hi < inf, one pair per column")
    if k < 4 or not rtol > 0:
        raise ValueError("k must be >= 4 and rtol > 0")
    C = lo.size
    frac = (np.arange(k) / (k - 1))[:, None]
    at_edge = np.zeros(C, dtype=bool)
    tf, val = np.full(C, np.nan), np.full(C, np.nan)
    rounds = np.zeros(C, dtype=np.int64)
    live = np.ones(C, dtype=bool)
    scans = 0
    while live.any():
        llo, lhi = np.log(lo), np.log(hi)
        tfs = np.exp(llo + (lhi - llo) * frac)
        tfs[0], tfs[-1] = lo, hi                                     # the ends exactly: a grid never leaves its bracket
        q = np.asarray(objective(tfs), dtype=np.float64).reshape(k, C)
        scans += 1
        best = np.argmax(np.where(np.isnan(q), -np.inf, q), axis=0)  # the first maximum of each column
        if scans == 1:
            at_edge = (best == 0) | (best == k - 1)
        c = np.flatnonzero(live)
        tf[c], val[c] = tfs[best[c], c], q[best[c], c]
        lo[c], hi[c] = tfs[np.maximum(best[c] - 1, 0), c], tfs[np.minimum(best[c] + 1, k - 1), c]
        rounds[c] += 1
        live &= ~(hi / lo - 1.0 <= rtol)
    return tf, val, {"scans": scans, "rounds": rounds, "lo": lo, "hi": hi, "at_edge": at_edge}


def _find_best_tf_columns(V, LL, u0, device, span, rtol, log_ratio=None):
    """find_best_tf of every row of V (D, S): (tf (D,), Q (D,), info of _bracket_search + device_scans)."""
    V, LL = _f64(V), _f64(LL)
    D = V.shape[0]
    device_scans = [0]

    def objective(tfs):                              # (k, D) -> Q (k, D): column d's temperatures matter for Q[:, d] only
        uniq, inv = np.unique(tfs, return_inverse=True)
        inv = inv.reshape(tfs.shape)
        Q = np.empty((uniq.size, D))
        for a in range(0, uniq.size, _abi.TF_SCAN_MAX):          # one device scan serves all D columns
            Q[a:a + _abi.TF_SCAN_MAX] = tf_scan(LL, uniq[a:a + _abi.TF_SCAN_MAX], V, device=device, log_ratio=log_ratio)["Q"]
            device_scans[0] += 1
        return Q[inv, np.arange(D)[None, :]]

    u0, span = float(u0), float(span)
    if not (u0 > 0 and span > 1):
        raise ValueError("u0 must be > 0 and span > 1")
    tf, q, info = _bracket_search(objective, np.full(D, u0 / span), np.full(D, u0 * span), TF_SCAN_POINTS, rtol)
    info["device_scans"] = device_scans[0]
    return tf, q, info


def find_best_tf(xi, P, u0, device=0, span=1e4, rtol=1e-6, info=None, log_ratio=None):
    """utils.py:181-183, same positional arguments (xi the parameter's values, P the log-likelihoods, u0 the starting
    temperature) and return value (tf, Q) with Q = -tf_driver(ln tf, xi, P) = sqrt(sum W^2 * weighted variance),
    W = normalize(P / tf).  Instead of fmin from ln u0: the deterministic search of _bracket_search over
    [u0 / span, u0 * span] with TF_SCAN_POINTS temperatures per device scan (tf_scan), until the bracket's relative width
    is at most rtol.  info receives scans, lo, hi (the final bracket) and at_edge: True when the largest Q of the first
    scan sat on an end of the outer bracket (the returned tf is then the best of that side, not a located maximum).
    log_ratio (S,): over a refined set, ln r(u) beside the log-likelihoods P; W is then tf_scan's with that ratio."""
    xi = _f64(xi)
    if xi.ndim != 1:
        raise ValueError("xi must be one-dimensional")
    tf, q, inf = _find_best_tf_columns(xi[None, :], P, u0, device, span, rtol, log_ratio)
    if info is not None:
        info.update(scans=inf["scans"], device_scans=inf["device_scans"], lo=float(inf["lo"][0]), hi=float(inf["hi"][0]),
                    at_edge=bool(inf["at_edge"][0]))
    return float(tf[0]), float(q[0])


def calc_max_uncertainty(columns, LL, num_observations, device=0, span=1e4, rtol=1e-6, info=None, log_ratio=None):
    """LikelihoodData.calc_max_uncertainty (utils.py:128-133): dict param -> (tf, Q) = find_best_tf(columns[param], LL,
    num_observations / 2000), bit for bit.  The columns share the rounds and the device scans: the first round is one scan
    for all of them (the same outer bracket), a later round scans its distinct temperatures once for all D columns
    (each column keeps its own bracket, so that is up to one scan per distinct bracket).  info receives scans (rounds: those
    of a single find_best_tf), device_scans, and per-parameter dicts lo, hi, at_edge.  log_ratio: as in find_best_tf."""
    names = list(columns)
    V = np.stack([_f64(columns[k]) for k in names])
    tf, q, inf = _find_best_tf_columns(V, LL, float(num_observations) / 2000.0, device, span, rtol, log_ratio)
    if info is not None:
        info.update(scans=inf["scans"], device_scans=inf["device_scans"], lo=dict(zip(names, inf["lo"].tolist())),
                    hi=dict(zip(names, inf["hi"].tolist())), at_edge=dict(zip(names, inf["at_edge"].tolist())))
    return {n: (float(tf[i]), float(q[i])) for i, n in enumerate(names)}


def _ess_search(objective, target, lo, hi, k, rtol):
    """Deterministic search on a grid for the smallest temperature whose effective sample size reaches `target`.

    objective(tfs) takes a (k,) array of temperatures and returns their (k,) effective sample sizes.  Every round lays k points,
    equally spaced in ln tf and including both ends, over [lo, hi] and takes the SMALLEST grid temperature whose value is
    >= target (a NaN never is).  The effective sample size need not be monotone in tf when the proposal ratio varies, so the
    rule is stated on the grid and not as a root: of several crossings the lowest one the grid sees is followed.  The new
    bracket is that point and its lower neighbour; rounds repeat until hi / lo - 1 <= rtol.  A round divides ln(hi / lo) by
    k - 1, so rounds = max(1, ceil(ln(ln(hi / lo) / ln(1 + rtol)) / ln(k - 1))).  k >= 4.

    Returns (tf, ess, info): tf is the upper end of the final bracket, a grid point whose value reached the target; info =
    dict(scans, lo, hi, at_edge).  at_edge is "hi" when no point of the first grid reaches the target (hi and its value are
    returned: the target was not met), "lo" when the lowest point already does (lo is returned), None otherwise."""
    lo, hi, target = float(lo), float(hi), float(target)
    if not (0 < lo < hi < np.inf):
        raise ValueError("the bracket needs 0 < lo < hi < inf")
    if k < 4 or not rtol > 0:
        raise ValueError("k must be >= 4 and rtol > 0")
    if not target > 0:
        raise ValueError("target must be > 0")
    frac = np.arange(k) / (k - 1)
    scans = 0
    while True:
        llo, lhi = np.log(lo), np.log(hi)
        tfs = np.exp(llo + (lhi - llo) * frac)
        tfs[0], tfs[-1] = lo, hi                                     # the ends exactly: a grid never leaves its bracket
        ess = np.asarray(objective(tfs), dtype=np.float64).reshape(k)
        scans += 1
        reached = ess >= target
        i = int(np.argmax(reached)) if reached.any() else k - 1     # the first point that reaches the target
        if scans == 1 and not reached.any():
            return hi, float(ess[-1]), {"scans": scans, "lo": lo, "hi": hi, "at_edge": "hi"}
        if scans == 1 and i == 0:
            return lo, float(ess[0]), {"scans": scans, "lo": lo, "hi": hi, "at_edge": "lo"}
        tf, val = float(tfs[i]), float(ess[i])
        if i > 0:                                                    # (i == 0 after the first round: only a non-deterministic objective)
            lo = float(tfs[i - 1])
        hi = tf
        if i == 0 or hi / lo - 1.0 <= rtol:
            return tf, val, {"scans": scans, "lo": lo, "hi": hi, "at_edge": None}


def tf_for_ess(LL, target, log_ratio=None, lo=1.0, hi=1e4, rtol=1e-6, device=0, info=None):
    """(tf, ess): the smallest temperature of the grid search _ess_search over [lo, hi] at which the weights of
    exp(LL / tf - log_ratio) have an effective sample size (sum W)^2 / sum W^2 of at least `target`, and that size;
    TF_SCAN_POINTS temperatures per device scan (tf_scan(..., log_ratio=)["ess"]; log_ratio None: zeros, the unrefined set).
    What building a proposal at a raised temperature needs (refine.run(target_ess=)).  A NaN in LL or log_ratio makes every
    effective sample size NaN: drop such samples first (filter_nan) or give them LL = -inf.  info receives scans, lo, hi (the
    final bracket) and at_edge: "hi" -- no temperature of the first grid reaches the target, hi and its ess are returned;
    "lo" -- lo already does; None otherwise."""
    LL = _f64(LL)
    if LL.ndim != 1:
        raise ValueError("LL must be one-dimensional")
    lnr = np.zeros(LL.size) if log_ratio is None else _log_ratio(log_ratio, LL.size)
    tf, ess, inf = _ess_search(lambda tfs: tf_scan(LL, tfs, device=device, log_ratio=lnr)["ess"], target, lo, hi,
                               TF_SCAN_POINTS, rtol)
    if info is not None:
        info.update(inf)
    return tf, ess


def log_evidence(LL, tf, log_ratio=None, device=0):
    """(ln_z, info): the log of the marginal likelihood Z(tf) = integral of exp(LL(u) / tf) p(u) du from an importance run: the log of
    the mean over the samples with no NaN of exp(LL / tf - log_ratio).  LL (S,) of draws from the prior box (log_ratio None), or of a
    refined set with its Population.log_ratio(); with an informative prior p on uniform draws, log_ratio = -ln p(u).  tf a scalar, or
    an array of at most TF_SCAN_MAX temperatures, which gives arrays back.

    Formed from ONE tf_scan call: its raw normalising sum is the sum of exp(((e - max e) + 1000 ln 2) - ln S), e = LL / tf - log_ratio,
    so ln_z = max e - 1000 ln 2 + ln S + ln(raw sum) - ln N with N the count of samples with no NaN.  info: ess, the effective sample
    size (sum W)^2 / sum W^2 of the weights; se = sqrt(1 / ess - 1 / N), the standard error of ln_z (the relative error of the mean);
    count = N.  A NaN sample is left out of ln_z and of N but makes ess and se NaN, as it does in tf_scan: drop such samples first
    (filter_nan) where the error is wanted.  The estimate is trustworthy where ess is large -- at the temperature tf_for_ess puts the hottest rung of a ladder,
    from which mcmc.Tempered.log_evidence bridges down to the temperature wanted."""
    import math
    LL = _f64(LL)
    scalar = np.ndim(tf) == 0
    tfs = np.atleast_1d(_f64(tf))
    if LL.ndim != 1 or LL.size < 1:
        raise ValueError("LL must be one-dimensional and not empty")
    if tfs.ndim != 1 or not 1 <= tfs.size <= TF_SCAN_POINTS:
        raise ValueError("tf must be a scalar or (K,), 1 <= K <= %d temperatures" % TF_SCAN_POINTS)
    st = tf_scan(LL, tfs, device=device, log_ratio=log_ratio)["stats"]
    with np.errstate(divide="ignore", invalid="ignore"):
        if log_ratio is None:
            top, raw, count, ess = st[:, 0], st[:, 1], st[:, 3], 1.0 / st[:, 2]
        else:
            top, raw, count, ess = st[:, 0], st[:, 1], st[:, 4], st[:, 5]
        ln_z = top - 1000.0 * math.log(2.0) + math.log(LL.size) + np.log(raw) - np.log(count)
        se = np.sqrt(np.maximum(1.0 / ess - 1.0 / count, 0.0))
    if scalar:
        return float(ln_z[0]), dict(ess=float(ess[0]), se=float(se[0]), count=float(count[0]))
    return ln_z, dict(ess=ess.copy(), se=se, count=count.copy())


# ---- the corner: every marginal of a finished run in one device call (trpl_corner, csrc/corner.hip) ----
# the 13 columns of the exported X under the package's names (sampler.PARAM_NAMES; marginalization_visual.py:67-70 lists them
# in this order) and the six secondary parameters of the same list, :69-70; the position is the TRPL_COL_* code
CORNER_COLUMNS = ("n0", "p0", "mun", "mup", "B", "Sf", "Sb", "CN", "CP", "taun", "taup", "lambda", "mag_offset",
                  "tau_eff", "tau_rad", "Sf+Sb", "mu'", "epsilon", "taun+taup")


def _corner_codes(enabled, do_log):
    enabled = list(enabled)
    unknown = [n for n in list(enabled) + list(do_log) if n not in CORNER_COLUMNS]
    if unknown:
        raise ValueError("unknown column name(s) %r: CORNER_COLUMNS lists the names" % (unknown,))
    if len(set(enabled)) != len(enabled):
        raise ValueError("a column is enabled twice")
    cols = np.array([CORNER_COLUMNS.index(n) for n in enabled], dtype=np.int32)
    lg = np.array([1 if n in do_log else 0 for n in enabled], dtype=np.int32)
    return enabled, cols, lg


def _exclusion(exclude_limits):
    """name -> (lo, hi) on the RAW values of primary columns -> the two host arrays of trpl_corner_columns_dev (NaN: not tested)."""
    if exclude_limits is None:
        return None, None
    lo, hi = np.full(_abi.CORNER_PRIMARY, np.nan), np.full(_abi.CORNER_PRIMARY, np.nan)
    for name, (a, b) in exclude_limits.items():
        c = CORNER_COLUMNS.index(name) if name in CORNER_COLUMNS else _abi.CORNER_MAX_COLS
        if c >= _abi.CORNER_PRIMARY:
            raise ValueError("exclusion limits apply to the 13 primary columns, not to %r" % (name,))
        if a != a or b != b:
            raise ValueError("exclusion limits of %r must not be NaN" % (name,))
        lo[c], hi[c] = a, b
    return lo, hi


def columns(X, enabled, thickness=2000.0, do_log=(), exclude_limits=None, LL=None, device=0):
    """The plotted columns of a finished run, formed on the device: X (S, 13) in the user's units (*_BAYRAN_X.npy), `enabled` a
    sequence of CORNER_COLUMNS names -- primary columns and the secondary parameters of secondary_parameters.py -- log10 taken of
    those in do_log.  Returns V (D, S), the layout moments, quantiles, tf_scan, summarize, credible_intervals and
    calc_max_uncertainty take.  With LL, returns (V, LLk, kept): LLk is LL with NaN at the samples outside exclude_limits
    (name -> (lo, hi) on the raw values of primary columns, utils.py:145-155), kept the number of samples left by filter_nan and
    the exclusion together; weights(LLk, tf) then normalises over the kept samples only.
    Cost: this is the host-buffer call trpl_corner with one bin per axis, so besides the columns kernel it uploads X, runs the
    weights on a flat likelihood (their NaNs are LLk's) and D one-bin histograms that each walk the S samples, and copies V back;
    the upload and the copy dominate.  Tensors already on the device go through device.corner_columns_device, which runs
    the columns kernel alone."""
    X = _f64(X)
    if X.ndim != 2 or X.shape[1] < _abi.CORNER_PRIMARY:
        raise ValueError("X must be (S, 13)")
    enabled, cols, lg = _corner_codes(enabled, do_log)
    S, D = X.shape[0], cols.size
    if LL is None:
        if exclude_limits is not None:
            raise ValueError("exclude_limits needs LL: the exclusion is returned as NaN in LLk")
        LL_in = np.zeros(S)
    else:
        LL_in = _f64(LL)
        if LL_in.shape != (S,):
            raise ValueError("LL must have one entry per sample")
    lo, hi = _exclusion(exclude_limits)
    # the columns alone: trpl_corner with one bin per axis over [0, 1] (its histograms are ignored)
    V, W = np.empty((D, S)), np.empty(S)
    kept = np.zeros(1, dtype=np.int64)
    h1, alo, ahi = np.zeros((D, 1)), np.zeros(D), np.ones(D)
    flat = np.where(np.isnan(LL_in), np.nan, 0.0)                # equal likelihoods: every kept sample gets a finite weight
    _abi.check(_abi.lib().trpl_corner(_abi.ptr(X), S, X.shape[1], _abi.ptr(flat), 1.0, _abi.ptr(cols), _abi.ptr(lg), D, float(thickness),
                                      _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(alo), _abi.ptr(ahi), 1, _abi.ptr(V), _abi.ptr(W),
                                      _abi.ptr(kept), _abi.ptr(h1), None, None, int(device), None))
    if LL is None:
        return V
    LLk = np.where(np.isnan(W), np.nan, LL_in)                   # W is NaN exactly where LLk is
    return V, LLk, int(kept[0])


def corner(X, LL, enabled, axis_limits, bin_count=96, tf=1.0, thickness=2000.0, do_log=(), exclude=False, secondary=None, device=0,
           info=None):
    """plot() of marginalization_visual.py:500-609 up to the drawing, in one device call (trpl_corner): exclusion by the axis
    limits, secondary parameters, log10, tempered weights, and the 1-D marginal of every enabled column and the 2-D marginal of
    every pair, each bin summed in ascending sample order (the same bits in every run).

    X (S, 13) in the user's units, LL (S,) log-likelihoods (NaN: dropped, like filter_nan), enabled: CORNER_COLUMNS names in
    plotting order, axis_limits: name -> (lo, hi) in PLOTTED units, i.e. after log10 for the names in do_log, as marginalize_1D /
    marginalize_2D receive them from loglimits() (plotutils.py:56-59).  exclude=True drops the samples outside the limits of the
    enabled PRIMARY columns, compared on the raw values as the reference does (utils.py:48-52): fromTK_get_axis_limits
    (plotutils.py:19-23) holds the raw limits and loglimits() (plotutils.py:56-59) turns them into log10 afterwards, so a
    log-scaled column's raw limits are 10 ** limit here.  secondary: name -> bool, which columns get the correction for
    non-uniform sampling besides the names containing "mu" (default: the six secondary parameters, SECONDARY_PARAMS :72-75).
    Returns {"h_1D": {name: (density, edges)}, "h_2D": {(px, py): (density, X_corr, Y_corr)}, "W", "kept", "V"} with the
    densities formed on the host from the raw sums by the arithmetic of marginalize_1D / marginalize_2D above."""
    X, LL = _f64(X), _f64(LL)
    if X.ndim != 2 or X.shape[1] < _abi.CORNER_PRIMARY or LL.shape != (X.shape[0],):
        raise ValueError("X must be (S, 13) and LL (S,)")
    enabled, cols, lg = _corner_codes(enabled, do_log)
    S, D, bins = X.shape[0], cols.size, int(bin_count)
    if secondary is None:
        secondary = {n: CORNER_COLUMNS.index(n) >= _abi.CORNER_PRIMARY for n in enabled}
    lo = np.array([axis_limits[n][0] for n in enabled], dtype=np.float64)
    hi = np.array([axis_limits[n][1] for n in enabled], dtype=np.float64)
    excl = None
    if exclude:
        excl = {n: (10.0 ** lo[d], 10.0 ** hi[d]) if lg[d] else (lo[d], hi[d])
                for d, n in enumerate(enabled) if cols[d] < _abi.CORNER_PRIMARY}
    elo, ehi = _exclusion(excl)
    if not 1 <= bins <= _abi.CORNER_MAX_BINS:
        raise ValueError("bin_count must be in [1, %d]" % _abi.CORNER_MAX_BINS)
    npair = D * (D - 1) // 2
    V, W = np.empty((D, S)), np.empty(S)
    kept = np.zeros(1, dtype=np.int64)
    h1, c1, h2 = np.zeros((D, bins)), np.zeros((D, bins)), np.zeros((npair, bins, bins))
    sec = _abi.C.c_double(0.0)
    _abi.check(_abi.lib().trpl_corner(_abi.ptr(X), S, X.shape[1], _abi.ptr(LL), float(tf), _abi.ptr(cols), _abi.ptr(lg), D,
                                      float(thickness), _abi.ptr(elo), _abi.ptr(ehi), _abi.ptr(lo), _abi.ptr(hi), bins, _abi.ptr(V),
                                      _abi.ptr(W), _abi.ptr(kept), _abi.ptr(h1), _abi.ptr(c1), _abi.ptr(h2) if npair else None,
                                      int(device), _abi.C.byref(sec)))
    if info is not None:
        info.update(seconds=sec.value, h1=h1, c1=c1, h2=h2)
    edges = [bin_edges(lo[d], hi[d], bins) for d in range(D)]
    h_1D, h_2D = {}, {}
    for d, n in enumerate(enabled):
        e, raw = edges[d], h1[d]
        marP = raw / (np.diff(e) * raw.sum())                              # numpy's density=True, as in marginalize_1D
        if secondary.get(n, False) or "mu" in n:
            corr = np.zeros_like(marP)
            nz = c1[d] != 0
            corr[nz] = marP[nz] / c1[d][nz]
            marP = corr / np.sum(np.diff(e) * corr)
        h_1D[n] = (marP, e)
    p = 0
    for i in range(1, D):                                                  # utils.py:103-106
        for j in range(i):
            raw = h2[p]
            dens = raw / (np.outer(np.diff(edges[j]), np.diff(edges[i])) * raw.sum())
            Y_corr, X_corr = np.meshgrid(edges[j], edges[i])               # :282, as the reference names them
            h_2D[(enabled[j], enabled[i])] = (dens, X_corr, Y_corr)
            p += 1
    return {"h_1D": h_1D, "h_2D": h_2D, "W": W, "kept": int(kept[0]), "V": V}
