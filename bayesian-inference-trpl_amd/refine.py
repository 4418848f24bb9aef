"""Refinement generations: a second (third, ...) generation of samples drawn around the posterior of the first, weighted so that
the union of all generations is an exact sample of the same posterior (trpl_refine_*, include/trpl.h; csrc/refine.hip).

The reference's ancestor refined the grid cells above minP (Legacy/legacy.py:refineGrid, Legacy/parallel_bayes.py:bayes); the
random sampler that replaced it draws the box once.  Here generation 1 is that uniform draw (bayeslib.random_grid), every further
generation is n_uniform uniform children plus m children in a box around each of K parents resampled from the posterior so far,
and every sample of every generation is weighted by the deterministic mixture of all proposals:

    r(u) = (S1 + sum_g [n_uniform_g + m_g B_g(u)]) / S_total,    B_g(u) = sum_k inv_vol_k 1[a_k <= u <= b_k],
    LLc = LL - tf ln r(u)

so that posterior.weights / moments / quantiles / corner and posterior_predictive work unchanged on the concatenated (X, LLc).
LLc is valid at the tf it was formed for only.  What depends on the temperature keeps ln r(u) beside LL instead:
Population.log_ratio() returns (X, LL, ln r), and posterior.weights / tf_scan / find_best_tf / calc_max_uncertainty / tf_for_ess
take it as log_ratio= (trpl_posterior_weights_lr, trpl_posterior_tf_scan_lr), so a temperature scan over a refined set is supported.
run(target_ess=) uses it to build each generation's proposal at the lowest temperature whose effective sample size reaches a
target, and comes down to the caller's tf as the union grows.

All sampling happens in unit coordinates of the ACTIVE columns (minX != maxX and not the target of an equal-mu / equal-S /
equal-Auger override); resampling, the draw, the mixture density and the unit map run on the device.  No CPU fallback.

The effective sample size these functions report is a diagnostic, not a guarantee: when the first generation's is of order 1, one
round under-covers the posterior; use several rounds and keep a uniform share.

Oriented proposals (oriented=True): a generation's boxes are axis-parallel in z = M (u - c), M the inverse
Cholesky factor of the population's shrunk weighted covariance (orientation, affine; trpl_refine_affine, trpl_refine_draw_oriented),
so that they follow a ridge of the posterior that lies across the axes.  The density is the same call on the transformed points;
a child that leaves the cube is kept with LL = -inf, which keeps r(u) exact.

This module takes and returns numpy arrays and goes through the host-buffer calls, like `posterior`: the likelihood it drives is any
callable on a host X, and the generations are kept on the host between its calls.  What it saves instead is the repetition: a
Population keeps every sample's mixture numerator and evaluates each (generation, proposal) pair's density once, and `run` forms the
union's weights once per round and reads the effective sample size off the resampling's own sums.  A pipeline whose samples stay on
the device composes the same steps from device.refine_resample_device / refine_draw_device / refine_density_device /
refine_unit_device."""
import collections

import numpy as np

from . import _abi, posterior
from .sampler import box_flags

# orient: None for axis-parallel boxes in u; for an oriented proposal the dict of orientation() plus zc (K, A), the parents in
# z = M (u - c) -- a, b, inv_vol are then the boxes in z
Proposal = collections.namedtuple("Proposal", "a b inv_vol K m n_uniform seed generation orient", defaults=(None,))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _box(minX, maxX, do_log):
    lo, hi = _f64(minX), _f64(maxX)
    lg = np.ascontiguousarray(do_log, dtype=np.int32)
    if not (lo.shape == hi.shape == lg.shape and lo.ndim == 1):
        raise ValueError("minX, maxX and do_log must be one-dimensional and of equal length")
    return lo, hi, lg


def active_columns(minX, maxX, sim_flags=None):
    """The columns a refinement samples: minX != maxX and not the target (2, 6, 8) of an override that is set."""
    lo, hi = _f64(minX), _f64(maxX)
    f = box_flags(sim_flags)
    target = {c for bit, c in ((1, 2), (2, 6), (4, 8)) if f & bit and (c != 2 or lo.size > 3)}
    return np.array([c for c in range(lo.size) if lo[c] != hi[c] and c not in target], dtype=np.int64)


def resample(W, K, offset=0.5, device=0):
    """Systematic resampling (trpl_refine_resample): idx (K,) int64, non-decreasing -- idx[k] is the smallest i whose cumulative
    weight exceeds (k + offset) / K of the total; a NaN or non-positive weight counts as 0.  Returns (idx, info) with info =
    dict(sum, sum_sq, ess, seconds).  ValueError when no weight is left."""
    W = _f64(W)
    if W.ndim != 1:
        raise ValueError("W must be one-dimensional")
    idx = np.empty(int(K), dtype=np.int64)
    stats = np.zeros(3)
    sec = _abi.C.c_double(0.0)
    _abi.check(_abi.lib().trpl_refine_resample(_abi.ptr(W), W.size, int(K), float(offset), _abi.ptr(idx), _abi.ptr(stats), int(device),
                                               _abi.C.byref(sec)))
    if not stats[0] > 0:
        raise ValueError("no sample has a positive weight: nothing to resample")
    return idx, {"sum": stats[0], "sum_sq": stats[1], "ess": stats[2], "seconds": sec.value}


def unit_coords(X, minX, maxX, do_log, sim_flags=None, device=0):
    """(U, active): the unit coordinates (S, A) of the active columns of X (S, ncol) -- (x - lo) / (hi - lo), or the same in log10
    for a log column -- and the indices of those columns (trpl_refine_unit; the device's log10)."""
    X = _f64(X)
    lo, hi, lg = _box(minX, maxX, do_log)
    if X.ndim != 2 or X.shape[1] < lo.size:
        raise ValueError("X must be (S, ncol)")
    act = active_columns(lo, hi, sim_flags)
    if not 1 <= act.size <= _abi.REFINE_MAX_DIMS:
        raise ValueError("the box has %d active columns; a refinement takes 1 .. %d" % (act.size, _abi.REFINE_MAX_DIMS))
    U = np.empty((X.shape[0], act.size))
    _abi.check(_abi.lib().trpl_refine_unit(_abi.ptr(X), X.shape[0], X.shape[1], lo.size, _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg),
                                           box_flags(sim_flags), act.size, _abi.ptr(U), int(device), None))
    return U, act


def bandwidth(U, W, S1, device=0):
    """Default half-widths h (A,): clip(max(sqrt 3 sd_d ESS^(-1 / (A + 4)), S1^(-1 / A) / 2), 0, 1 / 2) -- a box of the width of a
    uniform kernel with the posterior's deviation sd_d (posterior.moments on U), shrunk by the usual ESS^(-1 / (A + 4)), and never
    below about half the first generation's mean spacing, so that a collapsed posterior still gets a box."""
    U = _f64(U)
    W = np.where(np.asarray(W, dtype=np.float64) > 0, W, 0.0)
    A = U.shape[1]
    s, c = posterior.moments(np.ascontiguousarray(U.T), W, device=device)
    sd = np.sqrt(np.maximum(np.diag(c[:, :A]) / s[0], 0.0))
    ess = s[0] * s[0] / s[1]
    return np.clip(np.maximum(np.sqrt(3.0) * sd * ess ** (-1.0 / (A + 4)), 0.5 * float(S1) ** (-1.0 / A)), 0.0, 0.5)


def boxes(c, h):
    """a, b (K, A), inv_vol (K,) of the parents c (K, A) with half-widths h: [max(0, c - h), min(1, c + h)], the volume's product
    in ascending d and one division."""
    c = _f64(c)
    h = np.broadcast_to(_f64(h), (c.shape[1],))
    if not (np.all(h > 0) and np.all(h <= 1)):
        raise ValueError("every half-width must lie in (0, 1]")
    a, b = np.maximum(0.0, c - h), np.minimum(1.0, c + h)
    vol = np.ones(c.shape[0])
    for d in range(c.shape[1]):
        vol = vol * (b[:, d] - a[:, d])
    return np.ascontiguousarray(a), np.ascontiguousarray(b), 1.0 / vol


def orientation(U, W, S1, shrink=None, device=0):
    """The whitening of one generation: dict(c, L, M, logdet, h, lam, ess).  c and Sigma are the weighted mean
    and covariance of U (S, A) under W (posterior.moments, on the device); Sigma_dd >= (S1^(-1 / A) / 2)^2 / 3; Sigma_s = (1 - lam)
    Sigma + lam diag(Sigma) with lam = clip((A + 1) / ESS, 0, 1) unless shrink is given; L = chol(Sigma_s) (host, A <= 16), M = L^-1,
    logdet = sum ln L_dd; h_d = sqrt(3) ESS^(-1 / (A + 4)) in z."""
    U = _f64(U)
    W = np.where(np.asarray(W, dtype=np.float64) > 0, W, 0.0)
    A = U.shape[1]
    s, cen = posterior.moments(np.ascontiguousarray(U.T), W, device=device)
    c = s[2:2 + A] / s[0]
    Sigma = np.array(cen[:, :A]) / s[0]
    Sigma = 0.5 * (Sigma + Sigma.T)
    ess = s[0] * s[0] / s[1]
    d = np.maximum(np.diag(Sigma), (0.5 * float(S1) ** (-1.0 / A)) ** 2 / 3.0)
    Sigma[np.arange(A), np.arange(A)] = d
    lam = float(np.clip((A + 1) / ess, 0.0, 1.0)) if shrink is None else float(shrink)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("shrink must lie in [0, 1]")
    try:
        L = np.linalg.cholesky((1.0 - lam) * Sigma + lam * np.diag(d))
    except np.linalg.LinAlgError:
        raise ValueError("the shrunk covariance is not positive definite: use a larger shrink") from None
    M = np.tril(np.linalg.inv(L))
    return {"c": c, "L": L, "M": M, "logdet": float(np.sum(np.log(np.diag(L)))), "h": np.full(A, np.sqrt(3.0) * ess ** (-1.0 / (A + 4))),
            "lam": lam, "ess": float(ess)}


def affine(U, M, c, device=0):
    """Z (S, A) = M (U - c), M lower triangular: z_i = sum_{j <= i} M_ij (u_j - c_j) in ascending j (trpl_refine_affine)."""
    U, M, c = _f64(U), _f64(M), _f64(c)
    if U.ndim != 2 or M.shape != (U.shape[1], U.shape[1]) or c.shape != (U.shape[1],):
        raise ValueError("U must be (S, A), M (A, A) and c (A,)")
    Z = np.empty_like(U)
    if U.shape[0]:
        _abi.check(_abi.lib().trpl_refine_affine(_abi.ptr(U), U.shape[0], U.shape[1], U.shape[1], _abi.ptr(M), _abi.ptr(c), _abi.ptr(Z),
                                                 U.shape[1], int(device), None))
    return Z


def boxes_oriented(zc, h, logdet):
    """a, b (K, A), inv_vol (K,) of the parents zc in z: [zc - h, zc + h], not clipped; inv_vol = 1 / (prod_d 2 h_d * exp(logdet)),
    the product in ascending d: the density in u, the same for every parent."""
    zc = _f64(zc)
    h = np.broadcast_to(_f64(h), (zc.shape[1],))
    if not np.all(h > 0):
        raise ValueError("every half-width must be > 0")
    vol = 1.0
    for d in range(zc.shape[1]):
        vol = vol * (2.0 * h[d])
    return np.ascontiguousarray(zc - h), np.ascontiguousarray(zc + h), np.full(zc.shape[0], 1.0 / (vol * np.exp(logdet)))


def make_proposal(U, W, K, m, n_uniform, h=None, offset=0.5, seed=1, generation=2, S1=None, device=0, info=None, oriented=False,
                  shrink=None):
    """The proposal of one generation: K parents resampled from the weights W of the samples U (S, A), boxes of half-widths h
    (default: bandwidth(U, W, S1), S1 defaulting to S) around them.  info receives the resampling's sums (sum, sum_sq, ess of W).
    oriented: the boxes are axis-parallel in z = M (u - c) of orientation(U, W, S1, shrink) instead, with its half-widths unless h
    is given (then in z), and the proposal carries the orientation."""
    U = _f64(U)
    idx, stats = resample(W, K, offset, device=device)
    if info is not None:
        info.update(stats)
    if oriented:
        o = orientation(U, W, U.shape[0] if S1 is None else S1, shrink, device=device)
        if h is not None:
            o["h"] = np.array(np.broadcast_to(_f64(h), (U.shape[1],)))
        o["zc"] = affine(U[idx], o["M"], o["c"], device=device)
        a, b, iv = boxes_oriented(o["zc"], o["h"], o["logdet"])
        return Proposal(a, b, iv, int(K), int(m), int(n_uniform), int(seed), int(generation), o)
    if h is None:
        h = bandwidth(U, W, U.shape[0] if S1 is None else S1, device=device)
    a, b, iv = boxes(U[idx], h)
    return Proposal(a, b, iv, int(K), int(m), int(n_uniform), int(seed), int(generation))


def draw(proposal, minX, maxX, do_log, sim_flags=None, device=0):
    """(X2, U2): the n_uniform + K m children of a proposal, in the box's units (S_g, ncol) and in unit coordinates (S_g, A).  The
    first n_uniform are uniform in the cube, child n_uniform + j is uniform in the box of parent j mod K (trpl_refine_draw).
    An oriented proposal returns (X2, U2, inside): the boxes are in z, u = c + L z, and inside (S_g,) int32 is 0 for a child that
    left the cube -- not to be solved, LL = -inf (trpl_refine_draw_oriented)."""
    p = proposal
    lo, hi, lg = _box(minX, maxX, do_log)
    A = p.a.shape[1]
    total = p.n_uniform + p.K * p.m
    U2, X2 = np.empty((total, A)), np.empty((total, lo.size))
    if p.orient is not None:
        o = p.orient
        Z2, inside = np.empty((total, A)), np.empty(total, dtype=np.int32)
        _abi.check(_abi.lib().trpl_refine_draw_oriented(_abi.ptr(_f64(o["zc"])), _abi.ptr(_f64(o["h"])), _abi.ptr(_f64(o["L"])),
                                                        _abi.ptr(_f64(o["c"])), p.K, A, p.m, p.n_uniform, p.seed & 0xFFFFFFFFFFFFFFFF,
                                                        p.generation & 0xFFFFFFFF, lo.size, _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg),
                                                        box_flags(sim_flags), _abi.ptr(Z2), _abi.ptr(U2), _abi.ptr(X2), _abi.ptr(inside),
                                                        int(device), None))
        return X2, U2, inside
    _abi.check(_abi.lib().trpl_refine_draw(_abi.ptr(_f64(p.a)), _abi.ptr(_f64(p.b)), p.K, A, p.m, p.n_uniform,
                                           p.seed & 0xFFFFFFFFFFFFFFFF, p.generation & 0xFFFFFFFF, lo.size, _abi.ptr(lo), _abi.ptr(hi),
                                           _abi.ptr(lg), box_flags(sim_flags), _abi.ptr(U2), _abi.ptr(X2), int(device), None))
    return X2, U2


def density(U, proposal, device=0, info=None, Z=None):
    """B (S,): the sum of inv_vol over the proposal's boxes that hold each row of U, in ascending parent order: the sequential
    loop's bits (trpl_refine_density).  An oriented proposal's boxes hold z = M (u - c): U is transformed first (affine), into the
    buffer Z (S, A) when one is given."""
    U = _f64(U)
    p = proposal
    if U.ndim != 2 or U.shape[1] != p.a.shape[1]:
        raise ValueError("U must be (S, A) with the proposal's A")
    if p.orient is not None and U.shape[0]:
        if Z is None or Z.shape != U.shape:
            Z = np.empty_like(U)
        M, c = _f64(p.orient["M"]), _f64(p.orient["c"])
        _abi.check(_abi.lib().trpl_refine_affine(_abi.ptr(U), U.shape[0], U.shape[1], U.shape[1], _abi.ptr(M), _abi.ptr(c), _abi.ptr(Z),
                                                 U.shape[1], int(device), None))
        U = Z
    B = np.empty(U.shape[0])
    sec = _abi.C.c_double(0.0)
    _abi.check(_abi.lib().trpl_refine_density(_abi.ptr(U), U.shape[0], U.shape[1], U.shape[1], _abi.ptr(_f64(p.a)), _abi.ptr(_f64(p.b)),
                                              _abi.ptr(_f64(p.inv_vol)), p.K, _abi.ptr(B), int(device), _abi.C.byref(sec)))
    if info is not None:
        info.update(seconds=sec.value)
    return B


def _add_terms(num, U, proposals, device):
    """num + the mixture terms n_uniform_g + m_g B_g(u) of the proposals, one after the other; an oriented proposal's points go
    through its own (M, c) first, all of them into one Z buffer."""
    Z = np.empty_like(U) if any(p.orient is not None for p in proposals) else None
    for p in proposals:
        B = density(U, p, device=device) if p.orient is None else density(U, p, device=device, Z=Z)
        num = num + (float(p.n_uniform) + float(p.m) * B)
    return num


def log_ratio(U, S1, proposals, device=0):
    """ln r(u) for every row of U: r = (S1 + sum_g [n_uniform_g + m_g B_g(u)]) / S_total."""
    U = _f64(U)
    num = _add_terms(np.full(U.shape[0], float(S1)), U, proposals, device)
    total = float(S1)
    for p in proposals:
        total += p.n_uniform + p.K * p.m
    return np.log(num / total)


class Population:
    """The generations of a refinement: add(X, U, LL) the first, add(X2, U2, LL2, proposal) every further one.  The numerator of
    r(u) is kept per generation with the number of proposals it holds, so a (generation, proposal) pair's density is evaluated
    once however often corrected() is called; the terms enter in the proposals' order, as log_ratio adds them."""

    def __init__(self, device=0):
        self.X, self.U, self.LL, self.proposals, self.sizes = [], [], [], [], []
        self._num, self._held = [], []                           # per generation: S1 + the terms of proposals[:held]
        self.device = device

    def add(self, X, U, LL, proposal=None, inside=None):
        """inside (S,): 0 marks a child of an oriented proposal that left the cube; its LL becomes -inf (weight exactly 0) whatever
        was passed, and it stays in the population: it counts in S_total."""
        X, U, LL = _f64(X), _f64(U), _f64(LL)
        if inside is not None:
            inside = np.asarray(inside)
            if inside.shape != LL.shape:
                raise ValueError("inside must have one entry per sample")
            LL = np.where(inside == 0, -np.inf, LL)
        if X.ndim != 2 or U.ndim != 2 or LL.shape != (X.shape[0],) or U.shape[0] != X.shape[0]:
            raise ValueError("X must be (S, ncol), U (S, A) and LL (S,)")
        if (proposal is None) != (not self.X):
            raise ValueError("the first generation has no proposal, every further one needs its own")
        if proposal is not None and X.shape[0] != proposal.n_uniform + proposal.K * proposal.m:
            raise ValueError("a generation holds its proposal's n_uniform + K m children")
        self.X.append(X); self.U.append(U); self.LL.append(LL); self.sizes.append(X.shape[0])
        self._num.append(None); self._held.append(0)
        if proposal is not None:
            self.proposals.append(proposal)

    def _log_r(self):
        """ln r(u) of every sample, r recomputed over all generations' proposals (the cached numerators brought up to date)."""
        if not self.X:
            raise ValueError("the population is empty")
        for g, U in enumerate(self.U):
            if self._num[g] is None:
                self._num[g] = np.full(U.shape[0], float(self.sizes[0]))
            self._num[g] = _add_terms(self._num[g], U, self.proposals[self._held[g]:], self.device)
            self._held[g] = len(self.proposals)
        total = float(self.sizes[0])
        for p in self.proposals:
            total += p.n_uniform + p.K * p.m
        return np.log(np.concatenate(self._num) / total)

    def corrected(self, tf=1.0):
        """(X_all, LLc): the concatenated samples and LL - tf ln r(u), r recomputed over all generations' proposals."""
        lnr = self._log_r()
        return np.concatenate(self.X), np.concatenate(self.LL) - float(tf) * lnr

    def log_ratio(self):
        """(X_all, LL_all, lnr_all): the concatenated samples, their log-likelihoods and ln r(u) from corrected()'s numerators --
        what posterior.weights / tf_scan / find_best_tf / calc_max_uncertainty / tf_for_ess take as (LL, log_ratio=), at any tf."""
        lnr = self._log_r()
        return np.concatenate(self.X), np.concatenate(self.LL), lnr

    def tf_scan(self, tfs, V=None):
        """posterior.tf_scan of the union at the temperatures tfs, with its log-ratio: stats (K, 6), ess (K,) and, with V (D, S),
        mean, var, Q."""
        _, LL, lnr = self.log_ratio()
        return posterior.tf_scan(LL, tfs, V, device=self.device, log_ratio=lnr)

    def tf_for_ess(self, target, lo=1.0, hi=1e4, rtol=1e-6, info=None):
        """posterior.tf_for_ess of the union: (tf, ess), the smallest grid temperature in [lo, hi] whose effective sample size
        reaches target.  A NaN likelihood counts as weight 0 here, as in resample and ess."""
        _, LL, lnr = self.log_ratio()
        return posterior.tf_for_ess(np.where(np.isnan(LL), -np.inf, LL), target, log_ratio=lnr, lo=lo, hi=hi, rtol=rtol,
                                    device=self.device, info=info)

    def weights(self, tf=1.0):
        return posterior.weights(self.corrected(tf)[1], tf, device=self.device)

    def ess(self, tf=1.0):
        """(sum W)^2 / sum W^2 of the union's weights at temperature tf: the sums of trpl_refine_resample, one draw asked for."""
        return float(resample(self.weights(tf), 1, device=self.device)[1]["ess"])


def run(loglik, X1, LL1, minX, maxX, do_log, sim_flags=None, rounds=1, K=1024, m=32, n_uniform=None, tf=1.0, h=None, offset=0.5, seed=1,
        device=0, info=None, target_ess=None, tf_hi=None, oriented=False, shrink=None):
    """Refine a first generation (X1, LL1) of the box by `rounds` further generations; loglik(X) -> LL is any callable (the fused
    likelihood, a toy).  n_uniform defaults to a ninth of the generation (K m / 8).  Returns the Population; info receives ess (one
    entry per generation: the union so far) and nonzero (the share of each further generation's children with a weight > 0 in the
    final union).

    target_ess: the temperature ladder.  Generation g's proposal is built from the union's weights at tf_g = max(tf,
    tf_for_ess(union, target_ess, lo=tf, hi=tf_hi)), the lowest temperature at which the union so far has that effective sample
    size (tf_hi defaults to 1e4 tf), through the log-ratio calls; tf stays the caller's final temperature, at which nonzero and
    the last entry of ess are taken.  info then also receives tfs (one per further generation; the earlier entries of ess belong
    to these) and ess_at_tf (the union's effective sample size at tf: the first generation's, then after each further one).

    oriented: every generation's boxes are axis-parallel in the whitened coordinates of the union so far (make_proposal(oriented=True,
    shrink=shrink); with target_ess the orientation rests on the ladder's weights).  loglik is called on the children inside the
    cube only; the others enter with LL = -inf.  info then also receives outside (the share of each further generation's children
    that left the cube) and lam (each generation's shrinkage)."""
    pop = Population(device=device)
    U1, _ = unit_coords(X1, minX, maxX, do_log, sim_flags, device=device)
    pop.add(X1, U1, LL1)
    n_uniform = (int(K) * int(m)) // 8 if n_uniform is None else int(n_uniform)
    esses, tfs, at_tf, outside, lams = [], [], [], [], []
    tf = float(tf)
    for g in range(2, 2 + int(rounds)):
        if target_ess is None:
            W = pop.weights(tf)                                  # once per round; its effective sample size comes with the resampling
        else:
            _, LL, lnr = pop.log_ratio()
            LL0 = np.where(np.isnan(LL), -np.inf, LL)            # a NaN likelihood counts as weight 0, as in resample
            at_tf.append(float(posterior.tf_scan(LL0, [tf], device=device, log_ratio=lnr)["ess"][0]))
            tfs.append(max(tf, posterior.tf_for_ess(LL0, target_ess, log_ratio=lnr, lo=tf, hi=1e4 * tf if tf_hi is None else float(tf_hi),
                                                    device=device)[0]))
            W = posterior.weights(LL, tfs[-1], device=device, log_ratio=lnr)
        sums = {}
        prop = make_proposal(np.concatenate(pop.U), W, K, m, n_uniform, h=h, offset=offset, seed=seed, generation=g, S1=pop.sizes[0],
                             device=device, info=sums, **({"oriented": True, "shrink": shrink} if oriented else {}))
        esses.append(float(sums["ess"]))
        if oriented:
            X2, U2, inside = draw(prop, minX, maxX, do_log, sim_flags, device=device)
            keep = inside != 0
            LL2 = np.full(X2.shape[0], -np.inf)
            if keep.any():
                LL2[keep] = _f64(loglik(np.ascontiguousarray(X2[keep])))
            pop.add(X2, U2, LL2, prop, inside=inside)
            outside.append(float(np.mean(~keep)))
            lams.append(prop.orient["lam"])
            continue
        X2, U2 = draw(prop, minX, maxX, do_log, sim_flags, device=device)
        pop.add(X2, U2, loglik(X2), prop)
    if info is not None:
        W = pop.weights(tf)
        edges = np.cumsum([0] + pop.sizes)
        info.update(ess=esses + [float(resample(W, 1, device=device)[1]["ess"])],
                    nonzero=[float(np.mean(W[edges[g]:edges[g + 1]] > 0)) for g in range(1, len(pop.sizes))])
        if target_ess is not None:
            info.update(tfs=tfs, ess_at_tf=at_tf + [info["ess"][-1]])
        if oriented:
            info.update(outside=outside, lam=lams)
    return pop
