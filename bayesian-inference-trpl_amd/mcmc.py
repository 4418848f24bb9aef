"""Ensemble Metropolis sampling on the fused likelihood (trpl_mcmc_*, include/trpl.h; csrc/mcmc.hip; DESIGN.md sections 23 and 25).

An importance-weighted population stops being useful when its effective sample size is a dozen.  Here C chains advance in
lock-step instead: one sweep proposes a move for every chain, evaluates all proposals in one call of the likelihood, and accepts or
rejects each by the Metropolis rule.  The proposal is differential evolution (ter Braak 2006): the difference of two other chains,
scaled by gamma, plus a small uniform jitter -- it needs no tuning and follows a ridge of the posterior by construction.  The
ensemble is cut into two halves that are updated in turn, each with partners from the OTHER half (ter Braak & Vrugt 2008;
Foreman-Mackey et al. 2013): within a half-sweep the partners are fixed, so every chain's move is a symmetric Metropolis kernel
that leaves the posterior invariant, and all chains of the half can move at once.  kind="rw" is the plain random walk.
kind="stretch" is the affine-invariant stretch move (Goodman & Weare 2010), an asymmetric proposal, and prior= an informative
Gaussian prior: both enter the accept step and the early-rejection level as an untempered log term per chain (accept_h,
reject_levels_h).  kind="subspace" is DREAM's move (Vrugt et al. 2009; propose_subspace):
differential evolution on a random subset of the coordinates, along the sum of several difference pairs -- symmetric like "de", so
it goes through the same accept step.

Chains live in the unit coordinates of `refine` (the active columns of the box, uniform prior on the cube).  With bounds="reject",
the default, a proposal that leaves the cube is never solved and never accepted; with bounds="fold" it is reflected back at the
faces (TRPL_MCMC_FOLD, include/trpl.h), which keeps the proposal symmetric, so every proposal is solved and can be accepted -- what
a posterior that lies against a face of the box needs.  The proposal, the accept/reject step and the sums of split-R-hat run on the device;
there is no CPU fallback.  This module takes and returns numpy arrays and goes through the host-buffer calls, like `refine`: the
likelihood it drives is any callable on a host X.  A pipeline whose chains stay on the device composes the same steps from
device.mcmc_propose_device / mcmc_levels_device / mcmc_accept_device / mcmc_chain_stats_device.

run_tempered is parallel tempering (replica exchange): K copies of the ensemble at a ladder of temperatures,
all advanced by one call each of propose_rungs / reject_levels_rungs / accept_rungs and ONE call of the likelihood per half-sweep,
with states of adjacent rungs exchanged by swap.  The hot rungs cross between separated modes that a single temperature leaves
only slowly; Tempered.rung(0) is the ensemble at the temperature the caller asked for.

Chains.samples() returns (X, W = 1): what posterior.moments / quantiles / columns / corner / credible_intervals and
posterior_predictive take.  Those states are not independent draws: Chains.ess() says how many independent draws they amount to per column, Chains.mcse()
the Monte-Carlo error of a mean, Chains.autocorr() the pooled autocorrelation; the sums over the steps and the
chains run on the device (autocov, autocov_pool), the estimator on top is ess_from_sums."""
import numpy as np

from . import _abi, posterior, refine
from .refine import _box, _f64
from .sampler import box_flags

_M64, _M32 = _abi.SEED_MASK, _abi.STEP_MASK


def _timed(entry, info, *args):
    """The host-buffer call `entry` of the library on args, a device at their end, with its `seconds` behind them: info, a dict or
    None, receives seconds.  Every timed front end of this module goes through here."""
    sec = _abi.C.c_double(0.0)
    _abi.check(getattr(_abi.lib(), entry)(*args, _abi.C.byref(sec)))
    if info is not None:
        info.update(seconds=sec.value)


def _in_place(how, U, X, LL):
    for name, a in (("U", U), ("X", X), ("LL", LL)):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError("%s is %s in place: it must be a writeable C-contiguous float64 array" % (name, how))


def _ladder(tf):
    tf = _f64(tf)
    if tf.ndim != 1 or not 1 <= tf.size <= _abi.MCMC_MAX_RUNGS:
        raise ValueError("the ladder must be (K,), 1 <= K <= %d temperatures" % _abi.MCMC_MAX_RUNGS)
    return tf


def _rung_args(tf, count, refusal="count = %d is no multiple of the %d rungs"):
    """[K, group, tf]: the temperature arguments of a *_rungs call or a swap on count rows, tf a ladder that _ladder has passed."""
    if count % tf.size:
        raise ValueError(refusal % (count, tf.size))
    return [tf.size, count // tf.size, _abi.ptr(tf)]


def _propose(U, partners, group, gamma, scale, chain0, seed, step, minX, maxX, do_log, sim_flags, device, info, fold):
    """trpl_mcmc_propose, or with a group trpl_mcmc_propose_rungs, which takes it behind P: the marshaller of propose and
    propose_rungs.  A new argument of either goes HERE."""
    U = _f64(U)
    lo, hi, lg = _box(minX, maxX, do_log)
    if U.ndim != 2:
        raise ValueError("U must be (count, A)")
    count, A = U.shape
    scale = np.ascontiguousarray(np.broadcast_to(_f64(scale), (A,)))
    P = 0
    if partners is not None or group is not None:
        partners = _f64(partners)
        if partners.ndim != 2 or partners.shape[1] != A:
            raise ValueError("partners must be (P, A)")
        P = partners.shape[0]
    Up, Xp, inside = np.empty((count, A)), np.empty((count, lo.size)), np.empty(count, dtype=np.int32)
    _timed("trpl_mcmc_propose" if group is None else "trpl_mcmc_propose_rungs", info,
           _abi.ptr(U), None if partners is None else _abi.ptr(partners), count, P, *([] if group is None else [group]), A,
           float(gamma), _abi.ptr(scale), int(chain0), int(seed) & _M64, int(step) & _M32, lo.size, _abi.ptr(lo), _abi.ptr(hi),
           _abi.ptr(lg), box_flags(sim_flags) | (_abi.MCMC_FOLD if fold else 0), _abi.ptr(Up), _abi.ptr(Xp), _abi.ptr(inside), int(device))
    return Up, Xp, inside


def _accept(rungs, U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step, device, info, h=None):
    """trpl_mcmc_accept, or with rungs trpl_mcmc_accept_rungs, which takes (K, group, tf (K,)) where the other takes tf, or with h
    trpl_mcmc_accept_h, which takes h behind inside and the ladder like accept_rungs: the marshaller of accept, accept_rungs and
    accept_h."""
    _in_place("updated", U, X, LL)
    if rungs:
        tf = _ladder(tf)
    Up, Xp, LLp = _f64(Up), _f64(Xp), _f64(LLp)
    inside = np.ascontiguousarray(inside, dtype=np.int32)
    if U.ndim != 2 or X.ndim != 2 or X.shape[0] != U.shape[0] or Up.shape != U.shape or Xp.shape != X.shape:
        raise ValueError("U and Up must be (count, A), X and Xp (count, ncol)")
    count = U.shape[0]
    if LL.shape != (count,) or LLp.shape != (count,) or inside.shape != (count,):
        raise ValueError("LL, LLp and inside must be (count,)")
    term = []
    if h is not None:
        h = _f64(h)
        if h.shape != (count,):
            raise ValueError("h must be (count,)")
        term = [_abi.ptr(h)]
    temper = _rung_args(tf, count) if rungs else [float(tf)]
    accepted = np.empty(count, dtype=np.int32)
    _timed("trpl_mcmc_accept_h" if h is not None else "trpl_mcmc_accept_rungs" if rungs else "trpl_mcmc_accept", info,
           _abi.ptr(U), _abi.ptr(X), _abi.ptr(LL), _abi.ptr(Up), _abi.ptr(Xp), _abi.ptr(LLp), _abi.ptr(inside), *term, count, U.shape[1],
           X.shape[1], *temper, int(chain0), int(seed) & _M64, int(step) & _M32, _abi.ptr(accepted), int(device))
    return accepted


def _levels(rungs, LL, tf, chain0, seed, step, device, info, h=None):
    """trpl_mcmc_levels, or with rungs trpl_mcmc_levels_rungs, or with h trpl_mcmc_levels_h (h behind LL, the ladder like levels_rungs):
    the marshaller of reject_levels, reject_levels_rungs and reject_levels_h."""
    LL = _f64(LL)
    if rungs:
        tf = _ladder(tf)
    if LL.ndim != 1:
        raise ValueError("LL must be (count,)")
    term = []
    if h is not None:
        h = _f64(h)
        if h.shape != LL.shape:
            raise ValueError("h must be (count,)")
        term = [_abi.ptr(h)]
    temper = _rung_args(tf, LL.shape[0]) if rungs else [float(tf)]
    level = np.empty(LL.shape[0])
    _timed("trpl_mcmc_levels_h" if h is not None else "trpl_mcmc_levels_rungs" if rungs else "trpl_mcmc_levels", info,
           _abi.ptr(LL), *term, LL.shape[0], *temper, int(chain0), int(seed) & _M64, int(step) & _M32, _abi.ptr(level), int(device))
    return level


def propose(U, partners, gamma, scale, chain0, seed, step, minX, maxX, do_log, sim_flags=None, device=0, info=None, fold=False):
    """(Up, Xp, inside): one symmetric proposal per chain of U (count, A) (trpl_mcmc_propose).  partners (P >= 2, A): u' = (u + gamma
    (pa - pb)) + scale (2 xi - 1) with two distinct rows a, b of partners; partners None: the random walk u' = u + scale (2 xi - 1).
    scale (A,) or a scalar.  chain0 is the ensemble index of U's first row and step the half-sweep: they key the Philox stream.
    inside (count,) int32 is 0 where u' left the unit cube; Xp is formed either way.  fold=True (TRPL_MCMC_FOLD): u' is reflected
    back at the faces of the cube, and inside is 0 where a coordinate is not finite, 1 where nothing was folded, 2 where something
    was."""
    return _propose(U, partners, None, gamma, scale, chain0, seed, step, minX, maxX, do_log, sim_flags, device, info, fold)


def accept(U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step, device=0, info=None):
    """accepted (count,) int32: the Metropolis step of every chain at temperature tf (trpl_mcmc_accept).  U (count, A), X (count,
    ncol) and LL (count,) -- C-contiguous float64 arrays -- are updated IN PLACE: the rows of an accepted proposal are copied, the
    others stay."""
    return _accept(False, U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step, device, info)


def reject_levels(LL, tf, chain0, seed, step, device=0, info=None):
    """level (count,): for every chain the sse level above which accept(), called with the same (tf, chain0, seed, step), is certain
    to reject the proposal (trpl_mcmc_levels) -- the cut_levels of driver.loglik, one per proposal.  The accept step's uniform
    depends on (seed; chain, step) only, so the level is known before the proposal is solved.  +inf where nothing may be cut: a
    chain whose LL is NaN or -inf accepts anything.  LL must be minus the summed sse, i.e. come from a likelihood whose P starts
    from zero (include/trpl.h has the argument)."""
    return _levels(False, LL, tf, chain0, seed, step, device, info)


def propose_rungs(U, partners, group, gamma, scale, chain0, seed, step, minX, maxX, do_log, sim_flags=None, device=0, info=None,
                  fold=False):
    """(Up, Xp, inside): propose() for a block of rungs of `group` chains each (trpl_mcmc_propose_rungs): chain i of U (count, A) takes
    its two partners from the rows [(i // group) group, + group) of partners (P, A); P is a multiple of group, count <= P.  The rows
    of rung k are propose() on that slice of U with that block of partners and chain0 + k group, bit for bit."""
    return _propose(U, partners, int(group), gamma, scale, chain0, seed, step, minX, maxX, do_log, sim_flags, device, info, fold)


def accept_rungs(U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step, device=0, info=None):
    """accepted (count,) int32: accept() with a temperature per rung (trpl_mcmc_accept_rungs).  tf (K,): the count rows are K rungs of
    count / K chains each.  U, X and LL are updated IN PLACE.  The rows of rung k are accept() on them with tf[k] and chain0 + k
    count / K, bit for bit."""
    return _accept(True, U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step, device, info)


def reject_levels_rungs(LL, tf, chain0, seed, step, device=0, info=None):
    """level (count,): reject_levels() with a temperature per rung (trpl_mcmc_levels_rungs), tf (K,): the levels above which
    accept_rungs(), called with the same (tf, chain0, seed, step), is certain to reject."""
    return _levels(True, LL, tf, chain0, seed, step, device, info)


def swap(U, X, LL, tf, parity, chain0, seed, step, device=0, info=None):
    """swapped (K group,) int32: the replica exchange between adjacent rungs of one block (trpl_mcmc_swap).  U (K group, A), X (K group,
    ncol) and LL (K group,) -- writeable C-contiguous float64 arrays -- are exchanged IN PLACE between the rows a = k group + c and
    b = a + group for k = parity, parity + 2, .. with k + 1 < K: with d = (LL[b] - LL[a]) (1 / tf[k] - 1 / tf[k + 1]), when neither
    LL is NaN and d >= 0 or log(xi) < d.  swapped is 1 on both rows of an exchanged pair, 0 on every other row."""
    _in_place("exchanged", U, X, LL)
    tf = _ladder(tf)
    if U.ndim != 2 or X.ndim != 2 or X.shape[0] != U.shape[0] or LL.shape != (U.shape[0],):
        raise ValueError("U must be (K group, A), X (K group, ncol) and LL (K group,)")
    K, group, ladder = _rung_args(tf, U.shape[0], "the %d rows are no multiple of the %d rungs")
    swapped = np.empty(U.shape[0], dtype=np.int32)
    _timed("trpl_mcmc_swap", info, _abi.ptr(U), _abi.ptr(X), _abi.ptr(LL), K, group, U.shape[1], X.shape[1], ladder, int(parity), int(chain0),
           int(seed) & _M64, int(step) & _M32, _abi.ptr(swapped), int(device))
    return swapped


def propose_stretch(U, partners, group, a, chain0, seed, step, minX, maxX, do_log, sim_flags=None, device=0, info=None):
    """(Up, Xp, inside, z, lnq): one stretch proposal per chain of U (count, A) (trpl_mcmc_propose_stretch; Goodman & Weare 2010):
    u' = p + z (u - p) with p one row of the chain's rung [(i // group) group, + group) of partners (P, A) and z = ((a - 1) xi + 1)^2
    / a.  group None: one rung, group = P.  z (count,) is the stretch and lnq (count,) = (A - 1) log(z) the Hastings term that
    accept_h takes as h.  inside is 0 where u' left the unit cube; Xp is formed either way.  There is no fold: a reflected stretch is
    not reversible."""
    U, partners = _f64(U), _f64(partners)
    lo, hi, lg = _box(minX, maxX, do_log)
    if U.ndim != 2:
        raise ValueError("U must be (count, A)")
    count, A = U.shape
    if partners.ndim != 2 or partners.shape[1] != A:
        raise ValueError("partners must be (P, A)")
    P = partners.shape[0]
    Up, Xp, inside = np.empty((count, A)), np.empty((count, lo.size)), np.empty(count, dtype=np.int32)
    z, lnq = np.empty(count), np.empty(count)
    _timed("trpl_mcmc_propose_stretch", info, _abi.ptr(U), _abi.ptr(partners), count, P, P if group is None else int(group), A, float(a),
           int(chain0), int(seed) & _M64, int(step) & _M32, lo.size, _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg), box_flags(sim_flags),
           _abi.ptr(Up), _abi.ptr(Xp), _abi.ptr(inside), _abi.ptr(z), _abi.ptr(lnq), int(device))
    return Up, Xp, inside, z, lnq


def subspace_gamma_table(pairs, A, factor=1.0):
    """(pairs, A): the gamma of the subspace move by (delta - 1, dsel - 1), factor * 2.38 / sqrt(2 delta dsel) -- ter Braak's optimal
    jump for delta difference pairs in a subspace of dsel coordinates."""
    delta, dsel = np.arange(1, int(pairs) + 1, dtype=np.float64)[:, None], np.arange(1, int(A) + 1, dtype=np.float64)[None, :]
    return np.ascontiguousarray(float(factor) * (2.38 / np.sqrt(2.0 * delta * dsel)))


def _pcr_arg(pcr, ncr):
    """pcr of propose_subspace, run and run_tempered as an (ncr,) array of shares, or None (equal shares)."""
    if pcr is None:
        return None
    pcr = _f64(pcr)
    if pcr.shape != (ncr,):
        raise ValueError("pcr must be (ncr,) = (%d,) shares of the crossover classes" % ncr)
    if not (np.all(np.isfinite(pcr)) and np.all(pcr >= 0.0) and pcr.sum() > 0.0):
        raise ValueError("pcr: every share must be finite and >= 0 and their sum > 0")
    return pcr


def propose_subspace(U, partners, group, gamma_tab, scale, chain0, seed, step, minX, maxX, do_log, ncr=3, pcr=None, e_width=0.05,
                     sim_flags=None, device=0, info=None, fold=False):
    """(Up, Xp, inside, mask, sel): one subspace differential-evolution proposal per chain of U (count, A)
    (trpl_mcmc_propose_subspace; DREAM, Vrugt et al. 2009).  Per chain: a crossover class m is drawn with the shares pcr (ncr,) (None:
    equal), CR = (m + 1) / ncr; each coordinate is selected with probability CR (one at random if none is); delta, uniform in 1 ..
    pairs = gamma_tab.shape[0], pairs of distinct rows (a, b) are drawn from the chain's rung [(i // group) group, + group) of partners
    (P, A); on the selected coordinates u' = (u + g e sum_p (pa_p - pb_p)) + scale (2 xi - 1) with g = gamma_tab[delta - 1][selected
    - 1] and e = 1 + e_width (2 v - 1); the others keep their bits.  group None: one rung, group = P.  mask (count,) int32 has bit d
    set where coordinate d moved; sel (count,) int32 is delta | m << 8.  inside and fold as in propose.  With ncr = 1, one pair,
    e_width = 0 and a table filled with gamma the first three are propose_rungs' bit for bit."""
    U, partners = _f64(U), _f64(partners)
    lo, hi, lg = _box(minX, maxX, do_log)
    if U.ndim != 2:
        raise ValueError("U must be (count, A)")
    count, A = U.shape
    if partners.ndim != 2 or partners.shape[1] != A:
        raise ValueError("partners must be (P, A)")
    tab = _f64(gamma_tab)
    if tab.ndim != 2 or tab.shape[1] != A:
        raise ValueError("gamma_tab must be (pairs, A)")
    ncr = int(ncr)
    pcr = _pcr_arg(pcr, ncr)
    scale = np.ascontiguousarray(np.broadcast_to(_f64(scale), (A,)))
    P = partners.shape[0]
    Up, Xp = np.empty((count, A)), np.empty((count, lo.size))
    inside, mask, sel = (np.empty(count, dtype=np.int32) for _ in range(3))
    _timed("trpl_mcmc_propose_subspace", info, _abi.ptr(U), _abi.ptr(partners), count, P, P if group is None else int(group), A, 1.0,
           _abi.ptr(scale), int(chain0), int(seed) & _M64, int(step) & _M32, lo.size, _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg),
           box_flags(sim_flags) | (_abi.MCMC_FOLD if fold else 0), _abi.ptr(Up), _abi.ptr(Xp), _abi.ptr(inside), tab.shape[0], ncr,
           None if pcr is None else _abi.ptr(pcr), _abi.ptr(tab), float(e_width), _abi.ptr(mask), _abi.ptr(sel), int(device))
    return Up, Xp, inside, mask, sel


def accept_h(U, X, LL, Up, Xp, LLp, inside, h, tf, chain0, seed, step, device=0, info=None):
    """accepted (count,) int32: accept_rungs() with an untempered log term h (count,) per chain (trpl_mcmc_accept_h): d = (LLp - LL) /
    tf + h.  tf (K,), or a scalar for one temperature.  h is the log of the proposal's ratio q(u' -> u) / q(u -> u') (propose_stretch's
    lnq), of the prior's ratio (prior_term), or their sum; a chain whose h is NaN or -inf stays.  With h = 0 the bits of accept_rungs."""
    return _accept(True, U, X, LL, Up, Xp, LLp, inside, np.atleast_1d(_f64(tf)), chain0, seed, step, device, info, h=h)


def reject_levels_h(LL, h, tf, chain0, seed, step, device=0, info=None):
    """level (count,): reject_levels_rungs() for accept_h() called with the same (h, tf, chain0, seed, step) (trpl_mcmc_levels_h).  +inf
    also where h is NaN or infinite.  A level can be negative (h far below zero: every LLp <= 0 is rejected); driver.loglik takes
    max(level, 0)."""
    return _levels(True, LL, np.atleast_1d(_f64(tf)), chain0, seed, step, device, info, h=h)


def prior_term(U, Up, mean, sd, h=None, device=0, info=None):
    """h_out (count,) = h + (lnp(Up) - lnp(U)), lnp(u) = sum_d -t^2 / 2 with t = (u_d - mean_d) / sd_d: the log ratio of an independent
    Gaussian prior in unit coordinates between the proposals Up and the chains U, both (count, A), added to h (None: zeros)
    (trpl_mcmc_prior_term).  mean and sd are (A,); sd_d = inf is a flat column and adds exactly 0."""
    U, Up = _f64(U), _f64(Up)
    if U.ndim != 2 or Up.shape != U.shape:
        raise ValueError("U and Up must be (count, A)")
    count, A = U.shape
    mean, sd = _f64(mean), _f64(sd)
    if mean.shape != (A,) or sd.shape != (A,):
        raise ValueError("mean and sd must be (A,)")
    if h is not None:
        h = _f64(h)
        if h.shape != (count,):
            raise ValueError("h must be (count,)")
    out = np.empty(count)
    _timed("trpl_mcmc_prior_term", info, _abi.ptr(U), _abi.ptr(Up), count, A, _abi.ptr(mean), _abi.ptr(sd),
           None if h is None else _abi.ptr(h), _abi.ptr(out), int(device))
    return out


def gaussian_prior(center_X, width, minX, maxX, do_log, sim_flags=None):
    """(mean_u, sd_u), each (A,): the prior= of run and run_tempered from a centre row center_X (ncol,) in the box's units and a width
    (ncol,) per column -- one standard deviation, in the column's units on a linear column and in decades on a log column; inf (or
    a fixed column) means flat.  The unit coordinate of a column is (x - lo) / (hi - lo), in log10 on a log column, so the Gaussian
    is one in x on a linear column and a log-normal on a log column."""
    lo, hi, lg = _box(minX, maxX, do_log)
    c, w = np.broadcast_to(_f64(center_X), lo.shape), np.broadcast_to(_f64(width), lo.shape)
    act = refine.active_columns(lo, hi, sim_flags)
    mean, sd = np.full(act.size, 0.5), np.full(act.size, np.inf)
    for k, col in enumerate(act):
        if np.isinf(w[col]) and w[col] > 0:
            continue
        if not (w[col] > 0 and np.isfinite(c[col])):
            raise ValueError("column %d: the width must be > 0 (inf: flat) and the centre finite" % col)
        if lg[col]:
            if not c[col] > 0:
                raise ValueError("column %d: the centre of a log column must be > 0" % col)
            span = np.log10(hi[col]) - np.log10(lo[col])
            mean[k], sd[k] = (np.log10(c[col]) - np.log10(lo[col])) / span, w[col] / span
        else:
            span = hi[col] - lo[col]
            mean[k], sd[k] = (c[col] - lo[col]) / span, w[col] / span
    return mean, sd


def geometric_ladder(tf, tf_hot, K):
    """(K,) temperatures from tf to tf_hot in equal ratios: tf (tf_hot / tf)^(k / (K - 1)); K = 1 gives [tf]."""
    tf, tf_hot, K = float(tf), float(tf_hot), int(K)
    if not (np.isfinite(tf) and np.isfinite(tf_hot) and tf > 0.0 and tf_hot > 0.0):
        raise ValueError("tf and tf_hot must be finite and > 0")
    if not 1 <= K <= _abi.MCMC_MAX_RUNGS:
        raise ValueError("K=%d must be in [1, %d]" % (K, _abi.MCMC_MAX_RUNGS))
    if K == 1:
        return np.array([tf])
    out = tf * (tf_hot / tf) ** (np.arange(K) / float(K - 1))
    out[0], out[-1] = tf, tf_hot
    return out


def chain_stats(H, t0=0, t1=None, Q=None, device=0, info=None):
    """(mean, m2), each (Q,): per column q < Q of the history H (n, ldh >= Q), the mean and the centred sum of squares over the steps
    [t0, t1), both sums in ascending t from +0.0 (trpl_mcmc_chain_stats): the plain loop's bits.  Q defaults to ldh, t1 to n."""
    H = _f64(H)
    if H.ndim != 2:
        raise ValueError("H must be (n, ldh)")
    n, ldh = H.shape
    Q = ldh if Q is None else int(Q)
    t1 = n if t1 is None else int(t1)
    mean, m2 = np.empty(max(Q, 0)), np.empty(max(Q, 0))
    _timed("trpl_mcmc_chain_stats", info, _abi.ptr(H), n, ldh, Q, int(t0), t1, _abi.ptr(mean), _abi.ptr(m2), int(device))
    return mean, m2


def autocov(H, max_lag, t0=0, t1=None, Q=None, device=0, info=None):
    """(mean (Q,), s (max_lag, Q)): per column q < Q of the history H (n, ldh >= Q) over the steps [t0, t1), the mean and the sums
    s[l][q] of e[t] e[t + l], e = H - mean, t = t0 .. t1 - 1 - l ascending from +0.0, for the lags l < max_lag <= t1 - t0
    (trpl_mcmc_autocov): the plain loop's bits; s[0] is chain_stats' m2.  Q defaults to ldh, t1 to n."""
    H = _f64(H)
    if H.ndim != 2:
        raise ValueError("H must be (n, ldh)")
    n, ldh = H.shape
    Q = ldh if Q is None else int(Q)
    t1 = n if t1 is None else int(t1)
    L = int(max_lag)
    mean, s = np.empty(max(Q, 0)), np.empty((max(L, 0), max(Q, 0)))
    _timed("trpl_mcmc_autocov", info, _abi.ptr(H), n, ldh, Q, int(t0), t1, L, _abi.ptr(mean), _abi.ptr(s), int(device))
    return mean, s


def autocov_pool(s, M, A, device=0, info=None):
    """pooled (L, A): the sums of autocov over the M sequences of s (L, lds >= M A), whose columns are M groups of A:
    pooled[l][a] = sum over c of s[l][c A + a], c ascending from +0.0 (trpl_mcmc_autocov_pool)."""
    s = _f64(s)
    if s.ndim != 2:
        raise ValueError("s must be (L, lds)")
    L, lds = s.shape
    pooled = np.empty((L, max(int(A), 0)))
    _timed("trpl_mcmc_autocov_pool", info, _abi.ptr(s), L, lds, int(M), int(A), _abi.ptr(pooled), int(device))
    return pooled


def ess_from_sums(mean, m2, pooled, m):
    """(ess (A,), info): the effective sample size of M sequences of m steps each from their sums -- mean and m2 (M, A) (or (M A,),
    sequence-major) of chain_stats, pooled (L, A) of autocov_pool.  Pure numpy; the rule is Geyer's initial monotone sequence on
    the pooled autocorrelation (Geyer 1992; Vehtari et al. 2021).  Per column:
        W = mean over the sequences of m2 / (m - 1),   B / m = var(mean, ddof 1) (0 for M = 1),   var+ = (m - 1) / m W + B / m,
        acov[l] = pooled[l] / (M m),   rho[l] = 1 - (W - acov[l]) / var+,   rho[0] = 1,
        P_k = rho[2k] + rho[2k + 1];   K = the first k where P_k > 0 fails, or L // 2 if it never fails -- then truncated is True:
        the lags ran out before the correlation did, and the ESS is an upper bound;   P made non-increasing by a running minimum,
        tau = max(-1 + 2 sum_{k < K} P_k, 1 / log10(M m)),   ess = M m / tau.
    info: tau, var_plus (A,), rho (L, A), K (A,) int, truncated (A,) bool."""
    pooled = np.asarray(pooled, dtype=np.float64)
    if pooled.ndim != 2:
        raise ValueError("pooled must be (L, A)")
    L, A = pooled.shape
    mean, m2 = np.asarray(mean, dtype=np.float64).reshape(-1, A), np.asarray(m2, dtype=np.float64).reshape(-1, A)
    M, m = mean.shape[0], int(m)
    if m2.shape != mean.shape or M < 1 or L < 1:
        raise ValueError("mean and m2 must be (M, A) and pooled (L, A)")
    if m < 2:
        raise ValueError("m=%d: a sequence needs at least 2 steps" % m)
    with np.errstate(invalid="ignore", divide="ignore"):
        W = np.mean(m2 / (m - 1), axis=0)
        Bm = np.var(mean, axis=0, ddof=1) if M > 1 else np.zeros(A)
        var_plus = (m - 1) / m * W + Bm
        rho = 1.0 - (W - pooled / float(M * m)) / var_plus
    rho[0] = 1.0
    pairs = L // 2
    P = rho[0:2 * pairs:2] + rho[1:2 * pairs:2]                  # (pairs, A)
    K, truncated, tau = np.empty(A, dtype=np.int64), np.empty(A, dtype=bool), np.empty(A)
    floor = 1.0 / np.log10(M * m)
    for a in range(A):
        stop = np.flatnonzero(~(P[:, a] > 0.0))
        truncated[a] = stop.size == 0
        K[a] = pairs if truncated[a] else stop[0]
        mono = np.minimum.accumulate(P[:K[a], a])
        total = float(np.cumsum(mono)[-1]) if K[a] else 0.0      # the pairs added one by one, in order
        tau[a] = max(-1.0 + 2.0 * total, floor)
    ess = M * m / tau
    return ess, dict(tau=tau, var_plus=var_plus, rho=rho, K=K, truncated=truncated)


def evidence_sums(LL, tf, t0=0, t1=None, blocks=1, device=0, info=None):
    """(ext (K, 2), sums (K, blocks, 6)): from the kept LL (K, n, C) of the K rungs of the ladder tf (K,), over the steps [t0, t1) cut
    into `blocks` blocks of (t1 - t0) / blocks consecutive steps, the [maximum, minimum] of each rung and per block [sum LL, up, up2,
    down, down2, count above -inf] (trpl_mcmc_evidence_sums; include/trpl.h has the terms, the rule of -inf and the one association
    of every sum).  What log_evidence_ratios takes.  t1 defaults to n."""
    LL, tf = _f64(LL), _ladder(tf)
    if LL.ndim != 3 or LL.shape[0] != tf.size:
        raise ValueError("LL must be (K, n, C) with the ladder's K = %d" % tf.size)
    K, n, C = LL.shape
    t1 = n if t1 is None else int(t1)
    B = int(blocks)
    ext, sums = np.empty((K, 2)), np.empty((K, max(B, 0), _abi.MCMC_EVIDENCE_SUMS))
    _timed("trpl_mcmc_evidence_sums", info, _abi.ptr(LL), K, n, C, int(t0), t1, B, _abi.ptr(tf), _abi.ptr(ext), _abi.ptr(sums), int(device))
    return ext, sums


def log_evidence_ratios(ext, sums, ladder):
    """The log-evidence differences between the adjacent rungs of a ladder (K,) from evidence_sums' ext (K, 2) and sums (K, B, 6).
    Pure numpy, one rule (restated in include/trpl.h).  With Z(tf) the integral of exp(LL / tf) p(u) over the cube, delta_k =
    1 / tf_k - 1 / tf_(k+1), N_k the count of a rung's values above -inf (a state at -inf has no mass at any temperature), every
    sum over the blocks in ascending b, for each pair k, k + 1 three estimates of ln Z(tf_k) - ln Z(tf_(k+1)):
        forward = delta_k a  + ln(up_(k+1) / N_(k+1))      stepping-stone sampling from the hotter rung (Xie et al. 2011); a, a' are the
        reverse = delta_k a' - ln(down_k / N_k)            the same from the colder rung                         kernel's centres
        ti      = delta_k (mean LL_k + mean LL_(k+1)) / 2  the trapezoid of thermodynamic integration (Lartillot & Philippe 2006)
    forward is the stable direction (its terms are bounded by the hot rung's best state); reverse is carried by the colder rung's worst
    states and is biased upward when they are rare: where the two disagree by more than their errors, the rungs are too far apart
    or the run has not equilibrated (DESIGN.md section 34 has a case).
    ti has the trapezoid's discretisation bias, which no error bar shows.  Each estimate has a leave-one-block-out jackknife
    standard error over the B blocks (NaN for B = 1).  term_ess (K - 1, 2) = (sum e)^2 / (N sum e^2) of the forward and the reverse
    sum: the share of the states that carry it, the warning sign of a stepping stone that rests on a handful.  A Gaussian prior= of
    the run is common to the rungs and cancels in every difference.
    Returns dict(delta, N (K,), forward, reverse, ti and <name>_se (K - 1,), term_ess, <name>_total and <name>_total_se: the pairs
    added in ascending k from 0.0 -- ln Z(tf_0) - ln Z(tf_(K-1)) -- and their errors in quadrature; K = 1: empty and 0.0)."""
    tf = _ladder(ladder)
    K = tf.size
    ext, sums = np.asarray(ext, dtype=np.float64), np.asarray(sums, dtype=np.float64)
    if ext.shape != (K, 2) or sums.ndim != 3 or sums.shape[0] != K or sums.shape[1] < 1 or sums.shape[2] != _abi.MCMC_EVIDENCE_SUMS:
        raise ValueError("ext must be (K, 2) and sums (K, B >= 1, %d) with the ladder's K = %d" % (_abi.MCMC_EVIDENCE_SUMS, K))
    B = sums.shape[1]
    delta = 1.0 / tf[:-1] - 1.0 / tf[1:]
    a_up = np.where(delta >= 0.0, ext[1:, 0], ext[1:, 1])       # the centre of up of rung k + 1, of down of rung k
    a_down = np.where(delta >= 0.0, ext[:-1, 1], ext[:-1, 0])

    def estimates(S):                                            # S (K, 6): a rung's sums over some of the blocks
        N = S[:, 5]
        mean = S[:, 0] / N
        forward = np.where(delta == 0.0, 0.0, delta * a_up) + np.log(S[1:, 1] / N[1:])
        reverse = np.where(delta == 0.0, 0.0, delta * a_down) - np.log(S[:-1, 3] / N[:-1])
        return np.stack([forward, reverse, delta * (mean[:-1] + mean[1:]) / 2.0])

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        head, tail = np.zeros((B + 1, K, sums.shape[2])), np.zeros((B + 1, K, sums.shape[2]))
        for b in range(B):                                       # head[b]: the blocks before b; tail[b]: the blocks from b on
            head[b + 1] = head[b] + sums[:, b]
            tail[B - 1 - b] = sums[:, B - 1 - b] + tail[B - b]
        S = head[B]
        est = estimates(S)
        if B > 1:
            left_out = np.stack([estimates(head[b] + tail[b + 1]) for b in range(B)])        # (B, 3, K - 1)
            se = np.sqrt((B - 1.0) / B * np.sum((left_out - np.mean(left_out, axis=0)) ** 2, axis=0))
        else:
            se = np.full(est.shape, np.nan)
        term_ess = np.stack([S[1:, 1] ** 2 / (S[1:, 5] * S[1:, 2]), S[:-1, 3] ** 2 / (S[:-1, 5] * S[:-1, 4])], axis=1)
    out = dict(delta=delta, N=S[:, 5].copy(), term_ess=term_ess, blocks=B)
    for i, name in enumerate(("forward", "reverse", "ti")):
        total, var = 0.0, 0.0
        for k in range(K - 1):
            total, var = total + float(est[i, k]), var + float(se[i, k]) ** 2
        out.update({name: est[i], name + "_se": se[i], name + "_total": total, name + "_total_se": float(np.sqrt(var))})
    return out


def start(X, LL, C, minX, maxX, do_log, sim_flags=None, tf=1.0, offset=0.5, log_ratio=None, device=0):
    """(X0, U0, LL0): C starting states drawn from an importance-weighted set -- a first generation (X, LL), or a refined
    Population's log_ratio() as (X, LL, log_ratio=) -- by refine.resample of posterior.weights at temperature tf, with their unit
    coordinates (refine.unit_coords).  A set whose effective sample size is small starts many chains on the same point; the
    differential-evolution jitter separates them."""
    X, LL = _f64(X), _f64(LL)
    W = posterior.weights(LL, tf, device=device, log_ratio=log_ratio)
    idx, _ = refine.resample(W, int(C), offset, device=device)
    X0 = np.ascontiguousarray(X[idx])
    U0, _ = refine.unit_coords(X0, minX, maxX, do_log, sim_flags, device=device)
    return X0, U0, np.ascontiguousarray(LL[idx])


class Chains:
    """The kept history of a run: U (n, C, A) unit coordinates, X (n, C, ncol) in the box's units, LL (n, C), accept (n, C) bool (the
    chain moved in that sweep), one entry per kept sweep."""

    def __init__(self, U, X, LL, accept, device=0):
        self.U, self.X, self.LL, self.accept, self.device = U, X, LL, accept, device

    def samples(self, burn=0, thin=1):
        """(X (N, ncol), W = ones(N)): the states of the kept sweeps burn, burn + thin, ... of every chain, equally weighted."""
        X = self.X[int(burn)::int(thin)]
        X = np.ascontiguousarray(X.reshape(-1, X.shape[2]))
        return X, np.ones(X.shape[0])

    def rhat(self, burn=0):
        """Split-R-hat of every active column (A,).  The kept sweeps from burn on are cut into two halves of n2 = n // 2: 2 C
        sequences, whose means and centred sums of squares come from the device (chain_stats on the history where it lies).  W =
        mean of m2 / (n2 - 1), B = n2 var(means, ddof 1), R-hat = sqrt(((n2 - 1) / n2 W + B / n2) / W)."""
        n, C, A = self.U.shape
        burn = int(burn)
        n2 = (n - burn) // 2
        if n2 < 2:
            raise ValueError("split-R-hat needs two halves of at least 2 kept sweeps each; %d sweeps are left after burn" % max(n - burn, 0))
        H = self.U.reshape(n, C * A)
        parts = [chain_stats(H, burn + k * n2, burn + (k + 1) * n2, device=self.device) for k in (0, 1)]
        mean = np.concatenate([p[0].reshape(C, A) for p in parts])          # (2 C, A)
        m2 = np.concatenate([p[1].reshape(C, A) for p in parts])
        W = np.mean(m2 / (n2 - 1), axis=0)
        B = n2 * np.var(mean, axis=0, ddof=1)
        return np.sqrt(((n2 - 1) / n2 * W + B / n2) / W)

    def ess(self, burn=0, max_lag=None, values=None, max_workspace_bytes=1 << 30):
        """(ess (D,), info): the effective sample size of the kept sweeps from burn on, per column -- how many independent draws the
        n2 x 2 C states amount to (ess_from_sums has the rule and info's keys).  The history is cut into the two halves of rhat,
        2 C sequences of n2 = (n - burn) // 2; each half is one trpl_mcmc_autocov_chains call (the sums over the steps and over
        the chains on the device, s in device scratch), and the pooled sums are added, half 0 + half 1.  max_lag defaults to n2.
        values (n, C, D), 1 <= D <= 16, asks about other columns than U: LL[..., None], X, a derived column of posterior.columns.
        The scratch of a call, 8 max_lag C D bytes, is refused above max_workspace_bytes before anything runs."""
        n, C = self.U.shape[:2]
        V = self.U if values is None else _f64(values)
        if V.ndim != 3 or V.shape[:2] != (n, C) or not 1 <= V.shape[2] <= _abi.REFINE_MAX_DIMS:
            raise ValueError("values must be (n, C, D) = (%d, %d, 1 .. %d)" % (n, C, _abi.REFINE_MAX_DIMS))
        D = V.shape[2]
        burn = int(burn)
        n2 = (n - burn) // 2
        if n2 < 2:
            raise ValueError("split-R-hat needs two halves of at least 2 kept sweeps each; %d sweeps are left after burn" % max(n - burn, 0))
        L = n2 if max_lag is None else int(max_lag)
        if not 1 <= L <= n2:
            raise ValueError("max_lag=%d must be in [1, n2 = %d]" % (L, n2))
        need = 8 * L * C * D
        if need > int(max_workspace_bytes):
            raise ValueError("the sums of %d lags x %d chains x %d columns need %d bytes of device scratch, more than "
                             "max_workspace_bytes = %d" % (L, C, D, need, int(max_workspace_bytes)))
        H = _f64(V).reshape(n, C * D)
        mean, m2, pooled = np.empty((2, C * D)), np.empty((2, C * D)), np.empty((2, L, D))
        for k in (0, 1):
            _abi.check(_abi.lib().trpl_mcmc_autocov_chains(_abi.ptr(H), n, C * D, C, D, burn + k * n2, burn + (k + 1) * n2, L,
                                                           _abi.ptr(mean[k]), _abi.ptr(m2[k]), _abi.ptr(pooled[k]), int(self.device),
                                                           None))
        return ess_from_sums(mean.reshape(2 * C, D), m2.reshape(2 * C, D), pooled[0] + pooled[1], n2)

    def autocorr(self, burn=0, max_lag=None, values=None):
        """rho (max_lag, D): the pooled autocorrelation of ess(), lag by lag."""
        return self.ess(burn, max_lag, values)[1]["rho"]

    def mcse(self, burn=0, max_lag=None, values=None):
        """(D,): the Monte-Carlo standard error of the mean of each column over the kept sweeps from burn on, sqrt(var+ / ess)."""
        ess, info = self.ess(burn, max_lag, values)
        return np.sqrt(info["var_plus"] / ess)


_SUBSPACE_DEFAULTS = dict(pairs=3, ncr=3, e_width=0.05, pcr=None, adapt_cr=False)


def _proposal_args(C, kind, bounds, scale, gamma=None, jump_every=0, stretch_a=2.0, burn=0, **subspace):
    """What run and run_tempered refuse alike about the ensemble and its proposal; returns (scale with kind="de"'s default, the
    subspace move's settings or None).  subspace: pairs, ncr, e_width, pcr, adapt_cr as run takes them -- kind="subspace"'s alone."""
    if C < 4 or C % 2:
        raise ValueError("C=%d: the two halves of the ensemble need an even number of chains, at least 4" % C)
    if kind not in ("de", "rw", "stretch", "subspace"):
        raise ValueError("kind must be 'de', 'rw', 'stretch' or 'subspace'")
    if bounds not in ("reject", "fold"):
        raise ValueError("bounds must be 'reject' or 'fold'")
    sub = dict(_SUBSPACE_DEFAULTS, **subspace)
    if kind != "subspace":
        for name, default in _SUBSPACE_DEFAULTS.items():
            given = sub[name]
            if not (given is default or (isinstance(default, (int, float)) and not isinstance(given, bool) and np.isscalar(given)
                                         and given == default)):
                raise ValueError("%s belongs to kind='subspace'; kind=%r has none" % (name, kind))
    if kind == "stretch":
        if gamma is not None or scale is not None or int(jump_every) != 0:
            raise ValueError("kind='stretch' has no gamma, scale or jump_every: the move's only parameter is stretch_a")
        if bounds != "reject":
            raise ValueError("kind='stretch' needs bounds='reject': a reflected stretch is not reversible")
        if not (np.isfinite(stretch_a) and stretch_a > 1.0):
            raise ValueError("stretch_a=%r must be finite and > 1" % (stretch_a,))
        return 0.0, None
    if scale is None:
        if kind == "rw":
            raise ValueError("kind='rw' needs scale, the half-width of the random walk")
        scale = 1e-3
    if kind != "subspace":
        return scale, None
    pairs, ncr, e_width = sub["pairs"], sub["ncr"], sub["e_width"]
    if isinstance(pairs, bool) or not (isinstance(pairs, (int, np.integer)) and 1 <= pairs <= _abi.MCMC_MAX_PAIRS):
        raise ValueError("pairs=%r must be an integer in [1, %d]" % (pairs, _abi.MCMC_MAX_PAIRS))
    if isinstance(ncr, bool) or not (isinstance(ncr, (int, np.integer)) and 1 <= ncr <= _abi.MCMC_MAX_CR):
        raise ValueError("ncr=%r must be an integer in [1, %d]" % (ncr, _abi.MCMC_MAX_CR))
    if not (isinstance(e_width, (int, float, np.floating)) and 0.0 <= e_width < 1.0):
        raise ValueError("e_width=%r must be in [0, 1)" % (e_width,))
    if gamma is not None and not np.isfinite(gamma):
        raise ValueError("gamma=%r, the factor on the subspace move's table, must be finite" % (gamma,))
    if not (sub["adapt_cr"] is False or sub["adapt_cr"] is True):
        raise ValueError("adapt_cr must be False or True")
    if sub["adapt_cr"] and int(burn) < 1:
        raise ValueError("adapt_cr=True adapts the crossover shares during the burn sweeps only: burn must be >= 1")
    pcr = _pcr_arg(sub["pcr"], int(ncr))
    return scale, dict(pairs=int(pairs), ncr=int(ncr), e_width=float(e_width), adapt=sub["adapt_cr"], burn=int(burn),
                       pcr=np.full(int(ncr), 1.0 / int(ncr)) if pcr is None else pcr / pcr.sum())


def adapted_pcr(jump, tried, ncr):
    """(ncr,): the crossover shares of adapt_cr from the squared jump summed per class and the proposals tried per class: proportional
    to the mean squared jump per proposal (a class not tried yet takes the mean of the others; a total of zero gives equal shares),
    floored at 1 / (10 ncr) and then renormalised -- so no share ends below (1 / (10 ncr)) / 1.1."""
    jump, tried = np.asarray(jump, dtype=np.float64), np.asarray(tried)
    mean = np.full(ncr, np.nan)
    mean[tried > 0] = jump[tried > 0] / tried[tried > 0]
    mean[tried <= 0] = mean[tried > 0].mean() if np.any(tried > 0) else 1.0
    total = mean.sum()
    q = mean / total if total > 0.0 and np.isfinite(total) else np.full(ncr, 1.0 / ncr)
    q = np.maximum(q, 1.0 / (10.0 * ncr))
    return q / q.sum()


def _prior_args(prior, A):
    """prior=(mean_u, sd_u) of run and run_tempered as two (A,) arrays, or None."""
    if prior is None:
        return None
    mean, sd = (_f64(v) for v in prior)
    if mean.shape != (A,) or sd.shape != (A,):
        raise ValueError("prior must be (mean_u, sd_u), each (A,) with the box's A = %d active columns" % A)
    if not (np.all(np.isfinite(mean)) and np.all(sd > 0.0)):
        raise ValueError("prior: every mean must be finite and every sd > 0 (inf: a flat column)")
    return mean, sd


def _early_reject_arg(early_reject):
    """run's early_reject: False, True (a level per system, cut_levels) or "sample" (the level as the sample's budget, cut_budget)."""
    if not (early_reject is False or early_reject is True or (isinstance(early_reject, str) and early_reject == "sample")):
        raise ValueError("early_reject must be False, True or \"sample\", got %r" % (early_reject,))
    return early_reject


def _subspace_info(info, subspace, n):
    """What info receives about kind="subspace" from _sweeps' counters."""
    if subspace is not None:
        info.update(pairs=subspace["pairs"], ncr=subspace["ncr"], pcr=n["pcr"].tolist(), mean_dsel=n["dsel"])
        if subspace["adapt"]:
            info.update(pcr_trace=n["pcr_trace"])


def _active(lo, hi, sim_flags):
    A = refine.active_columns(lo, hi, sim_flags).size
    if not 1 <= A <= _abi.REFINE_MAX_DIMS:
        raise ValueError("the box has %d active columns; a chain takes 1 .. %d" % (A, _abi.REFINE_MAX_DIMS))
    return A


def _sweeps(loglik, U, X, LL, *, box, sim_flags, sweeps, kind, gamma, scale, jump_every, seed, kept, device, fold, early_reject, tf=None,
            ladder=None, swap_every=1, stretch_a=2.0, prior=None, subspace=None):
    """The sweeps of run (tf: the C rows of U, X, LL as run holds them, the single-temperature front ends) and of run_tempered
    (ladder (K,): the 2 K g rows half-major, the *_rungs front ends and the swap).  The state is advanced in place.  Returns the
    history -- U, X, LL, accept, each (K, n, C, ..), K = 1 for run -- and the counters: accept (sweeps, K) the share of chains that
    moved, outside, folded, levelled, solved (K,) proposals, tried, done (K - 1,) exchanges.

    kind="stretch" or a prior makes every half-sweep a Metropolis-Hastings step: it forms h (count,) -- propose_stretch's lnq, plus
    prior_term -- and goes through accept_h and reject_levels_h, which take a ladder of one for run.  A proposal whose h is NaN or
    -inf is not solved and counts as outside.  With neither, the calls are exactly the ones above.

    kind="subspace" (subspace: _proposal_args' settings) proposes with propose_subspace, its table subspace_gamma_table times gamma; a
    jump sweep is propose / propose_rungs with gamma = 1, all coordinates.  The counters then also hold dsel, the mean number of
    coordinates a subspace proposal moved, pcr (ncr,) the shares the kept sweeps ran with and pcr_trace (sweeps, ncr) the shares of
    every sweep.  With adapt the sweeps t < burn sum, per class, the squared jump of the accepted proposals in units of the rung's
    current deviation per column, and the proposals tried; adapted_pcr of the two replaces the shares after each such sweep."""
    lo, hi, lg = box
    hastings = kind == "stretch" or prior is not None
    level_kw = "cut_budget" if early_reject == "sample" else "cut_levels"       # the level is per system, or the sample's budget
    K = 1 if ladder is None else ladder.size
    half, A = U.shape[0] // 2, U.shape[1]
    g, C = half // K, 2 * half // K
    levels_of, accept_of, temper = (reject_levels, accept, tf) if ladder is None else (reject_levels_rungs, accept_rungs, ladder)
    ladder_h = np.array([float(tf)]) if ladder is None else ladder
    if K == 1:                                                   # one rung: the rows are the rung
        rung_major, per_rung = (lambda a: a[None]), np.count_nonzero
    else:
        def rung_major(a):                                       # (2 K g, ...) -> (K, C, ...)
            return a.reshape((2, K, g) + a.shape[1:]).swapaxes(0, 1).reshape((K, C) + a.shape[1:])

        def per_rung(flags):                                     # (K g,) flags of a block's rows -> how many are set in each rung
            return flags.reshape(K, g).sum(axis=1)

    gamma0 = 2.38 / np.sqrt(2.0 * A) if gamma is None else float(gamma)
    if subspace is not None:
        tab = subspace_gamma_table(subspace["pairs"], A, 1.0 if gamma is None else float(gamma))
        ncr, pcr = subspace["ncr"], subspace["pcr"]
        pcr_trace, dsel_sum, dsel_n = np.empty((sweeps, ncr)), 0, 0
        jump, tried_cr = np.zeros(ncr), np.zeros(ncr, dtype=np.int64)
    hU, hX = np.empty((K, len(kept), C, A)), np.empty((K, len(kept), C, lo.size))
    hLL, hAcc = np.empty((K, len(kept), C)), np.empty((K, len(kept), C), dtype=bool)
    shares, tried, done = np.empty((sweeps, K)), np.zeros(K - 1, dtype=np.int64), np.zeros(K - 1, dtype=np.int64)
    outside, folded, levelled, solved = (np.zeros(K, dtype=np.int64) for _ in range(4))
    moved, row = np.empty(2 * half, dtype=bool), 0
    for t in range(sweeps):
        jumping = jump_every > 0 and (t + 1) % jump_every == 0
        gm = 1.0 if jumping else gamma0
        adapting = subspace is not None and subspace["adapt"] and t < subspace["burn"] and not jumping
        if subspace is not None:
            pcr_trace[t] = pcr
        for h, (a, b) in enumerate(((0, half), (half, 2 * half))):
            step = 2 * t + h                                     # with chain0 = a, the key of the half-sweep's calls
            hh = None
            if subspace is not None and not jumping:
                Up, Xp, inside, mask, sel = propose_subspace(U[a:b], U[half:] if h == 0 else U[:half], g, tab, scale, a, seed, step, lo, hi,
                                                             lg, ncr, pcr, subspace["e_width"], sim_flags, device=device, fold=fold)
                dsel_sum += int(np.unpackbits(np.ascontiguousarray(mask).view(np.uint8)).sum())
                dsel_n += half
                if adapting:                                     # the deviation of each rung's ensemble as it stands, both halves
                    sd = rung_major(U).std(axis=1)
                    before = U[a:b].copy()
            elif kind == "stretch":
                Up, Xp, inside, _, hh = propose_stretch(U[a:b], U[half:] if h == 0 else U[:half], g, stretch_a, a, seed, step, lo, hi, lg,
                                                        sim_flags, device=device)
            elif kind == "rw":
                Up, Xp, inside = propose(U[a:b], None, gm, scale, a, seed, step, lo, hi, lg, sim_flags, device=device, fold=fold)
            elif ladder is None:                                 # "de", and the jump sweep of "subspace"
                Up, Xp, inside = propose(U[a:b], U[half:] if h == 0 else U[:half], gm, scale, a, seed, step, lo, hi, lg, sim_flags,
                                         device=device, fold=fold)
            else:
                Up, Xp, inside = propose_rungs(U[a:b], U[half:] if h == 0 else U[:half], g, gm, scale, a, seed, step, lo, hi, lg,
                                               sim_flags, device=device, fold=fold)
            ok = inside != 0
            if prior is not None:
                hh = prior_term(U[a:b], Up, prior[0], prior[1], hh, device=device)
            if hastings:
                ok &= ~np.isnan(hh) & (hh > -np.inf)
            LLp = np.full(half, -np.inf)
            if ok.any() and early_reject:
                if hastings:                                     # a level below 0 cuts what sse >= 0 has decided already
                    levels = np.maximum(reject_levels_h(LL[a:b], hh, ladder_h, a, seed, step, device=device), 0.0)
                else:
                    levels = levels_of(LL[a:b], temper, a, seed, step, device=device)
                LLp[ok] = _f64(loglik(np.ascontiguousarray(Xp[ok]), **{level_kw: levels[ok]}))
                levelled += per_rung(ok & np.isfinite(levels))
                solved += per_rung(ok)
            elif ok.any():
                LLp[ok] = _f64(loglik(np.ascontiguousarray(Xp[ok])))
            outside += per_rung(~ok)
            folded += per_rung(inside == 2)
            if hastings:
                moved[a:b] = accept_h(U[a:b], X[a:b], LL[a:b], Up, Xp, LLp, inside, hh, ladder_h, a, seed, step, device=device) != 0
            else:
                moved[a:b] = accept_of(U[a:b], X[a:b], LL[a:b], Up, Xp, LLp, inside, temper, a, seed, step, device=device) != 0
            if adapting:
                with np.errstate(invalid="ignore", divide="ignore"):
                    z2 = (((U[a:b] - before) / np.repeat(sd, g, axis=0)) ** 2).sum(axis=1)      # a rejected chain has not moved: zero
                cls = sel >> 8
                jump += np.bincount(cls, weights=np.where(np.isfinite(z2), z2, 0.0), minlength=ncr)[:ncr]
                tried_cr += np.bincount(cls, minlength=ncr)[:ncr]
        if adapting:
            pcr = adapted_pcr(jump, tried_cr, ncr)
        shares[t] = rung_major(moved).mean(axis=1)
        if K > 1 and (t + 1) % swap_every == 0:
            parity = (t // swap_every) % 2
            for a, b in ((0, half), (half, 2 * half)):
                sw = swap(U[a:b], X[a:b], LL[a:b], ladder, parity, a, seed, t, device=device)
                lower = np.arange(parity, K - 1, 2)
                tried[lower] += g
                done[lower] += sw.reshape(K, g)[lower].sum(axis=1)
        if t >= kept.start and (t - kept.start) % kept.step == 0:
            hU[:, row], hX[:, row], hLL[:, row], hAcc[:, row] = rung_major(U), rung_major(X), rung_major(LL), rung_major(moved)
            row += 1
    n = dict(accept=shares, outside=outside, folded=folded, levelled=levelled, solved=solved, tried=tried, done=done)
    if subspace is not None:
        n.update(dsel=dsel_sum / float(max(dsel_n, 1)), pcr=pcr, pcr_trace=pcr_trace)
    return (hU, hX, hLL, hAcc), n


def run(loglik, X0, LL0, minX, maxX, do_log, sim_flags=None, sweeps=1000, tf=1.0, kind="de", gamma=None, scale=None, jump_every=0,
        seed=1, keep_every=1, burn=0, max_history_bytes=4 << 30, device=0, info=None, U0=None, bounds="reject", stretch_a=2.0, prior=None,
        pairs=3, ncr=3, e_width=0.05, pcr=None, adapt_cr=False, early_reject=False):
    """Advance the C chains that start at X0 (C, ncol), LL0 (C,) by `sweeps` sweeps; loglik(X) -> LL is any callable (the fused
    likelihood, a toy).  Returns Chains: the states after the sweeps burn, burn + keep_every, ...

    One sweep updates the chains [0, C / 2) with the chains [C / 2, C) as partners (step = 2 t, chain0 = 0), then the chains [C / 2,
    C) with the already updated first half (step = 2 t + 1, chain0 = C / 2).  bounds="reject": loglik is called on the proposals
    inside the cube only; the others get LLp = -inf and are rejected.  bounds="fold": a proposal that leaves the cube is reflected
    back at its faces (propose(fold=True)) and solved like any other; only one with a coordinate that is not finite is left out.

    kind="de": differential evolution, gamma defaulting to 2.38 / sqrt(2 A) and, with jump_every > 0, 1.0 on every jump_every-th
    sweep (a jump between modes); scale (the uniform jitter's half-width, a scalar or (A,)) defaults to 1e-3.  kind="rw": the random
    walk of half-width scale, which must be given; no partners.  U0 (C, A): the unit coordinates of X0 when they are at hand (start
    returns them); default refine.unit_coords(X0).

    kind="stretch": the affine-invariant stretch move (Goodman & Weare 2010; propose_stretch) with stretch_a > 1, default 2: each
    chain moves along the line through one chain of the other half, u' = p + z (u - p), and the factor z^(A - 1) enters the accept
    step as its Hastings term (accept_h).  It has no other parameter: gamma, scale and jump_every must be left at their defaults, and
    bounds must be "reject" (a reflected stretch is not reversible); ValueError otherwise.  info receives stretch_a.

    kind="subspace": DREAM's move (Vrugt et al. 2009; propose_subspace): each proposal moves a random subset of the coordinates --
    a crossover class m of ncr is drawn with the shares pcr (default equal), each coordinate is selected with probability (m + 1) /
    ncr -- along the sum of delta difference pairs of the other half, delta uniform in 1 .. pairs, with gamma * 2.38 / sqrt(2 delta
    dsel) for the dsel selected coordinates (gamma: a factor, default 1) times 1 + e_width (2 v - 1), plus the jitter of half-width
    scale (default as for "de").  The move is symmetric: both bounds, prior, every early_reject and jump_every apply as for "de"; a
    jump sweep is "de"'s with gamma = 1 and moves all coordinates.  pairs, ncr, e_width, pcr and adapt_cr belong to this kind alone
    (ValueError with another).  info receives pairs, ncr, pcr (the shares of the kept sweeps) and mean_dsel, the mean number of
    coordinates a proposal moved.
    adapt_cr=True adapts the shares as DREAM does, during the burn sweeps ONLY: each of them adds, per class, the squared jump of the
    accepted proposals -- sum_d ((u_new_d - u_old_d) / sd_d)^2 with sd_d the current ensemble's deviation of column d; a rejected
    chain counts zero -- and the proposals tried, and sets pcr_m proportional to the mean squared jump per proposal of class m,
    floored at 1 / (10 ncr) before renormalising (adapted_pcr).  The shares are frozen after the last burn sweep, so the kept sweeps
    are a Markov chain with a fixed kernel that leaves the posterior invariant; the burn sweeps, whose kernel depends on the history,
    are not, and are discarded for that reason.  burn = 0 with adapt_cr=True is a ValueError.  info also receives pcr_trace (sweeps,
    ncr), the shares every sweep ran with.

    prior=(mean_u, sd_u), each (A,): an independent Gaussian prior in the unit coordinates of the active columns on top of the
    uniform one on the cube (gaussian_prior makes the pair from a centre and widths in the box's units; sd inf is a flat column).
    Valid with every kind and both bounds.  Its log ratio enters the accept step untempered (prior_term, accept_h): Chains.LL stays
    the likelihood alone, so early_reject and tf keep their meaning.  A prior whose widths are all inf gives the Chains of the run
    without it, bit for bit.

    early_reject=True (Solonen et al. 2012): each half-sweep computes reject_levels of its chains from their current LL and calls
    loglik(Xp[ok], cut_levels=levels[ok]), so a proposal whose running squared error makes its rejection certain stops being
    solved (trpl_loglik_cut_levels).  The callable must accept that keyword, one level per row, and its LL must be minus the summed
    sse of a P started from zero (driver.loglik with P=None); LL0 must come from such a call too.  accept is called unchanged, and
    the returned Chains are bit for bit those of the run without it: a cut proposal is one that run rejects.  info then also
    receives early_reject, the share of solved proposals that were given a finite level.

    early_reject="sample": the same levels, passed as loglik(Xp[ok], cut_budget=levels[ok]) -- the level is one for the proposal's
    summed sse, so it is spent across the curves (trpl_loglik_cut_budget; the callable chooses curves_per_launch) instead of being
    given to each curve whole: a proposal stops once its curves together decide its rejection.  A cut proposal's total is at or
    above its level, which accept rejects, so the Chains are again those of the run without it, bit for bit.  Any other value than
    False, True or "sample" is a ValueError.

    The history of n kept sweeps takes n C (A + ncol + 1) 8 + n C bytes; a run whose history would exceed max_history_bytes raises
    ValueError before anything is solved.  ValueError for an odd C or C < 4, or a bounds that is neither string.  info receives
    accept (the share of chains that moved, per sweep), outside (the share of all proposals that were not solved: those that left
    the cube, or under bounds="fold" the non-finite ones, normally 0.0) and folded (the share of all proposals that were reflected
    back: 0.0 under bounds="reject")."""
    early_reject = _early_reject_arg(early_reject)
    X, LL = np.array(X0, dtype=np.float64, order="C"), np.array(LL0, dtype=np.float64, order="C")
    lo, hi, lg = _box(minX, maxX, do_log)
    if X.ndim != 2 or X.shape[1] != lo.size or LL.shape != (X.shape[0],):
        raise ValueError("X0 must be (C, ncol) and LL0 (C,)")
    C = X.shape[0]
    scale, subspace = _proposal_args(C, kind, bounds, scale, gamma, jump_every, stretch_a, burn=burn, pairs=pairs, ncr=ncr, e_width=e_width,
                                     pcr=pcr, adapt_cr=adapt_cr)
    sweeps, keep_every, burn = int(sweeps), int(keep_every), int(burn)
    if sweeps < 1 or keep_every < 1 or burn < 0:
        raise ValueError("sweeps and keep_every must be >= 1 and burn >= 0")
    A = _active(lo, hi, sim_flags)
    prior = _prior_args(prior, A)
    kept = range(burn, sweeps, keep_every)
    need = len(kept) * C * ((A + lo.size + 1) * 8 + 1)
    if need > int(max_history_bytes):
        raise ValueError("the history of %d sweeps x %d chains needs %d bytes, more than max_history_bytes = %d"
                         % (len(kept), C, need, int(max_history_bytes)))
    if U0 is None:
        U, _ = refine.unit_coords(X, lo, hi, lg, sim_flags, device=device)
    else:
        U = np.array(U0, dtype=np.float64, order="C")
        if U.shape != (C, A):
            raise ValueError("U0 must be (C, A) with the box's A = %d active columns" % A)
    hist, n = _sweeps(loglik, U, X, LL, tf=tf, box=(lo, hi, lg), sim_flags=sim_flags, sweeps=sweeps, kind=kind, gamma=gamma, scale=scale,
                      jump_every=int(jump_every), seed=seed, kept=kept, device=device, fold=bounds == "fold", early_reject=early_reject,
                      stretch_a=float(stretch_a), prior=prior, subspace=subspace)
    if info is not None:
        if kind == "stretch":
            info.update(stretch_a=float(stretch_a))
        _subspace_info(info, subspace, n)
        info.update(accept=n["accept"][:, 0].tolist(), outside=int(n["outside"][0]) / float(sweeps * C),
                    folded=int(n["folded"][0]) / float(sweeps * C))
        if early_reject:
            info.update(early_reject=int(n["levelled"][0]) / float(max(int(n["solved"][0]), 1)))
    return Chains(*(h[0] for h in hist), device=device)


class Tempered:
    """The kept history of run_tempered: ladder (K,) the temperatures, rung(k) the Chains of rung k in run's (n, C, A) layout,
    swap_rate (K - 1,) the share of the proposed exchanges between rungs k and k + 1 that took place (NaN where none was proposed)."""

    def __init__(self, ladder, chains, swap_rate):
        self.ladder, self._chains, self.swap_rate = ladder, chains, swap_rate

    def rung(self, k):
        return self._chains[k]

    def samples(self, burn=0, thin=1):
        """rung(0).samples(burn, thin): ladder[0] is the temperature the caller asked for."""
        return self._chains[0].samples(burn, thin)

    def log_evidence(self, burn=0, blocks=16, base=None):
        """The log-evidence estimates of the run (log_evidence_ratios has the rule and the keys): the kept LL of the K rungs from the
        kept sweep `burn` on, in `blocks` blocks of consecutive sweeps for the jackknife errors, through one evidence_sums call --
        the hot rungs' histories give every ratio Z(ladder[k]) / Z(ladder[k + 1]) without another solve.  The oldest kept sweeps
        after burn are dropped until `blocks` divides the range: dropped says how many, t0 and t1 are the range.  K = 1: no call,
        empty ratios and totals of 0.0.

        base = (LL, tf_hot_check) or (LL, tf_hot_check, log_ratio) of an importance run -- the uniform first generation, or a
        refined Population's log_ratio() -- anchors the ladder: base_ln_z = posterior.log_evidence(LL, ladder[-1], log_ratio) is ln Z
        at the hottest rung (base_se, base_ess beside it), and ln_z = dict(forward, reverse, ti) the absolute ln Z(ladder[0]) =
        base_ln_z + <name>_total, ln_z_se the two errors in quadrature.  tf_hot_check must be ladder[-1] (ValueError): the base is
        only trustworthy at the temperature its effective sample size was checked at (posterior.tf_for_ess).  A Gaussian prior= of
        the run is common to the rungs and cancels in every ratio; only the base needs it: pass log_ratio = -ln p(u) of the
        base's draws (plus the Population's log_ratio, if refined)."""
        K, burn, blocks = len(self._chains), int(burn), int(blocks)
        if base is not None:
            if len(base) not in (2, 3):
                raise ValueError("base must be (LL, tf_hot_check) or (LL, tf_hot_check, log_ratio)")
            if float(base[1]) != float(self.ladder[-1]):
                raise ValueError("tf_hot_check = %r is not the hottest rung's temperature ladder[-1] = %r" % (float(base[1]), float(self.ladder[-1])))
        n = self._chains[0].LL.shape[0]
        if burn < 0 or blocks < 1 or n - burn < blocks:
            raise ValueError("blocks=%d must be >= 1 and at most the %d kept sweeps left after burn=%d" % (blocks, max(n - burn, 0), burn))
        dropped = (n - burn) % blocks
        t0 = burn + dropped
        if K == 1:
            ext, sums = np.full((1, 2), np.nan), np.zeros((1, blocks, _abi.MCMC_EVIDENCE_SUMS))
        else:
            ext, sums = evidence_sums(np.stack([c.LL for c in self._chains]), self.ladder, t0, n, blocks, device=self._chains[0].device)
        out = log_evidence_ratios(ext, sums, self.ladder)
        out.update(dropped=dropped, t0=t0, t1=n)
        if base is not None:
            ln_z, binfo = posterior.log_evidence(base[0], float(self.ladder[-1]), base[2] if len(base) == 3 else None,
                                                 device=self._chains[0].device)
            out.update(base_ln_z=ln_z, base_se=binfo["se"], base_ess=binfo["ess"],
                       ln_z={name: ln_z + out[name + "_total"] for name in ("forward", "reverse", "ti")},
                       ln_z_se={name: float(np.sqrt(out[name + "_total_se"] ** 2 + binfo["se"] ** 2)) for name in ("forward", "reverse", "ti")})
        return out


def run_tempered(loglik, X0, LL0, minX, maxX, do_log, ladder, sim_flags=None, sweeps=1000, swap_every=1, kind="de", gamma=None,
                 scale=None, jump_every=0, seed=1, keep_every=1, burn=0, max_history_bytes=4 << 30, device=0, info=None, U0=None,
                 bounds="reject", stretch_a=2.0, prior=None, pairs=3, ncr=3, e_width=0.05, pcr=None, adapt_cr=False, early_reject=False):
    """Parallel tempering (replica exchange: Swendsen & Wang 1986, Geyer 1991): K = len(ladder) copies of run's
    ensemble of C chains, rung k at temperature ladder[k], advanced together, and states of adjacent rungs exchanged by the
    Metropolis rule of swap().  The hot rungs cross between separated modes; the exchange carries that down to rung 0, whose
    temperature ladder[0] is the one the caller wants.  Returns Tempered.

    X0 (C, ncol) and LL0 (C,) start every rung from the same states; X0 (K, C, ncol) and LL0 (K, C) give each rung its own (U0
    likewise (C, A) or (K, C, A)).  The state is held half-major: with g = C / 2, row h K g + k g + c is chain c of half h of rung
    k, so the first halves of all rungs are one contiguous block and the second halves the other, and the row index keys Philox.
    One half-sweep is one propose_rungs over a block with the other block as partners (kind="rw": propose over the block),
    optionally one reject_levels_rungs, ONE call of loglik on the proposals of all rungs that are to be solved, and one
    accept_rungs; step and chain0 are run's (2 t + h, the block's first row).  After every swap_every-th sweep t (t + 1 a multiple
    of swap_every) each block gets one swap with parity = (t // swap_every) % 2, step = t and chain0 the block's first row.  With
    ladder = [tf] no swap is called and rung(0) is run(..., tf=tf)'s Chains bit for bit.  kind="stretch" takes each chain's partner
    from its own rung, kind="subspace" all its pairs (its shares pcr are common to the rungs, adapted on all of them together); a prior is common to the rungs and is not tempered, so it cancels in the swap, which is unchanged.

    The other keywords are run's.  Chains.accept of a rung is the Metropolis step's flag of the rung's slots; an exchange does not
    count as a move.  The history takes n K C (A + ncol + 1) 8 + n K C bytes and is refused above max_history_bytes before anything
    is solved.  info receives run's keys per rung -- accept (sweeps, K), outside (K,), folded (K,), early_reject (K,) -- and
    swap_rate (K - 1,)."""
    early_reject = _early_reject_arg(early_reject)
    ladder = np.array(ladder, dtype=np.float64, order="C")
    if ladder.ndim != 1 or not 1 <= ladder.size <= _abi.MCMC_MAX_RUNGS:
        raise ValueError("ladder must be (K,), 1 <= K <= %d temperatures" % _abi.MCMC_MAX_RUNGS)
    if not np.all(np.isfinite(ladder) & (ladder > 0.0)):
        raise ValueError("every temperature of the ladder must be finite and > 0")
    K = ladder.size
    X, LL = np.array(X0, dtype=np.float64, order="C"), np.array(LL0, dtype=np.float64, order="C")
    lo, hi, lg = _box(minX, maxX, do_log)
    if X.ndim == 2 and LL.ndim == 1:
        X, LL = np.broadcast_to(X, (K,) + X.shape), np.broadcast_to(LL, (K,) + LL.shape)
    if X.ndim != 3 or X.shape[0] != K or X.shape[2] != lo.size or LL.shape != X.shape[:2]:
        raise ValueError("X0 must be (C, ncol) and LL0 (C,), or (K, C, ncol) and (K, C) with the ladder's K = %d" % K)
    C = X.shape[1]
    scale, subspace = _proposal_args(C, kind, bounds, scale, gamma, jump_every, stretch_a, burn=burn, pairs=pairs, ncr=ncr, e_width=e_width,
                                     pcr=pcr, adapt_cr=adapt_cr)
    sweeps, keep_every, burn, swap_every = int(sweeps), int(keep_every), int(burn), int(swap_every)
    if sweeps < 1 or keep_every < 1 or burn < 0 or swap_every < 1:
        raise ValueError("sweeps, keep_every and swap_every must be >= 1 and burn >= 0")
    A = _active(lo, hi, sim_flags)
    prior = _prior_args(prior, A)
    kept = range(burn, sweeps, keep_every)
    need = len(kept) * K * C * ((A + lo.size + 1) * 8 + 1)
    if need > int(max_history_bytes):
        raise ValueError("the history of %d sweeps x %d rungs x %d chains needs %d bytes, more than max_history_bytes = %d"
                         % (len(kept), K, C, need, int(max_history_bytes)))

    def half_major(a):                                           # (K, C, ...) -> (2 K g, ...), a writeable copy
        return np.array(a.reshape((K, 2, C // 2) + a.shape[2:]).swapaxes(0, 1).reshape((K * C,) + a.shape[2:]), order="C")

    X, LL = half_major(X), half_major(LL)
    if U0 is None:
        U, _ = refine.unit_coords(X, lo, hi, lg, sim_flags, device=device)
    else:
        U = np.array(U0, dtype=np.float64, order="C")
        if U.shape == (C, A):
            U = np.broadcast_to(U, (K, C, A))
        if U.shape != (K, C, A):
            raise ValueError("U0 must be (C, A) or (K, C, A) with the box's A = %d active columns" % A)
        U = half_major(U)
    hist, n = _sweeps(loglik, U, X, LL, ladder=ladder, swap_every=swap_every, box=(lo, hi, lg), sim_flags=sim_flags, sweeps=sweeps, kind=kind,
                      gamma=gamma, scale=scale, jump_every=int(jump_every), seed=seed, kept=kept, device=device, fold=bounds == "fold",
                      early_reject=early_reject, stretch_a=float(stretch_a), prior=prior, subspace=subspace)
    with np.errstate(invalid="ignore"):
        swap_rate = n["done"] / n["tried"].astype(np.float64)
    if info is not None:
        if kind == "stretch":
            info.update(stretch_a=float(stretch_a))
        _subspace_info(info, subspace, n)
        info.update(accept=n["accept"], outside=n["outside"] / float(sweeps * C), folded=n["folded"] / float(sweeps * C), swap_rate=swap_rate)
        if early_reject:
            info.update(early_reject=n["levelled"] / np.maximum(n["solved"], 1).astype(np.float64))
    return Tempered(ladder, [Chains(*(h[k] for h in hist), device=device) for k in range(K)], swap_rate)
