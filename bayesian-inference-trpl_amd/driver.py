"""Host control loop: the semantics of bayeslib.simulate / bayes (bayeslib.py:83-252) over the
gfx950 kernels, plus the fused single-call likelihood the reference does not have.

Two paths compute the same P:
  * unfused (drop-in order of operations): model -> fastlog -> [time interpolation] -> prob per
    curve x sample block x experiment, exactly the reference's loop nest and dtypes;
  * fused (`loglik`): one launch per experiment, PL never leaves the registers; usable when
    every observation time grid is a prefix of the simulation grid (the shipped example data).
"""
import math
import os
import sys
import time

import numpy as np

from . import _abi
from .likelihood import fastlog, prob, weights_from_uncertainty
from .model import pvSim
from .sampler import make_grid


def almost_equal(x, x0, threshold=1e-10):
    """bayeslib.almost_equal (bayeslib.py:78-81)."""
    x = np.asarray(x)
    x0 = np.asarray(x0)
    if x.shape != x0.shape:
        return False
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(np.abs(np.nanmax((x - x0) / x0)) < threshold)


def is_grid_prefix(times, sim_t, threshold=1e-10):
    """True when `times` coincides with the first len(times) points of the simulation grid."""
    times = np.asarray(times, dtype=float)
    n = len(times)
    if n < 1 or n > len(sim_t):
        return False
    ref = sim_t[:n]
    scale = np.maximum(np.abs(ref), np.abs(sim_t[1]) if len(sim_t) > 1 else 1.0)
    return bool(np.all(np.abs(times - ref) <= threshold * scale))


def observations_on_grid(times, sim_t, literal=False):
    """How the fused level routes one curve's observation times.  True: compared point by point with the first
    len(times) simulation columns (entry points trpl_loglik / the on-grid form of trpl_loglik_from_pl_dev); False:
    interpolated in the kernel (trpl_loglik_obs / the bracket form).  Default rule: a PREFIX of the simulation grid is on
    the grid.  literal (gpu_info["interpolate_prefix"]): the reference's own test -- only the FULL grid bypasses the
    interpolation (bayeslib.py:173,:182-183), a prefix goes through it like any other set of times (:184-191)."""
    if literal:
        return almost_equal(sim_t, np.asarray(times, dtype=float))
    return is_grid_prefix(times, sim_t)


def fused_entry_point(exp_times, sim_t, num_curves, literal=False):
    """Name of the C entry point driver.simulate's fused level calls for one experiment (single-experiment branch): every
    curve on the grid -> "trpl_loglik", else "trpl_loglik_obs".  bench.py labels its e2e record with it."""
    on = all(observations_on_grid(exp_times[c], sim_t, literal) for c in range(num_curves))
    return "trpl_loglik" if on else "trpl_loglik_obs"


def _interp_rows_numpy(sim_t, pl, times):
    """interp_rows in NumPy: the arithmetic trpl_interp_rows restates (and the route for matrices it does not take)."""
    hi = np.clip(np.searchsorted(sim_t, times), 1, len(sim_t) - 1)
    lo = hi - 1
    slope = (pl[:, hi] - pl[:, lo]) / (sim_t[hi] - sim_t[lo])[None, :]
    return np.ascontiguousarray(slope * (times - sim_t[lo])[None, :] + pl[:, lo], dtype=np.float64)


def interp_rows(sim_t, pl, times):
    """1-D linear interpolation of every row of `pl` from sim_t onto `times`; the arithmetic of scipy's interp1d / griddata,
    which the reference applies row by row (bayeslib.py:186-189): slope = (y_hi - y_lo) / (x_hi - x_lo) with the difference
    taken in pl's own dtype (float32 for the reference's buffer), then slope * (x - x_lo) + y_lo in float64; NaN outside the
    grid.  Returns float64.  Row-contiguous float32 / float64 matrices go through trpl_interp_rows -- the same operations in
    plain host C++, bit for bit, without the interpreter lock, so the worker threads of simulate() interpolate side by side."""
    sim_t = np.asarray(sim_t, dtype=float)
    times = np.asarray(times, dtype=float)
    if (isinstance(pl, np.ndarray) and pl.ndim == 2 and pl.dtype in (np.float32, np.float64) and pl.shape[0] > 0
            and pl.strides[1] == pl.itemsize and pl.strides[0] % pl.itemsize == 0 and pl.strides[0] >= pl.shape[1] * pl.itemsize
            and pl.shape[1] == len(sim_t) and len(sim_t) >= 2 and len(times) > 0):
        hi, dx, h = bracket_times(sim_t, times)
        hi = np.ascontiguousarray(hi, dtype=np.int32)
        dx = np.ascontiguousarray(dx, dtype=np.float64)
        h = np.ascontiguousarray(h, dtype=np.float64)
        out = np.empty((pl.shape[0], len(times)), dtype=np.float64)
        _abi.check(_abi.lib().trpl_interp_rows(_abi.ptr(pl), pl.itemsize, pl.shape[0], pl.shape[1], pl.strides[0] // pl.itemsize,
                                               _abi.ptr(hi), _abi.ptr(dx), _abi.ptr(h), len(times), _abi.ptr(out), out.shape[1]))
    else:
        out = _interp_rows_numpy(sim_t, pl, times)
    outside = (times < sim_t[0]) | (times > sim_t[-1])
    out[:, outside] = np.nan
    return out


def bracket_times(sim_t, times):
    """The bracketing scipy's interp1d uses for linear interpolation (and griddata with it,
    bayeslib.py:189): hi = clip(searchsorted(x, x_new), 1, n-1), lo = hi - 1.  Returns
    (hi int32, x_new - x_lo, x_hi - x_lo)."""
    sim_t = np.asarray(sim_t, dtype=float)
    times = np.asarray(times, dtype=float)
    hi = np.clip(np.searchsorted(sim_t, times), 1, len(sim_t) - 1)
    lo = hi - 1
    return hi.astype(np.int32), times - sim_t[lo], sim_t[hi] - sim_t[lo]


DEFAULT_MAX_HOST_BYTES = 32 << 30      # gpu_info["max_host_bytes"]: what the results of the unfused overlapped path may hold at once


def unfused_curve_bytes(size, ncol, pl_dtype, n_interp, num_curves):
    """Host bytes of ONE (block, curve) result of the unfused path, as (full, done).  full: while it is being made -- the
    block's PL matrix (size x ncol in the caller's PL dtype, bayeslib.py:137) + a float64 interpolated copy (size x n_obs) per
    experiment whose times are off the grid (:184-191).  done: once it waits for prob() -- the same, minus the PL matrix when
    no experiment compares this curve on the grid (the matrix is then dropped as soon as it has been interpolated).
    n_interp: the n_obs of every (experiment, curve) that is interpolated, 0 for those compared on the grid,
    experiment-major; the largest curve counts."""
    n_interp = np.asarray(n_interp, dtype=np.int64).reshape(-1, max(int(num_curves), 1))
    pl = int(ncol) * np.dtype(pl_dtype).itemsize
    if not n_interp.size:
        return int(size) * pl, int(size) * pl
    interp = 8 * n_interp.sum(axis=0)                                     # per curve
    keeps_pl = (n_interp == 0).any(axis=0)                                # some experiment reads the PL matrix itself
    full = int(size) * int((pl + interp).max())
    done = int(size) * int(np.where(keeps_pl, pl + interp, interp).max())
    return full, done


def overlap_window(full, done, budget, num_curves):
    """How many (block, curve) results the overlapped unfused path may hold at once -- being made by a worker thread, waiting
    for prob(), or being consumed -- and how many worker threads make them: the largest window <= 2 * num_curves (this block's
    curves + the next block's) whose bytes, workers * full + (window - workers) * done, fit the budget.  (0, 0): not even two
    results fit -- the path then runs inline, one result at a time, like the reference (bayeslib.py:137)."""
    for w in range(2 * int(num_curves), 1, -1):
        workers = min(int(num_curves), 8, w - 1)
        if workers * full + (w - workers) * done <= budget:
            return w, workers
    return 0, 0


def loglik(X, init_params, lengths, Time, L, T, obs, tol=7, MAX=10000, plT=1, P=None, pl_f32=False,
           normalize=False, strict=False, device=0, info=None, times=None, fp32=False, devices=None, kernel=None,
           mixed=False, bundle=1, hist32=False, bdf_order=None, extra_flags=0, predict=False, mag_grid=None,
           mag_profile=False, weights=None, sse_cut=None, cut_levels=None, cut_budget=None, curves_per_launch=1):
    """Fused likelihood of one experiment (trpl_loglik / trpl_loglik_obs / trpl_loglik_multi).

    X (S,13) solver units; init_params (C,L) nm^-3; lengths scalar or (C,); obs = list of C
    arrays of log10 observations.  With times=None they sit on the first len(obs[c])
    simulation-grid points; otherwise times = list of C arrays of observation times in
    [0, Time] (any spacing), interpolated like the reference does (bayeslib.py:184-191).
    Accumulates into P (S,) if given (like probs.prob), else starts from zeros.  Returns P.
    devices: None = the single `device`; "all" = every visible device; or a list of device ordinals
    (contiguous sample shards, one per entry, run concurrently from this host thread).
    kernel: None (the library picks the stepper by launch size), "pair" or "single" (TRPL_FLAG_KERNEL_*).
    bundle: the reference's max_sims_per_block (TRPL_FLAG_BUNDLE; single-device calls only).
    bdf_order: cap the BDF order ramp at 1 .. 5 (TRPL_FLAG_BDF_ORDER); extra_flags: further TRPL_FLAG_* bits, ORed in
    (tests / measurements: _abi.FLAG_PAIR_ALWAYS_SEAM, _abi.FLAG_PAIR_ADJACENT, ...).
    predict: start each time step's iteration from the extrapolated history (TRPL_FLAG_PREDICT; opt-in, off by default:
    about half the solves; PL agrees with the default path to ~1e-9 median, within the tolerance include/trpl.h states).
    mag_grid: a sequence of M magnitude offsets ADDED to X[:, 12] -- the mag_grid loop of the reference's older
    likelihood (probs.lnP, probs.py:5-18) from ONE solve (trpl_loglik_moments + trpl_mag_grid): returns P (M, S), row m
    the likelihood at X[:, 12] + mag_grid[m] (accumulated into P if P (M, S) is given).  mag_profile=True (or
    "per_curve"): returns (best, P) -- the likelihood-maximising offset, (S,) or (C, S), and the likelihood there.
    Single-device calls only; info also receives esum and P, the one-offset likelihood trpl_loglik would return.
    weights: a list of C arrays shaped like obs (sorted together with times when off-grid), finite and >= 0 -- the
    uncertainty-weighted likelihood P[s] -= sum_c sum_i w_ci e_i^2 (trpl_loglik_weighted; likelihood.weights_from_uncertainty
    gives the chi-square weights 1 / (2 u^2) of probs.py:40).  A zero weight masks an observation.  info receives the weighted
    sse and esum and wsum (C,), the sum of each curve's weights.  Combines with mag_grid / mag_profile (trpl_mag_grid_w,
    trpl_mag_profile_w); single-device calls only.
    sse_cut: a float >= 0 (or +inf) routes to trpl_loglik_cut -- a system whose running squared error is above it after one
    of its 64-column batches stops there (include/trpl.h): its sse is the partial sum (> sse_cut), every other system's
    outputs are the plain call's bit for bit.  info also receives cut_col (C, S) (leading observations in a cut system's sum,
    -1 uncut, -2 flagged) and cut_fraction, the share of systems with cut_col >= 0.  Single-device calls on the plain FAST
    steppers only: not with mag_grid, mag_profile, weights, devices or bundle > 1.
    cut_levels: sse_cut with a level per system (trpl_loglik_cut_levels) -- (S,), one level per sample given to each of its
    curves, or (C, S); every level >= 0 or +inf.  System (c, s) reports what sse_cut = cut_levels[c, s] would make it report, bit
    for bit, whatever the other levels; info receives cut_col and cut_fraction as with sse_cut.  Excludes sse_cut and is refused
    with what sse_cut is refused with.  The levels of a Metropolis step: mcmc.reject_levels.
    cut_budget: (S,), every entry >= 0 or +inf -- a level for each sample's TOTAL sum_c sse[c, s], spent across its curves
    (trpl_loglik_cut_budget): the curves run as consecutive launches of curves_per_launch (1 .. 16) curves, and each launch's curves
    run at the level the budget leaves after what the earlier curves reported (include/trpl.h has the rule and its proof).  A sample
    with a cut system has a plain total >= its budget.  info receives cut_col and cut_fraction as with sse_cut, cut_level (C, S), the
    level every system ran at (-1: the sample was past its budget already), and cut_samples, the share of samples with any cut_col >=
    0.  curves_per_launch=1 is the tightest and serialises the curves; >= C is cut_levels with the budget as every curve's level.
    Excludes sse_cut and cut_levels and is refused with what those are refused with.
    """
    if cut_budget is not None:
        if sse_cut is not None or cut_levels is not None:
            raise ValueError("cut_budget, cut_levels and sse_cut exclude each other")
        cut_budget = np.ascontiguousarray(cut_budget, dtype=np.float64)
        curves_per_launch = int(curves_per_launch)
        if not 1 <= curves_per_launch <= 16:
            raise ValueError("curves_per_launch must be in [1, 16], got %d" % curves_per_launch)
    elif curves_per_launch != 1:
        raise ValueError("curves_per_launch goes with cut_budget")
    if cut_levels is not None:
        if sse_cut is not None:
            raise ValueError("cut_levels and sse_cut exclude each other")
        cut_levels = np.asarray(cut_levels, dtype=np.float64)
    if sse_cut is not None or cut_levels is not None or cut_budget is not None:
        word = "sse_cut" if sse_cut is not None else "cut_levels" if cut_levels is not None else "cut_budget"
        for name, on in (("mag_grid", mag_grid is not None), ("mag_profile", bool(mag_profile)), ("weights", weights is not None),
                         ("devices", devices is not None), ("bundle", int(bundle) != 1)):
            if on:
                raise ValueError("%s: not available with %s (trpl_loglik_cut runs the plain FAST steppers on one device)" % (word, name))
    if sse_cut is not None:
        sse_cut = float(sse_cut)
        if not sse_cut >= 0.0:
            raise ValueError("sse_cut must be >= 0 or +inf, got %r" % (sse_cut,))
    if weights is not None and devices is not None:
        raise ValueError("weights: not available with devices= (trpl_loglik_multi has no weighted form)")
    moments = mag_grid is not None or bool(mag_profile)
    if moments:
        if mag_grid is not None and mag_profile:
            raise ValueError("mag_grid and mag_profile exclude each other")
        if devices is not None:
            raise ValueError("mag_grid / mag_profile: not available with devices= (trpl_loglik_multi has no moments form)")
        P_out, P = P, None
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != 13:
        raise ValueError("X must have shape (S, 13)")
    S = X.shape[0]
    ini = np.ascontiguousarray(init_params, dtype=np.float64)
    if ini.ndim != 2 or ini.shape[1] != L:
        raise ValueError("init_params must have shape (C, L=%d), got %r" % (L, ini.shape))
    Cn = ini.shape[0]
    lengths = np.full(Cn, float(lengths)) if np.isscalar(lengths) else np.ascontiguousarray(lengths, dtype=float)
    if lengths.shape != (Cn,) or len(obs) != Cn or (times is not None and len(times) != Cn):
        raise ValueError("need one length and one observation set per curve")
    if weights is not None and len(weights) != Cn:
        raise ValueError("weights: need one array of weights per curve")
    n_obs = np.array([len(o) for o in obs], dtype=np.int64)
    obs_ld = int(n_obs.max())
    obs_mat = np.zeros((Cn, obs_ld))
    hi_mat = np.ones((Cn, obs_ld), dtype=np.int32)
    dx_mat = np.zeros((Cn, obs_ld))
    h_mat = np.ones((Cn, obs_ld))
    w_mat = np.zeros((Cn, obs_ld)) if weights is not None else None
    if times is not None:
        if plT != 1:
            raise ValueError("off-grid observation times need plT = 1")
        sim_t = np.linspace(0, Time, T + 1)                                   # bayeslib.py:115
    for c, o in enumerate(obs):
        o = np.asarray(o, dtype=float)
        if times is not None:
            tc = np.asarray(times[c], dtype=float)
            if tc.shape != o.shape:
                raise ValueError("curve %d: %d times for %d observations" % (c, len(tc), len(o)))
            if len(tc) and (tc.min() < sim_t[0] or tc.max() > sim_t[-1]):
                raise ValueError("curve %d: observation times outside [0, Time] (the reference would "
                                 "interpolate them to NaN)" % c)
            order = np.argsort(tc, kind="stable")
            tc, o = tc[order], o[order]
            hi_mat[c, :len(o)], dx_mat[c, :len(o)], h_mat[c, :len(o)] = bracket_times(sim_t, tc)
        obs_mat[c, :len(o)] = o
        if weights is not None:
            w = np.asarray(weights[c], dtype=float)
            if w.shape != o.shape:
                raise ValueError("curve %d: %d weights for %d observations" % (c, len(w), len(o)))
            w_mat[c, :len(o)] = w[order] if times is not None else w
    if cut_levels is not None:
        if cut_levels.shape not in ((S,), (Cn, S)):
            raise ValueError("cut_levels must have shape (S,) or (C, S) = (%d, %d), got %r" % (Cn, S, cut_levels.shape))
        if not np.all(cut_levels >= 0.0):
            raise ValueError("cut_levels must be >= 0 or +inf everywhere")
        cut_levels = np.ascontiguousarray(np.broadcast_to(cut_levels, (Cn, S)))
    if cut_budget is not None:
        if cut_budget.shape != (S,):
            raise ValueError("cut_budget must have shape (S,) = (%d,), got %r" % (S, cut_budget.shape))
        if not np.all(cut_budget >= 0.0):
            raise ValueError("cut_budget must be >= 0 or +inf everywhere")
    if P is None:
        P = np.zeros(S)
    if not (P.dtype == np.float64 and P.flags.c_contiguous and P.shape == (S,)):
        raise ValueError("P must be a contiguous float64 array of shape (S,)")
    sse = np.zeros((Cn, S))
    status = np.zeros((Cn, S), dtype=np.int32)
    iters = np.zeros((Cn, S), dtype=np.int64)
    floor_col = np.full((Cn, S), -1, dtype=np.int32)
    flags = (_abi.FLAG_STRICT if strict else 0) | (_abi.FLAG_PL_F32 if pl_f32 else 0) \
        | (_abi.FLAG_NORMALIZE if normalize else 0) | _abi.fp32_flags(fp32) | _abi.kernel_flag(kernel) \
        | (_abi.FLAG_MIXED if mixed else 0) | _abi.flag_bundle(bundle, L) | (_abi.FLAG_HIST32 if hist32 else 0) \
        | _abi.flag_bdf_order(bdf_order) | int(extra_flags) | (_abi.FLAG_PREDICT if predict else 0)
    sec = _abi.C.c_double(0.0)
    lib = _abi.lib()
    levels, budget = cut_levels is not None, cut_budget is not None
    weighted, cut, multi, off = weights is not None, sse_cut is not None or levels or budget, devices is not None, times is not None
    entry = "trpl_loglik_weighted" if weighted else "trpl_loglik_moments" if moments else "trpl_loglik_cut_levels" if levels \
        else "trpl_loglik_cut_budget" if budget else "trpl_loglik_cut" if cut \
        else "trpl_loglik_multi" if multi else "trpl_loglik_obs" if off else "trpl_loglik"
    own = {}                                       # the entry point's own outputs, as info receives them
    if weighted or moments:
        esum = np.zeros((Cn, S))
        own.update(esum=esum, P=P)                 # P: the one-offset likelihood trpl_loglik would return
    if weighted:
        own["wsum"] = wsum = np.array([math.fsum(w_mat[c, :n_obs[c]]) for c in range(Cn)])
    if cut:
        own["cut_col"] = cut_col = np.full((Cn, S), -1, dtype=np.int32)
    if budget:
        own["cut_level"] = level_out = np.full((Cn, S), np.inf)
    if multi:
        dev = None if isinstance(devices, str) else np.ascontiguousarray(devices, dtype=np.int32)
        if isinstance(devices, str) and devices != "all":
            raise ValueError("devices must be None, 'all' or a list of device ordinals")
        if dev is not None and (dev.ndim != 1 or len(dev) < 1):
            raise ValueError("devices must name at least one device")
    # The call, built once; an entry point's own arguments sit where include/trpl.h puts them: no plT in trpl_loglik_obs, wts
    # after obs, no brackets in trpl_loglik, sse_cut (or cut_level; or budget, curves_per_launch and the cut_level to fill) before P,
    # esum or cut_col after sse, the device list for the device.
    head = [_abi.ptr(X), S, Cn, _abi.ptr(lengths), float(Time), int(L), int(T)] \
        + ([] if entry == "trpl_loglik_obs" else [int(plT)]) + [int(tol), int(MAX), _abi.ptr(ini)]
    brackets = [_abi.ptr(hi_mat), _abi.ptr(dx_mat), _abi.ptr(h_mat)] if off else [None, None, None]
    observed = [_abi.ptr(obs_mat)] + ([_abi.ptr(w_mat)] if weighted else []) + ([] if entry == "trpl_loglik" else brackets) \
        + [obs_ld, _abi.ptr(n_obs)]
    level_args = [_abi.ptr(cut_budget), curves_per_launch, _abi.ptr(level_out)] if budget else [_abi.ptr(cut_levels)] if levels \
        else [sse_cut] if cut else []
    outputs = level_args + [_abi.ptr(P), _abi.ptr(sse)] + ([_abi.ptr(esum)] if "esum" in own else []) \
        + ([_abi.ptr(cut_col)] if cut else []) + [_abi.ptr(status), _abi.ptr(iters), _abi.ptr(floor_col)]
    tail = [flags] + ([_abi.ptr(dev), 0 if dev is None else len(dev)] if multi else [int(device)]) + [_abi.C.byref(sec)]
    _abi.check(getattr(lib, entry)(*head, *observed, *outputs, *tail))
    if cut:
        own["cut_fraction"] = float(np.mean(cut_col >= 0)) if cut_col.size else 0.0
    if budget:
        own["cut_samples"] = float(np.mean((cut_col >= 0).any(axis=0))) if cut_col.size else 0.0
    if info is not None:
        info.update(sse=sse, status=status, iters_total=iters, floor_col=floor_col, seconds=sec.value, **own)
    if not moments:
        return P
    # the likelihood over the magnitude offset, from the moments: n_obs, or the weighted entry points with wsum in its place
    per_curve, w = (wsum, "_w") if weighted else (n_obs, "")
    if mag_grid is not None:
        offs = np.ascontiguousarray(mag_grid, dtype=np.float64).ravel()
        Pm = np.zeros((len(offs), S)) if P_out is None else P_out
        if not (Pm.dtype == np.float64 and Pm.flags.c_contiguous and Pm.shape == (len(offs), S)):
            raise ValueError("P must be a contiguous float64 array of shape (len(mag_grid), S)")
        _abi.check(getattr(lib, "trpl_mag_grid" + w)(_abi.ptr(sse), _abi.ptr(esum), _abi.ptr(per_curve), S, Cn, _abi.ptr(offs),
                                                     len(offs), _abi.ptr(Pm)))
        return Pm
    best_per_curve = mag_profile == "per_curve"
    Pp = np.zeros(S) if P_out is None else P_out
    if not (Pp.dtype == np.float64 and Pp.flags.c_contiguous and Pp.shape == (S,)):
        raise ValueError("P must be a contiguous float64 array of shape (S,)")
    best = np.zeros((Cn, S) if best_per_curve else S)
    _abi.check(getattr(lib, "trpl_mag_profile" + w)(_abi.ptr(sse), _abi.ptr(esum), _abi.ptr(per_curve), S, Cn,
                                                    _abi.MAG_PER_CURVE if best_per_curve else 0, _abi.ptr(best), _abi.ptr(Pp)))
    return best, Pp


def next_cut(margin, best_total):
    """The sse_cut of the next sample block under gpu_info["cut_margin"]: +inf while no block has finished
    (best_total None), otherwise margin + best_total, where best_total is the smallest sum_c sse over all finished samples.
    The running minimum only falls, so every block's level is looser than the final one needs."""
    if best_total is None:
        return float("inf")
    return float(margin) + float(best_total)


def _bundle_of(gpu_info, L):
    """gpu_info['max_sims_per_block'] (bayeslib.py:93) as a TRPL_FLAG_BUNDLE size: 2 .. 4 at L = 128 and 2 .. 16 on
    grids of up to 64 nodes are honoured by the default arithmetic, anything else means every sample on its own
    (model.pvSim applies the same rule)."""
    m = int(gpu_info.get("max_sims_per_block", 1))
    return m if (1 <= m <= _abi.bundle_cap(L) and int(L) <= 128 and gpu_info.get("devices") is None) else 1


def _simulate_resident(e_data, P, X, num_curves, thicknesses, sim_params, init_params, normalize, pl_dtype, group,
                       num_gpus, gpu_id, device, solver_time, err_sq_time, sim_t, bundle=1, literal=False, predict=False,
                       mag_grid=None, weighted=False, irf=None, irf_bank=None):
    """Several experiments, fused option on: the reference's own loop order -- curves -> sample blocks ->
    experiments (bayeslib.py:117-171) -- with the block's PL matrix kept in HBM: one solve per (curve, block)
    (trpl_solve_pl_dev), then one pass over it per experiment (trpl_loglik_from_pl_dev: normalise, clamp,
    log10, time interpolation, squared error).  Only X goes in and P comes out.  literal: observations_on_grid's switch
    (gpu_info["interpolate_prefix"]).  mag_grid (gpu_info["mag_grid"]): P is (n_exp, M * S); each pass over the PL block also
    returns the first moment of the errors (trpl_loglik_moments_from_pl_dev), and after a block's last curve
    trpl_mag_grid_dev fills the M rows of every experiment.  weighted (gpu_info["weighted"]): every pass is
    trpl_loglik_weighted_from_pl_dev with the weights of the experiment's uncertainty column (and trpl_mag_grid_w_dev).
    irf (gpu_info["irf"]) = (h, k0): every solved block is convolved with the instrument response (trpl_convolve_irf_dev) and the
    passes run over the convolved block, whose ncol is T + 1 - k0.
    irf_bank (gpu_info["irf_bank"]) = dict(H, k0, mag, marginal, tf, log_prior): per experiment and curve the pass is
    trpl_loglik_irf_bank_dev, the moments of the J responses stay in HBM, and after a block's last curve ONE
    trpl_nuisance_reduce_dev per experiment adds the maximum or the marginal over responses x magnitude offsets to P."""
    import torch

    from . import device as tdev
    dev = torch.device("cuda", device)
    Time, L, T = sim_params[1], sim_params[2], sim_params[3]
    tdt = torch.float32 if pl_dtype == np.float32 else torch.float64
    flags = _abi.FLAG_NORMALIZE if normalize else 0
    with torch.cuda.device(dev):
        ini_d = torch.from_numpy(np.ascontiguousarray(init_params, dtype=np.float64)).to(dev)
        if irf is not None:
            h_d = torch.from_numpy(irf[0]).to(dev)
        if irf_bank is not None:
            H_d = torch.from_numpy(irf_bank["H"]).to(dev)
            lp_d = None if irf_bank["log_prior"] is None else torch.from_numpy(irf_bank["log_prior"]).to(dev)
        # per (experiment, curve), staged once: the keywords of its pass over a PL block -- observations, off the grid their
        # brackets, weights -- and what trpl_mag_grid[_w]_dev takes for the curve, n_obs or the sum of the weights
        def to_dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        staged = []
        for exp in e_data:
            per_curve = []
            for c in range(num_curves):
                t = np.asarray(exp[0][c], dtype=float)
                o = np.asarray(exp[1][c], dtype=float)
                w = weights_from_uncertainty(exp[2][c]) if weighted else None
                kw = {}
                if not observations_on_grid(t, sim_t, literal):               # bayeslib.py:182-183, and prefixes of the grid (below)
                    order = np.argsort(t, kind="stable")
                    o, w = o[order], (w[order] if weighted else None)
                    kw = dict(zip(("obs_hi", "obs_dx", "obs_h"), map(to_dev, bracket_times(sim_t, t[order]))))
                kw["obs"] = to_dev(o)
                if weighted:
                    kw["wts"] = to_dev(w)
                per_curve.append((kw, math.fsum(w) if weighted else len(o)))
            staged.append(per_curve)
        pass_name = "loglik_weighted_from_pl_device" if weighted else \
            "loglik_moments_from_pl_device" if mag_grid is not None else "loglik_from_pl_device"
        for blk in range(gpu_id * group, len(X), num_gpus * group):           # :131
            size = min(group, len(X) - blk)
            X_d = torch.from_numpy(np.ascontiguousarray(X[blk:blk + size], dtype=np.float64)).to(dev)
            mat_d, mag_d = X_d[:, :12].contiguous(), X_d[:, 12].contiguous()   # :144,:195
            P_d = torch.from_numpy(np.ascontiguousarray(P[:, blk:blk + size])).to(dev)
            pl_d = torch.empty((size, T // sim_params[4] + 1), dtype=tdt, device=dev)     # :137
            st_d = torch.empty(size, dtype=torch.int32, device=dev)
            seen_d = pl_d if irf is None else torch.empty((size, pl_d.shape[1] - irf[1]), dtype=tdt, device=dev)   # what the passes read
            if mag_grid is not None:
                S_all, M = len(X), len(mag_grid)
                P_d = torch.from_numpy(np.ascontiguousarray(
                    P.reshape(len(e_data), M, S_all)[:, :, blk:blk + size])).to(dev)            # (n_exp, M, size)
                sse_d = torch.zeros((len(e_data), num_curves, size), dtype=torch.float64, device=dev)
                esum_d = torch.zeros_like(sse_d)
            if irf_bank is not None:
                sse_d = torch.zeros((len(e_data), num_curves, len(irf_bank["H"]), size), dtype=torch.float64, device=dev)
                esum_d = torch.zeros_like(sse_d)
                LL_d = torch.empty(size, dtype=torch.float64, device=dev)
            for c in range(num_curves):                                       # :117
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                tdev.solve_pl_device(mat_d, thicknesses[c], Time, L, T, ini_d[c].contiguous(), pl_d, status=st_d,
                                     tol=sim_params[6], MAX=sim_params[7], plT=sim_params[4],
                                     flags=_abi.flag_bundle(bundle, L) | (_abi.FLAG_PREDICT if predict else 0))
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                if irf is not None:
                    tdev.convolve_irf_device(pl_d, h_d, irf[1], seen_d)
                for e, per_curve in enumerate(staged):                        # :171
                    if irf_bank is not None:
                        tdev.loglik_irf_bank_device(pl_d, H_d, irf_bank["k0"], mag=mag_d, sse=sse_d[e, c], esum=esum_d[e, c], status=st_d,
                                                    **per_curve[c][0])
                        continue
                    out = {"P": P_d[e]} if mag_grid is None else {"sse": sse_d[e, c], "esum": esum_d[e, c]}
                    getattr(tdev, pass_name)(seen_d, mag=mag_d, flags=flags, status=st_d, **per_curve[c][0], **out)
                torch.cuda.synchronize(dev)
                solver_time[gpu_id] += t1 - t0
                err_sq_time[gpu_id] += time.perf_counter() - t1
            if irf_bank is not None:
                for e, per_curve in enumerate(staged):
                    tdev.nuisance_reduce_device(sse_d[e], esum_d[e], [float(n) for _, n in per_curve], LL_d, mag=irf_bank["mag"],
                                                marginal=irf_bank["marginal"], tf=irf_bank["tf"], log_prior=lp_d)
                    P_d[e] += LL_d
            if mag_grid is not None:
                mag_grid_device = tdev.mag_grid_w_device if weighted else tdev.mag_grid_device
                for e, per_curve in enumerate(staged):
                    mag_grid_device(sse_d[e], esum_d[e], [n for _, n in per_curve], mag_grid, P_d[e])
                P.reshape(len(e_data), M, S_all)[:, :, blk:blk + size] = P_d.cpu().numpy()
                continue
            P[:, blk:blk + size] = P_d.cpu().numpy()


def _check_irf_bank(opt):
    """gpu_info['irf_bank'] checked as irf.loglik_nuisance checks its arguments -> dict(H, k0, mag, marginal, tf, log_prior)."""
    from .irf import _check_bank, _check_prior, _check_reduction
    if not isinstance(opt, dict) or "bank" not in opt:
        raise ValueError("gpu_info['irf_bank'] must be a dict with the entry bank=(H, k0[, table])")
    unknown = set(opt) - {"bank", "mag", "reduce", "tf", "log_prior"}
    if unknown:
        raise ValueError("gpu_info['irf_bank']: unknown entries %s" % sorted(unknown))
    H, k0 = _check_bank(opt["bank"])
    mag = opt.get("mag", "fixed")
    marginal, off, M, tf = _check_reduction(mag, opt.get("reduce", "max"), float(opt.get("tf", 1.0)), where="gpu_info['irf_bank']: ")
    return dict(H=H, k0=k0, mag=mag if off is None else off, marginal=marginal, tf=tf,
                log_prior=_check_prior(opt.get("log_prior"), H.shape[0], M, marginal))


def simulate(model, e_data, P, X, plI, plI_int, num_curves, sim_params, init_params, sim_flags, gpu_info, gpu_id,
             solver_time, err_sq_time, misc_time, logger=None):
    """bayeslib.simulate (bayeslib.py:83-205), GPU branch, same arguments and in-place effects.

    Loop order curves -> sample blocks of gpu_info['sims_per_gpu'] (blocks gpu_id, gpu_id +
    num_gpus, ...) -> experiments; float32 PL buffer (:137); X[:, :-1] to the model and
    X[:, -1] as the log offset (:144,:195).  With gpu_info['fused'] true and every observation
    grid a prefix of the simulation grid, each (curve-set, block, experiment) is one fused launch
    (spread over gpu_info['devices'] when that is given, see loglik).  gpu_info['predict'] = True (default False) runs
    every solve with the extrapolated start of TRPL_FLAG_PREDICT, on the fused and the unfused (pvSim) paths alike.
    gpu_info['mag_grid'] = offsets (default None: nothing changes): the likelihood at the M magnitude offsets X[:, 12] +
    offsets[m] from ONE solve per sample (trpl_loglik_moments + trpl_mag_grid; the mag_grid loop of the reference's probs.lnP,
    probs.py:5-18).  X stays (S, 13); P must then be (n_exp, M * S), column m * S + s = sample s at offset m (mag_grid_samples
    builds the matching X).  Fused levels on one device only: anything else is a ValueError naming the option.
    gpu_info['weighted'] = True (default False: nothing changes): the uncertainty column of the observations, e_data[e][2][c],
    weights every squared error by 1 / (2 u^2) -- the line the reference has commented out (probs.py:40) -- on all three
    levels: the fused single-experiment call (trpl_loglik_weighted), the resident-PL level
    (trpl_loglik_weighted_from_pl_dev) and the unfused sequence (prob(..., weighted=True); interpolated rows take the weights
    of their observation times).  Combines with 'mag_grid' and 'predict'; not with 'devices' or 'max_sims_per_block' > 1.
    gpu_info['cut_margin'] = a float (default None: every call path as before): early stop of hopeless samples on the fused
    single-experiment level, on one device.  The first sample block runs uncut; each later block runs trpl_loglik_cut with
    sse_cut = next_cut(margin, smallest sum_c sse over all finished samples).  A cut sample's P is an upper bound of its
    likelihood, at least `margin` below the best finished sample's; with margin = posterior.exact_cut_margin(tf) (and P
    starting from equal values, as bayes() does) the posterior weights at that tf equal the uncut run's.
    gpu_info['cut_log'], if a list, receives one dict per block (sse_cut, cut_fraction, cut_samples -- the share of the block's samples
    with any cut system -- and iters_total summed).  Anything but
    the fused one-experiment level on one device is a ValueError naming the option.
    gpu_info['cut_budget'] = True beside 'cut_margin' (default False): the same level is a level for a sample's TOTAL, so each later
    block runs trpl_loglik_cut_budget with it as every sample's budget, spent across the curves in launches of
    gpu_info['curves_per_launch'] (default 1) curves -- a sample stops once its curves together are past the level, not only when
    one curve alone is.  A cut sample's total is at or above the level, which is all the paragraph above needs: the posterior
    weights stay the uncut run's.  Without 'cut_margin' it is a ValueError.
    gpu_info['irf'] = (h, k0) (default None: nothing changes): the instrument response in the model (irf.gaussian,
    irf.from_samples; taps at the spacing of the simulation grid, tap k0 at time zero).  Every solved PL block is convolved on the
    device (trpl_convolve_irf_dev) before it is compared, on the resident-PL level whatever the number of experiments; the convolved
    curve ends at Time * (T - k0) / T, and a later observation is a ValueError.  Combines with 'predict', 'weighted' and 'mag_grid'
    (passes over the same block).  The unfused sequence, 'devices', 'cut_margin' and self_normalize are a ValueError naming the
    option: the fused steppers compare the bare curve, and a convolved curve's first column is not PL(0).
    gpu_info['irf_bank'] = dict(bank=(H, k0[, table]), mag="fixed" | "profile" | offsets, reduce="max" | "marginal", tf=1.0,
    log_prior=None) (default absent: nothing changes): the instrument response and the magnitude offset as nuisance parameters,
    reduced on the device (irf.loglik_nuisance has the meaning of every entry; only bank is required).  On the resident-PL level
    of one device, whatever the number of experiments: per experiment, block and curve one trpl_loglik_irf_bank_dev, then one
    trpl_nuisance_reduce_dev per experiment and block, whose result is added to P (n_exp, S); the moments never leave the device.
    Combines with 'predict' and 'weighted'.  'irf', 'mag_grid', 'devices', 'num_gpus' > 1, 'cut_margin', 'max_sims_per_block' > 1,
    self_normalize and the unfused sequence are a ValueError naming the option; so is an observation after the last convolved
    column, Time * (T - k0) / T.
    """
    group = int(gpu_info["sims_per_gpu"])
    num_gpus = int(gpu_info["num_gpus"])
    device = int(gpu_info.get("device", 0))
    LOG_PL = sim_flags["log_pl"]
    NORMALIZE = sim_flags["self_normalize"]
    if sim_flags.get("load_PL_from_file"):
        raise NotImplementedError("load PL not implemented")              # bayeslib.py:163-164
    if isinstance(sim_params[0], (int, float)):                           # :109-112
        thicknesses = [sim_params[0]] * num_curves
    else:
        thicknesses = list(sim_params[0])
    Time, L, T = sim_params[1], sim_params[2], sim_params[3]
    sim_t = np.linspace(0, Time, T + 1)                                   # :115
    pl_dtype = np.dtype(gpu_info.get("pl_dtype", np.float32))
    predict = bool(gpu_info.get("predict", False))
    if predict and int(gpu_info.get("max_sims_per_block", 1)) > 1:
        raise ValueError("gpu_info['predict'] does not combine with gpu_info['max_sims_per_block'] > 1: there is no bundled "
                         "stepper with the extrapolated start (TRPL_FLAG_PREDICT)")

    def in_range(t):
        t = np.asarray(t, dtype=float)
        return len(t) > 0 and t.min() >= sim_t[0] and t.max() <= sim_t[-1]

    fused = bool(gpu_info.get("fused", False)) and LOG_PL and sim_params[4] == 1 and all(
        in_range(exp[0][c]) for exp in e_data for c in range(num_curves))
    weighted = bool(gpu_info.get("weighted", False))
    if weighted:
        if gpu_info.get("devices") is not None:
            raise ValueError("gpu_info['weighted'] does not combine with gpu_info['devices']: trpl_loglik_multi has no weighted form")
        if int(gpu_info.get("max_sims_per_block", 1)) > 1:
            raise ValueError("gpu_info['weighted'] does not combine with gpu_info['max_sims_per_block'] > 1 (TRPL_FLAG_WEIGHTED has no bundles)")
    cut_margin = gpu_info.get("cut_margin")
    if cut_margin is not None:
        cut_margin = float(cut_margin)
        if not cut_margin >= 0.0:
            raise ValueError("gpu_info['cut_margin'] must be >= 0, got %r" % (cut_margin,))
        for name, bad in (("len(e_data) > 1", len(e_data) > 1), ("devices", gpu_info.get("devices") is not None),
                          ("num_gpus", num_gpus != 1), ("max_sims_per_block", int(gpu_info.get("max_sims_per_block", 1)) > 1),
                          ("mag_grid", gpu_info.get("mag_grid") is not None), ("weighted", weighted)):
            if bad:
                raise ValueError("gpu_info['cut_margin'] does not combine with %s: the early stop runs on the fused "
                                 "single-experiment level, on one device (trpl_loglik_cut)" % name)
        if not fused:
            raise ValueError("gpu_info['cut_margin'] needs the fused level: gpu_info['fused'] = True, log_pl, PL stride 1 and "
                             "observation times inside the simulated window")
    cut_budget = bool(gpu_info.get("cut_budget", False))
    if cut_budget and cut_margin is None:
        raise ValueError("gpu_info['cut_budget'] needs gpu_info['cut_margin']: the budget of a sample is margin + the best total so far")
    if gpu_info.get("curves_per_launch") is not None and not cut_budget:
        raise ValueError("gpu_info['curves_per_launch'] goes with gpu_info['cut_budget']")
    irf = gpu_info.get("irf")
    if irf is not None:
        from .irf import _check_irf, last_time
        irf = _check_irf(irf)
        for name, bad in (("devices", gpu_info.get("devices") is not None), ("cut_margin", cut_margin is not None),
                          ("self_normalize", bool(NORMALIZE))):
            if bad:
                raise ValueError("gpu_info['irf'] does not combine with %s: the convolution runs on the resident-PL level of one "
                                 "device, on curves that are not self-normalised" % name)
        if not fused:
            raise ValueError("gpu_info['irf'] needs the fused level, not the unfused sequence: gpu_info['fused'] = True, log_pl, PL "
                             "stride 1 and observation times inside the simulated window")
        if T + 1 - irf[1] < 2:
            raise ValueError("gpu_info['irf']: k0 = %d leaves fewer than two columns of a window of T = %d steps" % (irf[1], T))
        if any(np.max(np.asarray(exp[0][c], dtype=float)) > sim_t[T - irf[1]] for exp in e_data for c in range(num_curves)):
            raise ValueError("gpu_info['irf']: an observation lies after Time * (T - k0) / T = %g, the last convolved column"
                             % last_time(Time, T, irf[1]))
    irf_bank = gpu_info.get("irf_bank")
    if irf_bank is not None:
        irf_bank = _check_irf_bank(irf_bank)
        for name, bad in (("irf", irf is not None), ("mag_grid", gpu_info.get("mag_grid") is not None),
                          ("devices", gpu_info.get("devices") is not None), ("num_gpus", num_gpus != 1),
                          ("cut_margin", cut_margin is not None), ("max_sims_per_block", int(gpu_info.get("max_sims_per_block", 1)) > 1),
                          ("self_normalize", bool(NORMALIZE))):
            if bad:
                raise ValueError("gpu_info['irf_bank'] does not combine with %s: the bank is scored on the resident-PL level of one "
                                 "device, on curves that are not self-normalised, and brings its own reduction over the magnitude "
                                 "offset" % name)
        if not fused:
            raise ValueError("gpu_info['irf_bank'] needs the fused level, not the unfused sequence: gpu_info['fused'] = True, log_pl, PL "
                             "stride 1 and observation times inside the simulated window")
        k0 = irf_bank["k0"]
        if T + 1 - k0 < 2:
            raise ValueError("gpu_info['irf_bank']: k0 = %d leaves fewer than two columns of a window of T = %d steps" % (k0, T))
        if any(np.max(np.asarray(exp[0][c], dtype=float)) > sim_t[T - k0] for exp in e_data for c in range(num_curves)):
            raise ValueError("gpu_info['irf_bank']: an observation lies after Time * (T - k0) / T = %g, the last convolved column"
                             % (float(Time) * (T - k0) / T))
    mag_grid = gpu_info.get("mag_grid")
    if mag_grid is not None:
        mag_grid = np.ascontiguousarray(mag_grid, dtype=np.float64).ravel()
        if gpu_info.get("devices") is not None:
            raise ValueError("gpu_info['mag_grid'] does not combine with gpu_info['devices']: trpl_loglik_multi has no moments form")
        if num_gpus != 1:
            raise ValueError("gpu_info['mag_grid'] needs gpu_info['num_gpus'] = 1 (the rank driver keeps the one-offset likelihood)")
        if not fused:
            raise ValueError("gpu_info['mag_grid'] needs the fused level: gpu_info['fused'] = True, log_pl, PL stride 1 and "
                             "observation times inside the simulated window")
        if int(gpu_info.get("max_sims_per_block", 1)) > 1:
            raise ValueError("gpu_info['mag_grid'] does not combine with gpu_info['max_sims_per_block'] > 1 (TRPL_FLAG_MOMENTS has no bundles)")
        if P.shape != (len(e_data), len(mag_grid) * len(X)) or not P.flags.c_contiguous:
            raise ValueError("gpu_info['mag_grid']: P must be a contiguous (n_exp, M * S) = (%d, %d) array"
                             % (len(e_data), len(mag_grid) * len(X)))
    if fused and (len(e_data) > 1 or irf is not None or irf_bank is not None) and gpu_info.get("devices") is None:
        _simulate_resident(e_data, P, X, num_curves, thicknesses, sim_params, init_params, NORMALIZE, pl_dtype,
                           group, num_gpus, gpu_id, device, solver_time, err_sq_time, sim_t,
                           bundle=_bundle_of(gpu_info, L), literal=bool(gpu_info.get("interpolate_prefix", False)),
                           predict=predict, mag_grid=mag_grid, weighted=weighted, irf=irf, irf_bank=irf_bank)
        return
    if fused:
        # An experiment sampled exactly on the full simulation grid is compared point by point (the reference's bypass,
        # bayeslib.py:182-183); anything else is interpolated there (:184-191).  Observation times that are a PREFIX of the
        # simulation grid -- the shipped example data: 0.025 ns spacing, 140 .. 320 ns of a 2000 ns window; the reference's
        # shape test sends them to griddata -- are interpolated AT grid nodes, where the interp1d form returns the node's own
        # value to one rounding: they take the on-grid entry point too (batched emission, curve-pair table: 21 % faster on
        # the production shape, likelihoods equal to 7e-15, tools/bench_prefix_vs_interp.py); gpu_info["interpolate_prefix"]
        # = True keeps the literal interpolation (both fused branches: this one and _simulate_resident).
        literal = bool(gpu_info.get("interpolate_prefix", False))
        best_total = None                          # cut_margin: smallest sum_c sse over the finished samples
        for blk in range(gpu_id * group, len(X), num_gpus * group):
            size = min(group, len(X) - blk)
            for e, exp in enumerate(e_data):
                on_grid = fused_entry_point(exp[0], sim_t, num_curves, literal) == "trpl_loglik"
                info = {}
                args = (X[blk:blk + size], init_params, thicknesses, Time, L, T, [exp[1][c] for c in range(num_curves)])
                common = dict(tol=sim_params[6], MAX=sim_params[7], pl_f32=(pl_dtype == np.float32), normalize=NORMALIZE,
                              device=device, info=info, predict=predict,
                              times=None if on_grid else [exp[0][c] for c in range(num_curves)])
                if weighted:
                    common["weights"] = [weights_from_uncertainty(exp[2][c]) for c in range(num_curves)]
                if cut_margin is not None:         # one experiment, one device (checked above)
                    level = next_cut(cut_margin, best_total)
                    if cut_budget:
                        loglik(*args, P=P[e, blk:blk + size], cut_budget=np.full(size, level),
                               curves_per_launch=int(gpu_info.get("curves_per_launch") or 1), **common)
                    else:
                        loglik(*args, P=P[e, blk:blk + size], sse_cut=level, **common)
                    solver_time[gpu_id] += info["seconds"]
                    # a cut sample's reported total is at or above the level it was cut at, hence above the minimum so far:
                    # it never lowers it; NaN totals are skipped
                    total = info["sse"].sum(axis=0)
                    if np.any(total == total):
                        low = float(np.nanmin(total))
                        best_total = low if best_total is None else min(best_total, low)
                    if isinstance(gpu_info.get("cut_log"), list):
                        gpu_info["cut_log"].append({"block": blk, "sse_cut": level, "cut_fraction": info["cut_fraction"],
                                                    "cut_samples": float(np.mean((info["cut_col"] >= 0).any(axis=0))),
                                                    "iters_total": int(info["iters_total"].sum())})
                    continue
                if mag_grid is not None:
                    Pe = P[e].reshape(len(mag_grid), len(X))
                    Pm = np.ascontiguousarray(Pe[:, blk:blk + size])
                    loglik(*args, P=Pm, mag_grid=mag_grid, **common)
                    Pe[:, blk:blk + size] = Pm
                    solver_time[gpu_id] += info["seconds"]
                    continue
                loglik(*args, P=P[e, blk:blk + size], devices=gpu_info.get("devices"), bundle=_bundle_of(gpu_info, L), **common)
                solver_time[gpu_id] += info["seconds"]
        return

    # The reference walks curves -> blocks (:117,:131).  A sample only ever meets its own block, and every
    # P[e, j] receives its curves in the same order either way, so the loops can be swapped: blocks outside,
    # and -- when the model is this package's own (re-entrant: every call runs on a private stream) -- the
    # block's curves solved concurrently from a few host threads, which is what fills the chip when the
    # blocks are as small as the reference's default 1024 samples.  Since round 5 a worker also does its curve's
    # normalisation, fastlog and time interpolation (the calls release the GIL), and the next block's curves are
    # submitted while this thread accumulates the current block's squared errors with prob() in curve order: the
    # same calls on the same data in the same order per P[e, j], overlapped (production shape, sims_per_gpu 1024:
    # 147 s -> see DESIGN.md section 5).
    overlap = (model is pvSim or getattr(model, "reentrant", False)) and bool(gpu_info.get("overlap_curves", True)) \
        and num_curves > 1
    ncol = T // sim_params[4] + 1
    obs_times = [[np.asarray(exp[0][c], dtype=float) for c in range(num_curves)] for exp in e_data]
    on_grid = [[almost_equal(sim_t, t) for t in per_curve] for per_curve in obs_times]        # :173,:182-183

    # gpu_info["kernel"] = "pair" / "single" pins the FAST stepper of every pvSim launch (measurements; default None: the
    # library picks per launch -- the one-system kernel for the reference's 1024-sample blocks.  Pinning the paired kernel for
    # the overlapped launches was measured and rejected: three worker threads keep 3 x 1024 systems in flight, which under-fills
    # it -- production shape 126 s against 119 s, profiles/r6_e2e_production_ab.json)
    model_kw = {}
    if model is pvSim and gpu_info.get("kernel") is not None and int(gpu_info.get("max_sims_per_block", 1)) == 1:
        model_kw["kernel"] = gpu_info["kernel"]
    if predict:                                  # never dropped silently: only this package's pvSim has the mode
        if model is not pvSim:
            raise ValueError("gpu_info['predict'] needs this package's model (pvSim) on the unfused path, got %r" % (model,))
        model_kw["predict"] = True
    reads_pl = [any(on_grid[e][c] for e in range(len(e_data))) for c in range(num_curves)]

    def process_curve(ic_num, blk, size, last=True):
        par = list(sim_params)
        par[0] = thicknesses[ic_num]                                      # :119
        # a FRESH matrix per task, like the reference (:137).  Reusing the matrices of consumed results was measured and
        # rejected: at sims_per_gpu = 1024 the reused address ranges -- page-locked and released again by every pvSim and
        # fastlog call -- serialise the worker threads' launches (production shape / 4: 33 s against 27.5 s, shared or
        # per-thread reuse alike; profiles/r6_levelb_task_phases.txt)
        buf = np.empty((size, ncol), dtype=pl_dtype)
        sec = model(buf, None, None, None, X[blk:blk + size, :-1], par, init_params[ic_num], None, None,
                    int(gpu_info.get("max_sims_per_block", 1)), init_mode="points", **model_kw)      # :93,:146
        misc = 0.0
        if NORMALIZE:                                                     # :150-154
            buf /= buf[:, :1].copy()
        if LOG_PL:                                                        # :155-157
            misc += fastlog(buf, sys.float_info.min, device=device)
        ints = []
        for e in range(len(e_data)):                                      # :168
            if on_grid[e][ic_num]:
                ints.append(buf)
            else:                                                         # :184-191
                clock0 = time.perf_counter()
                ints.append(interp_rows(sim_t, buf, obs_times[e][ic_num]))
                misc += time.perf_counter() - clock0
        # the PL matrix itself is only read again when an experiment compares this curve on the grid; otherwise it is let go
        # here, while the result waits for prob() (the run's LAST result keeps it: plI[gpu_id] ends up holding the last PL
        # matrix, as in the reference)
        return (buf if (reads_pl[ic_num] or last) else None), ints, sec, misc

    blocks = list(range(gpu_id * group, len(X), num_gpus * group))        # :131
    tasks = [(blk, min(group, len(X) - blk), c) for blk in blocks for c in range(num_curves)]   # the order P receives them in
    # Host memory of the overlapped path is bounded by BYTES (gpu_info["max_host_bytes"], default 32 GiB), not by a block
    # count: overlap_window() picks how many results may exist at once -- at most two blocks' curves, the round-5 schedule --
    # and how many worker threads make them.
    full, done = unfused_curve_bytes(min(group, len(X)) if len(X) else 0, ncol, pl_dtype,
                                     [0 if on_grid[e][c] else len(obs_times[e][c]) for e in range(len(e_data))
                                      for c in range(num_curves)], num_curves)
    window, workers = overlap_window(full, done, int(gpu_info.get("max_host_bytes", DEFAULT_MAX_HOST_BYTES)), num_curves)
    if window < 2:
        overlap = False
    pool = None
    if overlap:
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=workers)
    try:
        nxt, queue = 0, None

        def submit_next():
            b2, s2, c2 = tasks[nxt]
            queue.append(pool.submit(process_curve, c2, b2, s2, nxt == len(tasks) - 1))

        if overlap:
            queue = deque()
            while nxt < len(tasks) and len(queue) < window - 1:          # + the result being consumed = window
                submit_next()
                nxt += 1
        for blk, size, ic_num in tasks:
            if ic_num == 0:
                if logger is not None:
                    logger.info("Calculating {} of {}".format(blk, len(X)))
                mag = np.ascontiguousarray(X[blk:blk + size, -1])
            sim_params[0] = thicknesses[ic_num]                           # :119 (the caller's list is mutated, as there)
            if overlap:
                res = queue.popleft().result()
            else:
                plI[gpu_id] = plI_int[gpu_id] = None                      # one result at a time
                res = process_curve(ic_num, blk, size)
            plI[gpu_id], ints, sec, misc = res
            del res
            solver_time[gpu_id] += sec
            misc_time[gpu_id] += misc
            for e, exp in enumerate(e_data):
                plI_int[gpu_id] = ints[e]
                if weighted:
                    err_sq_time[gpu_id] += prob(P[e, blk:blk + size], ints[e], exp[1][ic_num], exp[2][ic_num], mag,
                                                device=device, weighted=True)
                    continue
                err_sq_time[gpu_id] += prob(P[e, blk:blk + size], ints[e], exp[1][ic_num], None, mag, device=device)
            del ints                                                      # plI_int[gpu_id] keeps the last matrix, as there
            if overlap and nxt < len(tasks):                              # the previous result is gone: the window has room
                submit_next()
                nxt += 1
    finally:
        if pool is not None:
            pool.shutdown(wait=True)


def mag_grid_samples(X, offsets):
    """The sample matrix that goes with a gpu_info['mag_grid'] result: (M * S, 13), row m * S + s = sample s with
    offsets[m] added to its magnitude offset (column 12)."""
    X = np.asarray(X, dtype=np.float64)
    out = np.tile(X, (len(offsets), 1))
    out[:, 12] += np.repeat(np.asarray(offsets, dtype=np.float64), len(X))
    return out


def bayes(model, N, P, minX, maxX, do_log, init_params, sim_params, e_data, sim_flags, gpu_info, logger=None,
          rng=None):
    """bayeslib.bayes (bayeslib.py:207-252): sample the box, run simulate() for this process's
    share of the sample blocks, return (N, P, X).  The process's block index comes from
    SLURM_ARRAY_TASK_ID as in the reference (:231), falling back to RANK, then 0."""
    num_gpus = int(gpu_info["num_gpus"])
    solver_time, err_sq_time, misc_time = np.zeros(num_gpus), np.zeros(num_gpus), np.zeros(num_gpus)
    N, P, X = make_grid(len(e_data), minX, maxX, do_log, sim_flags, rng=rng)
    gpu_id = int(os.getenv("SLURM_ARRAY_TASK_ID", os.getenv("RANK", "0")))
    if not 0 <= gpu_id < num_gpus:
        raise ValueError("process index %d outside num_gpus=%d" % (gpu_id, num_gpus))
    plI, plI_int = [None] * num_gpus, [None] * num_gpus
    offsets = gpu_info.get("mag_grid")
    if offsets is not None:                           # M likelihoods per solved sample: P (n_exp, M * S), X (M * S, 13) below
        P = np.tile(P, (1, len(offsets)))
    simulate(model if model is not None else pvSim, e_data, P, X, plI, plI_int, len(init_params),
             list(sim_params), init_params, sim_flags, gpu_info, gpu_id, solver_time, err_sq_time, misc_time,
             logger=logger)
    if logger is not None:
        logger.info("Total tEvol time: {}".format(solver_time))
        logger.info("Total err_sq time: {}".format(err_sq_time))
        logger.info("Total misc time: {}".format(misc_time))
    if offsets is not None:
        X = mag_grid_samples(X, offsets)
        N = np.arange(len(X)) if isinstance(N, np.ndarray) and N.ndim == 1 else N
    return N, P, X
