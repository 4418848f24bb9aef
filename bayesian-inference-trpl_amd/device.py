"""Device-resident entry points: inputs and outputs are torch tensors already in HBM; nothing is
allocated, copied or synchronised by the library (trpl_*_dev in include/trpl.h).  torch is used
for device memory, streams and torch.distributed only -- plumbing, not compute."""
import numpy as np

from . import _abi


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _chk(t, dtype, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError("%s must be a contiguous CUDA tensor of dtype %s" % (name, dtype))
    return t.data_ptr()


def _opt(t, dtype, name):
    """_chk for an optional tensor: None stays None (a NULL pointer)."""
    return None if t is None else _chk(t, dtype, name)


def _brackets(obs, obs_hi, obs_dx, obs_h):
    """The bracketing arrays of driver.bracket_times as three pointers, each shaped like obs -- or three None on the grid
    (obs_hi is None)."""
    import torch
    if obs_hi is None:
        return [None, None, None]
    if not (obs.shape == obs_hi.shape == obs_dx.shape == obs_h.shape):
        raise ValueError("shape mismatch")
    return [_chk(obs_hi, torch.int32, "obs_hi"), _chk(obs_dx, torch.float64, "obs_dx"), _chk(obs_h, torch.float64, "obs_h")]


def _loglik_dev(entry, X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status, iters_total, tol, MAX, flags, floor_col,
                plT=1, obs_hi=None, obs_dx=None, obs_h=None, wts=None, sse_cut=None, esum=None, cut_col=None, cut_level=None, budget=None,
                curves_per_launch=1):
    """The one marshaller of the fused family trpl_loglik[_obs|_moments|_weighted|_cut|_cut_levels|_cut_budget]_dev: the arguments all seven
    share, with an entry point's own where include/trpl.h puts them -- wts after obs, the brackets after that (not in trpl_loglik_dev),
    sse_cut (or cut_level (C,S) f64 in its place; or budget (S,) f64, curves_per_launch and the cut_level to fill) before P, esum or
    cut_col after sse; trpl_loglik_obs_dev alone has no plT.  A new sink or argument goes HERE."""
    import torch
    f64 = torch.float64
    S, Cn = X.shape[0], init_params.shape[0]
    if X.shape[1] != 13 or init_params.shape[1] != L or obs.shape[0] != Cn or tuple(sse.shape) != (Cn, S) \
            or tuple(P.shape) != (S,) or (wts is not None and wts.shape != obs.shape) \
            or any(t is not None and tuple(t.shape) != (Cn, S) for t in (esum, cut_col, cut_level)) \
            or (budget is not None and tuple(budget.shape) != (S,)):
        raise ValueError("shape mismatch")
    brackets = _brackets(obs, obs_hi, obs_dx, obs_h)
    lengths = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths, dtype=np.float64), (Cn,)))
    n_obs = np.ascontiguousarray(np.broadcast_to(np.asarray(n_obs, dtype=np.int64), (Cn,)))
    args = [_chk(X, f64, "X"), S, Cn, _abi.ptr(lengths), float(Time), int(L), int(T)]
    if entry != "trpl_loglik_obs_dev":
        args.append(int(plT))
    args += [int(tol), int(MAX), _chk(init_params, f64, "init_params"), _chk(obs, f64, "obs")]
    if entry == "trpl_loglik_weighted_dev":
        args.append(_chk(wts, f64, "wts"))
    if entry != "trpl_loglik_dev":
        args += brackets
    args += [obs.shape[1], _abi.ptr(n_obs)]
    if entry == "trpl_loglik_cut_dev":
        args.append(float(sse_cut))
    if entry == "trpl_loglik_cut_levels_dev":
        args.append(_chk(cut_level, f64, "cut_level"))
    if entry == "trpl_loglik_cut_budget_dev":
        args += [_chk(budget, f64, "budget"), int(curves_per_launch), _chk(cut_level, f64, "cut_level")]
    args += [_chk(P, f64, "P"), _chk(sse, f64, "sse")]
    if entry in ("trpl_loglik_moments_dev", "trpl_loglik_weighted_dev"):
        args.append(_chk(esum, f64, "esum"))
    if entry in ("trpl_loglik_cut_dev", "trpl_loglik_cut_levels_dev", "trpl_loglik_cut_budget_dev"):
        args.append(_opt(cut_col, torch.int32, "cut_col"))
    args += [_opt(status, torch.int32, "status"), _opt(iters_total, torch.int64, "iters_total"),
             _opt(floor_col, torch.int32, "floor_col"), int(flags), _stream()]
    _abi.check(getattr(_abi.lib(), entry)(*args))


def loglik_device(X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status=None, iters_total=None,
                  tol=7, MAX=10000, plT=1, flags=0, floor_col=None):
    """trpl_loglik_dev on the current device and stream.  X (S,13) f64, init_params (C,L) f64,
    obs (C,obs_ld) f64, P (S,) f64 accumulated in place, sse (C,S) f64 out, optional status
    (C,S) int32, iters_total (C,S) int64 and floor_col (C,S) int32 (first compared PL column below the
    cancellation floor, -1 if none: include/trpl.h).  lengths / n_obs are host sequences."""
    _loglik_dev("trpl_loglik_dev", X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status, iters_total, tol, MAX, flags,
                floor_col, plT=plT)


def loglik_obs_device(X, init_params, lengths, Time, L, T, obs, obs_hi, obs_dx, obs_h, n_obs, P, sse, status=None,
                      iters_total=None, tol=7, MAX=10000, flags=0, floor_col=None):
    """trpl_loglik_obs_dev: observation times off the simulation grid.  obs / obs_dx / obs_h (C,obs_ld)
    f64 and obs_hi (C,obs_ld) int32 are the bracketing arrays of driver.bracket_times, on the device."""
    _loglik_dev("trpl_loglik_obs_dev", X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status, iters_total, tol, MAX,
                flags, floor_col, obs_hi=obs_hi, obs_dx=obs_dx, obs_h=obs_h)


def loglik_moments_device(X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, esum, status=None, iters_total=None,
                          tol=7, MAX=10000, plT=1, flags=0, floor_col=None, obs_hi=None, obs_dx=None, obs_h=None):
    """trpl_loglik_moments_dev: loglik_device / loglik_obs_device (with the bracketing arrays obs_hi, obs_dx, obs_h) that
    also fills esum (C,S) f64, the sum of the log-errors whose squares make sse -- the input of mag_grid_device and
    mag_profile_device.  P, sse, status, iters_total and floor_col are loglik[_obs]_device's, bit for bit."""
    _loglik_dev("trpl_loglik_moments_dev", X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status, iters_total, tol, MAX,
                flags, floor_col, plT=plT, obs_hi=obs_hi, obs_dx=obs_dx, obs_h=obs_h, esum=esum)


def loglik_cut_device(X, init_params, lengths, Time, L, T, obs, n_obs, sse_cut, P, sse, cut_col=None, status=None,
                      iters_total=None, tol=7, MAX=10000, plT=1, flags=0, floor_col=None, obs_hi=None, obs_dx=None,
                      obs_h=None):
    """trpl_loglik_cut_dev: loglik_device / loglik_obs_device (with the bracketing arrays obs_hi, obs_dx, obs_h) with an
    early stop -- a system whose running sse is above sse_cut (a float >= 0 or +inf) after one of its 64-column batches
    takes no further time step.  cut_col (C,S) int32 optional: the leading observations in a cut system's sse, -1 for an
    uncut system (all its outputs are loglik_device's, bit for bit), -2 for a flagged one (include/trpl.h)."""
    _loglik_dev("trpl_loglik_cut_dev", X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status, iters_total, tol, MAX,
                flags, floor_col, plT=plT, obs_hi=obs_hi, obs_dx=obs_dx, obs_h=obs_h, sse_cut=sse_cut, cut_col=cut_col)


def loglik_cut_levels_device(X, init_params, lengths, Time, L, T, obs, n_obs, cut_level, P, sse, cut_col=None, status=None,
                             iters_total=None, tol=7, MAX=10000, plT=1, flags=0, floor_col=None, obs_hi=None, obs_dx=None,
                             obs_h=None):
    """trpl_loglik_cut_levels_dev: loglik_cut_device with a level per system -- cut_level (C,S) f64 on the device in the place of
    sse_cut.  System (c, s) reports what loglik_cut_device reports for it at sse_cut = cut_level[c, s], bit for bit, whatever the
    other systems' levels.  Nobody looks at the values here: a NaN level never cuts, a negative one cuts after the first batch
    (include/trpl.h).  The levels of a Metropolis step come from mcmc_levels_device."""
    if cut_level is None:
        raise ValueError("cut_level must be a (C,S) float64 tensor")
    _loglik_dev("trpl_loglik_cut_levels_dev", X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status, iters_total, tol, MAX,
                flags, floor_col, plT=plT, obs_hi=obs_hi, obs_dx=obs_dx, obs_h=obs_h, cut_col=cut_col, cut_level=cut_level)


def loglik_cut_budget_device(X, init_params, lengths, Time, L, T, obs, n_obs, budget, cut_level, P, sse, curves_per_launch=1,
                             cut_col=None, status=None, iters_total=None, tol=7, MAX=10000, plT=1, flags=0, floor_col=None,
                             obs_hi=None, obs_dx=None, obs_h=None):
    """trpl_loglik_cut_budget_dev: the early stop on a sample's TOTAL -- budget (S,) f64 on the device is the level for sum_c sse[c, s],
    spent over consecutive launches of curves_per_launch (1 .. 16) curves: before each launch a kernel gives its curves the level the
    budget leaves after what the earlier curves reported.  cut_level (C,S) f64 is an OUTPUT, the level every system ran at; every
    system reports what loglik_cut_levels_device reports for it at that level, bit for bit.  A sample with any cut_col >= 0 has a plain
    total >= its budget.  Nobody looks at the values here: a NaN budget never cuts, a negative one cuts every system of the sample after
    its first batch (include/trpl.h)."""
    if budget is None or cut_level is None:
        raise ValueError("budget must be a (S,) and cut_level a (C,S) float64 tensor")
    _loglik_dev("trpl_loglik_cut_budget_dev", X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status, iters_total, tol, MAX,
                flags, floor_col, plT=plT, obs_hi=obs_hi, obs_dx=obs_dx, obs_h=obs_h, cut_col=cut_col, cut_level=cut_level, budget=budget,
                curves_per_launch=curves_per_launch)


def _mag_grid_dev(entry, sse, esum, per_curve, dtype, offsets, P):
    """trpl_mag_grid_dev / trpl_mag_grid_w_dev: one call, the per-curve host vector n_obs (int64) or wsum (float64)."""
    import torch
    Cn, S = sse.shape
    off = np.ascontiguousarray(offsets, dtype=np.float64).ravel()
    per_curve = np.ascontiguousarray(np.broadcast_to(np.asarray(per_curve, dtype=dtype), (Cn,)))
    if tuple(esum.shape) != (Cn, S) or tuple(P.shape) != (len(off), S):
        raise ValueError("shape mismatch")
    _abi.check(getattr(_abi.lib(), entry)(_chk(sse, torch.float64, "sse"), _chk(esum, torch.float64, "esum"),
                                          _abi.ptr(per_curve), S, Cn, _abi.ptr(off), len(off),
                                          _chk(P, torch.float64, "P"), _stream()))


def _mag_profile_dev(entry, sse, esum, per_curve, dtype, best, P, best_per_curve):
    """trpl_mag_profile_dev / trpl_mag_profile_w_dev: as _mag_grid_dev."""
    import torch
    Cn, S = sse.shape
    per_curve = np.ascontiguousarray(np.broadcast_to(np.asarray(per_curve, dtype=dtype), (Cn,)))
    if tuple(esum.shape) != (Cn, S) or tuple(P.shape) != (S,) \
            or tuple(best.shape) != ((Cn, S) if best_per_curve else (S,)):
        raise ValueError("shape mismatch")
    _abi.check(getattr(_abi.lib(), entry)(_chk(sse, torch.float64, "sse"), _chk(esum, torch.float64, "esum"),
                                          _abi.ptr(per_curve), S, Cn, _abi.MAG_PER_CURVE if best_per_curve else 0,
                                          _chk(best, torch.float64, "best"), _chk(P, torch.float64, "P"), _stream()))


def mag_grid_device(sse, esum, n_obs, offsets, P):
    """trpl_mag_grid_dev: P (M,S) f64 -= sum_c max(sse + 2 d_m esum + n_c d_m^2, 0) for the offsets d_m (host sequence,
    added to X[:, 12]); sse, esum (C,S) f64 from loglik_moments_device, n_obs a host sequence (C,)."""
    _mag_grid_dev("trpl_mag_grid_dev", sse, esum, n_obs, np.int64, offsets, P)


def mag_profile_device(sse, esum, n_obs, best, P, per_curve=False):
    """trpl_mag_profile_dev: the likelihood-maximising offset best (S,) -- (C,S) with per_curve -- and P (S,) -= the
    squared error there (the profile likelihood over the magnitude offset)."""
    _mag_profile_dev("trpl_mag_profile_dev", sse, esum, n_obs, np.int64, best, P, per_curve)


def loglik_weighted_device(X, init_params, lengths, Time, L, T, obs, wts, n_obs, P, sse, esum, status=None,
                           iters_total=None, tol=7, MAX=10000, plT=1, flags=0, floor_col=None, obs_hi=None, obs_dx=None,
                           obs_h=None):
    """trpl_loglik_weighted_dev: loglik_moments_device with the observation weights wts, a device tensor shaped like obs:
    sse (C,S) = sum w e^2, esum (C,S) = sum w e, P (S,) -= sum_c sse.  The weights are NOT checked here (no
    synchronisation): finite and >= 0 is the caller's responsibility."""
    _loglik_dev("trpl_loglik_weighted_dev", X, init_params, lengths, Time, L, T, obs, n_obs, P, sse, status, iters_total, tol,
                MAX, flags, floor_col, plT=plT, obs_hi=obs_hi, obs_dx=obs_dx, obs_h=obs_h, wts=wts, esum=esum)


def mag_grid_w_device(sse, esum, wsum, offsets, P):
    """trpl_mag_grid_w_dev: mag_grid_device from the weighted moments; wsum a host sequence (C,), the sum of each
    curve's weights, in place of n_obs."""
    _mag_grid_dev("trpl_mag_grid_w_dev", sse, esum, wsum, np.float64, offsets, P)


def mag_profile_w_device(sse, esum, wsum, best, P, per_curve=False):
    """trpl_mag_profile_w_dev: mag_profile_device from the weighted moments (wsum as in mag_grid_w_device)."""
    _mag_profile_dev("trpl_mag_profile_w_dev", sse, esum, wsum, np.float64, best, P, per_curve)


def _solve_pl_dev(entry, matPar, Length, Time, L, T, plI, status, iters_total, tol, MAX, plT, flags, dN=None, resume=None,
                  snap=None):
    """The one marshaller of trpl_solve_pl[_snap|_resume]_dev: head, where the solve starts -- dN, or resume = (t0, resN, resP,
    resE) -- the PL block and, not in trpl_solve_pl_dev, the snapshot block snap = (snap_steps, plN, plP, plE)."""
    import torch
    f64 = torch.float64
    S = matPar.shape[0]
    if matPar.shape[1] != 12 or (resume is None and tuple(dN.shape) != (L,)) or tuple(plI.shape) != (S, T // plT + 1):
        raise ValueError("shape mismatch")
    if plI.dtype not in (torch.float32, torch.float64):
        raise ValueError("plI must be float32 or float64")
    if resume is None:
        start = [_chk(dN, f64, "dN")]
    else:
        for t, w in zip(resume[1:], (L, L, L + 1)):
            if tuple(t.shape) != (S, 5, w):
                raise ValueError("resume tensors must be (S, 5, L) / (S, 5, L+1)")
        start = [int(resume[0])] + [_chk(t, f64, name) for t, name in zip(resume[1:], ("resN", "resP", "resE"))]
    tail = []
    if snap is not None:
        steps = np.ascontiguousarray(snap[0], dtype=np.int64)
        n = len(steps)
        for t, w in zip(snap[1:], (L, L, L + 1)):
            if t is not None and tuple(t.shape) != (S, n, w):
                raise ValueError("snapshot tensors must be (S, len(snap_steps), L) / (.., L+1)")
        tail = [_abi.ptr(steps) if n else None, n] + [_opt(t, f64, name) for t, name in zip(snap[1:], ("plN", "plP", "plE"))]
    _abi.check(getattr(_abi.lib(), entry)(
        _chk(matPar, f64, "matPar"), S, float(Length), float(Time), int(L), int(T), int(plT), int(tol), int(MAX), *start,
        _chk(plI, plI.dtype, "plI"), plI.element_size(), plI.shape[1], _opt(status, torch.int32, "status"),
        _opt(iters_total, torch.int64, "iters_total"), *tail, int(flags), _stream()))


def solve_pl_device(matPar, Length, Time, L, T, dN, plI, status=None, iters_total=None, tol=7, MAX=10000, plT=1,
                    flags=0):
    """trpl_solve_pl_dev: matPar (S,12) f64, dN (L,) f64, plI (S, T//plT+1) f32/f64 out."""
    _solve_pl_dev("trpl_solve_pl_dev", matPar, Length, Time, L, T, plI, status, iters_total, tol, MAX, plT, flags, dN=dN)


def pcr_solve_device(ld, d, ud, b, x, flags=0):
    """trpl_pcr_solve_batched_dev: all (S,L) tensors of one dtype (f64 or f32)."""
    import torch
    S, L = d.shape
    dt = d.dtype
    if dt not in (torch.float32, torch.float64):
        raise ValueError("dtype must be float32 or float64")
    for t in (ld, ud, b, x):
        if tuple(t.shape) != (S, L):
            raise ValueError("shape mismatch")
    _abi.check(_abi.lib().trpl_pcr_solve_batched_dev(_chk(ld, dt, "ld"), _chk(d, dt, "d"), _chk(ud, dt, "ud"),
                                                     _chk(b, dt, "b"), _chk(x, dt, "x"), S, L, d.element_size(),
                                                     int(flags), _stream()))


# ---- posterior core, device-resident (trpl_posterior_*_dev) ----
def posterior_workspace(D=16):
    """A workspace tensor large enough for any posterior_*_device call with up to D columns."""
    import torch
    n = int(_abi.lib().trpl_posterior_workspace_bytes(int(D)))
    return torch.empty(n // 8, dtype=torch.float64, device="cuda")


def posterior_weights_device(LL, tf, W, workspace, stats=None):
    """W <- normalize(LL / tf) (Visualization/utils.py:157-166); LL, W (S,) f64; stats (2,) f64 optional
    {max, raw sum}."""
    import torch
    if LL.shape != W.shape or LL.dim() != 1:
        raise ValueError("LL and W must be (S,)")
    _abi.check(_abi.lib().trpl_posterior_weights_dev(
        _chk(LL, torch.float64, "LL"), LL.shape[0], float(tf), _chk(W, torch.float64, "W"),
        None if stats is None else _chk(stats, torch.float64, "stats"), _chk(workspace, torch.float64, "workspace"),
        workspace.numel() * 8, _stream()))


def posterior_moments_device(V, W, sums, central, workspace, mean_in=None):
    """V (D,S), W (S,) -> sums (2+D,), central (D, D+2) as trpl_posterior_moments defines them."""
    import torch
    D, S = V.shape
    if tuple(W.shape) != (S,) or tuple(sums.shape) != (2 + D,) or tuple(central.shape) != (D, D + 2):
        raise ValueError("shape mismatch")
    _abi.check(_abi.lib().trpl_posterior_moments_dev(
        _chk(V, torch.float64, "V"), S, D, _chk(W, torch.float64, "W"),
        None if mean_in is None else _chk(mean_in, torch.float64, "mean_in"), _chk(sums, torch.float64, "sums"),
        _chk(central, torch.float64, "central"), _chk(workspace, torch.float64, "workspace"), workspace.numel() * 8,
        _stream()))


def posterior_tf_scan_workspace(S, D, K):
    """A workspace tensor for posterior_tf_scan_device with S samples, D columns and K temperatures."""
    import torch
    n = int(_abi.lib().trpl_posterior_tf_scan_workspace(int(S), int(D), int(K)))
    if n <= 0:
        raise ValueError("S, D, K = %r are outside what trpl_posterior_tf_scan accepts" % ((S, D, K),))
    return torch.empty(n // 8, dtype=torch.float64, device="cuda")


def posterior_tf_scan_device(LL, tfs, stats, workspace, V=None, mean=None, var=None, Q=None):
    """The posterior at the K temperatures tfs (device tensor) in one scan: stats (K, 4); with V (D, S) also mean, var,
    Q (K, D), row k being the bits of posterior_weights_device(LL, tfs[k]) + posterior_moments_device
    (trpl_posterior_tf_scan_dev)."""
    import torch
    S, K = LL.shape[0], tfs.shape[0]
    D = 0 if V is None else V.shape[0]
    if LL.dim() != 1 or tfs.dim() != 1 or tuple(stats.shape) != (K, 4) or (D and tuple(V.shape) != (D, S)):
        raise ValueError("shape mismatch")
    outs = []
    for t, name in ((mean, "mean"), (var, "var"), (Q, "Q")):
        if D and (t is None or tuple(t.shape) != (K, D)):
            raise ValueError("%s must be (K, D)" % name)
        outs.append(_chk(t, torch.float64, name) if D else None)
    _abi.check(_abi.lib().trpl_posterior_tf_scan_dev(
        _chk(LL, torch.float64, "LL"), S, _chk(V, torch.float64, "V") if D else None, D, _chk(tfs, torch.float64, "tfs"), K,
        _chk(stats, torch.float64, "stats"), outs[0], outs[1], outs[2], _chk(workspace, torch.float64, "workspace"),
        workspace.numel() * 8, _stream()))


def posterior_weights_lr_device(LL, log_ratio, tf, W, workspace, stats=None):
    """W <- the normalised weights exp(LL / tf - log_ratio) of a refined set (trpl_posterior_weights_lr_dev): LL, log_ratio,
    W (S,) f64; stats (2,) f64 optional {max of LL / tf - log_ratio, raw sum}; workspace as posterior_weights_device.  With
    log_ratio = +0.0 everywhere the bits of posterior_weights_device."""
    import torch
    if LL.shape != W.shape or LL.shape != log_ratio.shape or LL.dim() != 1:
        raise ValueError("LL, log_ratio and W must be (S,)")
    _abi.check(_abi.lib().trpl_posterior_weights_lr_dev(
        _chk(LL, torch.float64, "LL"), _chk(log_ratio, torch.float64, "log_ratio"), LL.shape[0], float(tf),
        _chk(W, torch.float64, "W"), _opt(stats, torch.float64, "stats"), _chk(workspace, torch.float64, "workspace"),
        workspace.numel() * 8, _stream()))


def posterior_tf_scan_lr_workspace(S, D, K):
    """A workspace tensor for posterior_tf_scan_lr_device with S samples, D columns and K temperatures."""
    import torch
    n = int(_abi.lib().trpl_posterior_tf_scan_lr_workspace(int(S), int(D), int(K)))
    if n <= 0:
        raise ValueError("S, D, K = %r are outside what trpl_posterior_tf_scan_lr accepts" % ((S, D, K),))
    return torch.empty(n // 8, dtype=torch.float64, device="cuda")


def posterior_tf_scan_lr_device(LL, log_ratio, tfs, stats, workspace, V=None, mean=None, var=None, Q=None):
    """posterior_tf_scan_device with the proposal log-ratio log_ratio (S,) kept beside LL (trpl_posterior_tf_scan_lr_dev):
    stats (K, 6) = [max, raw sum, sum W, sum W^2, count, ess]; with V (D, S) also mean, var, Q (K, D), row k being the bits
    of posterior_weights_lr_device(LL, log_ratio, tfs[k]) + posterior_moments_device."""
    import torch
    S, K = LL.shape[0], tfs.shape[0]
    D = 0 if V is None else V.shape[0]
    if LL.dim() != 1 or tuple(log_ratio.shape) != (S,) or tfs.dim() != 1 or tuple(stats.shape) != (K, 6) \
            or (D and tuple(V.shape) != (D, S)):
        raise ValueError("shape mismatch")
    outs = []
    for t, name in ((mean, "mean"), (var, "var"), (Q, "Q")):
        if D and (t is None or tuple(t.shape) != (K, D)):
            raise ValueError("%s must be (K, D)" % name)
        outs.append(_chk(t, torch.float64, name) if D else None)
    _abi.check(_abi.lib().trpl_posterior_tf_scan_lr_dev(
        _chk(LL, torch.float64, "LL"), _chk(log_ratio, torch.float64, "log_ratio"), S, _chk(V, torch.float64, "V") if D else None,
        D, _chk(tfs, torch.float64, "tfs"), K, _chk(stats, torch.float64, "stats"), outs[0], outs[1], outs[2],
        _chk(workspace, torch.float64, "workspace"), workspace.numel() * 8, _stream()))


# ---- posterior-predictive band, device-resident (trpl_predictive_*_dev) ----
def predictive_state(ncol):
    """The running state (5, ncol) f64 of a predictive band over ncol time columns: sw, mean, M2, lo, hi per column.
    Uninitialised: predictive_init_device sets it."""
    import torch
    if int(_abi.lib().trpl_predictive_state_bytes(int(ncol))) <= 0:
        raise ValueError("ncol = %r is outside what trpl_predictive accepts" % (ncol,))
    return torch.empty((5, int(ncol)), dtype=torch.float64, device="cuda")


def predictive_workspace(rows, ncol, elem):
    """A workspace tensor for predictive_accumulate_device over a (rows, >= ncol) block of `elem`-byte PL elements."""
    import torch
    n = int(_abi.lib().trpl_predictive_workspace_bytes(int(rows), int(ncol), int(elem)))
    if n <= 0:
        raise ValueError("rows, ncol, elem = %r are outside what trpl_predictive accepts" % ((rows, ncol, elem),))
    return torch.empty(n // 8, dtype=torch.float64, device="cuda")


def predictive_init_device(state):
    """trpl_predictive_init_dev: no row seen yet (sw = 0, lo = +inf, hi = -inf)."""
    import torch
    if state.dim() != 2 or state.shape[0] != 5:
        raise ValueError("state must be (5, ncol)")
    _abi.check(_abi.lib().trpl_predictive_init_dev(_chk(state, torch.float64, "state"), state.shape[1], _stream()))


def predictive_accumulate_device(pl, W, state, workspace, mag=None, status=None, ncol=None, flags=0):
    """trpl_predictive_accumulate_dev: add the used rows of pl (rows, ld) f32/f64 -- W (rows,) f64 finite and > 0, status
    (rows,) int32 zero or absent -- to state (5, ncol): y = log10 PL + mag (rows,) f64, formed as loglik_from_pl_device
    forms it (flags: FLAG_NORMALIZE, FLAG_PL_F32).  ncol defaults to ld."""
    import torch
    if pl.dim() != 2 or pl.dtype not in (torch.float32, torch.float64):
        raise ValueError("pl must be a 2-D float32/float64 tensor")
    rows, ld = pl.shape
    ncol = int(ld if ncol is None else ncol)
    if tuple(W.shape) != (rows,) or tuple(state.shape) != (5, ncol) or (mag is not None and tuple(mag.shape) != (rows,)) \
            or (status is not None and tuple(status.shape) != (rows,)):
        raise ValueError("shape mismatch")
    _abi.check(_abi.lib().trpl_predictive_accumulate_dev(
        _chk(pl, pl.dtype, "pl"), pl.element_size(), rows, ncol, ld, None if mag is None else _chk(mag, torch.float64, "mag"),
        _chk(W, torch.float64, "W"), None if status is None else _chk(status, torch.int32, "status"), int(flags),
        _chk(state, torch.float64, "state"), _chk(workspace, torch.float64, "workspace"), workspace.numel() * 8, _stream()))


def predictive_finish_device(state, out):
    """trpl_predictive_finish_dev: out (5, ncol) f64 <- mean, var, lo, hi, sw of the rows accumulated so far."""
    import torch
    if state.dim() != 2 or state.shape[0] != 5 or out.shape != state.shape:
        raise ValueError("state and out must be (5, ncol)")
    _abi.check(_abi.lib().trpl_predictive_finish_dev(_chk(state, torch.float64, "state"), state.shape[1],
                                                     _chk(out, torch.float64, "out"), _stream()))


# ---- weighted quantiles of many columns under one weight vector (trpl_weighted_quantiles_dev, trpl_predictive_gather_dev) ----
def quantile_requests(q, rule=None):
    """(q, rule) as the host arrays trpl_weighted_quantiles* takes: q a number or a sequence of numbers in (0, 1); rule None
    (Q_LAST_BELOW for q < 0.5, else Q_FIRST_ABOVE: the two ends of a credible interval and the median above), one rule, or
    one per q."""
    q = np.atleast_1d(np.ascontiguousarray(q, dtype=np.float64))
    if q.ndim != 1:
        raise ValueError("q must be a number or a one-dimensional sequence")
    if rule is None:
        rule = np.where(q < 0.5, _abi.Q_LAST_BELOW, _abi.Q_FIRST_ABOVE)
    rule = np.ascontiguousarray(np.broadcast_to(np.asarray(rule, dtype=np.int32), q.shape))
    return q, rule


def weighted_quantiles_device(Y, Wq, q, out, rule=None, n=None, flags=0):
    """trpl_weighted_quantiles_dev: out (K, ncols) f64 <- the K weighted quantiles of every column of the store Y (ncols, ldy)
    f64 -- column c's n (default ldy) keys contiguous in row c of the tensor -- under the weights Wq (>= n,) f64 shared by
    all columns (a row counts iff its weight is finite and > 0).  q, rule: quantile_requests."""
    import torch
    q, rule = quantile_requests(q, rule)
    if Y.dim() != 2 or Wq.dim() != 1:
        raise ValueError("Y must be (ncols, ldy) and Wq one-dimensional")
    ncols, ldy = Y.shape
    n = int(ldy if n is None else n)
    if Wq.shape[0] < n or tuple(out.shape) != (q.size, ncols):
        raise ValueError("Wq must hold n weights and out must be (K, ncols)")
    _abi.check(_abi.lib().trpl_weighted_quantiles_dev(_chk(Y, torch.float64, "Y"), ncols, n, ldy, _chk(Wq, torch.float64, "Wq"),
                                                      _abi.ptr(q), _abi.ptr(rule), q.size, int(flags),
                                                      _chk(out, torch.float64, "out"), _stream()))


def predictive_gather_device(pl, W, Y, Wq, row0=0, mag=None, status=None, ncol=None, flags=0):
    """trpl_predictive_gather_dev: the y = log10 PL + mag of the block pl (rows, ld) f32/f64, as predictive_accumulate_device
    forms them, transposed into the store: Y[i, row0 + j] = y[j, i] for Y (ncol, ldy) f64, and Wq[row0 + j] = W[j] for a
    used row (weight finite and > 0, status zero or absent), else 0."""
    import torch
    if pl.dim() != 2 or pl.dtype not in (torch.float32, torch.float64):
        raise ValueError("pl must be a 2-D float32/float64 tensor")
    rows, ld = pl.shape
    ncol = int(ld if ncol is None else ncol)
    if Y.dim() != 2 or Y.shape[0] != ncol or Wq.dim() != 1 or Wq.shape[0] < int(row0) + rows or tuple(W.shape) != (rows,) \
            or (mag is not None and tuple(mag.shape) != (rows,)) or (status is not None and tuple(status.shape) != (rows,)):
        raise ValueError("shape mismatch")
    _abi.check(_abi.lib().trpl_predictive_gather_dev(
        _chk(pl, pl.dtype, "pl"), pl.element_size(), rows, ncol, ld, None if mag is None else _chk(mag, torch.float64, "mag"),
        _chk(W, torch.float64, "W"), None if status is None else _chk(status, torch.int32, "status"), int(flags),
        _chk(Y, torch.float64, "Y"), Y.shape[1], int(row0), _chk(Wq, torch.float64, "Wq"), _stream()))


def convolve_irf_device(pl, h, k0, out, ncol=None):
    """trpl_convolve_irf_dev: out (rows, out_ld) <- the block pl (rows, ld) f32/f64, as solve_pl_device wrote it, convolved
    with the instrument response h (K,) f64 whose tap k0 sits at time zero: out[r, j] = sum_k h[k] pl[r, j + k0 - k] for
    j < ncol - k0, in fp64 and in ascending k (include/trpl.h).  out has pl's dtype and at least ncol - k0 columns; the columns
    beyond are not written.  ncol (default ld): the valid columns of pl."""
    import torch
    if pl.dim() != 2 or pl.dtype not in (torch.float32, torch.float64):
        raise ValueError("pl must be a 2-D float32/float64 tensor")
    rows, ld = pl.shape
    ncol = int(ld if ncol is None else ncol)
    if h.dim() != 1 or out.dim() != 2 or out.dtype != pl.dtype or out.shape[0] != rows:
        raise ValueError("h must be (K,) and out (rows, >= ncol - k0) of pl's dtype")
    if out.shape[1] < ncol - int(k0):
        raise ValueError("out must have at least ncol - k0 = %d columns, got %d" % (ncol - int(k0), out.shape[1]))
    _abi.check(_abi.lib().trpl_convolve_irf_dev(_chk(pl, pl.dtype, "pl"), pl.element_size(), rows, ncol, ld, _chk(h, torch.float64, "h"),
                                                h.shape[0], int(k0), _chk(out, out.dtype, "out"), out.shape[1], _stream()))


def loglik_irf_bank_device(pl, H, k0, obs, mag, sse, esum=None, wts=None, obs_hi=None, obs_dx=None, obs_h=None, ncol=None, flags=0,
                           status=None):
    """trpl_loglik_irf_bank_dev: the block pl (rows, ld) f32/f64, as solve_pl_device wrote it, scored against the bank H (J, K) f64
    of instrument responses whose tap k0 sits at time zero: sse (J, rows) f64 and esum (J, rows) f64 (optional) receive, per
    response, the bits of convolve_irf_device followed by loglik_moments_from_pl_device (with wts (n_obs,) f64:
    loglik_weighted_from_pl_device) on the same obs (n_obs,), brackets, mag (rows,) and status (rows,) int32 -- without the
    convolved block ever being written.  ncol (default ld): the valid columns of pl."""
    import torch
    f64 = torch.float64
    if pl.dim() != 2 or pl.dtype not in (torch.float32, torch.float64):
        raise ValueError("pl must be a 2-D float32/float64 tensor")
    rows, ld = pl.shape
    if H.dim() != 2 or obs.dim() != 1 or tuple(mag.shape) != (rows,) or tuple(sse.shape) != (H.shape[0], rows):
        raise ValueError("H must be (J, K), obs (n_obs,), mag (rows,) and sse (J, rows)")
    if (esum is not None and esum.shape != sse.shape) or (wts is not None and wts.shape != obs.shape) \
            or (status is not None and tuple(status.shape) != (rows,)):
        raise ValueError("shape mismatch")
    _abi.check(_abi.lib().trpl_loglik_irf_bank_dev(
        _chk(pl, pl.dtype, "pl"), pl.element_size(), rows, int(ld if ncol is None else ncol), ld, _chk(H, f64, "H"), H.shape[0],
        H.shape[1], int(k0), _chk(obs, f64, "obs"), *_brackets(obs, obs_hi, obs_dx, obs_h), obs.shape[0], _opt(wts, f64, "wts"),
        _chk(mag, f64, "mag"), _opt(status, torch.int32, "status"), _chk(sse, f64, "sse"), _opt(esum, f64, "esum"), int(flags),
        _stream()))


def irf_bank_profile_device(Pbank, best, P):
    """trpl_irf_bank_profile_dev: P (S,) f64 <- the greatest Pbank[j, s] of Pbank (J, S) f64, best (S,) int32 <- the first j that
    attains it; where every value is -inf or NaN, best = -1 and P = -inf."""
    import torch
    if Pbank.dim() != 2 or tuple(best.shape) != (Pbank.shape[1],) or tuple(P.shape) != (Pbank.shape[1],):
        raise ValueError("Pbank must be (J, S), best and P (S,)")
    _abi.check(_abi.lib().trpl_irf_bank_profile_dev(_chk(Pbank, torch.float64, "Pbank"), Pbank.shape[0], Pbank.shape[1],
                                                    _chk(best, torch.int32, "best"), _chk(P, torch.float64, "P"), _stream()))


def nuisance_flags(mag, marginal):
    """(flags, offsets) of a trpl_nuisance_reduce call: mag "fixed", "profile" or a sequence of offsets (grid mode); offsets is a
    host float64 array or None."""
    if isinstance(mag, str):
        if mag not in ("fixed", "profile"):
            raise ValueError('mag must be "fixed", "profile" or a sequence of offsets, got %r' % (mag,))
        flags, off = (_abi.NUISANCE_MAG_FIXED if mag == "fixed" else _abi.NUISANCE_MAG_PROFILE), None
    else:
        off = np.ascontiguousarray(mag, dtype=np.float64).ravel()
        flags = _abi.NUISANCE_MAG_GRID
    return flags | (_abi.NUISANCE_MARGINAL if marginal else 0), off


def nuisance_reduce_device(sse, esum, wsum, P, best=None, best_mag=None, mag="fixed", marginal=False, tf=1.0, log_prior=None):
    """trpl_nuisance_reduce_dev: P (S,) f64 <- the reduction over the nuisance grid, J responses x M magnitude offsets, of the
    moments sse, esum (C, J, S) f64 as loglik_irf_bank_device wrote them curve by curve (esum may be None with mag="fixed");
    wsum a host sequence (C,), n_obs or the sum of each curve's weights.  mag: "fixed" (M = 1, the offset 0), "profile" (M = 1,
    the likelihood-maximising offset per response) or a host sequence of M offsets (the grid).  marginal=False: the greatest
    cell; True: tf * log sum_i exp(v_i / tf + log_prior_i) (include/trpl.h).  log_prior (J * M,) or (J, M): a float64 CUDA tensor,
    used as it is (NaN and +inf are the caller's to exclude), or a host array, checked and uploaded; marginal only.  best (S,)
    int32 and best_mag (S,) f64, optional: the first cell j * M + m that attains the maximum and its offset."""
    import torch
    f64 = torch.float64
    if sse.dim() != 3:
        raise ValueError("sse must be (C, J, S)")
    Cn, J, S = sse.shape
    flags, off = nuisance_flags(mag, marginal)
    M = 1 if off is None else len(off)
    wsum = np.ascontiguousarray(np.broadcast_to(np.asarray(wsum, dtype=np.float64), (Cn,)))
    if (esum is not None and esum.shape != sse.shape) or tuple(P.shape) != (S,) \
            or any(t is not None and tuple(t.shape) != (S,) for t in (best, best_mag)):
        raise ValueError("shape mismatch")
    if log_prior is not None and not isinstance(log_prior, torch.Tensor):
        lp = np.ascontiguousarray(log_prior, dtype=np.float64)
        if marginal and (np.isnan(lp).any() or (lp == np.inf).any()):
            raise ValueError("log_prior must not hold NaN or +inf")
        log_prior = torch.from_numpy(lp).to(sse.device)
    if log_prior is not None and log_prior.numel() != J * M:
        raise ValueError("log_prior must hold J * M = %d entries, got %d" % (J * M, log_prior.numel()))
    _abi.check(_abi.lib().trpl_nuisance_reduce_dev(
        _chk(sse, f64, "sse"), _opt(esum, f64, "esum"), _abi.ptr(wsum), S, Cn, J, None if off is None else _abi.ptr(off), M,
        _opt(log_prior, f64, "log_prior"), float(tf), flags, _chk(P, f64, "P"), _opt(best, torch.int32, "best"),
        _opt(best_mag, f64, "best_mag"), _stream()))


def posterior_hist_device(x, W, lo, hi, out, y=None, ylo=0.0, yhi=1.0):
    """out (bins,) or (bins, ybins) += weighted counts (W None: counts); the caller zeroes out."""
    import torch
    xb = out.shape[0]
    yb = out.shape[1] if y is not None else 1
    _abi.check(_abi.lib().trpl_posterior_hist_dev(
        _chk(x, torch.float64, "x"), None if y is None else _chk(y, torch.float64, "y"),
        None if W is None else _chk(W, torch.float64, "W"), x.shape[0], float(lo), float(hi), int(xb), float(ylo),
        float(yhi), int(yb), _chk(out, torch.float64, "out"), _stream()))


# ---- the corner, device-resident (trpl_corner_*_dev) ----
def corner_workspace(S, D):
    """A workspace tensor for corner_hist_device with S samples and D columns (one key byte per sample and column)."""
    import torch
    n = int(_abi.lib().trpl_corner_workspace_bytes(int(S), int(D)))
    if n <= 0:
        raise ValueError("S, D = %r are outside what trpl_corner_hist_dev accepts" % ((S, D),))
    return torch.empty(n, dtype=torch.uint8, device="cuda")


def corner_columns_device(X, cols, V, do_log=None, thickness=2000.0, excl_lo=None, excl_hi=None, LL=None, LLk=None, kept=None):
    """V (D, S) <- the columns `cols` (TRPL_COL_* codes, host sequence) of the samples X (S, ld >= 13) f64, log10 where
    do_log[d]; excl_lo / excl_hi (host, 13 each, NaN = not tested): LLk (S,) <- LL for a kept sample, NaN otherwise, and kept
    (1,) int64 <- their number (trpl_corner_columns_dev)."""
    import torch
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    lg = np.zeros(cols.size, dtype=np.int32) if do_log is None else np.ascontiguousarray(do_log, dtype=np.int32)
    if X.dim() != 2 or cols.ndim != 1 or lg.shape != cols.shape or tuple(V.shape) != (cols.size, X.shape[0]):
        raise ValueError("X must be (S, ld), V (D, S) with D = len(cols) = len(do_log)")
    S, ldx = X.shape
    lo = None if excl_lo is None else np.ascontiguousarray(excl_lo, dtype=np.float64)
    hi = None if excl_hi is None else np.ascontiguousarray(excl_hi, dtype=np.float64)
    for a in (lo, hi):
        if a is not None and a.shape != (_abi.CORNER_PRIMARY,):
            raise ValueError("excl_lo and excl_hi must have %d entries" % _abi.CORNER_PRIMARY)
    for t, name in ((LL, "LL"), (LLk, "LLk")):
        if t is not None and tuple(t.shape) != (S,):
            raise ValueError("%s must be (S,)" % name)
    _abi.check(_abi.lib().trpl_corner_columns_dev(
        _chk(X, torch.float64, "X"), S, ldx, _abi.ptr(cols), _abi.ptr(lg), cols.size, float(thickness), _abi.ptr(lo), _abi.ptr(hi),
        None if LL is None else _chk(LL, torch.float64, "LL"), _chk(V, torch.float64, "V"),
        None if LLk is None else _chk(LLk, torch.float64, "LLk"), None if kept is None else _chk(kept, torch.int64, "kept"),
        _stream()))


def corner_hist_device(V, W, lo, hi, h1, workspace, c1=None, h2=None):
    """Every marginal of the columns V (D, S) under the weights W (S,): h1 (D, bins) weighted sums, c1 (D, bins) plain counts,
    h2 (D (D - 1) / 2, bins, bins) in the reference's pair order; lo, hi host sequences of D limits.  Each bin is the sum of
    its samples' weights in ascending sample index: the same bits in every run (trpl_corner_hist_dev)."""
    import torch
    D, S = V.shape
    bins = h1.shape[1] if h1.dim() == 2 else -1
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    if tuple(W.shape) != (S,) or lo.shape != (D,) or hi.shape != (D,) or tuple(h1.shape) != (D, bins) \
            or (c1 is not None and tuple(c1.shape) != (D, bins)) \
            or (h2 is not None and tuple(h2.shape) != (D * (D - 1) // 2, bins, bins)):
        raise ValueError("shape mismatch")
    if workspace.numel() * workspace.element_size() < int(_abi.lib().trpl_corner_workspace_bytes(S, D)):
        raise ValueError("workspace too small: see corner_workspace")
    _abi.check(_abi.lib().trpl_corner_hist_dev(
        _chk(V, torch.float64, "V"), S, S, D, _chk(W, torch.float64, "W"), _abi.ptr(lo), _abi.ptr(hi), int(bins),
        _chk(h1, torch.float64, "h1"), None if c1 is None else _chk(c1, torch.float64, "c1"),
        None if h2 is None or h2.numel() == 0 else _chk(h2, torch.float64, "h2"), _chk(workspace, workspace.dtype, "workspace"), _stream()))


# ---- refinement generations, device-resident (trpl_refine_*_dev) ----
def _refine_box(minX, maxX, do_log):
    lo = np.ascontiguousarray(minX, dtype=np.float64)
    hi = np.ascontiguousarray(maxX, dtype=np.float64)
    lg = np.ascontiguousarray(do_log, dtype=np.int32)
    if not (lo.shape == hi.shape == lg.shape and lo.ndim == 1):
        raise ValueError("minX, maxX and do_log must be one-dimensional and of equal length")
    return lo, hi, lg


def refine_workspace(S):
    """A workspace tensor for refine_resample_device over S weights."""
    import torch
    n = int(_abi.lib().trpl_refine_workspace_bytes(int(S)))
    if n <= 0:
        raise ValueError("S = %r is outside what trpl_refine_resample_dev accepts" % (S,))
    return torch.empty((n + 7) // 8, dtype=torch.float64, device="cuda")


def refine_resample_device(W, idx, workspace, offset=0.5, stats=None):
    """trpl_refine_resample_dev: idx (K,) int64 <- the K systematic draws of the weights W (S,) f64 (NaN or <= 0 counts as 0;
    -1 everywhere when no weight is left), stats (3,) f64 optional <- sum w, sum w^2, (sum w)^2 / sum w^2."""
    import torch
    if W.dim() != 1 or idx.dim() != 1 or (stats is not None and tuple(stats.shape) != (3,)):
        raise ValueError("W must be (S,), idx (K,) and stats (3,)")
    _abi.check(_abi.lib().trpl_refine_resample_dev(
        _chk(W, torch.float64, "W"), W.shape[0], idx.shape[0], float(offset), _chk(idx, torch.int64, "idx"),
        None if stats is None else _chk(stats, torch.float64, "stats"), _chk(workspace, torch.float64, "workspace"),
        workspace.numel() * 8, _stream()))


def refine_draw_device(a, b, m, n_uniform, seed, generation, minX, maxX, do_log, U2, X2, flags=0):
    """trpl_refine_draw_dev: the n_uniform + K m children of the boxes a, b (K, A) f64 -- U2 (S_g, A) unit coordinates, X2
    (S_g, ncol) the samples in the box's units; minX, maxX, do_log host sequences, flags the TRPL_BOX_EQUAL_* bits."""
    import torch
    lo, hi, lg = _refine_box(minX, maxX, do_log)
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError("a and b must be (K, A)")
    K, A = a.shape
    total = int(n_uniform) + K * int(m)
    if tuple(U2.shape) != (total, A) or tuple(X2.shape) != (total, lo.size):
        raise ValueError("U2 must be (n_uniform + K m, A) and X2 (n_uniform + K m, ncol)")
    _abi.check(_abi.lib().trpl_refine_draw_dev(
        _chk(a, torch.float64, "a"), _chk(b, torch.float64, "b"), K, A, int(m), int(n_uniform), int(seed) & 0xFFFFFFFFFFFFFFFF,
        int(generation) & 0xFFFFFFFF, lo.size, _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg), int(flags),
        _chk(U2, torch.float64, "U2"), _chk(X2, torch.float64, "X2"), _stream()))


def refine_density_device(U, a, b, inv_vol, B, A=None):
    """trpl_refine_density_dev: B (S,) <- the sum of inv_vol (K,) over the closed boxes a, b (K, A) that hold each row of U
    (S, ldu >= A), in ascending k: the sequential loop's bits."""
    import torch
    if U.dim() != 2 or a.dim() != 2 or a.shape != b.shape or tuple(inv_vol.shape) != (a.shape[0],) or tuple(B.shape) != (U.shape[0],):
        raise ValueError("U must be (S, ldu), a and b (K, A), inv_vol (K,) and B (S,)")
    K, Ab = a.shape
    A = Ab if A is None else int(A)
    if A != Ab:
        raise ValueError("A must be the boxes' number of dimensions")
    _abi.check(_abi.lib().trpl_refine_density_dev(
        _chk(U, torch.float64, "U"), U.shape[0], U.shape[1], A, _chk(a, torch.float64, "a"), _chk(b, torch.float64, "b"),
        _chk(inv_vol, torch.float64, "inv_vol"), K, _chk(B, torch.float64, "B"), _stream()))


def refine_unit_device(X, minX, maxX, do_log, U, flags=0):
    """trpl_refine_unit_dev: U (S, A) <- the unit coordinates of the active columns of X (S, ld >= ncol)."""
    import torch
    lo, hi, lg = _refine_box(minX, maxX, do_log)
    if X.dim() != 2 or U.dim() != 2 or U.shape[0] != X.shape[0]:
        raise ValueError("X must be (S, ld) and U (S, A)")
    _abi.check(_abi.lib().trpl_refine_unit_dev(
        _chk(X, torch.float64, "X"), X.shape[0], X.shape[1], lo.size, _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg), int(flags),
        U.shape[1], _chk(U, torch.float64, "U"), _stream()))


def refine_affine_device(U, M, c, Z, A=None):
    """trpl_refine_affine_dev: Z (S, ldz >= A) <- M (U (S, ldu >= A) - c); M (A, A) lower triangular and c (A,) host arrays (only
    j <= i of M is read), z_i = sum_{j <= i} M_ij (u_j - c_j) in ascending j."""
    import torch
    M = np.ascontiguousarray(M, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if U.dim() != 2 or Z.dim() != 2 or Z.shape[0] != U.shape[0] or M.ndim != 2 or M.shape[0] != M.shape[1] or c.shape != (M.shape[0],):
        raise ValueError("U must be (S, ldu), Z (S, ldz), M (A, A) and c (A,)")
    if A is not None and int(A) != M.shape[0]:
        raise ValueError("A must be M's number of dimensions")
    _abi.check(_abi.lib().trpl_refine_affine_dev(
        _chk(U, torch.float64, "U"), U.shape[0], U.shape[1], M.shape[0], _abi.ptr(M), _abi.ptr(c), _chk(Z, torch.float64, "Z"),
        Z.shape[1], _stream()))


def refine_draw_oriented_device(zc, h, L, c, m, n_uniform, seed, generation, minX, maxX, do_log, Z2, U2, X2, inside, flags=0):
    """trpl_refine_draw_oriented_dev: the n_uniform + K m children of the boxes [zc - h, zc + h] in z, zc (K, A) f64 on the device;
    h (A,), L (A, A) lower triangular and c (A,) host arrays.  Z2, U2 (S_g, A), X2 (S_g, ncol) f64 and inside (S_g,) int32 (0: the
    child left the unit cube; it is not to be solved)."""
    import torch
    lo, hi, lg = _refine_box(minX, maxX, do_log)
    h = np.ascontiguousarray(h, dtype=np.float64)
    L = np.ascontiguousarray(L, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if zc.dim() != 2:
        raise ValueError("zc must be (K, A)")
    K, A = zc.shape
    if h.shape != (A,) or L.shape != (A, A) or c.shape != (A,):
        raise ValueError("h must be (A,), L (A, A) and c (A,)")
    total = int(n_uniform) + K * int(m)
    if tuple(Z2.shape) != (total, A) or tuple(U2.shape) != (total, A) or tuple(X2.shape) != (total, lo.size) or tuple(inside.shape) != (total,):
        raise ValueError("Z2 and U2 must be (n_uniform + K m, A), X2 (n_uniform + K m, ncol) and inside (n_uniform + K m,)")
    _abi.check(_abi.lib().trpl_refine_draw_oriented_dev(
        _chk(zc, torch.float64, "zc"), _abi.ptr(h), _abi.ptr(L), _abi.ptr(c), K, A, int(m), int(n_uniform),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(generation) & 0xFFFFFFFF, lo.size, _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg), int(flags),
        _chk(Z2, torch.float64, "Z2"), _chk(U2, torch.float64, "U2"), _chk(X2, torch.float64, "X2"), _chk(inside, torch.int32, "inside"),
        _stream()))


# ---- ensemble Metropolis sampling, device-resident (trpl_mcmc_*_dev).  These calls are bound by their launch, 10 to 20 us each, so
# every wrapper marshals its own call: a marshaller shared by a pair, as mcmc.py has for the host-buffer calls, costs a Python frame
# per call, which shows at this size.
_M64, _M32 = _abi.SEED_MASK, _abi.STEP_MASK


def mcmc_propose_device(U, partners, gamma, scale, chain0, seed, step, minX, maxX, do_log, Up, Xp, inside, flags=0):
    """trpl_mcmc_propose_dev: Up (count, A), Xp (count, ncol) f64 and inside (count,) int32 <- one symmetric proposal per chain of U
    (count, A) f64: u' = (u + gamma (pa - pb)) + scale (2 xi - 1) with two distinct rows of partners (P >= 2, A), or the random walk
    u' = u + scale (2 xi - 1) with partners None.  scale (A,) is a host array (a scalar is broadcast); chain0 is the ensemble index of
    the first row, which keys its Philox stream.  flags: the TRPL_BOX_EQUAL_* bits and _abi.MCMC_FOLD (TRPL_MCMC_FOLD,
    include/trpl.h): with it a u' that leaves the unit cube is reflected back at the faces, and inside is a code -- 0 some coordinate
    is not finite, 1 nothing needed folding, 2 at least one coordinate was folded; without it inside is 0 (outside) or 1."""
    import torch
    lo, hi, lg = _refine_box(minX, maxX, do_log)
    if U.dim() != 2:
        raise ValueError("U must be (count, A)")
    count, A = U.shape
    scale = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (A,)))
    if partners is not None and (partners.dim() != 2 or partners.shape[1] != A):
        raise ValueError("partners must be (P, A)")
    if tuple(Up.shape) != (count, A) or tuple(Xp.shape) != (count, lo.size) or tuple(inside.shape) != (count,):
        raise ValueError("Up must be (count, A), Xp (count, ncol) and inside (count,)")
    _abi.check(_abi.lib().trpl_mcmc_propose_dev(
        _chk(U, torch.float64, "U"), _opt(partners, torch.float64, "partners"), count, 0 if partners is None else partners.shape[0], A,
        float(gamma), _abi.ptr(scale), int(chain0), int(seed) & _M64, int(step) & _M32, lo.size, _abi.ptr(lo),
        _abi.ptr(hi), _abi.ptr(lg), int(flags), _chk(Up, torch.float64, "Up"), _chk(Xp, torch.float64, "Xp"),
        _chk(inside, torch.int32, "inside"), _stream()))


def mcmc_accept_device(U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step, accepted):
    """trpl_mcmc_accept_dev: the Metropolis step of every chain at temperature tf.  U (count, A), X (count, ncol) and LL (count,) f64
    take the rows of Up, Xp, LLp where the proposal is accepted and keep theirs elsewhere; accepted (count,) int32 says which."""
    import torch
    if U.dim() != 2 or X.dim() != 2 or X.shape[0] != U.shape[0] or Up.shape != U.shape or Xp.shape != X.shape:
        raise ValueError("U and Up must be (count, A), X and Xp (count, ncol)")
    count = U.shape[0]
    if tuple(LL.shape) != (count,) or tuple(LLp.shape) != (count,) or tuple(inside.shape) != (count,) or tuple(accepted.shape) != (count,):
        raise ValueError("LL, LLp, inside and accepted must be (count,)")
    _abi.check(_abi.lib().trpl_mcmc_accept_dev(
        _chk(U, torch.float64, "U"), _chk(X, torch.float64, "X"), _chk(LL, torch.float64, "LL"), _chk(Up, torch.float64, "Up"),
        _chk(Xp, torch.float64, "Xp"), _chk(LLp, torch.float64, "LLp"), _chk(inside, torch.int32, "inside"), count, U.shape[1], X.shape[1],
        float(tf), int(chain0), int(seed) & _M64, int(step) & _M32, _chk(accepted, torch.int32, "accepted"), _stream()))


def mcmc_levels_device(LL, tf, chain0, seed, step, level):
    """trpl_mcmc_levels_dev: level (count,) f64 <- for every chain the sse level above which mcmc_accept_device, called with the same
    (tf, chain0, seed, step), is certain to reject the proposal: the cut_level of loglik_cut_levels_device, +inf where nothing may
    be cut (include/trpl.h).  LL (count,) f64 is the chains' current log-likelihood, minus the summed sse of a P started from zero."""
    import torch
    if LL.dim() != 1 or tuple(level.shape) != tuple(LL.shape):
        raise ValueError("LL and level must be (count,)")
    _abi.check(_abi.lib().trpl_mcmc_levels_dev(
        _chk(LL, torch.float64, "LL"), LL.shape[0], float(tf), int(chain0), int(seed) & _M64, int(step) & _M32,
        _chk(level, torch.float64, "level"), _stream()))


def _ladder(tf):
    tf = np.ascontiguousarray(tf, dtype=np.float64)
    if tf.ndim != 1 or tf.size < 1:
        raise ValueError("tf must be (K,), the temperatures of the rungs")
    return tf


def mcmc_propose_rungs_device(U, partners, group, gamma, scale, chain0, seed, step, minX, maxX, do_log, Up, Xp, inside, flags=0):
    """trpl_mcmc_propose_rungs_dev: mcmc_propose_device for a block of rungs of `group` chains each (parallel tempering, include/trpl.h):
    chain i of U (count, A) takes its two partners from the rows [(i // group) group, + group) of partners (P, A), P a multiple of
    group and count <= P.  Rung k's rows are mcmc_propose_device's on that slice with that partner block and chain0 + k group."""
    import torch
    lo, hi, lg = _refine_box(minX, maxX, do_log)
    if U.dim() != 2:
        raise ValueError("U must be (count, A)")
    count, A = U.shape
    scale = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (A,)))
    if partners is None or partners.dim() != 2 or partners.shape[1] != A:
        raise ValueError("partners must be (P, A)")
    if tuple(Up.shape) != (count, A) or tuple(Xp.shape) != (count, lo.size) or tuple(inside.shape) != (count,):
        raise ValueError("Up must be (count, A), Xp (count, ncol) and inside (count,)")
    _abi.check(_abi.lib().trpl_mcmc_propose_rungs_dev(
        _chk(U, torch.float64, "U"), _chk(partners, torch.float64, "partners"), count, partners.shape[0], int(group), A, float(gamma),
        _abi.ptr(scale), int(chain0), int(seed) & _M64, int(step) & _M32, lo.size, _abi.ptr(lo), _abi.ptr(hi),
        _abi.ptr(lg), int(flags), _chk(Up, torch.float64, "Up"), _chk(Xp, torch.float64, "Xp"), _chk(inside, torch.int32, "inside"),
        _stream()))


def mcmc_accept_rungs_device(U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step, accepted):
    """trpl_mcmc_accept_rungs_dev: mcmc_accept_device with a temperature per rung.  tf (K,) is a host array; the count rows are K rungs
    of count / K chains, and chain i decides at tf[i // (count / K)]."""
    import torch
    tf = _ladder(tf)
    if U.dim() != 2 or X.dim() != 2 or X.shape[0] != U.shape[0] or Up.shape != U.shape or Xp.shape != X.shape:
        raise ValueError("U and Up must be (count, A), X and Xp (count, ncol)")
    count = U.shape[0]
    if tuple(LL.shape) != (count,) or tuple(LLp.shape) != (count,) or tuple(inside.shape) != (count,) or tuple(accepted.shape) != (count,):
        raise ValueError("LL, LLp, inside and accepted must be (count,)")
    if count % tf.size:
        raise ValueError("count = %d is no multiple of the %d rungs" % (count, tf.size))
    _abi.check(_abi.lib().trpl_mcmc_accept_rungs_dev(
        _chk(U, torch.float64, "U"), _chk(X, torch.float64, "X"), _chk(LL, torch.float64, "LL"), _chk(Up, torch.float64, "Up"),
        _chk(Xp, torch.float64, "Xp"), _chk(LLp, torch.float64, "LLp"), _chk(inside, torch.int32, "inside"), count, U.shape[1], X.shape[1],
        tf.size, count // tf.size, _abi.ptr(tf), int(chain0), int(seed) & _M64, int(step) & _M32,
        _chk(accepted, torch.int32, "accepted"), _stream()))


def mcmc_levels_rungs_device(LL, tf, chain0, seed, step, level):
    """trpl_mcmc_levels_rungs_dev: mcmc_levels_device with a temperature per rung, tf (K,) a host array: the levels that
    mcmc_accept_rungs_device, called with the same (tf, chain0, seed, step), is certain to reject above."""
    import torch
    tf = _ladder(tf)
    if LL.dim() != 1 or tuple(level.shape) != tuple(LL.shape):
        raise ValueError("LL and level must be (count,)")
    if LL.shape[0] % tf.size:
        raise ValueError("count = %d is no multiple of the %d rungs" % (LL.shape[0], tf.size))
    _abi.check(_abi.lib().trpl_mcmc_levels_rungs_dev(
        _chk(LL, torch.float64, "LL"), LL.shape[0], tf.size, LL.shape[0] // tf.size, _abi.ptr(tf), int(chain0),
        int(seed) & _M64, int(step) & _M32, _chk(level, torch.float64, "level"), _stream()))


def mcmc_swap_device(U, X, LL, tf, parity, chain0, seed, step, swapped):
    """trpl_mcmc_swap_dev: the replica exchange between adjacent rungs of one block.  U (K group, A), X (K group, ncol) and LL (K
    group,) f64 are exchanged IN PLACE between the rows k group + c and (k + 1) group + c for k = parity, parity + 2, ..; tf (K,) is
    a host array; swapped (K group,) int32 is 1 on both rows of an exchanged pair, 0 elsewhere (include/trpl.h has the rule)."""
    import torch
    tf = _ladder(tf)
    if U.dim() != 2 or X.dim() != 2 or X.shape[0] != U.shape[0]:
        raise ValueError("U must be (K group, A) and X (K group, ncol)")
    count = U.shape[0]
    if tuple(LL.shape) != (count,) or tuple(swapped.shape) != (count,):
        raise ValueError("LL and swapped must be (K group,)")
    if count % tf.size:
        raise ValueError("the %d rows are no multiple of the %d rungs" % (count, tf.size))
    _abi.check(_abi.lib().trpl_mcmc_swap_dev(
        _chk(U, torch.float64, "U"), _chk(X, torch.float64, "X"), _chk(LL, torch.float64, "LL"), tf.size, count // tf.size, U.shape[1],
        X.shape[1], _abi.ptr(tf), int(parity), int(chain0), int(seed) & _M64, int(step) & _M32,
        _chk(swapped, torch.int32, "swapped"), _stream()))


def mcmc_propose_stretch_device(U, partners, group, a, chain0, seed, step, minX, maxX, do_log, Up, Xp, inside, z, lnq, flags=0):
    """trpl_mcmc_propose_stretch_dev: Up (count, A), Xp (count, ncol), z (count,), lnq (count,) f64 and inside (count,) int32 <- one
    stretch proposal per chain of U (count, A) f64 (Goodman & Weare 2010): u' = p + z (u - p), p a row of the chain's rung [(i //
    group) group, + group) of partners (P, A), z = ((a - 1) xi + 1)^2 / a, lnq = (A - 1) log(z) the h of mcmc_accept_h_device.  group
    None: one rung of P.  flags: the TRPL_BOX_EQUAL_* bits; _abi.MCMC_FOLD is refused."""
    import torch
    lo, hi, lg = _refine_box(minX, maxX, do_log)
    if U.dim() != 2:
        raise ValueError("U must be (count, A)")
    count, A = U.shape
    if partners is None or partners.dim() != 2 or partners.shape[1] != A:
        raise ValueError("partners must be (P, A)")
    if tuple(Up.shape) != (count, A) or tuple(Xp.shape) != (count, lo.size) or not (
            tuple(inside.shape) == tuple(z.shape) == tuple(lnq.shape) == (count,)):
        raise ValueError("Up must be (count, A), Xp (count, ncol) and inside, z and lnq (count,)")
    _abi.check(_abi.lib().trpl_mcmc_propose_stretch_dev(
        _chk(U, torch.float64, "U"), _chk(partners, torch.float64, "partners"), count, partners.shape[0],
        partners.shape[0] if group is None else int(group), A, float(a), int(chain0), int(seed) & _M64, int(step) & _M32, lo.size,
        _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg), int(flags), _chk(Up, torch.float64, "Up"), _chk(Xp, torch.float64, "Xp"),
        _chk(inside, torch.int32, "inside"), _chk(z, torch.float64, "z"), _chk(lnq, torch.float64, "lnq"), _stream()))


def mcmc_propose_subspace_device(U, partners, group, gamma_tab, scale, chain0, seed, step, minX, maxX, do_log, Up, Xp, inside, mask, sel,
                                 ncr=3, pcr=None, e_width=0.05, flags=0):
    """trpl_mcmc_propose_subspace_dev: Up (count, A), Xp (count, ncol) f64 and inside, mask, sel (count,) int32 <- one subspace
    differential-evolution proposal per chain of U (count, A) f64 (DREAM; include/trpl.h has the rule): a random subset of the
    coordinates moves along the sum of delta difference pairs of the chain's rung [(i // group) group, + group) of partners (P, A).
    gamma_tab (pairs, A) is a host array, the gamma by (delta - 1, selected - 1); pcr (ncr,) the host shares of the crossover classes,
    None for equal ones; scale (A,) as in mcmc_propose_device.  group None: one rung of P.  mask has bit d set where coordinate d
    moved, sel is delta | class << 8.  flags: the TRPL_BOX_EQUAL_* bits and _abi.MCMC_FOLD."""
    import torch
    lo, hi, lg = _refine_box(minX, maxX, do_log)
    if U.dim() != 2:
        raise ValueError("U must be (count, A)")
    count, A = U.shape
    scale = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (A,)))
    tab = np.ascontiguousarray(gamma_tab, dtype=np.float64)
    if tab.ndim != 2 or tab.shape[1] != A:
        raise ValueError("gamma_tab must be (pairs, A)")
    if pcr is not None:
        pcr = np.ascontiguousarray(pcr, dtype=np.float64)
        if pcr.shape != (int(ncr),):
            raise ValueError("pcr must be (ncr,)")
    if partners is None or partners.dim() != 2 or partners.shape[1] != A:
        raise ValueError("partners must be (P, A)")
    if tuple(Up.shape) != (count, A) or tuple(Xp.shape) != (count, lo.size) or not (
            tuple(inside.shape) == tuple(mask.shape) == tuple(sel.shape) == (count,)):
        raise ValueError("Up must be (count, A), Xp (count, ncol) and inside, mask and sel (count,)")
    _abi.check(_abi.lib().trpl_mcmc_propose_subspace_dev(
        _chk(U, torch.float64, "U"), _chk(partners, torch.float64, "partners"), count, partners.shape[0],
        partners.shape[0] if group is None else int(group), A, 1.0, _abi.ptr(scale), int(chain0), int(seed) & _M64, int(step) & _M32,
        lo.size, _abi.ptr(lo), _abi.ptr(hi), _abi.ptr(lg), int(flags), _chk(Up, torch.float64, "Up"), _chk(Xp, torch.float64, "Xp"),
        _chk(inside, torch.int32, "inside"), tab.shape[0], int(ncr), None if pcr is None else _abi.ptr(pcr), _abi.ptr(tab), float(e_width),
        _chk(mask, torch.int32, "mask"), _chk(sel, torch.int32, "sel"), _stream()))


def mcmc_accept_h_device(U, X, LL, Up, Xp, LLp, inside, h, tf, chain0, seed, step, accepted):
    """trpl_mcmc_accept_h_dev: mcmc_accept_rungs_device with an untempered log term h (count,) f64 per chain: d = (LLp - LL) / tf + h.
    tf (K,) is a host array, or a scalar for one temperature."""
    import torch
    tf = _ladder(np.atleast_1d(np.asarray(tf, dtype=np.float64)))
    if U.dim() != 2 or X.dim() != 2 or X.shape[0] != U.shape[0] or Up.shape != U.shape or Xp.shape != X.shape:
        raise ValueError("U and Up must be (count, A), X and Xp (count, ncol)")
    count = U.shape[0]
    if not (tuple(LL.shape) == tuple(LLp.shape) == tuple(inside.shape) == tuple(h.shape) == tuple(accepted.shape) == (count,)):
        raise ValueError("LL, LLp, inside, h and accepted must be (count,)")
    if count % tf.size:
        raise ValueError("count = %d is no multiple of the %d rungs" % (count, tf.size))
    _abi.check(_abi.lib().trpl_mcmc_accept_h_dev(
        _chk(U, torch.float64, "U"), _chk(X, torch.float64, "X"), _chk(LL, torch.float64, "LL"), _chk(Up, torch.float64, "Up"),
        _chk(Xp, torch.float64, "Xp"), _chk(LLp, torch.float64, "LLp"), _chk(inside, torch.int32, "inside"), _chk(h, torch.float64, "h"),
        count, U.shape[1], X.shape[1], tf.size, count // tf.size, _abi.ptr(tf), int(chain0), int(seed) & _M64, int(step) & _M32,
        _chk(accepted, torch.int32, "accepted"), _stream()))


def mcmc_levels_h_device(LL, h, tf, chain0, seed, step, level):
    """trpl_mcmc_levels_h_dev: level (count,) f64 <- the levels that mcmc_accept_h_device, called with the same (h, tf, chain0, seed,
    step), is certain to reject above; +inf also where h is NaN or infinite.  A level can be negative: pass max(level, 0) on."""
    import torch
    tf = _ladder(np.atleast_1d(np.asarray(tf, dtype=np.float64)))
    if LL.dim() != 1 or tuple(level.shape) != tuple(LL.shape) or tuple(h.shape) != tuple(LL.shape):
        raise ValueError("LL, h and level must be (count,)")
    if LL.shape[0] % tf.size:
        raise ValueError("count = %d is no multiple of the %d rungs" % (LL.shape[0], tf.size))
    _abi.check(_abi.lib().trpl_mcmc_levels_h_dev(
        _chk(LL, torch.float64, "LL"), _chk(h, torch.float64, "h"), LL.shape[0], tf.size, LL.shape[0] // tf.size, _abi.ptr(tf),
        int(chain0), int(seed) & _M64, int(step) & _M32, _chk(level, torch.float64, "level"), _stream()))


def mcmc_prior_term_device(U, Up, mean, sd, h_out, h_in=None):
    """trpl_mcmc_prior_term_dev: h_out (count,) f64 <- h_in + (lnp(Up) - lnp(U)) for the independent Gaussian prior (mean, sd), host
    arrays (A,), in the unit coordinates U and Up (count, A) f64; h_in None is zero, and may be h_out."""
    import torch
    if U.dim() != 2 or Up.shape != U.shape or tuple(h_out.shape) != (U.shape[0],) or (h_in is not None and h_in.shape != h_out.shape):
        raise ValueError("U and Up must be (count, A), h_out and h_in (count,)")
    count, A = U.shape
    mean, sd = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(sd, dtype=np.float64)
    if mean.shape != (A,) or sd.shape != (A,):
        raise ValueError("mean and sd must be (A,)")
    _abi.check(_abi.lib().trpl_mcmc_prior_term_dev(
        _chk(U, torch.float64, "U"), _chk(Up, torch.float64, "Up"), count, A, _abi.ptr(mean), _abi.ptr(sd),
        _opt(h_in, torch.float64, "h_in"), _chk(h_out, torch.float64, "h_out"), _stream()))


def mcmc_chain_stats_device(H, t0, t1, mean, m2, Q=None):
    """trpl_mcmc_chain_stats_dev: mean, m2 (Q,) f64 <- per column q < Q of the history H (n, ldh >= Q) f64, which stays where it is,
    the mean and the centred sum of squares over the steps [t0, t1), both sums in ascending t: the plain loop's bits.  Q defaults
    to ldh."""
    import torch
    if H.dim() != 2:
        raise ValueError("H must be (n, ldh)")
    Q = H.shape[1] if Q is None else int(Q)
    if tuple(mean.shape) != (Q,) or tuple(m2.shape) != (Q,):
        raise ValueError("mean and m2 must be (Q,)")
    _abi.check(_abi.lib().trpl_mcmc_chain_stats_dev(
        _chk(H, torch.float64, "H"), H.shape[0], H.shape[1], Q, int(t0), int(t1), _chk(mean, torch.float64, "mean"),
        _chk(m2, torch.float64, "m2"), _stream()))


def mcmc_autocov_device(H, t0, t1, mean, s, Q=None):
    """trpl_mcmc_autocov_dev: mean (Q,) and s (L, lds >= Q) f64 <- per column q < Q of the history H (n, ldh >= Q) f64, which stays
    where it is, the mean over the steps [t0, t1) and the sums s[l][q] of e[t] e[t + l], e = H - mean, over ascending t, for the
    L = s.shape[0] <= t1 - t0 lags 0 .. L - 1: the plain loop's bits, s[0] those of mcmc_chain_stats_device's m2.  Q defaults to ldh."""
    import torch
    if H.dim() != 2 or s.dim() != 2:
        raise ValueError("H must be (n, ldh) and s (L, lds)")
    Q = H.shape[1] if Q is None else int(Q)
    if tuple(mean.shape) != (Q,):
        raise ValueError("mean must be (Q,)")
    _abi.check(_abi.lib().trpl_mcmc_autocov_dev(
        _chk(H, torch.float64, "H"), H.shape[0], H.shape[1], Q, int(t0), int(t1), s.shape[0], _chk(mean, torch.float64, "mean"),
        _chk(s, torch.float64, "s"), s.shape[1], _stream()))


def mcmc_autocov_pool_device(s, M, A, pooled):
    """trpl_mcmc_autocov_pool_dev: pooled (L, A) f64 <- the sums over the M sequences of s (L, lds >= M A) f64, whose columns are M
    groups of A: pooled[l][a] = sum over c of s[l][c A + a], c ascending."""
    import torch
    if s.dim() != 2 or tuple(pooled.shape) != (s.shape[0], int(A)):
        raise ValueError("s must be (L, lds) and pooled (L, A)")
    _abi.check(_abi.lib().trpl_mcmc_autocov_pool_dev(
        _chk(s, torch.float64, "s"), s.shape[0], s.shape[1], int(M), int(A), _chk(pooled, torch.float64, "pooled"), _stream()))


def mcmc_evidence_sums_device(LL, tf, t0, t1, ext, sums):
    """trpl_mcmc_evidence_sums_dev: ext (K, 2) and sums (K, B, 6) f64 <- the kept LL (K, n, C) f64 of the K rungs of the host ladder tf
    (K,), which stays where it is, over the steps [t0, t1) in B = sums.shape[1] blocks of (t1 - t0) / B steps: the extrema of each
    rung and per block [sum LL, up, up2, down, down2, count above -inf], the stepping-stone sums of mcmc.log_evidence_ratios in one
    fixed association (include/trpl.h has the rule)."""
    import torch
    tf = _ladder(tf)
    if LL.dim() != 3 or LL.shape[0] != tf.size:
        raise ValueError("LL must be (K, n, C) with the ladder's K = %d" % tf.size)
    K = tf.size
    if tuple(ext.shape) != (K, 2) or sums.dim() != 3 or sums.shape[0] != K or sums.shape[2] != _abi.MCMC_EVIDENCE_SUMS:
        raise ValueError("ext must be (K, 2) and sums (K, B, %d)" % _abi.MCMC_EVIDENCE_SUMS)
    _abi.check(_abi.lib().trpl_mcmc_evidence_sums_dev(
        _chk(LL, torch.float64, "LL"), K, LL.shape[1], LL.shape[2], int(t0), int(t1), sums.shape[1], _abi.ptr(tf),
        _chk(ext, torch.float64, "ext"), _chk(sums, torch.float64, "sums"), _stream()))


def credible_interval_device(x, W, lo=0.025, hi=0.975):
    """utils.py:185-196 on the device: sort by x, cumulate the weights, last point below `lo` and first
    above `hi` (torch.sort / cumsum: library plumbing, no custom kernel)."""
    import torch
    xs, order = torch.sort(x)
    cs = torch.cumsum(W[order], 0)
    below = torch.nonzero(cs < lo)
    above = torch.nonzero(cs > hi)
    return float(xs[below[-1, 0]]), float(xs[above[0, 0]])


def sample_box_device(X, minX, maxX, do_log, seed=42, flags=0):
    """Fill X (S, ncol) f64 in HBM with bayeslib.random_grid's draws (trpl_sample_box_dev)."""
    import torch
    lo = np.ascontiguousarray(minX, dtype=np.float64)
    hi = np.ascontiguousarray(maxX, dtype=np.float64)
    lg = np.ascontiguousarray(do_log, dtype=np.int32)
    if X.dim() != 2 or X.shape[1] != lo.size or not (lo.shape == hi.shape == lg.shape):
        raise ValueError("X must be (S, ncol) with ncol = len(minX) = len(maxX) = len(do_log)")
    _abi.check(_abi.lib().trpl_sample_box_dev(int(seed) & 0xFFFFFFFF, X.shape[0], lo.size, _abi.ptr(lo), _abi.ptr(hi),
                                              _abi.ptr(lg), int(flags), _chk(X, torch.float64, "X"), _stream()))


def _loglik_from_pl_dev(entry, pl, obs, mag, P, sse, obs_hi, obs_dx, obs_h, ncol, flags, status, wts=None, esum=None):
    """The one marshaller of trpl_loglik[_moments|_weighted]_from_pl_dev: wts after obs (the weighted entry), esum after sse
    (not in trpl_loglik_from_pl_dev)."""
    import torch
    f64 = torch.float64
    if pl.dim() != 2 or pl.dtype not in (torch.float32, torch.float64):
        raise ValueError("pl must be a 2-D float32/float64 tensor")
    if wts is not None and wts.shape != obs.shape:
        raise ValueError("shape mismatch")
    rows, ld = pl.shape
    args = [_chk(pl, pl.dtype, "pl"), pl.element_size(), rows, int(ld if ncol is None else ncol), ld, _chk(obs, f64, "obs")]
    if entry == "trpl_loglik_weighted_from_pl_dev":
        args.append(_chk(wts, f64, "wts"))
    args += _brackets(obs, obs_hi, obs_dx, obs_h)
    args += [obs.shape[0], _chk(mag, f64, "mag"), _opt(status, torch.int32, "status"), _opt(P, f64, "P"), _opt(sse, f64, "sse")]
    if entry != "trpl_loglik_from_pl_dev":
        args.append(_opt(esum, f64, "esum"))
    _abi.check(getattr(_abi.lib(), entry)(*args, int(flags), _stream()))


def loglik_from_pl_device(pl, obs, mag, P=None, sse=None, obs_hi=None, obs_dx=None, obs_h=None, ncol=None, flags=0,
                          status=None):
    """trpl_loglik_from_pl_dev: likelihood of PL rows resident in HBM (pl (rows, ld) f32/f64, as written by
    solve_pl_device) against one observation set obs (n_obs,) f64 -- on the grid, or off-grid with the
    bracketing arrays obs_hi (int32), obs_dx, obs_h of driver.bracket_times.  mag (rows,) f64 log offsets;
    P (rows,) is decremented in place and/or sse (rows,) receives the squared-error sums; status (rows,)
    int32 from solve_pl_device makes flagged systems score +inf."""
    _loglik_from_pl_dev("trpl_loglik_from_pl_dev", pl, obs, mag, P, sse, obs_hi, obs_dx, obs_h, ncol, flags, status)


def loglik_moments_from_pl_device(pl, obs, mag, P=None, sse=None, esum=None, obs_hi=None, obs_dx=None, obs_h=None,
                                  ncol=None, flags=0, status=None):
    """trpl_loglik_moments_from_pl_dev: loglik_from_pl_device that also fills esum (rows,) f64, the sum of the row's
    log-errors (NaN for a flagged row): the resident-PL source of mag_grid_device's moments."""
    _loglik_from_pl_dev("trpl_loglik_moments_from_pl_dev", pl, obs, mag, P, sse, obs_hi, obs_dx, obs_h, ncol, flags, status,
                        esum=esum)


def loglik_weighted_from_pl_device(pl, obs, wts, mag, P=None, sse=None, esum=None, obs_hi=None, obs_dx=None, obs_h=None,
                                   ncol=None, flags=0, status=None):
    """trpl_loglik_weighted_from_pl_dev: loglik_moments_from_pl_device with the weights wts (n_obs,) f64 of the
    observations: sse = sum w e^2, esum = sum w e per row."""
    _loglik_from_pl_dev("trpl_loglik_weighted_from_pl_dev", pl, obs, mag, P, sse, obs_hi, obs_dx, obs_h, ncol, flags, status,
                        wts=wts, esum=esum)


def sse_accumulate_w_device(P, pl, values, wts, mag):
    """trpl_sse_accumulate_w_dev: P (rows,) f64 -= sum_i ((pl[j,i] + mag[j] - values[i])^2 * wts[i]), fp64, index order;
    pl (rows, n_obs) f32/f64 with contiguous rows, values / wts (n_obs,), mag (rows,) f64."""
    import torch
    if pl.dim() != 2 or pl.dtype not in (torch.float32, torch.float64):
        raise ValueError("pl must be a 2-D float32/float64 tensor")
    rows, n = pl.shape
    if tuple(P.shape) != (rows,) or tuple(mag.shape) != (rows,) or tuple(values.shape) != (n,) or tuple(wts.shape) != (n,):
        raise ValueError("shape mismatch")
    _abi.check(_abi.lib().trpl_sse_accumulate_w_dev(
        _chk(P, torch.float64, "P"), _chk(pl, pl.dtype, "pl"), pl.element_size(), rows, n, n,
        _chk(values, torch.float64, "values"), _chk(wts, torch.float64, "wts"), _chk(mag, torch.float64, "mag"), _stream()))


def solve_pl_snap_device(matPar, Length, Time, L, T, dN, plI, snap_steps, plN=None, plP=None, plE=None, status=None,
                         iters_total=None, tol=7, MAX=10000, plT=1, flags=0):
    """trpl_solve_pl_snap_dev: solve_pl_device that also records the state at the time steps snap_steps
    (host sequence) into plN, plP (S, len(snap_steps), L) and plE (S, len(snap_steps), L+1), f64 tensors."""
    _solve_pl_dev("trpl_solve_pl_snap_dev", matPar, Length, Time, L, T, plI, status, iters_total, tol, MAX, plT, flags, dN=dN,
                  snap=(snap_steps, plN, plP, plE))


def solve_pl_resume_device(matPar, Length, Time, L, T, t0, resN, resP, resE, plI, snap_steps=(), plN=None, plP=None,
                           plE=None, status=None, iters_total=None, tol=7, MAX=10000, plT=1, flags=0):
    """trpl_solve_pl_resume_dev: continue at step t0 from the five raw time levels resN, resP (S, 5, L) and resE
    (S, 5, L+1), f64 tensors as recorded by solve_pl_snap_device(..., snap_steps=[t0-4 .. t0], flags=FLAG_SNAP_RAW)."""
    _solve_pl_dev("trpl_solve_pl_resume_dev", matPar, Length, Time, L, T, plI, status, iters_total, tol, MAX, plT, flags,
                  resume=(t0, resN, resP, resE), snap=(snap_steps, plN, plP, plE))


class MultiDevice:
    """One process, several GPUs, results resident on every GPU (trpl_multi_* / trpl_loglik_multi_dev, SURVEY
    8e): contiguous sample shards, one RCCL all-gather of the per-sample likelihoods over xGMI.  The handle
    owns one stream and one RCCL rank per device; create it once and reuse it."""

    def __init__(self, devices=None, allow_duplicate_devices=False):
        """allow_duplicate_devices (tests): several ranks on one GPU, against a stand-in collective library named by
        TRPL_RCCL_LIBRARY (trpl_multi_create_ex, TRPL_MULTI_ALLOW_DUPLICATE_DEVICES); real RCCL refuses them."""
        self._h = _abi.C.c_void_p()
        dev = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        _abi.check(_abi.lib().trpl_multi_create_ex(_abi.ptr(dev), 0 if dev is None else len(dev),
                                                   _abi.MULTI_ALLOW_DUPLICATE_DEVICES if allow_duplicate_devices else 0,
                                                   _abi.C.byref(self._h)))
        self.n = int(_abi.lib().trpl_multi_device_count(self._h))
        self.devices = list(range(self.n)) if dev is None else [int(d) for d in dev]

    def close(self):
        if self._h:
            _abi.lib().trpl_multi_destroy(self._h)
            self._h = _abi.C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        _abi.check(_abi.lib().trpl_multi_synchronize(self._h))

    def shard_bounds(self, S):
        from .dist import shard_bounds
        return [shard_bounds(S, self.n, r) for r in range(self.n)]

    def _table(self, tensors, dtype, name, optional=False):
        import torch
        if tensors is None:
            if optional:
                return None
            raise ValueError("%s: one tensor per device is required" % name)
        if len(tensors) != self.n:
            raise ValueError("%s: need %d per-device tensors" % (name, self.n))
        tab = (_abi.C.c_void_p * self.n)()
        for r, t in enumerate(tensors):
            if t is None or t.numel() == 0:
                tab[r] = None
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
                    and t.device.index == self.devices[r]):
                raise ValueError("%s[%d] must be a contiguous %s tensor on cuda:%d" % (name, r, dtype, self.devices[r]))
            tab[r] = t.data_ptr()
        return tab

    def loglik(self, X, init_params, lengths, Time, L, T, obs, n_obs, P_full, sse=None, status=None, iters_total=None,
               obs_hi=None, obs_dx=None, obs_h=None, tol=7, MAX=10000, plT=1, flags=0, floor_col=None, order=True):
        """Enqueue the sharded fused likelihood + the all-gather; returns at once (synchronize() waits).
        X: list of per-device shards (n_r, 13); init_params / obs (/ obs_hi, obs_dx, obs_h): lists of per-device
        replicas; P_full: list of per-device (S,) f64 outputs; sse / status / iters_total / floor_col: optional
        lists of per-device (C, n_r) outputs.  S is taken from P_full.
        The handle works on its own streams.  With order=True (default) they are ordered on the device against
        torch's current stream of every device, both ways (trpl_multi_wait_stream before, trpl_multi_release_stream
        after): inputs just produced on the torch stream are complete when the solve reads them, and work given to
        the torch stream afterwards sees the gathered P_full -- no host wait.  order=False leaves both to the
        caller (synchronize())."""
        import torch
        S = int(P_full[0].shape[0])
        Cn = int(init_params[0].shape[0])
        bounds = self.shard_bounds(S)
        for r, (lo, hi) in enumerate(bounds):
            if tuple(X[r].shape) != (hi - lo, 13) or tuple(P_full[r].shape) != (S,) \
                    or tuple(init_params[r].shape) != (Cn, L) or obs[r].shape[0] != Cn:
                raise ValueError("rank %d: shapes do not match the shard [%d, %d) of S=%d" % (r, lo, hi, S))
            for name, lst, dt in (("sse", sse, torch.float64), ("status", status, torch.int32),
                                  ("iters_total", iters_total, torch.int64)):
                if lst is not None and tuple(lst[r].shape) != (Cn, hi - lo):
                    raise ValueError("%s[%d] must be (C, %d)" % (name, r, hi - lo))
            if floor_col is not None and tuple(floor_col[r].shape) != (Cn, hi - lo):
                raise ValueError("floor_col[%d] must be (C, %d)" % (r, hi - lo))
        lengths = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths, dtype=np.float64), (Cn,)))
        n_obs = np.ascontiguousarray(np.broadcast_to(np.asarray(n_obs, dtype=np.int64), (Cn,)))
        streams = [torch.cuda.current_stream(torch.device("cuda", d)).cuda_stream for d in self.devices] if order else []
        for r, s in enumerate(streams):
            _abi.check(_abi.lib().trpl_multi_wait_stream(self._h, r, s))
        _abi.check(_abi.lib().trpl_loglik_multi_dev(
            self._h, self._table(X, torch.float64, "X"), S, Cn, _abi.ptr(lengths), float(Time), int(L), int(T), int(plT),
            int(tol), int(MAX), self._table(init_params, torch.float64, "init_params"),
            self._table(obs, torch.float64, "obs"), self._table(obs_hi, torch.int32, "obs_hi", True),
            self._table(obs_dx, torch.float64, "obs_dx", True), self._table(obs_h, torch.float64, "obs_h", True),
            int(obs[0].shape[1]), _abi.ptr(n_obs), self._table(P_full, torch.float64, "P_full"),
            self._table(sse, torch.float64, "sse", True), self._table(status, torch.int32, "status", True),
            self._table(iters_total, torch.int64, "iters_total", True),
            self._table(floor_col, torch.int32, "floor_col", True), int(flags)))
        for r, s in enumerate(streams):
            _abi.check(_abi.lib().trpl_multi_release_stream(self._h, r, s))
