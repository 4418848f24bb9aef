"""The instrument response in the model: PL(t) convolved with the response function (IRF) of the detection chain.

A measured TRPL decay is the model curve convolved with the IRF.  The reference compares the bare curve and cuts the data after
its peak; with the IRF in the model the rising edge and the first nanoseconds after it -- where surface recombination and the
mobilities show most -- can be fitted.  The convolution is one kernel on a PL block resident in HBM (trpl_convolve_irf*,
include/trpl.h; csrc/irf.hip): every consumer of such a block takes the convolved block unchanged.  There is no CPU fallback.

    gaussian(fwhm_ns, dt_ns)                a normalised Gaussian response on the simulation grid -> (h, k0)
    from_samples(t_ns, counts, dt_ns)       a measured response resampled onto the simulation grid -> (h, k0)
    convolve(pl, h, k0)                     one PL matrix on the host -> the (rows, ncol - k0) convolved matrix
    loglik(X, ..., obs, irf)                the resident route solve -> convolve -> likelihood; X -> LL for refine / mcmc

An IRF is the pair (h, k0): the taps at the grid's spacing and the index of the tap that sits at time zero (the peak).  The
convolved curve has k0 columns less than the solved one: its last k0 columns would need PL past the solved window.
"""
import math

import numpy as np

from . import _abi


def max_taps():
    """trpl_irf_max_taps(): the most taps one call convolves with."""
    return int(_abi.lib().trpl_irf_max_taps())


def _check_irf(irf):
    """(h float64 contiguous, k0 int) of an IRF pair, refused as the library refuses it."""
    try:
        h, k0 = irf
    except (TypeError, ValueError):
        raise ValueError("irf must be the pair (h, k0)")
    h = np.ascontiguousarray(h, dtype=np.float64)
    k0 = int(k0)
    if h.ndim != 1 or not 1 <= h.size <= _abi.IRF_MAX_TAPS:
        raise ValueError("irf: h must hold 1 .. %d taps" % _abi.IRF_MAX_TAPS)
    if not 0 <= k0 < h.size:
        raise ValueError("irf: k0 = %d must be in [0, K - 1 = %d]" % (k0, h.size - 1))
    if not np.all(np.isfinite(h)):
        raise ValueError("irf: every tap must be finite")
    return h, k0


def gaussian(fwhm_ns, dt_ns, rel_cut=1e-12):
    """A Gaussian response of full width at half maximum fwhm_ns on a grid of spacing dt_ns: taps
    exp(-4 ln2 ((k - k0) dt / fwhm)^2), symmetric about k0, truncated where the value falls below rel_cut of the peak -- m =
    floor(fwhm / dt * sqrt(ln(1 / rel_cut) / (4 ln 2))) taps on either side -- and divided by their math.fsum.  Returns (h, k0)
    with K = 2 m + 1 taps and k0 = m.  ValueError if that is more than max_taps() taps."""
    fwhm_ns, dt_ns, rel_cut = float(fwhm_ns), float(dt_ns), float(rel_cut)
    if not (fwhm_ns > 0.0 and math.isfinite(fwhm_ns) and dt_ns > 0.0 and math.isfinite(dt_ns)):
        raise ValueError("fwhm_ns and dt_ns must be finite and > 0")
    if not 0.0 < rel_cut < 1.0:
        raise ValueError("rel_cut must lie in (0, 1)")

    def value(n):
        return math.exp(-4.0 * math.log(2.0) * (n * dt_ns / fwhm_ns) ** 2)

    width = fwhm_ns / dt_ns * math.sqrt(math.log(1.0 / rel_cut) / (4.0 * math.log(2.0)))
    cap = max_taps()
    if 2.0 * width + 1.0 > cap + 2.0:
        raise ValueError("a Gaussian of fwhm %g ns on a %g ns grid needs about %d taps above %g of its peak, more than "
                         "trpl_irf_max_taps() = %d" % (fwhm_ns, dt_ns, 2 * int(width) + 1, rel_cut, cap))
    m = int(width)
    while value(m + 1) >= rel_cut:            # the formula, made exact at the rounding of its last tap
        m += 1
    while m > 0 and value(m) < rel_cut:
        m -= 1
    if 2 * m + 1 > cap:
        raise ValueError("a Gaussian of fwhm %g ns on a %g ns grid needs %d taps above %g of its peak, more than "
                         "trpl_irf_max_taps() = %d" % (fwhm_ns, dt_ns, 2 * m + 1, rel_cut, cap))
    half = [value(n) for n in range(1, m + 1)]
    taps = half[::-1] + [1.0] + half
    total = math.fsum(taps)
    return np.array([v / total for v in taps], dtype=np.float64), m


def from_samples(t_ns, counts, dt_ns, background=0.0):
    """A measured response: counts at the increasing times t_ns.  The background is subtracted and the result clipped at 0, then
    resampled linearly onto the grid of spacing dt_ns laid so that the largest sample sits on a node (the nodes inside
    [t_ns[0], t_ns[-1]]); leading and trailing zeros are dropped and the taps divided by their math.fsum.  Returns (h, k0), k0
    the index of the maximum.  ValueError for a response without a positive sample or with more than max_taps() taps."""
    t = np.asarray(t_ns, dtype=np.float64)
    c = np.asarray(counts, dtype=np.float64)
    dt_ns = float(dt_ns)
    if t.ndim != 1 or t.shape != c.shape or t.size < 1:
        raise ValueError("t_ns and counts must be one-dimensional and of one length")
    if not (np.all(np.isfinite(t)) and np.all(np.isfinite(c)) and np.all(np.diff(t) > 0)):
        raise ValueError("t_ns must be finite and increasing, counts finite")
    if not (dt_ns > 0.0 and math.isfinite(dt_ns)):
        raise ValueError("dt_ns must be finite and > 0")
    c = np.clip(c - float(background), 0.0, None)
    peak = int(np.argmax(c))
    if not c[peak] > 0.0:
        raise ValueError("the response has no sample above the background")
    before, after = int(math.floor((t[peak] - t[0]) / dt_ns)), int(math.floor((t[-1] - t[peak]) / dt_ns))
    if before + after + 1 > 4 * _abi.IRF_MAX_TAPS:
        raise ValueError("the samples span %d nodes of a %g ns grid: far more than trpl_irf_max_taps() = %d"
                         % (before + after + 1, dt_ns, _abi.IRF_MAX_TAPS))
    nodes = t[peak] + dt_ns * np.arange(-before, after + 1)
    v = np.interp(nodes, t, c)
    v[before] = c[peak]                               # the node of the maximum holds it exactly
    keep = np.flatnonzero(v > 0.0)
    first, last = int(keep[0]), int(keep[-1])
    v = v[first:last + 1]
    if v.size > max_taps():
        raise ValueError("the response has %d taps on a %g ns grid, more than trpl_irf_max_taps() = %d" % (v.size, dt_ns, max_taps()))
    total = math.fsum(v)
    return np.array([x / total for x in v], dtype=np.float64), before - first


def convolve(pl, h, k0, device=0, info=None):
    """trpl_convolve_irf on host arrays: pl (rows, ncol) float32 / float64 PL as solve_pl returns it, (h, k0) the IRF.  Returns the
    (rows, ncol - k0) matrix out[r, j] = sum_k h[k] pl[r, j + k0 - k] in pl's dtype: fp64 sums in ascending k, the terms left
    of column 0 skipped (include/trpl.h has the definition).  info receives seconds, the kernel's time on the device."""
    pl = np.asarray(pl)
    if pl.ndim != 2 or pl.dtype not in (np.float32, np.float64):
        raise ValueError("pl must be a 2-D float32/float64 array")
    pl = np.ascontiguousarray(pl)
    h = np.ascontiguousarray(h, dtype=np.float64)
    if h.ndim != 1:
        raise ValueError("h must be one-dimensional")
    rows, ncol = pl.shape
    k0 = int(k0)
    out = np.empty((rows, max(ncol - k0, 0)), dtype=pl.dtype)
    sec = _abi.C.c_double(0.0)
    _abi.check(_abi.lib().trpl_convolve_irf(_abi.ptr(pl), pl.itemsize, rows, ncol, ncol, _abi.ptr(h), h.size, k0, _abi.ptr(out),
                                            out.shape[1], int(device), _abi.C.byref(sec)))
    if info is not None:
        info.update(seconds=sec.value)
    return out


def last_time(Time, T, k0):
    """The time of the last convolved column: Time * (T - k0) / T."""
    return float(Time) * (int(T) - int(k0)) / int(T)


def loglik(X, init_params, lengths, Time, L, T, obs, irf, times=None, weights=None, tol=7, MAX=10000, pl_f32=False,
           predict=False, block=8192, device=0, P=None, info=None, normalize=False):
    """The likelihood of one experiment with the instrument response in the model, on the resident route: per block of `block`
    samples and per curve, solve_pl_device writes the PL block into HBM, convolve_irf_device maps it to the block the detector
    saw, and loglik_from_pl_device (with weights=: loglik_weighted_from_pl_device) scores that block -- only X goes in and P
    comes out.

    X, init_params, lengths, Time, L, T, obs, times, weights, tol, MAX, predict, device, P as driver.loglik takes them; irf =
    (h, k0), the taps at the spacing Time / T of the simulation grid and the index of the tap at time zero (gaussian,
    from_samples).  The convolved curve has ncol_out = T + 1 - k0 columns, at the first ncol_out times of the grid.  With
    times=None observation i of a curve sits on column i, so len(obs[c]) <= ncol_out; otherwise the times are bracketed exactly
    as driver.loglik brackets them, on the convolved columns: an observation later than Time * (T - k0) / T is a ValueError.
    pl_f32: the PL block (solved and convolved) is float32, as the reference's buffer is.  Accumulates into P (S,) if given,
    else starts from zeros; returns P.  info receives sse (C, S), status (C, S) and ncol_out.
    normalize: self-normalisation is a ValueError -- normalising a convolved curve to its own first column is not what the
    reference's flag means (its first column is a fraction of the response's area, not PL(0)).
    A sample's bits are those of its block's launches: cut the samples with `block` as the run that is compared with cuts them.

    functools.partial(loglik, init_params=..., ..., irf=...) is a valid `loglik` for refine.run, mcmc.run and
    mcmc.run_tempered WITHOUT early_reject: the early stop lives in the fused steppers (trpl_loglik_cut*), which compare the
    bare curve and never see a convolved one."""
    if normalize:
        raise ValueError("normalize: self-normalisation does not combine with an IRF (the convolved curve's first column is not PL(0))")
    h, k0 = _check_irf(irf)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != 13:
        raise ValueError("X must have shape (S, 13)")
    S = X.shape[0]
    L, T, block = int(L), int(T), int(block)
    ini = np.ascontiguousarray(init_params, dtype=np.float64)
    if ini.ndim != 2 or ini.shape[1] != L:
        raise ValueError("init_params must have shape (C, L=%d), got %r" % (L, ini.shape))
    Cn = ini.shape[0]
    lengths = np.full(Cn, float(lengths)) if np.isscalar(lengths) else np.ascontiguousarray(lengths, dtype=float)
    if lengths.shape != (Cn,) or len(obs) != Cn or (times is not None and len(times) != Cn):
        raise ValueError("need one length and one observation set per curve")
    if weights is not None and len(weights) != Cn:
        raise ValueError("weights: need one array of weights per curve")
    if block < 1:
        raise ValueError("block must be >= 1")
    ncol_out = T + 1 - k0
    if ncol_out < 1:
        raise ValueError("irf: k0 = %d leaves no column of a window of T = %d steps" % (k0, T))
    from .driver import bracket_times
    sim_t = np.linspace(0, Time, T + 1)[:ncol_out]                         # bayeslib.py:115; the convolved columns
    staged = []
    for c, o in enumerate(obs):
        o = np.asarray(o, dtype=float)
        w = None if weights is None else np.asarray(weights[c], dtype=float)
        if w is not None and w.shape != o.shape:
            raise ValueError("curve %d: %d weights for %d observations" % (c, len(w), len(o)))
        kw = {}
        if times is None:
            if len(o) > ncol_out:
                raise ValueError("curve %d: %d observations on the grid, but the convolved curve has T + 1 - k0 = %d columns"
                                 % (c, len(o), ncol_out))
        else:
            tc = np.asarray(times[c], dtype=float)
            if tc.shape != o.shape:
                raise ValueError("curve %d: %d times for %d observations" % (c, len(tc), len(o)))
            if len(tc) and (tc.min() < sim_t[0] or tc.max() > sim_t[-1]):
                raise ValueError("curve %d: observation times outside [0, Time * (T - k0) / T = %g], the convolved window"
                                 % (c, last_time(Time, T, k0)))
            if ncol_out < 2:
                raise ValueError("off-grid observation times need two convolved columns")
            order = np.argsort(tc, kind="stable")
            tc, o = tc[order], o[order]
            w = None if w is None else w[order]
            kw.update(zip(("obs_hi", "obs_dx", "obs_h"), bracket_times(sim_t, tc)))
        kw["obs"] = o
        if w is not None:
            kw["wts"] = w
        staged.append(kw)
    if P is None:
        P = np.zeros(S)
    if not (P.dtype == np.float64 and P.flags.c_contiguous and P.shape == (S,)):
        raise ValueError("P must be a contiguous float64 array of shape (S,)")
    sse = np.zeros((Cn, S))
    status = np.zeros((Cn, S), dtype=np.int32)
    if info is not None:
        info.update(sse=sse, status=status, ncol_out=ncol_out)
    if S == 0:
        return P

    import torch

    from . import device as tdev
    dev = torch.device("cuda", device)
    tdt = torch.float32 if pl_f32 else torch.float64
    score = tdev.loglik_from_pl_device if weights is None else tdev.loglik_weighted_from_pl_device
    with torch.cuda.device(dev):
        def to_dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ini_d, h_d = to_dev(ini), to_dev(h)
        staged = [{k: to_dev(v) for k, v in kw.items()} for kw in staged]
        size = min(block, S)
        pl_d = torch.empty((size, T + 1), dtype=tdt, device=dev)
        cv_d = torch.empty((size, ncol_out), dtype=tdt, device=dev)
        for blk in range(0, S, block):
            n = min(block, S - blk)
            X_d = to_dev(X[blk:blk + n])
            mat_d, mag_d = X_d[:, :12].contiguous(), X_d[:, 12].contiguous()
            P_d = to_dev(P[blk:blk + n])
            sse_d = torch.zeros((Cn, n), dtype=torch.float64, device=dev)
            st_d = torch.zeros((Cn, n), dtype=torch.int32, device=dev)
            for c in range(Cn):
                tdev.solve_pl_device(mat_d, lengths[c], Time, L, T, ini_d[c].contiguous(), pl_d[:n], status=st_d[c], tol=tol,
                                     MAX=MAX, flags=_abi.FLAG_PREDICT if predict else 0)
                tdev.convolve_irf_device(pl_d[:n], h_d, k0, cv_d[:n])
                score(cv_d[:n], mag=mag_d, P=P_d, sse=sse_d[c], status=st_d[c], **staged[c])
            P[blk:blk + n] = P_d.cpu().numpy()
            sse[:, blk:blk + n] = sse_d.cpu().numpy()
            status[:, blk:blk + n] = st_d.cpu().numpy()
    return P
