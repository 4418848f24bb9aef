"""The instrument response in the model: PL(t) convolved with the response function (IRF) of the detection chain.

A measured TRPL decay is the model curve convolved with the IRF.  The reference compares the bare curve and cuts the data after
its peak; with the IRF in the model the rising edge and the first nanoseconds after it -- where surface recombination and the
mobilities show most -- can be fitted.  The convolution is one kernel on a PL block resident in HBM (trpl_convolve_irf*,
include/trpl.h; csrc/irf.hip): every consumer of such a block takes the convolved block unchanged.  There is no CPU fallback.

    gaussian(fwhm_ns, dt_ns)                a normalised Gaussian response on the simulation grid -> (h, k0)
    from_samples(t_ns, counts, dt_ns)       a measured response resampled onto the simulation grid -> (h, k0)
    convolve(pl, h, k0)                     one PL matrix on the host -> the (rows, ncol - k0) convolved matrix
    loglik(X, ..., obs, irf)                the resident route solve -> convolve -> likelihood; X -> LL for refine / mcmc
    gaussian_bank(fwhms_ns, shifts_ns, dt_ns)   a bank of Gaussian responses, widths x time shifts -> (H, k0, table)
    shift_bank((h, k0), shifts_ns, dt_ns)   a measured response at several time shifts -> (H, k0, table)
    loglik_bank(X, ..., obs, bank)          solve -> the likelihood per response of the bank, from one solve -> P (J, S)
    loglik_profile(X, ..., obs, bank)       the profile of loglik_bank over the bank; X -> LL for refine / mcmc
    loglik_nuisance(X, ..., obs, bank, mag=, reduce=)   the maximum or the marginal over responses x magnitude offsets, reduced
                                            on the device; X -> LL for refine / mcmc

An IRF is the pair (h, k0): the taps at the grid's spacing and the index of the tap that sits at time zero (the peak).  The
convolved curve has k0 columns less than the solved one: its last k0 columns would need PL past the solved window.
A bank is J responses of one length and one k0, H (J, K): a time shift lives in the taps of a row, zero-padded to the common
length (trpl_loglik_irf_bank*, include/trpl.h; csrc/irf_bank.hip).
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


_NO_NORMALIZE = "normalize: self-normalisation does not combine with an IRF (the convolved curve's first column is not PL(0))"


def _stage(X, init_params, lengths, Time, L, T, obs, k0, times, weights, block):
    """What loglik and loglik_bank check and stage before a device is touched: X, the curves' constants, and per curve the
    keyword arrays of the scoring call -- obs, with times the three brackets on the convolved columns (sorted by time), with
    weights wts.  Returns (X, ini, lengths, staged, ncol_out)."""
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
    return X, ini, lengths, staged, ncol_out


def _check_reduction(mag, reduce, tf, where=""):
    """The reduction over responses x magnitude offsets as loglik_nuisance and gpu_info['irf_bank'] (where names it) take it ->
    (marginal, off, M, tf): off the host array of grid offsets or None, M the offsets per response."""
    from . import device as tdev
    if reduce not in ("max", "marginal"):
        raise ValueError(where + 'reduce must be "max" or "marginal", got %r' % (reduce,))
    marginal = reduce == "marginal"
    _, off = tdev.nuisance_flags(mag, marginal)
    M = 1 if off is None else len(off)
    count_ok, finite = 1 <= M <= _abi.NUISANCE_MAX_OFFSETS, off is None or bool(np.all(np.isfinite(off)))
    if where and not (count_ok and finite):
        raise ValueError(where + "mag as a grid holds 1 .. %d finite offsets" % _abi.NUISANCE_MAX_OFFSETS)
    if not count_ok:
        raise ValueError("mag: a grid holds 1 .. %d offsets, got %d" % (_abi.NUISANCE_MAX_OFFSETS, M))
    if not finite:
        raise ValueError("mag: every offset must be finite")
    tf = float(tf)
    if marginal and not (tf > 0.0 and math.isfinite(tf)):
        raise ValueError(where + "tf must be finite and > 0")
    return marginal, off, M, tf


class _Resident:
    """What the resident routes -- loglik, loglik_bank, loglik_nuisance -- have in common: the refusals and the staging before a
    device is touched, in one order, and the loop over blocks of samples and curves around the one solve.  irf = (h, k0) or bank
    = (H, k0[, table]); reduction = (mag, reduce, tf) is checked between the normalize refusal and the bank (_check_reduction ->
    marginal, off, M, tf).  A route adds its host results, then per block its device buffers, per curve its scoring calls and at
    the end of a block its downloads."""

    def __init__(self, X, init_params, lengths, Time, L, T, obs, times, weights, block, normalize, irf=None, bank=None, reduction=None):
        if normalize:
            raise ValueError(_NO_NORMALIZE)
        if reduction is not None:
            self.marginal, self.off, self.M, self.tf = _check_reduction(*reduction)
        self.taps, self.k0 = _check_irf(irf) if bank is None else _check_bank(bank)
        self.X, self.ini, self.lengths, self.staged, self.ncol_out = _stage(X, init_params, lengths, Time, L, T, obs, self.k0, times,
                                                                            weights, block)
        if bank is not None:
            for c, kw in enumerate(self.staged):
                if len(kw["obs"]) < 1:
                    raise ValueError("curve %d: a bank needs at least one observation per curve" % c)
        self.S, self.Cn, self.Time, self.L, self.T, self.block = self.X.shape[0], self.ini.shape[0], Time, int(L), int(T), int(block)
        self.status = np.zeros((self.Cn, self.S), dtype=np.int32)

    def blocks(self, tol, MAX, pl_f32, predict, device):
        """The blocks of `block` samples, one after the other, each as a namespace b: n samples, sl their slice of the host arrays,
        first (the route's buffers that outlive a block are made then: size rows serve every block), mag (n,), pl (n, T + 1) the PL
        block, taps and kw the uploaded responses and per-curve keywords, torch, tdev, dev, to_dev(host array), zeros(*shape) f64.
        b.curves() yields c = 0 .. C - 1 with curve c solved into b.pl and its flags in b.status[c].  After the route's part of a
        block status comes down.  Without a sample nothing is yielded and no device is touched."""
        if self.S == 0:
            return
        import types

        import torch

        from . import device as tdev
        dev = torch.device("cuda", device)
        Cn, T = self.Cn, self.T
        with torch.cuda.device(dev):
            def to_dev(a):
                return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

            def zeros(*shape):
                return torch.zeros(shape, dtype=torch.float64, device=dev)
            ini_d, taps_d = to_dev(self.ini), to_dev(self.taps)
            staged = [{k: to_dev(v) for k, v in kw.items()} for kw in self.staged]
            size = min(self.block, self.S)
            pl_d = torch.empty((size, T + 1), dtype=torch.float32 if pl_f32 else torch.float64, device=dev)
            for blk in range(0, self.S, self.block):
                n = min(self.block, self.S - blk)
                X_d = to_dev(self.X[blk:blk + n])
                mat_d = X_d[:, :12].contiguous()
                b = types.SimpleNamespace(n=n, sl=slice(blk, blk + n), first=blk == 0, size=size, mag=X_d[:, 12].contiguous(), pl=pl_d[:n],
                                          taps=taps_d, kw=staged, torch=torch, tdev=tdev, dev=dev, to_dev=to_dev, zeros=zeros)

                def curves():
                    b.status = torch.zeros((Cn, n), dtype=torch.int32, device=dev)
                    for c in range(Cn):
                        tdev.solve_pl_device(mat_d, self.lengths[c], self.Time, self.L, T, ini_d[c].contiguous(), b.pl, status=b.status[c],
                                             tol=tol, MAX=MAX, flags=_abi.FLAG_PREDICT if predict else 0)
                        yield c
                b.curves = curves
                yield b
                self.status[:, b.sl] = b.status.cpu().numpy()

    def bank_moments(self, b, c, sse_d, es_d):
        """curve c of block b against the J responses: its moments into sse_d[c], es_d[c] (J, n)"""
        b.tdev.loglik_irf_bank_device(b.pl, b.taps, self.k0, mag=b.mag, sse=sse_d[c], esum=es_d[c], status=b.status[c], **b.kw[c])


def _moments_down(host, dev_t, sl):
    """the moments of a block, (C, J, n) on the device, into the columns sl of the host's (J, C, S)"""
    host[:, :, sl] = dev_t.cpu().numpy().transpose(1, 0, 2)


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
    r = _Resident(X, init_params, lengths, Time, L, T, obs, times, weights, block, normalize, irf=irf)
    if P is None:
        P = np.zeros(r.S)
    if not (P.dtype == np.float64 and P.flags.c_contiguous and P.shape == (r.S,)):
        raise ValueError("P must be a contiguous float64 array of shape (S,)")
    sse = np.zeros((r.Cn, r.S))
    if info is not None:
        info.update(sse=sse, status=r.status, ncol_out=r.ncol_out)
    for b in r.blocks(tol, MAX, pl_f32, predict, device):
        if b.first:
            cv_d = b.pl.new_empty((b.size, r.ncol_out))
            score = b.tdev.loglik_from_pl_device if weights is None else b.tdev.loglik_weighted_from_pl_device
        P_d, sse_d = b.to_dev(P[b.sl]), b.zeros(r.Cn, b.n)
        for c in b.curves():
            b.tdev.convolve_irf_device(b.pl, b.taps, r.k0, cv_d[:b.n])
            score(cv_d[:b.n], mag=b.mag, P=P_d, sse=sse_d[c], status=b.status[c], **b.kw[c])
        P[b.sl] = P_d.cpu().numpy()
        sse[:, b.sl] = sse_d.cpu().numpy()
    return P


# ------------------------------------------------------------------------------------------------ a bank of responses
def bank_cap():
    """trpl_irf_bank_max_responses(): the most responses one bank holds."""
    return int(_abi.lib().trpl_irf_bank_max_responses())


def _check_bank(bank):
    """(H float64 (J, K) contiguous, k0 int) of a bank (H, k0) or (H, k0, table), refused as the library refuses it."""
    try:
        H, k0 = bank[0], bank[1]
    except (TypeError, IndexError, KeyError):
        raise ValueError("bank must be (H, k0) or (H, k0, table)")
    H = np.ascontiguousarray(H, dtype=np.float64)
    k0 = int(k0)
    if H.ndim != 2 or not 1 <= H.shape[0] <= _abi.IRF_BANK_MAX_RESPONSES or not 1 <= H.shape[1] <= _abi.IRF_MAX_TAPS:
        raise ValueError("bank: H must be (J, K) with 1 .. %d responses of 1 .. %d taps" % (_abi.IRF_BANK_MAX_RESPONSES, _abi.IRF_MAX_TAPS))
    if not 0 <= k0 < H.shape[1]:
        raise ValueError("bank: k0 = %d must be in [0, K - 1 = %d]" % (k0, H.shape[1] - 1))
    if not np.all(np.isfinite(H)):
        raise ValueError("bank: every tap must be finite")
    return H, k0


def _check_counts(J, K):
    if J > bank_cap():
        raise ValueError("a bank of %d responses is more than trpl_irf_bank_max_responses() = %d" % (J, bank_cap()))
    if K > max_taps():
        raise ValueError("the bank needs %d taps, more than trpl_irf_max_taps() = %d" % (K, max_taps()))


def gaussian_bank(fwhms_ns, shifts_ns, dt_ns, rel_cut=1e-12):
    """A bank of Gaussian responses on a grid of spacing dt_ns: every width of fwhms_ns at every time shift of shifts_ns,
    width-major -- J = len(fwhms_ns) * len(shifts_ns), row j = w * len(shifts_ns) + s, table[j] = (fwhm, shift).  The taps of a row
    are exp(-4 ln2 (((k - k0) - shift / dt) dt / fwhm)^2), 0.0 where that is below rel_cut, divided by the row's own math.fsum.
    K = 2 k0 + 1 and k0 are common to the rows: the fewest taps that hold the widest response at the largest |shift|.  A positive
    shift moves the convolved curve later.  With shift 0 a row is gaussian(fwhm, dt_ns, rel_cut) zero-padded, bit for bit.
    Returns (H (J, K), k0, table (J, 2)).  ValueError above max_taps() taps or bank_cap() responses."""
    fw = np.atleast_1d(np.asarray(fwhms_ns, dtype=np.float64))
    sh = np.atleast_1d(np.asarray(shifts_ns, dtype=np.float64))
    dt_ns, rel_cut = float(dt_ns), float(rel_cut)
    if fw.ndim != 1 or sh.ndim != 1 or fw.size < 1 or sh.size < 1:
        raise ValueError("fwhms_ns and shifts_ns must be one-dimensional and not empty")
    if not (np.all(np.isfinite(fw)) and np.all(fw > 0.0) and np.all(np.isfinite(sh)) and dt_ns > 0.0 and math.isfinite(dt_ns)):
        raise ValueError("fwhms_ns and dt_ns must be finite and > 0, shifts_ns finite")
    if not 0.0 < rel_cut < 1.0:
        raise ValueError("rel_cut must lie in (0, 1)")
    J = fw.size * sh.size
    reach = float(fw.max()) / dt_ns * math.sqrt(math.log(1.0 / rel_cut) / (4.0 * math.log(2.0))) + float(np.abs(sh).max()) / dt_ns
    _check_counts(J, 2 * int(reach) - 1)                       # before anything of that size is built; exactly, below
    m0 = int(reach) + 2
    c = 4.0 * math.log(2.0)
    rows, table = [], []
    for f in fw.tolist():
        for t in sh.tolist():
            sig = t / dt_ns
            v = [math.exp(-c * ((n - sig) * dt_ns / f) ** 2) for n in range(-m0, m0 + 1)]
            rows.append([x if x >= rel_cut else 0.0 for x in v])
            table.append((f, t))
    m = max((abs(n - m0) for r in rows for n, x in enumerate(r) if x != 0.0), default=0)
    _check_counts(J, 2 * m + 1)
    H = np.empty((J, 2 * m + 1), dtype=np.float64)
    for j, r in enumerate(rows):
        r = r[m0 - m:m0 + m + 1]
        total = math.fsum(r)
        if not total > 0.0:
            raise ValueError("fwhm %g ns at shift %g ns on a %g ns grid leaves no tap above rel_cut" % (table[j] + (dt_ns,)))
        H[j] = [x / total for x in r]
    return H, m, np.array(table, dtype=np.float64)


def shift_bank(irf, shifts_ns, dt_ns):
    """A measured response (h, k0) (from_samples) at the time shifts shifts_ns, on the grid of spacing dt_ns: row j holds the taps
    moved by shifts_ns[j] / dt_ns steps -- the response resampled linearly between its taps, zero outside them: with shift / dt =
    i + f, 0 <= f < 1, tap n of the row is (1 - f) h[n - i] + f h[n - i - 1].  A shift of a whole number of steps moves the taps
    exactly; the rows are not normalised again (the resampling keeps the sum up to rounding).  K and k0 are common to the rows:
    the taps of (h, k0) padded with zeros on either side as far as the shifts reach.  A positive shift moves the convolved curve
    later.  Returns (H (J, K), k0, table (J,) = the shifts).  ValueError above max_taps() taps or bank_cap() responses."""
    h, k0 = _check_irf(irf)
    sh = np.atleast_1d(np.asarray(shifts_ns, dtype=np.float64))
    dt_ns = float(dt_ns)
    if sh.ndim != 1 or sh.size < 1 or not np.all(np.isfinite(sh)) or not (dt_ns > 0.0 and math.isfinite(dt_ns)):
        raise ValueError("shifts_ns must be one-dimensional, not empty and finite, dt_ns finite and > 0")
    sig = sh / dt_ns
    if float(np.abs(sig).max()) > 4 * _abi.IRF_MAX_TAPS:
        raise ValueError("a shift of %g steps is far more than trpl_irf_max_taps() = %d" % (float(np.abs(sig).max()), _abi.IRF_MAX_TAPS))
    whole = np.floor(sig)
    frac = sig - whole
    left = max(0, -int(whole.min()))
    right = max(0, int(np.max(whole + (frac > 0.0))))
    K = h.size + left + right
    _check_counts(sh.size, K)
    H = np.zeros((sh.size, K), dtype=np.float64)
    for j in range(sh.size):
        i, f = int(whole[j]), float(frac[j])
        a = left + i                                            # the row's index of tap 0 moved by the whole steps
        if f == 0.0:
            H[j, a:a + h.size] = h
        else:
            H[j, a:a + h.size] = (1.0 - f) * h
            H[j, a + 1:a + 1 + h.size] += f * h
    return H, k0 + left, sh.copy()


def loglik_bank(X, init_params, lengths, Time, L, T, obs, bank, times=None, weights=None, tol=7, MAX=10000, pl_f32=False,
                predict=False, block=8192, device=0, info=None, normalize=False):
    """loglik for every response of a bank at once, from ONE solve per block and curve: solve_pl_device writes the PL block and
    loglik_irf_bank_device scores it against the J responses of bank = (H (J, K), k0[, table]) (gaussian_bank, shift_bank) -- the
    convolved blocks are never written.  Returns P (J, S): row j is, bit for bit, loglik(X, ..., irf=(H[j], k0)) with the same
    arguments (P started from zeros, the curves subtracted in order).  Every other argument, the blocking and the refusals are
    loglik's.  info receives sse (J, C, S), esum (J, C, S) -- the sums of the errors, so that a magnitude profile can follow --
    status (C, S) and ncol_out."""
    r = _Resident(X, init_params, lengths, Time, L, T, obs, times, weights, block, normalize, bank=bank)
    J = r.taps.shape[0]
    P = np.zeros((J, r.S))
    sse = np.zeros((J, r.Cn, r.S))
    esum = np.zeros((J, r.Cn, r.S))
    if info is not None:
        info.update(sse=sse, esum=esum, status=r.status, ncol_out=r.ncol_out)
    for b in r.blocks(tol, MAX, pl_f32, predict, device):
        P_d, sse_d, es_d = b.zeros(J, b.n), b.zeros(r.Cn, J, b.n), b.zeros(r.Cn, J, b.n)
        for c in b.curves():
            r.bank_moments(b, c, sse_d, es_d)
            P_d -= sse_d[c]                                       # loglik's P[s] -= sse, curves in order
        P[:, b.sl] = P_d.cpu().numpy()
        _moments_down(sse, sse_d, b.sl)
        _moments_down(esum, es_d, b.sl)
    return P


def loglik_profile(X, init_params, lengths, Time, L, T, obs, bank, times=None, weights=None, tol=7, MAX=10000, pl_f32=False,
                   predict=False, block=8192, device=0, info=None, normalize=False):
    """The profile likelihood over a bank of instrument responses: LL[s] = max_j loglik_bank(...)[j, s].  The curves are summed
    first -- one response serves all curves of an experiment -- then irf_bank_profile_device takes the greatest row per sample.
    Returns LL (S,); info receives loglik_bank's entries, P (J, S) and best (S,) int32, the first response that attains the
    maximum (-1, with LL = -inf, where every response scores -inf or NaN).  The time shift and the width of the response are
    nuisance parameters that do not enter the solve: the profile costs one solve per sample, like mag_profile.

    functools.partial(loglik_profile, init_params=..., ..., bank=...) is a valid `loglik` for refine.run, mcmc.run and
    mcmc.run_tempered WITHOUT early_reject: the early stop lives in the fused steppers (trpl_loglik_cut*), which compare the
    bare curve and never see a convolved one."""
    own = {}
    Pb = loglik_bank(X, init_params, lengths, Time, L, T, obs, bank, times=times, weights=weights, tol=tol, MAX=MAX, pl_f32=pl_f32,
                     predict=predict, block=block, device=device, info=own, normalize=normalize)
    J, S = Pb.shape
    LL = np.full(S, -np.inf)
    best = np.full(S, -1, dtype=np.int32)
    if S:
        import torch

        from . import device as tdev
        dev = torch.device("cuda", device)
        with torch.cuda.device(dev):
            LL_d = torch.empty(S, dtype=torch.float64, device=dev)
            best_d = torch.empty(S, dtype=torch.int32, device=dev)
            tdev.irf_bank_profile_device(torch.from_numpy(Pb).to(dev), best_d, LL_d)
            LL, best = LL_d.cpu().numpy(), best_d.cpu().numpy()
    if info is not None:
        info.update(own, P=Pb, best=best)
    return LL


def _check_prior(log_prior, J, M, marginal):
    """The log prior weights of the J x M cells as a (J * M,) float64 array, or None: (J, M), (J * M,) or, with M == 1, (J,)."""
    if log_prior is None:
        return np.full(J * M, -math.log(J * M)) if marginal else None
    if not marginal:
        raise ValueError('log_prior: only reduce="marginal" takes prior weights')
    lp = np.ascontiguousarray(log_prior, dtype=np.float64)
    if lp.size != J * M or lp.shape not in ((J, M), (J * M,)):
        raise ValueError("log_prior must have shape (J, M) = (%d, %d) or (J * M,), got %r" % (J, M, lp.shape))
    if np.isnan(lp).any() or (lp == np.inf).any():
        raise ValueError("log_prior must not hold NaN or +inf (-inf excludes a cell)")
    return lp.ravel()


def loglik_nuisance(X, init_params, lengths, Time, L, T, obs, bank, mag="fixed", reduce="max", tf=1.0, log_prior=None, times=None,
                    weights=None, tol=7, MAX=10000, pl_f32=False, predict=False, block=8192, device=0, keep_moments=False,
                    info=None, normalize=False):
    """The likelihood of one experiment with its nuisance parameters reduced on the device: the J responses of bank = (H (J, K),
    k0[, table]) x the magnitude offset.  loglik_bank's staging and block loop -- one solve per block and curve,
    loglik_irf_bank_device for the J responses -- and, while the block's moments are resident, ONE nuisance_reduce_device over
    its cells: only LL, best, best_mag and status come down.

    mag: "fixed" (the offset of X[:, 12] as it is), "profile" (per response the likelihood-maximising common offset of the
    curves, mag_profile's) or a sequence of M <= 64 offsets (the grid of mag_grid); cell j * M + m is response j at offset m.
    reduce: "max", the profile -- LL[s] = the greatest cell -- or "marginal", LL[s] = tf * log sum_i exp(v_i / tf + log_prior_i),
    the log of the marginal of the tempered joint posterior over the cells.  log_prior (J, M) or (J * M,): the log prior weight
    of each cell, -inf excludes one; None is the uniform prior -ln(J M) per cell; marginal only.  weights: the curves' wsum is
    the math.fsum of each curve's weights, else the number of its observations.  Every other argument, the blocking and the
    refusals are loglik_bank's.  mag="fixed", reduce="max" is loglik_profile, bit for bit.

    Returns LL (S,).  info receives best (S,) int32, the first cell that attains the maximum (-1, with LL = -inf, where every
    cell is -inf or NaN), best_mag (S,), the offset at that cell, status (C, S), ncol_out, cells = (J, M) and, with
    keep_moments=True only, sse and esum (J, C, S).

    functools.partial(loglik_nuisance, init_params=..., ..., bank=...) is a valid `loglik` for refine.run and mcmc.run WITHOUT
    early_reject: the early stop lives in the fused steppers (trpl_loglik_cut*), which compare the bare curve and never see a
    convolved one.  A marginal is formed at ONE tf: it is a valid `loglik` for refine.run and mcmc.run at that tf, and NOT for
    mcmc.run_tempered, whose rungs differ in tf (the maximum is valid there)."""
    r = _Resident(X, init_params, lengths, Time, L, T, obs, times, weights, block, normalize, bank=bank, reduction=(mag, reduce, tf))
    S, Cn, J = r.S, r.Cn, r.taps.shape[0]
    lp = _check_prior(log_prior, J, r.M, r.marginal)
    wsum = np.array([float(len(kw["obs"])) if weights is None else math.fsum(kw["wts"]) for kw in r.staged])
    LL = np.full(S, -np.inf)
    best = np.full(S, -1, dtype=np.int32)
    best_mag = np.full(S, np.nan)
    if info is not None:
        info.update(best=best, best_mag=best_mag, status=r.status, ncol_out=r.ncol_out, cells=(J, r.M))
        if keep_moments:
            info.update(sse=np.zeros((J, Cn, S)), esum=np.zeros((J, Cn, S)))
    for b in r.blocks(tol, MAX, pl_f32, predict, device):
        if b.first:
            lp_d = None if lp is None else b.to_dev(lp)
            LL_d, bm_d = b.mag.new_empty(b.size), b.mag.new_empty(b.size)
            best_d = b.torch.empty(b.size, dtype=b.torch.int32, device=b.dev)
        sse_d, es_d = b.zeros(Cn, J, b.n), b.zeros(Cn, J, b.n)
        for c in b.curves():
            r.bank_moments(b, c, sse_d, es_d)
        b.tdev.nuisance_reduce_device(sse_d, es_d, wsum, LL_d[:b.n], best=best_d[:b.n], best_mag=bm_d[:b.n], mag=mag, marginal=r.marginal,
                                      tf=r.tf, log_prior=lp_d)
        LL[b.sl] = LL_d[:b.n].cpu().numpy()
        best[b.sl] = best_d[:b.n].cpu().numpy()
        best_mag[b.sl] = bm_d[:b.n].cpu().numpy()
        if keep_moments and info is not None:
            _moments_down(info["sse"], sse_d, b.sl)
            _moments_down(info["esum"], es_d, b.sl)
    return LL
