"""Posterior-predictive PL band: the posterior taken back to the data.

Per time column, the weighted mean, the weighted variance and the envelope of the model values
y = log10 PL + mag -- the values the likelihood compared with the observations -- over the samples whose posterior weight
is finite and > 0 and whose solve converged (trpl_predictive*, include/trpl.h; csrc/predictive.hip).  Every reduction over
the samples runs on the GPU; there is no CPU fallback.

    band(pl, W, ...)                        one PL matrix on the host -> dict(mean, var, lo, hi, sw)
    band_quantiles(pl, W, q, ...)           one PL matrix on the host -> (K, ncol) weighted quantiles of y per column
    merge(a, b)                             two finished bands (shards of a multi-GPU run, separate runs) -> one; NumPy
    posterior_predictive(X, W, ...)         re-solve the weighted samples per curve and accumulate on the device;
                                            quantiles=(0.025, 0.5, 0.975) adds the median and the 95 % band
"""
import numpy as np

from . import _abi

FIELDS = ("mean", "var", "lo", "hi", "sw")       # the rows of trpl_predictive_finish_dev's out[5][ncol]


def _result(out):
    return {k: out[i].copy() for i, k in enumerate(FIELDS)}


def band(pl, W, mag=None, status=None, normalize=False, device=0, ncol=None, info=None):
    """trpl_predictive on host arrays: pl (rows, ld) float32 / float64 PL as solve_pl returns it, W (rows,) posterior
    weights (a row counts iff its weight is finite and > 0), mag (rows,) log offsets (X[:, 12]; None: 0), status (rows,)
    int32 of the solve (a nonzero entry drops the row; None: all converged).  ncol (default ld): the valid columns.
    Returns dict(mean, var, lo, hi, sw), each (ncol,); a column no used row reached has sw = 0, NaN mean / var, lo = +inf,
    hi = -inf."""
    pl = np.asarray(pl)
    if pl.ndim != 2 or pl.dtype not in (np.float32, np.float64):
        raise ValueError("pl must be a 2-D float32/float64 array")
    pl = np.ascontiguousarray(pl)
    rows, ld = pl.shape
    ncol = int(ld if ncol is None else ncol)
    W = np.ascontiguousarray(W, dtype=np.float64)
    mag = None if mag is None else np.ascontiguousarray(mag, dtype=np.float64)
    status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
    if W.shape != (rows,) or (mag is not None and mag.shape != (rows,)) or (status is not None and status.shape != (rows,)):
        raise ValueError("W, mag and status must have one entry per row of pl")
    out = np.empty((5, max(ncol, 1)))
    sec = _abi.C.c_double(0.0)
    _abi.check(_abi.lib().trpl_predictive(_abi.ptr(pl), pl.itemsize, rows, ncol, ld, _abi.ptr(mag), _abi.ptr(W), _abi.ptr(status),
                                          _abi.FLAG_NORMALIZE if normalize else 0, _abi.ptr(out), int(device), _abi.C.byref(sec)))
    if info is not None:
        info.update(seconds=sec.value, chunks=int(_abi.lib().trpl_predictive_chunks(rows, ncol, pl.itemsize)))
    return _result(out)


def band_quantiles(pl, W, q, mag=None, status=None, normalize=False, rule=None, device=0, ncol=None, flags=0, keep_store=None):
    """The weighted quantiles of y = log10 PL + mag per time column, for one PL matrix on the host: the matrix is copied to
    the device, gathered into the transposed y store (trpl_predictive_gather_dev) and selected from
    (trpl_weighted_quantiles_dev).  pl, W, mag, status, normalize, ncol as band() takes them; q, rule as
    posterior.quantiles (default rule: the largest y below for q < 0.5, the smallest above otherwise); flags:
    _abi.Q_FORCE_STREAM.  Returns (K, ncol).  keep_store: a dict that receives the store `Y` (ncol, rows) and its weights `Wq`
    (rows,) as NumPy arrays."""
    import torch

    from . import device as tdev
    pl = np.asarray(pl)
    if pl.ndim != 2 or pl.dtype not in (np.float32, np.float64):
        raise ValueError("pl must be a 2-D float32/float64 array")
    pl = np.ascontiguousarray(pl)
    rows, ld = pl.shape
    ncol = int(ld if ncol is None else ncol)
    W = np.ascontiguousarray(W, dtype=np.float64)
    mag = None if mag is None else np.ascontiguousarray(mag, dtype=np.float64)
    status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
    if W.shape != (rows,) or (mag is not None and mag.shape != (rows,)) or (status is not None and status.shape != (rows,)):
        raise ValueError("W, mag and status must have one entry per row of pl")
    q, rule = tdev.quantile_requests(q, rule)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
        Y = torch.empty((max(ncol, 1), rows), dtype=torch.float64, device=dev)
        Wq = torch.empty(rows, dtype=torch.float64, device=dev)
        out = torch.empty((q.size, max(ncol, 1)), dtype=torch.float64, device=dev)
        tdev.predictive_gather_device(up(pl), up(W), Y, Wq, mag=up(mag), status=up(status), ncol=ncol,
                                      flags=_abi.FLAG_NORMALIZE if normalize else 0)
        tdev.weighted_quantiles_device(Y, Wq, q, out, rule=rule, flags=flags)
        if keep_store is not None:
            keep_store.update(Y=Y.cpu().numpy(), Wq=Wq.cpu().numpy())
        return out.cpu().numpy()


def merge(a, b):
    """Two FINISHED bands over the same columns -> the band of their union (Chan's pairwise formula on sw, mean,
    M2 = var * sw; lo / hi by min / max).  A side whose sw is 0 passes the other through bit for bit.  Plain NumPy.
    Quantiles do not merge: the `quantile` rows of posterior_predictive(quantiles=...) of two shards say nothing about the
    quantiles of their union, so sharded / multi-GPU quantiles are out of scope -- select from one store that holds every
    weighted sample (a store of ncol * n_used * 8 bytes; the weighted samples are few)."""
    a = {k: np.asarray(a[k], dtype=np.float64) for k in FIELDS}
    b = {k: np.asarray(b[k], dtype=np.float64) for k in FIELDS}
    if any(a[k].shape != a["sw"].shape or b[k].shape != a["sw"].shape for k in FIELDS):
        raise ValueError("both bands must cover the same columns")
    with np.errstate(invalid="ignore", divide="ignore"):
        s = a["sw"] + b["sw"]
        d = b["mean"] - a["mean"]
        mean = a["mean"] + d * (b["sw"] / s)
        var = ((a["var"] * a["sw"] + b["var"] * b["sw"]) + (d * d) * ((a["sw"] * b["sw"]) / s)) / s
    ea, eb = a["sw"] == 0, b["sw"] == 0
    out = {"mean": np.where(eb, a["mean"], np.where(ea, b["mean"], mean)),
           "var": np.where(eb, a["var"], np.where(ea, b["var"], var)),
           "lo": np.fmin(a["lo"], b["lo"]), "hi": np.fmax(a["hi"], b["hi"]),
           "sw": np.where(eb, a["sw"], np.where(ea, b["sw"], s))}
    return out


def posterior_predictive(X, W, init_params, sim_params, lengths=None, block=4096, predict=False, normalize=False, tol=7,
                         MAX=10000, device=0, quantiles=None, max_store_bytes=8 << 30, irf=None):
    """The posterior-predictive band of every curve.

    X (S, 13) samples in the solver's units (columns 0..11 matPar, 12 the magnitude offset), W (S,) their posterior weights
    (posterior.weights), init_params (C, L) the curves' excitations, sim_params = [Length or per-curve lengths, Time, L, T,
    plT, ...] as driver.simulate takes them (lengths overrides its first entry).  The samples with a finite weight > 0 are
    selected on the host -- most weights are exactly 0.0 (posterior.exact_cut_margin) and those samples are never solved;
    per curve they are solved in blocks of `block` (solve_pl_device, fp64 PL) and every block is accumulated on the device
    (predictive_accumulate_device, mag = X[:, 12]).  Flagged systems are left out and counted.
    Returns one dict per curve: times (ncol,), mean, var, lo, hi, sw (ncol,), n_used (samples with weight), n_solved
    (systems solved for this curve, = n_used), n_flagged (of those, the non-converged ones).
    quantiles: a tuple of numbers in (0, 1), e.g. (0.025, 0.5, 0.975): every curve's dict gains `q` (the tuple) and `quantile`
    (K, ncol), the weighted quantiles of y per time column (band_quantiles' default rules).  The y of every block is kept in
    a store (ncol, n_used) fp64 on the device (predictive_gather_device beside the accumulation) and one selection follows
    the last block; a store above max_store_bytes raises ValueError, before anything is solved.  One device only: quantiles
    do not merge (see merge).
    irf = (h, k0) (irf.gaussian, irf.from_samples; taps at the spacing of the PL columns): every solved block is convolved with
    the instrument response on the device (convolve_irf_device) before it is accumulated and gathered.  The band is then of the
    quantity the detector saw and has ncol - k0 columns, at the first ncol - k0 times; not with normalize."""
    import torch

    from . import device as tdev
    X = np.ascontiguousarray(X, dtype=np.float64)
    W = np.ascontiguousarray(W, dtype=np.float64)
    init_params = np.atleast_2d(np.ascontiguousarray(init_params, dtype=np.float64))
    if X.ndim != 2 or X.shape[1] != 13 or W.shape != (X.shape[0],):
        raise ValueError("X must be (S, 13) and W (S,)")
    Cn = init_params.shape[0]
    Time, L, T, plT = float(sim_params[1]), int(sim_params[2]), int(sim_params[3]), int(sim_params[4])
    lens = sim_params[0] if lengths is None else lengths
    lens = np.broadcast_to(np.asarray(lens, dtype=np.float64), (Cn,))
    if init_params.shape[1] != L or int(block) < 1:
        raise ValueError("init_params must be (C, L) and block >= 1")
    with np.errstate(invalid="ignore"):
        sel = np.flatnonzero(np.isfinite(W) & (W > 0))
    ncol = ncol_pl = T // plT + 1
    times = np.linspace(0, Time, T + 1)[::plT]
    if irf is not None:
        from .irf import _check_irf
        irf = _check_irf(irf)
        if normalize:
            raise ValueError("irf does not combine with normalize: a convolved curve's first column is not PL(0)")
        if ncol_pl - irf[1] < 1:
            raise ValueError("irf: k0 = %d leaves no column of %d" % (irf[1], ncol_pl))
        ncol = ncol_pl - irf[1]
        times = times[:ncol]
    if quantiles is not None:
        quantiles = tuple(float(v) for v in np.atleast_1d(quantiles))
        if not 1 <= len(quantiles) <= _abi.Q_MAX or not all(0.0 < v < 1.0 for v in quantiles):
            raise ValueError("quantiles must be 1 .. %d numbers in (0, 1)" % _abi.Q_MAX)
        need = int(ncol) * int(sel.size) * 8
        if need > int(max_store_bytes):
            raise ValueError("the y store of %d columns x %d weighted samples needs %d bytes, more than max_store_bytes = %d"
                             % (ncol, sel.size, need, int(max_store_bytes)))
    empty = {"mean": np.full(ncol, np.nan), "var": np.full(ncol, np.nan), "lo": np.full(ncol, np.inf),
             "hi": np.full(ncol, -np.inf), "sw": np.zeros(ncol)}
    if sel.size == 0:
        res = [dict(times=times, n_used=0, n_solved=0, n_flagged=0, **{k: v.copy() for k, v in empty.items()}) for _ in range(Cn)]
        if quantiles is not None:
            for r in res:
                r.update(q=quantiles, quantile=np.full((len(quantiles), ncol), np.nan))
        return res
    block = min(int(block), sel.size)
    dev = torch.device("cuda", device)
    flags = _abi.FLAG_PREDICT if predict else 0
    result = []
    with torch.cuda.device(dev):
        ini_d = torch.from_numpy(init_params).to(dev)
        Xs = torch.from_numpy(np.ascontiguousarray(X[sel])).to(dev)
        Ws = torch.from_numpy(np.ascontiguousarray(W[sel])).to(dev)
        pl_d = torch.empty((block, ncol_pl), dtype=torch.float64, device=dev)
        if irf is not None:
            h_d = torch.from_numpy(irf[0]).to(dev)
            seen_d = torch.empty((block, ncol), dtype=torch.float64, device=dev)          # what the band is taken of
        st_d = torch.empty(block, dtype=torch.int32, device=dev)
        state, out = tdev.predictive_state(ncol), torch.empty((5, ncol), dtype=torch.float64, device=dev)
        sizes = {block, sel.size % block or block}               # the row counts that occur: full blocks and the last one
        ws = max((tdev.predictive_workspace(n, ncol, 8) for n in sizes), key=lambda t: t.numel())
        if quantiles is not None:
            Y = torch.empty((ncol, sel.size), dtype=torch.float64, device=dev)
            Wq = torch.empty(sel.size, dtype=torch.float64, device=dev)
            qout = torch.empty((len(quantiles), ncol), dtype=torch.float64, device=dev)
        for c in range(Cn):
            tdev.predictive_init_device(state)
            n_flagged = n_solved = 0
            for a in range(0, sel.size, block):
                n = min(block, sel.size - a)
                mat_d, mag_d = Xs[a:a + n, :12].contiguous(), Xs[a:a + n, 12].contiguous()
                tdev.solve_pl_device(mat_d, lens[c], Time, L, T, ini_d[c].contiguous(), pl_d[:n], status=st_d[:n], tol=tol,
                                     MAX=MAX, plT=plT, flags=flags)
                if irf is not None:
                    tdev.convolve_irf_device(pl_d[:n], h_d, irf[1], seen_d[:n])
                blk_d = pl_d[:n] if irf is None else seen_d[:n]
                tdev.predictive_accumulate_device(blk_d, Ws[a:a + n], state, ws, mag=mag_d, status=st_d[:n],
                                                  flags=_abi.FLAG_NORMALIZE if normalize else 0)
                if quantiles is not None:
                    tdev.predictive_gather_device(blk_d, Ws[a:a + n], Y, Wq, row0=a, mag=mag_d, status=st_d[:n],
                                                  flags=_abi.FLAG_NORMALIZE if normalize else 0)
                n_flagged += int((st_d[:n] != 0).sum().item())
                n_solved += n
            tdev.predictive_finish_device(state, out)
            r = _result(out.cpu().numpy())
            r.update(times=times, n_used=int(sel.size), n_solved=n_solved, n_flagged=n_flagged)
            if quantiles is not None:
                tdev.weighted_quantiles_device(Y, Wq, quantiles, qout)
                r.update(q=quantiles, quantile=qout.cpu().numpy())
            result.append(r)
    return result
