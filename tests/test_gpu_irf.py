"""trpl_convolve_irf* on the device against the NumPy restatement of its definition (tests/irf_ref.py), bit for bit, at every
shape where the tiling can go wrong -- one column, a wave of columns and its neighbours, a tile of columns and its neighbours,
more than two tiles; one tap up to the cap; the tap of time zero first, second and last; a tile of rows and its neighbours; rows
that are only element-aligned, with a canary behind every row -- and the routes that carry it: irf.loglik against the three
device calls issued by hand, gpu_info["irf"] of simulate, posterior_predictive(irf=...).  Tile and cap are read from
include/trpl.h (tests/test_irf_host.py checks that the binding agrees)."""
import numpy as np
import pytest

import abi_header as H
import irf_ref as R
import likelihood_ref as LR

pytestmark = pytest.mark.gpu

_define = H.defines().__getitem__
TC, TR, CAP, MAXK = _define("TRPL_IRF_TILE_COLS"), _define("TRPL_IRF_TILE_ROWS"), _define("TRPL_IRF_GRID_CAP"), _define("TRPL_IRF_MAX_TAPS")
NCOLS = [1, 2, 63, 64, 65, TC - 1, TC, TC + 1, 2 * TC + 3]
KS = [1, 2, 3, 64, 65, MAXK]
ROWS = [1, TR - 1, TR, TR + 1]
DTYPES = [np.float32, np.float64]


def _up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared inputs are read-only


def _device_convolve(gpu, pl, h, k0, ncol, pad=5):
    """convolve_irf_device on pl [rows][ld] (ncol valid columns) into out [rows][ncol - k0 + pad] filled with the canary.
    Returns the whole out buffer and the input as the device holds it afterwards."""
    import torch
    pl_d = _up(pl)
    out_d = torch.full((pl.shape[0], ncol - k0 + pad), R.CANARY, dtype=pl_d.dtype, device="cuda")
    gpu.device.convolve_irf_device(pl_d, _up(np.asarray(h, dtype=np.float64)), k0, out_d, ncol=ncol)
    torch.cuda.synchronize()
    return out_d.cpu().numpy(), pl_d.cpu().numpy()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_bit_for_bit_at_every_boundary(gpu, dtype, K):
    """Every ncol of NCOLS x k0 in {0, 1, K - 1} x rows of ROWS, ld = ncol + 3 and out_ld = ncol_out + 5: the valid columns are
    the restatement's bits, the canaries behind them survive, the input is untouched.  Taps of mixed sign over 12 decades."""
    h = R.taps(K, 5)
    done = 0
    for ncol in NCOLS:
        for k0 in sorted({0, min(1, K - 1), K - 1}):
            if ncol - k0 < 1:
                continue
            for rows in ROWS:
                pl = R.block(rows, ncol, dtype)
                out, pl_after = _device_convolve(gpu, pl, h, k0, ncol)
                want = R.convolve_ref(pl, h, k0, ncol=ncol)
                label = (dtype.__name__, K, ncol, k0, rows)
                assert R.same_bits(out[:, :ncol - k0], want), label
                assert np.all(out[:, ncol - k0:] == R.CANARY), label
                assert R.same_bits(pl_after, pl), label
                done += 1
    assert done >= len(ROWS) * (len(NCOLS) if K == 1 else 2 * len([n for n in NCOLS if n > 1]))


def test_rows_beyond_the_grid_cap(gpu):
    """More row groups than TRPL_IRF_GRID_CAP workgroups at the narrowest shape: every workgroup walks to a second tile."""
    rows = CAP * TR + TR + 1
    rng = np.random.default_rng(11)
    pl = rng.normal(size=(rows, 2))
    out, _ = _device_convolve(gpu, pl, [-3.0], 0, 2, pad=1)
    assert R.same_bits(out[:, :2], R.convolve_ref(pl, [-3.0], 0)) and np.all(out[:, 2] == R.CANARY)
    assert np.array_equal(out[:, :2], -3.0 * pl)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_identity_and_shift_return_the_inputs_bits(gpu, dtype):
    ncol = TC + 9
    pl = R.block(TR + 1, ncol, dtype)
    out, _ = _device_convolve(gpu, pl, [1.0], 0, ncol)
    assert R.same_bits(out[:, :ncol], pl[:, :ncol])
    K = 9
    for k0 in (0, 4, 8):
        for d in (0, 3, 8):
            h = np.zeros(K)
            h[d] = 1.0
            out, _ = _device_convolve(gpu, pl, h, k0, ncol)
            j = np.arange(ncol - k0)
            ok = j + k0 - d >= 0
            want = np.zeros((pl.shape[0], ncol - k0), dtype=dtype)                  # +0.0 where the column is negative
            want[:, ok] = pl[:, :ncol][:, j[ok] + k0 - d]
            assert R.same_bits(out[:, :ncol - k0], want), (k0, d)
    assert R.same_bits(gpu.irf.convolve(pl[:, :ncol], [1.0], 0), pl[:, :ncol])       # the host-buffer form


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_one_nan_poisons_exactly_its_window(gpu, dtype):
    ncol, K, k0 = TC + 40, 33, 16
    pl = np.array(R.block(TR, ncol, dtype))
    col = TC - 5                                            # its window straddles the first two column tiles
    pl[2, col] = np.nan
    h = R.taps(K, 3)
    h[7] = 0.0                                              # 0 * NaN is NaN
    out, _ = _device_convolve(gpu, pl, h, k0, ncol)
    want = R.convolve_ref(pl, h, k0, ncol=ncol)
    assert R.same_bits(out[:, :ncol - k0], want)
    hit = np.zeros(want.shape, dtype=bool)
    hit[2, col - k0:col - k0 + K] = True
    assert np.array_equal(np.isnan(out[:, :ncol - k0]), hit)
    got = gpu.irf.convolve(pl[:, :ncol], h, k0)             # the host-buffer form stages the same kernel
    assert R.same_bits(got, want)


def test_refusals_that_need_a_device(gpu):
    import torch
    rows, ncol, K, k0 = 3, 20, 5, 2
    pl = torch.ones((rows, ncol), dtype=torch.float64, device="cuda")
    h = torch.full((K,), 0.2, dtype=torch.float64, device="cuda")
    out = torch.full((rows, ncol - k0), R.CANARY, dtype=torch.float64, device="cuda")
    conv = gpu.device.convolve_irf_device
    for bad in (lambda: conv(pl.cpu(), h, k0, out), lambda: conv(pl, h.cpu(), k0, out), lambda: conv(pl, h, k0, out.cpu()),
                lambda: conv(pl, h.float(), k0, out), lambda: conv(pl, h, k0, out.float()), lambda: conv(pl.int(), h, k0, out),
                lambda: conv(pl, h, k0, out[:, :-1].contiguous()), lambda: conv(pl, h, k0, out[:-1]), lambda: conv(pl[0], h, k0, out),
                lambda: conv(pl, h.reshape(1, K), k0, out), lambda: conv(pl.t(), h, k0, out), lambda: conv(pl, h, k0, out, ncol=ncol + 1)):
        with pytest.raises((ValueError, gpu.TrplError)):
            bad()
    for k0_bad in (-1, K):
        with pytest.raises(gpu.TrplError, match="k0"):
            conv(pl, h, k0_bad, torch.empty((rows, ncol + 1), dtype=torch.float64, device="cuda"))
    lib = gpu._abi.lib()
    rc = lib.trpl_convolve_irf_dev(pl.data_ptr(), 8, rows, ncol, ncol, h.data_ptr(), K, 0, pl.data_ptr(), ncol, None)
    assert rc == gpu._abi.ERR_ARG and b"out must not be pl" in lib.trpl_last_error()
    torch.cuda.synchronize()
    assert torch.all(out == R.CANARY) and torch.all(pl == 1.0)                    # a refused call launched nothing
    conv(pl[:0], h, k0, out[:0])                                                   # an empty block is a no-op
    conv(pl, h, k0, out)
    torch.cuda.synchronize()
    assert R.same_bits(out.cpu().numpy(), R.convolve_ref(np.ones((rows, ncol)), np.full(K, 0.2), k0))


# ------------------------------------------------------------------------------------------------ the routes that carry it
L_, T_, S_ = 32, 64, 8


@pytest.fixture(scope="module")
def problem(gpu):
    """Power_scan's first two curves at L = 32, T = 64, 8 samples, a Gaussian response of 12 taps either side; per curve the
    plain solve's PL matrix fetched from the device, and observations near the convolved curve of sample 0."""
    import torch
    w = gpu.workloads
    Time = T_ * 0.025
    ini, lens = w.power_scan(L_)
    ini, lens = np.ascontiguousarray(ini[:2]), lens[:2]
    X = w.samples(S_)
    irf = gpu.irf.gaussian(0.1, Time / T_)
    assert irf[1] >= 8 and T_ + 1 - irf[1] >= 40
    mat = _up(X[:, :12])
    pls = []
    for c in range(2):
        pl = torch.empty((S_, T_ + 1), dtype=torch.float64, device="cuda")
        st = torch.zeros(S_, dtype=torch.int32, device="cuda")
        gpu.device.solve_pl_device(mat, lens[c], Time, L_, T_, _up(ini[c]), pl, status=st)
        assert not st.cpu().numpy().any()
        pls.append(pl.cpu().numpy())
    ncol_out = T_ + 1 - irf[1]
    rng = np.random.default_rng(2)
    sim_t = np.linspace(0, Time, T_ + 1)
    n_obs = (ncol_out, 30)
    obs = [np.log10(np.abs(R.convolve_ref(pls[c], *irf)[0, :n_obs[c]])) + X[0, 12] + 0.05 * rng.normal(size=n_obs[c]) for c in range(2)]
    times = []
    for c in range(2):                                      # off the grid: unsorted, with the first and the last convolved node among them
        t = rng.uniform(0.0, sim_t[ncol_out - 1], n_obs[c])
        t[3], t[7], t[11] = sim_t[ncol_out - 1], 0.0, sim_t[5]
        times.append(t)
    wts = [LR.weights(n_obs[c], c) for c in range(2)]
    return dict(Time=Time, ini=ini, lens=lens, X=X, irf=irf, pls=pls, ncol_out=ncol_out, obs=obs, times=times, wts=wts, sim_t=sim_t)


def _by_hand(gpu, p, irf, dtype, offgrid, weighted):
    """solve_pl_device, convolve_irf_device (irf None: left out), loglik[_weighted]_from_pl_device per curve, issued here.
    Returns P, sse (C, S) and per curve the block the likelihood read, fetched from the device."""
    import torch
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    X = p["X"]
    mat, mag = _up(X[:, :12]), _up(X[:, 12])
    P = torch.zeros(S_, dtype=torch.float64, device="cuda")
    sse = torch.zeros((2, S_), dtype=torch.float64, device="cuda")
    seen, brackets = [], []
    k0 = 0 if irf is None else irf[1]
    for c in range(2):
        pl = torch.empty((S_, T_ + 1), dtype=tdt, device="cuda")
        st = torch.zeros(S_, dtype=torch.int32, device="cuda")
        gpu.device.solve_pl_device(mat, p["lens"][c], p["Time"], L_, T_, _up(p["ini"][c]), pl, status=st)
        blk = pl
        if irf is not None:
            blk = torch.empty((S_, T_ + 1 - k0), dtype=tdt, device="cuda")
            gpu.device.convolve_irf_device(pl, _up(irf[0]), k0, blk)
            assert R.same_bits(blk.cpu().numpy(), R.convolve_ref(pl.cpu().numpy(), *irf))      # the restatement's bits
        o, wt, kw, br = p["obs"][c], p["wts"][c], {}, None
        if offgrid:
            order = np.argsort(p["times"][c], kind="stable")
            o, wt = o[order], wt[order]
            br = gpu.bracket_times(p["sim_t"][:T_ + 1 - k0], p["times"][c][order])
            kw = dict(zip(("obs_hi", "obs_dx", "obs_h"), map(_up, br)))
        if weighted:
            gpu.device.loglik_weighted_from_pl_device(blk, _up(o), _up(wt), mag, P=P, sse=sse[c], status=st, **kw)
        else:
            gpu.device.loglik_from_pl_device(blk, _up(o), mag, P=P, sse=sse[c], status=st, **kw)
        seen.append(blk.cpu().numpy())
        brackets.append((o, wt if weighted else None, br))
    torch.cuda.synchronize()
    return P.cpu().numpy(), sse.cpu().numpy(), seen, brackets


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
def test_loglik_is_the_three_device_calls(gpu, problem, offgrid, weighted):
    from test_gpu_likelihood_instances import _sum_ratios
    p = problem
    kw = dict(times=p["times"] if offgrid else None, weights=p["wts"] if weighted else None)
    args = (p["X"], p["ini"], p["lens"], p["Time"], L_, T_, p["obs"])
    for dtype in DTYPES:
        info = {}
        P = gpu.irf.loglik(*args, p["irf"], pl_f32=dtype == np.float32, info=info, **kw)
        hP, hsse, seen, used = _by_hand(gpu, p, p["irf"], dtype, offgrid, weighted)
        assert R.same_bits(P, hP) and R.same_bits(info["sse"], hsse), (dtype.__name__, offgrid, weighted)
        assert info["ncol_out"] == p["ncol_out"] and not info["status"].any() and np.isfinite(P).all() and (P < 0).all()
        # accumulated into a given P, in sample blocks that do not divide S.  A block is a launch of its own size, and the FAST
        # steppers agree between launch sizes to 1e-9 in PL (gpu_common.RTOL_FAST), i.e. 4.3e-10 in log10 PL: on sse = sum e^2
        # that is 2 sum|e| 4.3e-10 <= 8.7e-10 sse / min|e|-weighted mean, inside 1e-7 sse while the mean |e| is above 0.01
        # (the observations carry 0.05 of noise); float32 rounds the same PL, so its log10 moves by an ulp, 1.2e-7 |lg|
        P0 = np.linspace(1.0, 2.0, S_)
        Pb = gpu.irf.loglik(*args, p["irf"], pl_f32=dtype == np.float32, P=P0.copy(), block=3, **kw)
        assert np.allclose(Pb - P0, P, rtol=1e-7 if dtype == np.float64 else 1e-4, atol=1e-9)
        # the one-tap response is the route without the convolution, bit for bit
        one = gpu.irf.loglik(*args, ([1.0], 0), pl_f32=dtype == np.float32, **kw)
        assert R.same_bits(one, _by_hand(gpu, p, None, dtype, offgrid, weighted)[0])
        # sse against the reference likelihood of the restated convolved block (its bits are the device block's, asserted in
        # _by_hand): the bound test_gpu_likelihood_instances.py holds the from_pl forms to, no new tolerance
        for c in range(2):
            o, wt, br = used[c]
            n = len(o)
            ref = LR.from_pl_ref(seen[c], o, p["X"][:, 12], 0, br, wt)
            f64_log = dtype == np.float64
            w2 = float(np.sum(wt)) if weighted else float(n)
            w1 = w2 if weighted else 2.0 * n
            depth = -(-n // 256) + 9 + (2 if weighted else 0)
            r = _sum_ratios(info["sse"][c], None, ref, depth, *((w2, w1) if f64_log else (None, None)), (dtype.__name__, offgrid, weighted, c))
            print("irf.loglik sse error / bound, curve %d %s: %.3g" % (c, dtype.__name__, r[0]))


def _simulate(gpu, p, e_data, gpu_info):
    info = dict(sims_per_gpu=S_, num_gpus=1, fused=True, pl_dtype=np.float64)
    info.update(gpu_info)
    P = np.zeros((len(e_data), S_))
    gpu.simulate(gpu.pvSim, e_data, P, p["X"], [None], [None], 2, [list(p["lens"]), p["Time"], L_, T_, 1, 0, 7, 10000], p["ini"],
                 dict(log_pl=True, self_normalize=False), info, 0, np.zeros(1), np.zeros(1), np.zeros(1))
    return P


def test_simulate_with_an_irf_is_loglik_per_experiment(gpu, problem):
    from trpl_amd.likelihood import weights_from_uncertainty
    p = problem
    rng = np.random.default_rng(8)
    grid_t = [p["sim_t"][:len(o)] for o in p["obs"]]
    unc = [rng.uniform(0.05, 0.5, len(o)) for o in p["obs"]]
    e_data = [(grid_t, p["obs"], unc),                                              # on the grid: prefixes of the simulation grid
              (p["times"], [o + 0.1 for o in p["obs"]], unc)]                       # off the grid
    args = (p["X"], p["ini"], p["lens"], p["Time"], L_, T_)
    for weighted in (False, True):
        P = _simulate(gpu, p, e_data, dict(irf=p["irf"], weighted=weighted))
        wts = [weights_from_uncertainty(u) for u in unc] if weighted else None
        want = [gpu.irf.loglik(*args, e_data[0][1], p["irf"], weights=wts),
                gpu.irf.loglik(*args, e_data[1][1], p["irf"], times=p["times"], weights=wts)]
        assert R.same_bits(P[0], want[0]) and R.same_bits(P[1], want[1]), weighted
    single = _simulate(gpu, p, e_data[:1], dict(irf=p["irf"]))                      # one experiment takes the resident route too
    assert R.same_bits(single[0], gpu.irf.loglik(*args, e_data[0][1], p["irf"]))
    # the one-tap response is the existing resident route, bit for bit
    assert R.same_bits(_simulate(gpu, p, e_data, dict(irf=([1.0], 0))), _simulate(gpu, p, e_data, {}))
    # float32 PL buffer, the reference's default
    P32 = _simulate(gpu, p, e_data, dict(irf=p["irf"], pl_dtype=np.float32))
    assert R.same_bits(P32[0], gpu.irf.loglik(*args, e_data[0][1], p["irf"], pl_f32=True))


def test_posterior_predictive_of_what_the_detector_saw(gpu, problem):
    """The band with irf= is predictive.band's reference (tests/predictive_ref.py, the allowances test_gpu_predictive.py uses end
    to end) over the restated convolution of the plain solve's PL, and has ncol - k0 columns."""
    from test_gpu_predictive import _check, _y
    p = problem
    W = np.zeros(S_)
    W[[1, 2, 4, 5, 7]] = [0.3, 0.1, 0.25, 0.15, 0.2]
    sel = np.flatnonzero(W)
    sim = [list(p["lens"]), p["Time"], L_, T_, 1]
    res = gpu.posterior_predictive(p["X"], W, p["ini"], sim, irf=p["irf"], quantiles=(0.25, 0.75))
    small = gpu.posterior_predictive(p["X"], W, p["ini"], sim, irf=p["irf"], block=2)
    n = p["ncol_out"]
    for c in range(2):
        cv = R.convolve_ref(p["pls"][c][sel], *p["irf"])
        y = _y(gpu, cv, n, p["X"][sel, 12])
        for r in (res[c], small[c]):
            assert r["mean"].shape == (n,) and np.array_equal(r["times"], p["sim_t"][:n]) and (r["n_used"], r["n_flagged"]) == (5, 0)
            _check(r, y, W[sel], np.ones(5, dtype=bool), ("posterior_predictive irf", c))
        assert res[c]["quantile"].shape == (2, n) and np.all(res[c]["lo"] <= res[c]["quantile"][0])
        assert np.all(res[c]["quantile"][0] <= res[c]["quantile"][1]) and np.all(res[c]["quantile"][1] <= res[c]["hi"])
    plain = gpu.posterior_predictive(p["X"], W, p["ini"], sim)
    one = gpu.posterior_predictive(p["X"], W, p["ini"], sim, irf=([1.0], 0))
    assert all(np.array_equal(plain[c][k], one[c][k]) for c in range(2) for k in ("mean", "var", "lo", "hi", "sw"))
