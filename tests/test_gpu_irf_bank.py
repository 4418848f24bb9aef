"""trpl_loglik_irf_bank_dev against its definition (include/trpl.h): for every response j of the bank, sse[j] and esum[j] are the
bits of trpl_convolve_irf_dev followed by trpl_loglik_moments_from_pl_dev (trpl_loglik_weighted_from_pl_dev with weights), the two
existing device calls issued here per j -- tolerance zero.  Covered: the chunk of 256 observations and its neighbours, one tap up
to the cap, the tap of time zero first, second and last, the pass of TRPL_IRF_BANK_BLOCK responses and its neighbours, rows that
are only element-aligned, observations off the grid on both of the kernel's paths, flagged rows, NaN, canaries behind both
outputs; then the profile kernel against its NumPy restatement and the routes irf.loglik_bank / irf.loglik_profile."""
import functools

import numpy as np
import pytest

import irf_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
N_OBS = [1, 2, 255, 256, 257, 513]
KS = [1, 2, 33, 1024]
PAD = 5


def _up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _jb(gpu):
    return int(gpu._abi.lib().trpl_irf_bank_block())


def _js(gpu):
    jb = _jb(gpu)
    assert jb == gpu._abi.IRF_BANK_BLOCK and jb >= 3
    return [1, 2, jb - 1, jb, jb + 1, 2 * jb + 1]


def _block(rows, ncol, dtype, seed):
    """PL rows [rows][ncol + 3]: positive values over four decades (every convolved value of the positive banks below is positive,
    so that no term of a sum is the clamp's -307.65 squared, which would hide the low bits of the others); the padding holds the
    canary."""
    rng = np.random.default_rng(1000 * seed + 31 * rows + ncol)
    pl = np.full((rows, ncol + 3), R.CANARY, dtype=dtype)
    pl[:, :ncol] = np.exp(rng.normal(0.0, 2.3, (rows, ncol))).astype(dtype)
    return pl


def _bank(J, K, seed, k0=0):
    """J rows of K positive taps over three decades; row 1 (if there is one) zero-padded at both ends, as a shifted response is --
    in front no further than k0, so that convolved column 0 still has a term (a zero there is -inf in a float32 block)."""
    rng = np.random.default_rng(77 * J + K + seed)
    H = rng.uniform(0.1, 1.0, (J, K)) * 10.0 ** rng.uniform(-3.0, 0.0, (J, K))
    if J > 1 and K >= 4:
        H[1, :min(K // 4, k0)] = 0.0
        H[1, K - K // 3:] = 0.0
    return H


def _weights(n, seed):
    rng = np.random.default_rng(5 + seed)
    w = rng.uniform(0.5, 2.0, n)
    w[rng.random(n) < 0.2] = 0.0
    if n > 2:
        w[1] = 0.0
    return w


def _two_calls(gpu, pl_d, ncol, H, k0, obs_d, mag_d, wts_d=None, br_d=None, status_d=None, flags=0):
    """The definition: per response convolve_irf_device into a block of ncol - k0 columns, then the moments (or weighted) score."""
    import torch
    J, rows = H.shape[0], pl_d.shape[0]
    sse = torch.zeros((J, rows), dtype=torch.float64, device="cuda")
    esum = torch.zeros((J, rows), dtype=torch.float64, device="cuda")
    cv = torch.empty((rows, ncol - k0), dtype=pl_d.dtype, device="cuda")
    kw = {} if br_d is None else dict(zip(("obs_hi", "obs_dx", "obs_h"), br_d))
    for j in range(J):
        gpu.device.convolve_irf_device(pl_d, _up(H[j]), k0, cv, ncol=ncol)
        if wts_d is None:
            gpu.device.loglik_moments_from_pl_device(cv, obs_d, mag_d, sse=sse[j], esum=esum[j], status=status_d, flags=flags, **kw)
        else:
            gpu.device.loglik_weighted_from_pl_device(cv, obs_d, wts_d, mag_d, sse=sse[j], esum=esum[j], status=status_d, flags=flags, **kw)
    torch.cuda.synchronize()
    return sse.cpu().numpy(), esum.cpu().numpy()


def _bank_call(gpu, pl_d, ncol, H, k0, obs_d, mag_d, wts_d=None, br_d=None, status_d=None, flags=0, with_esum=True):
    """loglik_irf_bank_device into buffers with PAD canaries behind them.  Returns sse, esum (J, rows); asserts the canaries."""
    import torch
    J, rows = H.shape[0], pl_d.shape[0]
    bufs = [torch.full((J * rows + PAD,), R.CANARY, dtype=torch.float64, device="cuda") for _ in range(2)]
    sse, esum = (b[:J * rows].view(J, rows) for b in bufs)
    kw = {} if br_d is None else dict(zip(("obs_hi", "obs_dx", "obs_h"), br_d))
    before = pl_d.clone()
    gpu.device.loglik_irf_bank_device(pl_d, _up(H), k0, obs_d, mag_d, sse, esum=esum if with_esum else None, wts=wts_d, ncol=ncol,
                                      flags=flags, status=status_d, **kw)
    torch.cuda.synchronize()
    assert all(bool(torch.all(b[J * rows:] == R.CANARY)) for b in bufs), "a canary behind sse / esum was overwritten"
    assert torch.equal(before.view(torch.uint8), pl_d.view(torch.uint8)), "the PL block was written"
    if not with_esum:
        assert bool(torch.all(bufs[1] == R.CANARY))
    return sse.cpu().numpy(), esum.cpu().numpy()


def _one_case(gpu, dtype, K, k0, n_obs, J, rows, slack, weighted, seed, signed=False, flags=0):
    ncol = n_obs + k0 + slack
    pl = R.block(rows, ncol, dtype) if signed else _block(rows, ncol, dtype, seed)        # ld = ncol + 3 either way
    H = R.taps(K, seed)[None, :] * np.linspace(1.0, 2.0, J)[:, None] if signed else _bank(J, K, seed, k0)
    rng = np.random.default_rng(seed)
    obs_d, mag_d = _up(rng.normal(0.0, 1.0, n_obs)), _up(rng.normal(0.0, 0.3, rows))
    wts_d = _up(_weights(n_obs, seed)) if weighted else None
    pl_d = _up(pl)
    want = _two_calls(gpu, pl_d, ncol, H, k0, obs_d, mag_d, wts_d, flags=flags)
    got = _bank_call(gpu, pl_d, ncol, H, k0, obs_d, mag_d, wts_d, flags=flags)
    label = (dtype.__name__, K, k0, n_obs, J, rows, slack, weighted, signed, flags)
    assert R.same_bits(got[0], want[0]), ("sse",) + label
    assert R.same_bits(got[1], want[1]), ("esum",) + label
    # the comparison is of finite sums, except where the float32 clamp makes a non-positive convolved value -inf (signed taps)
    assert np.isfinite(want[0]).all() or (signed and (dtype == np.float32 or flags)), label
    return label


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_bit_for_bit_with_the_two_calls_at_every_boundary(gpu, dtype, K):
    """Every n_obs of N_OBS x every k0 of {0, 1, K - 1}, the J values, rows in {1, 3}, ncol equal to and larger than n_obs + k0 and
    the weights cycling through them; then every J of {1, 2, J_B - 1, J_B, J_B + 1, 2 J_B + 1} at the chunk boundaries 255, 256
    and 257.  ld = ncol + 3.  The first chunk of every case with K > 1 skips the terms left of column 0."""
    js = _js(gpu)
    k0s = sorted({0, min(1, K - 1), K - 1})
    done, i = [], 0
    for n_obs in N_OBS:
        for k0 in k0s:
            done.append(_one_case(gpu, dtype, K, k0, n_obs, js[i % len(js)], (1, 3)[i % 2], (0, 7)[(i // 2) % 2], i % 3 == 0, i))
            i += 1
    for J in js:
        for n_obs in (255, 256, 257):
            done.append(_one_case(gpu, dtype, K, k0s[i % len(k0s)], n_obs, J, (3, 1)[i % 2], (7, 0)[(i // 2) % 2], i % 3 == 1, i))
            i += 1
    assert len(done) == len(N_OBS) * len(k0s) + 3 * len(js)
    seen = lambda pos: {d[pos] for d in done}
    assert seen(3) == set(N_OBS) and seen(4) == set(js) and seen(5) == {1, 3} and seen(6) == {0, 7} and seen(7) == {False, True}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_negative_sums_take_the_clamp_and_the_f32_flag_rounds_a_double_block(gpu, dtype):
    """Taps of mixed sign over 12 decades on rows with negative elements (tests/irf_ref.py): a convolved value below DBL_MIN is
    clamped before the logarithm on both routes.  TRPL_FLAG_PL_F32 on either block type."""
    for flags in (0, gpu._abi.FLAG_PL_F32):
        _one_case(gpu, dtype, 33, 16, 257, _jb(gpu) + 1, 3, 7, False, 3, signed=True, flags=flags)
        _one_case(gpu, dtype, 5, 2, 300, 3, 3, 0, True, 4, flags=flags)


def _brackets(rng, n_obs, ncol_out, order):
    """obs_hi in [1, ncol_out - 1] with both ends among them, dx in [0, h]."""
    if order == "narrow":                                   # a window of 40 columns somewhere in the row
        lo = int(rng.integers(1, max(2, ncol_out - 40)))
        hi = rng.integers(lo, min(lo + 40, ncol_out), n_obs)
    else:
        hi = rng.integers(1, ncol_out, n_obs)
        hi[0], hi[-1] = 1, ncol_out - 1
    if order == "sorted":
        hi = np.sort(hi)
    h = np.full(n_obs, 0.025)
    dx = rng.uniform(0.0, 0.025, n_obs)
    dx[0] = 0.0
    return hi.astype(np.int32), dx, h


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_off_the_grid_on_both_paths(gpu, dtype, weighted):
    """Brackets sorted and shuffled on a row short enough that every chunk's span is staged; then a row of 3000 columns whose
    first chunk of 256 shuffled brackets spans the row -- more than the kernel stages (256 + TRPL_IRF_MAX_TAPS doubles), so
    every lane reads its window through the cache -- while the brackets of the second chunk lie within 40 columns and are staged:
    one call, both paths.  K = 33 and K = 1 (no halo), k0 = 0 and in the middle, ncol_out = 2 (the only bracket)."""
    jb = _jb(gpu)
    stage = 256 + gpu._abi.IRF_MAX_TAPS
    cases = [(33, 16, 300, 257, "sorted", jb + 1), (33, 0, 300, 513, "shuffled", 2), (1, 0, 40, 255, "shuffled", jb),
             (2, 1, 3, 2, "sorted", 1), (1024, 1023, 1100, 256, "sorted", 3)]
    for seed, (K, k0, ncol, n_obs, order, J) in enumerate(cases):
        rng = np.random.default_rng(40 + seed)
        br = _brackets(rng, n_obs, ncol - k0, order)
        assert int(br[0].max()) - int(br[0].min()) + 2 + K - 1 <= stage
        _check_off_grid(gpu, dtype, weighted, K, k0, ncol, J, br, seed)
    K, k0, ncol, J = 33, 5, 3000, jb + 1
    rng = np.random.default_rng(50)
    wide, narrow = _brackets(rng, 256, ncol - k0, "shuffled"), _brackets(rng, 44, ncol - k0, "narrow")
    assert int(wide[0].max()) - int(wide[0].min()) + 2 + K - 1 > stage >= int(narrow[0].max()) - int(narrow[0].min()) + 2 + K - 1
    _check_off_grid(gpu, dtype, weighted, K, k0, ncol, J, tuple(np.concatenate(p) for p in zip(wide, narrow)), 9)


def _check_off_grid(gpu, dtype, weighted, K, k0, ncol, J, br, seed):
    rows, n_obs = 3, len(br[0])
    rng = np.random.default_rng(seed)
    pl_d = _up(_block(rows, ncol, dtype, seed))
    H = _bank(J, K, seed, k0)
    obs_d, mag_d = _up(rng.normal(0.0, 1.0, n_obs)), _up(rng.normal(0.0, 0.3, rows))
    wts_d = _up(_weights(n_obs, seed)) if weighted else None
    br_d = tuple(_up(b) for b in br)
    want = _two_calls(gpu, pl_d, ncol, H, k0, obs_d, mag_d, wts_d, br_d)
    got = _bank_call(gpu, pl_d, ncol, H, k0, obs_d, mag_d, wts_d, br_d)
    label = (dtype.__name__, weighted, K, k0, ncol, J, n_obs)
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1]), label
    assert np.isfinite(want[0]).all(), label


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
def test_flagged_rows_nan_and_a_null_esum(gpu, offgrid):
    """Row 1 flagged: sse = +inf and esum = NaN for every response, whatever its PL.  One NaN element in row 2 inside the windows
    of the observed columns and one in row 0 beyond them: exactly the rows the two calls poison -- row 2 for every response (the
    responses share K and k0, and 0 * NaN is NaN: a zero-padded row of the bank is poisoned too), row 0 for none.  esum = NULL
    leaves sse as it is and writes nothing else."""
    import torch
    K, k0, n_obs, J, rows = 9, 4, 300, _jb(gpu) + 1, 4
    ncol = n_obs + k0 + 40
    pl = _block(rows, ncol, np.float64, 1)
    pl[2, 100] = np.nan
    pl[0, n_obs + k0 + 5] = np.nan                      # no observed column's window reaches it
    H = _bank(J, K, 1, k0)
    rng = np.random.default_rng(3)
    br_d = None
    if offgrid:
        br = _brackets(rng, n_obs, n_obs, "shuffled")    # brackets within the first n_obs convolved columns
        br_d = tuple(_up(b) for b in br)
    obs_d, mag_d = _up(rng.normal(0.0, 1.0, n_obs)), _up(rng.normal(0.0, 0.3, rows))
    status_d = _up(np.array([0, 1, 0, 0], dtype=np.int32))
    pl_d = _up(pl)
    want = _two_calls(gpu, pl_d, ncol, H, k0, obs_d, mag_d, None, br_d, status_d)
    got = _bank_call(gpu, pl_d, ncol, H, k0, obs_d, mag_d, None, br_d, status_d)
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])
    bad = np.zeros((J, rows), dtype=bool)
    bad[:, [1, 2]] = True
    assert np.array_equal(np.isposinf(got[0]), bad) and np.array_equal(np.isnan(got[1]), bad) and np.isfinite(got[0][~bad]).all()
    only_sse = _bank_call(gpu, pl_d, ncol, H, k0, obs_d, mag_d, None, br_d, status_d, with_esum=False)
    assert R.same_bits(only_sse[0], want[0])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the profile
def profile_ref(Pbank):
    """P[s] = the greatest Pbank[j][s], best[s] = the first j that attains it; NaN is never the greatest; all -inf or NaN: -1, -inf."""
    J, S = Pbank.shape
    P, best = np.full(S, -np.inf), np.full(S, -1, dtype=np.int32)
    for j in range(J):
        with np.errstate(invalid="ignore"):
            up = Pbank[j] > P
        P[up], best[up] = Pbank[j][up], j
    return best, P


@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("S", [1, 255, 257])
def test_profile_kernel_is_its_restatement(gpu, S, J):
    import torch
    rng = np.random.default_rng(S + J)
    Pb = -rng.uniform(0.0, 50.0, (J, S))
    Pb[:, ::5] = Pb[0, ::5]                                  # ties: the first response wins
    Pb[rng.random((J, S)) < 0.2] = -np.inf
    Pb[rng.random((J, S)) < 0.2] = np.nan
    Pb[:, S // 2] = -np.inf
    if S > 3:
        Pb[:, 3] = np.nan
        Pb[:, 1] = [np.nan, -np.inf, -3.0][:J]
    best_d = torch.full((S + PAD,), -9, dtype=torch.int32, device="cuda")
    P_d = torch.full((S + PAD,), R.CANARY, dtype=torch.float64, device="cuda")
    gpu.device.irf_bank_profile_device(_up(Pb), best_d[:S], P_d[:S])
    torch.cuda.synchronize()
    best, P = profile_ref(Pb)
    assert np.array_equal(best_d[:S].cpu().numpy(), best) and R.same_bits(P_d[:S].cpu().numpy(), P)
    assert bool(torch.all(best_d[S:] == -9)) and bool(torch.all(P_d[S:] == R.CANARY))
    assert best[S // 2] == -1 and P[S // 2] == -np.inf
    hb, hP = np.empty(S, dtype=np.int32), np.empty(S)
    gpu._abi.check(gpu._abi.lib().trpl_irf_bank_profile(Pb.ctypes.data, J, S, hb.ctypes.data, hP.ctypes.data))
    assert np.array_equal(hb, best) and R.same_bits(hP, P)   # the host form is the same expression


def test_refusals_that_need_a_device(gpu):
    import torch
    rows, ncol, K, k0, J, n = 3, 20, 5, 2, 2, 10
    f64 = torch.float64
    pl = torch.ones((rows, ncol), dtype=f64, device="cuda")
    H = torch.full((J, K), 0.2, dtype=f64, device="cuda")
    obs, mag = torch.zeros(n, dtype=f64, device="cuda"), torch.zeros(rows, dtype=f64, device="cuda")
    sse = torch.full((J, rows), R.CANARY, dtype=f64, device="cuda")
    call = gpu.device.loglik_irf_bank_device
    for bad in (lambda: call(pl.cpu(), H, k0, obs, mag, sse), lambda: call(pl, H.cpu(), k0, obs, mag, sse),
                lambda: call(pl, H[0], k0, obs, mag, sse), lambda: call(pl, H, k0, obs, mag, sse[:1]),
                lambda: call(pl, H, k0, obs, mag[:2], sse), lambda: call(pl, H, k0, obs, mag, sse.float()),
                lambda: call(pl, H, k0, obs, mag, sse, wts=obs[:3]), lambda: call(pl, H, k0, obs, mag, sse, esum=sse[:1]),
                lambda: call(pl, H, k0, obs, mag, sse, status=mag), lambda: call(pl.int(), H, k0, obs, mag, sse),
                lambda: call(pl, H, k0, obs, mag, sse, ncol=ncol + 1), lambda: call(pl, H, K, obs, mag, sse),
                lambda: call(pl, H, k0, torch.zeros(ncol - k0 + 1, dtype=f64, device="cuda"), mag, sse),
                lambda: call(pl, H, k0, obs, mag, sse, flags=gpu._abi.FLAG_NORMALIZE)):
        with pytest.raises((ValueError, gpu.TrplError)):
            bad()
    torch.cuda.synchronize()
    assert bool(torch.all(sse == R.CANARY))                 # a refused call launched nothing
    call(pl[:0], H, k0, obs, mag[:0], sse[:, :0].contiguous())                   # an empty block is a no-op
    prof = gpu.device.irf_bank_profile_device
    P, best = torch.zeros(rows, dtype=f64, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda")
    for bad in (lambda: prof(sse, best[:2], P), lambda: prof(sse, best, P.float()), lambda: prof(sse.cpu(), best, P), lambda: prof(sse[0], best, P)):
        with pytest.raises((ValueError, gpu.TrplError)):
            bad()


# ------------------------------------------------------------------------------------------------ the routes
L_, T_, S_ = 32, 64, 8


@functools.lru_cache(maxsize=None)
def _problem():
    """tests/test_gpu_irf.py's small case: Power_scan's first two curves at L = 32, T = 64, 8 samples; a bank of 2 widths x 3
    shifts; observations near the convolved curve of sample 0 under one response of the bank, on the grid and at unsorted times.
    The per-response likelihoods by irf.loglik are computed once and shared."""
    import trpl_amd as gpu
    w = gpu.workloads
    Time = T_ * 0.025
    dt = Time / T_
    ini, lens = w.power_scan(L_)
    ini, lens = np.ascontiguousarray(ini[:2]), lens[:2]
    X = w.samples(S_)
    bank = gpu.irf.gaussian_bank([0.1, 0.15], [-dt, 0.0, 0.4 * dt], dt)
    H, k0, _ = bank
    ncol_out = T_ + 1 - k0
    assert H.shape[0] == 6 and k0 >= 8 and ncol_out >= 40
    pls = []
    for c in range(2):
        mat = _up(X[:, :12])
        import torch
        pl = torch.empty((S_, T_ + 1), dtype=torch.float64, device="cuda")
        gpu.device.solve_pl_device(mat, lens[c], Time, L_, T_, _up(ini[c]), pl)
        pls.append(pl.cpu().numpy())
    rng = np.random.default_rng(2)
    sim_t = np.linspace(0, Time, T_ + 1)
    n_obs = (ncol_out, 30)
    obs = [np.log10(np.abs(R.convolve_ref(pls[c], H[4], k0)[0, :n_obs[c]])) + X[0, 12] + 0.05 * rng.normal(size=n_obs[c]) for c in range(2)]
    times = []
    for c in range(2):
        t = rng.uniform(0.0, sim_t[ncol_out - 1], n_obs[c])
        t[3], t[7], t[11] = sim_t[ncol_out - 1], 0.0, sim_t[5]
        times.append(t)
    wts = [_weights(n_obs[c], c) + 0.25 for c in range(2)]
    args = (X, ini, lens, Time, L_, T_, obs)
    per = {}
    for offgrid in (False, True):
        for weighted in (False, True):
            for f32 in (False, True):
                kw = dict(times=times if offgrid else None, weights=wts if weighted else None, pl_f32=f32)
                rows, sse = [], []
                for j in range(H.shape[0]):
                    info = {}
                    rows.append(gpu.irf.loglik(*args, (H[j], k0), info=info, **kw))
                    sse.append(info["sse"])
                per[(offgrid, weighted, f32)] = (np.array(rows), np.array(sse), kw)
    return dict(args=args, bank=bank, per=per, ncol_out=ncol_out)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
def test_loglik_bank_rows_are_loglik_and_the_profile_is_their_maximum(gpu, offgrid, weighted):
    p = _problem()
    H, k0, _ = p["bank"]
    for f32 in (False, True):
        want, want_sse, kw = p["per"][(offgrid, weighted, f32)]
        info = {}
        P = gpu.irf.loglik_bank(*p["args"], p["bank"], info=info, **kw)
        assert P.shape == (H.shape[0], S_) and R.same_bits(P, want), (offgrid, weighted, f32)
        assert R.same_bits(info["sse"], want_sse) and info["esum"].shape == want_sse.shape and np.isfinite(info["esum"]).all()
        assert info["ncol_out"] == p["ncol_out"] and not info["status"].any() and np.isfinite(P).all() and (P < 0).all()
        pinfo = {}
        LL = gpu.irf.loglik_profile(*p["args"], (H, k0), info=pinfo, **kw)
        assert R.same_bits(LL, want.max(axis=0)) and np.array_equal(pinfo["best"], want.argmax(axis=0))
        assert R.same_bits(pinfo["P"], want)
    if not offgrid and not weighted:
        assert pinfo["best"][0] == 4                         # the observations were made with response 4, at sample 0's PL
        small = gpu.irf.loglik_bank(*p["args"], p["bank"], block=3)               # blocks that do not divide S: irf.loglik's bound
        assert np.allclose(small, p["per"][(False, False, False)][0], rtol=1e-7, atol=1e-9)


def test_mcmc_runs_on_the_profile_and_reproduces_itself(gpu):
    p = _problem()
    sm = gpu.sampler
    lo, hi, lg = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS, sm.DEFAULT_DO_LOG
    X, ini, lens, Time, L, T, obs = p["args"]
    loglik = functools.partial(gpu.irf.loglik_profile, init_params=ini, lengths=lens, Time=Time, L=L, T=T, obs=obs, bank=p["bank"])
    X0 = np.ascontiguousarray(gpu.workloads.samples(16, seed=29))
    LL0 = loglik(X0)
    assert R.same_bits(LL0, gpu.irf.loglik_bank(X0, ini, lens, Time, L, T, obs, p["bank"]).max(axis=0))
    runs = [gpu.mcmc.run(loglik, X0, LL0, lo, hi, lg, sweeps=4, seed=5, bounds="fold") for _ in range(2)]
    assert R.same_bits(runs[0].X, runs[1].X) and R.same_bits(runs[0].LL, runs[1].LL) and np.isfinite(runs[0].LL).all()
    # every kept LL is the profile at its state; a sweep scores half the chains per launch, and the FAST steppers agree between
    # launch sizes to 1e-9 in PL -- inside 1e-7 of sse (tests/test_gpu_irf.py), and a maximum moves no more than its arguments
    assert np.allclose(runs[0].LL[-1], loglik(np.ascontiguousarray(runs[0].X[-1])), rtol=1e-6, atol=1e-9)
