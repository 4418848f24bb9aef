"""The autocovariance sums on the device (trpl_mcmc_autocov*, csrc/mcmc.hip) and Chains.ess against tests/mcmc_ess_ref.py.

mean, s and pooled are BIT FOR BIT the sequential loops (a NaN matches a NaN), through the _dev forms and the host-buffer forms, at
the shapes where the register-blocked kernel can go wrong: fewer lags than a tile, exactly a tile, one more, several tiles and an
edge tile, as many lags as steps (the last lags have one term), ranges shorter than a tile, one column, a block of columns less
one, exactly one and one more.  Everything of H outside the rows [t0, t1) and the columns [0, Q) is NaN, so a read outside poisons a
sum; everything around mean, s and pooled is a sentinel that must stay.  Columns are independent and a sum over fewer lags is a
prefix, so the restatement is made once per range length, at the most lags and columns, and sliced."""
import numpy as np
import pytest

import mcmc_ess_ref as er
import mcmc_ref as mr
from test_gpu_mcmc import _cuda, _same_bits

pytestmark = pytest.mark.gpu
QS = (1, 255, 256, 257)
QMAX, T0, TAIL, SENTINEL = max(QS), 2, 3, -7.0
NAN_COL, ZERO_COL = 254, 1                                        # a column with one NaN (from Q = 255 on), a column of -0.0


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


@pytest.fixture(scope="module")
def tile(gpu):
    return int(gpu._abi.lib().trpl_mcmc_autocov_tile())


def _data(m):
    """(m, QMAX): columns of different scale and offset, -0.0 sprinkled in column 0, column ZERO_COL all -0.0, one NaN in NAN_COL."""
    rng = np.random.default_rng(m)
    x = rng.normal(size=(m, QMAX)) * 10.0 ** rng.integers(-3, 4, QMAX) + rng.normal(size=QMAX)
    x[::3, 0] = -0.0
    x[:, ZERO_COL] = -0.0
    x[m // 2, NAN_COL] = np.nan
    return x


def _history(x, Q):
    """H (T0 + m + TAIL, Q + 3), NaN wherever the call may not read."""
    m = x.shape[0]
    H = np.full((T0 + m + TAIL, Q + 3), np.nan)
    H[T0:T0 + m, :Q] = x[:, :Q]
    return H


def _autocov_dev(torch_dev, H, t0, t1, L, Q):
    """(mean, s) of the _dev form with lds = Q + 2, written into the middle of sentinel buffers that are checked."""
    torch, dev = torch_dev
    mean = torch.full((Q + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    s = torch.full((L + 2, Q + 2), SENTINEL, dtype=torch.float64, device="cuda")
    dev.mcmc_autocov_device(_cuda(torch, H), t0, t1, mean[1:1 + Q], s[1:1 + L], Q=Q)
    torch.cuda.synchronize()
    mean, s = mean.cpu().numpy(), s.cpu().numpy()
    assert mean[0] == SENTINEL and mean[-1] == SENTINEL
    assert np.all(s[0] == SENTINEL) and np.all(s[-1] == SENTINEL) and np.all(s[:, Q:] == SENTINEL)
    return mean[1:1 + Q], s[1:1 + L, :Q]


@pytest.mark.parametrize("m", (1, 2, "tile", 97))
def test_autocov_is_the_loop_bit_for_bit(gpu, torch_dev, tile, m):
    torch, dev = torch_dev
    m = tile if m == "tile" else m
    x = _data(m)
    want_mean, want_s = er.autocov(x, 0, m, m)                   # every lag, every column: once
    assert np.isnan(want_s[:, NAN_COL]).all() and np.isfinite(np.delete(want_s, NAN_COL, axis=1)).all()
    assert np.all(want_s[:, ZERO_COL] == 0.0) and not np.signbit(want_s[:, ZERO_COL]).any()
    lags = sorted({L for L in (1, tile - 1, tile, tile + 1, 2 * tile + 1, m) if 1 <= L <= m})
    for Q in QS:
        H = _history(x, Q)
        cm = torch.full((Q,), SENTINEL, dtype=torch.float64, device="cuda")
        cv = torch.full((Q,), SENTINEL, dtype=torch.float64, device="cuda")
        dev.mcmc_chain_stats_device(_cuda(torch, H), T0, T0 + m, cm, cv, Q=Q)
        torch.cuda.synchronize()
        for L in lags:
            mean, s = _autocov_dev(torch_dev, H, T0, T0 + m, L, Q)
            assert _same_bits(mean, want_mean[:Q]), (m, Q, L)
            assert _same_bits(s, want_s[:L, :Q]), (m, Q, L, np.argwhere(s != want_s[:L, :Q])[:4])
            assert _same_bits(mean, cm.cpu().numpy()) and _same_bits(s[0], cv.cpu().numpy())          # chain_stats' mean and m2
            hm, hs = gpu.mcmc.autocov(H, L, T0, T0 + m, Q=Q)    # the host-buffer form: the range only, s compact
            assert hs.shape == (L, Q) and _same_bits(hm, mean) and _same_bits(hs, s)
        if Q >= 255:                                             # the NaN poisons its column and no other
            assert np.isnan(s[:, NAN_COL]).all() and np.isfinite(np.delete(s, NAN_COL, axis=1)).all()


def test_autocov_of_a_range_inside_a_longer_history(gpu, torch_dev, tile):
    """t0 > 0 and t1 < n with finite rows around the range: the sums are those of the range alone."""
    rng = np.random.default_rng(3)
    n, Q, t0, t1 = 40, 5, 7, 30
    H = rng.normal(size=(n, Q + 1))
    for L in (1, tile + 1, t1 - t0):
        mean, s = _autocov_dev(torch_dev, H, t0, t1, L, Q)
        want_mean, want_s = er.autocov(H, t0, t1, L, Q)
        assert _same_bits(mean, want_mean) and _same_bits(s, want_s)
        assert _same_bits(s, er.autocov(H[t0:t1], 0, t1 - t0, L, Q)[1])
        hm, hs = gpu.mcmc.autocov(H, L, t0, t1, Q=Q)
        assert _same_bits(hm, mean) and _same_bits(hs, s)
    full = gpu.mcmc.autocov(H, 3)                                # the defaults: every column, every step
    assert _same_bits(full[1], er.autocov(H, 0, n, 3)[1])


@pytest.mark.parametrize("M", (1, 2, 7, 16, 33))                 # the kernel adds 16 sequences per round of loads: none, one, two and a rest
def test_pool_is_the_ascending_sum_over_the_sequences(gpu, torch_dev, M):
    torch, dev = torch_dev
    rng = np.random.default_rng(M)
    for A in (1, 3, 16):
        for L in (1, 5, 300):                                    # 300 lags x 16 columns: more than one block of sums
            Q = M * A
            s = np.full((L, Q + 2), np.nan)                      # the padding holds NaN: nothing may read it
            s[:, :Q] = rng.normal(size=(L, Q)) * 10.0 ** rng.integers(-6, 7, (L, Q))
            if L > 1 and M > 1:
                s[1, A] = np.nan                                 # sequence 1, column 0 of lag 1
            want = er.pool(s, M, A)
            pooled = torch.full((L + 2, A), SENTINEL, dtype=torch.float64, device="cuda")
            dev.mcmc_autocov_pool_device(_cuda(torch, s), M, A, pooled[1:1 + L])
            torch.cuda.synchronize()
            pooled = pooled.cpu().numpy()
            assert np.all(pooled[0] == SENTINEL) and np.all(pooled[-1] == SENTINEL)
            assert _same_bits(pooled[1:1 + L], want), (M, A, L)
            assert np.isnan(want).sum() == (1 if L > 1 and M > 1 else 0)
            assert _same_bits(gpu.mcmc.autocov_pool(s, M, A), want)
            if M == 1:
                assert _same_bits(want, 0.0 + s[:, :Q])


def _chains_call(gpu, H, M, A, t0, t1, L):
    lib, A_ = gpu._abi.lib(), gpu._abi
    mean, m2, pooled = np.full(M * A + 1, SENTINEL), np.full(M * A + 1, SENTINEL), np.full(L * A + 1, SENTINEL)
    A_.check(lib.trpl_mcmc_autocov_chains(A_.ptr(H), H.shape[0], H.shape[1], M, A, t0, t1, L, A_.ptr(mean), A_.ptr(m2), A_.ptr(pooled), 0,
                                          None))
    assert mean[-1] == SENTINEL and m2[-1] == SENTINEL and pooled[-1] == SENTINEL
    return mean[:-1], m2[:-1], pooled[:-1].reshape(L, A)


def test_the_fused_call_is_the_two_calls(gpu, tile):
    rng = np.random.default_rng(9)
    for M, A, m, L in ((1, 1, 2, 2), (7, 3, 19, tile + 1), (40, 16, 33, 33), (2, 16, 12, 1)):
        Q, t0 = M * A, 3
        H = np.full((t0 + m + 2, Q + 1), np.nan)
        H[t0:t0 + m, :Q] = rng.normal(size=(m, Q)) + rng.normal(size=Q)
        mean, m2, pooled = _chains_call(gpu, H, M, A, t0, t0 + m, L)
        want_mean, s = gpu.mcmc.autocov(H, L, t0, t0 + m, Q=Q)
        assert _same_bits(mean, want_mean) and _same_bits(m2, s[0]) and _same_bits(pooled, gpu.mcmc.autocov_pool(s, M, A))
        ref_mean, ref_s = er.autocov(H, t0, t0 + m, L, Q)
        assert _same_bits(mean, ref_mean) and _same_bits(m2, ref_s[0]) and _same_bits(pooled, er.pool(ref_s, M, A))


def _same_estimate(got, want):
    (ess, info), (want_ess, ref) = got, want
    assert np.array_equal(ess, want_ess), (ess, want_ess)
    for key in ("tau", "var_plus", "rho", "K", "truncated"):
        assert np.array_equal(info[key], ref[key]), key
    assert np.all(np.isfinite(ess)) and np.all(ess > 0.0)


def test_chains_ess_on_a_toy_run(gpu):
    """mcmc.run on the 3-D Gaussian, 8 chains, 64 sweeps: Chains.ess is the restatement on the same history, bit for bit -- for the
    unit coordinates, for LL as a column, after a burn-in, with fewer lags, and for a rung of a tempered run."""
    loglik = mr.toy(0.0)[0]
    lo, hi, lg = mr.CUBE
    U0 = mr.toy_start(8, 4)
    ch = gpu.mcmc.run(loglik, U0, loglik(U0), lo, hi, lg, sweeps=64, seed=4, scale=0.02, U0=U0)
    assert ch.U.shape == (64, 8, 3)
    got = ch.ess()
    _same_estimate(got, er.split_ess(ch.U, 0, 32))
    assert got[0].shape == (3,) and got[1]["rho"].shape == (32, 3) and np.all(got[0] < 8 * 64)
    _same_estimate(ch.ess(burn=5, max_lag=11), er.split_ess(ch.U, 5, 11))        # n2 = 29: the last of the 64 sweeps is left out
    _same_estimate(ch.ess(values=ch.LL[..., None]), er.split_ess(ch.LL[..., None], 0, 32))
    _same_estimate(ch.ess(values=ch.X, max_lag=9), er.split_ess(ch.X, 0, 9))
    assert np.array_equal(ch.autocorr(), got[1]["rho"]) and np.array_equal(ch.mcse(), np.sqrt(got[1]["var_plus"] / got[0]))
    print("toy: ess %s of %d, tau %s, truncated %s, R-hat %s" % (np.round(got[0], 1), 8 * 64, np.round(got[1]["tau"], 2),
                                                                 got[1]["truncated"], np.round(ch.rhat(), 3)))
    t = gpu.mcmc.run_tempered(loglik, U0, loglik(U0), lo, hi, lg, [1.0, 4.0], sweeps=64, seed=4, scale=0.02, U0=U0)
    for k in (0, 1):
        _same_estimate(t.rung(k).ess(), er.split_ess(t.rung(k).U, 0, 32))
