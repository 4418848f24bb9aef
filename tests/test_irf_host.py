"""The instrument-response convolution without a device: the NumPy restatement of the definition (tests/irf_ref.py) against
np.convolve inside the rounding bound of K ordered additions, its exact cases (one tap, a unit tap), the IRF builders
trpl_amd.irf.gaussian / from_samples, every refusal of trpl_convolve_irf[_dev] through the C ABI with the message naming the
argument, and the ValueErrors of irf.loglik and of gpu_info["irf"].  No compute call is made here."""
import ctypes
import math

import numpy as np
import pytest

import abi_header as H
import irf_ref as R


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_is_the_convolution_inside_the_rounding_bound(dtype):
    """Row by row against np.convolve(row, h)[k0 : k0 + ncol_out].  Both are sums of the same at most K products in fp64; an
    ordered sum of K terms is within (K - 1) u sum|terms| of the exact one to first order (u = 2^-53, each product adds one
    more u), so two such sums differ by at most K 2^-52 convolve(|row|, |h|) -- derived, not measured.  The float32 output
    adds one rounding of the sum: half a float32 ulp of the result."""
    for K, k0, ncol, rows in ((1, 0, 5, 2), (3, 1, 17, 3), (33, 16, 100, 4), (65, 0, 70, 2), (65, 64, 70, 2), (40, 7, 12, 3)):
        pl = R.block(rows, ncol, dtype)
        h = R.taps(K, k0)
        got = R.convolve_ref(pl, h, k0, ncol=ncol)
        ncol_out = ncol - k0
        assert got.shape == (rows, ncol_out) and got.dtype == dtype
        for r in range(rows):
            row = pl[r, :ncol].astype(np.float64)
            want = np.convolve(row, h)[k0:k0 + ncol_out]
            bound = K * 2.0 ** -52 * np.convolve(np.abs(row), np.abs(h))[k0:k0 + ncol_out]
            if dtype == np.float32:
                bound = bound + 2.0 ** -24 * np.abs(want) + float(np.finfo(np.float32).smallest_subnormal)
            assert np.all(np.abs(got[r].astype(np.float64) - want) <= bound), (K, k0, ncol, r)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_tap_returns_the_inputs_bits(dtype):
    pl = R.block(3, 40, dtype)
    assert R.same_bits(R.convolve_ref(pl, [1.0], 0, ncol=40), pl[:, :40])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_unit_tap_shifts_exactly(dtype):
    """A unit tap at index d beside zero taps: out[j] = pl[j + k0 - d], and +0.0 where that column is negative (every term that
    is left is a product with a zero tap, +-0.0, added to +0.0).  Finite rows: 0 * x is a zero."""
    ncol, K = 30, 9
    pl = R.block(2, ncol, dtype)
    for k0 in (0, 4, 8):
        for d in (0, 3, 8):
            h = np.zeros(K)
            h[d] = 1.0
            got = R.convolve_ref(pl, h, k0, ncol=ncol)
            want = np.zeros((2, ncol - k0), dtype=dtype)
            s = k0 - d                                     # out[j] = pl[j + s]
            j = np.arange(ncol - k0)
            ok = j + s >= 0
            want[:, ok] = pl[:, :ncol][:, j[ok] + s]
            assert R.same_bits(got, want), (k0, d)
            assert not np.signbit(got[:, ~ok]).any()


def test_nan_poisons_exactly_its_window():
    ncol, K, k0 = 40, 5, 2
    pl = np.array(R.block(2, ncol, np.float64))
    pl[1, 20] = np.nan
    h = R.taps(K, 1)
    h[3] = 0.0                                             # 0 * NaN is NaN: a zero tap does not shield its column
    got = R.convolve_ref(pl, h, k0, ncol=ncol)
    want = np.zeros((2, ncol - k0), dtype=bool)
    want[1, 20 - k0:20 - k0 + K] = True                    # j + k0 - k == 20 for k = 0 .. K-1
    assert np.array_equal(np.isnan(got), want)


# ------------------------------------------------------------------------------------------------ the builders
def test_gaussian_taps(trpl):
    irf = trpl.irf
    for fwhm, dt, cut in ((0.5, 0.025, 1e-12), (0.3, 0.25, 1e-12), (1.0, 0.025, 1e-6), (0.01, 0.25, 1e-12)):
        h, k0 = irf.gaussian(fwhm, dt, rel_cut=cut)
        K = len(h)
        m = int(math.floor(fwhm / dt * math.sqrt(math.log(1.0 / cut) / (4.0 * math.log(2.0)))))
        assert K == 2 * k0 + 1 and abs(k0 - m) <= 1 and h.dtype == np.float64
        assert np.array_equal(h, h[::-1])                                  # symmetric about k0, bit for bit
        assert abs(math.fsum(h) - 1.0) <= 2.0 ** -52                       # one ulp of 1
        assert int(np.argmax(h)) == k0 and np.all(h > 0)
        g = lambda n: math.exp(-4.0 * math.log(2.0) * (n * dt / fwhm) ** 2)
        assert g(k0) >= cut > g(k0 + 1)                                    # truncated where the value falls below rel_cut of the peak
        rel = h / h[k0]
        assert np.allclose(rel, [g(n - k0) for n in range(K)], rtol=1e-15, atol=0)
        if k0 >= 1 and fwhm / (2 * dt) == int(fwhm / (2 * dt)):            # the half-maximum sits on a node
            assert abs(rel[k0 + int(fwhm / (2 * dt))] - 0.5) < 1e-15
    assert trpl.irf.gaussian(0.01, 0.25)[0].tolist() == [1.0]              # narrower than the grid: the identity
    cap = trpl._abi.lib().trpl_irf_max_taps()
    assert cap == trpl._abi.IRF_MAX_TAPS == trpl.irf.max_taps() == 1024
    with pytest.raises(ValueError, match="trpl_irf_max_taps"):
        irf.gaussian(200.0, 0.25)                                          # ~ 5100 taps above 1e-12
    h, k0 = irf.gaussian(30.0, 0.25, rel_cut=1e-3)
    assert len(h) <= cap
    for bad in (dict(fwhm_ns=0.0, dt_ns=0.1), dict(fwhm_ns=1.0, dt_ns=-1.0), dict(fwhm_ns=1.0, dt_ns=0.1, rel_cut=1.0)):
        with pytest.raises(ValueError):
            irf.gaussian(**bad)


def test_from_samples(trpl):
    irf = trpl.irf
    # a triangle on a 0.1 ns raster with a background of 5 counts, peak at t = 1.03 ns, resampled at 0.05 ns
    t = 0.03 + 0.1 * np.arange(30)
    counts = 5.0 + np.clip(100.0 - 400.0 * np.abs(t - 1.03), 0.0, None)
    counts[2] = 3.0                                                        # below the background: clipped at 0
    h, k0 = irf.from_samples(t, counts, 0.05, background=5.0)
    assert int(np.argmax(h)) == k0 and abs(math.fsum(h) - 1.0) <= 2.0 ** -52
    assert h[0] > 0 and h[-1] > 0 and np.all(h >= 0)                       # leading and trailing zeros are dropped
    # the raster samples above the background are 20, 60, 100, 60, 20 at 0.83 .. 1.23 ns, zero at 0.73 and 1.33: linear
    # interpolation puts 10, 40, 80 on the nodes half way, so the nodes 1.03 + 0.05 n that are not zero are n = -5 .. 5
    assert len(h) == 11 and k0 == 5
    want = np.array([10.0, 20.0, 40.0, 60.0, 80.0, 100.0, 80.0, 60.0, 40.0, 20.0, 10.0])
    assert np.allclose(h, want / want.sum(), rtol=1e-12)
    # samples already on the grid come back as they are, normalised
    c2 = np.array([0.0, 0.0, 1.0, 4.0, 2.0, 1.0, 0.0])
    h2, k2 = irf.from_samples(0.25 * np.arange(7), c2, 0.25)
    assert k2 == 1 and np.allclose(h2, c2[2:6] / 8.0, rtol=1e-15)
    with pytest.raises(ValueError):
        irf.from_samples([0.0, 1.0], [1.0, 1.0], 0.25, background=2.0)    # nothing above the background
    with pytest.raises(ValueError):
        irf.from_samples([0.0, 0.0], [1.0, 2.0], 0.25)                    # times not increasing
    with pytest.raises(ValueError, match="trpl_irf_max_taps"):
        irf.from_samples(np.arange(3000.0), np.ones(3000), 1.0)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_kernel_agree_on_the_constants(trpl):
    define = H.defines().__getitem__
    A = trpl._abi
    assert (define("TRPL_IRF_MAX_TAPS"), define("TRPL_IRF_TILE_COLS"), define("TRPL_IRF_TILE_ROWS"), define("TRPL_IRF_GRID_CAP")) \
        == (A.IRF_MAX_TAPS, A.IRF_TILE_COLS, A.IRF_TILE_ROWS, A.IRF_GRID_CAP)
    for name in ("trpl_irf_max_taps", "trpl_convolve_irf_dev", "trpl_convolve_irf"):
        assert name in A.SIGNATURES and hasattr(A.lib(), name)
    assert A.lib().trpl_abi_version() == 5                                 # additive: the version stays


def test_every_refusal_names_its_argument_without_a_device(trpl):
    lib, E = trpl._abi.lib(), trpl._abi.ERR_ARG
    rows, ncol, K, k0 = 3, 10, 4, 1
    pl = np.ones((rows, ncol))
    h = np.full(K, 0.25)
    out = np.full((rows, ncol - k0), R.CANARY)
    base = dict(pl=pl.ctypes.data, elem=8, rows=rows, ncol=ncol, ld=ncol, h=h.ctypes.data, K=K, k0=k0, out=out.ctypes.data,
                out_ld=ncol - k0)

    def dev(**kw):
        a = dict(base, **kw)
        return lib.trpl_convolve_irf_dev(a["pl"], a["elem"], a["rows"], a["ncol"], a["ld"], a["h"], a["K"], a["k0"], a["out"],
                                         a["out_ld"], None)

    def host(**kw):
        a = dict(base, **kw)
        sec = ctypes.c_double(-1.0)
        rc = lib.trpl_convolve_irf(a["pl"], a["elem"], a["rows"], a["ncol"], a["ld"], a["h"], a["K"], a["k0"], a["out"],
                                   a["out_ld"], 0, ctypes.byref(sec))
        assert sec.value == 0.0
        return rc

    cases = ((dict(elem=2), b"elem_bytes"), (dict(elem=16), b"elem_bytes"), (dict(rows=-1), b"rows"), (dict(ncol=0), b"ncol"),
             (dict(ld=ncol - 1), b"ld="), (dict(K=0), b"K="), (dict(K=trpl._abi.IRF_MAX_TAPS + 1), b"TRPL_IRF_MAX_TAPS"),
             (dict(k0=-1), b"k0"), (dict(k0=K), b"k0"), (dict(ncol=3, ld=3, K=4, k0=3), b"k0"),
             (dict(out_ld=ncol - k0 - 1), b"out_ld"), (dict(pl=None), b"pl is NULL"), (dict(h=None), b"h is NULL"),
             (dict(out=None), b"out is NULL"), (dict(out=pl.ctypes.data, out_ld=ncol), b"out must not be pl"))
    for call in (dev, host):
        for kw, word in cases:
            assert call(**kw) == E and word in lib.trpl_last_error(), (call.__name__, kw, lib.trpl_last_error())
    msg = lambda: lib.trpl_last_error()
    assert dev(ncol=3, ld=3, K=4, k0=3) == E and b"ncol" in msg() and b"no output column" in msg()
    # the host form alone reads the taps: a tap that is not finite is refused, its index named
    for bad in (np.nan, np.inf, -np.inf):
        hb = h.copy()
        hb[2] = bad
        assert host(h=hb.ctypes.data) == E and b"h[2]" in msg() and b"finite" in msg()
    # an empty block is a successful no-op in both forms, NULL pointers included
    assert dev(rows=0) == 0 and host(rows=0) == 0
    assert dev(rows=0, pl=None, h=None, out=None) == 0 and host(rows=0, pl=None, h=None, out=None) == 0
    assert np.all(out == R.CANARY) and np.all(pl == 1.0)                   # no refused call wrote anything
    with pytest.raises(trpl.TrplError, match="k0"):
        trpl.irf.convolve(pl, h, K)
    with pytest.raises(ValueError):
        trpl.irf.convolve(np.ones(4), h, 0)
    with pytest.raises(ValueError):
        trpl.irf.convolve(pl.astype(np.int32), h, 0)


# ------------------------------------------------------------------------------------------------ the Python layer's own refusals
def _problem(trpl, S=4, L=32, T=64):
    w = trpl.workloads
    ini, lens = w.power_scan(L)
    Time = T * 0.025
    return dict(X=w.samples(S), init_params=ini[:2], lengths=lens[:2], Time=Time, L=L, T=T)


def test_loglik_refuses_before_it_touches_a_device(trpl):
    p = _problem(trpl)
    T, Time = p["T"], p["Time"]
    h, k0 = trpl.irf.gaussian(0.2, Time / T)
    assert k0 >= 3
    ncol_out = T + 1 - k0
    obs_ok = [np.zeros(ncol_out), np.zeros(5)]
    with pytest.raises(ValueError, match="T \\+ 1 - k0"):                   # one observation more than the convolved curve has columns
        trpl.irf.loglik(obs=[np.zeros(ncol_out + 1), np.zeros(5)], irf=(h, k0), **p)
    t_last = trpl.irf.last_time(Time, T, k0)
    assert t_last == Time * (T - k0) / T
    late = [np.array([0.0, 0.5 * t_last]), np.array([0.1, np.nextafter(np.linspace(0, Time, T + 1)[T - k0], np.inf)])]
    with pytest.raises(ValueError, match="convolved window"):
        trpl.irf.loglik(obs=[np.zeros(2), np.zeros(2)], times=late, irf=(h, k0), **p)
    with pytest.raises(ValueError, match="self-normalisation"):
        trpl.irf.loglik(obs=obs_ok, irf=(h, k0), normalize=True, **p)
    for bad in ((h, len(h)), (h, -1), (np.zeros(0), 0), (np.ones(trpl._abi.IRF_MAX_TAPS + 1), 0), ([1.0, np.nan], 0), h):
        with pytest.raises(ValueError, match="irf"):
            trpl.irf.loglik(obs=obs_ok, irf=bad, **p)
    with pytest.raises(ValueError, match="weights"):
        trpl.irf.loglik(obs=obs_ok, irf=(h, k0), weights=[np.ones(ncol_out), np.ones(4)], **p)
    info = {}
    P = trpl.irf.loglik(obs=obs_ok, irf=(h, k0), info=info, **dict(p, X=np.zeros((0, 13))))     # no sample: no device
    assert P.shape == (0,) and info["ncol_out"] == ncol_out and info["sse"].shape == (2, 0)


def test_simulate_refuses_what_the_irf_does_not_combine_with(trpl):
    p = _problem(trpl)
    T, Time, L = p["T"], p["Time"], p["L"]
    h, k0 = trpl.irf.gaussian(0.2, Time / T)
    sim_t = np.linspace(0, Time, T + 1)
    n = T + 1 - k0

    def run(gpu_info, normalize=False, times=None):
        t = sim_t[:n] if times is None else times
        e_data = [([t, t], [np.zeros(len(t))] * 2, [np.ones(len(t))] * 2)]
        info = dict(sims_per_gpu=8, num_gpus=1, fused=True, irf=(h, k0))
        info.update(gpu_info)
        Pm = np.zeros((1, len(p["X"])))
        trpl.simulate(trpl.pvSim, e_data, Pm, p["X"], [None], [None], 2, [list(p["lengths"]), Time, L, T, 1, 0, 7, 10000],
                      p["init_params"], dict(log_pl=True, self_normalize=normalize), info, 0, np.zeros(1), np.zeros(1), np.zeros(1))

    for kw, word in ((dict(fused=False), "unfused"), (dict(devices="all"), "devices"), (dict(devices=[0]), "devices"),
                     (dict(cut_margin=10.0), "cut_margin")):
        with pytest.raises(ValueError, match=r"gpu_info\['irf'\].*%s" % word):
            run(kw)
    with pytest.raises(ValueError, match=r"gpu_info\['irf'\].*self_normalize"):
        run({}, normalize=True)
    with pytest.raises(ValueError, match=r"gpu_info\['irf'\].*last convolved column"):
        run({}, times=sim_t[:n + 1])
    with pytest.raises(ValueError, match="irf"):
        run(dict(irf=(h, len(h))))
    with pytest.raises(ValueError, match="irf"):
        trpl.posterior_predictive(p["X"], np.ones(4), p["init_params"], [list(p["lengths"]), Time, L, T, 1], irf=(h, k0), normalize=True)
