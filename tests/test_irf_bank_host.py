"""The bank of instrument responses without a device: the builders trpl_amd.irf.gaussian_bank / shift_bank, the profile over a
bank (trpl_irf_bank_profile is plain host code) against its NumPy restatement, every refusal of trpl_loglik_irf_bank[_dev] and
trpl_irf_bank_profile[_dev] through the C ABI with the message naming the argument, the ValueErrors of irf.loglik_bank /
irf.loglik_profile, and the ABI.  No compute call touches a device here."""
import ctypes
import math

import numpy as np
import pytest

import abi_header as H
import irf_ref as R

DT = 0.03125                                                 # 2^-5: shift / dt is exact for shifts that are multiples of it


# ------------------------------------------------------------------------------------------------ the builders
def test_gaussian_bank(trpl):
    irf = trpl.irf
    fw, sh = [0.3, 0.5], [-2 * DT, 0.0, 0.01, 3 * DT]
    H, k0, table = irf.gaussian_bank(fw, sh, DT)
    J, K = H.shape
    assert J == 8 and K == 2 * k0 + 1 and H.dtype == np.float64 and H.flags.c_contiguous
    assert table.tolist() == [[f, s] for f in fw for s in sh]                     # width-major
    for j in range(J):
        assert abs(math.fsum(H[j]) - 1.0) <= 2.0 ** -52                           # one ulp of 1
        assert np.all(H[j] >= 0.0)
    for w, f in enumerate(fw):
        h, m = irf.gaussian(f, DT)
        pad = lambda d: np.concatenate([np.zeros(k0 - m + d), h, np.zeros(k0 - m - d)])
        assert R.same_bits(H[4 * w + 1], pad(0))                                  # shift 0: gaussian(), zero-padded
        assert R.same_bits(H[4 * w + 0], pad(-2)) and R.same_bits(H[4 * w + 3], pad(3))       # whole steps: the taps moved
        peak = int(np.argmax(H[4 * w + 2]))
        assert peak == k0 and H[4 * w + 2][k0 + 1] > H[4 * w + 2][k0 - 1]         # a positive shift leans later
    # K and k0 hold the widest response at the largest |shift|, and no more: some row reaches the first or the last tap
    assert (H[:, 0] > 0).any() or (H[:, -1] > 0).any()
    wide, m_wide = irf.gaussian(0.5, DT)
    assert k0 == m_wide + 3
    # one width, no shift: the bank is gaussian() itself
    H1, k1, t1 = irf.gaussian_bank(0.3, 0.0, DT)
    h, m = irf.gaussian(0.3, DT)
    assert k1 == m and R.same_bits(H1[0], h) and t1.tolist() == [[0.3, 0.0]]
    # rel_cut reaches the taps
    Hc, kc, _ = irf.gaussian_bank([0.3], [0.0], DT, rel_cut=1e-3)
    assert kc < k1 and R.same_bits(Hc[0], irf.gaussian(0.3, DT, rel_cut=1e-3)[0])
    cap, taps = trpl._abi.IRF_BANK_MAX_RESPONSES, trpl._abi.IRF_MAX_TAPS
    assert irf.bank_cap() == cap
    with pytest.raises(ValueError, match="trpl_irf_bank_max_responses"):
        irf.gaussian_bank([0.3], np.linspace(-0.1, 0.1, cap + 1), DT)
    with pytest.raises(ValueError, match="trpl_irf_max_taps"):
        irf.gaussian_bank([0.3, 200.0], [0.0], 0.25)
    with pytest.raises(ValueError, match="trpl_irf_max_taps"):
        irf.gaussian_bank([0.3], [0.0, taps * DT], DT)                            # the shift alone needs more taps
    for bad in (dict(fwhms_ns=[0.0], shifts_ns=[0.0], dt_ns=DT), dict(fwhms_ns=[0.3], shifts_ns=[np.nan], dt_ns=DT),
                dict(fwhms_ns=[], shifts_ns=[0.0], dt_ns=DT), dict(fwhms_ns=[0.3], shifts_ns=[], dt_ns=DT),
                dict(fwhms_ns=[0.3], shifts_ns=[0.0], dt_ns=0.0), dict(fwhms_ns=[0.3], shifts_ns=[0.0], dt_ns=DT, rel_cut=1.0)):
        with pytest.raises(ValueError):
            irf.gaussian_bank(**bad)


def test_shift_bank(trpl):
    irf = trpl.irf
    h = np.array([0.1, 0.5, 0.25, 0.15])
    H, k0, table = irf.shift_bank((h, 1), [-2 * DT, 0.0, 0.5 * DT, 3 * DT, -0.25 * DT], DT)
    assert H.shape == (5, 4 + 2 + 3) and k0 == 1 + 2 and table.tolist() == [-2 * DT, 0.0, 0.5 * DT, 3 * DT, -0.25 * DT]
    z = np.zeros
    assert R.same_bits(H[0], np.concatenate([h, z(5)]))                           # whole steps move the taps exactly
    assert R.same_bits(H[1], np.concatenate([z(2), h, z(3)]))
    assert R.same_bits(H[3], np.concatenate([z(5), h]))
    assert R.same_bits(H[2], np.concatenate([z(2), 0.5 * h, z(3)]) + np.concatenate([z(3), 0.5 * h, z(2)]))    # half a step: the mean of neighbours
    assert np.allclose(H[2][2:7], [0.05, 0.3, 0.375, 0.2, 0.075], rtol=1e-15)
    want = np.concatenate([z(1), 0.25 * h, z(4)]) + np.concatenate([z(2), 0.75 * h, z(3)])  # -0.25 = -1 + 0.75
    assert R.same_bits(H[4], want)
    for j in range(5):
        assert abs(math.fsum(H[j]) - 1.0) <= 4 * 2.0 ** -52
    # a positive shift moves the convolved curve later
    pl = np.zeros((1, 12))
    pl[0, 4] = 1.0
    assert int(np.argmax(R.convolve_ref(pl, H[3], k0))) == int(np.argmax(R.convolve_ref(pl, H[1], k0))) + 3
    same = irf.shift_bank((h, 1), [0.0], DT)
    assert R.same_bits(same[0][0], h) and same[1] == 1
    with pytest.raises(ValueError, match="trpl_irf_max_taps"):
        irf.shift_bank((h, 1), [trpl._abi.IRF_MAX_TAPS * DT], DT)
    with pytest.raises(ValueError, match="trpl_irf_bank_max_responses"):
        irf.shift_bank((h, 1), np.zeros(trpl._abi.IRF_BANK_MAX_RESPONSES + 1), DT)
    for bad in (lambda: irf.shift_bank((h, 4), [0.0], DT), lambda: irf.shift_bank((h, 1), [np.inf], DT),
                lambda: irf.shift_bank((h, 1), [], DT), lambda: irf.shift_bank((h, 1), [0.0], 0.0), lambda: irf.shift_bank(h, [0.0], DT)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ the profile
def _profile(trpl, Pb):
    J, S = Pb.shape
    best, P = np.full(S + 2, -9, dtype=np.int32), np.full(S + 2, R.CANARY)
    trpl._abi.check(trpl._abi.lib().trpl_irf_bank_profile(Pb.ctypes.data, J, S, best.ctypes.data, P.ctypes.data))
    assert np.all(best[S:] == -9) and np.all(P[S:] == R.CANARY)
    return best[:S], P[:S]


def test_profile_ties_all_minus_infinity_and_nan(trpl):
    from test_gpu_irf_bank import profile_ref
    n, i = np.nan, np.inf
    Pb = np.array([[-3.0, -1.0, -i, n, n, -2.0, -i, i, -0.0],
                   [-3.0, -2.0, -i, n, -i, n, -5.0, i, 0.0],
                   [-1.0, -1.0, -i, n, -7.0, -2.0, n, -i, -1.0]])
    best, P = _profile(trpl, Pb)
    assert best.tolist() == [2, 0, -1, -1, 2, 0, 1, 0, 0]                         # the first j that attains the maximum
    assert R.same_bits(P, np.array([-1.0, -1.0, -i, -i, -7.0, -2.0, -5.0, i, -0.0]))
    rng = np.random.default_rng(4)
    for J, S in ((1, 1), (1, 300), (3, 257), (7, 64)):
        Pb = -rng.uniform(0.0, 9.0, (J, S)).round(1)                              # one decimal: many ties
        Pb[rng.random((J, S)) < 0.3] = -np.inf
        Pb[rng.random((J, S)) < 0.3] = np.nan
        got, want = _profile(trpl, Pb), profile_ref(Pb)
        assert np.array_equal(got[0], want[0]) and R.same_bits(got[1], want[1])
        finite = np.where(np.isnan(Pb), -np.inf, Pb)
        assert np.array_equal(got[1], finite.max(axis=0)) and np.array_equal(got[0] == -1, np.isneginf(finite).all(axis=0))


# ------------------------------------------------------------------------------------------------ the C ABI
NEW = ("trpl_irf_bank_max_responses", "trpl_irf_bank_block", "trpl_loglik_irf_bank_dev", "trpl_loglik_irf_bank",
       "trpl_irf_bank_profile_dev", "trpl_irf_bank_profile")


def test_header_binding_and_library_agree(trpl):
    define = H.defines().__getitem__
    A = trpl._abi
    lib = A.lib()
    for name in NEW:
        assert name in A.SIGNATURES and hasattr(lib, name), name
        count = len(H.params(name))
        assert count == len(A.SIGNATURES[name]), (name, count)
    assert (define("TRPL_IRF_BANK_MAX_RESPONSES"), define("TRPL_IRF_BANK_BLOCK")) == (A.IRF_BANK_MAX_RESPONSES, A.IRF_BANK_BLOCK)
    assert lib.trpl_irf_bank_max_responses() == A.IRF_BANK_MAX_RESPONSES >= 256
    assert lib.trpl_irf_bank_block() == A.IRF_BANK_BLOCK >= 3
    assert lib.trpl_abi_version() == 5 == define("TRPL_ABI_VERSION")              # additive: the version stays


def test_every_refusal_names_its_argument_without_a_device(trpl):
    A = trpl._abi
    lib, E = A.lib(), A.ERR_ARG
    rows, ncol, K, k0, J, n = 3, 12, 4, 1, 2, 6
    pl, H = np.ones((rows, ncol)), np.full((J, K), 0.25)
    obs, mag, wts = np.zeros(n), np.zeros(rows), np.ones(n)
    hi, dx, oh = np.full(n, 2, dtype=np.int32), np.zeros(n), np.ones(n)
    sse, esum = np.full((J, rows), R.CANARY), np.full((J, rows), R.CANARY)
    p = lambda a: a.ctypes.data
    base = dict(pl=p(pl), elem=8, rows=rows, ncol=ncol, ld=ncol, H=p(H), J=J, K=K, k0=k0, obs=p(obs), hi=None, dx=None, oh=None, n=n,
                wts=None, mag=p(mag), status=None, sse=p(sse), esum=p(esum), flags=0)
    order = ("pl", "elem", "rows", "ncol", "ld", "H", "J", "K", "k0", "obs", "hi", "dx", "oh", "n", "wts", "mag", "status", "sse", "esum", "flags")

    def dev(**kw):
        a = dict(base, **kw)
        return lib.trpl_loglik_irf_bank_dev(*[a[k] for k in order], None)

    def host(**kw):
        a = dict(base, **kw)
        sec = ctypes.c_double(-1.0)
        rc = lib.trpl_loglik_irf_bank(*[a[k] for k in order], 0, ctypes.byref(sec))
        assert sec.value == 0.0
        return rc

    off = dict(hi=p(hi), dx=p(dx), oh=p(oh))
    cases = ((dict(elem=2), b"elem_bytes"), (dict(elem=16), b"elem_bytes"), (dict(rows=-1), b"rows"), (dict(rows=1 << 31), b"rows"),
             (dict(ncol=0), b"ncol"), (dict(ncol=1 << 31, ld=1 << 31), b"ncol"), (dict(ld=ncol - 1), b"ld="), (dict(K=0), b"K="),
             (dict(K=A.IRF_MAX_TAPS + 1), b"TRPL_IRF_MAX_TAPS"), (dict(k0=-1), b"k0"), (dict(k0=K), b"k0"),
             (dict(ncol=3, ld=3, k0=3), b"no output column"), (dict(J=0), b"J="),
             (dict(J=A.IRF_BANK_MAX_RESPONSES + 1), b"TRPL_IRF_BANK_MAX_RESPONSES"), (dict(n=0), b"n_obs"), (dict(n=-1), b"n_obs"),
             (dict(n=ncol - k0 + 1), b"n_obs"), (dict(hi=p(hi)), b"go together"), (dict(dx=p(dx), oh=p(oh)), b"go together"),
             (dict(off, ncol=2, ld=2, n=1), b"obs_hi needs two"), (dict(flags=A.FLAG_NORMALIZE), b"TRPL_FLAG_NORMALIZE"),
             (dict(flags=A.FLAG_MOMENTS), b"flags"), (dict(flags=A.FLAG_STRICT), b"flags"), (dict(pl=None), b"pl is NULL"),
             (dict(H=None), b"H is NULL"), (dict(obs=None), b"obs is NULL"), (dict(mag=None), b"mag is NULL"), (dict(sse=None), b"sse is NULL"))
    msg = lambda: lib.trpl_last_error()
    for call in (dev, host):
        for kw, word in cases:
            assert call(**kw) == E and word in msg(), (call.__name__, kw, msg())
    # the stated order: the first argument at fault is the one named
    assert dev(elem=3, rows=-1, J=0) == E and b"elem_bytes" in msg()
    assert dev(K=0, J=0, n=0) == E and b"K=" in msg()
    assert dev(J=0, n=0, flags=A.FLAG_NORMALIZE) == E and b"J=" in msg()
    assert dev(n=0, flags=A.FLAG_NORMALIZE, pl=None) == E and b"n_obs" in msg()
    assert dev(flags=A.FLAG_NORMALIZE, pl=None) == E and b"NORMALIZE" in msg()
    # the host form alone reads its arrays: a tap or a weight that is not finite, a bracket outside the convolved columns
    for bad in (np.nan, np.inf, -np.inf):
        Hb = H.copy()
        Hb[1, 2] = bad
        assert host(H=p(Hb)) == E and b"H[1][2]" in msg() and b"finite" in msg()
    for bad in (np.nan, np.inf, -1.0):
        wb = wts.copy()
        wb[3] = bad
        assert host(wts=p(wb)) == E and b"wts[3]" in msg()
    for bad in (0, ncol - k0, -4):
        hb = hi.copy()
        hb[4] = bad
        assert host(**dict(off, hi=p(hb))) == E and b"obs_hi[4]" in msg()
    # an empty block is a successful no-op in both forms, NULL pointers included
    assert dev(rows=0) == 0 and host(rows=0) == 0
    none = dict(rows=0, pl=None, H=None, obs=None, mag=None, sse=None, esum=None)
    assert dev(**none) == 0 and host(**none) == 0
    assert np.all(sse == R.CANARY) and np.all(esum == R.CANARY) and np.all(pl == 1.0)        # no refused call wrote anything

    Pb, best, P = np.zeros((J, 5)), np.full(5, -9, dtype=np.int32), np.full(5, R.CANARY)
    pbase = dict(Pb=p(Pb), J=J, S=5, best=p(best), P=p(P))
    prof_host = lambda **kw: lib.trpl_irf_bank_profile(*[dict(pbase, **kw)[k] for k in ("Pb", "J", "S", "best", "P")])
    prof_dev = lambda **kw: lib.trpl_irf_bank_profile_dev(*[dict(pbase, **kw)[k] for k in ("Pb", "J", "S", "best", "P")], None)
    for call in (prof_dev, prof_host):
        for kw, word in ((dict(J=0), b"J="), (dict(J=A.IRF_BANK_MAX_RESPONSES + 1), b"TRPL_IRF_BANK_MAX_RESPONSES"), (dict(S=-1), b"S="),
                         (dict(Pb=None), b"Pbank is NULL"), (dict(best=None), b"best is NULL"), (dict(P=None), b"P is NULL")):
            assert call(**kw) == E and word in msg(), (kw, msg())
        assert call(S=0) == 0 and call(S=0, Pb=None, best=None, P=None) == 0
    assert np.all(best == -9) and np.all(P == R.CANARY)


# ------------------------------------------------------------------------------------------------ the Python layer's own refusals
def _problem(trpl, S=4, L=32, T=64):
    w = trpl.workloads
    ini, lens = w.power_scan(L)
    Time = T * 0.025
    return dict(X=w.samples(S), init_params=ini[:2], lengths=lens[:2], Time=Time, L=L, T=T)


@pytest.mark.parametrize("route", ["loglik_bank", "loglik_profile"])
def test_the_routes_refuse_before_they_touch_a_device(trpl, route):
    call = getattr(trpl.irf, route)
    p = _problem(trpl)
    T, Time = p["T"], p["Time"]
    bank = trpl.irf.gaussian_bank([0.2], [-0.025, 0.0, 0.025], Time / T)
    H, k0, _ = bank
    assert k0 >= 3
    ncol_out = T + 1 - k0
    obs_ok = [np.zeros(ncol_out), np.zeros(5)]
    with pytest.raises(ValueError, match="T \\+ 1 - k0"):
        call(obs=[np.zeros(ncol_out + 1), np.zeros(5)], bank=bank, **p)
    late = [np.array([0.0, 0.1]), np.array([0.1, np.nextafter(np.linspace(0, Time, T + 1)[T - k0], np.inf)])]
    with pytest.raises(ValueError, match="convolved window"):
        call(obs=[np.zeros(2), np.zeros(2)], times=late, bank=bank, **p)
    with pytest.raises(ValueError, match="self-normalisation"):
        call(obs=obs_ok, bank=bank, normalize=True, **p)
    with pytest.raises(ValueError, match="at least one observation"):
        call(obs=[np.zeros(5), np.zeros(0)], bank=bank, **p)
    for bad in ((H, H.shape[1]), (H, -1), (H[0], k0), (np.zeros((0, 3)), 0), (np.ones((trpl._abi.IRF_BANK_MAX_RESPONSES + 1, 3)), 1),
                (np.ones((2, trpl._abi.IRF_MAX_TAPS + 1)), 0), (np.array([[1.0, np.nan]]), 0), 3.0):
        with pytest.raises(ValueError, match="bank"):
            call(obs=obs_ok, bank=bad, **p)
    with pytest.raises(ValueError, match="weights"):
        call(obs=obs_ok, bank=bank, weights=[np.ones(ncol_out), np.ones(4)], **p)
    with pytest.raises(ValueError, match="block"):
        call(obs=obs_ok, bank=bank, block=0, **p)
    info = {}
    out = call(obs=obs_ok, bank=(H, k0), info=info, **dict(p, X=np.zeros((0, 13))))          # no sample: no device
    assert out.shape == ((3, 0) if route == "loglik_bank" else (0,))
    assert info["ncol_out"] == ncol_out and info["sse"].shape == (3, 2, 0) and info["esum"].shape == (3, 2, 0)
    if route == "loglik_profile":
        assert info["best"].shape == (0,) and info["best"].dtype == np.int32 and info["P"].shape == (3, 0)
