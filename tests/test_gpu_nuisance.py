"""trpl_nuisance_reduce_dev on the device and the routes that carry it.  The kernel against the host form (tests/
test_nuisance_host.py holds that one to its restatement and to the three calls it is defined by): bit for bit with the maximum in P,
best and best_mag, and with the marginal an equal best and P inside the header's bound of the extended-precision value -- on the
host tests' cells, with S across the workgroup boundary.  Then irf.loglik_nuisance against irf.loglik_profile, trpl_mag_profile_w and
the extended-precision marginal of irf.loglik_bank's moments, mcmc.run on the marginal, and gpu_info["irf_bank"] of simulate."""
import functools
import math

import numpy as np
import pytest

import nuisance_ref as N
from irf_ref import same_bits
from test_nuisance_host import _offsets, _prior, check_marginal

pytestmark = pytest.mark.gpu
INF = np.inf
PAD = 5


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev(gpu, sse, esum, wsum, mode, off=None, marg=False, tf=1.0, logw=None, outputs=True):
    """nuisance_reduce_device -> (P, best, best_mag) on the host; the canaries behind every output are checked."""
    import torch
    S = sse.shape[2]
    P = torch.full((S + PAD,), -7.0, dtype=torch.float64, device="cuda")
    best = torch.full((S + PAD,), -9, dtype=torch.int32, device="cuda")
    mag = torch.full((S + PAD,), -7.0, dtype=torch.float64, device="cuda")
    gpu.device.nuisance_reduce_device(_up(sse), None if esum is None else _up(esum), wsum, P[:S], best=best[:S] if outputs else None,
                                      best_mag=mag[:S] if outputs else None, mag=mode if mode != N.GRID else off, marginal=marg, tf=tf,
                                      log_prior=logw)
    torch.cuda.synchronize()
    assert bool(torch.all(P[S:] == -7.0)) and bool(torch.all(best[S:] == -9)) and bool(torch.all(mag[S:] == -7.0))
    if not outputs:
        assert bool(torch.all(best == -9)) and bool(torch.all(mag == -7.0))
    return P[:S].cpu().numpy(), best[:S].cpu().numpy(), mag[:S].cpu().numpy()


@pytest.mark.parametrize("mode,M", [(N.FIXED, 1), (N.PROFILE, 1), (N.GRID, 1), (N.GRID, 5)])
@pytest.mark.parametrize("Cn,J", [(1, 1), (3, 9), (1, 9), (3, 1)])
@pytest.mark.parametrize("S", [1, 255, 257, 513])
def test_the_kernel_is_the_host_form(gpu, S, Cn, J, mode, M):
    sse, esum, wsum = N.moments(Cn, J, S, seed=S + 10 * Cn + J)
    off = _offsets(mode, M)
    want = N.host(gpu, sse, esum, wsum, mode, off)
    got = _dev(gpu, sse, esum, wsum, mode, off)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
    assert same_bits(_dev(gpu, sse, esum, wsum, mode, off, outputs=False)[0], want[0])                  # best and best_mag NULL
    if mode == N.FIXED:
        assert same_bits(_dev(gpu, sse, None, wsum, mode)[0], want[0])                                  # esum NULL
    if S > 1:
        assert got[0][1] == -INF and got[1][1] == -1 and np.isnan(got[2][1])
    # a curve without weight, and no weight at all
    if mode != N.FIXED and Cn > 1:
        for w0 in (np.where(np.arange(Cn) == 1, 0.0, wsum), np.zeros(Cn)):
            a, b = _dev(gpu, sse, esum, w0, mode, off), N.host(gpu, sse, esum, w0, mode, off)
            assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2])
    # the marginal: best equal, P inside the bound; the uniform prior and one with an excluded cell, from the host and from the device
    lib = gpu._abi.lib()
    for tf, logw in ((0.5, None), (1.0, _prior(J, M, seed=J)), (10.0, _prior(J, M, seed=J + 1))):
        got = _dev(gpu, sse, esum, wsum, mode, off, marg=True, tf=tf, logw=logw)
        ref = N.host(gpu, sse, esum, wsum, mode, off, marg=True, tf=tf, logw=logw)
        assert np.array_equal(got[1], ref[1]) and same_bits(got[2], ref[2])
        check_marginal(lib, got, sse, esum, wsum, mode, off, tf, logw)
        if logw is not None:
            again = _dev(gpu, sse, esum, wsum, mode, off, marg=True, tf=tf, logw=_up(logw), outputs=False)
            assert same_bits(again[0], got[0])


def test_cells_800_apart_ties_and_no_sample(gpu):
    import torch
    J, S, tf = 4, 3, 0.5
    sse = np.empty((1, J, S))
    sse[0] = (400.0 * np.arange(J))[:, None] + np.array([3.0, 7.5, 0.25])
    sse[0, :, 2] = sse[0, ::-1, 2]
    esum, wsum = np.zeros((1, J, S)), np.array([10.0])
    for logw in (None, np.array([-INF, -5.0, -1.0, -2.0])):
        got = _dev(gpu, sse, esum, wsum, N.FIXED, marg=True, tf=tf, logw=logw)
        assert np.array_equal(got[1], N.host(gpu, sse, esum, wsum, N.FIXED, marg=True, tf=tf, logw=logw)[1])
        check_marginal(gpu._abi.lib(), got, sse, esum, wsum, N.FIXED, None, tf, logw)
    assert same_bits(_dev(gpu, sse, esum, wsum, N.FIXED, marg=True, tf=tf)[0], np.array([-3.0, -7.5, -0.25]))
    # S = 0 is a successful no-op; the wrapper's own refusals launch nothing
    f64 = torch.float64
    empty = torch.empty((1, J, 0), dtype=f64, device="cuda")
    gpu.device.nuisance_reduce_device(empty, empty, wsum, torch.empty(0, dtype=f64, device="cuda"))
    s_d, P = _up(sse), torch.full((S,), -7.0, dtype=f64, device="cuda")
    call = gpu.device.nuisance_reduce_device
    for bad in (lambda: call(s_d, s_d, wsum, P[:2]), lambda: call(s_d[0], s_d[0], wsum, P), lambda: call(s_d.cpu(), s_d, wsum, P),
                lambda: call(s_d, s_d[:, :2], wsum, P), lambda: call(s_d, s_d, wsum, P, best=P), lambda: call(s_d, None, wsum, P, mag="profile"),
                lambda: call(s_d, s_d, wsum, P, mag="grid"), lambda: call(s_d, s_d, wsum, P, mag=np.zeros(65)), lambda: call(s_d, s_d, wsum, P, log_prior=np.zeros(J)),
                lambda: call(s_d, s_d, wsum, P, marginal=True, log_prior=np.zeros(J + 1)), lambda: call(s_d, s_d, wsum, P, marginal=True, tf=0.0),
                lambda: call(s_d, s_d, wsum, P, marginal=True, log_prior=np.array([0.0, np.nan, 0.0, 0.0])), lambda: call(s_d, s_d, [np.nan], P)):
        with pytest.raises((ValueError, gpu.TrplError)):
            bad()
    torch.cuda.synchronize()
    assert bool(torch.all(P == -7.0))


# ------------------------------------------------------------------------------------------------ irf.loglik_nuisance
def _problem():
    from test_gpu_irf_bank import _problem as bank_problem
    return bank_problem()


@functools.lru_cache(maxsize=None)
def _bank_moments(offgrid, weighted):
    """irf.loglik_bank's moments of the shared problem, its wsum and the keywords of the case: computed once."""
    import trpl_amd as gpu
    p = _problem()
    kw = p["per"][(offgrid, weighted, False)][2]
    info = {}
    gpu.irf.loglik_bank(*p["args"], p["bank"], info=info, **kw)
    obs = p["args"][6]
    wsum = np.array([math.fsum(w) for w in kw["weights"]] if weighted else [float(len(o)) for o in obs])
    sse, esum = (np.ascontiguousarray(info[k].transpose(1, 0, 2)) for k in ("sse", "esum"))           # (C, J, S)
    return sse, esum, wsum, kw


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
def test_loglik_nuisance_on_the_shared_problem(gpu, offgrid, weighted):
    p = _problem()
    sse, esum, wsum, kw = _bank_moments(offgrid, weighted)
    Cn, J, S = sse.shape
    lib = gpu._abi.lib()
    # fixed + max is loglik_profile, bit for bit
    pinfo, info = {}, {}
    want = gpu.irf.loglik_profile(*p["args"], p["bank"], info=pinfo, **kw)
    LL = gpu.irf.loglik_nuisance(*p["args"], p["bank"], info=info, keep_moments=True, **kw)
    assert same_bits(LL, want) and np.array_equal(info["best"], pinfo["best"]) and not info["best_mag"].any()
    assert same_bits(info["sse"], pinfo["sse"]) and same_bits(info["esum"], pinfo["esum"]) and info["cells"] == (J, 1)
    assert info["ncol_out"] == p["ncol_out"] and not info["status"].any()
    # profile: trpl_mag_profile_w on the moments of the winning response, bit for bit
    info = {}
    LL = gpu.irf.loglik_nuisance(*p["args"], p["bank"], mag="profile", info=info, **kw)
    assert "sse" not in info and (info["best"] >= 0).all()
    for s in range(S):
        j = int(info["best"][s])
        s2, e2 = np.ascontiguousarray(sse[:, j, s:s + 1]), np.ascontiguousarray(esum[:, j, s:s + 1])
        d, P = np.empty(1), np.zeros(1)
        gpu._abi.check(lib.trpl_mag_profile_w(s2.ctypes.data, e2.ctypes.data, wsum.ctypes.data, 1, Cn, 0, d.ctypes.data, P.ctypes.data))
        assert same_bits(LL[s:s + 1], P) and same_bits(info["best_mag"][s:s + 1], d), s
    assert np.all(LL >= want)                                                      # the profiled offset never fits worse than 0
    # the marginal: inside the bound of the extended-precision value of loglik_bank's moments, not below the greatest v + tf logw
    for mag, off, tf, logw in (("fixed", None, 1.0, None), (N.OFFSETS, N.OFFSETS, 10.0, None), ("profile", None, 0.5, _prior(J, 1, 3)),
                               (N.OFFSETS, N.OFFSETS, 2.0, _prior(J, 5, 4).reshape(J, 5))):
        mode = mag if isinstance(mag, str) else N.GRID
        info = {}
        LL = gpu.irf.loglik_nuisance(*p["args"], p["bank"], mag=mag, reduce="marginal", tf=tf, log_prior=logw, info=info, **kw)
        n = J * (len(off) if mode == N.GRID else 1)
        flat = np.full(n, -math.log(n)) if logw is None else np.ravel(logw)           # None is the uniform prior
        check_marginal(lib, (LL, info["best"], info["best_mag"]), sse, esum, wsum, mode, off, tf, flat)
    # S larger than the block: the same call's blocks run separately
    X = p["args"][0]
    for mag, red in (("profile", "max"), (N.OFFSETS, "marginal")):
        info = {}
        whole = gpu.irf.loglik_nuisance(*p["args"], p["bank"], mag=mag, reduce=red, tf=3.0, block=3, info=info, **kw)
        for blk in range(0, S, 3):
            one = {}
            part = gpu.irf.loglik_nuisance(X[blk:blk + 3], *p["args"][1:], p["bank"], mag=mag, reduce=red, tf=3.0, info=one, **kw)
            assert same_bits(whole[blk:blk + 3], part) and np.array_equal(info["best"][blk:blk + 3], one["best"])
            assert same_bits(info["best_mag"][blk:blk + 3], one["best_mag"])


def test_mcmc_runs_on_the_marginal_and_reproduces_itself(gpu):
    p = _problem()
    sm = gpu.sampler
    lo, hi, lg = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS, sm.DEFAULT_DO_LOG
    X, ini, lens, Time, L, T, obs = p["args"]
    tf = 4.0
    loglik = functools.partial(gpu.irf.loglik_nuisance, init_params=ini, lengths=lens, Time=Time, L=L, T=T, obs=obs, bank=p["bank"],
                               mag="profile", reduce="marginal", tf=tf)
    X0 = np.ascontiguousarray(gpu.workloads.samples(16, seed=29))
    LL0 = loglik(X0)
    runs = [gpu.mcmc.run(loglik, X0, LL0, lo, hi, lg, sweeps=3, seed=5, tf=tf, bounds="fold") for _ in range(2)]
    assert same_bits(runs[0].X, runs[1].X) and same_bits(runs[0].LL, runs[1].LL) and np.isfinite(runs[0].LL).all()


# ------------------------------------------------------------------------------------------------ gpu_info["irf_bank"]
def _simulate(gpu, p, e_data, gpu_info, **flags):
    X, ini, lens, Time, L, T, _ = p["args"]
    info = dict(sims_per_gpu=len(X), num_gpus=1, fused=True, pl_dtype=np.float64)
    info.update(gpu_info)
    P = np.zeros((len(e_data), len(X)))
    gpu.simulate(gpu.pvSim, e_data, P, X, [None], [None], 2, [list(lens), Time, L, T, 1, 0, 7, 10000], ini,
                 dict(dict(log_pl=True, self_normalize=False), **flags), info, 0, np.zeros(1), np.zeros(1), np.zeros(1))
    return P


def test_simulate_with_a_bank_is_loglik_nuisance_per_experiment(gpu):
    from trpl_amd.likelihood import weights_from_uncertainty
    p = _problem()
    X, ini, lens, Time, L, T, obs = p["args"]
    kw_off = p["per"][(True, False, False)][2]
    sim_t = np.linspace(0, Time, T + 1)
    rng = np.random.default_rng(8)
    unc = [rng.uniform(0.05, 0.5, len(o)) for o in obs]
    e_data = [([sim_t[:len(o)] for o in obs], obs, unc),                            # prefixes of the simulation grid
              (kw_off["times"], [o + 0.1 for o in obs], unc)]                       # off the grid
    args = (X, ini, lens, Time, L, T)
    for weighted in (False, True):
        wts = [weights_from_uncertainty(u) for u in unc] if weighted else None
        for opt in (dict(), dict(mag="profile"), dict(mag=N.OFFSETS)):
            P = _simulate(gpu, p, e_data, dict(irf_bank=dict(bank=p["bank"], **opt), weighted=weighted))
            want = [gpu.irf.loglik_nuisance(*args, e_data[0][1], p["bank"], weights=wts, **opt),
                    gpu.irf.loglik_nuisance(*args, e_data[1][1], p["bank"], times=kw_off["times"], weights=wts, **opt)]
            assert same_bits(P[0], want[0]) and same_bits(P[1], want[1]), (weighted, opt)
    opt = dict(mag="profile", reduce="marginal", tf=5.0, log_prior=_prior(6, 1, 2))
    P = _simulate(gpu, p, e_data[:1], dict(irf_bank=dict(bank=p["bank"], **opt), predict=True, pl_dtype=np.float32))
    assert same_bits(P[0], gpu.irf.loglik_nuisance(*args, e_data[0][1], p["bank"], predict=True, pl_f32=True, **opt))
    # every refused combination raises, naming the option
    bank = dict(bank=p["bank"])
    irf1 = (np.array([1.0]), 0)
    for extra, word in ((dict(irf=irf1), "irf"), (dict(mag_grid=[0.0, 0.1]), "mag_grid"), (dict(devices=[0]), "devices"), (dict(num_gpus=2), "num_gpus"),
                        (dict(cut_margin=5.0), "cut_margin"), (dict(max_sims_per_block=2), "max_sims_per_block"), (dict(fused=False), "unfused")):
        with pytest.raises(ValueError, match=word):
            _simulate(gpu, p, e_data[:1], dict(irf_bank=bank, **extra))
    with pytest.raises(ValueError, match="self_normalize"):
        _simulate(gpu, p, e_data[:1], dict(irf_bank=bank), self_normalize=True)
    late = ([sim_t[:5], np.array([0.0, np.nextafter(sim_t[T - p["bank"][1]], np.inf)])], [obs[0][:5], obs[1][:2]], [unc[0][:5], unc[1][:2]])
    with pytest.raises(ValueError, match="last convolved column"):
        _simulate(gpu, p, [late], dict(irf_bank=bank))
    for bad in (p["bank"], dict(mag="profile"), dict(bank=p["bank"], reduce="sum"), dict(bank=p["bank"], shifts=3),
                dict(bank=p["bank"], reduce="marginal", tf=-1.0), dict(bank=p["bank"], log_prior=np.zeros(6))):
        with pytest.raises(ValueError):
            _simulate(gpu, p, e_data[:1], dict(irf_bank=bad))
