"""Parallel tempering on the device (trpl_mcmc_*_rungs*, trpl_mcmc_swap*, csrc/mcmc.hip; trpl_amd.mcmc.run_tempered).

Slice identities: a rung's rows of propose_rungs / accept_rungs / levels_rungs are BIT FOR BIT the sampler's own call on those rows
with the rung's partner block, temperature and chain0 -- the existing kernels are the oracle, nothing is restated.  Swap: against
tests/mcmc_tempered_ref.py, bit for bit: its inputs excuse no decision (tests/test_mcmc_tempered_host.py).  run_tempered: one rung
is run(); three rungs against the restatement's run as tests/test_gpu_mcmc.py compares run; the bimodal toy, which a single
temperature never solves; a flat likelihood; early rejection on the fused likelihood."""
import numpy as np
import pytest

import mcmc_ref as mr
import mcmc_tempered_ref as tr
from test_gpu_mcmc import _cuda, _propose_dev, _same_bits, _states
from test_gpu_refine import TOY_HI, TOY_LG, TOY_LO, _box_for
from test_mcmc_fold_host import CHI2_GATE, FLAT, _chi2

pytestmark = pytest.mark.gpu
FOLD = 0x10
RUNGS = ((1, 4), (2, 5), (3, 2), (2, 129))                       # (K, group); the last crosses the 256-thread block


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


# ------------------------------------------------------------------ slice identities
@pytest.mark.parametrize("A", (1, 3, 16))
def test_propose_rungs_is_propose_on_every_rung(gpu, torch_dev, A):
    torch, dev = torch_dev
    box = 0 if A == 16 else 7
    rng = np.random.default_rng(A)
    lo, hi, lg = _box_for(A, box, rng)
    sim = {"override_equal_mu": bool(box & 1), "override_equal_s": bool(box & 2), "override_equal_auger": bool(box & 4)}
    scale, seed = rng.uniform(0.01, 0.05, A), (0x1234567 << 32) | 0x89abcdef
    differs = 0
    for K, group in RUNGS:
        P = K * group
        partners = rng.random((P, A))
        for count in sorted({P, P - 1, max(P - group - 1, 1)}):  # count == P, and count < P ending inside a rung
            U = _states(rng, count, A)
            for fold in (0, FOLD):
                for chain0, step in ((0, 4), ((1 << 32) + 5, 5)):
                    Up = torch.full((count, A), -7.0, dtype=torch.float64, device="cuda")
                    Xp = torch.full((count, lo.size), -7.0, dtype=torch.float64, device="cuda")
                    inside = torch.full((count,), -7, dtype=torch.int32, device="cuda")
                    dev.mcmc_propose_rungs_device(_cuda(torch, U), _cuda(torch, partners), group, 0.6, scale, chain0, seed, step, lo, hi,
                                                  lg, Up, Xp, inside, flags=box | fold)
                    torch.cuda.synchronize()
                    Up, Xp, inside = Up.cpu().numpy(), Xp.cpu().numpy(), inside.cpu().numpy()
                    for k in range(K):
                        s = slice(k * group, min((k + 1) * group, count))
                        if s.start >= count:
                            continue
                        wu, wx, wi = _propose_dev(torch_dev, U[s], partners[k * group:(k + 1) * group], 0.6, scale,
                                                  chain0 + k * group, seed, step, lo, hi, lg, box | fold)
                        assert _same_bits(Up[s], wu) and _same_bits(Xp[s], wx) and np.array_equal(inside[s], wi), (K, group, count, k)
                    if K > 1 and count == P:                     # ... and not the call that takes its partners from the whole block
                        whole = _propose_dev(torch_dev, U, partners, 0.6, scale, chain0, seed, step, lo, hi, lg, box | fold)
                        differs += not _same_bits(whole[0], Up)
                    hU, hX, hi_ = gpu.mcmc.propose_rungs(U, partners, group, 0.6, scale, chain0, seed, step, lo, hi, lg, sim,
                                                         fold=bool(fold))
                    assert _same_bits(hU, Up) and _same_bits(hX, Xp) and np.array_equal(hi_, inside)
                    assert fold or not (inside == 2).any()
    assert differs > 0


def _accept_dev(torch_dev, fn, U, X, LL, Up, Xp, LLp, inside, tf, chain0, seed, step):
    torch, dev = torch_dev
    dU, dX, dLL = _cuda(torch, U), _cuda(torch, X), _cuda(torch, LL)
    acc = torch.full((U.shape[0],), -7, dtype=torch.int32, device="cuda")
    getattr(dev, fn)(dU, dX, dLL, _cuda(torch, Up), _cuda(torch, Xp), _cuda(torch, LLp), _cuda(torch, inside), tf, chain0, seed, step, acc)
    torch.cuda.synchronize()
    return dU.cpu().numpy(), dX.cpu().numpy(), dLL.cpu().numpy(), acc.cpu().numpy()


def _same_accept(a, b):
    return all(_same_bits(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("K,group", RUNGS)
def test_accept_rungs_is_accept_on_every_rung(gpu, torch_dev, K, group):
    count = K * group
    ladder = np.array([37.5, 1.0, 4.0])[:K]                      # distinct, unsorted
    for A, ncol in ((3, 5), (16, 16), (1, 1)):
        U, X, LL, Up, Xp, LLp, inside = mr.accept_case(count, 1.0, A=A, ncol=ncol)
        for chain0, step in ((0, 0), ((1 << 32) + 5, 1)):
            got = _accept_dev(torch_dev, "mcmc_accept_rungs_device", U, X, LL, Up, Xp, LLp, inside, ladder, chain0, mr.ACCEPT_SEED, step)
            taken = 0
            for k in range(K):
                s = slice(k * group, (k + 1) * group)
                want = _accept_dev(torch_dev, "mcmc_accept_device", U[s], X[s], LL[s], Up[s], Xp[s], LLp[s], inside[s], ladder[k],
                                   chain0 + k * group, mr.ACCEPT_SEED, step)
                assert _same_accept([g[s] for g in got], want), (K, group, A, k)
                taken += int(want[3].sum())
            assert group < 5 or 0 < taken < count
            # a uniform ladder: the scalar call on the whole block
            flat = _accept_dev(torch_dev, "mcmc_accept_rungs_device", U, X, LL, Up, Xp, LLp, inside, np.full(K, 2.5), chain0, mr.ACCEPT_SEED,
                               step)
            assert _same_accept(flat, _accept_dev(torch_dev, "mcmc_accept_device", U, X, LL, Up, Xp, LLp, inside, 2.5, chain0,
                                                  mr.ACCEPT_SEED, step))
            # the host-buffer form, in place
            hU, hX, hLL = U.copy(), X.copy(), LL.copy()
            hacc = gpu.mcmc.accept_rungs(hU, hX, hLL, Up, Xp, LLp, inside, ladder, chain0, mr.ACCEPT_SEED, step)
            assert _same_accept((hU, hX, hLL, hacc), got)


@pytest.mark.parametrize("K,group", RUNGS)
def test_levels_rungs_is_levels_on_every_rung(gpu, torch_dev, K, group):
    torch, dev = torch_dev
    count = K * group
    ladder = np.array([37.5, 1.0, 4.0])[:K]
    LL = mr.accept_case(count, 1.0)[2] * 40.0                    # NaN and -inf among them

    def levels(fn, ll, tf, chain0, step):
        out = torch.full((ll.shape[0],), -7.0, dtype=torch.float64, device="cuda")
        getattr(dev, fn)(_cuda(torch, ll), tf, chain0, mr.ACCEPT_SEED, step, out)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    for chain0, step in ((0, 0), ((1 << 32) + 5, 1)):
        got = levels("mcmc_levels_rungs_device", LL, ladder, chain0, step)
        for k in range(K):
            s = slice(k * group, (k + 1) * group)
            assert _same_bits(got[s], levels("mcmc_levels_device", LL[s], ladder[k], chain0 + k * group, step)), (K, group, k)
        assert group < 5 or (np.isfinite(got).any() and np.isinf(got).any())
        assert _same_bits(levels("mcmc_levels_rungs_device", LL, np.full(K, 2.5), chain0, step),
                          levels("mcmc_levels_device", LL, 2.5, chain0, step))
        assert _same_bits(gpu.mcmc.reject_levels_rungs(LL, ladder, chain0, mr.ACCEPT_SEED, step), got)


# ------------------------------------------------------------------ swap
@pytest.mark.parametrize("K", tr.SWAP_KS)
def test_swap_against_the_restatement(gpu, torch_dev, K):
    torch, dev = torch_dev
    tf = tr.swap_ladder(K)
    exchanged = 0
    for group, parity, A, ncol, chain0, step in tr.swap_cases(K):
        U, X, LL = tr.swap_case(K, group, A, ncol)
        want_U, want_X, want_LL, want_sw, margin = tr.swap(U, X, LL, K, group, tf, parity, chain0, tr.SWAP_SEED, step)
        excused = margin <= mr.MARGIN
        assert excused.mean() <= 0.01 and not excused.any()      # the cap of the accept test; here nothing is excused at all
        dU, dX, dLL = _cuda(torch, U), _cuda(torch, X), _cuda(torch, LL)
        sw = torch.full((K * group,), -7, dtype=torch.int32, device="cuda")
        dev.mcmc_swap_device(dU, dX, dLL, tf, parity, chain0, tr.SWAP_SEED, step, sw)
        torch.cuda.synchronize()
        gU, gX, gLL, sw = dU.cpu().numpy(), dX.cpu().numpy(), dLL.cpu().numpy(), sw.cpu().numpy()
        case = (K, group, parity, A, ncol)
        assert np.array_equal(sw, want_sw), (case, np.flatnonzero(sw != want_sw)[:4])
        assert _same_bits(gU, want_U) and _same_bits(gX, want_X) and _same_bits(gLL, want_LL), case
        a, b, _ = tr.swap_pairs(K, group, parity)
        unpaired = np.setdiff1d(np.arange(K * group), np.concatenate([a, b]))
        assert np.all(sw[unpaired] == 0)
        assert _same_bits(gU[unpaired], U[unpaired]) and _same_bits(gX[unpaired], X[unpaired]) and _same_bits(gLL[unpaired], LL[unpaired])
        assert np.array_equal(sw[a], sw[b])
        exchanged += int(sw.sum())
        hU, hX, hLL = U.copy(), X.copy(), LL.copy()              # the host-buffer form, in place
        hsw = gpu.mcmc.swap(hU, hX, hLL, tf, parity, chain0, tr.SWAP_SEED, step)
        assert np.array_equal(hsw, sw) and _same_bits(hU, gU) and _same_bits(hX, gX) and _same_bits(hLL, gLL)
    assert exchanged > 0


def test_swap_of_one_rung_writes_zeros(gpu):
    U, X, LL = tr.swap_case(1, 257, 3, 5)
    for parity in (0, 1):
        hU, hX, hLL = U.copy(), X.copy(), LL.copy()
        sw = gpu.mcmc.swap(hU, hX, hLL, [3.0], parity, 0, 1, 0)
        assert not sw.any() and _same_bits(hU, U) and _same_bits(hX, X) and _same_bits(hLL, LL)


# ------------------------------------------------------------------ run_tempered
@pytest.mark.parametrize("bounds", ("reject", "fold"))
@pytest.mark.parametrize("kind", ("de", "rw"))
def test_a_ladder_of_one_is_the_plain_run(gpu, kind, bounds):
    U0 = mr.toy_start(32, 6)
    X0 = mr.rr.from_unit(U0, TOY_LO, TOY_HI, TOY_LG)
    LL0 = mr.e2e_loglik(X0)
    kw = dict(sweeps=6, kind=kind, scale=0.05, jump_every=4, seed=6, bounds=bounds, U0=U0)
    i0, i1 = {}, {}
    plain = gpu.mcmc.run(mr.e2e_loglik, X0, LL0, TOY_LO, TOY_HI, TOY_LG, tf=2.5, info=i0, **kw)
    t = gpu.mcmc.run_tempered(mr.e2e_loglik, X0, LL0, TOY_LO, TOY_HI, TOY_LG, [2.5], info=i1, **kw)
    one = t.rung(0)
    for k in ("U", "X", "LL", "accept"):
        assert getattr(one, k).tobytes() == getattr(plain, k).tobytes() and getattr(one, k).shape == getattr(plain, k).shape, k
    assert np.array_equal(t.ladder, [2.5]) and t.swap_rate.shape == (0,) and i1["swap_rate"].shape == (0,)
    assert np.array_equal(i1["accept"][:, 0], i0["accept"]) and i1["outside"][0] == i0["outside"] and i1["folded"][0] == i0["folded"]
    assert 0 < plain.accept.mean() < 1 and (bounds == "reject") == (i0["outside"] > 0)
    assert all(np.array_equal(x, y) for x, y in zip(t.samples(2, 2), plain.samples(2, 2)))


@pytest.mark.parametrize("swap_every", (1, 3))
def test_three_rungs_end_to_end_against_the_restatement(gpu, swap_every):
    U0, X0, LL0, ref = tr.e2e_reference(swap_every)
    assert ref["margin"] > mr.E2E_MARGIN                         # no decision near the margin: the device must decide the same
    calls, info = [], {}

    def loglik(X):
        calls.append(X.shape[0])
        return mr.e2e_loglik(X)

    K, C, sweeps = len(tr.E2E["ladder"]), tr.E2E["C"], tr.E2E["sweeps"]
    t = gpu.mcmc.run_tempered(loglik, X0, LL0, TOY_LO, TOY_HI, TOY_LG, tr.E2E["ladder"], sweeps=sweeps, swap_every=swap_every,
                              seed=tr.E2E["seed"], info=info, U0=U0)
    assert len(calls) <= 2 * sweeps                              # ONE likelihood call per half-sweep, all rungs in it
    assert sum(calls) == round(float((1.0 - ref["outside"]).sum()) * sweeps * C)
    for k in range(K):
        ch = t.rung(k)
        assert ch.U.shape == (sweeps, C, 3) and ch.X.shape == (sweeps, C, 3) and ch.LL.shape == (sweeps, C)
        for s in range(sweeps):
            assert np.array_equal(ch.accept[s], ref["accepted"][k, s]), (k, s)
        assert _same_bits(ch.U, ref["U"][k])
        assert np.allclose(ch.LL, ref["LL"][k], rtol=0, atol=1e-9)
        assert np.allclose(info["accept"][:, k], ref["accepted"][k].mean(axis=1), rtol=0, atol=1e-15)
        assert np.allclose(ch.rhat(burn=2), mr.rhat(ref["U"][k], 2), rtol=1e-12, atol=0)
    assert np.array_equal(info["outside"], ref["outside"])
    assert np.array_equal(t.swap_rate, ref["swap_rate"]) and np.array_equal(info["swap_rate"], ref["swap_rate"])
    assert np.all(t.swap_rate > 0)
    print("three rungs, swap_every=%d: acceptance %s, swap rates %s" % (swap_every, info["accept"].mean(axis=0), t.swap_rate))


def test_the_bimodal_toy_needs_the_ladder(gpu):
    """An equal mixture of two Gaussians of deviation 0.03, 16 deviations apart along each axis, every chain started in the first.
    One temperature: no state ever lies in the second mode -- exactly none.  Seven rungs up to tf = 64: the cold rung's share of the
    second mode is 1/2 within 5 standard deviations of the restatement's share over 8 seeds (tests/mcmc_tempered_ref.py,
    BI_SHARES; tests/test_mcmc_tempered_host.py recomputes them)."""
    seed = tr.BI_DEVICE_SEED
    U0, LL0 = tr.bimodal_start(seed)
    lo, hi, lg = tr.BI_BOX
    plain = gpu.mcmc.run(tr.bimodal_loglik, U0, LL0, lo, hi, lg, sweeps=tr.BI_SWEEPS, seed=seed, U0=U0)
    assert tr.second_mode_share(plain.U) == 0.0
    lad = gpu.mcmc.geometric_ladder(1.0, tr.BI_HOT, tr.BI_K)
    assert np.array_equal(lad, tr.geometric_ladder(1.0, tr.BI_HOT, tr.BI_K))
    info = {}
    t = gpu.mcmc.run_tempered(tr.bimodal_loglik, U0, LL0, lo, hi, lg, lad, sweeps=tr.BI_SWEEPS, seed=seed, U0=U0, info=info)
    share = tr.second_mode_share(t.rung(0).U[tr.BI_BURN:])
    print("bimodal: cold share %.6f (restatement %.6f, margin %.4f), per rung %s, swap rates %s"
          % (share, tr.BI_SHARES[tr.BI_SEEDS.index(seed)], tr.BI_MARGIN,
             [round(tr.second_mode_share(t.rung(k).U[tr.BI_BURN:]), 3) for k in range(tr.BI_K)], np.round(t.swap_rate, 3)))
    assert abs(share - 0.5) < tr.BI_MARGIN
    assert t.swap_rate.shape == (tr.BI_K - 1,) and np.all(t.swap_rate > 0)
    Xs, W = t.samples(burn=tr.BI_BURN)
    assert Xs.shape == ((tr.BI_SWEEPS - tr.BI_BURN) * tr.BI_C, 2) and tr.second_mode_share(Xs) == share


def test_a_flat_likelihood_exchanges_every_pair_and_keeps_every_rung_uniform(gpu):
    """d = 0 whatever the ladder: every proposed exchange takes place.  Each rung stays uniform under the folded proposal: the
    chi-square gate of tests/test_mcmc_fold_host.py (20 bins, 19 degrees of freedom, tail 1e-6) on the same pooled sweeps."""
    lo, hi, lg = mr.CUBE
    C, K = 256, 3
    U0 = mr.toy_start(C, 11)
    info = {}
    t = gpu.mcmc.run_tempered(lambda X: np.zeros(X.shape[0]), U0, np.zeros(C), lo, hi, lg, [1.0, 3.0, 9.0], sweeps=FLAT["sweeps"],
                              seed=11, bounds="fold", kind="de", gamma=1.0, U0=U0, info=info)
    assert np.array_equal(t.swap_rate, [1.0, 1.0])
    assert np.all(info["accept"] == 1.0) and np.all(info["outside"] == 0) and np.all(info["folded"] > 0)
    for k in range(K):
        chi = _chi2(dict(U=t.rung(k).U))
        print("flat, rung %d: chi-square per dimension %s, gate %.2f" % (k, chi, CHI2_GATE))
        assert np.all(chi < CHI2_GATE), (k, chi)
    assert not _same_bits(t.rung(0).U[-1], t.rung(1).U[-1])


# ------------------------------------------------------------------ early rejection on the fused likelihood
@pytest.mark.parametrize("bounds", ["reject", "fold"])
def test_early_rejection_leaves_the_tempered_chains_unchanged(gpu, oracle, bounds):
    """tests/test_gpu_mcmc_early_reject.py's problem and batch (16 rows per half-sweep): two rungs of 16 chains, 4 sweeps."""
    import test_gpu_mcmc_early_reject as er
    ini, lens, X0, obs, (lo, hi, lg) = er._problem(gpu, oracle)
    X0 = np.ascontiguousarray(np.concatenate([X0[:8], X0[16:24]]))      # 8 cluster chains and 8 box samples per rung
    T, L, DT = er.T, er.L, er.DT

    def likelihood(work):
        def f(X, cut_levels=None):
            info = {}
            P = gpu.loglik(X, ini, lens, T * DT, L, T, obs, info=info, cut_levels=cut_levels)
            work["iters"] += int(info["iters_total"].sum())
            work["calls"] += 1
            if cut_levels is not None:
                assert cut_levels.shape == (len(X),)
                work["cut"] += int((info["cut_col"] >= 0).any(axis=0).sum())
            return P
        return f

    LL0 = likelihood(dict(iters=0, calls=0, cut=0))(X0)
    runs = {}
    for early in (False, True):
        work, info = dict(iters=0, calls=0, cut=0), {}
        t = gpu.mcmc.run_tempered(likelihood(work), X0, LL0, lo, hi, lg, [1.0, 8.0], sweeps=4, seed=er.SEED, bounds=bounds, info=info,
                                  early_reject=early)
        runs[early] = (t, work, info)
    (plain, w0, i0), (fast, w1, i1) = runs[False], runs[True]
    print("bounds=%s: acceptance %s, swap rate %s, %d cut (levelled %s), iterations %d -> %d"
          % (bounds, i0["accept"].mean(axis=0), plain.swap_rate, w1["cut"], i1["early_reject"], w0["iters"], w1["iters"]))
    for k in range(2):
        for name in ("U", "X", "LL", "accept"):
            assert getattr(fast.rung(k), name).tobytes() == getattr(plain.rung(k), name).tobytes(), (k, name)
    assert np.array_equal(i1["accept"], i0["accept"]) and np.array_equal(i1["outside"], i0["outside"])
    assert np.array_equal(fast.swap_rate, plain.swap_rate, equal_nan=True)
    assert "early_reject" not in i0 and i1["early_reject"].shape == (2,)
    assert w0["calls"] == w1["calls"] <= 8                       # one likelihood call per half-sweep
    assert w1["cut"] >= 1 and w0["cut"] == 0
    assert w1["iters"] < w0["iters"]
