"""The ensemble Metropolis kernels on the device (trpl_mcmc_*, csrc/mcmc.hip) against tests/mcmc_ref.py.

Propose: Up and inside BIT FOR BIT the restatement (Philox, genrand_res53, separate subtract, multiply and add are exact
restatements); the columns of Xp by the rule of tests/test_gpu_refine.py for the draw: linear columns, fixed columns and overrides
bit for bit, log columns within that file's 4 ulp (the distance of the device's pow to numpy's).  Accept: `accepted` equals the
restatement's except where |ln xi - d| <= 1e-12 max(1, |d|) in longdouble (the device's log against the longdouble one), at most
1 % of the decisions -- and the inputs are seeded so that the restatement excuses none (tests/test_mcmc_host.py); accepted rows are
the proposal's bits, rejected rows untouched.  Chain stats: bit for bit the loop.  End to end: trpl_amd.mcmc.run against the
restatement's run: the same decisions on every sweep and the same bits of U."""
import numpy as np
import pytest

import mcmc_ref as mr
import quantiles_ref as qr
import refine_ref as rr
from test_gpu_refine import TOY_HI, TOY_LG, TOY_LO, _box_for

pytestmark = pytest.mark.gpu
LOG_ULP = 4                                                      # tests/test_gpu_refine.py's bound for a log column of the draw


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


def _same_bits(a, b):
    """Equal bit patterns; a NaN matches a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ propose
def _propose_dev(torch_dev, U, partners, gamma, scale, chain0, seed, step, lo, hi, lg, flags):
    torch, dev = torch_dev
    count, A = U.shape
    Up = torch.full((count, A), -7.0, dtype=torch.float64, device="cuda")
    Xp = torch.full((count, lo.size), -7.0, dtype=torch.float64, device="cuda")
    inside = torch.full((count,), -7, dtype=torch.int32, device="cuda")
    dev.mcmc_propose_device(_cuda(torch, U), None if partners is None else _cuda(torch, partners), gamma, scale, chain0, seed, step, lo, hi,
                            lg, Up, Xp, inside, flags=flags)
    torch.cuda.synchronize()
    return Up.cpu().numpy(), Xp.cpu().numpy(), inside.cpu().numpy()


def _check_columns(Xp, want_x, lo, hi, lg, flags):
    """tests/test_gpu_refine.py's rule for the columns of a draw.  Returns the largest distance of a log column in ulp."""
    worst = 0.0
    for c in range(lo.size):
        src = {2: 3, 6: 5, 8: 7}.get(c) if ((c == 2 and flags & 1) or (c == 6 and flags & 2) or (c == 8 and flags & 4)) else None
        if src is not None:
            assert _same_bits(Xp[:, c], Xp[:, src]), c           # the override, applied last
        ref_c = c if src is None else src
        if lo[ref_c] == hi[ref_c]:
            assert np.all(Xp[:, c] == lo[ref_c]), c
        elif lg[ref_c]:
            ok = ~np.isnan(want_x[:, c])
            assert np.array_equal(np.isnan(Xp[:, c]), ~ok), c
            if ok.any():
                ulp = np.abs(Xp[ok, c] - want_x[ok, c]) / np.spacing(np.abs(want_x[ok, c]))
                worst = max(worst, float(ulp.max()))
                assert np.all(ulp <= LOG_ULP), (c, ulp.max())
        else:
            assert _same_bits(Xp[:, c], want_x[:, c]), c
    return worst


def _states(rng, count, A):
    """Chains of which some sit at the faces of the cube (their proposals leave it); row 1 holds a NaN."""
    U = rng.random((count, A))
    U[::5] = np.where(rng.random(U[::5].shape) < 0.5, 1e-4, 1.0 - 1e-4)
    if count > 1:
        U[1, A - 1] = np.nan
    return U


@pytest.mark.parametrize("A", (1, 2, 3, 7, 16))
def test_propose_against_the_restatement(gpu, torch_dev, A):
    flags = 0 if A == 16 else 7                                  # sixteen active columns leave no room for the overrides' targets
    rng = np.random.default_rng(A)
    lo, hi, lg = _box_for(A, flags, rng)
    assert rr.active_columns(lo, hi, flags).size == A and lg.any()
    assert flags == 0 or (np.any(lo == hi) and lo.size >= 9)     # a fixed column, and all three overrides apply
    seed = (0x1234567 << 32) | 0x89abcdef
    scale = rng.uniform(0.01, 0.05, A)
    sim = {"override_equal_mu": bool(flags & 1), "override_equal_s": bool(flags & 2), "override_equal_auger": bool(flags & 4)}
    worst, outside, total = 0.0, 0, 0
    for count in (1, 255, 256, 257, 1000):
        U = _states(rng, count, A)
        for P in (0, 2, 3, 1000):
            partners = rng.random((P, A)) if P else None
            for chain0 in (0, (1 << 32) + 5):
                got = {}
                for step in (4, 5):
                    Up, Xp, inside = _propose_dev(torch_dev, U, partners, 0.6, scale, chain0, seed, step, lo, hi, lg, flags)
                    want_u, want_x, want_in = mr.propose(U, partners, 0.6, scale, chain0, seed, step, lo, hi, lg, flags)
                    assert _same_bits(Up, want_u), (count, P, chain0, step)
                    assert np.array_equal(inside, want_in), (count, P, chain0, step)
                    worst = max(worst, _check_columns(Xp, want_x, lo, hi, lg, flags))
                    if count > 1:
                        assert inside[1] == 0 and np.isnan(Up[1, A - 1])          # a NaN coordinate is outside
                    outside += int((inside == 0).sum())
                    total += count
                    got[step] = Up
                assert not _same_bits(got[4], got[5])            # another step, another stream
                if count == 257 and P in (0, 3):
                    # a second call: the same bits; the host-buffer form: the same bits
                    again = _propose_dev(torch_dev, U, partners, 0.6, scale, chain0, seed, 5, lo, hi, lg, flags)
                    assert _same_bits(again[0], Up) and _same_bits(again[1], Xp) and np.array_equal(again[2], inside)
                    Uh, Xh, ih = gpu.mcmc.propose(U, partners, 0.6, scale, chain0, seed, 5, lo, hi, lg, sim)
                    assert _same_bits(Uh, Up) and _same_bits(Xh, Xp) and np.array_equal(ih, inside)
    print("propose A=%d: log columns within %.2f ulp; %.1f %% of the proposals left the cube" % (A, worst, 100.0 * outside / total))
    assert 0 < outside < total                                   # both kinds occurred


@pytest.mark.parametrize("count", (1, 257))
def test_propose_host_form_without_partners(gpu, torch_dev, count):
    """partners NULL with P = 0 through the host-buffer form, one chain and one block boundary: the _dev form's bits."""
    A, flags = 3, 0
    rng = np.random.default_rng(count)
    lo, hi, lg = _box_for(A, flags, rng)
    U, scale = _states(rng, count, A), rng.uniform(0.01, 0.05, A)
    info = {}
    Uh, Xh, ih = gpu.mcmc.propose(U, None, 0.6, scale, 7, 11, 5, lo, hi, lg, info=info)
    Up, Xp, inside = _propose_dev(torch_dev, U, None, 0.6, scale, 7, 11, 5, lo, hi, lg, flags)
    assert _same_bits(Uh, Up) and _same_bits(Xh, Xp) and np.array_equal(ih, inside)
    assert _same_bits(Uh, mr.propose(U, None, 0.6, scale, 7, 11, 5, lo, hi, lg, flags)[0])


# ------------------------------------------------------------------ accept
@pytest.mark.parametrize("count", mr.ACCEPT_COUNTS)
def test_accept_against_the_restatement(gpu, torch_dev, count):
    torch, dev = torch_dev
    for tf in mr.ACCEPT_TFS:
        U, X, LL, Up, Xp, LLp, inside = mr.accept_case(count, tf)
        for step, chain0 in ((0, 0), (1, 0)):
            want_U, want_X, want_LL, want_acc, margin = mr.accept(U, X, LL, Up, Xp, LLp, inside, tf, chain0, mr.ACCEPT_SEED, step)
            dU, dX, dLL = _cuda(torch, U), _cuda(torch, X), _cuda(torch, LL)
            acc = torch.full((count,), -7, dtype=torch.int32, device="cuda")
            dev.mcmc_accept_device(dU, dX, dLL, _cuda(torch, Up), _cuda(torch, Xp), _cuda(torch, LLp), _cuda(torch, inside), tf, chain0,
                                   mr.ACCEPT_SEED, step, acc)
            torch.cuda.synchronize()
            acc, gU, gX, gLL = acc.cpu().numpy(), dU.cpu().numpy(), dX.cpu().numpy(), dLL.cpu().numpy()
            excused = margin <= mr.MARGIN
            print("accept count=%d tf=%g step=%d: %d taken, %d excused, smallest margin %.3g" % (count, tf, step, int(acc.sum()),
                                                                                                int(excused.sum()), margin.min()))
            assert excused.mean() <= 0.01
            assert np.all(np.isin(acc, (0, 1))) and np.array_equal(acc[~excused], want_acc[~excused]), np.flatnonzero(acc != want_acc)[:4]
            take = acc != 0
            assert _same_bits(gU[take], Up[take]) and _same_bits(gX[take], Xp[take]) and _same_bits(gLL[take], LLp[take])
            assert _same_bits(gU[~take], U[~take]) and _same_bits(gX[~take], X[~take]) and _same_bits(gLL[~take], LL[~take])
            if not excused.any():
                assert _same_bits(gU, want_U) and _same_bits(gX, want_X) and _same_bits(gLL, want_LL)
            # the host-buffer form: the same decisions, in place
            hU, hX, hLL = U.copy(), X.copy(), LL.copy()
            hacc = gpu.mcmc.accept(hU, hX, hLL, Up, Xp, LLp, inside, tf, chain0, mr.ACCEPT_SEED, step)
            assert np.array_equal(hacc, acc) and _same_bits(hU, gU) and _same_bits(hX, gX) and _same_bits(hLL, gLL)
        if count > 1:                                            # the branches, by their rows (mr.accept_case)
            assert not take[inside == 0].any() and not take[np.isnan(LLp)].any() and not take[LLp == -np.inf].any()
            plain = (inside != 0) & np.isfinite(LLp)
            assert np.all(take[plain & ~(LL > -np.inf)]) and np.all(take[plain & (LLp == LL)])
            assert np.all(take[(inside != 0) & (LLp == np.inf) & (LL < np.inf)])
    # a chain's stream is its ensemble index: rows 5 .. of a call at chain0 = 0 decide as rows 0 .. of a call at chain0 = 5
    if count > 5:
        tf = mr.ACCEPT_TFS[0]
        U, X, LL, Up, Xp, LLp, inside = mr.accept_case(count, tf)
        full = gpu.mcmc.accept(U.copy(), X.copy(), LL.copy(), Up, Xp, LLp, inside, tf, (1 << 32), mr.ACCEPT_SEED, 0)
        part = gpu.mcmc.accept(U[5:].copy(), X[5:].copy(), LL[5:].copy(), Up[5:], Xp[5:], LLp[5:], inside[5:], tf, (1 << 32) + 5,
                               mr.ACCEPT_SEED, 0)
        assert np.array_equal(full[5:], part)


# ------------------------------------------------------------------ chain stats
@pytest.mark.parametrize("n", (1, 2, 3, 257))
def test_chain_stats_are_the_loop_bit_for_bit(gpu, torch_dev, n):
    torch, dev = torch_dev
    rng = np.random.default_rng(n)
    for Q in (1, 63, 64, 65, 1000):
        ldh = Q + 3
        H = np.full((n, ldh), np.nan)                            # the padding holds NaN: nothing may read it
        H[:, :Q] = rng.normal(size=(n, Q)) * 10.0 ** rng.integers(-3, 4, Q) + rng.normal(size=Q)
        if Q > 1:
            H[n // 2, Q - 1] = np.nan                            # a NaN column
        dH = _cuda(torch, H)
        ranges = {(0, n), (0, 1), (n - 1, n), (n // 3, max(n // 3 + 1, (2 * n) // 3))}
        for t0, t1 in sorted(ranges):
            mean = torch.full((Q,), -7.0, dtype=torch.float64, device="cuda")
            m2 = torch.full((Q,), -7.0, dtype=torch.float64, device="cuda")
            dev.mcmc_chain_stats_device(dH, t0, t1, mean, m2, Q=Q)
            torch.cuda.synchronize()
            want_mean, want_m2 = mr.chain_stats(H, t0, t1, Q)
            assert _same_bits(mean.cpu().numpy(), want_mean), (n, Q, t0, t1)
            assert _same_bits(m2.cpu().numpy(), want_m2), (n, Q, t0, t1)
            if Q > 1:
                holds = t0 <= n // 2 < t1
                assert bool(np.isnan(want_mean[Q - 1])) == holds and np.all(np.isfinite(want_mean[:Q - 1]))
            hm, hv = gpu.mcmc.chain_stats(H, t0, t1, Q=Q)        # the host-buffer form copies the range only
            assert _same_bits(hm, want_mean) and _same_bits(hv, want_m2)


# ------------------------------------------------------------------ end to end
def test_the_toy_end_to_end_on_the_device(gpu):
    assert np.array_equal(mr.E2E_LO, TOY_LO) and np.array_equal(mr.E2E_HI, TOY_HI) and np.array_equal(mr.E2E_LG, TOY_LG)
    U0, X0, LL0, ref = mr.e2e_reference()
    assert ref["margin"] > mr.E2E_MARGIN                         # no decision near the margin: the device must decide the same
    calls = []

    def loglik(X):
        calls.append(X.shape[0])
        return mr.e2e_loglik(X)

    info = {}
    ch = gpu.mcmc.run(loglik, X0, LL0, TOY_LO, TOY_HI, TOY_LG, sweeps=mr.E2E["sweeps"], seed=mr.E2E["seed"], info=info, U0=U0)
    C, sweeps = mr.E2E["C"], mr.E2E["sweeps"]
    assert ch.U.shape == (sweeps, C, 3) and ch.X.shape == (sweeps, C, 3) and ch.LL.shape == (sweeps, C)
    for t in range(sweeps):
        assert np.array_equal(ch.accept[t], ref["accepted"][t]), t
    assert _same_bits(ch.U, ref["U"])
    assert np.allclose(ch.LL, ref["LL"], rtol=0, atol=1e-9)
    assert np.allclose(info["accept"], ref["accepted"].mean(axis=1), rtol=0, atol=1e-15) and info["outside"] == ref["outside"]
    assert sum(calls) == round((1.0 - ref["outside"]) * sweeps * C) and ref["outside"] > 0        # only the inside proposals are solved
    r, want = ch.rhat(burn=20), mr.rhat(ref["U"], 20)
    print("end to end: acceptance %.3f, outside %.4f, R-hat %s" % (np.mean(info["accept"]), info["outside"], r))
    assert np.allclose(r, want, rtol=1e-12, atol=0)
    # the existing posterior tools take the samples unchanged.  A chain repeats its state wherever a move was rejected, so the
    # samples hold ties: the numpy rule is tests/quantiles_ref.py's (tie groups, longdouble cumulative weights), here on weights of 1
    Xs, W = ch.samples(burn=20, thin=2)
    N = Xs.shape[0]
    assert N == 20 * C and np.all(W == 1.0)
    assert np.unique(Xs[:, 0]).size < N                          # there are ties
    q = [0.0251, 0.5003, 0.9751]                                 # q N is no integer: no cumulative weight sits on a threshold
    assert all(v * N != np.floor(v * N) for v in q)
    got = gpu.posterior.quantiles(np.ascontiguousarray(Xs.T), W, q)
    qref = qr.reference(Xs.T, W, q, qr.default_rules(q))
    assert not qref["ambiguous"].any()
    assert np.array_equal(got, qref["want"]), (got, qref["want"])
    for d in range(3):                                           # ... and each is an order statistic of the column
        assert np.all(np.isin(got[:, d], Xs[:, d])) and got[0, d] < got[1, d] < got[2, d]
    # start(): chains drawn from an importance-weighted set
    Xi = rr.from_unit(np.random.default_rng(1).random((2000, 3)), TOY_LO, TOY_HI, TOY_LG)
    LLi = mr.e2e_loglik(Xi)
    Xs0, Us0, LLs0 = gpu.mcmc.start(Xi, LLi, 64, TOY_LO, TOY_HI, TOY_LG)
    assert Xs0.shape == (64, 3) and Us0.shape == (64, 3) and LLs0.shape == (64,)
    assert np.array_equal(LLs0, mr.e2e_loglik(Xs0)) and np.all(LLs0 > np.median(LLi))
    assert np.max(np.abs(Us0 - rr.unit_coords(Xs0, TOY_LO, TOY_HI, TOY_LG)[0])) <= 4 * 2.0 ** -47
