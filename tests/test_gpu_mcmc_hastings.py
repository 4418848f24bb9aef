"""The Metropolis-Hastings kernels on the device (trpl_mcmc_propose_stretch, trpl_mcmc_accept_h, trpl_mcmc_levels_h,
trpl_mcmc_prior_term; csrc/mcmc_hastings.hip) against tests/mcmc_hastings_ref.py, and run / run_tempered with kind="stretch" and
prior=.

Bits: Up, inside, z, h_out, `accepted`, the updated U / X / LL and every level equal the restatement bit for bit.  The one operation
numpy cannot restate is the device library's log (tests/test_gpu_cut_levels.py has the measurement), so the accept rule and the level
rule are handed log(xi) from the device's library (torch.log on the GPU: plumbing) and every other operation is numpy's.  Xp is, bit
for bit, the X that the existing propose kernel forms from the same Up (the same device expressions), and the restatement's within
tests/test_gpu_mcmc.py's rule for the columns.  lnq is held to (A - 1) numpy.log(z) within the bound derived at LNQ_ULPS."""
import numpy as np
import pytest

import mcmc_hastings_ref as hr
import mcmc_ref as mr
import refine_ref as rr
from test_gpu_mcmc import _check_columns, _cuda, _same_bits

pytestmark = pytest.mark.gpu
STEP = 5


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


def _device_log(torch, xi):
    with np.errstate(divide="ignore"):
        want = np.log(xi)
    lx = torch.log(torch.from_numpy(xi).cuda()).cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(lx[~fin], want[~fin]) and (np.abs(lx[fin] - want[fin]) <= 2.0 * np.spacing(np.abs(want[fin]))).all()
    return lx


def _lnq_bound(A, z):
    """LNQ_ULPS, derived: the device's log(z) and numpy's are each within one ulp of the true logarithm (the documented bound of both
    libraries), so they differ by at most 2 ulp of log(z); the factor (A - 1) scales that difference exactly, and each product is
    then rounded once, half an ulp of the product each.  |lnq - (A - 1) numpy.log(z)| <= (A - 1) 2 ulp(log z) + ulp(product)."""
    l = np.log(z)
    return (A - 1) * 2.0 * np.spacing(np.abs(l)) + np.spacing(np.abs((A - 1) * l))


@pytest.mark.parametrize("count,A,K,group,chain0", hr.DEVICE_SHAPES)
def test_the_four_kernels_equal_the_restatement(gpu, torch_dev, count, A, K, group, chain0):
    torch, dev = torch_dev
    m = gpu.mcmc
    lo, hi, lg = hr.device_box(A)
    ncol = lo.size
    U, partners, X, LL, Up_c, Xp_c, LLp, inside_c, h = hr.device_case(count, A, K, chain0)
    ladder = hr.DEVICE_LADDER[:K]
    seed = hr.DEVICE_SEED

    # ---- the stretch
    a = 2.0 if A != 3 else 3.5
    Up, Xp, inside, z, lnq = m.propose_stretch(U, partners, group, a, chain0, seed, STEP, lo, hi, lg)
    want_Up, want_in, want_z, row = hr.stretch_unit(U, partners, group, a, chain0, seed, STEP)
    assert _same_bits(Up, want_Up) and np.array_equal(inside, want_in) and _same_bits(z, want_z)
    assert np.array_equal(row // group, np.arange(count) // group)
    _, X_same, _ = m.propose(Up, None, 0.0, 0.0, chain0, seed, STEP, lo, hi, lg)     # u + 0 (2 xi - 1): the existing kernel's X of Up
    assert _same_bits(Xp, X_same)
    _check_columns(Xp, rr.from_unit(want_Up, lo, hi, lg, 0), lo, hi, lg, 0)
    bound = _lnq_bound(A, z)
    assert np.all(np.abs(lnq - (A - 1) * np.log(z)) <= bound), float(np.max(np.abs(lnq - (A - 1) * np.log(z)) / np.maximum(bound, 1e-300)))
    if A == 1:
        assert _same_bits(lnq, np.zeros(count))
    d = dict(Up=torch.full((count, A), -7.0, dtype=torch.float64, device="cuda"), Xp=torch.full((count, ncol), -7.0, dtype=torch.float64, device="cuda"),
             inside=torch.full((count,), -7, dtype=torch.int32, device="cuda"), z=torch.full((count,), -7.0, dtype=torch.float64, device="cuda"),
             lnq=torch.full((count,), -7.0, dtype=torch.float64, device="cuda"))
    dev.mcmc_propose_stretch_device(_cuda(torch, U), _cuda(torch, partners), group, a, chain0, seed, STEP, lo, hi, lg, d["Up"], d["Xp"],
                                    d["inside"], d["z"], d["lnq"])
    torch.cuda.synchronize()
    for name, host in (("Up", Up), ("Xp", Xp), ("z", z), ("lnq", lnq)):
        assert _same_bits(d[name].cpu().numpy(), host), name
    assert np.array_equal(d["inside"].cpu().numpy(), inside)

    # ---- the prior term
    mean, sd = np.linspace(0.1, 0.9, A), np.where(np.arange(A) % 3 == 1, np.inf, 0.05 + 0.1 * np.arange(A))
    for h_in in (None, h):
        got = m.prior_term(U, Up, mean, sd, h_in)
        assert _same_bits(got, hr.prior_term(U, Up, mean, sd, h_in))
        out = torch.full((count,), -7.0, dtype=torch.float64, device="cuda")
        dev.mcmc_prior_term_device(_cuda(torch, U), _cuda(torch, Up), mean, sd, out, None if h_in is None else _cuda(torch, h_in))
        torch.cuda.synchronize()
        assert _same_bits(out.cpu().numpy(), got)
    assert _same_bits(m.prior_term(U, Up * np.nan, mean, np.full(A, np.inf)), np.zeros(count))

    # ---- accept and levels with h, on the accept case of mcmc_ref
    lx = _device_log(torch, mr.accept_uniform(count, chain0, seed, STEP))
    want_U, want_X, want_LL, want_acc = hr.accept_h(U, X, LL, Up_c, Xp_c, LLp, inside_c, h, ladder, chain0, seed, STEP, lx=lx)
    gU, gX, gLL = U.copy(), X.copy(), LL.copy()
    acc = m.accept_h(gU, gX, gLL, Up_c, Xp_c, LLp, inside_c, h, ladder, chain0, seed, STEP)
    assert np.array_equal(acc, want_acc) and _same_bits(gU, want_U) and _same_bits(gX, want_X) and _same_bits(gLL, want_LL)
    dU, dX, dLL = _cuda(torch, U), _cuda(torch, X), _cuda(torch, LL)
    dacc = torch.full((count,), -7, dtype=torch.int32, device="cuda")
    dev.mcmc_accept_h_device(dU, dX, dLL, _cuda(torch, Up_c), _cuda(torch, Xp_c), _cuda(torch, LLp), _cuda(torch, inside_c), _cuda(torch, h),
                             ladder, chain0, seed, STEP, dacc)
    torch.cuda.synchronize()
    assert np.array_equal(dacc.cpu().numpy(), acc) and _same_bits(dU.cpu().numpy(), gU) and _same_bits(dX.cpu().numpy(), gX)
    assert _same_bits(dLL.cpu().numpy(), gLL)
    level = m.reject_levels_h(LL, h, ladder, chain0, seed, STEP)
    assert level.tobytes() == hr.levels_h(LL, h, ladder, chain0, seed, STEP, lx=lx).tobytes()
    dlev = torch.full((count,), -7.0, dtype=torch.float64, device="cuda")
    dev.mcmc_levels_h_device(_cuda(torch, LL), _cuda(torch, h), ladder, chain0, seed, STEP, dlev)
    torch.cuda.synchronize()
    assert dlev.cpu().numpy().tobytes() == level.tobytes()
    # the edge values of h, by their rows: NaN and -inf never move and NaN, -inf, +inf give no level
    assert not acc[np.isnan(h) | (h == -np.inf)].any() and np.all(level[~np.isfinite(h)] == np.inf)
    if count >= 256:
        assert np.isnan(h).any() and (h == -np.inf).any() and (h == np.inf).any() and (np.signbit(h) & (h == 0.0)).any()
        valid = (inside_c != 0) & np.isfinite(LLp) & np.isfinite(LL)
        assert acc[valid & (h == np.inf)].all() and np.isfinite(level).any()
    # what the levels are for: accept_h rejects whatever a proposal cut at them can report
    fin = np.isfinite(level)
    cur = LL.copy()
    acc2 = m.accept_h(U.copy(), X.copy(), cur, Up_c, Xp_c, np.where(fin, -level, -np.inf), np.ones(count, dtype=np.int32), h, ladder, chain0,
                      seed, STEP)
    assert not acc2[fin].any() and _same_bits(cur[fin], LL[fin])


@pytest.mark.parametrize("count,A,K,group,chain0", hr.DEVICE_SHAPES)
def test_a_zero_h_is_the_rung_kernels(gpu, count, A, K, group, chain0):
    m = gpu.mcmc
    U, _, X, LL, Up_c, Xp_c, LLp, inside_c, _ = hr.device_case(count, A, K, chain0)
    ladder = hr.DEVICE_LADDER[:K]
    for zero in (0.0, -0.0):
        h = np.full(count, zero)
        a, b = (U.copy(), X.copy(), LL.copy()), (U.copy(), X.copy(), LL.copy())
        acc_h = m.accept_h(*a, Up_c, Xp_c, LLp, inside_c, h, ladder, chain0, hr.DEVICE_SEED, STEP)
        acc_r = m.accept_rungs(*b, Up_c, Xp_c, LLp, inside_c, ladder, chain0, hr.DEVICE_SEED, STEP)
        assert np.array_equal(acc_h, acc_r) and all(_same_bits(p, q) for p, q in zip(a, b))
        assert m.reject_levels_h(LL, h, ladder, chain0, hr.DEVICE_SEED, STEP).tobytes() \
            == m.reject_levels_rungs(LL, ladder, chain0, hr.DEVICE_SEED, STEP).tobytes()


def _equal_chains(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("U", "X", "LL", "accept"))


def test_a_flat_prior_is_the_plain_run_and_a_ladder_of_one_is_run(gpu):
    m = gpu.mcmc
    C, sweeps, seed = 16, 10, 4
    U0 = mr.toy_start(C, seed)
    X0 = rr.from_unit(U0, mr.E2E_LO, mr.E2E_HI, mr.E2E_LG)
    LL0 = mr.e2e_loglik(X0)
    box = (mr.E2E_LO, mr.E2E_HI, mr.E2E_LG)
    flat = (np.full(3, 0.5), np.full(3, np.inf))
    for kw in (dict(kind="de"), dict(kind="de", bounds="fold"), dict(kind="rw", scale=0.05)):
        plain = m.run(mr.e2e_loglik, X0, LL0, *box, sweeps=sweeps, seed=seed, U0=U0, tf=1.5, **kw)
        assert _equal_chains(m.run(mr.e2e_loglik, X0, LL0, *box, sweeps=sweeps, seed=seed, U0=U0, tf=1.5, prior=flat, **kw), plain)
        assert plain.accept.any()
    info = {}
    one = m.run(mr.e2e_loglik, X0, LL0, *box, sweeps=sweeps, seed=seed, U0=U0, tf=1.5, kind="stretch", stretch_a=2.5, info=info)
    assert info["stretch_a"] == 2.5 and one.accept.any() and not one.accept.all()
    t = m.run_tempered(mr.e2e_loglik, X0, LL0, *box, [1.5], sweeps=sweeps, seed=seed, U0=U0, kind="stretch", stretch_a=2.5)
    assert _equal_chains(t.rung(0), one)
    # three rungs with a prior: it runs, every rung moves, and the prior is felt (a narrow one around 0.3 pulls the cold rung there)
    prior = (np.full(3, 0.3), np.full(3, 0.01))
    t3 = m.run_tempered(mr.e2e_loglik, X0, LL0, *box, [1.0, 4.0, 16.0], sweeps=200, seed=seed, U0=U0, kind="stretch", prior=prior)
    assert all(t3.rung(k).accept.any() for k in range(3)) and abs(t3.rung(0).U[-1].mean() - 0.3) < 0.05


def test_the_stretch_toy(gpu):
    """3-D Gaussian with correlation 0.99 in the unit cube, 256 chains x 400 sweeps from over-dispersed starts, the second half kept.
    Mean, deviation and correlation (averaged over the coordinates and the pairs) within the mean +- 5 sd of the restatement's eight
    seeds (tests/mcmc_hastings_ref.py STRETCH_STATS, taken on the CPU; stretch_gates() has the intervals: (0.4879, 0.5116),
    (0.0762, 0.0842), (0.98861, 0.99154)).  The move without its Hastings term has a deviation of 0.0575, outside
    (tests/test_mcmc_hastings_host.py).  R-hat is recorded."""
    t = hr.STRETCH_TOY
    loglik, _ = mr.toy(t["rho"])
    U0 = mr.toy_start(t["C"], hr.STRETCH_DEVICE_SEED)
    info = {}
    ch = gpu.mcmc.run(loglik, U0, loglik(U0), *mr.CUBE, sweeps=t["sweeps"], seed=hr.STRETCH_DEVICE_SEED, U0=U0, kind="stretch", info=info)
    got = np.array(hr.toy_stats(ch.U[t["sweeps"] // 2:]))
    lo, hi = hr.stretch_gates()
    rhat = ch.rhat(burn=t["sweeps"] // 2)
    print("stretch toy: mean %.5f deviation %.5f correlation %.5f; acceptance %.3f, outside %.4f, worst split-R-hat %.4f"
          % (got[0], got[1], got[2], float(np.mean(info["accept"])), info["outside"], float(rhat.max())))
    assert np.all((lo < got) & (got < hi)), (got, lo, hi)
    assert np.all(np.isfinite(rhat))


@pytest.mark.parametrize("bounds", ("reject", "fold"))
def test_the_prior_toy(gpu, bounds):
    """A flat likelihood and the prior N(0, 0.2^2) on the first coordinate, centred on the face u = 0: the posterior is the
    half-Gaussian, E u = 0.2 sqrt(2 / pi), E u^2 = 0.04.  Both moments of the kept half within 5 standard errors, the standard
    error by batch means (mcmc_hastings_ref.prior_gate)."""
    t = hr.PRIOR_TOY
    U0 = np.random.default_rng([t["seed"], 1]).random((t["C"], 2))
    info = {}
    ch = gpu.mcmc.run(hr.flat_loglik, U0, np.zeros(t["C"]), *hr.PRIOR_BOX, sweeps=t["sweeps"], seed=t["seed"], U0=U0, kind="de", prior=hr.PRIOR,
                      bounds=bounds, info=info)
    kept = ch.U[t["sweeps"] // 2:, :, 0]
    for series, truth in ((kept.mean(axis=1), hr.PRIOR_M1), ((kept ** 2).mean(axis=1), hr.PRIOR_M2)):
        err, gate = hr.prior_gate(series, truth)
        print("prior toy bounds=%s: moment %.5f, truth %.5f, off by %.2e (gate %.2e); acceptance %.3f, outside %.3f, folded %.3f"
              % (bounds, series.mean(), truth, err, gate, float(np.mean(info["accept"])), info["outside"], info["folded"]))
        assert err < gate
    assert (info["folded"] > 0.0) == (bounds == "fold")


@pytest.mark.parametrize("kernel", ["single", "pair"])
@pytest.mark.parametrize("move", ["stretch", "de_prior"])
def test_early_rejection_leaves_the_chain_unchanged(gpu, oracle, move, kernel):
    """The small fused-likelihood problem of tests/test_gpu_mcmc_early_reject.py: with a Hastings term in the accept step the run with
    early_reject=True is the run without it, bit for bit, and proposals are cut."""
    from test_gpu_mcmc_early_reject import CHAINS, DT, L, SEED, SWEEPS, T, TF, _problem
    ini, lens, X0, obs, (lo, hi, lg) = _problem(gpu, oracle)

    def likelihood(work):
        def f(X, cut_levels=None):
            info = {}
            P = gpu.loglik(X, ini, lens, T * DT, L, T, obs, kernel=kernel, info=info, cut_levels=cut_levels)
            work["solved"] += len(X)
            if cut_levels is not None:
                work["cut"] += int((info["cut_col"] >= 0).any(axis=0).sum())
            return P
        return f

    LL0 = likelihood(dict(solved=0, cut=0))(X0)
    if move == "stretch":
        kw = dict(kind="stretch")
    else:                                                        # the first chain's mobilities known to 20 %, the rest flat
        w = np.full(lo.size, np.inf)
        w[[2, 3]] = 0.2 * X0[0, [2, 3]]
        kw = dict(kind="de", prior=gpu.mcmc.gaussian_prior(X0[0], w, lo, hi, lg))
        assert np.isfinite(kw["prior"][1]).any()
    runs = {}
    for early in (False, True):
        work, info = dict(solved=0, cut=0), {}
        runs[early] = (gpu.mcmc.run(likelihood(work), X0, LL0, lo, hi, lg, sweeps=SWEEPS, tf=TF, seed=SEED, info=info, early_reject=early, **kw),
                       work, info)
    (plain, w0, i0), (fast, w1, i1) = runs[False], runs[True]
    print("move=%s kernel=%s: acceptance %.3f, %d proposals solved, %d cut (%.3f levelled)"
          % (move, kernel, float(np.mean(i0["accept"])), w1["solved"], w1["cut"], i1["early_reject"]))
    assert _equal_chains(fast, plain) and i1["accept"] == i0["accept"] and i1["outside"] == i0["outside"]
    assert w1["solved"] == w0["solved"] > 0 and w1["cut"] >= 1 and w0["cut"] == 0
    assert CHAINS == plain.U.shape[1]
