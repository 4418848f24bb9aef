"""The subspace differential-evolution proposal on the device (trpl_mcmc_propose_subspace; csrc/mcmc_subspace.hip) against
tests/mcmc_subspace_ref.py, and run / run_tempered with kind="subspace".

Bits: Up, inside, mask and sel equal the restatement bit for bit, in the host-buffer and the _dev form.  Xp is, bit for bit, the X
that the existing propose kernel forms from the same Up (the same device expressions), and the restatement's within
tests/test_gpu_mcmc.py's rule for the columns (a log column goes through the device's pow).  At the anchor setting every output is
trpl_mcmc_propose_rungs'.  The move keeps the uniform distribution under a flat likelihood and samples a correlated 10-D Gaussian;
early rejection, a ladder of one and a flat prior change no bit of a run."""
import numpy as np
import pytest

import mcmc_ref as mr
import mcmc_subspace_ref as sr
import refine_ref as rr
from test_gpu_mcmc import _box_for, _check_columns, _cuda, _same_bits
from test_mcmc_fold_host import CHI2_GATE, FLAT, _chi2

pytestmark = pytest.mark.gpu
STEP, SEED = 5, (0x1234567 << 32) | 0x89abcdef
HI = (1 << 32) + 5                                               # a chain0 whose counter uses its high word
BLOCK = 256
PCR = np.array([0.6, 0.1, 0.3])


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


def _states(rng, count, A, P):
    """Chains of which every third sits at the centre of the cube and some sit at its faces, partners in [0.4, 0.6]: a proposal of a
    centred chain stays inside, one of a chain at a face leaves the cube or is folded."""
    U = rng.random((count, A))
    U[::5] = np.where(rng.random(U[::5].shape) < 0.5, 1e-4, 1.0 - 1e-4)
    U[2::3] = 0.5
    return U, 0.4 + 0.2 * rng.random((P, A))


def _dev_form(torch_dev, U, partners, group, tab, scale, chain0, lo, hi, lg, ncr, pcr, e_width, flags):
    torch, dev = torch_dev
    count, A = U.shape
    Up = torch.full((count, A), -7.0, dtype=torch.float64, device="cuda")
    Xp = torch.full((count, lo.size), -7.0, dtype=torch.float64, device="cuda")
    inside, mask, sel = (torch.full((count,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    dev.mcmc_propose_subspace_device(_cuda(torch, U), _cuda(torch, partners), group, tab, scale, chain0, SEED, STEP, lo, hi, lg, Up, Xp, inside,
                                     mask, sel, ncr=ncr, pcr=pcr, e_width=e_width, flags=flags)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (Up, Xp, inside, mask, sel))


def _one_case(gpu, torch_dev, U, partners, group, pairs, ncr, pcr, fold, chain0, lo, hi, lg, flags, scale, sim=None):
    """Both forms against the restatement; returns the codes of `inside`."""
    A = U.shape[1]
    tab = sr.gamma_table(pairs, A)
    want = sr.propose(U, partners, group, tab, scale, chain0, SEED, STEP, lo, hi, lg, ncr, pcr, 0.2, flags, fold)
    got = gpu.mcmc.propose_subspace(U, partners, group, tab, scale, chain0, SEED, STEP, lo, hi, lg, ncr, pcr, 0.2, sim, fold=fold)
    where = (U.shape, group, pairs, ncr, pcr is not None, fold)
    assert _same_bits(got[0], want[0]), where
    for j in (2, 3, 4):
        assert got[j].dtype == np.int32 and np.array_equal(got[j], want[j]), (j, where)
    _, X_same, _ = gpu.mcmc.propose(got[0], None, 0.0, 0.0, chain0, SEED, STEP, lo, hi, lg, sim)   # u + 0 (2 xi - 1): the existing kernel's X of Up
    assert _same_bits(got[1], X_same), where
    _check_columns(got[1], want[1], lo, hi, lg, flags)
    dev = _dev_form(torch_dev, U, partners, group, tab, scale, chain0, lo, hi, lg, ncr, pcr, 0.2, flags | (gpu._abi.MCMC_FOLD if fold else 0))
    assert _same_bits(dev[0], got[0]) and _same_bits(dev[1], got[1]), where
    assert all(np.array_equal(dev[j], got[j]) for j in (2, 3, 4)), where
    return got


@pytest.mark.parametrize("A", (1, 2, 10, 16))
def test_both_forms_equal_the_restatement(gpu, torch_dev, A):
    rng = np.random.default_rng(A)
    lo, hi, lg = _box_for(A, 0, rng)
    assert rr.active_columns(lo, hi, 0).size == A and (A == 1 or lg.any())
    scale = rng.uniform(0.01, 0.05, A)
    codes, deltas, classes, fallback = {False: set(), True: set()}, set(), set(), 0
    for count in (1, BLOCK + 44):
        for group in (2, 3, max(count, 2)):
            P = max(3 * group, -(-count // group) * group)       # three rungs at least, and a rung for every chain
            U, partners = _states(rng, count, A, P)
            for pairs in (1, 4):
                for ncr, pcr in ((1, None), (3, None), (3, PCR)):
                    for fold in (False, True):
                        got = _one_case(gpu, torch_dev, U, partners, group, pairs, ncr, pcr, fold, HI, lo, hi, lg, 0, scale)
                        codes[fold] |= set(got[2].tolist())
                        deltas |= set((got[4] & 0xFF).tolist())
                        classes |= set((got[4] >> 8).tolist())
                        if ncr == 1:
                            assert np.all(got[3] == (1 << A) - 1)
                        fallback += int(((got[3] & (got[3] - 1)) == 0).sum())
    assert codes[False] == {0, 1} and codes[True] == {1, 2}       # both outcomes of the range test, both fold codes
    assert deltas == {1, 2, 3, 4} and classes == {0, 1, 2} and fallback > 0
    # the low counter word: chain0 = 0 is another stream, and a second call gives the same bits
    U, partners = _states(rng, BLOCK + 44, A, 2 * BLOCK)
    a = _one_case(gpu, torch_dev, U, partners, BLOCK, 4, 3, PCR, True, 0, lo, hi, lg, 0, scale)
    b = _one_case(gpu, torch_dev, U, partners, BLOCK, 4, 3, PCR, True, HI, lo, hi, lg, 0, scale)
    c = _one_case(gpu, torch_dev, U, partners, BLOCK, 4, 3, PCR, True, HI, lo, hi, lg, 0, scale)
    assert not _same_bits(a[0], b[0]) and _same_bits(b[0], c[0]) and np.array_equal(b[3], c[3])


def test_the_overrides_of_the_box_apply(gpu, torch_dev):
    A, flags = 7, 7
    rng = np.random.default_rng(77)
    lo, hi, lg = _box_for(A, flags, rng)
    assert rr.active_columns(lo, hi, flags).size == A and np.any(lo == hi) and lo.size >= 9
    sim = {"override_equal_mu": True, "override_equal_s": True, "override_equal_auger": True}
    U, partners = _states(rng, BLOCK + 44, A, 2 * BLOCK)
    for fold in (False, True):
        _one_case(gpu, torch_dev, U, partners, BLOCK, 4, 3, PCR, fold, HI, lo, hi, lg, flags, rng.uniform(0.01, 0.05, A), sim)


@pytest.mark.parametrize("A", (1, 2, 10, 16))
def test_the_anchor_is_propose_rungs_bit_for_bit(gpu, A):
    """ncr = 1, one pair, e_width = 0 and a table filled with gamma: trpl_mcmc_propose_rungs' outputs, folded and not."""
    rng = np.random.default_rng(100 + A)
    lo, hi, lg = _box_for(A, 0, rng)
    scale, gamma = rng.uniform(0.01, 0.05, A), 0.6
    for count in (1, BLOCK + 44):
        for group in (2, 3, max(count, 2)):
            P = max(3 * group, -(-count // group) * group)
            U, partners = _states(rng, count, A, P)
            for fold in (False, True):
                want = gpu.mcmc.propose_rungs(U, partners, group, gamma, scale, HI, SEED, STEP, lo, hi, lg, fold=fold)
                got = gpu.mcmc.propose_subspace(U, partners, group, np.full((1, A), gamma), scale, HI, SEED, STEP, lo, hi, lg, 1, None, 0.0,
                                                fold=fold)
                assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]), (count, group, fold)
                assert np.all(got[3] == (1 << A) - 1) and np.all(got[4] == 1)


def test_a_flat_likelihood_keeps_the_uniform_distribution(gpu):
    """bounds="fold" under a flat likelihood: every proposal is accepted, so the chains are the proposal's own walk, and the pooled
    coordinates stay uniform -- tests/test_mcmc_fold_host.py's chi-square gate (20 bins, 19 degrees of freedom, tail 1e-6) on every
    coordinate.  gamma = 2 makes the jumps long enough to be folded often."""
    lo, hi, lg = mr.CUBE
    C = 256
    U0 = mr.toy_start(C, 11)
    info = {}
    ch = gpu.mcmc.run(lambda X: np.zeros(X.shape[0]), U0, np.zeros(C), lo, hi, lg, sweeps=FLAT["sweeps"], seed=11, bounds="fold", kind="subspace",
                      gamma=2.0, U0=U0, info=info)
    assert np.all(np.array(info["accept"]) == 1.0) and info["outside"] == 0 and info["folded"] > 0.05
    chi = _chi2(dict(U=ch.U))
    print("flat, subspace: chi-square per dimension %s, gate %.2f; folded %.3f, mean dsel %.2f" % (chi, CHI2_GATE, info["folded"], info["mean_dsel"]))
    assert chi.shape == (3,) and np.all(chi < CHI2_GATE), chi
    assert 1.0 < info["mean_dsel"] < 3.0 and info["pairs"] == 3 and info["ncr"] == 3 and info["pcr"] == [1 / 3, 1 / 3, 1 / 3]


def test_the_correlated_ten_dimensional_gaussian(gpu):
    """256 chains on the 10-D Gaussian of tests/mcmc_subspace_ref.py, coordinates 0 and 1 correlated at 0.9: the ten means, the ten
    deviations and that correlation over the kept sweeps lie within the mean +- 5 standard deviations of the numpy restatement's own
    runs over 8 seeds (mcmc_subspace_ref.ten_gates, computed here on the CPU; tests/test_mcmc_subspace_host.py holds the truth to the
    same gates)."""
    lo, hi = sr.ten_gates()
    U0, LL0 = sr.ten_start(sr.TEN_DEVICE_SEED)
    info = {}
    ch = gpu.mcmc.run(sr.ten_loglik, U0, LL0, *sr.TEN_BOX, sweeps=sr.TEN_SWEEPS, seed=sr.TEN_DEVICE_SEED, bounds="fold", kind="subspace", U0=U0,
                      burn=sr.TEN_BURN, info=info)
    got = sr.ten_stats(ch.U)
    print("10-D toy, subspace: acceptance %.3f, folded %.4f, mean dsel %.2f; means %s deviations %s correlation %.4f"
          % (float(np.mean(info["accept"])), info["folded"], info["mean_dsel"], np.array2string(got[:10], precision=4),
             np.array2string(got[10:20], precision=4), got[20]))
    assert ch.U.shape == (sr.TEN_SWEEPS - sr.TEN_BURN, sr.TEN_C, sr.TEN_A)
    assert np.all((lo < got) & (got < hi)), (got, lo, hi)


def _equal_chains(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("U", "X", "LL", "accept"))


@pytest.mark.parametrize("kernel", ["single", "pair"])
@pytest.mark.parametrize("bounds", ["reject", "fold"])
def test_early_rejection_leaves_the_chain_unchanged(gpu, oracle, bounds, kernel):
    """The small fused-likelihood problem of tests/test_gpu_mcmc_early_reject.py: kind="subspace" with early_reject=True and with
    early_reject="sample" is the run without either, bit for bit."""
    from test_gpu_mcmc_early_reject import CHAINS, DT, L, SEED as ER_SEED, SWEEPS, T, TF, _problem
    ini, lens, X0, obs, (lo, hi, lg) = _problem(gpu, oracle)

    def likelihood(work):
        def f(X, cut_levels=None, cut_budget=None):
            info = {}
            P = gpu.loglik(X, ini, lens, T * DT, L, T, obs, kernel=kernel, info=info, cut_levels=cut_levels, cut_budget=cut_budget)
            work["solved"] += len(X)
            if cut_levels is not None or cut_budget is not None:
                work["cut"] += int((info["cut_col"] >= 0).any(axis=0).sum())
            return P
        return f

    LL0 = likelihood(dict(solved=0, cut=0))(X0)
    runs = {}
    for early in (False, True, "sample"):
        work, info = dict(solved=0, cut=0), {}
        runs[early] = (gpu.mcmc.run(likelihood(work), X0, LL0, lo, hi, lg, sweeps=SWEEPS, tf=TF, seed=ER_SEED, bounds=bounds, kind="subspace",
                                    info=info, early_reject=early), work, info)
    plain, w0, i0 = runs[False]
    for early in (True, "sample"):
        fast, w1, i1 = runs[early]
        print("subspace bounds=%s kernel=%s early_reject=%r: acceptance %.3f, %d proposals solved, %d cut (%.3f levelled), mean dsel %.2f"
              % (bounds, kernel, early, float(np.mean(i0["accept"])), w1["solved"], w1["cut"], i1["early_reject"], i1["mean_dsel"]))
        assert _equal_chains(fast, plain) and i1["accept"] == i0["accept"] and i1["outside"] == i0["outside"] and i1["folded"] == i0["folded"]
        assert w1["solved"] == w0["solved"] > 0 and w0["cut"] == 0
    assert CHAINS == plain.U.shape[1] and "early_reject" not in i0


def test_a_ladder_of_one_is_run_and_a_flat_prior_changes_no_bit(gpu):
    m = gpu.mcmc
    C, sweeps, seed = 16, 10, 4
    U0 = mr.toy_start(C, seed)
    X0 = rr.from_unit(U0, mr.E2E_LO, mr.E2E_HI, mr.E2E_LG)
    LL0 = mr.e2e_loglik(X0)
    box = (mr.E2E_LO, mr.E2E_HI, mr.E2E_LG)
    flat = (np.full(3, 0.5), np.full(3, np.inf))
    for kw in (dict(), dict(bounds="fold", pairs=4, ncr=2, e_width=0.3), dict(jump_every=3), dict(adapt_cr=True, burn=4, bounds="fold")):
        info = {}
        one = m.run(mr.e2e_loglik, X0, LL0, *box, sweeps=sweeps, seed=seed, U0=U0, tf=1.5, kind="subspace", info=info, **kw)
        assert one.accept.any() and not one.accept.all() and 1.0 <= info["mean_dsel"] <= 3.0
        tinfo = {}
        t = m.run_tempered(mr.e2e_loglik, X0, LL0, *box, [1.5], sweeps=sweeps, seed=seed, U0=U0, kind="subspace", info=tinfo, **kw)
        assert _equal_chains(t.rung(0), one) and tinfo["pcr"] == info["pcr"] and tinfo["mean_dsel"] == info["mean_dsel"]
        assert _equal_chains(m.run(mr.e2e_loglik, X0, LL0, *box, sweeps=sweeps, seed=seed, U0=U0, tf=1.5, kind="subspace", prior=flat, **kw), one)
    # the run is the restatement's, sweep by sweep, where no decision is near its margin
    ref = sr.run(mr.e2e_loglik, U0, LL0, *box, sweeps=sweeps, seed=seed, tf=1.5)
    if ref["margin"] > mr.E2E_MARGIN:
        one = m.run(mr.e2e_loglik, X0, LL0, *box, sweeps=sweeps, seed=seed, U0=U0, tf=1.5, kind="subspace")
        assert _same_bits(one.U, ref["U"]) and np.array_equal(one.accept, ref["accepted"])
    # three rungs: every rung moves
    t3 = m.run_tempered(mr.e2e_loglik, X0, LL0, *box, [1.0, 4.0, 16.0], sweeps=20, seed=seed, U0=U0, kind="subspace", bounds="fold")
    assert all(t3.rung(k).accept.any() for k in range(3))
