"""mcmc.run(early_reject=True) on the fused likelihood (include/trpl.h, trpl_mcmc_levels and trpl_loglik_cut_levels): the chain
is the chain of the run without it, bit for bit -- every state, every likelihood, every accept flag -- while proposals are cut and
fewer solver iterations are paid for.  The problem is small: Power_scan, 32 chains, 6 sweeps, 201 observations per curve on the
grid (three full batches and a partial one), synthesised by the CPU oracle at the reference's marked point.  The first 16 chains
start in a tight cluster around that point (their sse is tiny, so their level is about tf |log xi|), the other 16 on a seeded sample
of the default box: a differential-evolution proposal of a cluster chain is the difference of two box samples away, far worse in
every curve, and is cut in its first batches -- a curve's level is the chain's TOTAL sse plus slack, so a cut needs one curve alone
above it (first version of this test: all chains on box samples against straight-line observations, every curve about as wrong as
the others, acceptance independent of tf and not one cut in 192 proposals)."""
import numpy as np
import pytest

from gpu_common import DT

pytestmark = pytest.mark.gpu

CHAINS, SWEEPS, T, L, SEED = 32, 6, 200, 128, 7
TF = 1.0
_CACHE = {}


def _problem(gpu, oracle):
    if _CACHE:
        return _CACHE["p"]
    w, sm = gpu.workloads, gpu.sampler
    ini, lens = w.power_scan(L)
    lo, hi, lg = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS, sm.DEFAULT_DO_LOG
    mark = (w.MARKED_POINT * gpu.UNIT_CONVERSIONS)[None, :]
    obs = [np.log10(oracle.pvsim(np.ascontiguousarray(mark[:, :-1]), lens[c], T * DT, L, T, ini[c])["plI"][0]) for c in range(len(lens))]
    U_mark, _ = gpu.refine.unit_coords(np.ascontiguousarray(mark), lo, hi, lg)
    _, cluster, inside = gpu.mcmc.propose(np.repeat(U_mark, CHAINS // 2, axis=0), None, 0.0, 0.002, 0, SEED, 0xFFFF, lo, hi, lg)
    assert inside.all()                                       # the marked point lies inside the box, not on a face
    X0 = np.ascontiguousarray(np.concatenate([cluster, w.samples(CHAINS // 2, seed=29)]))
    _CACHE["p"] = (ini, lens, X0, obs, (lo, hi, lg))
    return _CACHE["p"]


@pytest.mark.parametrize("kernel", ["single", "pair"])
@pytest.mark.parametrize("bounds", ["reject", "fold"])
def test_the_chain_is_unchanged_and_proposals_are_cut(gpu, oracle, bounds, kernel):
    ini, lens, X0, obs, (lo, hi, lg) = _problem(gpu, oracle)

    def likelihood(work):
        def f(X, cut_levels=None):
            info = {}
            P = gpu.loglik(X, ini, lens, T * DT, L, T, obs, kernel=kernel, info=info, cut_levels=cut_levels)   # P from zero
            work["iters"] += int(info["iters_total"].sum())
            work["solved"] += len(X)
            if cut_levels is not None:
                assert cut_levels.shape == (len(X),)
                work["cut"] += int((info["cut_col"] >= 0).any(axis=0).sum())
            return P
        return f

    LL0 = likelihood(dict(iters=0, solved=0, cut=0))(X0)
    runs = {}
    for early in (False, True):
        work, info = dict(iters=0, solved=0, cut=0), {}
        ch = gpu.mcmc.run(likelihood(work), X0, LL0, lo, hi, lg, sweeps=SWEEPS, tf=TF, seed=SEED, bounds=bounds, info=info,
                          **({"early_reject": True} if early else {}))
        runs[early] = (ch, work, info)
    (plain, w0, i0), (fast, w1, i1) = runs[False], runs[True]
    print("bounds=%s kernel=%s: acceptance %.3f, %d proposals solved, %d cut (%.3f levelled), iterations %d -> %d (%.3f)"
          % (bounds, kernel, float(np.mean(i0["accept"])), w1["solved"], w1["cut"], i1["early_reject"], w0["iters"], w1["iters"],
             w1["iters"] / float(w0["iters"])))
    for k in ("U", "X", "LL", "accept"):
        assert getattr(fast, k).tobytes() == getattr(plain, k).tobytes(), k
    assert i1["accept"] == i0["accept"] and i1["outside"] == i0["outside"] and i1["folded"] == i0["folded"]
    assert "early_reject" not in i0 and w1["solved"] == w0["solved"] > 0
    assert w1["cut"] >= 1 and w0["cut"] == 0
    assert w1["iters"] < w0["iters"]
    assert plain.accept.mean() < 1.0                              # chains refused
    # a cut proposal's reported likelihood was never stored: every kept LL is a full solve's
    full = gpu.loglik(np.ascontiguousarray(fast.X[-1]), ini, lens, T * DT, L, T, obs, kernel=kernel)
    assert np.array_equal(full, fast.LL[-1])


def test_a_callable_without_the_keyword_is_an_error(gpu, oracle):
    ini, lens, X0, obs, (lo, hi, lg) = _problem(gpu, oracle)
    with pytest.raises(TypeError):
        gpu.mcmc.run(lambda X: np.zeros(len(X)), X0, np.zeros(CHAINS), lo, hi, lg, sweeps=1, seed=SEED, bounds="fold",
                     early_reject=True)
