"""trpl_loglik_cut_budget on the GPU (include/trpl.h): the early stop on a sample's total, a budget carried across the curves.
Checked against the numpy restatement of the rule (tests/cut_budget_ref.py) and against trpl_loglik_cut_levels on the same inputs
(which tests/test_gpu_cut_levels.py holds to the scalar call, and tests/test_gpu_cut.py that to the plain call) -- never against
figures of its own.  The problem is small: Power_scan's 3 curves, 12 samples, 201 observations per curve on the grid (three full
64-column batches and a ragged one) or 150 + 7 c sorted random times off it.  Each sample's budget is chosen from the plain call's
own sse: with R1 = sse_0, R2 = fl(R1 + sse_1), total = fl(R2 + sse_2),
    +inf | 0 | sse_0 / 2 | between R1 and R2 | exactly R1 | exactly total | the total's successor | between R2 and total (only the last
    curve passes it) | 0.3, 0.7, 0.9 and 1.5 of the total."""
import os

import numpy as np
import pytest

import cut_budget_ref as ref
from conftest import GOLDEN
from gpu_common import DT

pytestmark = pytest.mark.gpu

OUT = ("P", "sse", "cut_col", "status", "iters_total", "floor_col")
S, C, T = 12, 3, 200
CASES = [(128, "pair", False), (128, "pair", True), (128, "single", False), (128, "single", True), (32, "single", False),
         (32, "single", True)]
IDS = ["L%d-%s-%s" % (L, k, "times" if off else "grid") for L, k, off in CASES]
_PLAIN = {}


def _problem(gpu, L, offgrid):
    w = gpu.workloads
    ini, lens = w.power_scan(L)
    assert len(lens) == C
    X = w.samples(S, seed=17)
    if not offgrid:
        return X, ini, lens, None, [18.0 - 0.2 * DT * np.arange(T + 1) for _ in range(C)]
    rng = np.random.default_rng(5)
    times = [np.sort(rng.uniform(0.0, T * DT, 150 + 7 * c)) for c in range(C)]
    return X, ini, lens, times, [18.0 - 0.2 * t + 0.05 * rng.standard_normal(len(t)) for t in times]


def _run(gpu, case, X=None, **kw):
    L, kernel, offgrid = case
    X0, ini, lens, times, obs = _problem(gpu, L, offgrid)
    info = {}
    info["P"] = gpu.loglik(X0 if X is None else X, ini, lens, T * DT, L, T, obs, times=times, kernel=kernel, info=info, **kw)
    return info


def _plain(gpu, case):
    """The plain call of a case and the budgets chosen from its sse: computed once, shared, never changed."""
    if case not in _PLAIN:
        p = _run(gpu, case)
        sse = p["sse"]
        R1 = ref.carried(sse[:1])
        R2 = ref.carried(sse[:2])
        total = ref.carried(sse)
        assert np.array_equal(p["P"], -total) and np.isfinite(total).all() and (sse > 0.0).all() and not p["status"].any()
        B = np.empty(S)
        B[0], B[1], B[2] = np.inf, 0.0, 0.5 * sse[0, 2]
        B[3], B[4], B[5] = 0.5 * (R1[3] + R2[3]), R1[4], total[5]
        B[6], B[7] = np.nextafter(total[6], np.inf), 0.5 * (R2[7] + total[7])
        B[8:] = np.array([0.3, 0.7, 0.9, 1.5]) * total[8:]
        assert R1[3] < B[3] < R2[3] and R2[7] < B[7] < total[7]
        for a in (p["P"], sse, B, total):
            a.setflags(write=False)
        _PLAIN[case] = (p, B, total)
    return _PLAIN[case]


def _same(a, b, keys=OUT):
    for k in keys:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k


def _device_call(gpu, case, which, arg, g=None):
    """loglik_cut_budget_device (arg: the budget; also returns the levels) or loglik_cut_levels_device (arg: the levels)."""
    import torch
    L, kernel, offgrid = case
    X, ini, lens, times, obs = _problem(gpu, L, offgrid)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)          # a copy: the shared reference stays read-only
    n_obs = [len(o) for o in obs]
    ld = max(n_obs)
    pad = lambda rows, fill, dtype=np.float64: np.stack([np.concatenate([np.asarray(r, dtype=dtype), np.full(ld - len(r), fill, dtype=dtype)]) for r in rows])
    br = {}
    if offgrid:
        b = [gpu.driver.bracket_times(np.linspace(0, T * DT, T + 1), tc) for tc in times]
        br = dict(obs_hi=t(pad([x[0] for x in b], 1, np.int32)), obs_dx=t(pad([x[1] for x in b], 0.0)), obs_h=t(pad([x[2] for x in b], 1.0)))
    out = dict(P=torch.zeros(S, dtype=torch.float64, device=dev), sse=torch.empty((C, S), dtype=torch.float64, device=dev),
               cut_col=torch.empty((C, S), dtype=torch.int32, device=dev), status=torch.empty((C, S), dtype=torch.int32, device=dev),
               iters_total=torch.empty((C, S), dtype=torch.int64, device=dev), floor_col=torch.empty((C, S), dtype=torch.int32, device=dev))
    common = dict(cut_col=out["cut_col"], status=out["status"], iters_total=out["iters_total"], floor_col=out["floor_col"],
                  flags=gpu.FLAG_KERNEL_PAIR if kernel == "pair" else gpu.FLAG_KERNEL_SINGLE, **br)
    head = (t(X), t(ini), lens, T * DT, L, T, t(pad(obs, 0.0)), n_obs)
    if which == "budget":
        out["cut_level"] = torch.full((C, S), np.nan, dtype=torch.float64, device=dev)
        gpu.device.loglik_cut_budget_device(*head, t(arg), out["cut_level"], out["P"], out["sse"], curves_per_launch=g, **common)
    else:
        gpu.device.loglik_cut_levels_device(*head, t(arg), out["P"], out["sse"], **common)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_levels_are_the_rule_and_every_system_is_the_levels_call_at_its_level(gpu, case, g):
    plain, B, total = _plain(gpu, case)
    host = _run(gpu, case, cut_budget=B, curves_per_launch=g)
    # the returned levels: the restatement applied to the budget and the REPORTED sse, bit for bit
    want = ref.levels(B, host["sse"], g)
    assert host["cut_level"].tobytes() == want.tobytes(), (host["cut_level"], want)
    assert np.array_equal(host["cut_level"][0], B) and (host["cut_level"][:, 0] == np.inf).all()
    # every output of every system: trpl_loglik_cut_levels_dev at those levels (-1 among them: the host form would refuse it)
    assert (host["cut_level"] == -1.0).any() or g == 3
    lv = _device_call(gpu, case, "levels", host["cut_level"])
    _same(host, lv)
    # the device form is the host form
    dev = _device_call(gpu, case, "budget", B, g)
    _same(dev, host, keys=OUT + ("cut_level",))
    acc = np.zeros(S)
    for c in range(C):
        acc = acc + (0.0 - host["sse"][c])
    assert np.array_equal(host["P"], acc)
    cut = host["cut_col"] >= 0
    assert host["cut_fraction"] == cut.mean() and host["cut_samples"] == cut.any(axis=0).mean()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_an_infinite_budget_is_the_plain_call_and_one_launch_is_the_levels_call(gpu, case):
    plain, B, total = _plain(gpu, case)
    for g in (1, 2):
        free = _run(gpu, case, cut_budget=np.full(S, np.inf), curves_per_launch=g)
        _same(free, plain, keys=("P", "sse", "status", "iters_total", "floor_col"))
        assert (free["cut_col"] == -1).all() and (free["cut_level"] == np.inf).all() and free["cut_samples"] == 0.0
    per_system = _run(gpu, case, cut_levels=B)                       # the budget as every curve's level
    for g in (C, 16):
        one = _run(gpu, case, cut_budget=B, curves_per_launch=g)
        _same(one, per_system)
        assert np.array_equal(one["cut_level"], np.broadcast_to(B, (C, S)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_cut_sample_is_past_its_budget_and_the_budget_is_spent_across_the_curves(gpu, case):
    """Safety: a sample with any cut_col >= 0 has a plain total >= its budget.  Tightness, curves_per_launch = 1: the last curve's
    level is at most two ulp above fl(B - R2), so an uncut sample has total = fl(R2 + sse_2) <= fl(R2 + l) <= B (1 + 4 * 2^-52) --
    the roundings of the difference, the two successors and the sum; a sample whose plain total is above B (1 + 2^-49) is cut."""
    plain, B, total = _plain(gpu, case)
    per_system = _run(gpu, case, cut_levels=B)
    for g in (1, 2, 3):
        got = _run(gpu, case, cut_budget=B, curves_per_launch=g)
        cut = (got["cut_col"] >= 0).any(axis=0)
        assert (total[cut] >= B[cut]).all(), (g, np.nonzero(cut & ~(total >= B))[0])
        assert not cut[0] and not cut[6] and not cut[11]             # +inf, the total's successor, 1.5 of the total
        assert cut[1] and (got["cut_col"][:, 1] >= 0).all()          # budget 0: every system of the sample after its first batch
        reported = ref.carried(got["sse"])
        assert (reported[cut] >= B[cut]).all() and np.array_equal(reported[~cut], total[~cut])
        if g == 1:
            must = total > B * (1.0 + 2.0 ** -49)
            assert must.sum() >= 7 and cut[must].all(), np.nonzero(must & ~cut)[0]
            later = (got["cut_col"][1:] >= 0) & (per_system["cut_col"][1:] == -1)
            print("%s: cut samples %d (per-system call: %d); systems of curves 1, 2 cut here and not there: %d; iterations %d (per-system %d, "
                  "plain %d)" % (case, cut.sum(), (per_system["cut_col"] >= 0).any(axis=0).sum(), later.sum(), got["iters_total"].sum(),
                                 per_system["iters_total"].sum(), plain["iters_total"].sum()))
            assert later.any() and cut[3] and cut[7]
            assert cut.sum() >= (per_system["cut_col"] >= 0).any(axis=0).sum()


def test_results_do_not_depend_on_pairing_rule_seam_form_or_sharding(gpu):
    A = gpu._abi
    case = (128, "pair", False)
    plain, B, total = _plain(gpu, case)
    for g in (1, 2):
        base = _run(gpu, case, cut_budget=B, curves_per_launch=g)
        for extra in (A.FLAG_PAIR_ADJACENT, A.FLAG_PAIR_ALWAYS_SEAM):
            _same(_run(gpu, case, cut_budget=B, curves_per_launch=g, extra_flags=extra), base, keys=OUT + ("cut_level",))
        X = _problem(gpu, 128, False)[0]
        for lo, hi in ((0, 5), (5, S)):                              # two uneven shards, the first of odd size
            part = _run(gpu, case, X=np.ascontiguousarray(X[lo:hi]), cut_budget=np.ascontiguousarray(B[lo:hi]), curves_per_launch=g)
            for k in OUT + ("cut_level",):
                whole = base[k][lo:hi] if k == "P" else base[k][:, lo:hi]
                assert part[k].tobytes() == np.ascontiguousarray(whole).tobytes(), (g, lo, k)


# ------------------------------------------------------------------ mcmc.run(early_reject="sample")
CHAINS, SWEEPS, LM, SEED = 32, 6, 128, 7
_MC = {}


def _mcmc_problem(gpu, oracle):
    """The problem of tests/test_gpu_mcmc_early_reject.py: half the chains in a tight cluster at the reference's marked point, the
    observations synthesised there by the CPU oracle, the other half on a seeded sample of the default box."""
    if not _MC:
        w, sm = gpu.workloads, gpu.sampler
        ini, lens = w.power_scan(LM)
        lo, hi, lg = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS, sm.DEFAULT_DO_LOG
        mark = (w.MARKED_POINT * gpu.UNIT_CONVERSIONS)[None, :]
        obs = [np.log10(oracle.pvsim(np.ascontiguousarray(mark[:, :-1]), lens[c], T * DT, LM, T, ini[c])["plI"][0]) for c in range(len(lens))]
        U_mark, _ = gpu.refine.unit_coords(np.ascontiguousarray(mark), lo, hi, lg)
        _, cluster, inside = gpu.mcmc.propose(np.repeat(U_mark, CHAINS // 2, axis=0), None, 0.0, 0.002, 0, SEED, 0xFFFF, lo, hi, lg)
        assert inside.all()
        X0 = np.ascontiguousarray(np.concatenate([cluster, w.samples(CHAINS // 2, seed=29)]))
        _MC["p"] = (ini, lens, X0, obs, (lo, hi, lg))
    return _MC["p"]


def _likelihood(gpu, problem, kernel, work):
    ini, lens, _, obs, _ = problem

    def f(X, cut_levels=None, cut_budget=None):
        info = {}
        P = gpu.loglik(X, ini, lens, T * DT, LM, T, obs, kernel=kernel, info=info, cut_levels=cut_levels, cut_budget=cut_budget)
        work["iters"] += int(info["iters_total"].sum())
        work["solved"] += len(X)
        for lv in (cut_levels, cut_budget):
            if lv is not None:
                assert lv.shape == (len(X),)
                work["cut"] += int((info["cut_col"] >= 0).any(axis=0).sum())
        return P
    return f


def _three_runs(gpu, problem, kernel, runner):
    runs = {}
    for early in (False, True, "sample"):
        work, info = dict(iters=0, solved=0, cut=0), {}
        runs[early] = (runner(_likelihood(gpu, problem, kernel, work), info, early), work, info)
    return runs


def _check(runs, label, chains_of):
    (plain, w0, i0), (per_system, w1, i1), (sample, w2, i2) = runs[False], runs[True], runs["sample"]
    print("%s: %d proposals solved; cut %d per system, %d per sample; iterations %d plain, %d per system, %d per sample"
          % (label, w0["solved"], w1["cut"], w2["cut"], w0["iters"], w1["iters"], w2["iters"]))
    for a, b in zip(chains_of(sample), chains_of(plain)):
        for k in ("U", "X", "LL", "accept"):
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert np.array_equal(i2["accept"], i0["accept"]) and np.array_equal(i2["outside"], i0["outside"]) and np.array_equal(i2["folded"], i0["folded"])
    assert np.array_equal(i2["early_reject"], i1["early_reject"]) and "early_reject" not in i0      # the same levels
    assert w2["solved"] == w1["solved"] == w0["solved"] > 0 and w0["cut"] == 0
    assert w2["cut"] >= w1["cut"] >= 1
    assert w2["iters"] <= w1["iters"] < w0["iters"]


@pytest.mark.parametrize("kernel", ["single", "pair"])
@pytest.mark.parametrize("bounds", ["reject", "fold"])
def test_run_with_a_budget_per_proposal_keeps_the_chain_and_cuts_no_less(gpu, oracle, bounds, kernel):
    problem = _mcmc_problem(gpu, oracle)
    ini, lens, X0, obs, (lo, hi, lg) = problem
    LL0 = _likelihood(gpu, problem, kernel, dict(iters=0, solved=0, cut=0))(X0)
    runs = _three_runs(gpu, problem, kernel, lambda f, info, early: gpu.mcmc.run(
        f, X0, LL0, lo, hi, lg, sweeps=SWEEPS, tf=1.0, seed=SEED, bounds=bounds, info=info, early_reject=early))
    _check(runs, "bounds=%s kernel=%s" % (bounds, kernel), lambda ch: [ch])


def test_run_with_a_prior_and_a_budget_per_proposal(gpu, oracle):
    problem = _mcmc_problem(gpu, oracle)
    ini, lens, X0, obs, (lo, hi, lg) = problem
    A = int(gpu.refine.unit_coords(X0[:1], lo, hi, lg)[0].shape[1])
    prior = (np.full(A, 0.5), np.full(A, 0.4))
    LL0 = _likelihood(gpu, problem, "pair", dict(iters=0, solved=0, cut=0))(X0)
    runs = _three_runs(gpu, problem, "pair", lambda f, info, early: gpu.mcmc.run(
        f, X0, LL0, lo, hi, lg, sweeps=SWEEPS, tf=1.0, seed=SEED, info=info, prior=prior, early_reject=early))
    _check(runs, "prior", lambda ch: [ch])


def test_run_tempered_with_a_budget_per_proposal(gpu, oracle):
    problem = _mcmc_problem(gpu, oracle)
    ini, lens, X0, obs, (lo, hi, lg) = problem
    LL0 = _likelihood(gpu, problem, "pair", dict(iters=0, solved=0, cut=0))(X0)
    ladder = [1.0, 8.0]
    runs = _three_runs(gpu, problem, "pair", lambda f, info, early: gpu.mcmc.run_tempered(
        f, X0, LL0, lo, hi, lg, ladder, sweeps=SWEEPS, seed=SEED, info=info, early_reject=early))
    _check(runs, "two rungs", lambda tp: [tp.rung(0), tp.rung(1)])
    assert np.array_equal(runs["sample"][0].swap_rate, runs[False][0].swap_rate, equal_nan=True)


# ------------------------------------------------------------------ driver.bayes with gpu_info["cut_budget"]
def test_bayes_with_the_exact_margin_as_a_budget_gives_the_uncut_posterior(gpu):
    """driver.bayes over the default box against the shipped 6 ns observations (241 points per curve), 8 sample blocks: with
    cut_margin = exact_cut_margin(tf) and cut_budget = True the posterior weights at that tf and the best sample's P are the uncut
    run's, bit for bit, and no fewer samples are cut than by the per-system run at the same margin."""
    sm = gpu.sampler
    ini = gpu.get_initpoints(os.path.join(GOLDEN, "exc_power_scan.csv"), {"select_obs_sets": None})
    flags = {"load_PL_from_file": False, "override_equal_auger": False, "override_equal_mu": False, "override_equal_s": False,
             "log_pl": True, "self_normalize": False, "random_sample": True, "num_points": 256}
    e_data = gpu.get_data([os.path.join(GOLDEN, "obs_balanced_6ns.csv")], {"time_cutoff": None, "select_obs_sets": None, "noise_level": None},
                          flags, scale_f=1e-23)
    Time, T_ = 6.0, 240
    assert all(len(t) == T_ + 1 for t in e_data[0][0])
    simPar = [2000.0, Time, 128, T_, 1, (0,), 7, 10000]
    minX, maxX = sm.DEFAULT_MINX * sm.UNIT_CONVERSIONS, sm.DEFAULT_MAXX * sm.UNIT_CONVERSIONS
    base = dict(num_gpus=1, has_GPU=True, max_sims_per_block=1, sims_per_gpu=32, fused=True, pl_dtype=np.float64)

    def run(**kw):
        return gpu.bayes(gpu.pvSim, None, None, minX, maxX, sm.DEFAULT_DO_LOG, ini, list(simPar), e_data, dict(flags),
                         dict(base, **kw), rng=np.random.RandomState(42))
    _, P0, X0 = run()
    best = int(np.nanargmax(P0[0]))
    for tf in (1.0, 0.1):
        margin = gpu.posterior.exact_cut_margin(tf)
        logs = {}
        for name, kw in (("system", {}), ("sample", dict(cut_budget=True)), ("sample2", dict(cut_budget=True, curves_per_launch=2))):
            logs[name] = []
            _, Pc, Xc = run(cut_margin=margin, cut_log=logs[name], **kw)
            assert np.array_equal(Xc, X0) and len(logs[name]) == 8 and logs[name][0]["sse_cut"] == float("inf")
            W0, Wc = gpu.posterior.weights(P0[0], tf), gpu.posterior.weights(Pc[0], tf)
            assert W0.tobytes() == Wc.tobytes(), name
            assert Pc[0, best] == P0[0, best] and int(np.nanargmax(Pc[0])) == best
            changed = Pc[0] != P0[0]
            assert (W0[changed] == 0.0).all() and (Pc[0][changed] >= P0[0][changed]).all()
        assert [b["sse_cut"] for b in logs["sample"]] == [b["sse_cut"] for b in logs["system"]]      # the same levels, block by block
        n = {k: sum(b["cut_samples"] for b in v) * 32 for k, v in logs.items()}
        it = {k: sum(b["iters_total"] for b in v) for k, v in logs.items()}
        print("tf = %g: margin %.1f; cut samples per system %d, per sample g=1 %d, g=2 %d of 256; iterations %d, %d, %d"
              % (tf, margin, n["system"], n["sample"], n["sample2"], it["system"], it["sample"], it["sample2"]))
        for a, b, c in zip(logs["system"], logs["sample2"], logs["sample"]):
            assert a["cut_samples"] <= b["cut_samples"] <= c["cut_samples"]
    with pytest.raises(ValueError, match="cut_margin"):
        run(cut_budget=True)
