"""trpl_loglik_cut_levels on the GPU (include/trpl.h): the early stop with a level per system, checked through driver.loglik
against the SCALAR call trpl_loglik_cut on the same inputs (which tests/test_gpu_cut.py holds to the plain call) -- never against
figures of its own:
  * a level array filled with one value gives every output of the scalar call at that value, bit for bit;
  * with a level per system, every system reports what the scalar call at ITS level reports, whatever its wavefront partner's;
  * the outputs do not depend on pairing rule, seam form or sharding;
  * trpl_mcmc_levels equals the restatement of tests/mcmc_levels_ref.py bit for bit, host form and device form.
Levels come from {0, the median of the plain call's sse, +inf}: 0 cuts every system after its first batch, +inf none."""
import numpy as np
import pytest

import mcmc_levels_ref as lr
from gpu_common import DT

pytestmark = pytest.mark.gpu

OUT = ("P", "sse", "cut_col", "status", "iters_total", "floor_col")
S, T = 66, 330                                               # 331 columns: five full batches and a partial one


def _workload(gpu, name, L=128, n=S):
    w = gpu.workloads
    ini, lens = w.power_scan(L) if name == "power_scan" else w.twothick(L)
    return w.samples(n, seed=17), ini, lens


def _observations(C, T_, plT=1, offgrid=False, shift=0.0):
    """On the grid every curve has all ncol points of a straight line in log10 (equal counts: curves of one thickness share
    wavefronts).  Off the grid: sorted random times, 300 + 7 c of them."""
    if not offgrid:
        return None, [18.0 - shift - 0.2 * DT * plT * np.arange(T_ // plT + 1) for _ in range(C)]
    rng = np.random.default_rng(5)
    times = [np.sort(rng.uniform(0.0, T_ * DT, 300 + 7 * c)) for c in range(C)]
    return times, [18.0 - 0.2 * t + 0.05 * rng.standard_normal(len(t)) for t in times]


def _run(gpu, X, ini, lens, T_, obs, times, kw, L=128, **cut):
    info = {}
    info["P"] = gpu.loglik(X, ini, lens, T_ * DT, L, T_, obs, times=times, info=info, **cut, **kw)
    return info


def _median_level(gpu, X, ini, lens, T_, obs, times, kw, L=128):
    ref = _run(gpu, X, ini, lens, T_, obs, times, kw, L=L)
    return float(np.median(ref["sse"][ref["status"] == 0]))


def _same(a, b, keys=OUT, where=None):
    for k in keys:
        x, y = (a[k], b[k]) if where is None or k == "P" else (a[k][where], b[k][where])
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), k


@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
@pytest.mark.parametrize("kernel", ["single", "pair"])
@pytest.mark.parametrize("workload", ["power_scan", "twothick"])
def test_uniform_levels_are_the_scalar_call(gpu, workload, kernel, predict):
    X, ini, lens = _workload(gpu, workload)
    C = len(lens)
    times, obs = _observations(C, T)
    kw = dict(kernel=kernel, predict=predict)
    level = _median_level(gpu, X, ini, lens, T, obs, times, kw)
    for value in (level, 0.0, float("inf")):
        want = _run(gpu, X, ini, lens, T, obs, times, kw, sse_cut=value)
        got = _run(gpu, X, ini, lens, T, obs, times, kw, cut_levels=np.full((C, S), value))
        _same(got, want)
        assert got["cut_fraction"] == want["cut_fraction"]
        if value == level:
            cut = want["cut_col"] >= 0
            assert cut.sum() * 4 >= cut.size and (~cut).sum() * 4 >= cut.size
            _same(_run(gpu, X, ini, lens, T, obs, times, kw, cut_levels=np.full(S, value)), want)      # (S,) is given to each curve


@pytest.mark.parametrize("L", [16, 512])
def test_uniform_levels_are_the_scalar_call_on_the_one_system_kernel_at_other_grids(gpu, L):
    X, ini, lens = _workload(gpu, "power_scan", L=L, n=5)
    times, obs = _observations(len(lens), T)
    kw = dict(kernel="single")
    level = _median_level(gpu, X, ini, lens, T, obs, times, kw, L=L)
    want = _run(gpu, X, ini, lens, T, obs, times, kw, L=L, sse_cut=level)
    got = _run(gpu, X, ini, lens, T, obs, times, kw, L=L, cut_levels=np.full((len(lens), 5), level))
    _same(got, want)
    assert (want["cut_col"] >= 0).any() and (want["cut_col"] == -1).any()


def _pair_table(gpu, lens, n_obs, T_):
    C = len(lens)
    ln, no = np.ascontiguousarray(lens, dtype=np.float64), np.ascontiguousarray(n_obs, dtype=np.int64)
    out = [np.full(C, -1, dtype=np.int32) for _ in range(4)]
    n = gpu._abi.lib().trpl_pair_table(ln.ctypes.data, no.ctypes.data, C, 128, T_, T_ * DT, *[o.ctypes.data for o in out])
    return [tuple(int(o[k]) for o in out) for k in range(max(n, 0))]


def _draw_levels(C, n, level, seed=23):
    return np.random.default_rng(seed).choice([0.0, level, np.inf], size=(C, n))


def _check_each_system_against_the_scalar_call_at_its_level(gpu, X, ini, lens, T_, obs, times, kw, lv, level):
    got = _run(gpu, X, ini, lens, T_, obs, times, kw, cut_levels=lv)
    for value in (0.0, level, np.inf):
        want = _run(gpu, X, ini, lens, T_, obs, times, kw, sse_cut=value)
        m = lv == value
        assert m.any()
        _same(got, want, keys=OUT[1:], where=m)
    acc = np.zeros(len(X))
    for c in range(len(lens)):
        acc = acc + (0.0 - got["sse"][c])
    assert np.array_equal(got["P"], acc)
    cut = got["cut_col"] >= 0
    assert got["cut_fraction"] == cut.mean() and (cut | (got["cut_col"] == -2))[lv == 0.0].all() and not cut[lv == np.inf].any()
    return got, cut


@pytest.mark.parametrize("kernel", ["single", "pair"])
@pytest.mark.parametrize("workload", ["power_scan", "twothick"])
def test_every_system_stops_at_its_own_level(gpu, workload, kernel):
    X, ini, lens = _workload(gpu, workload)
    C = len(lens)
    times, obs = _observations(C, T)
    kw = dict(kernel=kernel)
    level = _median_level(gpu, X, ini, lens, T, obs, times, kw)
    lv = _draw_levels(C, S, level)
    got, cut = _check_each_system_against_the_scalar_call_at_its_level(gpu, X, ini, lens, T, obs, times, kw, lv, level)
    # the two halves of a wavefront: for the same-sample pairs and for the cross-sample pairs of the table, both halves were given
    # different values somewhere, and both orders occur -- A cut beside B uncut, A uncut beside B cut
    table = _pair_table(gpu, lens, [len(o) for o in obs], T)
    assert len(table) == C
    kinds = {"same_sample": [t for t in table if t[0] != t[2]], "cross_sample": [t for t in table if t[0] == t[2]]}
    assert kinds["same_sample"] and kinds["cross_sample"]
    for kind, rows in kinds.items():
        a_only = b_only = differ = 0
        for cA, oA, cB, oB in rows:
            for p in range(S // 2):
                sA, sB = 2 * p + oA, 2 * p + oB
                differ += lv[cA, sA] != lv[cB, sB]
                a_only += cut[cA, sA] and not cut[cB, sB]
                b_only += cut[cB, sB] and not cut[cA, sA]
        assert differ and a_only and b_only, (kind, differ, a_only, b_only)


@pytest.mark.parametrize("variant", ["offgrid", "plT2", "pl_f32_normalize"])
def test_a_level_per_system_off_the_grid_with_a_pl_stride_and_with_f32_staging(gpu, variant):
    X, ini, lens = _workload(gpu, "power_scan")
    C = len(lens)
    if variant == "offgrid":
        T_, kw = T, dict(kernel="pair")
        times, obs = _observations(C, T_, offgrid=True)
    elif variant == "plT2":
        T_, kw = 2 * T, dict(kernel="pair", plT=2)
        times, obs = _observations(C, T_, plT=2)
    else:
        T_, kw = T, dict(kernel="single", pl_f32=True, normalize=True)
        times, obs = _observations(C, T_, shift=18.0)             # self-normalised PL starts at 1
    level = _median_level(gpu, X, ini, lens, T_, obs, times, kw)
    lv = _draw_levels(C, S, level)
    _, cut = _check_each_system_against_the_scalar_call_at_its_level(gpu, X, ini, lens, T_, obs, times, kw, lv, level)
    assert cut[lv == level].any() and not cut[lv == level].all()


@pytest.mark.parametrize("predict", [False, True], ids=["default", "predict"])
def test_outputs_do_not_depend_on_pairing_rule_seam_form_or_sharding(gpu, predict):
    A = gpu._abi
    X, ini, lens = _workload(gpu, "power_scan")
    C = len(lens)
    times, obs = _observations(C, T)
    kw = dict(kernel="pair", predict=predict)
    level = _median_level(gpu, X, ini, lens, T, obs, times, kw)
    lv = _draw_levels(C, S, level)
    base = _run(gpu, X, ini, lens, T, obs, times, kw, cut_levels=lv)
    for extra in (A.FLAG_PAIR_ADJACENT, A.FLAG_PAIR_ALWAYS_SEAM):
        _same(_run(gpu, X, ini, lens, T, obs, times, dict(kw, extra_flags=extra), cut_levels=lv), base)
    for lo, hi in ((0, 25), (25, S)):                             # two uneven shards, the first of odd size
        part = _run(gpu, X[lo:hi], ini, lens, T, obs, times, kw, cut_levels=np.ascontiguousarray(lv[:, lo:hi]))
        for k in OUT:
            whole = base[k][lo:hi] if k == "P" else base[k][:, lo:hi]
            assert part[k].tobytes() == np.ascontiguousarray(whole).tobytes(), (lo, k)


def test_the_device_form_is_the_host_form_and_takes_any_level(gpu):
    """loglik_cut_levels_device against driver.loglik(cut_levels=); where the host form refuses -- a NaN level never cuts (the
    outputs of +inf), a negative one cuts after the first batch (the outputs of 0)."""
    import torch
    dv = gpu.device
    dev = torch.device("cuda", 0)
    X, ini, lens = _workload(gpu, "power_scan", n=16)
    C, n = len(lens), 16
    _, obs = _observations(C, T)
    kw = dict(kernel="pair")
    level = _median_level(gpu, X, ini, lens, T, obs, None, kw)
    lv = _draw_levels(C, n, level, seed=4)
    odd = lv.copy()
    odd[lv == np.inf] = np.nan
    odd[lv == 0.0] = -1.0
    want = _run(gpu, X, ini, lens, T, obs, None, kw, cut_levels=lv)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for levels in (lv, odd):
        out = dict(P=torch.zeros(n, dtype=torch.float64, device=dev), sse=torch.empty((C, n), dtype=torch.float64, device=dev),
                   cut_col=torch.empty((C, n), dtype=torch.int32, device=dev), status=torch.empty((C, n), dtype=torch.int32, device=dev),
                   iters_total=torch.empty((C, n), dtype=torch.int64, device=dev),
                   floor_col=torch.empty((C, n), dtype=torch.int32, device=dev))
        dv.loglik_cut_levels_device(t(X), t(ini), lens, T * DT, 128, T, t(np.stack(obs)), [T + 1] * C, t(levels), out["P"], out["sse"],
                                    cut_col=out["cut_col"], status=out["status"], iters_total=out["iters_total"],
                                    floor_col=out["floor_col"], flags=gpu.FLAG_KERNEL_PAIR)
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in out.items()}, want)
    with pytest.raises(ValueError):
        _run(gpu, X, ini, lens, T, obs, None, kw, cut_levels=odd)


@pytest.mark.parametrize("tf", lr.DEVICE_TFS)
@pytest.mark.parametrize("count,chain0", lr.DEVICE_CASES)
def test_the_levels_kernel_equals_the_restatement(gpu, count, chain0, tf):
    """Bit for bit against the numpy restatement of the rule, host form and device form.  The rule draws log(xi) as the accept
    kernel does -- the device math library's log -- and that is the one operation numpy cannot restate: numpy's log and the device's
    round differently for about 3 % of the uniforms (measured on an MI355X: 5 to 9 of ~256 per case; with numpy's log 7 of these 10
    cases have 1 or 2 levels off, by an ulp -- 0.3998214793047903 against 0.39982147930479023 -- or, where that ulp decides which candidate verifies, by the
    2^-39 relative step between the candidates).  So the restatement is handed log(xi) from the device's library (torch.log on the
    GPU: plumbing, no code of this project), held to numpy's within the two ulp that two logarithms of one ulp each can differ by;
    every other operation of the rule is numpy's.  The count of levels that numpy's own log would give differently is printed."""
    import torch
    import mcmc_ref as mr
    dev = torch.device("cuda", 0)
    step = 2 * count + 1
    LL = lr.device_case(count, chain0, tf)
    xi = mr.accept_uniform(count, chain0, lr.SEED, step)
    lx = torch.log(torch.from_numpy(xi).to(dev)).cpu().numpy()
    lx_np = np.log(xi)
    assert (np.abs(lx - lx_np) <= 2.0 * np.spacing(np.abs(lx_np))).all()
    want = lr.levels_from_log(LL, tf, xi, lx)
    assert np.isfinite(want).any() and (count < 6 or np.isinf(want).any())
    got = gpu.mcmc.reject_levels(LL, tf, chain0, lr.SEED, step)
    plain = lr.levels(LL, tf, chain0, lr.SEED, step)
    print("count %d chain0 %d tf %g: %d of %d logarithms and %d levels differ between numpy's log and the device's"
          % (count, chain0, tf, int((lx != lx_np).sum()), count, int((plain.view(np.int64) != want.view(np.int64)).sum())))
    assert got.tobytes() == want.tobytes(), np.nonzero(got.view(np.int64) != want.view(np.int64))[0][:5]
    LL_d = torch.from_numpy(LL).to(dev)
    lv_d = torch.empty(count, dtype=torch.float64, device=dev)
    gpu.device.mcmc_levels_device(LL_d, tf, chain0, lr.SEED, step, lv_d)
    torch.cuda.synchronize()
    assert lv_d.cpu().numpy().tobytes() == want.tobytes()
    # what the levels are for: the accept step rejects whatever a proposal cut at them can report
    fin = np.isfinite(got)
    U, Xc = np.zeros((count, 1)), np.zeros((count, 1))
    cur = LL.copy()
    acc = gpu.mcmc.accept(U, Xc, cur, U + 0.5, Xc + 0.5, np.where(fin, -np.nextafter(got, np.inf), -np.inf),
                          np.ones(count, dtype=np.int32), tf, chain0, lr.SEED, step)
    assert not acc[fin].any() and np.array_equal(cur[fin], LL[fin])


@pytest.mark.parametrize("tf", lr.DEVICE_TFS)
@pytest.mark.parametrize("count,chain0", lr.DEVICE_CASES)
def test_the_levels_kernel_follows_the_rule_for_a_logarithm_within_two_ulp(gpu, count, chain0, tf):
    """The device's log and numpy's are each within an ulp of the true logarithm, so at most two ulp apart: every level the
    kernel returns is, bit for bit, the restated rule evaluated with one of the five doubles within two ulp of numpy's log(xi)."""
    import mcmc_ref as mr
    step = 2 * count + 1
    LL = lr.device_case(count, chain0, tf)
    got = gpu.mcmc.reject_levels(LL, tf, chain0, lr.SEED, step)
    xi = mr.accept_uniform(count, chain0, lr.SEED, step)
    lx = np.log(xi)
    near = [lx]
    for toward in (-np.inf, np.inf):
        a = np.nextafter(lx, toward)
        near += [a, np.nextafter(a, toward)]
    hit = np.zeros(count, dtype=bool)
    for cand in near:
        hit |= lr.levels_from_log(LL, tf, xi, cand).view(np.int64) == got.view(np.int64)
    assert hit.all(), (np.nonzero(~hit)[0][:5], got[~hit][:5])
