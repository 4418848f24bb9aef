"""The refinement kernels on the device (trpl_refine_*, csrc/refine.hip) against tests/refine_ref.py.

Density: BIT FOR BIT the sequential numpy loop.  Draw: U2 and the linear columns of X2 bit for bit (Philox, genrand_res53, separate
multiply and add are all exact restatements); log columns within 4 ulp -- the exponent l + (lh - l) u is the same double on both
sides (log10 of the bounds is the host's in both), so the distance is that of the device's pow to numpy's, the sampler's stated
distance.  Resampling: idx equals the longdouble reference except at draws whose threshold lies within 1e-12 of the total of a
cumulative value of THE REFERENCE (the device's cumulative weight is three levels of at most 16 + 256 + S / 4096 sequential fp64
additions, 4e-14 relative at S = 2^17; the inputs are seeded so that the reference excuses no draw at all, tests/test_refine_host.py),
at most 1 % of the draws; stats to rtol 1e-12.  End to end: the toy of tests/test_refine_host.py through trpl_amd.refine.run
against the reference's run, rtol 1e-9 (unit_coords' device log10 and the device's moments and weights are the unpinned steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_ref as rr
from test_refine_host import TOY_A, TOY_K, TOY_M, TOY_NU, TOY_ROUNDS, TOY_S1, TOY_SD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ density
def _parents(rng, K, A):
    """K parents: some near both faces of the cube (clipped boxes), the last a duplicate of the first."""
    c = rng.random((K, A))
    if K > 2:
        c[1] = 0.01
        c[2] = 0.995
    if K > 3:
        c[-1] = c[0]
    h = rng.uniform(0.05, 0.45, A) if A <= 2 else rng.uniform(0.3, 0.5, A)
    return rr.boxes(c, h)


def _points(rng, S, A, a, b):
    U = rng.random((S, A))
    K = a.shape[0]
    for s in range(0, S, 7):                                     # rows exactly on a lower / upper face of some parent
        k = int(rng.integers(K))
        U[s] = a[k] if (s // 7) % 2 == 0 else b[k]
    if S > 3:
        U[3] = 2.0                                               # outside the cube: inside no box
    return U


def _density_dev(torch_dev, U, a, b, iv, pad=3):
    torch, dev = torch_dev
    S, A = U.shape
    Up = np.full((S, A + pad), np.nan)
    Up[:, :A] = U
    B = torch.full((S,), -7.0, dtype=torch.float64, device="cuda")
    if pad == 0:
        dev.refine_density_device(_cuda(torch, Up), _cuda(torch, a), _cuda(torch, b), _cuda(torch, iv), B)
    else:
        _abi_density(torch_dev, _cuda(torch, Up), A, _cuda(torch, a), _cuda(torch, b), _cuda(torch, iv), B)
    torch.cuda.synchronize()
    return B.cpu().numpy()


def _abi_density(torch_dev, U, A, a, b, iv, B):
    """ldu > A: the binding directly (the wrapper takes A from the boxes, ldu from the tensor)."""
    torch, dev = torch_dev
    A_ = dev._abi
    A_.check(A_.lib().trpl_refine_density_dev(U.data_ptr(), U.shape[0], U.shape[1], A, a.data_ptr(), b.data_ptr(), iv.data_ptr(), a.shape[0],
                                              B.data_ptr(), torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("A", (1, 2, 10, 16))
def test_density_is_the_sequential_loop_bit_for_bit(gpu, torch_dev, A):
    tile = gpu._abi.lib().trpl_refine_tile_parents()
    rng = np.random.default_rng(A)
    zeros = 0
    for K in (1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3):
        a, b, iv = _parents(rng, K, A)
        for S in (1, 64, 65, 257, 5000):
            U = _points(rng, S, A, a, b)
            want = rr.density(U, a, b, iv)
            got = _density_dev(torch_dev, U, a, b, iv)
            assert _same_bits(got, want), (A, K, S, np.flatnonzero(got != want)[:4])
            zeros += int((got == 0.0).sum())
            if S > 3:
                assert got[3] == 0.0 and not np.signbit(got[3])
            on_face = got[0]                                     # row 0 sits on a lower face: it is inside that box
            assert on_face > 0.0
    assert zeros > 0
    # the host-buffer form, ldu == A, agrees with the _dev form
    a, b, iv = _parents(rng, tile + 1, A)
    U = _points(rng, 257, A, a, b)
    prop = gpu.refine.Proposal(a, b, iv, tile + 1, 1, 0, 0, 2)
    assert _same_bits(gpu.refine.density(U, prop), _density_dev(torch_dev, U, a, b, iv, pad=0))


# ------------------------------------------------------------------ draw
def _box_for(A, flags, rng):
    """A box with exactly A active columns: columns 1 and 4 fixed, the set overrides' targets (2, 6, 8) sampled but not active,
    every other column active, log and linear in turn."""
    lo, hi, lg = [], [], []
    n = 0
    plain = A > 13                                               # no room for fixed columns
    while n < A or len(lo) < (9 if flags & 4 else 7 if flags & 2 else 4 if flags & 1 else 1):
        c = len(lo)
        target = (c == 2 and flags & 1) or (c == 6 and flags & 2) or (c == 8 and flags & 4)
        if not plain and c in (1, 4):
            lo.append(3.5); hi.append(3.5); lg.append(0)
            continue
        if c % 2 == 0:
            lo.append(10.0 ** rng.integers(-30, 3)); hi.append(lo[-1] * 10.0 ** rng.integers(1, 4)); lg.append(1)
        else:
            lo.append(float(rng.integers(-5, 5))); hi.append(lo[-1] + float(rng.integers(1, 50))); lg.append(0)
        if not target:
            if n >= A:                                           # filler beyond the A-th active column: fix it
                hi[-1] = lo[-1]
            else:
                n += 1
    return np.array(lo), np.array(hi), np.array(lg, dtype=np.int32)


def _draw_dev(torch_dev, a, b, m, nu, seed, gen, lo, hi, lg, flags):
    torch, dev = torch_dev
    K, A = a.shape
    total = nu + K * m
    U2 = torch.full((total, A), -7.0, dtype=torch.float64, device="cuda")
    X2 = torch.full((total, lo.size), -7.0, dtype=torch.float64, device="cuda")
    dev.refine_draw_device(_cuda(torch, a), _cuda(torch, b), m, nu, seed, gen, lo, hi, lg, U2, X2, flags=flags)
    torch.cuda.synchronize()
    return U2.cpu().numpy(), X2.cpu().numpy()


@pytest.mark.parametrize("K,A,m,nu,flags", [(5, 3, 4, 7, 0), (1, 1, 3, 0, 0), (3, 7, 0, 5, 3), (4, 4, 2, 0, 1), (300, 10, 3, 100, 7),
                                            (2, 16, 2, 1, 0), (7, 5, 40, 3, 7)])
def test_draw_against_the_reference(gpu, torch_dev, K, A, m, nu, flags):
    rng = np.random.default_rng([K, A, m, nu])
    lo, hi, lg = _box_for(A, flags, rng)
    act = rr.active_columns(lo, hi, flags)
    assert act.size == A
    a, b, _ = rr.boxes(rng.random((K, A)), rng.uniform(0.01, 0.4, A))
    seed, gen = (0x1234567 << 32) | 0x89abcdef, 2
    U2, X2 = _draw_dev(torch_dev, a, b, m, nu, seed, gen, lo, hi, lg, flags)
    want_u = rr.draw_unit(a, b, m, nu, seed, gen)
    assert _same_bits(U2, want_u)
    total = nu + K * m
    assert np.all((U2 >= 0) & (U2 <= 1))
    par = (np.arange(total - nu)) % K
    assert np.all((U2[nu:] >= a[par]) & (U2[nu:] <= b[par]))
    want_x = rr.from_unit(want_u, lo, hi, lg, flags)
    worst = 0.0
    for c in range(lo.size):
        src = {2: 3, 6: 5, 8: 7}.get(c) if ((c == 2 and flags & 1) or (c == 6 and flags & 2) or (c == 8 and flags & 4)) else None
        if src is not None:
            assert _same_bits(X2[:, c], X2[:, src]), c           # the override, applied last
        ref_c = c if src is None else src
        if lo[ref_c] == hi[ref_c]:
            assert np.all(X2[:, c] == lo[ref_c]), c
        elif lg[ref_c]:
            ulp = np.abs(X2[:, c] - want_x[:, c]) / np.spacing(np.abs(want_x[:, c]))
            worst = max(worst, float(ulp.max()) if total else 0.0)
            assert np.all(ulp <= 4), (c, ulp.max())
        else:
            assert _same_bits(X2[:, c], want_x[:, c]), c
    print("draw K=%d A=%d: log columns within %.2f ulp" % (K, A, worst))
    # the same call twice: the same bits; another generation or seed: every row changes
    U2b, X2b = _draw_dev(torch_dev, a, b, m, nu, seed, gen, lo, hi, lg, flags)
    assert _same_bits(U2, U2b) and _same_bits(X2, X2b)
    for s2, g2 in ((seed, gen + 1), (seed + 1, gen), (seed + (1 << 32), gen)):
        U3, _ = _draw_dev(torch_dev, a, b, m, nu, s2, g2, lo, hi, lg, flags)
        assert np.all(np.any(U3 != U2, axis=1))
    # the host-buffer form
    prop = gpu.refine.Proposal(a, b, None, K, m, nu, seed, gen)
    sim = {"override_equal_mu": bool(flags & 1), "override_equal_s": bool(flags & 2), "override_equal_auger": bool(flags & 4)}
    Xh, Uh = gpu.refine.draw(prop, lo, hi, lg, sim)
    assert _same_bits(Uh, U2) and _same_bits(Xh, X2)


def test_unit_coords_invert_the_draw(gpu, torch_dev):
    rng = np.random.default_rng(3)
    lo, hi, lg = _box_for(10, 7, rng)
    U = rng.random((1000, 10))
    X = rr.from_unit(U, lo, hi, lg, 7)
    sim = {"override_equal_mu": True, "override_equal_s": True, "override_equal_auger": True}
    got, act = gpu.refine.unit_coords(X, lo, hi, lg, sim)
    want, act_ref = rr.unit_coords(X, lo, hi, lg, 7)
    assert list(act) == list(act_ref)
    # two log10 evaluations, each within 1 ulp at a magnitude below 64 (2^-47), over a range >= 1; a factor 2 for the roundings of
    # the subtraction and the division
    assert np.max(np.abs(got - want)) <= 4 * 2.0 ** -47
    torch, dev = torch_dev
    Ud = torch.empty((1000, 10), dtype=torch.float64, device="cuda")
    dev.refine_unit_device(_cuda(torch, X), lo, hi, lg, Ud, flags=7)
    torch.cuda.synchronize()
    assert _same_bits(Ud.cpu().numpy(), got)


# ------------------------------------------------------------------ resampling
def _resample_dev(torch_dev, W, K, offset):
    torch, dev = torch_dev
    idx = torch.full((K,), -7, dtype=torch.int64, device="cuda")
    stats = torch.full((3,), -7.0, dtype=torch.float64, device="cuda")
    dev.refine_resample_device(_cuda(torch, W), idx, dev.refine_workspace(W.size), offset=offset, stats=stats)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("name", rr.PATTERNS)
def test_resample_against_longdouble(gpu, torch_dev, name):
    chunk = gpu._abi.lib().trpl_refine_chunk_rows()
    assert chunk == 4096                                         # the shapes tests/test_refine_host.py clears of excused draws
    for S in (1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, (1 << 17) + 3):
        W = rr.weight_pattern(name, S)
        w = rr.used_weights(W)
        for K in (1, 2, 64, 1000, 4096):
            idx, stats = _resample_dev(torch_dev, W, K, rr.OFFSET)
            want, margin, want_stats = rr.resample(W, K, rr.OFFSET)
            if name == "zero":
                assert np.all(idx == -1) and stats[0] == 0.0, (S, K)
                continue
            excused = margin < rr.MARGIN
            assert excused.mean() <= 0.01, (name, S, K, excused.sum())
            assert np.array_equal(idx[~excused], want[~excused]), (name, S, K, np.flatnonzero(idx != want)[:4])
            assert np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < S, (name, S, K)
            assert np.all(w[idx] > 0), (name, S, K)
            cnt = np.bincount(idx[~excused], minlength=S)
            kp = K * w.astype(np.longdouble) / w.astype(np.longdouble).sum()
            touched = np.zeros(S, dtype=bool)
            touched[want[excused]] = True
            ok = (cnt >= np.floor(kp)) & (cnt <= np.ceil(kp))
            assert np.all(ok | touched), (name, S, K)
            assert np.allclose(stats, want_stats, rtol=1e-12, atol=0), (name, S, K, stats, want_stats)
            if K == 1000 and S in (chunk + 1, (1 << 17) + 3):    # the same call twice: the same bits
                idx2, stats2 = _resample_dev(torch_dev, W, K, rr.OFFSET)
                assert np.array_equal(idx, idx2) and _same_bits(stats, stats2)
    if name == "zero":
        with pytest.raises(ValueError, match="positive weight"):
            gpu.refine.resample(np.zeros(5), 3)
    else:                                                        # the host-buffer form
        W = rr.weight_pattern(name, chunk + 1)
        idx, info = gpu.refine.resample(W, 64, rr.OFFSET)
        assert np.array_equal(idx, _resample_dev(torch_dev, W, 64, rr.OFFSET)[0]) and info["ess"] > 0


# ------------------------------------------------------------------ the host-buffer forms at the edges of their staging
def _ragged(a, ld):
    """The rows of `a` at leading dimension ld in a buffer that ENDS with the last row's entries; NaN in the padding."""
    S, w = a.shape
    flat = np.full((S - 1) * ld + w, np.nan)
    for s in range(S):
        flat[s * ld:s * ld + w] = a[s]
    return flat


@pytest.mark.parametrize("S", (1, 257))
def test_host_forms_with_a_ragged_last_row_and_no_stats(gpu, torch_dev, S):
    """One sample and one block boundary (257 = 256 + 1): ld = width + 3 with the buffer ending after the last row's entries, and
    the optional stats absent.  Bit for bit the restatement (density), the compact call (unit) and the call with stats (resample)."""
    A_, lib = gpu._abi, gpu._abi.lib()
    rng = np.random.default_rng(S)
    A = 3
    a, b, iv = _parents(rng, 65, A)
    U = _points(rng, S, A, a, b)
    Ur, B = _ragged(U, A + 3), np.full(S, -7.0)
    sec = A_.C.c_double(-1.0)
    A_.check(lib.trpl_refine_density(A_.ptr(Ur), S, A + 3, A, A_.ptr(a), A_.ptr(b), A_.ptr(iv), 65, A_.ptr(B), 0, A_.C.byref(sec)))
    assert _same_bits(B, rr.density(U, a, b, iv)) and sec.value > 0.0
    assert _same_bits(B, _density_dev(torch_dev, U, a, b, iv))
    lo, hi, lg = _box_for(A, 0, rng)
    X = rr.from_unit(rng.random((S, A)), lo, hi, lg, 0)
    want, _ = gpu.refine.unit_coords(X, lo, hi, lg)
    Xr, got = _ragged(X, lo.size + 3), np.full((S, A), -7.0)
    A_.check(lib.trpl_refine_unit(A_.ptr(Xr), S, lo.size + 3, lo.size, A_.ptr(lo), A_.ptr(hi), A_.ptr(lg), 0, A, A_.ptr(got), 0, None))
    assert _same_bits(got, want)
    W = rr.weight_pattern("decades", S)
    idx = np.full(64, -7, dtype=np.int64)
    A_.check(lib.trpl_refine_resample(A_.ptr(W), S, 64, rr.OFFSET, A_.ptr(idx), None, 0, None))
    assert np.array_equal(idx, gpu.refine.resample(W, 64, rr.OFFSET)[0]) and np.array_equal(idx, _resample_dev(torch_dev, W, 64, rr.OFFSET)[0])


def test_host_forms_with_nothing_to_do_return_at_once(gpu):
    """S == 0 (density, unit) and n_uniform + K m == 0 (draw): TRPL_OK, seconds 0, the outputs as they were."""
    A_, lib = gpu._abi, gpu._abi.lib()
    rng = np.random.default_rng(0)
    A = 3
    a, b, iv = _parents(rng, 5, A)
    lo, hi, lg = _box_for(A, 0, rng)
    out = np.full(8, -7.0)
    for call in (lambda sec: lib.trpl_refine_density(None, 0, A, A, A_.ptr(a), A_.ptr(b), A_.ptr(iv), 5, A_.ptr(out), 0, sec),
                 lambda sec: lib.trpl_refine_unit(None, 0, lo.size, lo.size, A_.ptr(lo), A_.ptr(hi), A_.ptr(lg), 0, A, A_.ptr(out), 0, sec),
                 lambda sec: lib.trpl_refine_draw(A_.ptr(a), A_.ptr(b), 5, A, 0, 0, 1, 2, lo.size, A_.ptr(lo), A_.ptr(hi), A_.ptr(lg), 0,
                                                  A_.ptr(out), A_.ptr(out), 0, sec)):
        sec = A_.C.c_double(-1.0)
        A_.check(call(A_.C.byref(sec)))
        assert sec.value == 0.0 and np.all(out == -7.0)


# ------------------------------------------------------------------ end to end
TOY_LO, TOY_HI, TOY_LG = np.array([2.0, 1e-3, -1.0]), np.array([5.0, 1e1, 1.0]), np.array([0, 1, 0])


def test_the_toy_end_to_end_on_the_device(gpu):
    loglik_unit, Z = rr.gaussian_toy(TOY_SD, TOY_A)
    U1 = np.random.default_rng(0).random((TOY_S1, TOY_A))
    ref = rr.run(loglik_unit, U1, TOY_ROUNDS, TOY_K, TOY_M, TOY_NU, seed=0)

    def loglik(X):
        return loglik_unit(rr.unit_coords(X, TOY_LO, TOY_HI, TOY_LG)[0])

    X1 = rr.from_unit(U1, TOY_LO, TOY_HI, TOY_LG)
    info = {}
    pop = gpu.refine.run(loglik, X1, loglik(X1), TOY_LO, TOY_HI, TOY_LG, rounds=TOY_ROUNDS, K=TOY_K, m=TOY_M, n_uniform=TOY_NU, tf=1.0,
                         seed=0, info=info)
    X_all, LLc = pop.corrected(1.0)
    assert LLc.shape == ref["LLc"].shape
    err = np.abs(LLc - ref["LLc"]) / np.abs(ref["LLc"])
    print("LLc: largest relative distance %.3g; ess %s vs %s" % (err.max(), info["ess"], ref["ess"]))
    assert np.all(err <= 1e-9), err.max()
    assert np.allclose(info["ess"], ref["ess"], rtol=1e-9, atol=0)
    ev, ev_ref = float(np.mean(np.exp(LLc))), rr.evidence(ref)
    assert abs(ev - ev_ref) <= 1e-9 * ev_ref and abs(pop.ess(1.0) - ref["ess"][-1]) <= 1e-9 * ref["ess"][-1]
    assert len(info["nonzero"]) == TOY_ROUNDS and all(0 < f <= 1 for f in info["nonzero"])
    # the existing stack takes the concatenated set unchanged
    P = gpu.posterior
    W = P.weights(LLc, 1.0)
    assert abs(W.sum() - 1.0) < 1e-12
    q = P.quantiles(np.ascontiguousarray(X_all.T), W, [0.025, 0.5, 0.975])
    assert q.shape == (3, 3) and np.all(np.isfinite(q)) and np.all(np.diff(q, axis=0) >= 0)
    assert abs(q[1, 0] - 3.5) < 0.05                             # the median of the first column: the cube's centre
    X13 = np.ones((X_all.shape[0], 13))
    X13[:, :3] = X_all
    cr = P.corner(X13, LLc, ["n0", "p0"], {"n0": (2.0, 5.0), "p0": (-3.0, 1.0)}, bin_count=16, do_log=("p0",))
    assert cr["kept"] == X_all.shape[0] and abs(cr["W"].sum() - 1.0) < 1e-12
    assert all(np.all(np.isfinite(d)) for d, _ in cr["h_1D"].values())


def test_one_trpl_pass_through_the_tool(gpu):
    """sampler -> fused likelihood -> refine -> fused likelihood -> combined posterior (tools/e2e_inference.py --refine) on a small
    batch: it finishes, the union's weights sum to 1 (a plain sum over the samples with a finite LL: a NaN among them fails it) and
    no NaN in LLc comes from a finite LL.  The effective sample size is printed and recorded, not gated.  No test before this one ran
    the tool, so there was no shape to take over: 256 samples, 200 steps, c = 1e-3 is this test's own choice, the smallest batch
    that still gives the refinement 8 parents (S // 32) and a uniform share of 32, at a few seconds."""
    r = subprocess.run([sys.executable, os.path.join("tools", "e2e_inference.py"), "256", "200", "1e-3", "--refine"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])["refine"]
    print("refine on TRPL, S = 256, T = 200:", out)
    assert abs(out["weight_sum"] - 1.0) < 1e-9 and out["nan_llc_from_finite_ll"] == 0 and out["nan_weights_from_finite_ll"] == 0
    assert len(out["ess_per_generation"]) == 2 and out["samples"] == 256 + out["n_uniform"] + out["parents"] * out["children_per_parent"]
