"""The oriented refinement kernels on the device (trpl_refine_affine*, trpl_refine_draw_oriented*, csrc/refine_oriented.hip) against
tests/refine_oriented_ref.py.

affine: BIT FOR BIT the ascending-j loop.  Draw: Z2, U2, inside and the linear columns of X2 bit for bit (Philox, genrand_res53 and
every multiply and add are exact restatements); log columns within the 4 ulp of tests/test_gpu_refine.py (the device's pow).  Density:
trpl_refine_density, unchanged, on the device's Z: bit for bit the sequential loop on the reference's Z.  End to end: the correlated
toy of tests/test_refine_oriented_host.py through trpl_amd.refine.run(oriented=True) against the reference's run at the rtol 1e-9 of
tests/test_gpu_refine.py's toy (the device's moments, weights and unit_coords' log10 are the unpinned steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_oriented_ref as ro
import refine_ref as rr
from test_gpu_refine import TOY_HI, TOY_LG, TOY_LO, _box_for
from test_refine_oriented_host import TOY_K, TOY_M, TOY_NU, TOY_RHO, TOY_ROUNDS, TOY_S1, TOY_SD

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


def _lower(rng, A, scale=1.0):
    """A dense lower-triangular matrix, entries of mixed sign over six decades, a positive diagonal."""
    T = np.tril(rng.standard_normal((A, A)) * 10.0 ** rng.uniform(-3, 3, (A, A))) * scale
    T[np.arange(A), np.arange(A)] = np.abs(T[np.arange(A), np.arange(A)]) + 1e-3 * scale
    return T


# ------------------------------------------------------------------ affine
@pytest.mark.parametrize("A", (1, 2, 10, 16))
def test_affine_is_the_ascending_loop_bit_for_bit(gpu, torch_dev, A):
    torch, dev = torch_dev
    rng = np.random.default_rng(A)
    M = _lower(rng, A)
    c = rng.random(A)
    poisoned = M.copy()
    poisoned[np.triu_indices(A, 1)] = np.nan                     # only j <= i is read
    for S in (1, 64, 65, 257, 5000):
        U = rng.random((S, A))
        want = ro.affine(U, M, c)
        Up = np.full((S, A + 3), np.nan)
        Up[:, :A] = U
        for mat in (M, poisoned):
            Z = torch.full((S, A + 2), -7.0, dtype=torch.float64, device="cuda")
            dev.refine_affine_device(_cuda(torch, Up), mat, c, Z)
            torch.cuda.synchronize()
            got = Z.cpu().numpy()
            assert _same_bits(got[:, :A], want), (A, S, np.argwhere(got[:, :A] != want)[:4])
            assert np.all(got[:, A:] == -7.0)                    # the padding of a row is not written
        assert _same_bits(gpu.refine.affine(U, poisoned, c), want), (A, S)            # the host-buffer form, ldu == ldz == A
    # ldu > A and ldz > A through the host-buffer form: the padding of Z on the host stays
    Zh = np.full((257, A + 2), -7.0)
    Uc = np.ascontiguousarray(Up[:257])                          # kept alive over the call
    A_ = gpu._abi
    A_.check(A_.lib().trpl_refine_affine(A_.ptr(Uc), 257, A + 3, A, A_.ptr(M), A_.ptr(c), A_.ptr(Zh), A + 2, 0, None))
    assert _same_bits(Zh[:, :A], ro.affine(Up[:257, :A], M, c)) and np.all(Zh[:, A:] == -7.0)


@pytest.mark.parametrize("S", (1, 257))
def test_affine_host_form_with_padded_rows_on_both_sides(gpu, S):
    """ldu = ldz = A + 3 through the host-buffer form, one sample and one block boundary: the rows bit for bit, the padding of Z stays."""
    A = 3
    rng = np.random.default_rng(S)
    M, c = _lower(rng, A), rng.random(A)
    Up = np.full((S, A + 3), np.nan)
    Up[:, :A] = rng.random((S, A))
    Zh = np.full((S, A + 3), -7.0)
    A_ = gpu._abi
    sec = A_.C.c_double(-1.0)
    A_.check(A_.lib().trpl_refine_affine(A_.ptr(Up), S, A + 3, A, A_.ptr(M), A_.ptr(c), A_.ptr(Zh), A + 3, 0, A_.C.byref(sec)))
    assert _same_bits(Zh[:, :A], ro.affine(Up[:, :A], M, c)) and np.all(Zh[:, A:] == -7.0) and sec.value > 0.0


def test_oriented_draw_of_no_children_returns_at_once(gpu):
    """n_uniform + K m == 0: TRPL_OK, seconds 0, the outputs as they were."""
    A = 3
    rng = np.random.default_rng(0)
    lo, hi, lg = _box_for(A, 0, rng)
    L, M, c, h = _tilted(rng, A)
    zc = ro.affine(rng.uniform(0.2, 0.8, (5, A)), M, c)
    out, ins = np.full(8, -7.0), np.full(8, -7, dtype=np.int32)
    A_ = gpu._abi
    sec = A_.C.c_double(-1.0)
    A_.check(A_.lib().trpl_refine_draw_oriented(A_.ptr(zc), A_.ptr(h), A_.ptr(L), A_.ptr(c), 5, A, 0, 0, 1, 2, lo.size, A_.ptr(lo), A_.ptr(hi),
                                                A_.ptr(lg), 0, A_.ptr(out), A_.ptr(out), A_.ptr(out), A_.ptr(ins), 0, A_.C.byref(sec)))
    assert sec.value == 0.0 and np.all(out == -7.0) and np.all(ins == -7)


# ------------------------------------------------------------------ draw
def _tilted(rng, A):
    """An orientation tilted against the axes: L with off-diagonal entries of the size of its diagonal, c the cube's centre,
    half-widths of 0.6 in z, i.e. about 0.1 in u."""
    L = np.tril(rng.uniform(-0.12, 0.12, (A, A)))
    L[np.arange(A), np.arange(A)] = rng.uniform(0.1, 0.2, A)
    M = np.tril(np.linalg.inv(L))
    return L, M, np.full(A, 0.5), np.full(A, 0.6)


def _draw_dev(torch_dev, zc, h, L, c, m, nu, seed, gen, lo, hi, lg, flags):
    torch, dev = torch_dev
    K, A = zc.shape
    total = nu + K * m
    Z2 = torch.full((total, A), -7.0, dtype=torch.float64, device="cuda")
    U2 = torch.full((total, A), -7.0, dtype=torch.float64, device="cuda")
    X2 = torch.full((total, lo.size), -7.0, dtype=torch.float64, device="cuda")
    ins = torch.full((total,), -7, dtype=torch.int32, device="cuda")
    dev.refine_draw_oriented_device(_cuda(torch, zc), h, L, c, m, nu, seed, gen, lo, hi, lg, Z2, U2, X2, ins, flags=flags)
    torch.cuda.synchronize()
    return Z2.cpu().numpy(), U2.cpu().numpy(), X2.cpu().numpy(), ins.cpu().numpy()


def _same_bits_or_nan(a, b):
    return a.shape == b.shape and np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))


@pytest.mark.parametrize("A,flags", [(3, 0), (10, 7), (16, 0)])
def test_oriented_draw_against_the_reference(gpu, torch_dev, A, flags):
    rng = np.random.default_rng([A, flags])
    lo, hi, lg = _box_for(A, flags, rng)
    assert rr.active_columns(lo, hi, flags).size == A
    L, M, c, h = _tilted(rng, A)
    seed, gen = (0x1234567 << 32) | 0x89abcdef, 3
    worst, both_in_a_wave = 0.0, 0
    for K in (1, 63, 64, 65, 259):
        Up = rng.uniform(0.2, 0.8, (K, A))
        Up[0] = 1.0                                              # a parent at a corner of the cube: most of its children leave
        zc = ro.affine(Up, M, c)
        for m in (1, 32):
            for nu in (0, 37):
                Z2, U2, X2, ins = _draw_dev(torch_dev, zc, h, L, c, m, nu, seed, gen, lo, hi, lg, flags)
                wz, wu, wi = ro.draw(zc, h, L, c, m, nu, seed, gen)
                key = (A, K, m, nu)
                assert _same_bits_or_nan(Z2, wz) and np.all(np.isnan(Z2[:nu])) and not np.isnan(Z2[nu:]).any(), key
                assert _same_bits(U2, wu), key
                assert ins.dtype == np.int32 and np.array_equal(ins, wi), key
                assert np.all(ins[:nu] == 1) and np.all((U2[:nu] >= 0) & (U2[:nu] < 1)), key
                assert np.array_equal(ins == 1, np.all((U2 >= 0) & (U2 <= 1), axis=1)), key
                both_in_a_wave += int(any(0 < ins[w:w + 64].sum() < ins[w:w + 64].size for w in range(0, ins.size, 64)))
                assert np.all(np.isfinite(X2)), key              # an outside child keeps a finite X beyond the prior box
                want_x = rr.from_unit(wu, lo, hi, lg, flags)
                for col in range(lo.size):
                    src = {2: 3, 6: 5, 8: 7}.get(col) if ((col == 2 and flags & 1) or (col == 6 and flags & 2) or (col == 8 and flags & 4)) else None
                    if src is not None:
                        assert _same_bits(X2[:, col], X2[:, src]), (key, col)
                    ref_c = col if src is None else src
                    if lo[ref_c] == hi[ref_c]:
                        assert np.all(X2[:, col] == lo[ref_c]), (key, col)
                    elif lg[ref_c]:
                        ulp = np.abs(X2[:, col] - want_x[:, col]) / np.spacing(np.abs(want_x[:, col]))
                        worst = max(worst, float(ulp.max()))
                        assert np.all(ulp <= 4), (key, col, ulp.max())
                    else:
                        assert _same_bits(X2[:, col], want_x[:, col]), (key, col)
    print("oriented draw A=%d: log columns within %.2f ulp; %d calls with both values of inside in one wave" % (A, worst, both_in_a_wave))
    assert both_in_a_wave >= 10
    # the host-buffer form, and its uniforms are trpl_refine_draw's
    prop = gpu.refine.Proposal(zc - h, zc + h, None, K, m, nu, seed, gen, dict(zc=zc, h=h, L=L, c=c))
    sim = {"override_equal_mu": bool(flags & 1), "override_equal_s": bool(flags & 2), "override_equal_auger": bool(flags & 4)}
    Xh, Uh, ih = gpu.refine.draw(prop, lo, hi, lg, sim)
    assert _same_bits(Uh, U2) and _same_bits(Xh, X2) and np.array_equal(ih, ins)
    plain = gpu.refine.Proposal(np.zeros((K, A)), np.ones((K, A)), None, K, m, nu, seed, gen)
    _, Uplain = gpu.refine.draw(plain, lo, hi, lg, sim)
    assert _same_bits(Uplain[:nu], U2[:nu])


# ------------------------------------------------------------------ density on the device's Z
@pytest.mark.parametrize("A", (2, 10))
def test_density_of_oriented_boxes_bit_for_bit(gpu, torch_dev, A):
    torch, dev = torch_dev
    rng = np.random.default_rng(100 + A)
    L, M, c, h = _tilted(rng, A)
    K, S = 131, 1000
    U = rng.random((S, A))
    Zref = ro.affine(U, M, c)
    zc = ro.affine(rng.uniform(0.2, 0.8, (K, A)), M, c)
    a, b, iv = ro.boxes(zc, 4.0 * h if A > 2 else h, float(np.sum(np.log(np.diag(L)))))
    a[5], b[7] = Zref[11], Zref[12]                              # rows 11 and 12 lie exactly on a lower / an upper face: the bits of
    b[5], a[7] = Zref[11] + 1.0, Zref[12] - 1.0                  # the reference's Z are the box's bounds
    want = rr.density(Zref, a, b, iv)
    assert want[11] >= iv[5] and want[12] >= iv[7] and (want == 0).any() and (want > 0).any()
    Z = torch.empty((S, A), dtype=torch.float64, device="cuda")
    dev.refine_affine_device(_cuda(torch, U), M, c, Z)
    B = torch.full((S,), -7.0, dtype=torch.float64, device="cuda")
    dev.refine_density_device(Z, _cuda(torch, a), _cuda(torch, b), _cuda(torch, iv), B)
    torch.cuda.synchronize()
    assert _same_bits(B.cpu().numpy(), want), np.flatnonzero(B.cpu().numpy() != want)[:4]
    # the Python layer: density() and log_ratio() transform with the proposal's own (M, c)
    prop = gpu.refine.Proposal(a, b, iv, K, 4, 9, 0, 2, dict(M=M, c=c))
    assert _same_bits(gpu.refine.density(U, prop), want)
    axis = gpu.refine.Proposal(*rr.boxes(rng.random((7, A)), 0.3), 7, 5, 3, 0, 3)
    pr = [dict(a=a, b=b, inv_vol=iv, m=4, n_uniform=9, M=M, c=c), dict(a=axis.a, b=axis.b, inv_vol=axis.inv_vol, m=5, n_uniform=3)]
    assert _same_bits(gpu.refine.log_ratio(U, 500, [prop, axis]), ro.log_ratio(U, 500, pr))


# ------------------------------------------------------------------ a -inf likelihood beside a finite ln r
def test_minus_inf_likelihood_has_weight_exactly_zero(gpu):
    P = gpu.posterior
    rng = np.random.default_rng(5)
    S = 700
    LL = -rng.random(S) * 30.0
    lnr = rng.standard_normal(S)
    out = rng.random(S) < 0.3
    LL[out] = -np.inf
    V = rng.random((2, S))
    for tf in (1.0, 7.5):
        W = P.weights(LL, tf, log_ratio=lnr)
        assert np.all(W[out] == 0.0) and not np.isnan(W).any() and abs(W.sum() - 1.0) < 1e-12
        Wc = P.weights(LL - tf * lnr, tf)
        assert np.all(Wc[out] == 0.0) and not np.isnan(Wc).any() and np.allclose(Wc, W, rtol=1e-10, atol=0)
        sc = P.tf_scan(LL, [tf, 2 * tf], V, log_ratio=lnr)
        assert all(np.all(np.isfinite(np.asarray(sc[k]))) for k in ("stats", "ess", "mean", "var"))
        keep = ~out
        s_all, c_all = P.moments(V, W)
        s_in, c_in = P.moments(V[:, keep], W[keep])
        assert np.all(np.isfinite(s_all)) and np.all(np.isfinite(c_all))
        assert np.allclose(s_all, s_in, rtol=1e-12, atol=0) and np.allclose(c_all, c_in, rtol=1e-9, atol=1e-18)
        q = P.quantiles(V, W, [0.025, 0.5, 0.975])
        assert np.all(np.isfinite(q)) and np.allclose(q, P.quantiles(V[:, keep], W[keep], [0.025, 0.5, 0.975]), rtol=0, atol=1e-12)
    X13 = np.ones((S, 13))
    X13[:, 0], X13[:, 1] = 2.0 + 3.0 * V[0], 10.0 ** (-3.0 + 4.0 * V[1])
    LLc = LL - lnr
    cr = P.corner(X13, LLc, ["n0", "p0"], {"n0": (2.0, 5.0), "p0": (-3.0, 1.0)}, bin_count=16, do_log=("p0",))
    assert cr["kept"] == S and not np.isnan(cr["W"]).any() and abs(cr["W"].sum() - 1.0) < 1e-12 and np.all(cr["W"][out] == 0.0)
    assert all(np.all(np.isfinite(d)) for d, _ in cr["h_1D"].values())


# ------------------------------------------------------------------ end to end
def test_the_correlated_toy_end_to_end_on_the_device(gpu):
    loglik_unit, Z = ro.correlated_toy(TOY_SD, TOY_RHO)
    U1 = np.random.default_rng(0).random((TOY_S1, 3))
    ref = ro.run(loglik_unit, U1, TOY_ROUNDS, TOY_K, TOY_M, TOY_NU, seed=0)
    calls = []

    def loglik(X):
        U = rr.unit_coords(X, TOY_LO, TOY_HI, TOY_LG)[0]
        calls.append(U)
        return loglik_unit(U)

    X1 = rr.from_unit(U1, TOY_LO, TOY_HI, TOY_LG)
    info = {}
    pop = gpu.refine.run(loglik, X1, loglik(X1), TOY_LO, TOY_HI, TOY_LG, rounds=TOY_ROUNDS, K=TOY_K, m=TOY_M, n_uniform=TOY_NU, tf=1.0,
                         seed=0, info=info, oriented=True)
    X_all, LLc = pop.corrected(1.0)
    inside = ref["inside"] == 1
    assert LLc.shape == ref["LLc"].shape and np.array_equal(np.isneginf(np.concatenate(pop.LL)), ~inside)
    err = np.abs(LLc[inside] - ref["LLc"][inside]) / np.abs(ref["LLc"][inside])
    print("LLc: largest relative distance %.3g; ess %s vs %s; outside %s vs %s; lam %s" % (err.max(), info["ess"], ref["ess"], info["outside"],
                                                                                          ref["outside"], info["lam"]))
    assert np.all(err <= 1e-9), err.max()
    assert np.all(np.isneginf(LLc[~inside]))
    W = gpu.posterior.weights(LLc, 1.0)
    assert np.all(W[~inside] == 0.0) and not np.isnan(W).any() and abs(W.sum() - 1.0) < 1e-12
    assert np.allclose(info["ess"], ref["ess"], rtol=1e-9, atol=0)
    assert info["outside"] == ref["outside"] and np.allclose(info["lam"], ref["lam"], rtol=1e-9, atol=0)
    # the likelihood saw the inside children only: every point it was given lies in the cube
    assert sum(u.shape[0] for u in calls[1:]) == int(inside[TOY_S1:].sum())
    assert all(np.all((u >= -1e-12) & (u <= 1 + 1e-12)) for u in calls[1:])
    ev, ev_ref = float(np.mean(np.exp(LLc))), ro.evidence(ref)
    assert abs(ev - ev_ref) <= 1e-9 * ev_ref


def test_run_without_orientation_keeps_its_bits(gpu):
    loglik_unit, _ = rr.gaussian_toy(0.12, 3)

    def loglik(X):
        return loglik_unit(rr.unit_coords(X, TOY_LO, TOY_HI, TOY_LG)[0])

    X1 = rr.from_unit(np.random.default_rng(1).random((1024, 3)), TOY_LO, TOY_HI, TOY_LG)
    LL1 = loglik(X1)
    kw = dict(rounds=2, K=32, m=8, n_uniform=64, tf=1.0, seed=3)
    ia, ib = {}, {}
    pa = gpu.refine.run(loglik, X1, LL1, TOY_LO, TOY_HI, TOY_LG, info=ia, **kw)
    pb = gpu.refine.run(loglik, X1, LL1, TOY_LO, TOY_HI, TOY_LG, info=ib, oriented=False, **kw)
    for x, y in zip(pa.corrected(1.0) + pa.log_ratio(), pb.corrected(1.0) + pb.log_ratio()):
        assert _same_bits(x, y)
    assert _same_bits(np.concatenate(pa.U), np.concatenate(pb.U)) and ia == ib and "outside" not in ib
    assert all(p.orient is None for p in pb.proposals)


def test_one_oriented_trpl_pass_through_the_tool(gpu):
    """tools/e2e_inference.py --refine --oriented at the shape of tests/test_gpu_refine.py's pass: it finishes, the union's weights
    sum to 1, no NaN weight comes from a finite LL, and the share of children outside the prior box is reported."""
    r = subprocess.run([sys.executable, os.path.join("tools", "e2e_inference.py"), "256", "200", "1e-3", "--refine", "--oriented"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])["refine"]
    print("oriented refine on TRPL, S = 256, T = 200:", out)
    assert abs(out["weight_sum"] - 1.0) < 1e-9 and out["nan_llc_from_finite_ll"] == 0 and out["nan_weights_from_finite_ll"] == 0
    assert out["oriented"] is True and len(out["outside_share_of_children"]) == 1 and 0.0 <= out["outside_share_of_children"][0] < 1.0
    assert len(out["shrinkage_per_generation"]) == 1 and 0.0 <= out["shrinkage_per_generation"][0] <= 1.0
    assert len(out["ess_per_generation"]) == 2 and out["samples"] == 256 + out["n_uniform"] + out["parents"] * out["children_per_parent"]
