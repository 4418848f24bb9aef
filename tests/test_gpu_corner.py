"""The corner on the device (trpl_corner*, csrc/corner.hip) against tests/corner_ref.py: columns against the longdouble
restatement, LLk and kept exactly, keys exactly, every weighted bin BIT FOR BIT the numpy.add.at sum in ascending sample order,
and posterior.corner end to end against the golden of the reference's own functions.

Bounds.  Secondary columns: 32 * 2^-53 relative -- a chain of at most 16 correctly rounded operations on positive operands, each
adding at most one rounding, with a factor 2 to spare.  log10 columns: the ROCm installation ships no accuracy table of its math library for fp64 log10,
so the bound is the fallback of 4 ulp; the largest distance measured is printed (DESIGN.md section 18 records it: 0.61 ulp).

Weights.  trpl_corner marks a dropped sample with NaN and normalises the full vector; the reference drops first and normalises the
kept samples (utils.py:50-51 before marginalization_visual.py:589-591).  The two are the same numbers but not the same bits:
the weights kernel lifts the exponent by ln S of the FULL length where the dropped-first call uses ln kept, so exp sees another
argument, and the normalising sum groups its terms by another grid.  Bound, in units of ulp = 2^-52 relative, per evaluation:
the unnormalised weight 1.5 (exp within 1 ulp, one fma of the correction), the normalising sum 1.5 for its terms plus 0.5 per
addition on the longest path -- at S <= 2048: one sample per thread, 6 shuffle levels, 3 waves, then 8 block partials through 6
levels and 3 waves, 18 additions -- and 0.5 for the division: 12.5, taken as W_ULP = 16 against an extended-precision
evaluation (tests/highprec.weights) and twice that between two device evaluations.  Against the fp64 host restatement
(oracle.posterior.normalize, whose exponent is rounded three times at magnitude < 1024, 2^-44 each, per sample) the bound is
4 * 2^-44 relative."""
import numpy as np
import pytest

import corner_ref as cr
import highprec as hp

pytestmark = pytest.mark.gpu

SHAPES = (1, 63, 64, 65, 257, 1025)
ULP_SECONDARY = 32 * 2.0 ** -53
ULP_LOG10 = 4
W_ULP = 16


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu.device


def _draw(S, seed=1):
    X, LL = cr.draw(seed, S)
    return X, LL


def _columns(torch_dev, X, codes, dolog=None, thickness=2000.0, elo=None, ehi=None, LL=None):
    torch, dev = torch_dev
    S, D = X.shape[0], len(codes)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    V = torch.full((D, S), -7.0, dtype=torch.float64, device="cuda")
    LLd = None if LL is None else torch.from_numpy(LL).cuda()
    LLk = None if LL is None else torch.empty(S, dtype=torch.float64, device="cuda")
    kept = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    dev.corner_columns_device(Xd, codes, V, do_log=dolog, thickness=thickness, excl_lo=elo, excl_hi=ehi, LL=LLd, LLk=LLk, kept=kept)
    torch.cuda.synchronize()
    return V.cpu().numpy(), None if LLk is None else LLk.cpu().numpy(), int(kept.item())


def _hist(torch_dev, V, W, lo, hi, bins, pairs=True, counts=True):
    torch, dev = torch_dev
    D, S = V.shape
    Vd, Wd = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(W)).cuda()
    h1 = torch.full((D, bins), -1.0, dtype=torch.float64, device="cuda")
    c1 = torch.full((D, bins), -1.0, dtype=torch.float64, device="cuda") if counts else None
    h2 = torch.full((D * (D - 1) // 2, bins, bins), -1.0, dtype=torch.float64, device="cuda") if pairs and D > 1 else None
    ws = dev.corner_workspace(S, D)
    dev.corner_hist_device(Vd, Wd, lo, hi, h1, ws, c1=c1, h2=h2)
    torch.cuda.synchronize()
    return h1.cpu().numpy(), None if c1 is None else c1.cpu().numpy(), None if h2 is None else h2.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


CODES = {1: [16], 7: [1, 13, 14, 15, 16, 17, 18], 19: list(range(19))}


@pytest.mark.parametrize("S", SHAPES)
def test_columns_against_longdouble(torch_dev, S):
    X, _ = _draw(S, seed=S)
    worst_sec, worst_log = 0.0, 0.0
    for D, codes in CODES.items():
        for logged in (False, True):
            dolog = [int(logged and c not in (12,)) for c in codes]          # mag_offset crosses 0: never logged
            V, _, kept = _columns(torch_dev, X, codes, dolog)
            assert kept == S
            for d, c in enumerate(codes):
                want = cr.column(X, c, 2000.0, bool(dolog[d]))
                got = V[d]
                if not dolog[d]:
                    if c < cr.PRIMARY:
                        assert _same_bits(got, np.ascontiguousarray(X[:, c])), (S, D, c)
                        continue
                    err = float(np.max(np.abs(got.astype(cr.LD) - want) / np.abs(want)))
                    worst_sec = max(worst_sec, err)
                    assert err <= ULP_SECONDARY, (S, D, c, err)
                else:
                    # the argument of log10 is the device's own unlogged value: measure log10 alone
                    arg = _columns(torch_dev, X, [c], [0])[0][0]
                    ref = np.log10(arg.astype(cr.LD))
                    ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(cr.LD)
                    err = float(np.max(np.abs(got.astype(cr.LD) - ref) / ulp))
                    worst_log = max(worst_log, err)
                    assert err <= ULP_LOG10, (S, D, c, err)
    print("S=%d: secondary columns %.3g ulp (bound 32), log10 %.3g ulp (bound %d, the fallback: no ROCm table found)"
          % (S, worst_sec / 2.0 ** -53, worst_log, ULP_LOG10))


def test_columns_zero_and_inf_are_exact(torch_dev):
    X, _ = _draw(65, seed=3)
    X[::2, 2] = 0.0                                              # mu_n = 0: 1 / mu_n = inf, mu' = 0, Dif = 0, tau_surf = inf
    X[1::4, 11] = 0.0                                            # lambda = 0: epsilon = inf
    codes = [13, 16, 17]
    V, _, _ = _columns(torch_dev, X, codes, [0, 0, 0])
    want = cr.columns(X, codes).astype(np.float64)
    assert np.all(V[1][::2] == 0.0) and np.all(np.isinf(V[2][1::4]))
    special = ~np.isfinite(want) | (want == 0)
    assert special.any() and np.array_equal(V[special], want[special])
    ok = ~special
    assert np.max(np.abs(V[ok] - want[ok]) / np.abs(want[ok])) <= ULP_SECONDARY
    # log10 of those: -inf and +inf exactly
    Vl, _, _ = _columns(torch_dev, X, [16, 17], [1, 1])
    assert np.all(Vl[0][::2] == -np.inf) and np.all(Vl[1][1::4] == np.inf)


@pytest.mark.parametrize("S", SHAPES)
def test_llk_and_kept_are_exact(torch_dev, S):
    X, LL = _draw(S, seed=10 + S)
    rng = np.random.default_rng(S)
    elo, ehi = np.full(13, np.nan), np.full(13, np.nan)
    elo[1], ehi[1] = 2e14, 6e15
    elo[9], ehi[9] = 100.0, 900.0
    elo[12], ehi[12] = -0.25, 0.25
    X[rng.random(S) < 0.1, 9] = np.nan                           # a NaN in a limited column: excluded
    X[rng.random(S) < 0.1, 5] = np.nan                           # a NaN in a column without limits: kept
    LL[rng.random(S) < 0.1] = np.nan                             # a NaN likelihood: stays NaN, not counted
    on = rng.random(S)
    X[on < 0.1, 9] = 100.0                                       # exactly on a limit: kept
    X[(on > 0.1) & (on < 0.2), 9] = 900.0
    X[(on > 0.2) & (on < 0.25), 9] = np.nextafter(100.0, 0.0)    # one ulp outside: excluded
    X[(on > 0.25) & (on < 0.3), 9] = np.nextafter(900.0, 1e4)
    want, n = cr.llk(X, LL, elo, ehi)
    for codes in CODES.values():
        _, got, kept = _columns(torch_dev, X, codes, None, elo=elo, ehi=ehi, LL=LL)
        assert _same_bits(got, want) and kept == n, (S, kept, n)
    _, got, kept = _columns(torch_dev, X, [0], None, LL=LL)      # no exclusion: LL itself
    assert _same_bits(got, LL) and kept == int(np.count_nonzero(~np.isnan(LL)))


def _axis_points(S, D, bins, seed):
    """V (D, S) on the axes lo = 0.2, hi = 0.9 (the computed last edge differs from hi at several bin counts): every edge, the last
    edge and its neighbours, values outside, NaN and +-inf (highprec.hist_points), each column its own shuffle."""
    rng = np.random.default_rng(seed)
    return np.stack([hp.hist_points(rng, 0.2, 0.9, bins, S) for _ in range(D)])


@pytest.mark.parametrize("bins", (1, 2, 96, 128))
def test_keys_and_bits_at_every_shape(torch_dev, bins):
    for S in SHAPES:
        for D in (1, 2, 19):
            V = _axis_points(S, D, bins, seed=1000 * bins + 10 * S + D)
            lo, hi = np.full(D, 0.2), np.full(D, 0.9)
            rng = np.random.default_rng(S + D)
            W = np.exp(rng.uniform(-40.0, 0.0, S))
            W[rng.random(S) < 0.2] = 0.0
            W[rng.random(S) < 0.05] = np.nan
            want = cr.hist(V, W, lo, hi, bins)
            got = _hist(torch_dev, V, W, lo, hi, bins)
            assert _same_bits(got[0], want[0]), (S, D, bins)
            assert np.array_equal(got[1], want[1]), (S, D, bins)
            assert (got[2] is None) == (D == 1)
            if D > 1:
                assert _same_bits(got[2], want[2]), (S, D, bins)
            # the keys themselves: all-ones weights turn every weighted bin into an exact count
            ones = np.ones(S)
            g1, gc, g2 = _hist(torch_dev, V, ones, lo, hi, bins)
            k = cr.keys(V, lo, hi, bins)
            for d in range(D):
                assert np.array_equal(g1[d], np.bincount(k[d][k[d] >= 0], minlength=bins)), (S, D, bins, d)
            assert np.array_equal(g1, gc)
            if D > 1:
                for p, (j, i) in enumerate(cr.pairs(D)):
                    ok = (k[j] >= 0) & (k[i] >= 0)
                    assert np.array_equal(g2[p].ravel(), np.bincount(k[j][ok] * bins + k[i][ok], minlength=bins * bins)), (S, D, bins, p)


def test_last_edge_is_the_computed_one(torch_dev):
    bins, lo, hi = 100, 0.2, 0.9
    e = cr.bin_edges(lo, hi, bins)
    assert e[-1] != hi                                           # 0.8999999999999999
    pts = np.array([e[-1], np.nextafter(e[-1], 0.0), np.nextafter(e[-1], 1.0), hi, lo, np.nextafter(lo, 0.0), np.nan, np.inf, -np.inf])
    V = np.stack([pts, pts[::-1].copy()])
    W = np.ones(len(pts))
    want = cr.hist(V, W, np.full(2, lo), np.full(2, hi), bins)
    got = _hist(torch_dev, V, W, np.full(2, lo), np.full(2, hi), bins)
    assert want[0][0].sum() == 3 and want[0][0][-1] == 2        # the last edge and the value below it; hi itself is outside
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("S", (64, 257, 1025))
def test_order_decides_the_bits(torch_dev, S):
    """All samples in one bin (64 equal keys in every wave: lane order decides) with one weight of 1.0 among many of 1e-16, first
    and last: any other order of addition changes the bits -- checked on the host first."""
    for D in (1, 2):
        V = np.full((D, S), 0.5)
        lo, hi = np.zeros(D), np.ones(D)
        for where in (0, S - 1):
            W = np.full(S, 1e-16)
            W[where] = 1.0
            want = cr.hist(V, W, lo, hi, 96)
            rev = cr.hist(V, W[::-1].copy(), lo, hi, 96)
            assert not _same_bits(want[0], rev[0])               # the order is visible in the bits
            got = _hist(torch_dev, V, W, lo, hi, 96)
            assert _same_bits(got[0], want[0]), (S, D, where)
            if D > 1:
                assert _same_bits(got[2], want[2]), (S, D, where)


def test_weight_families(torch_dev):
    S, D, bins = 1025, 3, 96
    rng = np.random.default_rng(77)
    V = rng.uniform(-0.05, 1.05, (D, S))
    lo, hi = np.zeros(D), np.ones(D)
    fam = {"300 decades": 10.0 ** rng.uniform(-300, 0, S), "all zero": np.zeros(S), "few bins": np.exp(rng.uniform(-5, 0, S))}
    nasty = np.exp(rng.uniform(-5, 0, S))
    nasty[::5] = np.nan
    nasty[1::7] = np.inf
    nasty[2::11] = -np.inf
    nasty[3::13] = -1.0
    fam["NaN and inf"] = nasty
    for name, W in fam.items():
        Vf = np.clip(V, 0.4, 0.45) if name == "few bins" else V
        want = cr.hist(Vf, W, lo, hi, bins)
        got = _hist(torch_dev, Vf, W, lo, hi, bins)
        assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and _same_bits(got[2], want[2]), name
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2])), name
    assert not _hist(torch_dev, V, fam["all zero"], lo, hi, bins)[0].any()
    # the accuracy of the fixed order against exact sums: n_k 2^-53 relative per bin
    W = fam["300 decades"]
    got = _hist(torch_dev, V, W, lo, hi, bins)
    for d in range(D):
        e = cr.bin_edges(lo[d], hi[d], bins)
        exact, n = hp.hist(V[d], W, e), hp.hist(V[d], None, e)
        ok = exact > 0
        assert np.all(np.abs(got[0][d][ok] - exact[ok]) <= n[ok] * 2.0 ** -53 * exact[ok])


def test_runs_streams_and_null_outputs_give_the_same_bits(torch_dev):
    torch, dev = torch_dev
    S, D, bins = 1025, 4, 96
    rng = np.random.default_rng(9)
    V = rng.normal(0.5, 0.2, (D, S))
    W = np.exp(rng.uniform(-30, 0, S))
    lo, hi = np.zeros(D), np.ones(D)
    a = _hist(torch_dev, V, W, lo, hi, bins)
    b = _hist(torch_dev, V, W, lo, hi, bins)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        c = _hist(torch_dev, V, W, lo, hi, bins)
    n = _hist(torch_dev, V, W, lo, hi, bins, pairs=False, counts=False)
    for x, y, z in zip(a, b, c):
        assert _same_bits(x, y) and _same_bits(x, z)
    assert _same_bits(n[0], a[0]) and n[1] is None and n[2] is None


@pytest.fixture(scope="module")
def golden_case(golden):
    g = golden("corner_ref")
    names = [str(n) for n in g["names"]]
    dolog = [str(n) for n in g["do_log"]]
    X, LL = cr.draw(int(g["seed"]), int(g["S"]))
    limits = {n: (float(g["lo"][d]), float(g["hi"][d])) for d, n in enumerate(names)}
    return g, names, dolog, X, LL, limits


def test_corner_end_to_end_against_the_reference(gpu, golden_case):
    g, names, dolog, X, LL, limits = golden_case
    info = {}
    out = gpu.posterior.corner(X, LL, names, limits, bin_count=int(g["bins"]), tf=float(g["tf"]), thickness=float(g["thickness"]),
                               do_log=dolog, exclude=True, info=info)
    assert out["kept"] == int(g["kept"])
    for d, n in enumerate(names):
        dens, e = out["h_1D"][n]
        np.testing.assert_allclose(dens, g["h1"][d], rtol=1e-10, atol=0, err_msg=n)
        assert np.array_equal(e, cr.bin_edges(limits[n][0], limits[n][1], int(g["bins"])))
    assert list(out["h_2D"]) == [(names[j], names[i]) for j, i in cr.pairs(len(names))]
    for p, key in enumerate(out["h_2D"]):
        np.testing.assert_allclose(out["h_2D"][key][0], g["h2"][p], rtol=1e-10, atol=0, err_msg=str(key))
    # W: posterior.weights of the kept likelihoods, scattered back into the full vector (NaN marks a dropped sample)
    ref = cr.corner(X, LL, names, limits, int(g["bins"]), float(g["tf"]), float(g["thickness"]), dolog, exclude=True)
    W = gpu.posterior.weights(ref["LLk"], float(g["tf"]))
    assert _same_bits(out["W"], W) and np.count_nonzero(~np.isnan(W)) == out["kept"]
    # ... and the case itself: drop first, normalise afterwards, scatter back.  Not the same bits (module docstring): bounds
    keep, tf = ~np.isnan(ref["LLk"]), float(g["tf"])
    assert np.array_equal(np.isnan(out["W"]), ~keep)
    got = out["W"][keep]
    dropped_first = gpu.posterior.weights(np.ascontiguousarray(LL[keep]), tf)
    exact = hp.weights(LL[keep], tf)
    rel = lambda a, b: float(np.max(np.abs(a.astype(cr.LD) - b) / np.abs(b)) / 2.0 ** -52)
    figs = (rel(got, exact), rel(dropped_first, exact), rel(got, dropped_first.astype(cr.LD)), rel(got, ref["W"][keep].astype(cr.LD)))
    print("W of the kept samples, largest distance in ulp: to longdouble %.3g (dropped first: %.3g), to the dropped-first device "
          "call %.3g, to the fp64 restatement %.3g; bit-equal to the dropped-first call: %s"
          % (figs + (_same_bits(got, dropped_first),)))
    assert figs[0] <= W_ULP and figs[1] <= W_ULP and figs[2] <= 2 * W_ULP and figs[3] <= 4 * 2.0 ** -44 / 2.0 ** -52
    assert abs(float(np.sum(got.astype(cr.LD))) - 1.0) <= W_ULP * 2.0 ** -52
    # columns() returns the same V, LLk and kept
    excl = {n: ((10.0 ** limits[n][0], 10.0 ** limits[n][1]) if n in dolog else limits[n]) for n in names if cr.NAMES.index(n) < 13}
    V, LLk, kept = gpu.posterior.columns(X, names, float(g["thickness"]), dolog, excl, LL)
    assert _same_bits(V, out["V"]) and _same_bits(LLk, ref["LLk"]) and kept == out["kept"]
    # the raw sums against the existing histogram kernel on the same columns: its order is not fixed, hence 1e-12 and no bits
    Wz = np.where(np.isnan(out["W"]), 0.0, out["W"])
    for d, n in enumerate(names):
        old = gpu.posterior.hist(out["V"][d], Wz, limits[n][0], limits[n][1], int(g["bins"]))
        np.testing.assert_allclose(info["h1"][d], old, rtol=1e-12, atol=0)
    for p, (j, i) in enumerate(cr.pairs(len(names))):
        old = gpu.posterior.hist(out["V"][j], Wz, *limits[names[j]], int(g["bins"]), y=out["V"][i], ylo=limits[names[i]][0],
                                 yhi=limits[names[i]][1], ybins=int(g["bins"]))
        np.testing.assert_allclose(info["h2"][p], old, rtol=1e-12, atol=0)


def test_corner_of_no_samples_is_zeros(gpu):
    info = {}
    with np.errstate(divide="ignore", invalid="ignore"):         # the densities of an empty run are 0 / 0
        out = gpu.posterior.corner(np.empty((0, 13)), np.empty(0), ["p0", "taun"], {"p0": (0.0, 1.0), "taun": (0.0, 1.0)}, bin_count=8,
                                   info=info)
    assert out["kept"] == 0 and out["W"].size == 0
    assert not info["h1"].any() and not info["c1"].any() and not info["h2"].any()


@pytest.mark.parametrize("S", (1, 257))
def test_corner_host_form_without_its_optional_outputs(gpu, S):
    """c1, h2, V, W and kept all NULL, one sample and one block boundary, ldx = 13 + 3 with X ending after its last row's entries:
    h1 is bit for bit the full call's on the compact X."""
    A_ = gpu._abi
    X, LL = cr.draw(5, S)
    names, bins = ["p0", "taun", "taup"], 8
    limits = {n: (float(np.min(X[:, cr.NAMES.index(n)])) - 1.0, float(np.max(X[:, cr.NAMES.index(n)])) + 1.0) for n in names}
    info = {}
    with np.errstate(divide="ignore", invalid="ignore"):         # one sample: the densities of the empty bins are 0 / 0
        gpu.posterior.corner(X, LL, names, limits, bin_count=bins, info=info)
    _, cols, lg = gpu.posterior._corner_codes(names, ())
    lo = np.array([limits[n][0] for n in names])
    hi = np.array([limits[n][1] for n in names])
    ld = X.shape[1] + 3
    Xr = np.full((S - 1) * ld + A_.CORNER_PRIMARY, np.nan)
    for s in range(S):
        Xr[s * ld:s * ld + A_.CORNER_PRIMARY] = X[s, :A_.CORNER_PRIMARY]
    h1 = np.full((len(names), bins), -7.0)
    sec = A_.C.c_double(-1.0)
    A_.check(A_.lib().trpl_corner(A_.ptr(Xr), S, ld, A_.ptr(LL), 1.0, A_.ptr(cols), A_.ptr(lg), len(names), 2000.0, None, None, A_.ptr(lo),
                                  A_.ptr(hi), bins, None, None, None, A_.ptr(h1), None, None, 0, A_.C.byref(sec)))
    assert _same_bits(h1, info["h1"]) and h1.sum() > 0.0 and sec.value > 0.0
