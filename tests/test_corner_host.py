"""The host restatement of the corner (tests/corner_ref.py) against the golden that the reference's own functions produced
(tests/golden/corner_ref.npz, tools/gen_corner_golden.py), the pair order against the reference's loop, and what summing in
ascending order costs against exact sums.  No GPU needed."""
import numpy as np
import pytest

import corner_ref as cr
import highprec as hp


@pytest.fixture(scope="module")
def case(golden):
    g = golden("corner_ref")
    names = [str(n) for n in g["names"]]
    dolog = [str(n) for n in g["do_log"]]
    X, LL = cr.draw(int(g["seed"]), int(g["S"]))
    limits = {n: (float(g["lo"][d]), float(g["hi"][d])) for d, n in enumerate(names)}
    ref = cr.corner(X, LL, names, limits, int(g["bins"]), float(g["tf"]), float(g["thickness"]), dolog, exclude=True)
    return dict(g=g, names=names, dolog=dolog, X=X, LL=LL, limits=limits, ref=ref)


def test_golden_is_what_the_issue_asks_for(case):
    g = case["g"]
    assert case["names"] == ["p0", "mun", "taun", "tau_eff", "mu'", "Sf+Sb"] and case["dolog"] == ["p0", "tau_eff"]
    assert int(g["S"]) == 2048 and int(g["bins"]) == 24
    assert g["h1"].shape == (6, 24) and g["h2"].shape == (15, 24, 24)


def test_conditions_of_the_golden_hold(case):
    """No plotted value within 64 ulp of a bin edge or of an exclusion limit (one rounding cannot move a sample), and 25 % .. 90 %
    of the samples kept: asserted by the generator on the reference's values, and here on the restatement's."""
    g, ref = case["g"], case["ref"]
    S, bins = int(g["S"]), int(g["bins"])
    assert 0.25 * S <= int(g["kept"]) <= 0.90 * S
    margin = np.inf
    for d in range(len(case["names"])):
        margin = min(margin, cr.ulp_margin(ref["V"][d], cr.bin_edges(ref["lo"][d], ref["hi"][d], bins)))
    for c in range(cr.PRIMARY):
        if ref["elo"][c] == ref["elo"][c]:
            margin = min(margin, cr.ulp_margin(case["X"][:, c], [ref["elo"][c], ref["ehi"][c]]))
    print("smallest distance to an edge or a limit: %.3g ulp (generator: %.3g)" % (margin, float(g["margin_ulp"])))
    assert margin >= 64 and float(g["margin_ulp"]) >= 64


def test_restatement_equals_the_reference(case):
    g, ref = case["g"], case["ref"]
    assert ref["kept"] == int(g["kept"])
    for d, n in enumerate(case["names"]):
        np.testing.assert_allclose(ref["h1d"][n], g["h1"][d], rtol=1e-10, atol=0, err_msg=n)
    pp = cr.pairs(len(case["names"]))
    for p, (j, i) in enumerate(pp):
        key = (case["names"][j], case["names"][i])
        np.testing.assert_allclose(ref["h2d"][key], g["h2"][p], rtol=1e-10, atol=0, err_msg=str(key))
    assert np.count_nonzero(g["h2"]) > 200 and np.count_nonzero(g["h1"]) > 100


def test_pair_order_is_the_reference_loop():
    """utils.py:103-106 literally, on names; against the (x, y) index pairs of the restatement and the closed form of the kernel:
    pair p = i (i - 1) / 2 + j."""
    for D in (1, 2, 3, 6, 19):
        enabled = ["c%d" % d for d in range(D)]
        param_pairs = []
        for i, py in enumerate(enabled):
            for j, px in enumerate(enabled):
                if i > j:
                    param_pairs.append((px, py))
        got = cr.pairs(D)
        assert [(enabled[j], enabled[i]) for j, i in got] == param_pairs
        assert len(got) == D * (D - 1) // 2
        for p, (j, i) in enumerate(got):
            assert p == i * (i - 1) // 2 + j and j < i


def test_ascending_sum_against_exact_sums():
    """numpy.add.at in ascending order against math.fsum per bin: the weights are non-negative, so there is no cancellation and a
    bin of n_k samples is within n_k 2^-53 relative of its exact sum."""
    rng = np.random.default_rng(5)
    S, bins = 20000, 24
    V = np.stack([rng.uniform(-0.1, 1.1, S), rng.normal(0.5, 0.3, S)])
    W = np.exp(rng.uniform(-300 * np.log(10), 0, S))            # 300 decades
    W[::7] = 0.0
    lo, hi = np.array([0.0, 0.0]), np.array([1.0, 1.0])
    h1, c1, h2 = cr.hist(V, W, lo, hi, bins)
    worst = 0.0
    for d in range(2):
        e = cr.bin_edges(lo[d], hi[d], bins)
        want = hp.hist(V[d], W, e)
        n = hp.hist(V[d], None, e)
        ok = want > 0
        worst = max(worst, float(np.max(np.abs(h1[d][ok] - want[ok]) / want[ok] / (n[ok] * 2.0 ** -53))))
        assert np.array_equal(c1[d], n)
    e0, e1 = cr.bin_edges(lo[0], hi[0], bins), cr.bin_edges(lo[1], hi[1], bins)
    want = hp.hist(V[0], W, e0, y=V[1], ey=e1)
    n = hp.hist(V[0], None, e0, y=V[1], ey=e1)
    ok = want > 0
    worst = max(worst, float(np.max(np.abs(h2[0][ok] - want[ok]) / want[ok] / (n[ok] * 2.0 ** -53))))
    print("largest error / (n_k 2^-53): %.3g" % worst)
    assert worst <= 1.0


def test_order_is_visible_in_the_bits():
    """The GPU test's order case, checked on the host first: one weight of 1.0 among many of 1e-16 gives different bits when it
    comes first and when it comes last, so a kernel that adds in another order cannot pass both."""
    first = np.array([1.0] + [1e-16] * 200)
    last = first[::-1].copy()
    a, b = np.zeros(1), np.zeros(1)
    np.add.at(a, np.zeros(201, dtype=np.int64), first)
    np.add.at(b, np.zeros(201, dtype=np.int64), last)
    assert a[0] == 1.0 and b[0] > 1.0 and a[0] != b[0]


@pytest.mark.parametrize("bins", (1, 2, 5, 96, 128))
def test_the_kernel_scheme_gives_the_ascending_sum(bins):
    """The scheme of hist_kernel -- tiles in order, one owning wave per x bin, equal keys ranked by lane, one round per rank --
    restated lane by lane on the host (corner_ref.emulate_hist_kernel) equals numpy.add.at bit for bit: edge values, dropped
    values, zero and NaN weights, and every sample in one bin (S = 257)."""
    rng = np.random.default_rng(bins)
    for S in (1, 63, 65, 257):
        V = np.stack([hp.hist_points(rng, 0.2, 0.9, bins, S) for _ in range(2)])
        if S == 257:
            V[:] = 0.5
        W = np.exp(rng.uniform(-40, 0, S))
        W[rng.random(S) < 0.2] = 0.0
        W[rng.random(S) < 0.05] = np.nan
        lo, hi = np.full(2, 0.2), np.full(2, 0.9)
        k = cr.keys(V, lo, hi, bins)
        k = np.where(k < 0, 255, k)
        h1, _, h2 = cr.hist(V, W, lo, hi, bins)
        one = cr.emulate_hist_kernel(k[0], None, W, bins)
        two = cr.emulate_hist_kernel(k[0], k[1], W, bins)
        assert np.array_equal(one.view(np.uint64), h1[0].view(np.uint64)), (bins, S)
        assert np.array_equal(two.view(np.uint64), h2[0].ravel().view(np.uint64)), (bins, S)
