"""The rule of trpl_loglik_cut_budget (include/trpl.h; tests/cut_budget_ref.py restates it) on random (budget, carried sum) pairs:
it is safe (the level added to what was carried reaches the budget), tight (the exact difference or one of its two successors), and
almost never has to give up.  No GPU needed."""
import numpy as np
import pytest

import cut_budget_ref as ref

N = 200_000


@pytest.fixture(scope="module")
def pairs():
    """B log-uniform in [1e-3, 1e6]; R / B uniform, skewed towards 0, skewed towards 1, and within 1e-16 .. 1e-1 of 1."""
    rng = np.random.default_rng(20)
    B = 10.0 ** rng.uniform(-3.0, 6.0, N)
    u = rng.uniform(0.0, 1.0, N)
    kind = rng.integers(0, 4, N)
    ratio = np.where(kind == 0, u, np.where(kind == 1, u ** 4, np.where(kind == 2, 1.0 - u ** 4, 1.0 - 10.0 ** rng.uniform(-16.0, -1.0, N))))
    R = B * ratio
    return B, R, ref.level(B, R)


def test_the_level_is_safe(pairs):
    B, R, l = pairs
    run = np.isfinite(l) & (l >= 0.0)
    assert run.sum() > 0.9 * N
    assert np.all(R[run] + l[run] >= B[run])                         # fl(R + l) >= B: a system above l puts the total at or above B
    assert np.all(R[l == -1.0] >= B[l == -1.0])                      # only a sample already past its budget gets -1
    assert not np.any((l < 0.0) & (l != -1.0)) and not np.any(np.isnan(l))


def test_the_level_is_tight(pairs):
    B, R, l = pairs
    run = np.isfinite(l) & (l >= 0.0)
    l0 = np.maximum(B - R, 0.0)
    l1 = np.nextafter(l0, np.inf)
    l2 = np.nextafter(l1, np.inf)
    assert np.all((l[run] == l0[run]) | (l[run] == l1[run]) | (l[run] == l2[run]))
    first, second = np.mean(l[run] == l1[run]), np.mean(l[run] == l2[run])
    print("first successor %.4f, second %.6f of %d" % (first, second, run.sum()))
    # the earliest candidate that verifies is taken: the one before it does not
    took1 = run & (l == l1)
    assert not np.any(R[took1] + l0[took1] >= B[took1])
    took2 = run & (l == l2)
    assert not np.any(R[took2] + l1[took2] >= B[took2])


def test_the_fallback_is_rare(pairs):
    B, R, l = pairs
    open_ = np.isfinite(B) & (B > R)
    gave_up = open_ & (l == np.inf)
    print("fallbacks to +inf: %d of %d" % (gave_up.sum(), open_.sum()))
    assert gave_up.sum() <= 0.01 * open_.sum()


def test_the_edge_inputs():
    inf, nan = np.inf, np.nan
    assert ref.level(5.0, 5.0) == -1.0                               # R = B: past the budget
    assert ref.level(5.0, 7.0) == -1.0 and ref.level(5.0, inf) == -1.0
    assert ref.level(0.0, 0.0) == -1.0                               # B = 0 with nothing carried: spent (launch 0 does not ask: levels())
    assert ref.level(inf, 0.0) == inf and ref.level(inf, 1e300) == inf and ref.level(inf, inf) == inf
    assert ref.level(5.0, nan) == inf and ref.level(nan, 1.0) == inf and ref.level(nan, nan) == inf
    assert ref.level(-1.0, 0.0) == -1.0                              # a negative budget (the _dev form cannot look): every system cut
    assert ref.level(5.0, 0.0) == 5.0                                # launch 0: the budget itself
    assert ref.level(1.0, np.nextafter(1.0, 0.0)) == 2.0 ** -53      # one ulp below: the exact difference verifies
    tiny = 5e-324
    assert ref.level(tiny, 0.0) == tiny and ref.level(1.0, tiny) == 1.0
    big = np.finfo(np.float64).max
    assert ref.level(big, 0.0) == big and ref.level(big, big / 2) == big / 2
    # vectorised, one rule per element
    got = ref.level(np.array([5.0, 5.0, inf, 5.0]), np.array([0.0, 5.0, 5.0, nan]))
    assert np.array_equal(got, [5.0, -1.0, inf, inf])


def test_carried_and_levels_follow_the_launches():
    rng = np.random.default_rng(4)
    sse = rng.uniform(0.0, 10.0, (5, 7))
    R = ref.carried(sse[:3])
    assert np.array_equal(R, ((0.0 + sse[0]) + sse[1]) + sse[2]) and np.array_equal(ref.carried(sse[:0]), np.zeros(7))
    # minus what the reduction over the curves makes of a P that starts at zero: p += (0.0 - sse[c])
    p = np.zeros(7)
    for c in range(3):
        p = p + (0.0 - sse[c])
    assert np.array_equal(R, -p)
    B = rng.uniform(5.0, 30.0, 7)
    for g in (1, 2, 3, 5, 16):
        lv = ref.levels(B, sse, g)
        assert lv.shape == sse.shape and np.array_equal(lv[0], B)    # launch 0 runs at the budget
        for c in range(5):
            c0 = (c // g) * g
            assert np.array_equal(lv[c], ref.level(B, ref.carried(sse[:c0])))
    # launch 0 is the budget itself, 0 included (the rule at R = +0.0 would call a budget of 0 spent); a NaN budget never cuts
    edge = np.array([0.0, np.inf, np.nan, 3.0, 5.0, 1.0, 2.0])
    lv = ref.levels(edge, sse, 2)
    assert np.array_equal(lv[0], [0.0, np.inf, np.inf, 3.0, 5.0, 1.0, 2.0]) and np.array_equal(lv[0], lv[1])
    assert lv[2, 0] == -1.0 and lv[2, 1] == np.inf and lv[2, 2] == np.inf
    assert np.array_equal(ref.levels(B, sse, 5), np.broadcast_to(B, sse.shape))
