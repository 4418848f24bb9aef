"""posterior._bracket_search, the deterministic search behind find_best_tf, on analytic objectives (no device: the
objective is a callable).  Tolerance: the search ends with a bracket of relative width <= rtol that holds both the returned
point and, for a unimodal objective, the maximiser -- so the two differ by at most rtol, relative."""
import math

import numpy as np
import pytest

K, RTOL = 64, 1e-6


def predicted_rounds(lo, hi, k, rtol):
    """A round lays k points over ln(hi / lo) and keeps the two intervals around the best one: the width in ln tf is
    multiplied by 2 / (k - 1).  The search stops once hi / lo - 1 <= rtol, i.e. ln(hi / lo) <= ln(1 + rtol):
        rounds = max(1, ceil(ln(ln(hi / lo) / ln(1 + rtol)) / ln((k - 1) / 2)))
    objective calls, rounds * k temperatures (the formula of _bracket_search's docstring)."""
    return max(1, math.ceil(math.log(math.log(hi / lo) / math.log1p(rtol)) / math.log((k - 1) / 2)))


class Counting:
    def __init__(self, f):
        self.f, self.calls, self.points = f, 0, 0

    def __call__(self, tfs):
        assert tfs.shape[0] == K and np.all(np.diff(tfs, axis=0) > 0)
        self.calls += 1
        self.points += tfs.shape[0]
        return self.f(tfs)


@pytest.mark.parametrize("centre", [3.4349, 0.0123, 77.7, 1.0])
@pytest.mark.parametrize("span", [1e4, 1e2])
def test_parabola_in_ln_tf(trpl, centre, span):
    obj = Counting(lambda t: 5.0 - (np.log(t) - math.log(centre)) ** 2)
    lo, hi = 1.0 / span, 1.0 * span
    tf, val, info = trpl.posterior._bracket_search(obj, [lo], [hi], K, RTOL)
    assert abs(tf[0] / centre - 1) <= RTOL, (tf, centre)
    assert info["lo"][0] <= centre <= info["hi"][0] and info["hi"][0] / info["lo"][0] - 1 <= RTOL
    assert info["lo"][0] <= tf[0] <= info["hi"][0] and val[0] == obj.f(tf)[0]
    assert not info["at_edge"][0]
    n = predicted_rounds(lo, hi, K, RTOL)
    assert obj.calls == info["scans"] == n and obj.points == n * K, (obj.calls, n)
    assert n == {1e4: 5, 1e2: 5}[span]


def test_the_round_count_follows_the_formula_over_k_and_rtol(trpl):
    for k, rtol, span in ((4, 1e-3, 10.0), (8, 1e-6, 1e4), (64, 1e-9, 1e4), (64, 1e-2, 1e4), (33, 1e-6, 1e6)):
        calls = []
        tf, _, info = trpl.posterior._bracket_search(lambda t: calls.append(1) or -(np.log(t) - 0.3217) ** 2,
                                                     [1 / span], [span], k, rtol)
        assert len(calls) == info["scans"] == predicted_rounds(1 / span, span, k, rtol), (k, rtol, span, len(calls))
        assert abs(tf[0] / math.exp(0.3217) - 1) <= rtol


def test_a_maximum_at_the_edge_is_flagged_not_silently_accepted(trpl):
    for f, want in ((lambda t: np.log(t), 1e4), (lambda t: -np.log(t), 1e-4)):
        tf, _, info = trpl.posterior._bracket_search(f, [1e-4], [1e4], K, RTOL)
        assert info["at_edge"][0] and abs(tf[0] / want - 1) <= RTOL
        assert info["scans"] <= predicted_rounds(1e-4, 1e4, K, RTOL)          # an end point shrinks faster
    # an interior maximum one grid point from the edge is not an edge
    first = np.exp(np.log(1e-4) + (np.log(1e4) - np.log(1e-4)) / (K - 1))
    tf, _, info = trpl.posterior._bracket_search(lambda t: -(np.log(t) - np.log(first)) ** 2, [1e-4], [1e4], K, RTOL)
    assert not info["at_edge"][0] and abs(tf[0] / first - 1) <= RTOL


def test_a_plateau_resolves_to_its_lowest_temperature(trpl):
    a, b = 2.0, 30.0
    f = lambda t: ((t >= a) & (t <= b)).astype(float)
    runs = [trpl.posterior._bracket_search(f, [1e-4], [1e4], K, RTOL) for _ in range(2)]
    tf, val, info = runs[0]
    assert val[0] == 1.0 and a <= tf[0] <= a * (1 + RTOL), tf                   # ties go to the lowest index, every round
    assert runs[1][0][0] == tf[0] and runs[1][2]["scans"] == info["scans"]      # deterministic
    # all equal everywhere: the first point of the outer bracket, flagged as an edge
    tf, _, info = trpl.posterior._bracket_search(lambda t: np.zeros_like(t), [1e-4], [1e4], K, RTOL)
    assert tf[0] == 1e-4 and info["at_edge"][0]
    # NaN values never win
    tf, _, info = trpl.posterior._bracket_search(lambda t: np.where(t < 1.0, np.nan, -np.log(t)), [1e-4], [1e4], K, RTOL)
    assert 1.0 <= tf[0] <= 1.0 + 2 * RTOL and not info["at_edge"][0]


def test_columns_are_searched_independently(trpl):
    """Several brackets in one call give, column by column, the bits of the separate calls (what makes
    calc_max_uncertainty equal to one find_best_tf per parameter), whatever round each column finishes in."""
    centres = np.array([0.5, 3.0, 9999.9, 1e-4, 42.0])
    los, his = np.array([1e-4, 1e-4, 1e-4, 1e-4, 41.0]), np.array([1e4, 1e4, 1e4, 1e4, 43.0])
    f = lambda c: (lambda t: -(np.log(t) - np.log(c)) ** 2)
    tf, val, info = trpl.posterior._bracket_search(lambda t: -(np.log(t) - np.log(centres)[None, :]) ** 2, los, his, K, RTOL)
    for i, c in enumerate(centres):
        tf1, val1, info1 = trpl.posterior._bracket_search(f(c), [los[i]], [his[i]], K, RTOL)
        assert tf1[0] == tf[i] and val1[0] == val[i] and info1["lo"][0] == info["lo"][i] and info1["hi"][0] == info["hi"][i]
        assert info1["scans"] == info["rounds"][i] and info1["at_edge"][0] == info["at_edge"][i]
    assert info["scans"] == info["rounds"].max() and info["rounds"][4] < info["rounds"][0]


def test_bad_brackets_are_refused(trpl):
    s = trpl.posterior._bracket_search
    for lo, hi in (([0.0], [1.0]), ([2.0], [1.0]), ([1.0], [np.inf]), ([1.0, 2.0], [3.0])):
        with pytest.raises(ValueError):
            s(lambda t: t, lo, hi, K, RTOL)
    with pytest.raises(ValueError):
        s(lambda t: t, [1.0], [2.0], 3, RTOL)
    with pytest.raises(ValueError):
        s(lambda t: t, [1.0], [2.0], K, 0.0)
