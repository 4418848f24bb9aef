"""The conditions tests/test_gpu_stepper_grids.py relies on, proved on the CPU from the reference alone (tests/grid_cases.py) at
every grid size and film: every system converges at the default cap, every PL column is above 1e-12 of PL(0) and above the
cancellation floor (floor_col == -1 by the header's rule), forced_max finds a cap away from every knife edge, and no cut
decision of the seeded inputs lies within the likelihood gate of the level."""
import numpy as np
import pytest

import grid_cases as G


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


@pytest.mark.parametrize("film", G.FILMS)
@pytest.mark.parametrize("L", G.SIZES)
def test_every_system_converges_far_above_the_floor(L, film):
    ini, lens = G.film(film, L)
    X = G.samples()
    for c, r in enumerate(G.solution(L, film)):
        pl = r["plI"]
        assert not r["status"].any() and pl.shape == (G.S, G.T + 1)
        assert (np.abs(pl) >= 1e-12 * np.abs(pl[:, :1])).all()                         # gpu_common.above_floor: nothing left out
        ratio = pl / G.excess_scale(X, lens[c], L)[:, None]
        assert (pl > 0).all() and (ratio >= G.FLOOR).all(), float(ratio.min())         # include/trpl.h: floor_col = -1
        assert ratio.min() > 1e3                                                       # K / r is below 1e-11 of the envelope


@pytest.mark.parametrize("L,film", G.FORCED_CASES)
def test_forced_max_splits_the_batch_away_from_a_knife_edge(oracle, L, film):
    sol = G.solution(L, film)
    steps = np.concatenate([r["step_iters"] for r in sol])
    cap = G.forced_max(steps)
    m = steps.max(axis=1)
    assert (m >= cap + 2).any() and (m <= cap - 1).any() and not ((m == cap) | (m == cap + 1)).any()
    forced = G.solution(L, film, MAX=cap)
    st = np.concatenate([r["status"] for r in forced])
    assert np.array_equal(st != 0, m >= cap)                                           # exactly the systems above the cap
    for r0, r1 in zip(sol, forced):
        for s in range(G.S):
            t = r1["status"][s] - 1 if r1["status"][s] else G.T + 1
            assert np.array_equal(r1["plI"][s, :t], r0["plI"][s, :t]) and np.isnan(r1["plI"][s, t:]).all()


def test_forced_max_raises_when_no_cap_exists():
    for L in (4, 8, 16):                                  # grid_cases.FORCED_CASES: consecutive counts, no cap clear of all
        with pytest.raises(ValueError):
            G.forced_max(np.concatenate([r["step_iters"] for r in G.solution(L, "thick")]))
    with pytest.raises(ValueError):
        G.forced_max(np.array([[3, 2], [4, 2], [5, 2], [6, 2]]))
    assert G.forced_max(np.array([[3, 2], [9, 2]])) == 4


@pytest.mark.parametrize("film", G.FILMS)
@pytest.mark.parametrize("L", G.SIZES)
def test_reference_sums_agree_and_no_cut_decision_is_on_a_knife_edge(L, film):
    for offgrid in (False, True):
        ref = G.reference(L, film, offgrid)
        assert ref["n"] == ([151, 148, 145] if not offgrid else [140, 147, 154])[:ref["C"]]
        for c in range(ref["C"]):
            s = ref["sums"][c]
            # the reference's float64 evaluation against the longdouble sums: rounding of n terms
            assert np.max(np.abs(ref["sse"][c] / np.asarray(s["sse"], dtype=float) - 1)) < 1e-12
            assert (ref["sse"][c] > 0.1 * ref["n"][c] * G.NOISE ** 2).all() and (ref["sse"][c] < 100.0 * ref["n"][c]).all()   # O(n)
            w = ref["wts"][c]
            assert (w == 0).sum() == 1 and (w == 0.25).sum() == 1 and (w >= 0).all()
            if offgrid:
                assert ref["times"][c][0] == 0.0 and ref["times"][c][-1] == G.TIME and (np.diff(ref["times"][c]) >= 0).all()
    ref = G.reference(L, film, False)
    level = G.cut_level(ref)
    col, edge = G.cut_plan(ref, level, 1e-8)
    assert not edge.any()
    assert (col >= 0).sum() * 4 >= col.size and (col < 0).sum() * 4 >= col.size
    assert np.array_equal(col >= 0, ref["sse"] > level)
