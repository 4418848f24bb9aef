"""The conditions tests/test_gpu_snapshot_grids.py relies on, proved on the CPU from the reference alone (tests/
snapshot_cases.py) at every grid size and film, over the GPU tests' own window (nothing is shortened): every system converges
far above the cancellation floor; a segment of t0 steps has the window's time step exactly; in every recorded snapshot of every
system neighbouring nodes differ by at least 100 times the FAST gate, so that a node map that swaps two neighbours -- let alone
two distant nodes -- cannot pass; and forced_max finds a cap on the thin film that flags a system before the late resume point
and leaves one alive."""
import numpy as np
import pytest

import snapshot_cases as C
from gpu_common import above_floor


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


@pytest.mark.parametrize("film", C.FILMS)
@pytest.mark.parametrize("L", C.SIZES)
def test_every_system_converges_above_the_floor(L, film):
    sols = [C.solution(L, film)] + [C.late_solution(L, film, t0) for t0 in C.T0S]
    for r in sols:
        assert not r["status"].any() and r["plI"].shape == (C.S, C.T + 1)
        assert above_floor(r["plI"]).all() and (r["plI"] > 0).all()
        assert np.array_equal(r["plI"], sols[0]["plI"]) and np.array_equal(r["iters_total"], sols[0]["iters_total"])
    r = sols[0]
    for k, width in (("plN", L), ("plP", L), ("plE", L + 1)):
        assert r[k].shape == (C.S, len(C.snaps(film)), width)
        assert np.isfinite(r[k]).all() and (r[k][:, C.N_LIVE:] == 0).all()         # the repeat and the step beyond T: untouched
    assert (r["plN"][:, :C.N_LIVE] > 0).all() and (r["plP"][:, :C.N_LIVE] > 0).all()


def test_a_segment_has_the_windows_time_step_exactly():
    for t0 in C.T0S:
        assert (C.TIME * t0 / C.T) / t0 == C.TIME / C.T == C.DT
        assert 4 <= t0 < t0 + 1 < 80 < C.T and C.late_steps(t0) == (t0, t0 + 1, 80, C.T)
    assert C.TIME == 3.0 and C.SNAPS[C.N_LIVE - 1] == C.T
    for film in C.FILMS:                   # slots 0 .. 6 ascending and distinct, slot 7 repeats slot 6, slot 8 is never reached
        sn = C.snaps(film)
        assert len(sn) == 9 and sn[:5] == [0, 1, 2, 4, 5] and sorted(set(sn[:C.N_LIVE])) == sn[:C.N_LIVE]
        assert sn[C.N_LIVE] == sn[C.N_LIVE - 1] <= C.T < sn[-1] and sn[5] > 5


@pytest.mark.parametrize("film", C.FILMS)
@pytest.mark.parametrize("L", C.SIZES)
def test_a_node_swap_would_be_seen_in_every_snapshot(L, film):
    """Per system and recorded slot: the largest difference between neighbouring nodes is >= 100 x the FAST gate on that
    snapshot (1e-6 x max for plN and plP, 2e-5 x max for plE from the first step with a field, t = 1)."""
    r = C.solution(L, film)
    worst = {}
    for k, gate, first in (("plN", C.GATE_NP, 0), ("plP", C.GATE_NP, 0), ("plE", C.GATE_E, 1)):
        v = r[k][:, first:C.N_LIVE]
        top = np.abs(v).max(axis=2)
        step = np.abs(np.diff(v, axis=2)).max(axis=2)
        assert (top > 0).all(), (L, film, k)
        ratio = step / (gate * top)
        worst[k] = float(ratio.min())
        at = np.unravel_index(np.argmin(ratio), ratio.shape)
        assert (ratio >= 100.0).all(), (L, film, k, "system %d, step %d" % (at[0], C.snaps(film)[first + at[1]]), worst[k])
    assert (r["plE"][:, 0] == 0).all()                                              # t = 0: no field yet
    print("L %d %s: smallest neighbour step over gate %s" % (L, film, ", ".join("%s %.3g" % kv for kv in worst.items())))


@pytest.mark.parametrize("L", C.FORCED_SIZES)
def test_forced_cap_flags_a_system_before_the_late_resume_point(L):
    cap = C.forced_cap(L)
    m = C.solution(L, "thin")["step_iters"].max(axis=1)
    forced = C.solution(L, "thin", MAX=cap)
    st = forced["status"]
    assert np.array_equal(st != 0, m >= cap)
    assert ((st > 0) & (st - 1 < max(C.T0S))).any() and (st == 0).any()             # one fails before step 37, one survives
    late = C.late_solution(L, "thin", max(C.T0S), MAX=cap)
    assert np.array_equal(late["status"], st)
    for s in range(C.S):
        t = st[s] - 1 if st[s] else C.T + 1
        assert np.isnan(forced["plI"][s, t:]).all() and np.array_equal(forced["plI"][s, :t], C.solution(L, "thin")["plI"][s, :t])
        for k in ("plN", "plP", "plE"):
            sn = C.snaps("thin")
            dead = np.array([i < C.N_LIVE and sn[i] >= t for i in range(len(sn))])
            assert np.isnan(forced[k][s, dead]).all() and np.isfinite(forced[k][s, ~dead]).all(), (L, s, k)
