"""The cases of tests/test_gpu_snapshot_grids.py and their CPU reference: one short window at every grid size the one-system
stepper is compiled for, two films with one curve each, the state snapshots plN / plP / plE at steps on the BDF ramp, in the
middle and at the end of the window, and the late snapshots of a run that is checkpointed and continued -- all from the CPU
oracle alone (oracle.pvsim with snap_steps).  tests/test_snapshot_cases_host.py proves on the CPU what the GPU tests rely on
(everything converges, a segment has the window's time step exactly, neighbouring nodes of every snapshot differ by far more
than the FAST gates so that a swapped node is seen, forced_max finds a cap that flags a system before the late resume point).
Plain module: no fixtures, nothing of the product but `workloads` (through grid_cases)."""
import functools

import grid_cases as G

SIZES = G.SIZES
FILMS = G.FILMS                    # "thick": curve 0 of workloads.power_scan(L) (2000 nm); "thin": the 311 nm film
S, T, DT = G.S, 96, 2.0 ** -5      # a power of two: a segment of t0 steps over TIME * t0 / T has the window's time step exactly
TIME = T * DT                      # 3.0 ns
assert S == 5
SNAPS = [0, 1, 2, 4, 5, 48, 96, 96, 200]   # the BDF ramp, a mid step, the last step, a repeated step and one beyond T
# The 311 nm film is flat within 2 ns: from step 12 on (L = 512; step 30 at L = 4) neighbouring nodes of plN and plP differ by
# less than 100 x the FAST gate, at steps 48 and 96 by about the gate itself (L = 4) or 2 % of it (L = 512), and a swapped node
# would pass.  So on that film the mid step and the (repeated) last recorded step are moved earlier, to 7 and 10, still past
# the BDF ramp; the snapshot at t = T is held on the 2000 nm film, at every size (tests/test_snapshot_cases_host.py).
SNAPS_THIN = [0, 1, 2, 4, 5, 7, 10, 10, 200]
N_LIVE = 7                         # slots 0 .. 6 are recorded; slot 7 (the repeat) and slot 8 (beyond T) are never written
T0S = (4, 37)                      # resume points: the minimum, and an odd step off any PL stride
FORCED_SIZES = (4, 64, 512)        # one size per FAST node layout, on the thin film (grid_cases.FORCED_CASES)
GATE_NP, GATE_E = 1e-6, 2e-5       # tests/test_gpu_snapshots.py's FAST gates, times the snapshot's largest value


def snaps(film):
    return SNAPS_THIN if film == "thin" else SNAPS


def late_steps(t0):
    return (t0, t0 + 1, 80, T)


def case(L, film):
    """(matPar (S, 12), length, excitation (L,)) of the film's one curve."""
    ini, lens = G.film(film, L)
    return G.samples()[:, :12], float(lens[0]), ini[0]


def _solve(L, film, T_, snap_steps, MAX=10000, plT=1):
    import oracle
    X, length, ini = case(L, film)
    return oracle.pvsim(X, length, T_ * DT, L, T_, ini, plT=plT, MAX=MAX, want_step_iters=True, snap_steps=list(snap_steps),
                        nthreads=G.nthreads())


@functools.lru_cache(maxsize=None)
def solution(L, film, MAX=10000):
    """The oracle's dict (plI, status, iters_total, step_iters, plN, plP, plE) of the window with the snapshots snaps(film)."""
    return _solve(L, film, T, snaps(film), MAX=MAX)


@functools.lru_cache(maxsize=None)
def late_solution(L, film, t0, MAX=10000, plT=1):
    """The same window (uninterrupted) with the snapshots of a run continued at t0: late_steps(t0)."""
    return _solve(L, film, T, late_steps(t0), MAX=MAX, plT=plT)


def forced_cap(L):
    """grid_cases.forced_max on the thin film's per-step iteration counts: flags some systems, clear of every knife edge."""
    return G.forced_max(solution(L, "thin")["step_iters"])
