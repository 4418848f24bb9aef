"""stepper_kernel<L, STRICT, SNAP = true> (csrc/stepper_impl.hpp) -- the instantiation a call takes when it records state
snapshots or resumes from a checkpoint -- at EVERY compiled grid size, L = 4 .. 512, in STRICT and FAST, held to the CPU oracle
(tests/snapshot_cases.py): SnapSink::take's node map in each layout, fail_fill's NaN pattern, the resume prologue's refill of
the BDF history (registers, or the LDS ring from L = 128 on) and status_of_checkpoint.  PL is a sum over nodes and cannot see a
wrong node map; the snapshots can, node by node (tests/test_snapshot_cases_host.py proves on the CPU that neighbouring nodes
of every recorded snapshot differ by >= 100 x the gates below, that everything converges, that a segment has the window's time
step exactly and that the forced cap flags a system before the late resume point).

Gates (none of them new):
  STRICT       the oracle bit for bit: PL, status, iteration totals, plN / plP / plE in every slot; a continued run equals the
               oracle's UNINTERRUPTED run bit for bit.
  FAST         status equal, follows_iteration_path; plN, plP within 1e-6 x the snapshot's largest value node by node, plE
               within 2e-5 x the largest field (tests/test_gpu_snapshots.py); PL, status and iteration totals of the SNAP
               instantiation equal the plain one's bit for bit (it only adds stores); a continued run equals the uninterrupted
               FAST run bit for bit (tests/test_gpu_resume.py).
Measured worst error / allowance per size, film and field: printed, and in the record file test_snapshot_grids.json."""
import numpy as np
import pytest

import snapshot_cases as C
from gpu_common import follows_iteration_path, record
from grid_cases import LAYOUT_SIZES
from test_gpu_resume import _split_run

pytestmark = pytest.mark.gpu

MODES = {"strict": dict(strict=True), "single": dict(kernel="single")}
FIELDS = ("plN", "plP", "plE")
REC = {}


def _note(key, **figures):
    REC.setdefault(key, {}).update({k: float(v) for k, v in figures.items()})
    print("%s: %s" % (key, ", ".join("%s %.3g" % kv for kv in figures.items())))
    record("snapshot_grids", REC)


def _snap_run(gpu, L, film, **kw):
    X, length, ini = C.case(L, film)
    got = {}
    pl, st, it, _ = gpu.solve_pl(X, length, C.TIME, L, C.T, ini, snap_steps=C.snaps(film), snapshots=got, **kw)
    return pl, st, it, got


def _same_where_finite(got, want, label):
    """The NaN pattern is the reference's and every other value has its bits."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), label
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]), label


def _fast_gates(got, want, rows, label):
    """plN, plP, plE of the systems `rows` over the recorded slots against the oracle: the worst error / allowance per field
    (1e-6 x the snapshot's largest value for plN and plP, 2e-5 x the largest field for plE).  t = 0 has no field: exactly 0."""
    worst = {}
    for k, gate in (("plN", C.GATE_NP), ("plP", C.GATE_NP), ("plE", C.GATE_E)):
        first = 1 if k == "plE" else 0
        g, w = got[k][rows, first:C.N_LIVE], want[k][rows, first:C.N_LIVE]
        assert np.isfinite(g).all() and np.isfinite(w).all(), (label, k)
        top = np.abs(w).max(axis=2, keepdims=True)
        assert (top > 0).all(), (label, k)
        ratio = np.abs(g - w) / (gate * top)
        worst[k] = float(ratio.max())
        assert (ratio < 1.0).all(), (label, k, worst[k], np.argwhere(ratio >= 1.0)[:4].tolist())
    assert (got["plE"][rows, 0] == 0).all(), label
    return worst


def _untouched_slots_and_edges(got, L, label):
    for k in FIELDS:
        assert (got[k][:, C.N_LIVE:] == 0).all(), (label, k)                        # the repeated step, the step beyond T
    e = got["plE"][:, :C.N_LIVE]
    live = ~np.isnan(e[:, :, 0])
    assert (e[:, :, 0][live] == 0).all() and (e[:, :, L][live] == 0).all(), label   # E_0 = E_L = 0


# ------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("film", C.FILMS)
@pytest.mark.parametrize("L", C.SIZES)
def test_strict_snapshots_are_the_oracles(gpu, oracle, L, film):
    want = C.solution(L, film)
    pl, st, it, got = _snap_run(gpu, L, film, strict=True)
    label = "L %d %s strict" % (L, film)
    assert not want["status"].any() and np.array_equal(st, want["status"]), label
    assert np.array_equal(pl, want["plI"]) and np.array_equal(it, want["iters_total"]), label
    for k in FIELDS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (label, k)
    _untouched_slots_and_edges(got, L, label)
    assert (got["plN"][:, :C.N_LIVE] > 0).all() and (got["plP"][:, :C.N_LIVE] > 0).all(), label


# ------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("film", C.FILMS)
@pytest.mark.parametrize("L", C.SIZES)
def test_fast_snapshots_against_the_oracle_and_the_plain_instantiation(gpu, oracle, L, film):
    X, length, ini = C.case(L, film)
    want = C.solution(L, film)
    pl, st, it, got = _snap_run(gpu, L, film, kernel="single")
    label = "L %d %s single" % (L, film)
    assert np.array_equal(st, want["status"]) and not st.any(), label
    follows_iteration_path(it, want["iters_total"], label)
    worst = _fast_gates(got, want, np.arange(C.S), label)
    _untouched_slots_and_edges(got, L, label)
    # the SNAP instantiation only adds stores: the plain call's PL, status and iteration totals, bit for bit
    pl0, st0, it0, _ = gpu.solve_pl(X, length, C.TIME, L, C.T, ini, kernel="single")
    same = pl.tobytes() == pl0.tobytes() and np.array_equal(st, st0) and np.array_equal(it, it0)
    _note("L%d_%s" % (L, film), snap_equals_plain_bits=same, **{"fast_%s_worst_over_allowance" % k: v for k, v in worst.items()})
    assert same, (label, "PL differs from the plain instantiation's in %d of %d values" % ((pl != pl0).sum(), pl.size),
                  it.tolist(), it0.tolist())


# ------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("t0", C.T0S)
@pytest.mark.parametrize("film", C.FILMS)
@pytest.mark.parametrize("L", C.SIZES)
def test_continued_run_is_the_uninterrupted_run(gpu, oracle, L, film, t0):
    """STRICT: the continuation is the ORACLE's uninterrupted run bit for bit (PL, iteration totals with the step at t0
    counted once, the late snapshots); FAST: the uninterrupted FAST run's.  Columns before ceil(t0 / plT) of the caller's
    buffer keep a sentinel.  plT = 4 as well at one size per node layout and at L = 512."""
    X, length, ini = C.case(L, film)
    late = C.late_steps(t0)
    for plT in (1, 4) if (L in LAYOUT_SIZES or L == 512) else (1,):
        want = C.late_solution(L, film, t0, plT=plT)
        assert not want["status"].any() and want["plI"].shape == (C.S, C.T // plT + 1)
        first = -(-t0 // plT)
        for mode, kw in MODES.items():
            label = "L %d %s t0 %d plT %d %s" % (L, film, t0, plT, mode)
            (pl, st, it, sn), (pl2, st_a, st_b, it2, sn2) = _split_run(gpu, X, length, C.TIME, L, C.T, ini, t0, plT=plT, late=late, **kw)
            assert not st.any() and not st_a.any() and not st_b.any(), label
            ref = dict(want, iters=want["iters_total"]) if mode == "strict" else dict(plI=pl, iters=it, **sn)
            assert pl2.shape == ref["plI"].shape and pl2.tobytes() == ref["plI"].tobytes(), label
            assert np.array_equal(it2, ref["iters"]), (label, it2.tolist(), ref["iters"].tolist())
            for k in FIELDS:
                assert sn2[k].shape == ref[k].shape and np.array_equal(sn2[k], ref[k]), (label, k)
                assert np.isfinite(sn2[k]).all() and np.abs(sn2[k]).max(axis=2).min() > 0, (label, k)
            # what the continuation writes: columns from ceil(t0 / plT) on, nothing before
            ck = {}
            gpu.solve_pl(X, length, C.TIME * t0 / C.T, L, t0, ini, plT=plT, snap_steps=gpu.checkpoint_steps(t0), snapshots=ck,
                         snap_raw=True, **kw)
            out = np.full((C.S, C.T // plT + 1), -3.0)
            gpu.solve_pl(X, length, C.TIME, L, C.T, None, plT=plT, out=out, resume=(t0, ck["plN"], ck["plP"], ck["plE"]), **kw)
            assert (out[:, :first] == -3.0).all() and out[:, first:].tobytes() == ref["plI"][:, first:].tobytes(), label


# ------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("L", C.FORCED_SIZES)
def test_forced_nonconvergence_snapshots_and_resume_through_a_flag(gpu, oracle, L, mode):
    """MAX = forced_max(...) on the thin film.  A flagged system's PL and snapshot slots are NaN from its failing step on, its
    wavefront's other systems' rows are complete; STRICT has the oracle's bits wherever the oracle has a number, FAST the
    gates of the snapshot test on the live systems.  Then a checkpoint at step 37, after the flag, and a resume: the flagged
    systems keep their status word and take no step, their PL stays NaN from the failing step on; everything else equals the
    uninterrupted run bit for bit."""
    film = "thin"
    X, length, ini = C.case(L, film)
    cap = C.forced_cap(L)
    want = C.solution(L, film, MAX=cap)
    flagged = want["status"] != 0
    assert flagged.any() and not flagged.all()
    kw = dict(MAX=cap, **MODES[mode])
    label = "L %d %s MAX %d" % (L, mode, cap)
    pl, st, it, got = _snap_run(gpu, L, film, **kw)
    assert np.array_equal(st, want["status"]), (label, st.tolist(), want["status"].tolist())
    for s in range(C.S):
        assert np.isnan(pl[s, (st[s] - 1 if st[s] else C.T + 1):]).all(), (label, s)
    assert np.array_equal(np.isnan(pl), np.isnan(want["plI"])), label
    for k in FIELDS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (label, k)
        assert np.isfinite(got[k][~flagged]).all(), (label, k)                      # the partners' rows are complete
    if mode == "strict":
        _same_where_finite(pl, want["plI"], label)
        assert np.array_equal(it, want["iters_total"]), label
        for k in FIELDS:
            _same_where_finite(got[k], want[k], (label, k))
    else:
        follows_iteration_path(it[~flagged], want["iters_total"][~flagged], label)
        worst = _fast_gates(got, want, np.flatnonzero(~flagged), label)
        _note("L%d_%s" % (L, film), **{"forced_fast_%s_worst_over_allowance" % k: v for k, v in worst.items()})
    _untouched_slots_and_edges(got, L, label)

    # resume through the flag
    t0 = max(C.T0S)
    late = C.late_steps(t0)
    assert (st[flagged] - 1 < t0).any()
    early = flagged & (st - 1 <= t0)                           # flagged by the checkpoint: status travels in its NaN payload
    (plf, stf, itf, snf), (pl2, st_a, st_b, it2, sn2) = _split_run(gpu, X, length, C.TIME, L, C.T, ini, t0, late=late, **kw)
    assert np.array_equal(stf, st) and plf.tobytes() == pl.tobytes() and np.array_equal(itf, it), label
    assert np.array_equal(st_a[early], st[early]) and not st_a[~early].any(), (label, st_a.tolist())
    assert np.array_equal(st_b, st), (label, st_b.tolist(), st.tolist())            # the ORIGINAL failing step
    for s in np.flatnonzero(flagged):
        assert np.isnan(pl2[s, st[s] - 1:]).all(), (label, s)
    _same_where_finite(pl2, plf, label)
    for k in FIELDS:
        _same_where_finite(sn2[k], snf[k], (label, k))
        assert np.isfinite(sn2[k][~flagged]).all() and np.isnan(sn2[k][early]).all(), (label, k)
    assert np.array_equal(it2, itf), (label, it2.tolist(), itf.tolist())
    if mode == "strict":
        ref = C.late_solution(L, film, t0, MAX=cap)
        assert np.array_equal(st_b, ref["status"]) and np.array_equal(it2, ref["iters_total"]), label
        _same_where_finite(pl2, ref["plI"], label)
        for k in FIELDS:
            _same_where_finite(sn2[k], ref[k], (label, k))
    print("%s: flags %d of %d systems, at steps %s" % (label, flagged.sum(), C.S, sorted((st[flagged] - 1).tolist())))


# ------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("film", C.FILMS)
@pytest.mark.parametrize("L", [8, 256])
def test_device_entry_unordered_steps_only_plp(gpu, oracle, L, film):
    """trpl_solve_pl_snap_dev with unordered steps and only plP requested: the oracle's plP bit for bit, and not one value
    written on either side of it."""
    import torch
    X, length, ini = C.case(L, film)
    steps = [10, 0, 3]
    want = oracle.pvsim(X, length, C.TIME, L, C.T, ini, snap_steps=steps)
    dev = torch.device("cuda", 0)
    n, guard = C.S * len(steps) * L, 2 * (L + 1) * len(steps)
    buf = torch.full((guard + n + guard,), -7.0, dtype=torch.float64, device=dev)
    plP = buf[guard:guard + n].view(C.S, len(steps), L)
    plP.zero_()
    pl = torch.empty((C.S, C.T + 1), dtype=torch.float64, device=dev)
    st = torch.full((C.S,), -1, dtype=torch.int32, device=dev)
    gpu.device.solve_pl_snap_device(torch.from_numpy(X.copy()).to(dev), length, C.TIME, L, C.T, torch.from_numpy(ini.copy()).to(dev),
                                    pl, steps, plP=plP, status=st, flags=gpu.FLAG_STRICT)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert not st.cpu().numpy().any() and np.array_equal(pl.cpu().numpy(), want["plI"])
    assert np.array_equal(host[guard:guard + n].reshape(C.S, len(steps), L), want["plP"]), (L, film)
    assert (host[:guard] == -7.0).all() and (host[guard + n:] == -7.0).all(), (L, film)
