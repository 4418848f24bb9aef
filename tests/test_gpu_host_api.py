"""Host-buffer entry points under concurrency and in place: calls from several host threads overlap and agree; a large PL
matrix is written by the kernel straight into the caller's mapped buffer."""
import numpy as np
import pytest


pytestmark = pytest.mark.gpu


def test_host_calls_from_several_threads_overlap_and_agree(trpl, gpu):
    """Host-buffer entry points are re-entrant (private stream, stream-ordered allocations, thread-local
    error string): eight threads solving different curves / sample sets at once return exactly what
    the same calls return one after the other, and an error in one thread stays in that thread."""
    from concurrent.futures import ThreadPoolExecutor
    ini, lengths = trpl.workloads.power_scan(128)
    jobs = [(trpl.workloads.samples(200 + 17 * k, seed=30 + k)[:, :12], k % 3) for k in range(8)]

    def run(job):
        X, c = job
        pl, st, it, _ = trpl.solve_pl(X, lengths[c], 2.0, 128, 80, ini[c])
        lp = np.log10(np.maximum(pl, 1e-300))
        trpl.fastlog(pl, 1e-300)
        return pl, lp, st, it

    serial = [run(j) for j in jobs]
    with ThreadPoolExecutor(max_workers=8) as pool:
        threaded = list(pool.map(run, jobs))
    for a, b in zip(serial, threaded):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert np.allclose(a[0], a[1], rtol=1e-15, atol=0)

    def bad(_):
        try:
            trpl.solve_pl(jobs[0][0], lengths[0], 2.0, 100, 80, ini[0][:100])       # L not a power of two
        except trpl.TrplError as e:
            return str(e)
        return None
    with ThreadPoolExecutor(max_workers=2) as pool:
        msgs = list(pool.map(bad, range(4))) + [r[0].shape for r in pool.map(run, jobs[:2])]
    assert all(isinstance(m, str) and "power of two" in m for m in msgs[:4])


def test_host_buffer_solve_writes_pl_straight_into_the_callers_memory(gpu):
    """A PL block above 8 MB is written by the kernel directly into the caller's (page-locked and mapped for the
    call) numpy buffer -- also a row-strided view of a larger array, float32 and float64 -- and equals the
    device-resident solve bit for bit; the bytes between the rows of the view are untouched."""
    import torch
    w = gpu.workloads
    ini, lens = w.power_scan(128)
    S, T = 1024, 2200
    Time = T * 0.025
    X = w.samples(S, seed=81)[:, :12]
    dev = torch.device("cuda", 0)
    Xd = torch.from_numpy(X.copy()).to(dev)
    ini_d = torch.from_numpy(ini[1]).to(dev)
    for dtype, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        ref = torch.empty((S, T + 1), dtype=tdt, device=dev)
        gpu.device.solve_pl_device(Xd, lens[1], Time, 128, T, ini_d, ref)
        torch.cuda.synchronize()
        ref = ref.cpu().numpy()
        plain = np.empty((S, T + 1), dtype=dtype)
        assert plain.nbytes > (8 << 20)
        _, st, it, sec = gpu.solve_pl(X, lens[1], Time, 128, T, ini[1], out=plain)
        assert sec > 0 and not st.any() and np.array_equal(plain, ref)
        big = np.full((S, T + 1 + 37), -5.0, dtype=dtype)
        view = big[:, 5:5 + T + 1]
        gpu.solve_pl(X, lens[1], Time, 128, T, ini[1], out=view)
        assert np.array_equal(view, ref)
        assert (big[:, :5] == -5.0).all() and (big[:, 5 + T + 1:] == -5.0).all()
    # the same buffer again right away (registration is per call), and from two threads at once
    from concurrent.futures import ThreadPoolExecutor
    bufs = [np.empty((S, T + 1), dtype=np.float32) for _ in range(2)]
    with ThreadPoolExecutor(2) as ex:
        list(ex.map(lambda b: gpu.solve_pl(X, lens[1], Time, 128, T, ini[1], out=b), bufs))
    assert np.array_equal(bufs[0], bufs[1])


# ----------------------------------------------------------------------------- the staged solve against its _dev form
S5, L5, T5, DT5 = 5, 32, 96, 2.0 ** -5          # DT5 a power of two: a segment of t0 steps has the window's time step exactly


@pytest.fixture(scope="module")
def small(gpu):
    w = gpu.workloads
    ini, lens = w.twothick(L5)
    return dict(X=np.ascontiguousarray(w.samples(S5, seed=13)[:, :12]), ini=np.ascontiguousarray(ini[0]), length=float(lens[0]))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _solve_snap(gpu, p, dev, plT, pl, ld, status, iters, steps, n_snap, plN, plP, plE):
    """trpl_solve_pl_snap (numpy buffers; returns seconds) or trpl_solve_pl_snap_dev (CUDA tensors), the arguments as given."""
    import ctypes
    import torch
    a = gpu._abi
    at = (lambda t: None if t is None else t.data_ptr()) if dev else a.ptr
    give = (lambda v: torch.from_numpy(v).cuda()) if dev else (lambda v: v)
    X, ini = give(p["X"]), give(p["ini"])
    sec = ctypes.c_double(-1.0)
    args = [at(X), S5, p["length"], T5 * DT5, L5, T5, plT, 7, 10000, at(ini), at(pl), pl.element_size() if dev else pl.itemsize, ld,
            at(status), at(iters), a.ptr(steps), n_snap, at(plN), at(plP), at(plE), 0]
    if dev:
        a.check(a.lib().trpl_solve_pl_snap_dev(*args, _stream()))
        torch.cuda.synchronize()
        return None
    a.check(a.lib().trpl_solve_pl_snap(*args, 0, ctypes.byref(sec)))
    return sec.value


@pytest.mark.parametrize("outputs", [False, True], ids=["status-null", "status-given"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("plT", [1, 4])
def test_staged_solve_equals_the_device_form_bit_for_bit(gpu, small, plT, dtype, outputs):
    """A PL matrix below the mapping threshold goes through device memory and a pitched copy back: rows of ncol columns in a
    leading dimension of ncol + 3, the padding keeps the caller's sentinel; status and iters_total both NULL or both given."""
    import torch
    ncol = T5 // plT + 1
    ld = ncol + 3
    host = np.full((S5, ld), -7.0, dtype=dtype)
    dev = torch.from_numpy(host.copy()).cuda()
    st, it = (np.full(S5, 9, np.int32), np.full(S5, -1, np.int64)) if outputs else (None, None)
    dst, dit = (torch.from_numpy(st.copy()).cuda(), torch.from_numpy(it.copy()).cuda()) if outputs else (None, None)
    sec = _solve_snap(gpu, small, False, plT, host, ld, st, it, None, 0, None, None, None)
    _solve_snap(gpu, small, True, plT, dev, ld, dst, dit, None, 0, None, None, None)
    assert np.isfinite(sec) and sec > 0
    assert np.isfinite(host[:, :ncol]).all() and (host[:, :ncol] > 0).all() and (host[:, ncol:] == -7.0).all()
    assert np.array_equal(host, dev.cpu().numpy())
    if outputs:
        assert not st.any() and (it > 0).all()
        assert np.array_equal(st, dst.cpu().numpy()) and np.array_equal(it, dit.cpu().numpy())


def test_staged_snapshots_keep_the_unfilled_slot_and_take_pln_alone(gpu, small):
    """n_snap = 3 with one step outside [0, T]: that slot keeps the caller's sentinel, in the host-buffer form (the snapshot
    arrays go up and come back) as in the _dev form; plP and plE are NULL."""
    import torch
    steps = np.array([10, T5 + 5, 40], dtype=np.int64)
    plN = np.full((S5, 3, L5), -3.0)
    dN = torch.from_numpy(plN.copy()).cuda()
    pl, dpl = np.empty((S5, T5 + 1)), torch.empty((S5, T5 + 1), dtype=torch.float64, device="cuda")
    sec = _solve_snap(gpu, small, False, 1, pl, T5 + 1, None, None, steps, 3, plN, None, None)
    _solve_snap(gpu, small, True, 1, dpl, T5 + 1, None, None, steps, 3, dN, None, None)
    assert np.isfinite(sec) and sec > 0
    assert (plN[:, 1] == -3.0).all() and np.isfinite(plN).all() and (plN[:, [0, 2]] != -3.0).all() and not np.array_equal(plN[:, 0], plN[:, 2])
    assert np.array_equal(plN, dN.cpu().numpy()) and np.array_equal(pl, dpl.cpu().numpy())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_staged_resume_keeps_the_columns_before_t0_in_a_padded_matrix(gpu, small, dtype):
    """The small twin of test_continue_into_a_large_host_buffer_written_in_place: below the mapping threshold a resume stages the
    caller's matrix up and back (pitched, rows of ncol columns in ncol + 3), so columns before ceil(t0 / plT) and the padding
    keep the caller's sentinel and the rest is the uninterrupted run."""
    p, t0, plT = small, 41, 4
    Time, ncol, first = T5 * DT5, T5 // plT + 1, -(-41 // 4)
    full, st, _, _ = gpu.solve_pl(p["X"], p["length"], Time, L5, T5, p["ini"], plT=plT, dtype=dtype)
    ck = {}
    gpu.solve_pl(p["X"], p["length"], Time * t0 / T5, L5, t0, p["ini"], plT=plT, snap_steps=gpu.checkpoint_steps(t0), snapshots=ck,
                 snap_raw=True, dtype=dtype)
    big = np.full((S5, ncol + 3), -3.0, dtype=dtype)
    _, st_b, _, sec = gpu.solve_pl(p["X"], p["length"], Time, L5, T5, None, plT=plT, out=big[:, :ncol],
                                   resume=(t0, ck["plN"], ck["plP"], ck["plE"]))
    assert not st.any() and not st_b.any() and np.isfinite(sec) and sec > 0
    assert (big[:, :first] == -3.0).all() and (big[:, ncol:] == -3.0).all()
    assert np.array_equal(big[:, first:ncol], full[:, first:])


def test_solve_seconds_are_zero_at_the_early_return(gpu, small):
    import ctypes
    a, p = gpu._abi, small
    sec = ctypes.c_double(-1.0)
    pl = np.empty((1, T5 + 1))
    a.check(a.lib().trpl_solve_pl(a.ptr(p["X"]), 0, p["length"], T5 * DT5, L5, T5, 1, 7, 10000, a.ptr(p["ini"]), a.ptr(pl), 8, T5 + 1,
                                  None, None, 0, 0, ctypes.byref(sec)))
    assert sec.value == 0.0
