"""The paired stepper's persistent launch (stepper_pair_impl.hpp: a launch of more blocks than the device holds waves starts
R = compute units x occupancy one-wave workgroups, and a wave takes its further blocks from a device ticket): which wave runs a block
must not change a bit of it.  Reference of every comparison: the same systems in contiguous even-sized shards of at most R
blocks each -- launches in which every wave runs exactly one block, the mapping of the one-block-per-wave launch.

Shapes: L = 128, Power_scan (C = 3), T = 16, tol 7, TRPL_FLAG_KERNEL_PAIR.  A launch has ((S + 1) / 2) * 3 blocks, a multiple of 3,
so the block counts are the multiples of 3 next to the boundaries: the largest <= R - 1 (no ticket), the smallest >= R (for
R = 2048: R + 1, one wave draws one block), >= R + 3, >= 2 R + 3 (every wave draws at least once), and an odd S past R (the
duplicated tail block is drawn from the ticket).  R is the launcher's own figure and every launch's form is asserted, both from
the library's launch counters (trpl_pair_launch_info: persistent launches, one-block-per-wave launches, R)."""
import ctypes

import numpy as np
import pytest

from gpu_common import DT, follows_iteration_path, nthreads

pytestmark = pytest.mark.gpu

L, C, T, TIME = 128, 3, 16, 16 * DT


def _launch_info(gpu):
    """(persistent launches, one-block-per-wave launches, R) of the paired stepper in this process so far"""
    out = (ctypes.c_int64 * 3)()
    fn = gpu._abi.lib().trpl_pair_launch_info
    fn.argtypes, fn.restype = [ctypes.POINTER(ctypes.c_int64)], None
    fn(out)
    return tuple(int(v) for v in out)


def _resident(gpu):
    """R as the launcher computes it (compute units x hipOccupancyMaxActiveBlocksPerMultiprocessor of the plain paired kernel): one
    two-sample launch makes it ask; the kernel is built for 2 waves on each of a compute unit's 4 SIMDs."""
    import torch
    w = gpu.workloads
    ini, lens = w.power_scan(L)
    gpu.loglik(w.samples(2, seed=31), ini, lens, TIME, L, T, [np.full(T + 1, 20.0)] * C, kernel="pair")
    R = _launch_info(gpu)[2]
    assert R == 8 * torch.cuda.get_device_properties(0).multi_processor_count, R
    return R


def _samples_for_blocks(nblk_min):
    """the even S whose launch has the smallest multiple of 3 blocks >= nblk_min"""
    return 2 * ((nblk_min + C - 1) // C)


@pytest.fixture(scope="module")
def setup(gpu):
    w = gpu.workloads
    ini, lens = w.power_scan(L)
    R = _resident(gpu)
    X = w.samples(_samples_for_blocks(2 * R + 3) + 1, seed=31)
    obs = [np.full(T + 1, 20.0) - 0.02 * np.arange(T + 1)] * C
    return dict(ini=ini, lens=lens, R=R, X=X, obs=obs)


def _run(gpu, s, X, **kw):
    info = {}
    P = gpu.loglik(X, s["ini"], s["lens"], TIME, L, T, s["obs"], info=info, kernel="pair", **kw)
    out = {"P": np.asarray(P)}
    out.update({k: np.asarray(v) for k, v in info.items() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[-1] == len(X)})
    return out


def _sharded(gpu, s, X, **kw):
    per = 2 * (s["R"] // C)                      # an even number of samples with at most R blocks
    assert (per // 2) * C <= s["R"]
    parts = [_run(gpu, s, X[i:i + per], **kw) for i in range(0, len(X), per)]
    return {k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0]}


def _assert_same(a, b, keys=None):
    assert set(a) == set(b)
    for k in keys or a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("P", "sse", "status", "iters_total"):
        assert k in a, k


def _shapes(R):
    below = 2 * ((R - 1) // C)                   # the largest block count <= R - 1
    return {"below_R": below, "at_R": _samples_for_blocks(R), "R_plus_3": _samples_for_blocks(R + 3),
            "2R_plus_3": _samples_for_blocks(2 * R + 3), "odd_tail": _samples_for_blocks(R + 3) + 1}


@pytest.mark.parametrize("shape", ["below_R", "at_R", "R_plus_3", "2R_plus_3", "odd_tail"])
def test_one_launch_equals_its_one_block_per_wave_shards(gpu, setup, shape):
    s = setup
    S = _shapes(s["R"])[shape]
    nblk = ((S + 1) // 2) * C
    assert (nblk <= s["R"] - 1) if shape == "below_R" else (nblk >= s["R"])
    X = s["X"][:S]
    before = _launch_info(gpu)
    one = _run(gpu, s, X)
    after = _launch_info(gpu)
    took_ticket = nblk > s["R"]
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if took_ticket else (0, 1)), (before, after)
    before = after
    parts = _sharded(gpu, s, X)
    after = _launch_info(gpu)
    assert after[0] == before[0] and after[1] > before[1], (before, after)      # every shard: one block per wave
    _assert_same(one, parts)


def test_highest_blocks_against_the_oracle(gpu, oracle, setup):
    """18 systems of the blocks drawn last (the six last samples of the 2 R + 3 shape), against the CPU oracle: likelihoods
    within the suite's 1e-8, iteration totals by follows_iteration_path."""
    s = setup
    S = _shapes(s["R"])["2R_plus_3"]
    X = s["X"][:S]
    got = _run(gpu, s, X)
    assert not got["status"].any()
    tail = X[-6:]
    e_data = [([np.linspace(0, TIME, T + 1)] * C, s["obs"])]
    want = oracle.simulate_loglik(tail, s["ini"], s["lens"], TIME, L, T, e_data, pl_dtype=np.float64, nthreads=nthreads())[0]
    rel = np.abs(got["P"][-6:] - want) / np.abs(want)
    assert rel.max() < 1e-8, rel.max()
    for c in range(C):
        r = oracle.pvsim(tail[:, :12], s["lens"][c], TIME, L, T, s["ini"][c], nthreads=nthreads())
        follows_iteration_path(got["iters_total"][c, -6:], r["iters_total"], "curve %d" % c)


@pytest.mark.parametrize("seam", [False, True], ids=["optimistic", "always_seam"])
def test_waves_that_parked_a_system_take_clean_tickets(gpu, setup, seam):
    """EVERY block below R holds NaN / Inf material parameters (all samples whose blocks start below R), with MAX = 200 so that
    they are flagged and parked in step 0: the launch starts R waves, each of them runs one of those blocks first, so every block
    from R on (2 R + 3 blocks: R + 3 tickets) is run by a wave that parked both its systems before.  The samples of those blocks
    equal, bit for bit, the run with benign rows in the hostile ones' place (park() overwrites the lanes' material
    parameters, the ring and the field history: the next block must start from its own), and the hostile rows are flagged."""
    s = setup
    kw = dict(MAX=200)
    if seam:
        kw["extra_flags"] = gpu._abi.FLAG_PAIR_ALWAYS_SEAM
    R = s["R"]
    S = _shapes(R)["2R_plus_3"]
    clean_X = s["X"][:S]
    n_bad = 2 * ((R - 1) // C + 1)                       # samples 2p, 2p + 1 hold blocks 3p .. 3p + 2: all periods with 3p < R
    assert (n_bad // 2) * C >= R and ((S + 1) // 2) * C >= 2 * R + 3
    bad = clean_X.copy()
    rows = np.arange(n_bad)
    bad[rows[0::4], 9] = np.nan                          # tau_n
    bad[rows[1::4], 4] = np.inf                          # radiative rate
    bad[rows[2::4], 10] = np.nan                         # tau_p
    bad[rows[3::4], 2] = np.nan                          # electron diffusivity
    before = _launch_info(gpu)
    got = _run(gpu, s, bad, **kw)
    assert _launch_info(gpu)[0] == before[0] + 1         # persistent: the blocks from R on were drawn from the ticket
    clean = _run(gpu, s, clean_X, **kw)
    ok = np.arange(n_bad, S)
    assert (clean["status"][:, ok] == 0).mean() > 0.9    # the cap leaves the benign systems alone (all but a few)
    for k in ("P", "sse", "status", "iters_total"):
        assert np.array_equal(got[k][..., ok], clean[k][..., ok], equal_nan=True), k
    assert (got["status"][:, rows] > 0).all() and np.isinf(got["sse"][:, rows]).all()
    assert not np.isfinite(got["P"][rows]).any()
    # and the hostile batch itself does not depend on the launch shape either
    _assert_same(got, _sharded(gpu, s, bad, **kw))


def test_moments_and_cut_sinks_start_every_block_from_fresh_parked_words(gpu, setup):
    """The MOMENTS and CUT sinks keep their sums in LDS words behind the ring: a wave's second block must not see its first
    block's.  R + 3 blocks against the one-block-per-wave shards."""
    s = setup
    S = _shapes(s["R"])["R_plus_3"]
    X = s["X"][:S]
    offsets = [0.0, 0.25]
    _assert_same(_run(gpu, s, X, mag_grid=offsets), _sharded(gpu, s, X, mag_grid=offsets))
    # CUT parks a system at a batch boundary (every 64 PL columns): 81 columns, 2 R + 3 blocks, the level at the median of
    # the uncut sums -- about half of the systems are cut and parked at column 64, and every wave draws at least one more block
    T2 = 80
    s2 = dict(s, obs=[np.full(T2 + 1, 20.0) - 0.02 * np.arange(T2 + 1)] * C)
    X2 = s["X"][:_shapes(s["R"])["2R_plus_3"]]

    def run2(X, **kw):
        info = {}
        P = gpu.loglik(X, s["ini"], s["lens"], T2 * DT, L, T2, s2["obs"], info=info, kernel="pair", **kw)
        out = {"P": np.asarray(P)}
        out.update({k: np.asarray(v) for k, v in info.items() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[-1] == len(X)})
        return out

    level = float(np.median(run2(X2)["sse"]))
    before = _launch_info(gpu)
    one = run2(X2, sse_cut=level)
    assert _launch_info(gpu)[0] == before[0] + 1
    cut = one["cut_col"] >= 0
    assert 0.2 < cut.mean() < 0.8, cut.mean()
    per = 2 * (s["R"] // C)
    parts = [run2(X2[i:i + per], sse_cut=level) for i in range(0, len(X2), per)]
    _assert_same(one, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0]})


def _device_call(gpu, s, S):
    import torch
    from trpl_amd import device as tdev
    dev = torch.device("cuda:0")
    X = torch.from_numpy(np.ascontiguousarray(s["X"][:S])).to(dev)
    ini = torch.from_numpy(s["ini"]).to(dev)
    obs = torch.from_numpy(np.stack(s["obs"])).to(dev)
    flags = gpu._abi.FLAG_KERNEL_PAIR

    def outputs():
        return dict(P=torch.zeros(S, dtype=torch.float64, device=dev), sse=torch.full((C, S), -1.0, dtype=torch.float64, device=dev),
                    status=torch.full((C, S), -7, dtype=torch.int32, device=dev), it=torch.full((C, S), -7, dtype=torch.int64, device=dev))

    def call(o):
        o["P"].zero_()
        tdev.loglik_device(X, ini, s["lens"], TIME, L, T, obs, [T + 1] * C, o["P"], o["sse"], o["status"], o["it"], flags=flags, tol=7)

    return outputs, call


def _host(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_captured_launch_replays_to_identical_outputs(gpu, setup):
    """A launch on a capturing stream is one block per wave (a captured node may run in any number of executable graphs at once:
    it holds no ticket slot); its replays equal the persistent solo launch."""
    import torch
    s = setup
    S = _shapes(s["R"])["R_plus_3"]
    outputs, call = _device_call(gpu, s, S)
    solo = outputs()
    call(solo)
    torch.cuda.synchronize()
    want = _host(solo)
    o = outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(o)                                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    before = _launch_info(gpu)
    with torch.cuda.graph(g):
        call(o)
    after = _launch_info(gpu)
    assert (after[0] - before[0], after[1] - before[1]) == (0, 1), (before, after)
    for _ in range(2):
        o["sse"].fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        got = _host(o)
        for k in want:
            assert np.array_equal(got[k], want[k]), k


def test_two_streams_in_flight_each_equal_their_solo_result(gpu, setup):
    import torch
    s = setup
    S = _shapes(s["R"])["R_plus_3"]
    outputs, call = _device_call(gpu, s, S)
    solo = outputs()
    call(solo)
    torch.cuda.synchronize()
    want = _host(solo)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [outputs(), outputs()]
    torch.cuda.synchronize()
    before = _launch_info(gpu)
    for st, o in zip(streams, outs):
        with torch.cuda.stream(st):
            call(o)
    assert _launch_info(gpu)[0] == before[0] + 2         # both persistent, each on a ticket slot of its own
    torch.cuda.synchronize()
    for o in outs:
        got = _host(o)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
