"""The stand-alone likelihood kernels (csrc/likelihood.hip) at every launch path, through their _dev entry points on torch
tensors, against the references of tests/likelihood_ref.py (proved on the CPU by tests/test_likelihood_ref_host.py):
  log10_clamp_flat_kernel   every n % V and n < V, the grid-stride loop past the 256 * 32-block cap;
  log10_clamp_rows_kernel   padded rows, the row stride past gridDim.y = 8192, the column stride past 64 blocks, the
                            misaligned base pointer with ld == cols;
  sse_accumulate_kernel     all twelve <T, R, W> instantiations (R = 4 / 8 / 16 at rows <= 4096 / <= 16384 / above), the load
                            ring refilled (n_obs > 512) and not, aliased tail rows, padded and odd leading dimensions, NaN / inf rows;
  pl_loglik_kernel          n_obs around the block size, a padded ld, brackets on the first and last interval, the DBL_MIN clamp,
                            with and without status, every flag combination, the three forms against each other and the reference;
  mag_grid_kernel / mag_profile_kernel   M across the 256 offsets of one launch, C up to TRPL_MAG_MAX_CURVES, bit for bit
                            against the plain host forms.
Gates: log10 float32 within one float32 ulp of the correctly rounded value, at most 0.01 % of the elements different at all;
float64 |got - want| <= 2 eps |want| per element and 4e-16 max|want|; the sums array_equal to the serial loop; the stored-PL
sums within the derived bound of test_gpu_moments.py / test_gpu_weighted.py (depth ceil(n / 256) + 9, + 2 weighted).  Measured
worst figures: printed, and in the record file test_likelihood_instances.json.  Every pointer is valid and every index in range."""
import numpy as np
import pytest

import likelihood_ref as R
from gpu_common import record
from test_gpu_moments import EPS

pytestmark = pytest.mark.gpu

REC = {}
DTYPES = ["float32", "float64"]


def _note(key, **figures):
    REC.setdefault(key, {}).update({k: float(v) for k, v in figures.items()})
    print("%s: %s" % (key, ", ".join("%s %.3g" % kv for kv in figures.items())))
    record("likelihood_instances", REC)


def _up(v):
    import torch
    return torch.from_numpy(np.array(v, order="C")).cuda()          # a copy: the shared inputs are read-only


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ a. log10 clamp
def _check_log(got, x, mn, label):
    """The element-wise gates of the module docstring against log10_clamp_ref; returns the worst error in ulps."""
    want = R.log10_clamp_ref(x, mn)
    assert R.same_classes(got, want), label
    fin = np.isfinite(want)
    g, w = got[fin], want[fin]
    u = R.ulps(g, w)
    if got.dtype == np.float32:
        assert (u <= 1.0).all(), (label, float(u.max()))
        assert np.count_nonzero(g != w) <= R.DIFFER_CAP * g.size, (label, int(np.count_nonzero(g != w)), g.size)
    else:
        d = np.abs(g - w)
        assert (d <= 2 * EPS * np.abs(w)).all(), (label, float(u.max()))
        assert (d <= 4e-16 * np.abs(w).max(initial=0.0)).all(), label
    return float(u.max(initial=0.0))


def _clamp_dev(gpu, dev, rows, cols, ld, mn):
    a = gpu._abi
    a.check(a.lib().trpl_log10_clamp_dev(dev.data_ptr(), dev.element_size(), rows, cols, ld, mn, _stream()))
    _sync()


@pytest.mark.parametrize("dtype", DTYPES)
def test_log10_flat_kernel_at_every_tail(gpu, dtype):
    """Contiguous and aligned: 1 x n for n = 1 .. 9 covers every n % V (V = 4 / 2) and n < V (the scalar tail alone); 3 x 171.
    The elements after the buffer keep the sentinel."""
    worst = 0.0
    for mn in R.MINS[dtype]:
        for rows, cols in [(1, n) for n in range(1, 10)] + [(3, 171)]:
            n = rows * cols
            buf = np.full(n + 8, R.SENTINEL, dtype=dtype)
            buf[:n] = R.clamp_values((n,), dtype, mn, seed=cols).ravel()
            dev = _up(buf)
            assert dev.data_ptr() % 16 == 0
            _clamp_dev(gpu, dev, rows, cols, cols, mn)
            got = dev.cpu().numpy()
            assert (got[n:] == R.SENTINEL).all()
            worst = max(worst, _check_log(got[:n], buf[:n], mn, (mn, rows, cols)))
    _note("log10 flat tails %s" % dtype, worst_ulp=worst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_log10_flat_kernel_past_the_block_cap(gpu, oracle, dtype):
    """256 * 8192 * V + V + 1 elements: 8192 blocks is the cap, so one vector is reached by the grid-stride loop's second trip,
    and one element by the scalar tail.  The longdouble reference on every 64th element and on the last 2 V + 1; the whole buffer
    against the oracle's fastlog at the gates the suite has for it (4e-16 max|want|; float32: 2^-23 relative)."""
    V = 16 // np.dtype(dtype).itemsize
    n = 256 * 8192 * V + V + 1
    worst = 0.0
    for k, mn in enumerate(R.MINS[dtype]):
        x = R.clamp_values((1, n), dtype, mn, seed=40 + k)
        dev = _up(x)
        assert dev.data_ptr() % 16 == 0
        _clamp_dev(gpu, dev, 1, n, n, mn)
        got = dev.cpu().numpy()
        idx = np.unique(np.concatenate([np.arange(0, n, 64), np.arange(n - (2 * V + 1), n)]))
        worst = max(worst, _check_log(got[0, idx], x[0, idx], mn, ("cap", mn)))
        want = x.copy()
        oracle.fastlog(want, mn)
        assert R.same_classes(got, want), mn
        fin = np.isfinite(want)
        d = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
        if dtype == "float32":
            assert (d <= 2.0 ** -23 * np.abs(want[fin])).all(), mn
        else:
            assert d.max() <= 4e-16 * np.abs(want[fin]).max(), mn
    _note("log10 flat cap %s" % dtype, worst_ulp=worst, elements=n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_log10_rows_kernel_padded(gpu, dtype):
    """ld > cols: 5 x 7 in 10; 8193 x 5 in 8 (the row loop's second trip: gridDim.y is capped at 8192); 2 x 16390 in 16393 (the
    column loop's second trip: 64 blocks of 256).  The padding comes back as the same bits."""
    worst = 0.0
    for mn in R.MINS[dtype]:
        for k, (rows, cols, ld) in enumerate([(5, 7, 10), (8193, 5, 8), (2, 16390, 16393)]):
            buf = np.full((rows, ld), R.SENTINEL, dtype=dtype)
            buf[:, :cols] = R.clamp_values((rows, cols), dtype, mn, seed=50 + k)
            dev = _up(buf)
            _clamp_dev(gpu, dev, rows, cols, ld, mn)
            got = dev.cpu().numpy()
            assert np.array_equal(np.ascontiguousarray(got[:, cols:]).view(np.uint8), np.ascontiguousarray(buf[:, cols:]).view(np.uint8)), (mn, rows, cols)
            worst = max(worst, _check_log(got[:, :cols], buf[:, :cols], mn, (mn, rows, cols, ld)))
    _note("log10 rows padded %s" % dtype, worst_ulp=worst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_log10_rows_kernel_on_a_misaligned_contiguous_view(gpu, dtype):
    """ld == cols but the base pointer is one element into an allocation: not 16-byte aligned, so the vector kernel must not
    run; the element before the view and the ones after it keep the sentinel."""
    rows, cols = 4, 33
    n = rows * cols
    worst = 0.0
    for k, mn in enumerate(R.MINS[dtype]):
        buf = np.full(1 + n + 7, R.SENTINEL, dtype=dtype)
        buf[1:1 + n] = R.clamp_values((n,), dtype, mn, seed=60 + k)
        dev = _up(buf)
        view = dev[1:1 + n]
        assert view.data_ptr() % 16 != 0
        a = gpu._abi
        a.check(a.lib().trpl_log10_clamp_dev(view.data_ptr(), view.element_size(), rows, cols, cols, mn, _stream()))
        _sync()
        got = dev.cpu().numpy()
        assert got[0] == R.SENTINEL and (got[1 + n:] == R.SENTINEL).all()
        worst = max(worst, _check_log(got[1:1 + n], buf[1:1 + n], mn, ("misaligned", mn)))
    _note("log10 rows misaligned %s" % dtype, worst_ulp=worst)


# ------------------------------------------------------------------------------------------------ b. squared-error accumulation
SSE_CASES = {                                      # R -> (rows, n_obs); launch_sse_t: R = 4 / 8 / 16 at rows <= 4096 / <= 16384 / above
    4: [(rows, n) for rows in (1, 5) for n in (1, 63, 64, 65, 511, 512, 513, 577, 1100)] + [(4096, 70)],
    8: [(rows, n) for rows in (4097, 16384) for n in (70, 577)],     # 4097: the last block has one live row, seven aliased
    16: [(16385, 70), (16385, 577)],
}
SSE_SPECIAL = {4: (5, 577), 8: (4097, 577), 16: (16385, 577)}       # the case of each R that holds a NaN row and a +inf row


@pytest.mark.parametrize("R_", [4, 8, 16], ids=["R4", "R8", "R16"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sse_accumulate_equals_the_serial_loop_at_every_instantiation(gpu, oracle, dtype, weighted, R_):
    """sse_accumulate_kernel<T, R, W>: array_equal to sse_ref (and, unweighted, to the oracle's probs.prob) for every case of
    the R, ld = n_obs + 3 in every other case (float32 rows at an odd ld are not 8-byte aligned), P from non-zero values.  In
    the special case the NaN row comes out NaN, the +inf row -inf (weighted: NaN, its column's weight is 0), and every other
    row -- the same block's included -- is bit-exact."""
    a, lib = gpu._abi, gpu._abi.lib()
    name = "trpl_sse_accumulate_w_dev" if weighted else "trpl_sse_accumulate_dev"
    for k, (rows, n_obs) in enumerate(SSE_CASES[R_]):
        ld = n_obs + 3 if k % 2 == 0 else n_obs
        special = (rows, n_obs) == SSE_SPECIAL[R_]
        c = R.sse_inputs(rows, n_obs, ld, special)
        pl = c["pl"].astype(dtype)
        wts = c["wts"] if weighted else None
        want = R.sse_ref(c["P0"], pl[:, :n_obs], c["values"], c["mag"], wts)
        dP, dpl, dv, dm = _up(c["P0"]), _up(pl), _up(c["values"]), _up(c["mag"])
        dw = [_up(wts)] if weighted else []
        a.check(getattr(lib, name)(dP.data_ptr(), dpl.data_ptr(), dpl.element_size(), rows, n_obs, ld, dv.data_ptr(),
                                   *[w.data_ptr() for w in dw], dm.data_ptr(), _stream()))
        _sync()
        got = dP.cpu().numpy()
        label = "sse_accumulate_kernel<%s, %d, %s> rows=%d n_obs=%d ld=%d" % (dtype, R_, str(weighted).lower(), rows, n_obs, ld)
        print(label + (" (NaN and inf rows)" if special else ""))
        assert np.array_equal(got, want, equal_nan=True), label
        assert np.array_equal(dpl.cpu().numpy().view(np.uint8), pl.view(np.uint8)), label            # the input is only read
        if special:
            bad = list(c["bad"])
            assert np.isnan(got[bad[0]]) and (np.isnan(got[bad[1]]) if weighted else got[bad[1]] == -np.inf), label
            assert np.isfinite(np.delete(got, bad)).all(), label
        else:
            assert np.isfinite(got).all(), label
        if not weighted:
            Po = c["P0"].copy()
            oracle.prob(Po, np.ascontiguousarray(pl[:, :n_obs]), c["values"], c["mag"])
            assert np.array_equal(got, Po, equal_nan=True), label
    REC.setdefault("sse instantiations launched", []).append("<%s, %d, %s>" % (dtype, R_, str(weighted).lower()))
    record("likelihood_instances", REC)


# ------------------------------------------------------------------------------------------------ c. likelihood of stored PL rows
def _from_pl(gpu, form, pl, ncol, c, flags, status, wts):
    """One call of trpl_loglik[_moments | _weighted]_from_pl_dev; returns P (from 3.0), sse, esum (None for the plain form)."""
    import torch
    a, lib = gpu._abi, gpu._abi.lib()
    rows, ld = pl.shape
    n = len(c["obs"])
    P = torch.full((rows,), 3.0, dtype=torch.float64, device="cuda")
    sse = torch.zeros(rows, dtype=torch.float64, device="cuda")
    es = None if form == "plain" else torch.zeros(rows, dtype=torch.float64, device="cuda")
    br = [None] * 3 if c["brackets"] is None else [_up(v) for v in c["brackets"]]
    obs, mag, st = _up(c["obs"]), _up(c["mag"]), None if status is None else _up(status)
    head = [pl.data_ptr(), pl.element_size(), rows, ncol, ld, obs.data_ptr()]
    tail = [_p(br[0]), _p(br[1]), _p(br[2]), n, mag.data_ptr(), _p(st), P.data_ptr(), sse.data_ptr()]
    if form == "plain":
        a.check(lib.trpl_loglik_from_pl_dev(*head, *tail, flags, _stream()))
    elif form == "moments":
        a.check(lib.trpl_loglik_moments_from_pl_dev(*head, *tail, es.data_ptr(), flags, _stream()))
    else:
        w = _up(wts)
        a.check(lib.trpl_loglik_weighted_from_pl_dev(*head, w.data_ptr(), *tail, es.data_ptr(), flags, _stream()))
    _sync()
    return P.cpu().numpy(), sse.cpu().numpy(), None if es is None else es.cpu().numpy()


def _sum_ratios(sse, es, ref, depth, w2, w1, label):
    """The derived bound of test_moments_from_stored_pl / test_weighted_from_stored_pl per row: depth eps sum (w) e^2 on sse,
    depth eps sum (w) |e| on esum, and where the logarithm is the device's float64 one (w2, w1 not None) its allowance with
    the row's own max|lg|: 2 sqrt(w2 sse) eps max|lg| on sse (w2 = wsum; n for unit weights), w1 eps max|lg| on esum (w1 = 2 n
    for unit weights, wsum for the weighted form).  Rows whose reference is not finite are compared as classes.  Returns the
    worst error / bound of sse and of esum."""
    want2, want1 = np.asarray(ref["sse"], dtype=np.float64), np.asarray(ref["esum"], dtype=np.float64)
    fin = np.isfinite(want2) & np.isfinite(want1)
    assert np.array_equal(np.isposinf(sse), np.isposinf(want2)) and not np.isnan(sse).any(), label
    if es is not None:
        assert R.same_classes(es[~fin], want1[~fin]), label
    if not fin.any():
        return 0.0, 0.0
    lgmax = np.abs(ref["lg"]).max(axis=1)[fin]
    b2 = depth * EPS * want2[fin]
    b1 = depth * EPS * np.asarray(ref["abs"], dtype=np.float64)[fin]
    if w2 is not None:
        b2 = b2 + 2 * np.sqrt(w2 * want2[fin]) * EPS * lgmax
        b1 = b1 + w1 * EPS * lgmax
    d2 = np.abs((sse[fin].astype(R.LD) - ref["sse"][fin]).astype(np.float64))
    d1 = np.zeros_like(d2) if es is None else np.abs((es[fin].astype(R.LD) - ref["esum"][fin]).astype(np.float64))
    ratio = lambda d, b: float((d[b > 0] / b[b > 0]).max(initial=0.0))           # a bound of 0 (every weight 0): equality
    assert (d2 <= b2).all() and (d1 <= b1).all(), (label, ratio(d2, b2), ratio(d1, b1))
    return ratio(d2, b2), ratio(d1, b1)


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_loglik_from_pl_forms_on_synthetic_rows(gpu, dtype, offgrid):
    """pl_loglik_kernel<T, MOM, WT> on lognormal rows in a leading dimension of ncol + 3: rows 1 and 3, n_obs 1, 255, 256, 257
    (the block size and its neighbours) and 1030 (five trips of the thread loop), every combination of TRPL_FLAG_NORMALIZE and
    TRPL_FLAG_PL_F32.  status NULL: plain == moments == unit-weight weighted bit for bit, each within the derived bound of
    from_pl_ref, the weighted form with real weights too; the row with the clamped 0 is finite in float64 and scores
    sse = +inf under the float32 staging.  With a status that flags the last row: sse = +inf, esum = NaN, P = -inf there, the
    other rows keep their bits."""
    worst = dict(sse=0.0, esum=0.0, wsse=0.0, wesum=0.0)
    for rows in (1, 3):
        for n_obs in (1, 255, 256, 257, 1030):
            c = R.pl_case(rows, n_obs, offgrid)
            ncol = c["ncol"]
            pl = _up(c["pl"].astype(dtype))
            depth = -(-n_obs // 256) + 9
            for flags in (0, R.FLAG_NORMALIZE, R.FLAG_PL_F32, R.FLAG_NORMALIZE | R.FLAG_PL_F32):
                label = (dtype, offgrid, rows, n_obs, flags)
                host = c["pl"].astype(dtype)[:, :ncol]
                f64_log = dtype == "float64" and not flags & R.FLAG_PL_F32
                ref = R.from_pl_ref(host, c["obs"], c["mag"], flags, c["brackets"])
                refw = R.from_pl_ref(host, c["obs"], c["mag"], flags, c["brackets"], c["wts"])
                plain = _from_pl(gpu, "plain", pl, ncol, c, flags, None, None)
                mom = _from_pl(gpu, "moments", pl, ncol, c, flags, None, None)
                one = _from_pl(gpu, "weighted", pl, ncol, c, flags, None, np.ones(n_obs))
                wtd = _from_pl(gpu, "weighted", pl, ncol, c, flags, None, c["wts"])
                assert np.array_equal(plain[0], mom[0]) and np.array_equal(plain[1], mom[1]), label
                for x, y in zip(mom, one):
                    assert np.array_equal(x, y, equal_nan=True), label
                for P, sse, _ in (mom, wtd):
                    assert np.array_equal(P, 3.0 - sse), label
                if c["zero_col"] is not None:
                    assert np.isfinite(mom[1][1]) == f64_log and np.isfinite(mom[1][[0, 2]]).all(), label
                wsum = float(np.sum(c["wts"]))
                r = _sum_ratios(mom[1], mom[2], ref, depth, *((float(n_obs), 2.0 * n_obs) if f64_log else (None, None)), label)
                rw = _sum_ratios(wtd[1], wtd[2], refw, depth + 2, *((wsum, wsum) if f64_log else (None, None)), label)
                worst.update(sse=max(worst["sse"], r[0]), esum=max(worst["esum"], r[1]), wsse=max(worst["wsse"], rw[0]),
                             wesum=max(worst["wesum"], rw[1]))
                status = np.zeros(rows, dtype=np.int32)
                status[rows - 1] = 7
                for form, clean in (("plain", plain), ("moments", mom), ("weighted", wtd)):
                    got = _from_pl(gpu, form, pl, ncol, c, flags, status, c["wts"])
                    assert got[0][-1] == -np.inf and got[1][-1] == np.inf and (got[2] is None or np.isnan(got[2][-1])), label
                    for x, y in zip(got, clean):
                        assert x is None or np.array_equal(x[:-1], y[:-1], equal_nan=True), (label, form)
    _note("from_pl %s %s" % (dtype, "offgrid" if offgrid else "ongrid"), **{k + "_err_over_bound": v for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ d. mag grid and profile
MAG_M = (1, 32, 33, 256, 257, 300)                 # kMagAcc = 32 offsets per register pass, kMagChunk = 256 per launch


@pytest.mark.parametrize("weighted", [False, True], ids=["n_obs", "wsum"])
@pytest.mark.parametrize("C", [1, 3, 64])
@pytest.mark.parametrize("S", [1, 1000])
def test_mag_grid_and_profile_equal_the_host_forms_bit_for_bit(gpu, S, C, weighted):
    """trpl_mag_grid[_w]_dev at M = 1 .. 300 (the second launch starts at offset 256: P + 256 S) and trpl_mag_profile[_w]_dev
    with both per_curve settings, against the plain host forms on the same moments: flagged entries, a sum that cancels below
    zero, a curve of weight 0 (wsum; alone when C = 1), P from non-zero values."""
    a, lib = gpu._abi, gpu._abi.lib()
    sfx = "_w" if weighted else ""
    cases = [R.mag_moments(S, C, weighted)]
    if weighted and C == 1:
        cases.append(dict(cases[0], n=np.zeros(1)))
    for m in cases:
        dsse, desum = _up(m["sse"]), _up(m["esum"])
        for M in MAG_M:
            offsets = R.mag_offsets(M)
            P = np.tile(m["P0"], (M, 1))
            dP = _up(P)
            a.check(getattr(lib, "trpl_mag_grid" + sfx)(a.ptr(m["sse"]), a.ptr(m["esum"]), a.ptr(m["n"]), S, C, a.ptr(offsets), M, a.ptr(P)))
            a.check(getattr(lib, "trpl_mag_grid%s_dev" % sfx)(dsse.data_ptr(), desum.data_ptr(), a.ptr(m["n"]), S, C, a.ptr(offsets), M,
                                                              dP.data_ptr(), _stream()))
            _sync()
            assert np.array_equal(dP.cpu().numpy(), P), (S, C, M, weighted)
            assert not np.isnan(P).any() and np.isfinite(P[:, 0]).all() and (S == 1 or (P[:, 3] == -np.inf).all())
            if m["n"][0] > 0:                                                    # the cancelling entry: curve 0 adds exactly 0 at offsets[0]
                nf = np.asarray(m["n"], dtype=np.float64)
                rest = 0.0
                for c in range(1, C):
                    rest = rest + max(R.mag_poly(m["sse"][c, 0], m["esum"][c, 0], nf[c], R.CANCEL_D), 0.0)
                assert P[0, 0] == m["P0"][0] - rest
        for per_curve in (False, True):
            best, Pp = np.full((C, S) if per_curve else S, 5.0), m["P0"].copy()
            dbest, dPp = _up(best), _up(Pp)
            fl = a.MAG_PER_CURVE if per_curve else 0
            a.check(getattr(lib, "trpl_mag_profile" + sfx)(a.ptr(m["sse"]), a.ptr(m["esum"]), a.ptr(m["n"]), S, C, fl, a.ptr(best), a.ptr(Pp)))
            a.check(getattr(lib, "trpl_mag_profile%s_dev" % sfx)(dsse.data_ptr(), desum.data_ptr(), a.ptr(m["n"]), S, C, fl, dbest.data_ptr(),
                                                                 dPp.data_ptr(), _stream()))
            _sync()
            assert np.array_equal(dbest.cpu().numpy(), best, equal_nan=True) and np.array_equal(dPp.cpu().numpy(), Pp), (S, C, per_curve)
