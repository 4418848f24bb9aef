"""trpl_predictive* on the device against the extended-precision band of tests/predictive_ref.py, at every shape where the
tiling can go wrong: one column, a tile of columns and its neighbours, rows that are not 16-byte aligned (odd strides), one
row, a chunk of rows and its neighbours, three chunks with a ragged last one, both element sizes.  The reference's y comes
from the project's own log10 (fastlog = trpl_log10_clamp) on the same PL plus mag in fp64, so the comparison tests the
reduction, not log10; the envelope must equal the extreme y bit for bit.  Tile width and chunk length are read from the
library (csrc/predictive.hip, trpl_predictive_chunks), not written down here."""
import math
import os
import re

import numpy as np
import pytest

import predictive_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "csrc", "predictive.hip")).read()
TILE = int(re.search(r"constexpr int kTileCols = (\d+);", _SRC).group(1))
NCOLS = [1, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
DTYPES = [np.float32, np.float64]


def _rows(gpu, ncol, elem):
    one, ragged = pr.chunk_rows(gpu._abi.lib().trpl_predictive_chunks, ncol, elem)
    assert one >= 2 and ragged * (ncol + 3) * elem < 600 << 10          # a few hundred KB at most
    return [1, one - 1, one, one + 1, ragged]


def _y(gpu, pl, ncol, mag=None, normalize=False):
    """The model values through the project's own log10: the PL as the likelihood path forms it (divided by column 0 in the
    buffer's dtype under NORMALIZE), fastlog in place in that dtype, + mag in fp64."""
    v = np.array(pl[:, :ncol], order="C")
    if normalize:
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            v = np.ascontiguousarray(v / v[:, :1])
    gpu.fastlog(v)
    y = v.astype(np.float64)
    return y if mag is None else y + np.asarray(mag, dtype=np.float64)[:, None]


def _inputs(gpu, seed, rows, ncol, ld, dtype):
    pl = pr.pl_family(seed, rows, ncol, ld, dtype)
    W = gpu.posterior.weights(pr.ll_family(seed, rows))
    return pl, W, pr.mag_family(seed, rows)


def _check(got, y, W, used, what):
    want = pr.band_ref(y, W, used)
    err = pr.errors(got, want)
    print("predictive %s: error / allowance %s" % (what, {k: "%.3g" % v for k, v in err.items()}))
    assert all(v <= 1.0 for v in err.values()), (what, err)
    if used.any():                              # the envelope is exact: the extreme y of the used rows, bit for bit
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got["lo"], np.fmin.reduce(y[used], axis=0)) and np.array_equal(got["hi"], np.fmax.reduce(y[used], axis=0)), what


def _bits_equal(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in pr.FIELDS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ncol", NCOLS)
def test_band_meets_the_reference_at_every_tile_and_chunk_boundary(gpu, ncol, dtype):
    elem = np.dtype(dtype).itemsize
    seen_zero_weight = 0
    for ld in (ncol, ncol + 3):                 # ncol + 3: odd strides, rows that are only element-aligned
        for rows in _rows(gpu, ncol, elem):
            pl, W, mag = _inputs(gpu, 100 * ncol + rows, rows, ncol, ld, dtype)
            used = pr.used_rows(W)
            seen_zero_weight += int((W == 0.0).sum())
            info = {}
            got = gpu.predictive.band(pl, W, mag=mag, ncol=ncol, info=info)
            assert info["chunks"] == gpu._abi.lib().trpl_predictive_chunks(rows, ncol, elem)
            _check(got, _y(gpu, pl, ncol, mag), W, used, (rows, ncol, ld, dtype.__name__, info["chunks"]))
            assert np.array_equal(got["sw"], np.full(ncol, got["sw"][0]))
    assert seen_zero_weight > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_is_the_likelihood_paths_division(gpu, dtype):
    elem = np.dtype(dtype).itemsize
    for ncol, ld in ((1, 1), (3, 6), (TILE + 1, TILE + 4)):
        for rows in _rows(gpu, ncol, elem)[2:]:
            pl, W, mag = _inputs(gpu, 7 * ncol + rows, rows, ncol, ld, dtype)
            got = gpu.predictive.band(pl, W, mag=mag, ncol=ncol, normalize=True)
            y = _y(gpu, pl, ncol, mag, normalize=True)
            assert np.array_equal(y[:, 0], mag)                    # column 0 of a normalised curve is log10 1
            _check(got, y, W, pr.used_rows(W), ("normalize", rows, ncol, ld, dtype.__name__))
    # without mag: the offset is 0
    pl, W, _ = _inputs(gpu, 5, 40, 9, 12, dtype)
    _check(gpu.predictive.band(pl, W, ncol=9, normalize=True), _y(gpu, pl, 9, None, True), W, pr.used_rows(W), "no mag")


@pytest.mark.parametrize("dtype", DTYPES)
def test_flagged_rows_are_rows_without_weight(gpu, dtype):
    elem = np.dtype(dtype).itemsize
    ncol, ld = TILE + 1, TILE + 4
    rows = _rows(gpu, ncol, elem)[-1]
    pl, W, mag = _inputs(gpu, 31, rows, ncol, ld, dtype)
    used = pr.used_rows(W)
    status = np.zeros(rows, dtype=np.int32)
    status[np.flatnonzero(used)[::3]] = 1 + np.arange(len(np.flatnonzero(used)[::3]))       # 1 + failing step
    status[np.flatnonzero(~used)[:2]] = 5
    assert (status[used] != 0).any() and (status[used] == 0).any()
    got = gpu.predictive.band(pl, W, mag=mag, status=status, ncol=ncol)
    W0 = np.where(status != 0, 0.0, W)
    assert _bits_equal(got, gpu.predictive.band(pl, W0, mag=mag, ncol=ncol))
    _check(got, _y(gpu, pl, ncol, mag), W, pr.used_rows(W, status), ("status", rows, dtype.__name__))
    assert not _bits_equal(got, gpu.predictive.band(pl, W, mag=mag, ncol=ncol))
    # no used row at all: by status, and by weight
    for w, st in ((W, np.ones(rows, dtype=np.int32)), (np.where(used, -W, W), None), (np.full(rows, np.nan), None), (np.zeros(rows), None)):
        none = gpu.predictive.band(pl, w, mag=mag, status=st, ncol=ncol)
        assert not none["sw"].any() and np.isnan(none["mean"]).all() and np.isnan(none["var"]).all()
        assert np.isposinf(none["lo"]).all() and np.isneginf(none["hi"]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_element_makes_only_its_column_nan(gpu, dtype):
    elem = np.dtype(dtype).itemsize
    ncol = TILE + 1
    rows = _rows(gpu, ncol, elem)[-1]
    pl, W, mag = _inputs(gpu, 77, rows, ncol, ncol, dtype)
    pl[pl == 0] = 1.0                           # (an exact zero is -inf in a float32 buffer: columns of their own)
    used = np.flatnonzero(pr.used_rows(W))
    clean = gpu.predictive.band(pl, W, mag=mag, ncol=ncol)
    assert np.isfinite(clean["mean"]).all() and np.isfinite(clean["var"]).all()
    hit = {0: used[0], TILE - 1: used[-1], TILE: used[len(used) // 2]}              # first / last used row, both waves' edges
    unused = np.flatnonzero(~pr.used_rows(W))[0]
    for c, r in hit.items():
        pl[r, c] = np.nan
    pl[unused, 5] = np.nan                      # a NaN in a row without weight is never read
    got = gpu.predictive.band(pl, W, mag=mag, ncol=ncol)
    bad = np.zeros(ncol, dtype=bool)
    bad[list(hit)] = True
    assert np.isnan(got["mean"][bad]).all() and np.isnan(got["var"][bad]).all()
    for k in pr.FIELDS:
        assert np.array_equal(got[k][~bad], clean[k][~bad]), k
    assert np.isfinite(got["lo"]).all() and np.isfinite(got["hi"]).all()            # the envelope skips the NaN
    _check(got, _y(gpu, pl, ncol, mag), W, pr.used_rows(W), ("nan", dtype.__name__))


def _dev_band(gpu, pl, W, mag, status, ncol, splits, flags=0):
    import torch
    dv = gpu.device
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pl_d, W_d, mag_d, st_d = up(pl), up(W), up(mag), up(status)
    state, out = dv.predictive_state(ncol), torch.empty((5, ncol), dtype=torch.float64, device=dev)
    dv.predictive_init_device(state)
    for a, b in splits:
        ws = dv.predictive_workspace(b - a, ncol, pl.itemsize)
        dv.predictive_accumulate_device(pl_d[a:b], W_d[a:b], state, ws, mag=None if mag is None else mag_d[a:b],
                                        status=None if status is None else st_d[a:b], ncol=ncol, flags=flags)
    dv.predictive_finish_device(state, out)
    torch.cuda.synchronize()
    return dict(zip(pr.FIELDS, out.cpu().numpy()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulation_over_several_calls(gpu, dtype):
    elem = np.dtype(dtype).itemsize
    ncol, ld = 2 * TILE + 5, 2 * TILE + 8
    one, rows = pr.chunk_rows(gpu._abi.lib().trpl_predictive_chunks, ncol, elem)
    pl, W, mag = _inputs(gpu, 55, rows, ncol, ld, dtype)
    used = pr.used_rows(W)
    y = _y(gpu, pl, ncol, mag)
    whole = _dev_band(gpu, pl, W, mag, None, ncol, [(0, rows)])
    _check(whole, y, W, used, ("one call", dtype.__name__))
    assert _bits_equal(whole, gpu.predictive.band(pl, W, mag=mag, ncol=ncol))       # the host form: init + accumulate + finish
    for cut in (1, one + 1, rows - 1):
        split = _dev_band(gpu, pl, W, mag, None, ncol, [(0, cut), (cut, rows)])
        _check(split, y, W, used, ("two calls", cut, dtype.__name__))
        assert _bits_equal(split, _dev_band(gpu, pl, W, mag, None, ncol, [(0, cut), (cut, rows)]))     # the same sequence again
    assert _bits_equal(whole, _dev_band(gpu, pl, W, mag, None, ncol, [(0, rows)]))
    # a block whose rows are all flagged in between changes nothing
    st = np.where(np.arange(rows) < rows // 2, 0, 1).astype(np.int32)
    assert _bits_equal(_dev_band(gpu, pl, W, mag, st, ncol, [(0, rows), (rows // 2, rows)]), _dev_band(gpu, pl, W, mag, st, ncol, [(0, rows)]))
    # TRPL_FLAG_PL_F32 on a float64 buffer rounds PL and log10 through float32 like the float32 buffer
    if dtype == np.float64:
        pl32 = pl.astype(np.float32)
        with_flag = _dev_band(gpu, pl32.astype(np.float64), W, mag, None, ncol, [(0, rows)], flags=gpu._abi.FLAG_PL_F32)
        assert _bits_equal(with_flag, _dev_band(gpu, pl32, W, mag, None, ncol, [(0, rows)]))


def test_every_refusal_names_its_argument(gpu):
    import torch
    lib, E = gpu._abi.lib(), gpu._abi.ERR_ARG
    dev = torch.device("cuda", 0)
    rows, ncol = 8, 6
    pl = torch.ones((rows, ncol), dtype=torch.float64, device=dev)
    W = torch.ones(rows, dtype=torch.float64, device=dev)
    state = torch.zeros((5, ncol), dtype=torch.float64, device=dev)
    out = torch.zeros((5, ncol), dtype=torch.float64, device=dev)
    need = lib.trpl_predictive_workspace_bytes(rows, ncol, 8)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=dev)
    before = state.clone()

    def acc(**kw):
        a = dict(pl=pl.data_ptr(), elem=8, rows=rows, ncol=ncol, ld=ncol, W=W.data_ptr(), flags=0, state=state.data_ptr(),
                 ws=ws.data_ptr(), wsb=need)
        a.update(kw)
        return lib.trpl_predictive_accumulate_dev(a["pl"], a["elem"], a["rows"], a["ncol"], a["ld"], None, a["W"], None, a["flags"],
                                                  a["state"], a["ws"], a["wsb"], None)

    for kw, word in ((dict(rows=0), b"rows"), (dict(ncol=0), b"ncol"), (dict(ld=ncol - 1), b"ld"), (dict(elem=2), b"elem_bytes"),
                     (dict(elem=16), b"elem_bytes"), (dict(pl=None), b"plI"), (dict(W=None), b"W is NULL"),
                     (dict(state=None), b"state"), (dict(ws=None), b"workspace"), (dict(wsb=need - 8), b"workspace"),
                     (dict(flags=gpu._abi.FLAG_STRICT), b"flags"), (dict(flags=gpu._abi.FLAG_NORMALIZE | gpu._abi.FLAG_PREDICT), b"flags")):
        assert acc(**kw) == E and word in lib.trpl_last_error(), (kw, lib.trpl_last_error())
    assert lib.trpl_predictive_init_dev(None, ncol, None) == E and b"state" in lib.trpl_last_error()
    assert lib.trpl_predictive_init_dev(state.data_ptr(), 0, None) == E and b"ncol" in lib.trpl_last_error()
    assert lib.trpl_predictive_finish_dev(None, ncol, out.data_ptr(), None) == E and b"state" in lib.trpl_last_error()
    assert lib.trpl_predictive_finish_dev(state.data_ptr(), ncol, None, None) == E and b"out" in lib.trpl_last_error()
    assert lib.trpl_predictive_finish_dev(state.data_ptr(), 0, out.data_ptr(), None) == E and b"ncol" in lib.trpl_last_error()
    host = np.ones((rows, ncol))
    assert lib.trpl_predictive(host.ctypes.data, 8, rows, ncol, ncol, None, np.ones(rows).ctypes.data, None, 0, None, 0, None) == E
    assert b"out" in lib.trpl_last_error()
    torch.cuda.synchronize()
    assert torch.equal(state, before)                                     # a refused call launched nothing
    # TRPL_FLAG_PL_F32 absent with a 4-byte buffer is fine, as in trpl_loglik_from_pl_dev
    pl4 = torch.ones((rows, ncol), dtype=torch.float32, device=dev)
    assert lib.trpl_predictive_init_dev(state.data_ptr(), ncol, None) == 0
    assert acc(pl=pl4.data_ptr(), elem=4) == 0 and acc(pl=pl4.data_ptr(), elem=4, flags=gpu._abi.FLAG_PL_F32) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_values_are_the_ones_the_likelihood_compared(gpu, dtype, normalize):
    """One used row: the mean IS that row's y, and sum (mean - obs)^2 is the sse trpl_loglik_from_pl_dev reports for it."""
    import torch
    dev = torch.device("cuda", 0)
    rows, ncol, ld = 9, TILE + 37, TILE + 40
    # 30 decades: the normalised values stay inside float32's range
    pl = np.ascontiguousarray((10.0 ** np.random.default_rng(3).uniform(-15, 15, (rows, ld))).astype(dtype))
    mag = pr.mag_family(3, rows)
    obs = np.random.default_rng(9).normal(size=ncol) * 5
    k = 4
    W = np.zeros(rows)
    W[k] = 0.37
    flags = gpu._abi.FLAG_NORMALIZE if normalize else 0
    got = gpu.predictive.band(pl, W, mag=mag, ncol=ncol, normalize=normalize)
    y = _y(gpu, pl, ncol, mag, normalize)
    assert np.array_equal(got["mean"], y[k]) and not got["var"].any()
    assert np.array_equal(got["lo"], y[k]) and np.array_equal(got["hi"], y[k]) and np.array_equal(got["sw"], np.full(ncol, 0.37))
    sse = torch.zeros(rows, dtype=torch.float64, device=dev)
    gpu.device.loglik_from_pl_device(torch.from_numpy(pl).to(dev), torch.from_numpy(obs).to(dev), torch.from_numpy(mag).to(dev),
                                     sse=sse, ncol=ncol, flags=flags)
    want = float(sse[k].item())
    mine = math.fsum(((got["mean"] - obs) ** 2).tolist())
    print("sse of the likelihood %.17g, from the band's mean %.17g" % (want, mine))
    assert want > 0 and abs(mine - want) <= 1e-12 * want


def test_posterior_predictive_end_to_end(gpu):
    """Power_scan's three curves at L = 128, T = 64, 24 samples of which 16 carry a weight of exactly 0.0: the band of every
    curve is the reference band over the PL of a plain solve of the 8 weighted samples, and only those 8 are solved."""
    import torch
    w = gpu.workloads
    L, T, S = 128, 64, 24
    Time = T * 0.025
    ini, lens = w.power_scan(L)
    X = w.samples(S)
    rng = np.random.default_rng(4)
    sel = np.sort(rng.choice(S, 8, replace=False))
    W = np.zeros(S)
    W[sel] = rng.random(8) + 0.05
    W /= W.sum()
    res = gpu.predictive.posterior_predictive(X, W, ini, [list(lens), Time, L, T, 1])
    small = gpu.predictive.posterior_predictive(X, W, ini, [list(lens), Time, L, T, 1], block=3)
    assert len(res) == len(small) == 3
    dev = torch.device("cuda", 0)
    mat = torch.from_numpy(np.ascontiguousarray(X[sel, :12])).to(dev)
    for c in range(3):
        pl = torch.empty((8, T + 1), dtype=torch.float64, device=dev)
        st = torch.empty(8, dtype=torch.int32, device=dev)
        gpu.device.solve_pl_device(mat, lens[c], Time, L, T, torch.from_numpy(ini[c].copy()).to(dev), pl, status=st)
        assert not st.cpu().numpy().any()
        y = _y(gpu, pl.cpu().numpy(), T + 1, X[sel, 12])
        for r in (res[c], small[c]):
            assert (r["n_used"], r["n_solved"], r["n_flagged"]) == (8, 8, 0)
            assert np.array_equal(r["times"], np.linspace(0, Time, T + 1)) and r["mean"].shape == (T + 1,)
            _check(r, y, W[sel], np.ones(8, dtype=bool), ("posterior_predictive", c))
        assert np.all(res[c]["lo"] <= res[c]["mean"]) and np.all(res[c]["mean"] <= res[c]["hi"]) and np.all(res[c]["var"] > 0)
    none = gpu.predictive.posterior_predictive(X, np.zeros(S), ini, [list(lens), Time, L, T, 1])
    assert all(r["n_used"] == r["n_solved"] == 0 and not r["sw"].any() and np.isnan(r["mean"]).all() for r in none)
