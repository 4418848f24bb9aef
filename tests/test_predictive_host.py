"""The posterior-predictive band without a device: the reference and its allowances (tests/predictive_ref.py) are ones fp64
itself can meet on every input family the -m gpu tests use; predictive.merge (plain NumPy) combines finished bands; header,
binding and library agree on the seven entry points; the argument checks need no device."""
import numpy as np
import pytest

import abi_header as H
import predictive_ref as pr

SYMBOLS = ("trpl_predictive_state_bytes", "trpl_predictive_workspace_bytes", "trpl_predictive_chunks", "trpl_predictive_init_dev",
           "trpl_predictive_accumulate_dev", "trpl_predictive_finish_dev", "trpl_predictive")

# (rows, ncol, ld): shapes of the size the GPU tests use -- one row, a handful, several chunks' worth; odd strides
SHAPES = [(1, 1, 1), (1, 5, 8), (2, 3, 3), (31, 7, 10), (33, 255, 258), (64, 257, 257), (167, 517, 520)]
FAMILIES = [(np.float64, False), (np.float64, True), (np.float32, False), (np.float32, True)]


def _case(seed, rows, ncol, ld, dtype, normalize):
    pl = pr.pl_family(seed, rows, ncol, ld, dtype)
    W = pr.weights_np(pr.ll_family(seed, rows))
    mag = pr.mag_family(seed, rows)
    return pr.y_numpy(pl, ncol, mag, normalize), W


def _assert_within(err, what):
    assert all(v <= 1.0 for v in err.values()), (what, err)


@pytest.mark.parametrize("dtype,normalize", FAMILIES)
def test_fp64_meets_every_allowance_on_the_gpu_tests_inputs(dtype, normalize):
    seen_nan = seen_fin = False
    for seed, (rows, ncol, ld) in enumerate(SHAPES):
        y, W = _case(seed, rows, ncol, ld, dtype, normalize)
        used = pr.used_rows(W)
        if rows >= 31:                          # the weights are what the family promises: most exactly zero, one NaN
            assert 0.5 < np.mean(W == 0.0) < 0.9 and np.isnan(W).sum() == 1 and used.sum() >= 3
        want = pr.band_ref(y, W, used)
        _assert_within(pr.errors(pr.band_fp64(y, W, used), want), (rows, ncol, dtype, normalize))
        seen_nan |= bool(np.isnan(want["mean"]).any())
        seen_fin |= bool(np.isfinite(want["var"]).any())
    # exact zeros: -inf in a float32 buffer (columns without mean), log10 DBL_MIN in a float64 one (every column finite)
    assert seen_fin and seen_nan == (dtype == np.float32)


def test_reference_edge_cases():
    y = np.array([[1.0, 2.0, np.nan], [3.0, 2.0, 5.0], [100.0, 2.0, 7.0]])
    W = np.array([0.25, 0.75, 0.0])
    r = pr.band_ref(y, W, pr.used_rows(W))
    assert r["mean"][0] == 2.5 and r["var"][0] == 0.75 and (r["lo"][0], r["hi"][0]) == (1.0, 3.0)
    assert r["mean"][1] == 2.0 and r["var"][1] == 0.0                                  # a constant column
    assert np.isnan(r["mean"][2]) and np.isnan(r["var"][2]) and r["lo"][2] == r["hi"][2] == 5.0     # the NaN rule
    assert pr.errors(r, r) == dict.fromkeys(pr.FIELDS, 0.0)
    off = dict(r, var=r["var"] + np.array([0, 1e-300, 0]))                            # allowance 0 demands equality
    assert pr.errors(off, r)["var"] == np.inf
    one = pr.band_ref(y, W, np.array([False, True, False]))
    assert np.array_equal(one["mean"], y[1]) and not one["var"].any()                  # one used row
    none = pr.band_ref(y, W, pr.used_rows(W, status=[1, 2, 0]))
    assert not none["sw"].any() and np.isnan(none["mean"]).all() and np.isposinf(none["lo"]).all() and np.isneginf(none["hi"]).all()
    assert list(pr.used_rows([1.0, 0.0, np.nan, np.inf, -1.0, 1e-300])) == [True, False, False, False, False, True]


def _finished(b):
    return {k: np.asarray(b[k], dtype=np.float64) for k in pr.FIELDS}


@pytest.mark.parametrize("dtype,normalize", FAMILIES)
def test_merge_of_the_halves_is_the_band_of_the_whole(trpl, dtype, normalize):
    for seed, (rows, ncol, ld) in enumerate(SHAPES):
        if rows < 2:
            continue
        y, W = _case(seed, rows, ncol, ld, dtype, normalize)
        used = pr.used_rows(W)
        for cut in sorted({1, rows // 2, rows - 1}):
            a = _finished(pr.band_ref(y[:cut], W[:cut], used[:cut]))
            b = _finished(pr.band_ref(y[cut:], W[cut:], used[cut:]))
            _assert_within(pr.errors(trpl.predictive.merge(a, b), pr.band_ref(y, W, used)), (rows, ncol, dtype, normalize, cut))


def test_merge_with_an_empty_side_is_the_identity(trpl):
    y, W = _case(3, 33, 9, 9, np.float32, False)
    full = _finished(pr.band_ref(y, W, pr.used_rows(W)))
    assert np.isnan(full["mean"]).any() and np.isfinite(full["mean"]).any()
    empty = _finished(pr.band_ref(y, W, np.zeros(33, dtype=bool)))
    for got in (trpl.predictive.merge(full, empty), trpl.predictive.merge(empty, full)):
        for k in pr.FIELDS:
            assert np.array_equal(got[k].view(np.uint64), full[k].view(np.uint64)), k
    both = trpl.predictive.merge(empty, empty)
    assert not both["sw"].any() and np.isnan(both["mean"]).all() and np.isposinf(both["lo"]).all()


def test_header_binding_and_library_agree_on_the_seven_symbols(trpl):
    lib = trpl._abi.lib()
    for name in SYMBOLS:
        assert H.returns(name), name
        assert name in trpl._abi.SIGNATURES and hasattr(lib, name), name
    # the argument counts of the binding are the header's
    for name in SYMBOLS:
        assert len(H.params(name)) == len(trpl._abi.SIGNATURES[name]), name
    assert trpl.posterior_predictive is trpl.predictive.posterior_predictive


def test_the_chunking_rule_is_exported_and_bounds_the_workspace(trpl):
    lib = trpl._abi.lib()
    assert lib.trpl_predictive_state_bytes(80001) == 80001 * 40
    for rows, ncol, elem in ((16384, 80001, 4), (4096, 80001, 8), (1, 1, 4), (100, 8001, 8), (10 ** 6, 3, 4)):
        k = lib.trpl_predictive_chunks(rows, ncol, elem)
        assert 1 <= k <= rows and lib.trpl_predictive_workspace_bytes(rows, ncol, elem) == k * ncol * 40
        assert (k - 1) * -(-rows // k) < rows                                # no empty chunk
    # the production block: enough blocks of 256 columns to fill 256 compute units several times, under 256 MiB
    k = lib.trpl_predictive_chunks(16384, 80001, 4)
    assert k * -(-80001 // 256) >= 4096 and lib.trpl_predictive_workspace_bytes(16384, 80001, 4) < 256 << 20
    for bad in ((0, 5, 4), (5, 0, 4), (5, 5, 2), (-1, 5, 8)):
        assert lib.trpl_predictive_chunks(*bad) == 0 and lib.trpl_predictive_workspace_bytes(*bad) == 0
    one, ragged = pr.chunk_rows(lib.trpl_predictive_chunks, 5, 8)
    assert lib.trpl_predictive_chunks(one, 5, 8) == 1 and lib.trpl_predictive_chunks(one + 1, 5, 8) == 2
    assert lib.trpl_predictive_chunks(ragged, 5, 8) >= 3


def test_refusals_need_no_device(trpl):
    lib, E = trpl._abi.lib(), trpl._abi.ERR_ARG
    pl, W, out = np.ones((4, 6)), np.ones(4), np.zeros((5, 6))
    p, w, o = pl.ctypes.data, W.ctypes.data, out.ctypes.data

    def host(**kw):
        a = dict(pl=p, elem=8, rows=4, ncol=6, ld=6, W=w, flags=0, out=o)
        a.update(kw)
        return lib.trpl_predictive(a["pl"], a["elem"], a["rows"], a["ncol"], a["ld"], None, a["W"], None, a["flags"], a["out"], 0, None)

    for kw, word in ((dict(rows=0), b"rows"), (dict(ncol=0), b"ncol"), (dict(ld=5), b"ld"), (dict(elem=2), b"elem_bytes"),
                     (dict(pl=None), b"plI"), (dict(W=None), b"W is NULL"), (dict(out=None), b"out"),
                     (dict(flags=trpl._abi.FLAG_STRICT), b"flags"), (dict(flags=trpl._abi.FLAG_PL_F32 | 0x100000), b"flags")):
        assert host(**kw) == E and word in lib.trpl_last_error(), (kw, lib.trpl_last_error())
    with pytest.raises(ValueError):
        trpl.predictive.band(pl, W[:3])
    with pytest.raises(trpl.TrplError) as e:
        trpl.predictive.band(pl, W, ncol=7)
    assert e.value.code == E
