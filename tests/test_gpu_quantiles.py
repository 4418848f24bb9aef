"""trpl_weighted_quantiles* and trpl_predictive_gather_dev on the device against the extended-precision reference of
tests/quantiles_ref.py (equality with ==, either neighbour where the reference calls the pair ambiguous; the cap on ambiguous
pairs is asserted first and proven on the CPU by tests/test_quantiles_host.py).  Column lengths around a wave, the workgroup's
stride and the staged / streamed threshold are read from the library; the gather is tied to predictive.band bit for bit."""
import numpy as np
import pytest

import predictive_ref as pr
import quantiles_ref as qr

pytestmark = pytest.mark.gpu


def _consts(gpu):
    return gpu._abi.Q_BLOCK, int(gpu._abi.lib().trpl_quantiles_stage_rows())


def _select(gpu, Y, W, q, rule, flags=0):
    """The device form on tensors: Y (ncols, ldy) with the first W.size entries of every row valid."""
    import torch
    dev = torch.device("cuda", 0)
    Yd, Wd = torch.from_numpy(np.ascontiguousarray(Y)).to(dev), torch.from_numpy(np.ascontiguousarray(W)).to(dev)
    out = torch.full((len(q), Y.shape[0]), -7.0, dtype=torch.float64, device=dev)
    gpu.device.weighted_quantiles_device(Yd, Wd, q, out, rule=rule, n=W.size, flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _host(gpu, Y, W, q, rule, flags=0):
    lib, A = gpu._abi.lib(), gpu._abi
    q, rule = gpu.device.quantile_requests(q, rule)
    out = np.full((q.size, Y.shape[0]), -7.0)
    Y, W = np.ascontiguousarray(Y), np.ascontiguousarray(W)
    A.check(lib.trpl_weighted_quantiles(A.ptr(Y), Y.shape[0], W.size, Y.shape[1], A.ptr(W), A.ptr(q), A.ptr(rule), q.size, flags,
                                        A.ptr(out), 0, None))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_case(gpu, args, stage):
    Y, W, q, rule, ref = qr.case(*args)
    got = _select(gpu, Y, W, q, rule)
    bad = qr.mismatches(got, ref)
    print("quantiles %s: %d of %d pairs ambiguous, %d mismatches" % (args, ref["ambiguous"].sum(), ref["ambiguous"].size, len(bad)))
    assert not bad, (args, bad[:5])
    # the streamed form gives the staged form's bits (above the threshold both calls are the streamed form: repeatability)
    assert np.array_equal(_bits(got), _bits(_select(gpu, Y, W, q, rule, flags=gpu._abi.Q_FORCE_STREAM))), args
    assert np.array_equal(_bits(got), _bits(_select(gpu, Y, W, q, rule))), args
    return got


@pytest.mark.parametrize("which", range(12))
def test_every_column_length_where_the_kernels_can_go_wrong(gpu, which):
    block, stage = _consts(gpu)
    n = qr.shape_list(block, stage)[which]
    for args in qr.shape_cases(n):
        _check_case(gpu, args, stage)


@pytest.mark.parametrize("wkind", qr.WEIGHTS)
def test_every_weight_family_with_every_key_family(gpu, wkind):
    block, stage = _consts(gpu)
    FA, LB = qr.FIRST_ABOVE, qr.LAST_BELOW
    for args in qr.family_cases(block):
        if args[4] != wkind:
            continue
        Y, W, q, rule, ref = qr.case(*args)
        got = _check_case(gpu, args, stage)
        lb = np.array(rule) == LB
        kk = args[5]
        if kk == "constant":                      # LAST_BELOW has no key below the constant, FIRST_ABOVE is the constant
            assert np.isnan(got[lb]).all() and np.array_equal(got[~lb], np.tile(np.arange(3) - 0.5, (int((~lb).sum()), 1)))
        elif kk == "nan_used":                    # the whole column, and only that column
            assert np.isnan(got[:, 0]).all() and np.isnan(got[:, -1]).all() and not np.isnan(got[~lb, 1]).any()
        elif kk == "nan_unused":                  # never looked at
            assert not np.isnan(got[~lb]).any()
        elif kk == "inf":
            assert (wkind == "one_row" or np.isinf(got).any()) and not np.isnan(got[~lb]).any()
        elif kk == "zeros":
            assert set(np.unique(got[~np.isnan(got)])) <= {-1.0, 0.0, 1.0}
    # no used row at all: NaN everywhere
    Y, W, q, rule, _ = qr.case(2 * block + 1, 3, 3, 8, wkind, "random")
    for w in (np.zeros(W.size), np.full(W.size, np.nan), -np.abs(np.where(np.isfinite(W), W, 1.0)), np.full(W.size, np.inf)):
        assert np.isnan(_select(gpu, Y, w, q, rule)).all()


def test_the_host_form_equals_the_device_form(gpu):
    block, stage = _consts(gpu)
    for args in ((block + 1, 3, 3, 8, "uniform", "random"), (stage + 1, 3, 0, 3, "decades", "ties"), (65, 257, 3, 1, "sparse", "random")):
        Y, W, q, rule, ref = qr.case(*args)
        got = _host(gpu, Y, W, q, rule)
        assert np.array_equal(_bits(got), _bits(_select(gpu, Y, W, q, rule))), args
        assert np.array_equal(_bits(got), _bits(_host(gpu, Y, W, q, rule, flags=gpu._abi.Q_FORCE_STREAM))), args
        assert not qr.mismatches(got, ref)


def test_posterior_quantiles_and_credible_intervals_on_the_streamed_form(gpu):
    S, D = 2 ** 17 + 1, 5
    assert S > _consts(gpu)[1]
    rng = np.random.default_rng(11)
    V = rng.normal(size=(D, S)) * np.arange(1, D + 1)[:, None]          # tie-free columns
    V[1] = np.exp(V[1] / 2)
    LL = -0.5 * (V[0] ** 2) * 3 + rng.normal(size=S)
    P = gpu.posterior.weights(LL)
    assert abs(P.sum() - 1) < 1e-9
    q, rule = [0.025, 0.16, 0.5, 0.84, 0.975], None
    got = gpu.posterior.quantiles(V, P, q)
    ref = qr.reference(V, P, q, qr.default_rules(q))
    bad = qr.mismatches(got, ref)
    print("posterior.quantiles S = %d: %d ambiguous, %d mismatches" % (S, ref["ambiguous"].sum(), len(bad)))
    assert not bad, bad[:5]
    ci = gpu.posterior.credible_intervals({"p%d" % d: V[d] for d in range(D)}, P)
    ref2 = qr.reference(V, P, [0.025, 0.975], [qr.LAST_BELOW, qr.FIRST_ABOVE])
    assert qr.within_cap(ref2)
    assert list(ci) == ["p%d" % d for d in range(D)]
    for d in range(D):
        assert ci["p%d" % d] == (got[0, d], got[4, d])                  # one call for all columns, the same selection
        old = gpu.posterior.credible_interval(V[d], P)                  # the existing host argsort: fp64 cumsum, sum P = 1
        for k in (0, 1):
            allowed = (ref2["below"][k, d], ref2["above"][k, d]) if ref2["ambiguous"][k, d] else (ref2["want"][k, d],)
            assert ci["p%d" % d][k] in allowed and old[k] in allowed, (d, k, ci["p%d" % d], old, allowed)
    # a one-dimensional V is one column; a scalar q one request
    one = gpu.posterior.quantiles(V[2], P, 0.5)
    assert one.shape == (1, 1) and one[0, 0] == got[2, 2]


# ------------------------------------------------------------------------------------------------ the gather
def _gather(gpu, pl, W, mag, status, ncol, blocks, flags=0, pad=2):
    """The store (ncol, rows + pad) and its weights after gathering `blocks` = [(a, b), ...] row ranges of pl at row0 = a."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows = pl.shape[0]
    pl_d, W_d, mag_d, st_d = up(pl), up(W), up(mag), up(status)
    Y = torch.full((ncol, rows + pad), -7.0, dtype=torch.float64, device=dev)
    Wq = torch.full((rows + pad,), -7.0, dtype=torch.float64, device=dev)
    for a, b in blocks:
        gpu.device.predictive_gather_device(pl_d[a:b], W_d[a:b], Y, Wq, row0=a, mag=None if mag is None else mag_d[a:b],
                                            status=None if status is None else st_d[a:b], ncol=ncol, flags=flags)
    torch.cuda.synchronize()
    return Y.cpu().numpy(), Wq.cpu().numpy()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_store_holds_the_bands_values_bit_for_bit(gpu, dtype, normalize):
    """Column j of the store is lo (= hi) of predictive.band over the single row j: the gather forms y with the device function
    of the existing band, not with a host log10.  Odd strides, a tile of columns and its neighbours, two consecutive blocks
    of which the second starts at an odd row0, a tile of rows and its neighbours."""
    flags = gpu._abi.FLAG_NORMALIZE if normalize else 0
    for seed, (rows, cut, ncol, ld) in enumerate(((65, 64, 63, 67), (70, 63, 64, 257), (66, 65, 65, 1025), (9, 4, 129, 131))):
        pl = pr.pl_family(seed, rows, ncol, ld, dtype)
        W = np.random.default_rng(seed).random(rows) + 0.1
        W[::5] = [0.0, np.nan, -1.0, np.inf][seed % 4]
        mag = pr.mag_family(seed, rows)
        status = np.zeros(rows, dtype=np.int32)
        status[3::7] = 1 + np.arange(len(status[3::7]))
        used = pr.used_rows(W, status)
        assert used.any() and (~used).sum() > len(W[::5])
        Y, Wq = _gather(gpu, pl, W, mag, status, ncol, [(0, cut), (cut, rows)], flags=flags)
        assert np.array_equal(_bits(Wq[:rows]), _bits(np.where(used, W, 0.0)))        # zero exactly for the unused rows
        assert (Wq[rows:] == -7.0).all() and (Y[:, rows:] == -7.0).all()               # nothing past the blocks is written
        one = np.ones(1)
        for j in range(rows):
            b = gpu.predictive.band(pl[j:j + 1], one, mag=mag[j:j + 1], ncol=ncol, normalize=normalize)
            assert np.array_equal(_bits(b["lo"]), _bits(b["hi"]))
            assert np.array_equal(_bits(Y[:, j]), _bits(b["lo"])), (rows, ncol, ld, j)
        # one call over all rows writes the same store; no mag is an offset of 0
        Y1, Wq1 = _gather(gpu, pl, W, mag, status, ncol, [(0, rows)], flags=flags)
        assert np.array_equal(_bits(Y1), _bits(Y)) and np.array_equal(_bits(Wq1), _bits(Wq))
        Y0, _ = _gather(gpu, pl, W, None, None, ncol, [(0, rows)], flags=flags)
        b = gpu.predictive.band(pl[:1], one, ncol=ncol, normalize=normalize)
        assert np.array_equal(_bits(Y0[:, 0]), _bits(b["lo"]))
    if dtype == np.float64:       # TRPL_FLAG_PL_F32 on a float64 buffer rounds PL and log10 through float32 like a float32 buffer
        pl32 = pr.pl_family(9, 66, 65, 67, np.float32)
        W = np.ones(66)
        a, _ = _gather(gpu, pl32.astype(np.float64), W, None, None, 65, [(0, 66)], flags=flags | gpu._abi.FLAG_PL_F32)
        b, _ = _gather(gpu, pl32, W, None, None, 65, [(0, 66)], flags=flags)
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_band_quantiles_against_the_reference_and_the_envelope(gpu, dtype):
    rows, ncol, ld = 300, 70, 73
    rng = np.random.default_rng(5)
    pl = np.ascontiguousarray((10.0 ** rng.uniform(-15, 15, (rows, ld))).astype(dtype))
    pl[:, ncol:] = np.nan
    W = rng.random(rows) + 1e-3                                         # 300 rows of comparable weight: 2.5 % is several rows
    W[::9] = 0.0
    mag = pr.mag_family(5, rows)
    status = np.zeros(rows, dtype=np.int32)
    status[4::50] = 3
    q = (0.025, 0.5, 0.975)
    for normalize in (False, True):
        store = {}
        got = gpu.predictive.band_quantiles(pl, W, q, mag=mag, status=status, normalize=normalize, ncol=ncol, keep_store=store)
        assert got.shape == (3, ncol) and store["Y"].shape == (ncol, rows)
        assert np.array_equal(store["Wq"] > 0, pr.used_rows(W, status))
        ref = qr.reference(store["Y"], store["Wq"], q, qr.default_rules(q))
        assert not qr.mismatches(got, ref)
        env = gpu.predictive.band(pl, W, mag=mag, status=status, ncol=ncol, normalize=normalize)
        assert np.all(env["lo"] <= got[0]) and np.all(got[0] <= got[1]) and np.all(got[1] <= got[2]) and np.all(got[2] <= env["hi"])
        streamed = gpu.predictive.band_quantiles(pl, W, q, mag=mag, status=status, normalize=normalize, ncol=ncol,
                                                 flags=gpu._abi.Q_FORCE_STREAM)
        assert np.array_equal(_bits(got), _bits(streamed))


def test_posterior_predictive_with_quantiles_end_to_end(gpu):
    """Power_scan's three curves at L = 128, T = 64 (the grid of the existing end-to-end test), 24 samples of which 8 carry
    weight, solved in two blocks of 5 and 3; one of the 8 has a NaN lifetime and is flagged.  The quantiles are the reference's
    on the y of a plain solve of the other 7; without `quantiles` nothing changes."""
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
    X[sel[6], 9] = np.nan                                               # tau_n: the solve flags this system
    sim = [list(lens), Time, L, T, 1]
    q = (0.1, 0.5, 0.9)
    plain = gpu.predictive.posterior_predictive(X, W, ini, sim, block=5)
    same = gpu.predictive.posterior_predictive(X, W, ini, sim, block=5, quantiles=None)
    res = gpu.predictive.posterior_predictive(X, W, ini, sim, block=5, quantiles=q)
    whole = gpu.predictive.posterior_predictive(X, W, ini, sim, quantiles=q)
    dev = torch.device("cuda", 0)
    good = np.delete(sel, 6)
    mat = torch.from_numpy(np.ascontiguousarray(X[good, :12])).to(dev)
    for c in range(3):
        assert set(plain[c]) == set(same[c]) and set(res[c]) == set(plain[c]) | {"q", "quantile"}
        for k in plain[c]:
            a, b, r = (np.asarray(d[c][k], dtype=np.float64) for d in (plain, same, res))
            assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(r)), k
        assert (res[c]["n_used"], res[c]["n_solved"], res[c]["n_flagged"]) == (8, 8, 1)
        assert res[c]["q"] == q and res[c]["quantile"].shape == (3, T + 1)
        pl = torch.empty((7, T + 1), dtype=torch.float64, device=dev)
        st = torch.empty(7, dtype=torch.int32, device=dev)
        gpu.device.solve_pl_device(mat, lens[c], Time, L, T, torch.from_numpy(ini[c].copy()).to(dev), pl, status=st)
        assert not st.cpu().numpy().any()
        v = pl.cpu().numpy()
        gpu.fastlog(v)                                                  # the project's own log10, as the band's test forms y
        y = v + X[good, 12][:, None]
        ref = qr.reference(np.ascontiguousarray(y.T), W[good], q, qr.default_rules(q))
        assert not qr.mismatches(res[c]["quantile"], ref)
        assert not qr.mismatches(whole[c]["quantile"], ref)            # the cut into blocks does not matter
        qq = res[c]["quantile"]
        assert np.all(res[c]["lo"] <= qq[1]) and np.all(qq[1] <= qq[2]) and np.all(qq[2] <= res[c]["hi"])
    none = gpu.predictive.posterior_predictive(X, np.zeros(S), ini, sim, quantiles=q)
    assert all(r["q"] == q and np.isnan(r["quantile"]).all() and r["quantile"].shape == (3, T + 1) for r in none)
