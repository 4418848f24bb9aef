"""trpl_mcmc_autocov*, trpl_mcmc_autocov_pool*, trpl_mcmc_autocov_chains (include/trpl.h, the sums of the effective sample size):
header, binding and library agree; the kernels are in the library beside the ones the sampler had; every refusal the header states
is TRPL_ERR_ARG with a message naming the argument, decided with no device present; the Python refusals of Chains.ess.  No GPU
needed."""
import re

import numpy as np
import pytest

import abi_header as H

NEW = {"trpl_mcmc_autocov_dev": 11, "trpl_mcmc_autocov": 11, "trpl_mcmc_autocov_pool_dev": 7, "trpl_mcmc_autocov_pool": 8,
       "trpl_mcmc_autocov_chains": 13}
TILE = 8                                                         # trpl_mcmc_autocov_tile(): the lags one thread sums


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    for name, n_args in NEW.items():
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]) == n_args, name
    assert re.search(r"\bint trpl_mcmc_autocov_tile\s*\(void\);", H.code()) and A.SIGNATURES["trpl_mcmc_autocov_tile"] == []
    assert A.lib().trpl_mcmc_autocov_tile() == TILE
    assert H.defines()["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version() == A.ABI_VERSION          # additive: the version stays
    for fn in ("autocov", "autocov_pool", "ess_from_sums"):
        assert callable(getattr(trpl.mcmc, fn)), fn
    for fn in ("ess", "autocorr", "mcse"):
        assert callable(getattr(trpl.mcmc.Chains, fn)), fn
    for fn in ("mcmc_autocov_device", "mcmc_autocov_pool_device"):
        assert callable(getattr(trpl.device, fn)), fn


def test_the_library_exports_the_symbols_and_holds_the_kernels(trpl):
    for name in list(NEW) + ["trpl_mcmc_autocov_tile"]:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    filt = H.demangled()
    tiles = {int(n) for n in re.findall(r"trpl::mcmc::__device_stub__autocov_kernel<(\d+)>", filt)}
    assert tiles == {TILE}, sorted(tiles)
    for kernel in ("autocov_mean_kernel", "autocov_pool_kernel", "chain_stats_kernel", "levels_kernel", "levels_rungs_kernel"):
        assert "trpl::mcmc::__device_stub__%s" % kernel in filt, kernel
    # the templated kernels the sampler had keep their names and instantiations
    for kernel in ("propose_kernel", "propose_fold_kernel", "accept_kernel", "propose_rungs_kernel", "propose_rungs_fold_kernel",
                   "accept_rungs_kernel", "swap_kernel"):
        have = {int(n) for n in re.findall(r"trpl::mcmc::__device_stub__%s<(\d+)>" % kernel, filt)}
        assert have == set(range(1, 17)), (kernel, sorted(have))


def _args():
    z = np.zeros(4096)
    p = z.ctypes.data
    base = dict(H=p, n=12, ldh=7, Q=6, t0=1, t1=11, L=4, mean=p, s=p, lds=8, M=3, A=2, m2=p, pooled=p)
    return z, base


def _call(lib, form, a):
    if form == "autocov_dev":
        return lib.trpl_mcmc_autocov_dev(a["H"], a["n"], a["ldh"], a["Q"], a["t0"], a["t1"], a["L"], a["mean"], a["s"], a["lds"], None)
    if form == "autocov":
        return lib.trpl_mcmc_autocov(a["H"], a["n"], a["ldh"], a["Q"], a["t0"], a["t1"], a["L"], a["mean"], a["s"], 0, None)
    if form == "pool_dev":
        return lib.trpl_mcmc_autocov_pool_dev(a["s"], a["L"], a["lds"], a["M"], a["A"], a["pooled"], None)
    if form == "pool":
        return lib.trpl_mcmc_autocov_pool(a["s"], a["L"], a["lds"], a["M"], a["A"], a["pooled"], 0, None)
    return lib.trpl_mcmc_autocov_chains(a["H"], a["n"], a["ldh"], a["M"], a["A"], a["t0"], a["t1"], a["L"], a["mean"], a["m2"], a["pooled"],
                                        0, None)


def test_every_refusal_is_err_arg_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    keep, base = _args()

    def refused(word, forms, **kw):
        for form in forms:
            a = dict(base)
            a.update(kw)
            assert _call(lib, form, a) == A.ERR_ARG, (word, form, kw)
            assert word in lib.trpl_last_error(), (word, form, lib.trpl_last_error())

    cov, pool, chains = ("autocov", "autocov_dev"), ("pool", "pool_dev"), ("chains",)
    for arg in ("H", "mean", "s"):
        refused(arg.encode() + b" is NULL", cov, **{arg: None})
    for arg in ("s", "pooled"):
        refused(arg.encode() + b" is NULL", pool, **{arg: None})
    for arg in ("H", "mean", "m2", "pooled"):
        refused(arg.encode() + b" is NULL", chains, **{arg: None})
    for n in (0, -1):
        refused(b"n=%d" % n, cov + chains, n=n)
    for Q in (0, -1, -(1 << 40)):
        refused(b"Q=%d" % Q, cov, Q=Q)
    refused(b"ldh=5", cov + chains, ldh=5)                       # Q = M A = 6
    refused(b"lds=5", ("autocov_dev",) + pool, lds=5)
    refused(b"lds=8 must be >= M * A = 9", pool, A=3)
    for t0, t1 in ((-1, 7), (3, 3), (5, 4), (1, 13), (12, 13)):
        refused(b"t0=%d, t1=%d" % (t0, t1), cov + chains, t0=t0, t1=t1)
    for L in (0, -1, 11, 1 << 40):
        refused(b"L=%d" % L, cov + chains, L=L)                  # the range holds 10 steps
    for L in (0, -1):
        refused(b"L=%d" % L, pool, L=L)
    for M in (0, -1, -(1 << 40)):
        refused(b"M=%d" % M, pool + chains, M=M)
    for n in (0, -1, 17, 1000):
        refused(b"A=%d" % n, pool + chains, A=n)
    # the grid: 2^31 blocks of 256 columns, of 256 sequences, of columns times lag tiles, of the pool's sums
    big = (1 << 31) * 256
    refused(b"blocks", cov, Q=big, ldh=big, lds=big)
    refused(b"blocks", pool + chains, M=big, lds=16 * big, ldh=16 * big)
    refused(b"blocks", cov, n=1 << 40, t0=0, t1=1 << 40, L=1 << 39, Q=1 << 20, ldh=1 << 20, lds=1 << 20)
    refused(b"blocks", pool, L=1 << 40, A=16, M=1, lds=16)
    # no refusal: these go as far as the device.  The host-buffer forms stage the numpy buffers themselves; a _dev form takes device
    # pointers, so it is called with these host addresses only where there is no device to launch on
    suffixes = ("", "_dev") if lib.trpl_device_count() < 1 else ("",)
    for form, kw in (("autocov", {}), ("autocov", dict(L=10)), ("autocov", dict(L=1, t0=11, t1=12)), ("autocov", dict(Q=7, lds=7)),
                     ("pool", {}), ("pool", dict(M=1, A=8)), ("pool", dict(M=8, A=1)), ("pool", dict(A=16, M=1, lds=16, L=1))):
        for suffix in suffixes:
            assert _call(lib, form + suffix, dict(base, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (form, kw, lib.trpl_last_error())
    for kw in ({}, dict(L=10), dict(M=1, A=7, ldh=7), dict(M=6, A=1, t0=0, t1=12, L=12)):
        assert _call(lib, "chains", dict(base, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (kw, lib.trpl_last_error())
    del keep


def test_python_refusals(trpl):
    M = trpl.mcmc
    ch = M.Chains(np.zeros((8, 4, 2)), np.zeros((8, 4, 5)), np.zeros((8, 4)), np.zeros((8, 4), dtype=bool))
    for call in (ch.ess, ch.autocorr, ch.mcse):
        with pytest.raises(ValueError, match="split-R-hat"):     # rhat's refusal: n2 < 2
            call(burn=5)
    short = M.Chains(np.zeros((3, 4, 2)), np.zeros((3, 4, 5)), np.zeros((3, 4)), np.zeros((3, 4), dtype=bool))
    with pytest.raises(ValueError, match="split-R-hat"):
        short.ess()
    # 4 lags x 4 chains x 2 columns x 8 bytes = 256
    with pytest.raises(ValueError, match="need 256 bytes of device scratch, more than max_workspace_bytes = 255"):
        ch.ess(max_workspace_bytes=255)
    with pytest.raises(ValueError, match="need 192 bytes"):      # max_lag and values count: 3 lags x 4 chains x 2 columns
        ch.ess(max_lag=3, max_workspace_bytes=191)
    with pytest.raises(ValueError, match="need 128 bytes"):
        ch.ess(values=ch.LL[..., None], max_workspace_bytes=127)
    for bad in (np.zeros((8, 4)), np.zeros((7, 4, 2)), np.zeros((8, 5, 2)), np.zeros((8, 4, 0)), np.zeros((8, 4, 17))):
        with pytest.raises(ValueError, match="values must be"):
            ch.ess(values=bad)
    for lag in (0, -1, 5):
        with pytest.raises(ValueError, match="max_lag=%d" % lag):
            ch.ess(max_lag=lag)
    with pytest.raises(ValueError, match="H must be"):
        M.autocov(np.zeros(5), 2)
    with pytest.raises(ValueError, match="s must be"):
        M.autocov_pool(np.zeros(5), 1, 1)
    with pytest.raises(ValueError, match="at least 2 steps"):
        M.ess_from_sums(np.zeros((2, 1)), np.zeros((2, 1)), np.zeros((1, 1)), 1)
    with pytest.raises(ValueError, match="pooled must be"):
        M.ess_from_sums(np.zeros((2, 1)), np.zeros((2, 1)), np.zeros(4), 8)
    with pytest.raises(trpl.TrplError, match="L=9"):             # the library's own refusal reaches Python
        M.autocov(np.zeros((8, 3)), 9)
