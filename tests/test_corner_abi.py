"""trpl_corner, trpl_corner_columns_dev, trpl_corner_hist_dev, trpl_corner_workspace_bytes (include/trpl.h): header, binding and
library agree; the column codes and limits are one set of numbers; every refusal the header states is TRPL_ERR_ARG with a
message, decided with no device present.  No GPU needed."""
import os
import re

import numpy as np

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_corner", "trpl_corner_columns_dev", "trpl_corner_hist_dev", "trpl_corner_workspace_bytes")
CODES = ("N0", "P0", "MU_N", "MU_P", "B", "SF", "SB", "CN", "CP", "TAU_N", "TAU_P", "LAMBDA", "MAG",
         "TAU_EFF", "TAU_RAD", "S_SUM", "MU_EFF", "EPSILON", "TAU_SUM")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    for name in NEW:
        assert H.returns(name) in ("int", "int64_t"), name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]), name
    defs = H.defines()
    assert defs["TRPL_CORNER_MAX_COLS"] == A.CORNER_MAX_COLS == 19 == len(trpl.posterior.CORNER_COLUMNS)
    assert defs["TRPL_CORNER_MAX_BINS"] == A.CORNER_MAX_BINS == 128
    assert defs["TRPL_CORNER_PRIMARY"] == A.CORNER_PRIMARY == 13
    for k, c in enumerate(CODES):
        assert defs["TRPL_COL_" + c] == getattr(A, "COL_" + c) == k, c
    assert trpl.posterior.CORNER_COLUMNS[:13] == tuple(trpl.PARAM_NAMES)
    assert defs["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version()          # additive: the version stays
    assert A.lib().trpl_corner_workspace_bytes.restype.__name__ == "c_long"
    for fn in ("columns", "corner"):
        assert callable(getattr(trpl.posterior, fn)), fn
    for fn in ("corner_columns_device", "corner_hist_device", "corner_workspace"):
        assert callable(getattr(trpl.device, fn)), fn
    assert trpl.corner is trpl.posterior.corner


def test_the_library_exports_the_symbols_and_holds_the_kernels(trpl):
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    have = set(re.findall(r"trpl::corner::__device_stub__(\w+)[<(]", H.demangled()))
    assert have == {"columns_kernel", "keys_kernel", "hist_kernel"}, sorted(have)
    mk = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "Makefile")).read()
    rule = re.search(r"\$\(OBJ\)/corner\.o:[^\n]*\n\t([^\n]*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(1) and "$(OBJ)/corner.o" in mk.split("$(LIB):")[1]


def test_workspace_bytes(trpl):
    lib = trpl._abi.lib()
    for S, D in ((0, 1), (1, 1), (1025, 19), (1 << 33, 19)):
        n = lib.trpl_corner_workspace_bytes(S, D)
        assert S * D <= n <= S * D + 1024, (S, D, n)
    for S, D in ((-1, 1), (1, 0), (1, 20)):
        assert lib.trpl_corner_workspace_bytes(S, D) == 0, (S, D)


def _args():
    z = np.zeros(64)
    p = z.ctypes.data
    cols = np.arange(19, dtype=np.int32)
    lg = np.zeros(19, dtype=np.int32)
    lo, hi = np.zeros(19), np.ones(19)
    ex = np.full(13, np.nan)
    keep = (z, cols, lg, lo, hi, ex)
    base = dict(X=p, S=4, ldx=13, LL=p, tf=1.0, cols=cols.ctypes.data, dolog=lg.ctypes.data, D=2, thickness=2000.0, excl_lo=ex.ctypes.data,
                excl_hi=ex.ctypes.data, lo=lo.ctypes.data, hi=hi.ctypes.data, bins=8, V=p, W=p, kept=p, h1=p, c1=p, h2=p, ldv=4, LLk=p, ws=p)
    return keep, base


def _call(lib, form, a):
    if form == "host":
        return lib.trpl_corner(a["X"], a["S"], a["ldx"], a["LL"], a["tf"], a["cols"], a["dolog"], a["D"], a["thickness"], a["excl_lo"],
                               a["excl_hi"], a["lo"], a["hi"], a["bins"], a["V"], a["W"], a["kept"], a["h1"], a["c1"], a["h2"], 0, None)
    if form == "columns":
        return lib.trpl_corner_columns_dev(a["X"], a["S"], a["ldx"], a["cols"], a["dolog"], a["D"], a["thickness"], a["excl_lo"],
                                           a["excl_hi"], a["LL"], a["V"], a["LLk"], a["kept"], None)
    return lib.trpl_corner_hist_dev(a["V"], a["S"], a["ldv"], a["D"], a["W"], a["lo"], a["hi"], a["bins"], a["h1"], a["c1"], a["h2"],
                                    a["ws"], None)


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

    every, col, hist = ("host", "columns", "hist"), ("host", "columns"), ("host", "hist")
    for D in (0, -1, 20, 1000):
        refused(b"D=%d" % D, every, D=D)
    for S in (-1, -(1 << 40)):
        refused(b"S=%d" % S, every, S=S)
    for bad in (-1, 19, 255):
        for d in (0, 1):
            cols = np.array([1, 2], dtype=np.int32)
            cols[d] = bad
            refused(b"cols[%d]=%d" % (d, bad), col, cols=cols.ctypes.data)
    for bins in (0, -3, 129, 1 << 20):
        refused(b"bins=%d" % bins, hist, bins=bins)
    for d, (a, b) in enumerate(((np.nan, 1.0), (0.0, np.inf), (-np.inf, 1.0), (0.0, np.nan), (1.0, 1.0), (2.0, 1.0))):
        lo, hi = np.zeros(6), np.ones(6)
        lo[d], hi[d] = a, b
        refused(b"lo[%d]" % d, hist, lo=lo.ctypes.data, hi=hi.ctypes.data, D=6)
    tau = np.array([3, 13], dtype=np.int32)
    for th in (0.0, -1.0, np.inf, np.nan):
        refused(b"thickness_nm", col, cols=tau.ctypes.data, thickness=th)
    notau = np.array([3, 14], dtype=np.int32)                    # tau_rad does not need the thickness
    a = dict(base, cols=notau.ctypes.data, thickness=-1.0)
    assert _call(lib, "host", a) in (A.OK, A.ERR_NODEVICE)
    refused(b"excl_lo and excl_hi", col, excl_lo=None)
    refused(b"excl_lo and excl_hi", col, excl_hi=None)
    half_lo, half_hi = np.full(13, np.nan), np.full(13, np.nan)
    half_lo[9] = 1.0                                             # a tested column without its upper limit would drop every sample
    refused(b"excl_hi[9] is NaN", col, excl_lo=half_lo.ctypes.data, excl_hi=half_hi.ctypes.data)
    for ldx in (12, 0, -1):
        refused(b"ldx=%d" % ldx, col, ldx=ldx)
    refused(b"ldv=3", ("hist",), ldv=3)
    refused(b"h1 is NULL", hist, h1=None)
    for arg in ("cols", "dolog"):
        refused(arg.encode() + b" is NULL", col, **{arg: None})
    for arg in ("lo", "hi"):
        refused(arg.encode() + b" is NULL", hist, **{arg: None})
    refused(b"X is NULL", col, X=None)
    refused(b"V is NULL", ("columns", "hist"), V=None)
    refused(b"W is NULL", ("hist",), W=None)
    refused(b"workspace is NULL", ("hist",), ws=None)
    refused(b"LLk needs LL", ("columns",), LL=None)
    refused(b"LL is NULL", ("host",), LL=None)
    for tf in (0.0, -1.0, np.nan):
        refused(b"tf=", ("host",), tf=tf)
    # S == 0 is no refusal: it goes as far as the device
    assert _call(lib, "host", dict(base, S=0, X=None, LL=None)) in (A.OK, A.ERR_NODEVICE)
    del keep


def test_python_refusals(trpl):
    import pytest
    P = trpl.posterior
    X, LL = np.ones((4, 13)), np.zeros(4)
    with pytest.raises(ValueError, match="unknown column"):
        P.corner(X, LL, ["p0", "nope"], {"p0": (0, 1), "nope": (0, 1)})
    with pytest.raises(ValueError, match="twice"):
        P.corner(X, LL, ["p0", "p0"], {"p0": (0, 1)})
    with pytest.raises(ValueError, match="bin_count"):
        P.corner(X, LL, ["p0"], {"p0": (0, 1)}, bin_count=129)
    with pytest.raises(ValueError, match="primary"):
        P.columns(X, ["p0"], exclude_limits={"tau_eff": (0, 1)}, LL=LL)
    with pytest.raises(ValueError, match=r"\(S, 13\)"):
        P.columns(np.ones((4, 12)), ["p0"])
