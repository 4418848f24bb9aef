"""trpl_refine_* (include/trpl.h): header, binding and library agree; every refusal the header states is TRPL_ERR_ARG with a
message naming the argument, decided with no device present.  No GPU needed."""
import os
import re

import numpy as np

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_refine_chunk_rows", "trpl_refine_tile_parents", "trpl_refine_workspace_bytes", "trpl_refine_resample",
       "trpl_refine_resample_dev", "trpl_refine_draw", "trpl_refine_draw_dev", "trpl_refine_density", "trpl_refine_density_dev",
       "trpl_refine_unit", "trpl_refine_unit_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    for name in NEW:
        assert H.returns(name) in ("int", "int64_t"), name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        args = [a for a in H.params(name) if a.strip() != "void"]
        assert len(args) == len(A.SIGNATURES[name]), name
    defs = H.defines()
    assert defs["TRPL_REFINE_MAX_DIMS"] == A.REFINE_MAX_DIMS == 16
    assert defs["TRPL_REFINE_MAX_PARENTS"] == A.REFINE_MAX_PARENTS
    assert defs["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version()          # additive: the version stays
    for name in NEW[:3]:
        assert getattr(A.lib(), name).restype.__name__ == "c_long", name
    for fn in ("resample", "unit_coords", "bandwidth", "make_proposal", "draw", "density", "log_ratio", "run", "Population", "Proposal"):
        assert callable(getattr(trpl.refine, fn)), fn
    for fn in ("refine_workspace", "refine_resample_device", "refine_draw_device", "refine_density_device", "refine_unit_device"):
        assert callable(getattr(trpl.device, fn)), fn


def test_the_library_exports_the_symbols_and_holds_the_kernels(trpl):
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    have = set(re.findall(r"trpl::refine::__device_stub__(\w+)[<(]", H.demangled()))
    assert have == {"chunk_sums_kernel", "chunk_prefix_kernel", "resample_kernel", "draw_kernel", "unit_kernel", "density_kernel"}, sorted(have)
    mk = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "Makefile")).read()
    rule = re.search(r"\$\(OBJ\)/refine\.o:[^\n]*\n\t([^\n]*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(1) and "$(OBJ)/refine.o" in mk.split("$(LIB):")[1]


def test_constants_and_workspace(trpl):
    lib = trpl._abi.lib()
    chunk, tile = lib.trpl_refine_chunk_rows(), lib.trpl_refine_tile_parents()
    assert chunk >= 64 and chunk * 8 <= 64 * 1024                # the chunk's cumulative weights fit a workgroup's LDS share
    assert tile >= 1 and tile * (2 * 16 + 1) * 8 <= 160 * 1024   # a tile of parents at A = 16 fits the LDS of one CU
    assert lib.trpl_refine_workspace_bytes(-1) == 0
    for S in (0, 1, chunk, chunk + 1, 1 << 30):
        nch = (S + chunk - 1) // chunk
        assert (4 * nch + 1) * 8 <= lib.trpl_refine_workspace_bytes(S) <= (4 * nch + 1) * 8 + 1024, S


def _args():
    z = np.zeros(1024)
    p = z.ctypes.data
    lo, hi = np.zeros(4), np.array([1.0, 0.0, 3.0, 5.0])         # three active columns, one fixed
    lg = np.zeros(4, dtype=np.int32)
    keep = (z, lo, hi, lg)
    base = dict(W=p, S=8, K=4, offset=0.5, idx=p, stats=p, ws=p, wsb=1 << 20, a=p, b=p, inv_vol=p, A=3, m=2, n_uniform=3, seed=7,
                generation=2, ncol=4, lo=lo.ctypes.data, hi=hi.ctypes.data, do_log=lg.ctypes.data, flags=0, U2=p, X2=p, U=p, ldu=3, B=p,
                X=p, ldx=4)
    return keep, base


def _call(lib, form, a):
    if form == "resample":
        return lib.trpl_refine_resample(a["W"], a["S"], a["K"], a["offset"], a["idx"], a["stats"], 0, None)
    if form == "resample_dev":
        return lib.trpl_refine_resample_dev(a["W"], a["S"], a["K"], a["offset"], a["idx"], a["stats"], a["ws"], a["wsb"], None)
    if form == "draw":
        return lib.trpl_refine_draw(a["a"], a["b"], a["K"], a["A"], a["m"], a["n_uniform"], a["seed"], a["generation"], a["ncol"], a["lo"],
                                    a["hi"], a["do_log"], a["flags"], a["U2"], a["X2"], 0, None)
    if form == "draw_dev":
        return lib.trpl_refine_draw_dev(a["a"], a["b"], a["K"], a["A"], a["m"], a["n_uniform"], a["seed"], a["generation"], a["ncol"],
                                        a["lo"], a["hi"], a["do_log"], a["flags"], a["U2"], a["X2"], None)
    if form == "density":
        return lib.trpl_refine_density(a["U"], a["S"], a["ldu"], a["A"], a["a"], a["b"], a["inv_vol"], a["K"], a["B"], 0, None)
    if form == "density_dev":
        return lib.trpl_refine_density_dev(a["U"], a["S"], a["ldu"], a["A"], a["a"], a["b"], a["inv_vol"], a["K"], a["B"], None)
    if form == "unit":
        return lib.trpl_refine_unit(a["X"], a["S"], a["ldx"], a["ncol"], a["lo"], a["hi"], a["do_log"], a["flags"], a["A"], a["U"], 0, None)
    return lib.trpl_refine_unit_dev(a["X"], a["S"], a["ldx"], a["ncol"], a["lo"], a["hi"], a["do_log"], a["flags"], a["A"], a["U"], None)


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

    res, drw, den, unt = ("resample", "resample_dev"), ("draw", "draw_dev"), ("density", "density_dev"), ("unit", "unit_dev")
    for S in (-1, -(1 << 40)):
        refused(b"S=%d" % S, res + den + unt, S=S)
    for K in (0, -1, A.REFINE_MAX_PARENTS + 1):
        refused(b"K=%d" % K, res + drw + den, K=K)
    for n in (0, -1, 17, 1000):
        refused(b"A=%d" % n, drw + den + unt, A=n, ldu=2000)
    refused(b"A=2, but the box has 3 active", drw + unt, A=2)                        # not the box's count
    refused(b"A=3, but the box has 2 active", drw + unt, flags=1)                    # equal mu: column 2 is a target
    for m in (-1, -(1 << 40)):
        refused(b"m=%d" % m, drw, m=m)
    refused(b"n_uniform=-1", drw, n_uniform=-1)
    refused(b"children", drw, K=1 << 20, m=1 << 20)
    refused(b"children", drw, n_uniform=1 << 40)
    for off in (-0.1, 1.0, 1.5, np.nan, np.inf):
        refused(b"offset=", res, offset=off)
    for ldu in (2, 0, -1):
        refused(b"ldu=%d" % ldu, den, ldu=ldu)
    refused(b"ldx=3", unt, ldx=3)
    for ncol in (0, 17):
        refused(b"ncol=%d" % ncol, drw + unt, ncol=ncol)
    refused(b"flags=0x8", drw + unt, flags=8)
    bad_hi = np.array([1.0, -2.0, 3.0, 5.0])
    refused(b"column 1", drw + unt, hi=bad_hi.ctypes.data)
    lg = np.array([1, 0, 0, 0], dtype=np.int32)
    refused(b"column 0: log-uniform", drw + unt, do_log=lg.ctypes.data)
    refused(b"W is NULL", res, W=None)
    refused(b"idx is NULL", res, idx=None)
    refused(b"workspace is NULL", ("resample_dev",), ws=None)
    refused(b"workspace_bytes=8", ("resample_dev",), wsb=8)
    for arg in ("a", "b"):
        refused(arg.encode() + b" is NULL", drw + den, **{arg: None})
    for arg in ("U2", "X2"):
        refused(arg.encode() + b" is NULL", drw, **{arg: None})
    for arg in ("lo", "hi", "do_log"):
        refused(arg.encode() + b" is NULL", drw + unt, **{arg: None})
    refused(b"inv_vol is NULL", den, inv_vol=None)
    refused(b"U is NULL", den + unt, U=None)
    refused(b"B is NULL", den, B=None)
    refused(b"X is NULL", unt, X=None)
    w = np.ones(8)
    w[5] = np.inf
    refused(b"W[5] is +inf", ("resample",), W=w.ctypes.data)
    # no refusal: these go as far as the device
    for form, kw in (("resample", dict(S=0, W=None)), ("draw", dict(m=0, n_uniform=0)), ("density", dict(S=0, U=None, B=None)),
                     ("unit", dict(S=0, X=None, U=None)), ("resample", dict(offset=0.0))):
        assert _call(lib, form, dict(base, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (form, kw)
    del keep


def test_python_refusals(trpl):
    import pytest
    R = trpl.refine
    lo, hi, lg = [0.0, 0.0], [1.0, 1.0], [0, 0]
    with pytest.raises(ValueError, match="one-dimensional"):
        R.resample(np.ones((2, 2)), 4)
    with pytest.raises(ValueError, match="active columns"):
        R.unit_coords(np.ones((4, 2)), [1.0, 2.0], [1.0, 2.0], lg)
    with pytest.raises(ValueError, match="half-width"):
        R.boxes(np.full((3, 2), 0.5), [0.1, 0.0])
    pop = R.Population()
    with pytest.raises(ValueError, match="first generation"):
        pop.add(np.ones((4, 2)), np.ones((4, 2)), np.zeros(4), R.Proposal(None, None, None, 1, 1, 3, 0, 2))
    with pytest.raises(ValueError, match="empty"):
        pop.corrected()
    assert list(R.active_columns([0, 0, 0, 0], [1, 0, 1, 1], {"override_equal_mu": True})) == [0, 3]
    del lo, hi
