"""trpl_refine_affine*, trpl_refine_draw_oriented* (include/trpl.h): header, binding and library agree; the kernels are in the
library and their unit is compiled without contraction; every refusal the header states is TRPL_ERR_ARG with a message naming the
argument, decided with no device present.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_refine_affine", "trpl_refine_affine_dev", "trpl_refine_draw_oriented", "trpl_refine_draw_oriented_dev")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]), name
    assert H.defines()["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version() == A.ABI_VERSION          # additive: the version stays
    for fn in ("orientation", "affine", "boxes_oriented", "make_proposal", "draw", "density", "run"):
        assert callable(getattr(trpl.refine, fn)), fn
    assert trpl.refine.Proposal(None, None, None, 1, 1, 0, 0, 2).orient is None      # eight fields still make a proposal
    for fn in ("refine_affine_device", "refine_draw_oriented_device"):
        assert callable(getattr(trpl.device, fn)), fn


def test_the_library_exports_the_symbols_and_holds_the_kernels(trpl):
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    for kernel in ("affine_kernel", "draw_oriented_kernel"):
        have = {int(n) for n in re.findall(r"trpl::refine_oriented::__device_stub__%s<(\d+)>" % kernel, H.demangled())}
        assert have == set(range(1, 17)), (kernel, sorted(have))
    mk = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "Makefile")).read()
    rule = re.search(r"\$\(OBJ\)/refine_oriented\.o:([^\n]*)\n\t([^\n]*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(2) and "refine_common.hpp" in rule.group(1)
    assert "$(OBJ)/refine_oriented.o" in mk.split("$(LIB):")[1]
    old = re.search(r"\$\(OBJ\)/refine\.o:([^\n]*)\n\t([^\n]*)", mk)                  # the shared header rebuilds both units
    assert old and "refine_common.hpp" in old.group(1) and "-ffp-contract=off" in old.group(2)


def _args():
    A = 3
    z = np.zeros(1024)
    p = z.ctypes.data
    M = np.array([[2.0, np.nan, np.nan], [-0.5, 1.5, np.nan], [0.25, -0.75, 3.0]])           # the strict upper part is never read
    c = np.array([0.5, 0.4, 0.6])
    h = np.array([0.1, 0.2, 0.3])
    lo, hi = np.zeros(4), np.array([1.0, 0.0, 3.0, 5.0])         # three active columns, one fixed
    lg = np.zeros(4, dtype=np.int32)
    keep = (z, M, c, h, lo, hi, lg)
    base = dict(U=p, S=8, ldu=3, A=A, M=M.ctypes.data, c=c.ctypes.data, Z=p, ldz=3, zc=p, h=h.ctypes.data, L=M.ctypes.data, K=4, m=2,
                n_uniform=3, seed=7, generation=2, ncol=4, lo=lo.ctypes.data, hi=hi.ctypes.data, do_log=lg.ctypes.data, flags=0, Z2=p,
                U2=p, X2=p, inside=p)
    return keep, base


def _call(lib, form, a):
    if form == "affine":
        return lib.trpl_refine_affine(a["U"], a["S"], a["ldu"], a["A"], a["M"], a["c"], a["Z"], a["ldz"], 0, None)
    if form == "affine_dev":
        return lib.trpl_refine_affine_dev(a["U"], a["S"], a["ldu"], a["A"], a["M"], a["c"], a["Z"], a["ldz"], None)
    args = [a["zc"], a["h"], a["L"], a["c"], a["K"], a["A"], a["m"], a["n_uniform"], a["seed"], a["generation"], a["ncol"], a["lo"], a["hi"],
            a["do_log"], a["flags"], a["Z2"], a["U2"], a["X2"], a["inside"]]
    if form == "draw":
        return lib.trpl_refine_draw_oriented(*(args + [0, None]))
    return lib.trpl_refine_draw_oriented_dev(*(args + [None]))


def test_every_refusal_is_err_arg_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    keep, base = _args()
    good_M = keep[1]

    def refused(word, forms, **kw):
        for form in forms:
            a = dict(base)
            a.update(kw)
            assert _call(lib, form, a) == A.ERR_ARG, (word, form, kw)
            assert word in lib.trpl_last_error(), (word, form, lib.trpl_last_error())

    aff, drw = ("affine", "affine_dev"), ("draw", "draw_dev")
    for arg in ("U", "M", "c", "Z"):
        refused(arg.encode() + b" is NULL", aff, **{arg: None})
    for arg in ("zc", "h", "L", "c", "Z2", "U2", "X2", "inside", "lo", "hi", "do_log"):
        refused(arg.encode() + b" is NULL", drw, **{arg: None})
    for n in (0, -1, 17, 1000):
        refused(b"A=%d" % n, aff + drw, A=n, ldu=2000, ldz=2000)
    refused(b"A=2, but the box has 3 active", drw, A=2)
    for ld in (2, 0, -1):
        refused(b"ldu=%d" % ld, aff, ldu=ld)
        refused(b"ldz=%d" % ld, aff, ldz=ld)
    for S in (0, -1, -(1 << 40)):
        refused(b"S=%d" % S, aff, S=S)
    for K in (0, -1, A.REFINE_MAX_PARENTS + 1):
        refused(b"K=%d" % K, drw, K=K)
    for m in (-1, -(1 << 40)):
        refused(b"m=%d" % m, drw, m=m)
    refused(b"n_uniform=-1", drw, n_uniform=-1)
    refused(b"children", drw, K=1 << 20, m=1 << 20)
    # non-finite entries of the lower triangle, of c and of h; a diagonal that is not positive; h_d <= 0
    for bad in (np.nan, np.inf, -np.inf):
        for (i, j) in ((0, 0), (1, 0), (2, 1), (2, 2)):
            T = np.where(np.isnan(good_M), 0.0, good_M)
            T[i, j] = bad
            refused(b"M[%d][%d] is not finite" % (i, j), aff, M=T.ctypes.data)
            refused(b"L[%d][%d] is not finite" % (i, j), drw, L=T.ctypes.data)
        v = np.array([0.5, bad, 0.6])
        refused(b"c[1] is not finite", aff + drw, c=v.ctypes.data)
        refused(b"h[1]=", drw, h=v.ctypes.data)
    for d in (0.0, -0.0, -1.5):
        T = np.where(np.isnan(good_M), 0.0, good_M)
        T[1, 1] = d
        refused(b"M[1][1]=", aff, M=T.ctypes.data)
        refused(b"L[1][1]=", drw, L=T.ctypes.data)
        refused(b"h[2]=", drw, h=np.array([0.1, 0.2, d]).ctypes.data)
    # no refusal: these go as far as the device -- the NaN in the strict upper part of M and L is not looked at
    for form, kw in (("affine", {}), ("draw", {}), ("draw", dict(m=0, n_uniform=0)), ("affine", dict(ldu=5, ldz=4))):
        assert _call(lib, form, dict(base, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (form, kw, lib.trpl_last_error())
    del keep


def test_python_refusals(trpl):
    R = trpl.refine
    with pytest.raises(ValueError, match="M \\(A, A\\)"):
        R.affine(np.zeros((4, 3)), np.eye(2), np.zeros(3))
    with pytest.raises(ValueError, match="half-width"):
        R.boxes_oriented(np.zeros((2, 2)), [0.1, 0.0], 0.0)
    a, b, iv = R.boxes_oriented(np.array([[0.0, 1.0], [5.0, -3.0]]), [0.5, 0.25], np.log(2.0))
    assert np.array_equal(b - a, [[1.0, 0.5], [1.0, 0.5]]) and np.allclose(iv, 1.0 / (1.0 * 0.5 * 2.0), rtol=1e-15, atol=0)
    assert a[1, 1] == -3.25                                      # not clipped to the cube
    pop = R.Population()
    pop.add(np.ones((2, 2)), np.ones((2, 2)), np.zeros(2))
    with pytest.raises(ValueError, match="inside"):
        pop.add(np.ones((3, 2)), np.ones((3, 2)), np.zeros(3), R.Proposal(None, None, None, 1, 1, 2, 0, 2), inside=np.ones(2))
    pop.add(np.ones((3, 2)), np.ones((3, 2)), np.array([1.0, 2.0, 3.0]), R.Proposal(None, None, None, 1, 1, 2, 0, 2),
            inside=np.array([1, 0, 1], dtype=np.int32))
    assert np.array_equal(pop.LL[1], [1.0, -np.inf, 3.0])        # an outside child has LL = -inf whatever was passed
