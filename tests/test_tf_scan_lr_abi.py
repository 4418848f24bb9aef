"""trpl_posterior_weights_lr[_dev], trpl_posterior_tf_scan_lr[_dev] and trpl_posterior_tf_scan_lr_workspace (include/trpl.h: the
posterior weights and the temperature scan with a proposal log-ratio kept beside LL): header, binding and library agree; every
refusal the header states is TRPL_ERR_ARG with its argument named, with no device present; the workspace is 0 for refused shapes;
the Makefile compiles the shared unit without contraction; the exports are only added (ABI 5).  No GPU needed."""
import os
import re

import numpy as np

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bayesian-inference-trpl_amd")
NEW = ("trpl_posterior_weights_lr", "trpl_posterior_weights_lr_dev", "trpl_posterior_tf_scan_lr", "trpl_posterior_tf_scan_lr_dev",
       "trpl_posterior_tf_scan_lr_workspace")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    hdr = open(os.path.join(ROOT, "include", "trpl.h")).read()          # with its comments: the sentences below
    for name in NEW:
        assert H.returns(name) in ("int", "int64_t"), name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]), name
        # the ratio follows LL in every call that takes samples
        assert name.endswith("workspace") or [a.split()[-1].lstrip("*") for a in H.params(name)][:2] == ["LL", "lnr"], name
    assert H.defines()["TRPL_ABI_VERSION"] == 5 == A.ABI_VERSION == A.lib().trpl_abi_version()      # additive: the version stays
    assert A.lib().trpl_posterior_tf_scan_lr_workspace.restype.__name__ == "c_long"               # bytes, not an int
    for name in NEW:
        if not name.endswith("workspace"):
            assert getattr(A.lib(), name).restype.__name__ == "c_int", name
    # the definition and the refusals are stated with the declarations
    doc = hdr[hdr.index("trpl_posterior_weights_lr, trpl_posterior_tf_scan_lr"):hdr.index("int trpl_posterior_weights_lr(")]
    for words in ("LL[s] / tf_k - lnr[s]", "nanmax_s e_k[s]", "1000 ln 2", "stats[K][6]", "BIT FOR BIT", "NULL lnr", "lnr = +inf",
                  "lnr = -inf"):
        assert words in doc, words


def test_python_surface(trpl):
    import inspect
    P, R, Dv = trpl.posterior, trpl.refine, trpl.device
    for fn in (P.weights, P.tf_scan, P.find_best_tf, P.calc_max_uncertainty):
        assert inspect.signature(fn).parameters["log_ratio"].default is None, fn
    sig = inspect.signature(P.tf_for_ess).parameters
    assert list(sig)[:3] == ["LL", "target", "log_ratio"] and sig["rtol"].default == 1e-6 and sig["info"].default is None
    assert all(k in sig for k in ("lo", "hi", "device"))
    for fn in ("posterior_weights_lr_device", "posterior_tf_scan_lr_device", "posterior_tf_scan_lr_workspace"):
        assert callable(getattr(Dv, fn)), fn
    for fn in ("log_ratio", "tf_scan", "tf_for_ess", "corrected", "weights", "ess"):
        assert callable(getattr(R.Population, fn)), fn
    run = inspect.signature(R.run).parameters
    assert run["target_ess"].default is None and run["tf_hi"].default is None


def _scan(lib, dev, LL, lnr, S, V, D, tfs, K, stats, mean, var, Q, ws=None, wsb=1 << 40):
    if dev:
        return lib.trpl_posterior_tf_scan_lr_dev(LL, lnr, S, V, D, tfs, K, stats, mean, var, Q, ws, wsb, None)
    return lib.trpl_posterior_tf_scan_lr(LL, lnr, S, V, D, tfs, K, stats, mean, var, Q, 0, None)


def test_scan_refusals_name_their_argument_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.zeros(6 * 64)
    good = np.geomspace(1.0, 100.0, 64)
    p, t = z.ctypes.data, good.ctypes.data

    def refused(word, dev, **kw):
        a = dict(LL=p, lnr=p, S=8, V=p, D=2, tfs=t, K=3, stats=p, mean=p, var=p, Q=p, ws=p)
        a.update(kw)
        assert _scan(lib, dev, **a) == A.ERR_ARG, (word, dev, kw)
        assert word in lib.trpl_last_error(), (word, dev, lib.trpl_last_error())

    for dev in (False, True):
        for K in (0, -1, 65, 1 << 20):
            refused(b"K=%d" % K, dev, K=K)
        assert b"TRPL_TF_SCAN_MAX" in lib.trpl_last_error()
        for D in (-1, 17, 1000):
            refused(b"D=%d" % D, dev, D=D)
        for S in (0, -5):
            refused(b"S=%d" % S, dev, S=S)
        for arg in ("LL", "lnr", "tfs", "stats", "mean", "var", "Q", "V"):
            refused(arg.encode() + b" is NULL", dev, **{arg: None})
    refused(b"workspace is NULL", True, ws=None)
    refused(b"workspace of 8 bytes", True, wsb=8)
    for k, bad in ((0, 0.0), (1, -1.0), (2, float("nan")), (63, float("inf")), (31, -float("inf"))):
        tfs = good.copy()
        tfs[k] = bad
        refused(b"tfs[%d]" % k, False, tfs=tfs.ctypes.data, K=64)
    # D == 0 takes no columns and no column outputs: accepted as far as the device
    assert _scan(lib, False, p, p, 8, None, 0, t, 3, p, None, None, None) in (A.OK, A.ERR_NODEVICE)


def test_weights_refusals_name_their_argument_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    z = np.zeros(64)
    p = z.ctypes.data

    def refused(word, dev, LL=p, lnr=p, S=8, tf=2.0, W=p, ws=p, wsb=1 << 40):
        rc = (lib.trpl_posterior_weights_lr_dev(LL, lnr, S, tf, W, None, ws, wsb, None) if dev
              else lib.trpl_posterior_weights_lr(LL, lnr, S, tf, W, None, 0, None))
        assert rc == A.ERR_ARG, (word, dev)
        assert word in lib.trpl_last_error(), (word, dev, lib.trpl_last_error())

    for dev in (False, True):
        for S in (0, -5):
            refused(b"S=%d" % S, dev, S=S)
        for arg in ("LL", "lnr", "W"):
            refused(arg.encode() + b" is NULL", dev, **{arg: None})
        for tf in (0.0, -1.0, float("nan"), float("inf")):
            refused(b"tf=", dev, tf=tf)
    refused(b"workspace is NULL", True, ws=None)
    refused(b"workspace of 8 bytes", True, wsb=8)


def test_workspace_bytes(trpl):
    lib = trpl._abi.lib()
    blocks = 1024                                   # kMaxBlocks of csrc/posterior_common.hpp (tests/test_tf_scan_abi.py pins it)
    for S, D, K in ((1, 0, 1), (1000, 13, 64), (1 << 33, 16, 64)):
        n = lib.trpl_posterior_tf_scan_lr_workspace(S, D, K)
        # the block partials of the widest phase, [K][kMaxBlocks][2 + D], then max[K], count, norm[K], sums[K][2 + D], central[K][D]
        assert n >= 8 * (K * blocks * (2 + D) + 1 + K * (4 + 2 * D)) and n % 8 == 0, (S, D, K, n)
        assert n < 8 * (K * blocks * (2 + D) + 4096)
        # the max phase keeps K rows of block maxima and one row of block counts in the partials
        assert K * blocks * (2 + D) >= (K + 1) * blocks
    for S, D, K in ((0, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 17, 1), (1, 1, 0), (1, 1, 65)):
        assert lib.trpl_posterior_tf_scan_lr_workspace(S, D, K) == 0, (S, D, K)


def test_the_unit_is_compiled_without_contraction_and_shares_the_reductions():
    """The calls with a ratio are instantiations of the kernels of posterior_scan.hip and posterior.hip: no unit of their own."""
    mk = open(os.path.join(PKG, "Makefile")).read()
    rule = re.search(r"\$\(OBJ\)/posterior_scan\.o:([^\n]*)\n\t([^\n]*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(2) and "posterior_common.hpp" in rule.group(1)
    link = re.search(r"^\$\(LIB\):([^\n]*)", mk, flags=re.M).group(1)
    assert "$(OBJ)/posterior_scan.o" in link and "posterior_lr.o" not in link and "posterior_lr" not in mk
    assert not os.path.exists(os.path.join(PKG, "csrc", "posterior_lr.hip"))
    src = open(os.path.join(PKG, "csrc", "posterior_scan.hip")).read()
    assert '#include "posterior_common.hpp"' in src
    assert not re.search(r"constexpr int (kThreads|kMaxBlocks|kMaxDim)\b", src)
    assert "__shfl_xor" not in src and "grid_for(int64_t" not in src and "two_sum(double" not in src
    assert "final_reduce" in src and "__global__ void final_reduce" not in src and "block_reduce<" in src


def test_the_kernels_are_in_the_shared_object(trpl):
    from test_tf_scan_abi import SCAN_KERNELS, WEIGHTS_KERNELS, kernels_of
    have, nm = kernels_of("trpl::post::scan")           # also asserts that no trpl::post::lr:: symbol remains
    assert have == SCAN_KERNELS, sorted(have)
    assert {k for k in have if k.endswith("<trpl::post::Ratio>")} == {
        "weights_partial<trpl::post::Ratio>", "moments1_partial<trpl::post::Ratio>", "moments2_partial<trpl::post::Ratio>",
        "finish_kernel<trpl::post::Ratio>"}
    have, _ = kernels_of("trpl::post")
    assert WEIGHTS_KERNELS <= have, sorted(have)
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, nm), name
