"""trpl_mcmc_evidence_sums[_dev] (include/trpl.h, the sums of the log-evidence estimates of a tempered run): header, binding and
library agree; the kernels are in the library; the version stays; every refusal the header states is TRPL_ERR_ARG with a message
naming the argument, in both forms, decided with no device present.  No GPU needed."""
import os
import re

import numpy as np

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"trpl_mcmc_evidence_sums_dev": 11, "trpl_mcmc_evidence_sums": 12}
KERNELS = ("evidence_extrema_block_kernel", "evidence_extrema_kernel", "evidence_sums_kernel")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    for name, n_args in NEW.items():
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        assert len(H.params(name)) == len(A.SIGNATURES[name]) == n_args, name
    defs = H.defines()
    assert defs["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version() == A.ABI_VERSION          # additive: the version stays
    assert defs["TRPL_MCMC_EVIDENCE_SUMS"] == 6 == A.MCMC_EVIDENCE_SUMS
    for fn in ("evidence_sums", "log_evidence_ratios"):
        assert callable(getattr(trpl.mcmc, fn)), fn
    assert callable(trpl.mcmc.Tempered.log_evidence) and callable(trpl.posterior.log_evidence)
    assert callable(trpl.device.mcmc_evidence_sums_device)


def test_the_library_exports_the_symbols_and_holds_the_kernels(trpl):
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    for kernel in KERNELS:
        assert "trpl::mcmc::__device_stub__%s(" % kernel in H.demangled(), kernel
    listed = open(os.path.join(ROOT, "tools", "kernel_resources.py")).read()
    assert "mcmc_evidence" in listed.split('"""')[1] and '"mcmc_evidence"' in listed          # usage and the contraction flag


def _call(lib, form, a):
    head = (a["LL"], a["K"], a["n"], a["C"], a["t0"], a["t1"], a["B"], a["tf"], a["ext"], a["sums"])
    if form == "dev":
        return lib.trpl_mcmc_evidence_sums_dev(*head, None)
    return lib.trpl_mcmc_evidence_sums(*head, 0, None)


def test_every_refusal_is_err_arg_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()
    keep, tf = np.zeros(8192), np.array([1.0, 2.0, 2.0, 1.5] + [3.0] * 61)          # 65 temperatures: K = 65 reads none of them
    p = keep.ctypes.data
    base = dict(LL=p, K=4, n=12, C=5, t0=1, t1=11, B=5, tf=tf.ctypes.data, ext=p, sums=p)

    def refused(word, **kw):
        for form in ("host", "dev"):
            assert _call(lib, form, dict(base, **kw)) == A.ERR_ARG, (word, form, kw)
            assert word in lib.trpl_last_error(), (word, form, lib.trpl_last_error())

    for arg in ("LL", "tf", "ext", "sums"):
        refused(arg.encode() + b" is NULL", **{arg: None})
    for K in (0, -1, 65, 1 << 20):
        refused(b"K=%d" % K, K=K)
    for n in (0, -1, -(1 << 40)):
        refused(b"n=%d" % n, n=n)
    for C in (0, -1, -(1 << 40)):
        refused(b"C=%d" % C, C=C)
    refused(b"C=%d" % (1 << 58), C=1 << 58)                      # K n C would not fit
    for t0, t1 in ((-1, 7), (3, 3), (5, 4), (1, 13), (12, 13)):
        refused(b"t0=%d, t1=%d" % (t0, t1), t0=t0, t1=t1)
    for B in (0, -1, 3, 4, 11, 20):                              # the range holds 10 steps
        refused(b"B=%d" % B, B=B)
    for k, bad in ((0, 0.0), (1, -1.0), (2, np.inf), (3, np.nan), (0, -np.inf)):
        t = tf.copy()
        t[k] = bad
        refused(b"tf[%d]=" % k, tf=t.ctypes.data)
    # more than 2^31 - 1 workgroups: K B = 4 * 2^29
    refused(b"workgroups", n=1 << 29, t0=0, t1=1 << 29, B=1 << 29, C=1)
    # no refusal: these go as far as the device.  The host-buffer form stages the numpy buffers itself; the _dev form takes device
    # pointers, so it is called with these host addresses only where there is no device to launch on
    forms = ("host", "dev") if lib.trpl_device_count() < 1 else ("host",)
    for kw in ({}, dict(B=1), dict(B=10), dict(B=2), dict(K=1), dict(t0=0, t1=12, B=12), dict(K=64, n=2, t0=0, t1=2, B=1, C=1)):
        for form in forms:
            assert _call(lib, form, dict(base, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (form, kw, lib.trpl_last_error())
    del keep
