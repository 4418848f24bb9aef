"""trpl_mcmc_propose_subspace* (include/trpl.h, subspace differential evolution): header, binding and library agree; the kernel is in
the library for every A, folded and not, and its unit is compiled without contraction; every refusal the header states is
TRPL_ERR_ARG with a message naming the argument, decided with no device present, and of two simultaneous faults the one the header
lists first wins.  No GPU needed."""
import inspect
import itertools
import os
import re

import numpy as np

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trpl_mcmc_propose_subspace", "trpl_mcmc_propose_subspace_dev")
# the arguments in the entry point's order, before the tail (stream, or device and seconds)
ARGS = ("U", "partners", "count", "P", "group", "A", "gamma", "scale", "chain0", "seed", "step", "ncol", "lo", "hi", "do_log", "flags", "Up",
        "Xp", "inside", "pairs", "ncr", "pcr", "gamma_tab", "e_width", "mask", "sel")


def test_header_binding_and_library_agree(trpl):
    A = trpl._abi
    hdr = open(os.path.join(ROOT, "include", "trpl.h")).read()          # with its comments: the Philox indices below
    for name in NEW:
        assert H.returns(name) == "int", name
        assert name in A.SIGNATURES and hasattr(A.lib(), name), name
        names = [re.search(r"(\w+)\s*$", a).group(1) for a in H.params(name)]
        tail = ["stream"] if name.endswith("_dev") else ["device", "seconds"]
        assert names == list(ARGS) + tail, name                   # propose_rungs' arguments in its order, then the move's
        assert len(names) == len(A.SIGNATURES[name]), name
        rungs = A.SIGNATURES[name.replace("subspace", "rungs")]
        assert A.SIGNATURES[name][:19] == rungs[:19] and A.SIGNATURES[name][26:] == rungs[19:], name
        assert [t.__name__ for t in A.SIGNATURES[name][19:26]] == ["c_int", "c_int", "c_void_p", "c_void_p", "c_double", "c_void_p", "c_void_p"]
    defs = H.defines()
    assert defs["TRPL_MCMC_MAX_PAIRS"] == 4 == A.MCMC_MAX_PAIRS and defs["TRPL_MCMC_MAX_CR"] == 8 == A.MCMC_MAX_CR
    assert defs["TRPL_ABI_VERSION"] == 5 == A.lib().trpl_abi_version() == A.ABI_VERSION          # additive: the version stays
    for j in ("12 .. 19", "20 .. 27", "j = 28 ", "j = 28 + p"):  # every Philox index of the move is written into the header
        assert j in hdr, j
    common = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "csrc", "mcmc_common.hpp")).read()
    assert re.search(r"kCrossCall = 12, kJumpCall = 20, kSelectCall = 28, kPairCall = 28;", common)
    assert callable(trpl.mcmc.propose_subspace) and callable(trpl.device.mcmc_propose_subspace_device)
    for fn in (trpl.mcmc.run, trpl.mcmc.run_tempered):
        sig = inspect.signature(fn).parameters
        assert (sig["pairs"].default, sig["ncr"].default, sig["e_width"].default, sig["adapt_cr"].default) == (3, 3, 0.05, False)
        assert sig["kind"].default == "de"


def test_the_library_holds_the_kernel_and_its_unit_is_uncontracted(trpl):
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, H.exports()), name
    have = set(re.findall(r"trpl::mcmc::__device_stub__subspace_kernel<(\d+), (true|false)>", H.demangled()))
    assert have == {(str(n), f) for n in range(1, 17) for f in ("true", "false")}, sorted(have)
    mk = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "Makefile")).read()
    rule = re.search(r"\$\(OBJ\)/mcmc_subspace\.o:([^\n]*)\n\t([^\n]*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(2) and "mcmc_common.hpp" in rule.group(1)
    assert "$(OBJ)/mcmc_subspace.o" in mk.split("$(LIB):")[1]
    src = open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "csrc", "mcmc.hip")).read()
    assert "fold_outside(double" not in src                       # one definition, in the shared header
    assert "fold_outside(double" in open(os.path.join(ROOT, "bayesian-inference-trpl_amd", "csrc", "mcmc_common.hpp")).read()


# ---- the refusals.  The faultless call: three active columns and a fixed one; the arrays live as long as the module.
Z = np.zeros(4096)
LO, HI, LG = np.zeros(4), np.array([1.0, 0.0, 3.0, 5.0]), np.zeros(4, dtype=np.int32)
SCALE, PCR, TAB = np.full(3, 1e-3), np.array([0.5, 0.0, 0.5]), np.full((2, 3), 0.7)
BASE = dict({k: Z.ctypes.data for k in ("U", "partners", "Up", "Xp", "inside", "mask", "sel")}, count=8, P=8, group=4, A=3, gamma=1.0,
            scale=SCALE.ctypes.data, chain0=0, seed=7, step=2, ncol=4, lo=LO.ctypes.data, hi=HI.ctypes.data, do_log=LG.ctypes.data, flags=0,
            pairs=2, ncr=3, pcr=PCR.ctypes.data, gamma_tab=TAB.ctypes.data, e_width=0.05)
KEEP = [np.array([1e-3, -1.0, 1e-3]), np.array([0.5, -0.1, 0.6]), np.array([0.5, np.nan, 0.5]), np.zeros(3), np.array([[0.7, 0.7, 0.7], [0.7, np.inf, 0.7]]),
        np.array([1.0, 0.0, -3.0, 5.0]), np.array([1, 0, 0, 0], dtype=np.int32), np.array([np.inf, 0.5, 0.5])]
# (the text of the refusal, the arguments that provoke it), in the order the header lists the refusals: trpl_mcmc_propose_rungs'
# first, then the move's own, then the box's.  Two faults on one argument are no pair.
FAULTS = [
    (b"count=0 must be >= 1", dict(count=0)),
    (b"count=549755813888 is more than 2^31 - 1 blocks", dict(count=(1 << 31) * 256)),
    (b"A=17 must be in", dict(A=17)),
    (b"chain0=-1 must be >= 0", dict(chain0=-1)),
    (b"P=1 must be >= 2", dict(P=1)),
    (b"partners is NULL", dict(partners=None)),
    (b"U is NULL", dict(U=None)),
    (b"scale is NULL", dict(scale=None)),
    (b"Up is NULL", dict(Up=None)),
    (b"Xp is NULL", dict(Xp=None)),
    (b"inside is NULL", dict(inside=None)),
    (b"gamma=nan must be finite", dict(gamma=np.nan)),
    (b"flags=0x28: only the TRPL_BOX_EQUAL_* bits and TRPL_MCMC_FOLD apply", dict(flags=0x28)),
    (b"scale[1]=-1 must be finite and >= 0", dict(scale=KEEP[0].ctypes.data)),
    (b"group=1 must be >= 2", dict(group=1)),
    (b"P=9 must be a positive multiple of group=4", dict(P=9)),
    (b"count=12 must be <= P=8", dict(count=12)),
    (b"pairs=5 must be in [1, TRPL_MCMC_MAX_PAIRS = 4]", dict(pairs=5)),
    (b"ncr=9 must be in [1, TRPL_MCMC_MAX_CR = 8]", dict(ncr=9)),
    (b"pcr[1]=-0.1 must be finite and >= 0", dict(pcr=KEEP[1].ctypes.data)),
    (b"pcr: the sum 0 of the 3 shares must be > 0", dict(pcr=KEEP[3].ctypes.data)),
    (b"gamma_tab[1][1]=inf must be finite", dict(gamma_tab=KEEP[4].ctypes.data)),
    (b"e_width=1 must be in [0, 1)", dict(e_width=1.0)),
    (b"gamma_tab is NULL", dict(gamma_tab=None)),
    (b"mask is NULL", dict(mask=None)),
    (b"sel is NULL", dict(sel=None)),
    (b"ncol=17 must be in [1, 16]", dict(ncol=17)),
    (b"lo is NULL", dict(lo=None)),
    (b"hi is NULL", dict(hi=None)),
    (b"do_log is NULL", dict(do_log=None)),
    (b"column 0: log-uniform needs lo > 0", dict(do_log=KEEP[6].ctypes.data)),
    (b"column 2: lo must be <= hi", dict(hi=KEEP[5].ctypes.data)),
]


def _call(lib, suffix, a):
    fn = getattr(lib, "trpl_mcmc_propose_subspace" + suffix)
    return fn(*[a[k] for k in ARGS], *([None] if suffix else [0, None]))


def test_every_refusal_is_err_arg_with_no_device_present(trpl):
    A = trpl._abi
    lib = A.lib()

    def refused(word, **kw):
        for suffix in ("", "_dev"):
            assert _call(lib, suffix, dict(BASE, **kw)) == A.ERR_ARG, (word, suffix, kw)
            assert word in lib.trpl_last_error(), (word, suffix, lib.trpl_last_error())

    for word, kw in FAULTS:
        refused(word, **kw)
    for count in (-1, -(1 << 40)):
        refused(b"count=%d" % count, count=count)
    for n in (0, -1, 1000):
        refused(b"A=%d" % n, A=n)
    refused(b"A=2, but the box has 3 active", A=2)
    for P in (-1, -(1 << 40)):
        refused(b"P=%d" % P, P=P)
    for P, group in ((0, 4), (8, 3), (4, 8), (2, 4)):
        refused(b"P=%d must be a positive multiple of group=%d" % (P, group), P=P, group=group, count=1)
    for group in (0, -1, -(1 << 40)):
        refused(b"group=%d must be >= 2" % group, group=group)
    for g in (np.inf, -np.inf):
        refused(b"gamma=", gamma=g)
    refused(b"flags=0x8", flags=8)
    for pairs in (0, -1, 1 << 20):
        refused(b"pairs=%d" % pairs, pairs=pairs)
    for ncr in (0, -1, 1 << 20):
        refused(b"ncr=%d" % ncr, ncr=ncr)
    refused(b"pcr[1]=nan", pcr=KEEP[2].ctypes.data)
    refused(b"pcr[0]=inf", pcr=KEEP[7].ctypes.data)
    for e in (-0.1, -np.inf, 1.5, np.inf, np.nan):
        refused(b"e_width=", e_width=e)
    for bad in (np.nan, -np.inf):
        tab = np.full((2, 3), 0.7)
        tab[0, 2] = bad
        refused(b"gamma_tab[0][2]=", gamma_tab=tab.ctypes.data)
    # no refusal: these go as far as the device.  An entry of the table or of pcr beyond pairs, A or ncr is not read.
    tab1 = np.array([[0.7, 0.7, 0.7], [np.nan, np.nan, np.nan]])
    for kw in ({}, dict(pcr=None), dict(flags=A.MCMC_FOLD), dict(flags=A.MCMC_FOLD | 4), dict(group=2), dict(group=8), dict(count=3),
               dict(pairs=1, gamma_tab=tab1.ctypes.data), dict(pairs=4, gamma_tab=Z.ctypes.data), dict(ncr=1), dict(ncr=2, pcr=KEEP[7].ctypes.data + 8),
               dict(ncr=8, pcr=None), dict(e_width=0.0), dict(e_width=1.0 - 2.0 ** -53), dict(gamma=-2.0),
               dict(P=64, group=4, count=64, chain0=(1 << 32) + 5)):
        for suffix in ("", "_dev"):
            assert _call(lib, suffix, dict(BASE, **kw)) in (A.OK, A.ERR_NODEVICE, A.ERR_HIP), (kw, suffix, lib.trpl_last_error())


def test_which_of_two_refusals_wins(trpl):
    """Of two simultaneous faults the one earlier in FAULTS is reported: the refusals of trpl_mcmc_propose_rungs in its order, then the
    move's own in the order the header lists them, then the box's.  Both forms."""
    A = trpl._abi
    lib = A.lib()
    pairs = 0
    for (wa, ka), (wb, kb) in itertools.combinations(FAULTS, 2):
        if set(ka) & set(kb):
            continue
        pairs += 1
        for suffix in ("", "_dev"):
            assert _call(lib, suffix, dict(BASE, **ka, **kb)) == A.ERR_ARG, (wa, wb, suffix)
            assert wa in lib.trpl_last_error(), (wa, wb, suffix, lib.trpl_last_error())
    assert pairs > 450
