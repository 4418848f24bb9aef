"""ctypes binding of libtrpl_hip.so (the C ABI declared in include/trpl.h).

The argument and return types of every entry point are read from the prototypes of include/trpl.h when this module is
imported (_parse_header): a new entry point is declared there and nowhere else.  The constants below restate the header's
#defines as literals; tests/test_abi.py holds them to it.

The library is built in-tree by `make -C bayesian-inference-trpl_amd` (or
`__graft_entry__.build()`).  There is NO fallback: if the shared object is missing or a call
fails, an exception is raised -- the product path never routes through the CPU oracle.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRPL_LIBRARY", os.path.join(_HERE, "libtrpl_hip.so"))   # override: A/B builds

# status codes / flags (include/trpl.h)
OK, ERR_ARG, ERR_HIP, ERR_NODEVICE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4
FLAG_STRICT, FLAG_PL_F32, FLAG_NORMALIZE, FLAG_FP32 = 0x1, 0x2, 0x4, 0x8
FLAG_KERNEL_PAIR, FLAG_KERNEL_SINGLE, FLAG_MIXED, FLAG_SNAP_RAW = 0x10, 0x20, 0x40, 0x80
FLAG_FP32_LONG, FP32_MAX_STEPS = 0x1000, 256
FLAG_HIST32 = 0x2000
FLAG_PAIR_ALWAYS_SEAM, FLAG_PAIR_ADJACENT, FLAG_MULTI_FORCE_PAD = 0x20000, 0x40000, 0x80000   # tests / measurements
FLAG_PREDICT = 0x100000    # opt-in: extrapolated start of every time step's iteration (include/trpl.h)
FLAG_MOMENTS = 0x200000    # set by trpl_loglik_moments[_dev] themselves (esum beside sse); trpl_kernel_name accepts it
FLAG_WEIGHTED = 0x400000   # set by trpl_loglik_weighted[_dev] themselves (sse, esum weighted per observation)
FLAG_CUT = 0x800000        # set by trpl_loglik_cut[_levels][_dev] themselves (a system stops once its running sse is above sse_cut / its cut_level)
MAG_PER_CURVE = 0x1        # trpl_mag_profile: one best offset per curve instead of one per sample
MAG_MAX_CURVES = 64        # TRPL_MAG_MAX_CURVES
MULTI_ALLOW_DUPLICATE_DEVICES = 0x1     # trpl_multi_create_ex


def flag_bdf_order(k):
    """TRPL_FLAG_BDF_ORDER(k): cap the BDF order ramp of pvSimPCR.py:241-250 at k = 1 .. 5 (None / 0: the reference's
    ramp); 2 is the scheme of Legacy/pvSim.py:94-97."""
    k = 0 if k is None else int(k)
    if not 0 <= k <= 5:
        raise ValueError("bdf_order must be None or 1 .. 5")
    return (k & 0x7) << 14


def fp32_flags(fp32):
    """fp32 = False | True (TRPL_FLAG_FP32: windows of up to FP32_MAX_STEPS steps) | "long" (+ TRPL_FLAG_FP32_LONG: any
    window, as a screening pass -- an fp32 state loses the decay over thousands of steps)."""
    if not fp32:
        return 0
    return FLAG_FP32 | (FLAG_FP32_LONG if fp32 == "long" else 0)
MAX_BUNDLE = 16                 # the flag's range; the library accepts bundle_cap(L) of it
PL_FLOOR_EXCESS = 1e-4          # TRPL_PL_FLOOR_EXCESS
PL_ENVELOPE_K_THICK = 5e-13     # TRPL_PL_ENVELOPE_K_THICK: |dPL / PL| <= 1e-9 + K / r on the 2000 nm films (L = 128)
PL_ENVELOPE_K_THIN = 1e-11      # TRPL_PL_ENVELOPE_K_THIN: the same on the 311 nm films
PL_ENVELOPE_K_L512 = 2e-12      # TRPL_PL_ENVELOPE_K_L512: the same on the 2000 nm film at L = 512


def bundle_cap(L):
    """Largest TRPL_FLAG_BUNDLE(m) at L nodes (one wavefront per system, one workgroup per bundle): 16 up to
    L = 64, 4 from L = 128 on (csrc/trpl_common.hpp)."""
    return 16 if int(L) <= 64 else 4


def flag_bundle(m, L=None):
    """TRPL_FLAG_BUNDLE(m): the reference's max_sims_per_block."""
    cap = MAX_BUNDLE if L is None else bundle_cap(L)
    if not 1 <= int(m) <= cap:
        raise ValueError("max_sims_per_block must be in [1, %d]%s" % (cap, "" if L is None else " at L = %d" % int(L)))
    return ((int(m) - 1) & 0xF) << 8

KERNEL_FAST, KERNEL_FAST_PAIR, KERNEL_STRICT, KERNEL_FP32, KERNEL_MIXED, KERNEL_HIST32 = 0, 1, 2, 3, 4, 5
ABI_VERSION = 5
MAX_SNAPS = 16
TF_SCAN_MAX = 64              # TRPL_TF_SCAN_MAX: temperatures of one trpl_posterior_tf_scan
Q_MAX, Q_BLOCK = 8, 256       # TRPL_Q_MAX: requests of one trpl_weighted_quantiles; TRPL_Q_BLOCK: threads that sum one column
Q_FIRST_ABOVE, Q_LAST_BELOW = 1, 2      # TRPL_Q_FIRST_ABOVE / TRPL_Q_LAST_BELOW: the two selection rules
Q_FORCE_STREAM = 0x1          # TRPL_Q_FORCE_STREAM (tests): the streamed kernel at any column length
# trpl_corner*: the primary columns of X, all column codes, the largest bin count; TRPL_COL_* in the order of the codes
CORNER_PRIMARY, CORNER_MAX_COLS, CORNER_MAX_BINS = 13, 19, 128
(COL_N0, COL_P0, COL_MU_N, COL_MU_P, COL_B, COL_SF, COL_SB, COL_CN, COL_CP, COL_TAU_N, COL_TAU_P, COL_LAMBDA, COL_MAG,
 COL_TAU_EFF, COL_TAU_RAD, COL_S_SUM, COL_MU_EFF, COL_EPSILON, COL_TAU_SUM) = range(19)
REFINE_MAX_DIMS, REFINE_MAX_PARENTS = 16, 1 << 20      # TRPL_REFINE_MAX_DIMS, TRPL_REFINE_MAX_PARENTS
MCMC_FOLD = 0x10              # TRPL_MCMC_FOLD: trpl_mcmc_propose reflects a proposal back at the faces of the unit cube
MCMC_MAX_RUNGS = 64           # TRPL_MCMC_MAX_RUNGS: temperatures of one trpl_mcmc_*_rungs / trpl_mcmc_swap call
MCMC_EVIDENCE_SUMS = 6        # TRPL_MCMC_EVIDENCE_SUMS: the columns of a row of trpl_mcmc_evidence_sums' sums
MCMC_MAX_PAIRS, MCMC_MAX_CR = 4, 8      # TRPL_MCMC_MAX_PAIRS, TRPL_MCMC_MAX_CR: difference pairs and crossover classes of trpl_mcmc_propose_subspace
IRF_MAX_TAPS = 1024           # TRPL_IRF_MAX_TAPS: taps of one trpl_convolve_irf (trpl_irf_max_taps())
IRF_TILE_COLS, IRF_TILE_ROWS, IRF_GRID_CAP = 512, 4, 65536      # TRPL_IRF_TILE_COLS / _ROWS: a workgroup's tile; TRPL_IRF_GRID_CAP: workgroups of a launch
IRF_BANK_MAX_RESPONSES, IRF_BANK_BLOCK = 256, 8      # TRPL_IRF_BANK_MAX_RESPONSES: responses of one trpl_loglik_irf_bank; TRPL_IRF_BANK_BLOCK: those of one pass over the taps
NUISANCE_MAX_OFFSETS = 64     # TRPL_NUISANCE_MAX_OFFSETS: magnitude offsets of one trpl_nuisance_reduce
NUISANCE_MAG_FIXED, NUISANCE_MAG_GRID, NUISANCE_MAG_PROFILE, NUISANCE_MARGINAL = 0x0, 0x1, 0x2, 0x10      # TRPL_NUISANCE_*: a mag mode | the marginal
SEED_MASK, STEP_MASK = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF      # a uint64_t seed and a uint32_t step of the trpl_mcmc_* calls, from any int


class TrplError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("trpl error %d: %s" % (code, msg))
        self.code = code


_HEADER = os.path.join(os.path.dirname(_HERE), "include", "trpl.h")
_pd = C.POINTER(C.c_double)
_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
_RETURNS = dict(_SCALARS, **{"int": C.c_int, "const char *": C.c_char_p})


def _parse_header(text):
    """name -> (restype, argtypes) of every trpl_* prototype in `text`, the contents of include/trpl.h.  A parameter with a
    `*` is a c_void_p, except `double *seconds`, a POINTER(c_double) (callers pass byref); any other is one of _SCALARS, a
    return type one of _RETURNS.  A spelling outside these raises ValueError: nothing is guessed."""
    import re
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    text = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("#"))
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s*]*?)\b(trpl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret, args = " ".join(ret.split()), " ".join(args.split())
        argtypes = []
        for a in ([] if args == "void" else args.split(", ")):
            kind = a.replace("const ", "").split(" ")[0]
            if "*" in a:
                argtypes.append(_pd if a == "double *seconds" else C.c_void_p)
            elif kind in _SCALARS:
                argtypes.append(_SCALARS[kind])
            else:
                raise ValueError("include/trpl.h: parameter %r of %s is of no type the binding knows" % (a, name))
        if ret not in _RETURNS:
            raise ValueError("include/trpl.h: return type %r of %s is none the binding knows" % (ret, name))
        out[name] = (_RETURNS[ret], argtypes)
    return out


# name -> argtypes and name -> restype, read from include/trpl.h at import: the header is the binding, there is no table to
# keep in step with it.  Without the header both are empty, and lib() refuses to load anything.
try:
    with open(_HEADER) as _fh:
        _protos = _parse_header(_fh.read())
except OSError:
    _protos = {}
SIGNATURES = {name: argtypes for name, (_, argtypes) in _protos.items()}
RESTYPES = {name: restype for name, (restype, _) in _protos.items()}

_lib = None


def source_hash():
    """sha256 of the concatenated sources the library is built from -- csrc/*.hip, csrc/*.hpp (byte order),
    include/trpl.h, the Makefile: the same bytes in the same order as the Makefile's SRCFILES rule hashes."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")))
    files += [_HEADER, os.path.join(_HERE, "Makefile")]
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def library_is_current():
    """True when libtrpl_hip.so exists and was built from the sources that are here now."""
    try:
        with open(LIB_PATH + ".srchash") as fh:
            return os.path.isfile(LIB_PATH) and fh.read().strip() == source_hash()
    except OSError:
        return False


def _build_if_stale():
    """A fresh checkout has no shared object (it is git-ignored), and a prebuilt one may predate an edit of
    csrc/ or include/: build the HIP library in-tree with the package Makefile when hipcc is present.  This
    is a build step, not a fallback -- the result is the same gfx950 library; set TRPL_AUTOBUILD=0 to forbid
    it.  `make` decides by file times; if the hash of the sources still differs from the one recorded at the
    last link (times not preserved by a copy), everything is rebuilt.

    Under torch.distributed.run every rank of a fresh checkout arrives here at once: the build is
    serialised with an exclusive lock file and re-checked under the lock, and the Makefile links under
    a temporary name and renames, so no rank ever loads a half-written library."""
    import fcntl
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.isfile("/opt/rocm/bin/hipcc") else None)
    if os.environ.get("TRPL_AUTOBUILD", "1") == "0" or hipcc is None or "TRPL_LIBRARY" in os.environ:
        return
    with open(os.path.join(_HERE, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            for force in ([], ["-B"]):
                if library_is_current():                           # another process may have built it meanwhile
                    break
                subprocess.check_call(["make", "-s", "-j4", "-C", _HERE, "all", "HIPCC=" + hipcc] + force)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def ensure_built():
    """Build the library if it is missing OR older than its sources (called when the package is imported, i.e.
    before anything in this process has touched the GPU)."""
    if not library_is_current():
        _build_if_stale()


def _share_torch_hip_runtime():
    """One HIP runtime per process.  A PyTorch-ROCm wheel bundles its own libamdhip64 / libhsa-runtime64 and
    loads them by path; if libtrpl_hip.so has pulled in /opt/rocm's copies first, a later `import torch` maps a
    SECOND runtime and torch.cuda reports no GPU (measured on this image, tools/load_order_probe.py).  So when
    torch is installed and not yet imported, its two runtime libraries are loaded first (without importing
    torch): libtrpl_hip.so's `NEEDED libamdhip64.so.7` then binds to them by soname, whichever of the two is
    imported first.  TRPL_HIP_RUNTIME=system skips this (pure-ctypes callers that never import torch)."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("TRPL_HIP_RUNTIME", "") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.isfile(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return
    # ... and the RCCL that was built against that runtime is the one trpl_multi_create binds (by path, at its
    # first call; nothing is loaded here)
    rccl = os.path.join(libdir, "librccl.so")
    if os.path.isfile(rccl):
        os.environ.setdefault("TRPL_RCCL_LIBRARY", rccl)


def lib():
    """Load libtrpl_hip.so once; raise loudly if it is absent and cannot be built.  The argument and return types of every
    entry point come from include/trpl.h, so a tree without that header raises ImportError here (it used to make only
    library_is_current() false)."""
    global _lib
    if _lib is None:
        if not SIGNATURES:
            raise ImportError("%s could not be read: the package needs include/trpl.h beside it (the ctypes binding is "
                              "derived from that header)" % _HEADER)
        if not os.path.isfile(LIB_PATH):
            _build_if_stale()
        if not os.path.isfile(LIB_PATH):
            raise ImportError("%s not found: build it with `make -C %s` (hipcc, gfx950); "
                              "there is no CPU fallback" % (LIB_PATH, _HERE))
        if "TRPL_LIBRARY" not in os.environ and not library_is_current():
            # no compiler here (or TRPL_AUTOBUILD=0): the binary could not be brought up to date -- say so, loudly
            import warnings
            warnings.warn("%s was built from other sources than the ones next to it (csrc/, include/trpl.h, Makefile) and "
                          "could not be rebuilt here: results are those of the OLD kernels; run `make -C %s`"
                          % (LIB_PATH, _HERE), RuntimeWarning, stacklevel=2)
        _share_torch_hip_runtime()
        dll = C.CDLL(LIB_PATH)
        dll.trpl_abi_version.restype = C.c_int
        # A/B tools compare an older build under the current binding (tools/compare_builds.py, tools/ab_multi.sh with
        # TRPL_LIBRARY=<old .so> TRPL_LIBRARY_ANY_ABI=1): entry points the old build lacks are then simply absent
        any_abi = "TRPL_LIBRARY" in os.environ and os.environ.get("TRPL_LIBRARY_ANY_ABI") == "1"
        if dll.trpl_abi_version() != ABI_VERSION and not any_abi:
            raise ImportError("%s has ABI version %d, this binding needs %d: rebuild it (`make -C %s`)"
                              % (LIB_PATH, dll.trpl_abi_version(), ABI_VERSION, _HERE))
        for name, argtypes in SIGNATURES.items():
            if any_abi and not hasattr(dll, name):
                continue
            fn = getattr(dll, name)
            fn.argtypes = argtypes
            fn.restype = RESTYPES[name]
        _lib = dll
    return _lib


def check(rc):
    if rc != OK:
        raise TrplError(rc, lib().trpl_last_error().decode("utf-8", "replace"))


def has_experimental():
    """True when the loaded library was built with `make EXPERIMENTAL=1` (TRPL_FLAG_MIXED / TRPL_FLAG_HIST32 steppers)."""
    return hasattr(lib(), "trpl_has_experimental") and bool(lib().trpl_has_experimental())


def kernel_flag(kernel):
    """TRPL_FLAG_KERNEL_* bit for kernel = None (library's choice) | "pair" | "single"."""
    if kernel is None:
        return 0
    try:
        return {"pair": FLAG_KERNEL_PAIR, "single": FLAG_KERNEL_SINGLE}[kernel]
    except KeyError:
        raise ValueError("kernel must be None, 'pair' or 'single', got %r" % (kernel,))


def kernel_name(nsys, L, steps, flags=0, snapshots=False):
    """trpl_kernel_name: the C++ name of the time-stepper kernel such a launch runs (what rocprofv3 lists after "void ")."""
    if not hasattr(lib(), "trpl_kernel_name"):          # an older build under TRPL_LIBRARY_ANY_ABI
        return "unknown"
    buf = C.create_string_buffer(256)
    check(lib().trpl_kernel_name(int(nsys), int(L), int(steps), int(flags), int(bool(snapshots)), C.addressof(buf), 256))
    return buf.value.decode()


def pin_variant(flags, nsys_total, L, steps):
    """`flags` with the stepper variant of a LOGICAL batch of nsys_total systems pinned, for callers that cut
    the batch into several launches (sample shards over ranks, blocks): every launch then runs the kernel the
    whole batch would, and a sample's bits do not depend on the cut (include/trpl.h, TRPL_FLAG_KERNEL_*)."""
    if flags & (FLAG_KERNEL_PAIR | FLAG_KERNEL_SINGLE):
        return flags
    v = lib().trpl_kernel_variant(int(nsys_total), int(L), int(steps), int(flags))
    return flags | {KERNEL_FAST_PAIR: FLAG_KERNEL_PAIR, KERNEL_FAST: FLAG_KERNEL_SINGLE}.get(v, 0)


def ptr(a):
    """Address of a numpy array / int device pointer / None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if isinstance(a, C.Array):
        return C.addressof(a)
    return int(a)
