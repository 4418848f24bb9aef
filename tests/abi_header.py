"""One reading of include/trpl.h and of the shared object's symbol table for the per-feature ABI tests, written independently of
the product's reader (trpl_amd._abi._parse_header is never used here): a count or a type asserted through this module checks that
reader.  Plain module, no fixtures; every function is computed once per process."""
import functools
import os
import re
import subprocess

from conftest import ROOT


@functools.lru_cache(maxsize=None)
def code():
    """The header's text without its /* */ comments."""
    with open(os.path.join(ROOT, "include", "trpl.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


@functools.lru_cache(maxsize=None)
def _prototypes():
    found = re.findall(r"^([a-z][\w \t*]*?)\b(trpl_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", code(), flags=re.M)
    return {name: (" ".join(ret.split()), [" ".join(p.split()) for p in args.split(",")]) for ret, name, args in found}


def names():
    return sorted(_prototypes())


def returns(name):
    """The return type of a prototype, as written but for white space."""
    return _prototypes()[name][0]


def params(name):
    """The parameter declarations of a prototype, as written but for white space; [] for (void)."""
    p = _prototypes()[name][1]
    return [] if p == ["void"] else list(p)


@functools.lru_cache(maxsize=None)
def defines():
    """TRPL_X -> number, for every #define whose body is one decimal, hex (either with a u suffix) or floating literal."""
    found = re.findall(r"^#define (TRPL_[A-Z0-9_]+)[ \t]+(0[xX][0-9a-fA-F]+|[0-9][0-9.]*(?:[eE][+-]?[0-9]+)?)u?[ \t]*$", code(), flags=re.M)
    return {name: int(v, 0) if re.fullmatch(r"0[xX][0-9a-fA-F]+|\d+", v) else float(v) for name, v in found}


@functools.lru_cache(maxsize=None)
def exports():
    """`nm -D --defined-only` of the library the package loads, as text."""
    import trpl_amd
    return subprocess.run(["nm", "-D", "--defined-only", trpl_amd._abi.LIB_PATH], capture_output=True, text=True, check=True).stdout


@functools.lru_cache(maxsize=None)
def demangled():
    """exports() through c++filt."""
    return subprocess.run(["c++filt"], input=exports(), capture_output=True, text=True, check=True).stdout
