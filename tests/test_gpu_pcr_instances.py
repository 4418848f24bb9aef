"""Every instantiation of the stand-alone batched tridiagonal solve (csrc/pcr_batched_impl.hpp: 8 L x {fp64, fp32} x {STRICT,
FAST} = 32 kernels) and its launch boundaries (S around kPcrbGridCap, where a wave starts looping over systems and reuses its
LDS buffers) against the oracle and longdouble Thomas elimination (tests/highprec.py).

Bounds: fp64 STRICT is the oracle's bits; fp64 FAST is within 1e-13 max |x| of it; fp32 (both modes) is within 8 x the error of
a plain float32 Thomas solve of the exact (longdouble) solution of the float32-rounded system -- measured kernel / Thomas error
ratios per L are in DESIGN.md section 14."""
import numpy as np
import pytest

import highprec as hp
from highprec import LD

pytestmark = pytest.mark.gpu

GRID_CAP = 65536                  # kPcrbGridCap
_cases = {}


def case(oracle, L, S, seed):
    """The family's systems with their references, computed once per (L, S): oracle bits, longdouble Thomas, the fp32 case."""
    key = (L, S, seed)
    if key not in _cases:
        ops = hp.pcr_family(seed, S, L)
        ld, d, ud, b = ops
        orc = np.array([oracle.pcreduce(ld[s], d[s], ud[s], b[s]) for s in range(S)])
        f32, want32, plain32 = hp.fp32_case(*ops)
        for a in ops + (orc,) + tuple(f32):
            a.setflags(write=False)
        _cases[key] = dict(ops=ops, oracle=orc, f32=f32, want32=want32, plain32=plain32)
    return _cases[key]


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("L", hp.PCR_SIZES)
def test_every_instantiation_against_oracle_and_longdouble_thomas(gpu, oracle, L, dtype, mode):
    S = 67                                                  # more than one wave, odd, all systems distinct
    c = case(oracle, L, S, 100 + L)
    flags = gpu.FLAG_STRICT if mode == "strict" else 0
    ops = [np.array(a) for a in (c["ops"] if dtype == "fp64" else c["f32"])]
    keep = [a.copy() for a in ops]
    x = np.full_like(ops[1], np.nan)
    gpu._abi.check(gpu._abi.lib().trpl_pcr_solve_batched(*(a.ctypes.data for a in ops), x.ctypes.data, S, L, x.itemsize,
                                                         flags, 0, None))
    assert all(np.array_equal(a, k) for a, k in zip(ops, keep))                         # inputs untouched
    if dtype == "fp64":
        want = c["oracle"]
        err = float(np.max(np.abs(x - want)))
        print("L=%d fp64 %s: max err %.3e (max |x| %.3f)" % (L, mode, err, np.max(np.abs(want))))
        if mode == "strict":
            assert np.array_equal(x, want)
        else:
            assert err <= 1e-13 * np.max(np.abs(want))
    else:
        err, plain = float(np.max(np.abs(x.astype(LD) - c["want32"]))), float(c["plain32"].max())
        print("L=%d fp32 %s: kernel err %.3e, float32 Thomas err %.3e, ratio %.2f (bound 8; the old 2e-5 is %.0f x this error)"
              % (L, mode, err, plain, err / plain, 2e-5 / err))
        assert np.isfinite(x).all() and err <= 8 * plain


# L, dtype, mode: the two smallest LDS-staged shapes (row through LDS both ways), the widest direct FAST shape, and W < 64
BOUNDARY_SHAPES = [(256, "fp64", "fast"), (512, "fp32", "fast"), (128, "fp64", "fast"), (4, "fp64", "strict")]


@pytest.mark.parametrize("S", [1, GRID_CAP, GRID_CAP + 1, GRID_CAP + 193])
@pytest.mark.parametrize("L,dtype,mode", BOUNDARY_SHAPES)
def test_launch_boundaries_with_device_tiled_systems(gpu, oracle, L, dtype, mode, S):
    """U = 257 distinct systems tiled on the device by s % 257 (coprime to the grid cap: the two systems one wave solves always
    differ); x is a view between two sentinel rows."""
    import torch
    U = 257
    c = case(oracle, L, U, 900 + L)
    dev = torch.device("cuda")
    tdt = torch.float64 if dtype == "fp64" else torch.float32
    base = [torch.from_numpy(np.array(a)).to(dev) for a in (c["ops"] if dtype == "fp64" else c["f32"])]
    idx = torch.arange(S, device=dev) % U
    ops = [t.index_select(0, idx).contiguous() for t in base]
    sentinel = -777.25
    buf = torch.full((S + 2, L), sentinel, dtype=tdt, device=dev)
    x = buf[1:S + 1]
    assert x.is_contiguous() and x.data_ptr() == buf.data_ptr() + L * buf.element_size()
    gpu.device.pcr_solve_device(*ops, x, flags=gpu.FLAG_STRICT if mode == "strict" else 0)
    torch.cuda.synchronize()
    assert bool((buf[0] == sentinel).all()) and bool((buf[S + 1] == sentinel).all())       # nothing written outside x
    assert all(torch.equal(t, b.index_select(0, idx)) for t, b in zip(ops, base))         # inputs untouched
    if dtype == "fp64":
        want = torch.from_numpy(np.array(c["oracle"])).to(dev).index_select(0, idx)
        err = float((x - want).abs().max())
        print("L=%d fp64 %s S=%d: max err %.3e" % (L, mode, S, err))
        if mode == "strict":
            assert torch.equal(x, want)
        else:
            assert err <= 1e-13 * float(np.max(np.abs(c["oracle"][:min(S, U)])))
    else:
        # compared on the device in float64: the longdouble reference is rounded to it, and that rounding (2^-53 max |x|)
        # is taken off the bound
        w64 = c["want32"].astype(np.float64)
        want = torch.from_numpy(w64).to(dev).index_select(0, idx)
        err, plain = float((x.double() - want).abs().max()), float(c["plain32"][:min(S, U)].max())
        print("L=%d fp32 %s S=%d: max err %.3e, float32 Thomas err %.3e, ratio %.2f" % (L, mode, S, err, plain, err / plain))
        assert bool(torch.isfinite(x).all()) and err <= 8 * plain - 2.0 ** -53 * float(np.max(np.abs(w64)))
