// What the kernels that score a row of PL against one set of observations do with log_pl's value (log_pl.hpp): the value between
// two grid points, the error and its two sums, and the finish of a row by a 256-thread workgroup.  One definition, shared by
// pl_loglik_kernel (likelihood.hip) and the bank kernel (irf_bank.hip), whose results are defined as the bits of the former's.
// Both units are compiled with -ffp-contract=off: one rounding per operation below.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace trpl {

// the model value at an observation dx past the lower of two grid points h apart, from the logs at the two: scipy interp1d's
// slope * (x - x_lo) + y_lo (bayeslib.py:184-191), the difference in float32 where the reference's buffer is float32
__device__ __forceinline__ double interp_log_pl(double lg_hi, double lg_lo, double h, double dx, bool f32)
{
    const double dy = f32 ? (double)((float)lg_hi - (float)lg_lo) : lg_hi - lg_lo;
    return (dy / h) * dx + lg_lo;
}

// one observation into a thread's sums (probs.py:33-41): s2 += err^2 and, with MOM, s1 += err; WT: both times the weight w
template <bool WT, bool MOM = true>
__device__ __forceinline__ void score_add(double y, double m, double ob, double w, double &s2, double &s1)
{
    static_assert(MOM || !WT, "the weighted form emits both sums");
    double err = y + m;
    err -= ob;
    if constexpr (WT) { s2 += (err * err) * w; s1 += err * w; }
    else {
        s2 += err * err;
        if constexpr (MOM) s1 += err;
    }
}

// v <- its sum over the 64 lanes of the wave, in every lane: the xor butterfly, widest exchange first
__device__ __forceinline__ void wave_add(double &v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
}

// a row's sum from the four wave sums of its workgroup
__device__ __forceinline__ double row_sum(const double *p) { return ((p[0] + p[1]) + p[2]) + p[3]; }

// a system flagged non-converged (its PL is NaN from that step on) scores +inf, like the fused path; so does a NaN sum
__device__ __forceinline__ void row_flag(bool flagged, double &r2, double &r1)
{
    if (flagged || !(r2 == r2)) { r2 = INFINITY; r1 = NAN; }
}

}  // namespace trpl
