// What the posterior core's translation units share (posterior.hip, posterior_scan.hip): the launch geometry, the tempered
// weight expression and the fixed-order reductions.  A sum of the posterior core is defined by this file alone: sample i of S
// belongs to thread i % kThreads of block (i / kThreads) % grid_for(S); a thread adds its samples in rising order; a block
// adds its threads with block_reduce; final_reduce adds the blocks.  Two kernels that follow it produce the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace trpl {
namespace post {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;
constexpr int kMaxDim = 16;

__device__ __forceinline__ double wave_add(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
// block-wide sum / max of one value per thread (kThreads = 4 waves); result valid in thread 0
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double *sm)
{
    v = MAX ? wave_max(v) : wave_add(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[w] = v;
    __syncthreads();
    double r = sm[0];
#pragma unroll
    for (int i = 1; i < kThreads / 64; i++) r = MAX ? fmax(r, sm[i]) : r + sm[i];
    return r;
}

// the unnormalised weight of a sample with log-likelihood ll at temperature tf, m = nanmax(LL / tf), c_up = 1000 ln 2,
// c_size = ln S: utils.py:164, in its order of operations, with what that order rounds away put back.  The exponent u is the
// reference's fp64 one; at |ll / tf| ~ 1000 the quotient and the three sums each round by up to 5.7e-14, which is the weight's
// relative error.  The remainder of the division (one fma) and the rounding of each sum (two_sum) are exact in fp64, so
// w (1 + corr) carries the exponent to ~1e-19 and the weight to exp's own error.  The roundings of m, c_up and c_size
// themselves are common to all samples and leave with the division by the sum.  corr depends on the sample alone, and a
// weight that is 0, inf or NaN stays what it is (so does the smallest subnormal: exact_cut_margin holds as derived).
__device__ __forceinline__ double two_sum(double a, double b, double &err)
{
    const double s = a + b, bb = s - a;
    err = (a - (s - bb)) + (b - bb);
    return s;
}
__device__ __forceinline__ double tempered_weight(double ll, double tf, double m, double c_up, double c_size)
{
    const double q = ll / tf;
    double e0, e1, e2;
    const double u = two_sum(two_sum(two_sum(q, -m, e0), c_up, e1), -c_size, e2);
    const double corr = fma(-q, tf, ll) * __builtin_amdgcn_rcp(tf) + ((e0 + e1) + e2);      // ~1e-13: v_rcp_f64 is plenty
    const double w = exp(u);
    return fabs(corr) < 0x1p-30 ? fma(w, corr, w) : w;        // false for the NaN that an infinite q leaves in corr
}

// part is [gridDim.y][nb][ncol]; block (c, y) reduces column c of slab y over the nb block partials:
// thread t takes b = t, t + 256, ... in order, then the fixed block tree -- deterministic  (defined in posterior.hip)
__global__ void final_reduce(const double *part, int nb, int ncol, bool is_max, double *out);

inline int grid_for(int64_t S)
{
    int64_t nb = (S + kThreads - 1) / kThreads;
    return (int)(nb < 1 ? 1 : (nb > kMaxBlocks ? kMaxBlocks : nb));
}

}  // namespace post
}  // namespace trpl
