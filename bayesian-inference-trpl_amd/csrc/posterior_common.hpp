// What the posterior core's translation units share (posterior.hip, posterior_scan.hip): the launch geometry, the tempered
// weight expression, the two sample sources (with and without a proposal log-ratio) and the fixed-order reductions.  A sum of the posterior core is defined by this file alone: sample i of S
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

// the unnormalised weight of a sample whose exponent is e at temperature tf (e = ll / tf for log-likelihood ll alone),
// m = nanmax(e), c_up = 1000 ln 2, c_size = ln S: utils.py:164, in its order of operations, with what that order rounds away
// put back.  The exponent u is the reference's fp64 one; at |ll / tf| ~ 1000 the quotient and the three sums each round by up
// to 5.7e-14, which is the weight's relative error.  What the source of e dropped on the way (`lost`, see the sources below) and
// the rounding of each sum (two_sum) are exact in fp64, so w (1 + corr) carries the exponent to ~1e-19 and the weight to exp's
// own error.  The roundings of m, c_up and c_size themselves are common to all samples and leave with the division by the
// sum.  corr depends on the sample alone, and a weight that is 0, inf or NaN stays what it is (so does the smallest subnormal:
// exact_cut_margin holds as derived).  e = -inf (ll = -inf, or a ratio of +inf) gives exp(-inf) = 0 exactly, corr then being
// NaN; a NaN in the sample gives NaN.
__device__ __forceinline__ double two_sum(double a, double b, double &err)
{
    const double s = a + b, bb = s - a;
    err = (a - (s - bb)) + (b - bb);
    return s;
}
__device__ __forceinline__ double weight(double e, double lost, double m, double c_up, double c_size)
{
    double e0, e1, e2;
    const double u = two_sum(two_sum(two_sum(e, -m, e0), c_up, e1), -c_size, e2);
    const double corr = lost + ((e0 + e1) + e2);
    const double w = exp(u);
    return fabs(corr) < 0x1p-30 ? fma(w, corr, w) : w;        // false for the NaN that an infinite e leaves in corr
}

// Where a kernel's samples come from: the log-likelihood alone, or with a proposal log-ratio lnr beside it (a refined set,
// csrc/refine.hip, weights sample s by exp(LL[s] / tf) / r(u_s); folding ln r into LL would fix the temperature).  A source is
// passed to a kernel by value and chosen at compile time: a Plain kernel holds no pointer, load or register for lnr.
//   load(i)                  sample i
//   exponent(x, tf, lost)    e = ll / tf [- lnr] rounded to fp64, and in `lost` what its roundings dropped: the remainder of
//                            the division (one fma; ~1e-13 relative, so v_rcp_f64 is plenty) and, with a ratio, the error of
//                            the subtraction (two_sum), both exact.  lnr = +0.0 leaves e = ll / tf and adds +0.0 to lost (a
//                            lost of -0.0 may become +0.0, which fma(w, corr, w) does not see): the bits of Plain.
//   usable(x)                whether the sample counts (np.nanmax and np.nansum leave the others out)
struct Plain {
    const double *LL;
    __device__ __forceinline__ double load(int64_t i) const { return LL[i]; }
    // what the quotient q = ll / tf rounded away
    static __device__ __forceinline__ double remainder(double ll, double q, double tf) { return fma(-q, tf, ll) * __builtin_amdgcn_rcp(tf); }
    static __device__ __forceinline__ double exponent(double ll, double tf, double &lost)
    {
        const double q = ll / tf;
        lost = remainder(ll, q, tf);
        return q;
    }
    static __device__ __forceinline__ bool usable(double ll) { return ll == ll; }
};
struct Ratio {
    const double *LL, *lnr;
    struct Sample { double ll, r; };
    __device__ __forceinline__ Sample load(int64_t i) const { return {LL[i], lnr[i]}; }
    static __device__ __forceinline__ double exponent(Sample x, double tf, double &lost)
    {
        const double q = x.ll / tf;
        double el;
        const double e = two_sum(q, -x.r, el);
        lost = Plain::remainder(x.ll, q, tf) + el;
        return e;
    }
    static __device__ __forceinline__ bool usable(Sample x) { return x.ll == x.ll && x.r == x.r; }
};
// the weight of sample x of a source at temperature tf, m = nanmax of the source's exponent at tf
template <class Src, class Sample>
__device__ __forceinline__ double tempered_weight(Sample x, double tf, double m, double c_up, double c_size)
{
    double lost;
    const double e = Src::exponent(x, tf, lost);
    return weight(e, lost, m, c_up, c_size);
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
