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
// c_size = ln S: utils.py:164, in its order of operations
__device__ __forceinline__ double tempered_weight(double ll, double tf, double m, double c_up, double c_size)
{
    const double q = ll / tf;
    return exp(((q - m) + c_up) - c_size);
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
