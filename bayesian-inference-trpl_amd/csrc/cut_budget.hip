// trpl_loglik_cut_budget[_dev] (include/trpl.h): the level of one launch of curves from a sample's budget for its TOTAL squared error
// and what the curves before that launch reported.  One kernel, one thread per sample; trpl::loglik_dev (trpl_api.hip) launches it
// before every group of curves_per_launch curves, on the call's stream.  Built with -ffp-contract=off: every addition below is
// one rounding, in the order of reduce_curves_kernel (likelihood.hip), so R is minus what that kernel makes of a P that starts at
// zero from the same rows.  No atomics; plain vector loads and stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "trpl_common.hpp"

namespace trpl {
namespace budget {

// the next double above x, for x >= +0.0 or +inf (+inf stays): nextafter(x, +inf)
__device__ __forceinline__ double next_up(double x)
{
    return x == INFINITY ? x : __longlong_as_double(__double_as_longlong(x) + 1);
}

// THE RULE of include/trpl.h.  B: the sample's budget; R: the reported sse of its earlier curves, summed.  A level l that is
// returned finite and >= 0 has fl(R + l) >= B: a system cut at l reports sse > l, and adding non-negative terms is monotone.
__device__ __forceinline__ double level_of(double B, double R)
{
    if (B != B || R != R) return INFINITY;                 // NaN: never cut
    if (B == INFINITY) return INFINITY;
    if (R >= B) return -1.0;                               // already past its budget: the sink cuts after the first batch
    double l = fmax(B - R, 0.0);
    for (int k = 0; k < 3; k++) {                          // l0, its successor, and the successor of that
        if (R + l >= B) return l;
        l = next_up(l);
    }
    return INFINITY;
}

// budget [S]; sse [C][S], of which the rows 0 .. c0 - 1 are read; cut_level [C][S], of which the rows c0 .. c0 + g - 1 are written
__global__ void __launch_bounds__(256) level_kernel(const double *budget, const double *sse, double *cut_level, int64_t S, int c0, int g)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (int64_t)gridDim.x * blockDim.x) {
        double R = 0.0;
        for (int c = 0; c < c0; c++) R = R + sse[(int64_t)c * S + s];
        const double B = budget[s];
        const double l = c0 == 0 ? (B != B ? INFINITY : B) : level_of(B, R);      // launch 0 has nothing carried: the budget itself
        for (int c = c0; c < c0 + g; c++) cut_level[(int64_t)c * S + s] = l;
    }
}

}  // namespace budget

hipError_t launch_budget_level(const double *budget, const double *sse, double *cut_level, int64_t S, int c0, int g, hipStream_t stream)
{
    if (S <= 0 || g <= 0) return hipSuccess;
    int64_t blocks = (S + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(budget::level_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, budget, sse, cut_level, S, c0, g);
    return hipGetLastError();
}

}  // namespace trpl
