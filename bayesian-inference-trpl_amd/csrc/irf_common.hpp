// How the instrument-response kernels (irf.hip, irf_bank.hip) read an input column of a PL row that may lie outside it: one
// definition of the two rules, so that "the bits of trpl_convolve_irf_dev" is the same text in both.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace trpl {

// every load is of a column of the row: no branch around it, and a column outside the row is never used
__device__ __forceinline__ int64_t clamp_col(int64_t c, int64_t ncol) { return c < 0 ? 0 : c < ncol ? c : ncol - 1; }

// what is staged for column c from the element v loaded at clamp_col(c, ncol): fp64, and 0.0 outside [0, ncol - 1]
template <typename T>
__device__ __forceinline__ double staged_value(T v, int64_t c, int64_t ncol) { return (c >= 0 && c < ncol) ? (double)v : 0.0; }

template <typename T>
__device__ __forceinline__ double staged_col(const T *__restrict__ prow, int64_t c, int64_t ncol)
{
    return staged_value<T>(prow[clamp_col(c, ncol)], c, ncol);
}

}  // namespace trpl
