// What the two refinement units share (refine.hip: axis-parallel boxes; refine_oriented.hip: boxes in whitened coordinates): the
// kernels' view of the parameter box, Philox4x32-10 with the genrand_res53 uniforms, the sampler's expressions that turn a unit
// coordinate into a column of X, and the host checks of the box.  One definition of each, so a child's X is the same function of
// its u in both draws.  Both units are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"

namespace trpl {
namespace refine {

constexpr int kThreads = 256;

struct Box {
    double lo[16], hi[16];     // bounds as sample_box receives them
    double l[16], lh[16];      // log10 of both for the log columns (host libm)
    int32_t do_log[16];
    int32_t act[16];           // active index -> column
    int32_t fixed[16];         // column -> 1: lo == hi, the value is lo
    int32_t ncol, A;
    uint32_t flags;            // TRPL_BOX_EQUAL_*
};

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ double res53(uint32_t x, uint32_t y)                  // genrand_res53, as csrc/sampler.hip forms it
{
    return ((double)(x >> 5) * 67108864.0 + (double)(y >> 6)) / 9007199254740992.0;
}

// ---- a row of X from unit coordinates, by the sampler's expressions: fixed columns copied, an active column c from its u, the
// overrides applied last
__device__ __forceinline__ void put_fixed(const Box &bx, double *row)
{
    for (int c = 0; c < bx.ncol; c++)
        if (bx.fixed[c]) row[c] = bx.lo[c];
}
__device__ __forceinline__ double column_value(const Box &bx, int c, double u)
{
    return bx.do_log[c] ? pow(10.0, bx.l[c] + (bx.lh[c] - bx.l[c]) * u) : bx.lo[c] + (bx.hi[c] - bx.lo[c]) * u;
}
__device__ __forceinline__ void put_overrides(const Box &bx, double *row)
{
    if ((bx.flags & TRPL_BOX_EQUAL_MU) && bx.ncol > 3) row[2] = row[3];
    if ((bx.flags & TRPL_BOX_EQUAL_S) && bx.ncol > 6) row[6] = row[5];
    if ((bx.flags & TRPL_BOX_EQUAL_AUGER) && bx.ncol > 8) row[8] = row[7];
}

}  // namespace refine

static const int64_t kRefineMaxBlocks = 0x7fffffff;              // gridDim.x

// the number of active dimensions A a kernel is instantiated for: switch (A) { TRPL_REFINE_DIMS(CASE) }
#define TRPL_REFINE_DIMS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

// the grid of one thread per item: blocks of kThreads over n, refused above gridDim.x ("S=.. is more than .. blocks of 256 samples")
static inline unsigned refine_blocks(int64_t n) { return (unsigned)((n + refine::kThreads - 1) / refine::kThreads); }
static inline int refine_check_blocks(const char *name, int64_t n, const char *items)
{
    if ((n + refine::kThreads - 1) / refine::kThreads > kRefineMaxBlocks)
        return api_fail(TRPL_ERR_ARG, "%s=%lld is more than 2^31 - 1 blocks of %d %s", name, (long long)n, refine::kThreads, items);
    return TRPL_OK;
}
// after the launches of a _dev form: TRPL_ERR_HIP "<what> launch: .." if one of them was refused
static inline int refine_launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRPL_OK : api_fail(TRPL_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
}

static inline int refine_check_counts(int64_t K, int32_t A)
{
    if (K < 1 || K > TRPL_REFINE_MAX_PARENTS)
        return api_fail(TRPL_ERR_ARG, "K=%lld must be in [1, TRPL_REFINE_MAX_PARENTS = %d]", (long long)K, TRPL_REFINE_MAX_PARENTS);
    if (A < 1 || A > TRPL_REFINE_MAX_DIMS) return api_fail(TRPL_ERR_ARG, "A=%d must be in [1, %d]", A, TRPL_REFINE_MAX_DIMS);
    return TRPL_OK;
}

// the number of children of a draw: m >= 0, n_uniform >= 0, n_uniform + K m at most 2^31 - 2
static inline int refine_check_children(int64_t K, int64_t m, int64_t n_uniform)
{
    if (m < 0) return api_fail(TRPL_ERR_ARG, "m=%lld must be >= 0", (long long)m);
    if (n_uniform < 0) return api_fail(TRPL_ERR_ARG, "n_uniform=%lld must be >= 0", (long long)n_uniform);
    if (m > (kRefineMaxBlocks - 1) / K || n_uniform > kRefineMaxBlocks - 1 - K * m)
        return api_fail(TRPL_ERR_ARG, "n_uniform=%lld + K * m = %lld * %lld is more than 2^31 - 2 children", (long long)n_uniform, (long long)K,
                        (long long)m);
    return TRPL_OK;
}

// the box as sample_box takes it -> the kernels' view; refuses a box whose number of active columns is not A
static inline int refine_make_box(int32_t ncol, const double *lo, const double *hi, const int32_t *do_log, uint32_t flags, int32_t A,
                                  refine::Box &bx)
{
    if (ncol < 1 || ncol > 16) return api_fail(TRPL_ERR_ARG, "ncol=%d must be in [1, 16]", ncol);
    if (!lo) return api_fail(TRPL_ERR_ARG, "lo is NULL");
    if (!hi) return api_fail(TRPL_ERR_ARG, "hi is NULL");
    if (!do_log) return api_fail(TRPL_ERR_ARG, "do_log is NULL");
    if (flags & ~(uint32_t)(TRPL_BOX_EQUAL_MU | TRPL_BOX_EQUAL_S | TRPL_BOX_EQUAL_AUGER))
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: only the TRPL_BOX_EQUAL_* bits apply", flags);
    bx = refine::Box();
    bx.ncol = ncol; bx.flags = flags;
    int n = 0;
    for (int c = 0; c < ncol; c++) {
        if (!(lo[c] <= hi[c])) return api_fail(TRPL_ERR_ARG, "column %d: lo must be <= hi", c);
        if (do_log[c] && lo[c] != hi[c] && !(lo[c] > 0)) return api_fail(TRPL_ERR_ARG, "column %d: log-uniform needs lo > 0", c);
        const bool target = (c == 2 && (flags & TRPL_BOX_EQUAL_MU) && ncol > 3) || (c == 6 && (flags & TRPL_BOX_EQUAL_S)) ||
                            (c == 8 && (flags & TRPL_BOX_EQUAL_AUGER));
        bx.lo[c] = lo[c]; bx.hi[c] = hi[c];
        bx.fixed[c] = lo[c] == hi[c];
        bx.do_log[c] = do_log[c] != 0 && !bx.fixed[c];
        if (bx.do_log[c]) { bx.l[c] = log10(lo[c]); bx.lh[c] = log10(hi[c]); }
        if (!bx.fixed[c] && !target) {
            if (n < 16) bx.act[n] = c;
            n++;
        }
    }
    if (n != A) return api_fail(TRPL_ERR_ARG, "A=%d, but the box has %d active columns", A, n);
    bx.A = A;
    return TRPL_OK;
}

}  // namespace trpl
