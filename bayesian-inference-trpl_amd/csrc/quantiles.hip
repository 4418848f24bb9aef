// Weighted quantiles of many columns that share one weight vector (trpl_weighted_quantiles*, trpl_predictive_gather_dev;
// include/trpl.h): the credible intervals of the parameters (utils.py:185-196 for all columns in one call) and the
// quantile band of the posterior-predictive PL.
//
//   select_kernel<STAGE>  one workgroup of TRPL_Q_BLOCK threads per column.  Pass 0 looks at every row once: the used rows
//       (weight finite and > 0), their total weight sw, the smallest and the largest key as order-preserving 64-bit images,
//       a NaN among them.  Then bisection on the image: every pass compares each key with the pivots of all K requests and
//       forms the K cumulative weights S(pivot_k); at most 64 passes, fewer because the interval starts at [min, max].
//       A LAST_BELOW request ends with one more pass, the largest key below the point the bisection found.
//       Every cumulative weight is summed in ONE order, a pure function of n: thread t adds rows t, t + B, t + 2B, ... in
//       that order (an unselected row adds 0.0, which changes nothing), a shuffle-down tree over the 64 lanes, the waves in
//       wave order.  Adding non-negative terms in a fixed order is monotone in every term, so S is non-decreasing in the
//       pivot and the bisection is well defined; no atomics, nothing depends on scheduling.
//       STAGE = true (n <= kStageRows): images and weights are written to LDS in pass 0 and read from there;
//       STAGE = false: every pass streams keys and weights from global memory.  Same rows per thread, same order: same bits.
//   gather_kernel<T>      a resident PL block (rows, ld) -> the transposed store Y[i][row0 + j] = log_pl + mag[j] through a
//       64 x 64 LDS tile (one element per lane along a PL row, any odd ld; 64 consecutive doubles along a row of Y), and the
//       weights Wq[row0 + j] = W[j] for a used row, else 0.
// Compiled with the FAST contraction flag like predictive.hip: y is the band's y bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "log_pl.hpp"

namespace trpl {
namespace quant {

constexpr int kBlock = TRPL_Q_BLOCK;
constexpr int kWaves = kBlock / 64;
constexpr int kLdsPerCu = 160 * 1024;                            // MI355X
constexpr int kScratchBytes = 1024;                              // the reduction buffers below
// two workgroups per CU: 16 B per staged row (image + weight) and the reduction buffers in half the LDS
constexpr int kStageRows = (kLdsPerCu / 2 - kScratchBytes) / 16;
constexpr int kTile = 64;                                        // gather: rows x columns of one transposed tile

struct Requests {
    double q[TRPL_Q_MAX];
    int32_t rule[TRPL_Q_MAX];
};

// doubles that are not NaN -> unsigned integers in the same order; no number maps to 0 (that would be a NaN's bits)
__device__ __forceinline__ uint64_t image(double v)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double number(uint64_t u)
{
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

// row j as the passes see it: the weight (0 for an unused row) and the key's image (0 for an unused row, whose key is not read)
__device__ __forceinline__ void fetch(const double *y, const double *wq, int64_t j, uint64_t &u, double &w)
{
    const double wj = wq[j];
    const bool used = wj > 0.0 && wj < INFINITY;                 // a NaN fails the first test
    w = used ? wj : 0.0;
    u = 0;
    if (used) {
        double key = y[j];
        if (key == 0.0) key = 0.0;                               // -0.0 and +0.0 are one point
        u = image(key);
    }
}

__device__ __forceinline__ double lane_tree_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;                                                    // lane 0 holds the wave's sum
}
__device__ __forceinline__ uint64_t lane_tree_max(uint64_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = __shfl_down((unsigned long long)v, off);
        v = o > v ? o : v;
    }
    return v;
}

template <bool STAGE>
__global__ void __launch_bounds__(kBlock) select_kernel(const double *Y, int64_t n, int64_t ldy, const double *Wq, Requests rq, int K,
                                                        int64_t ncols, double *out)
{
    __shared__ uint64_t s_u[STAGE ? kStageRows : 1];
    __shared__ double s_w[STAGE ? kStageRows : 1];
    __shared__ double s_part[2][kWaves][TRPL_Q_MAX];             // wave partials, two buffers in turn: one barrier per pass
    __shared__ uint64_t s_ured[kWaves][TRPL_Q_MAX];
    static_assert(sizeof(double) * 2 * kWaves * TRPL_Q_MAX + sizeof(uint64_t) * kWaves * TRPL_Q_MAX <= kScratchBytes, "scratch");
    const int64_t c = blockIdx.x;
    const double *y = Y + c * ldy;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // ---- pass 0: used rows, sw, [min, max] of the images, a NaN key
    double a0 = 0.0;
    uint64_t nmin = 0, umax = 0;                                 // nmin = ~min: both are max-reductions
    uint64_t bad = 0;
    for (int64_t j = threadIdx.x; j < n; j += kBlock) {
        uint64_t u;
        double w;
        fetch(y, Wq, j, u, w);
        if (w > 0.0) {
            if (u > image(INFINITY) || u < image(-INFINITY)) bad = 1;        // the images of the NaNs lie outside the numbers'
            nmin = ~u > nmin ? ~u : nmin;
            umax = u > umax ? u : umax;
        }
        if (STAGE) { s_u[j] = u; s_w[j] = w; }
        a0 += w;
    }
    a0 = lane_tree_sum(a0);
    nmin = lane_tree_max(nmin); umax = lane_tree_max(umax); bad = lane_tree_max(bad);
    if (lane == 0) { s_part[0][wave][0] = a0; s_ured[wave][0] = nmin; s_ured[wave][1] = umax; s_ured[wave][2] = bad; }
    __syncthreads();
    double sw = s_part[0][0][0];
    nmin = s_ured[0][0]; umax = s_ured[0][1]; bad = s_ured[0][2];
#pragma unroll
    for (int w = 1; w < kWaves; w++) {
        sw += s_part[0][w][0];
        nmin = s_ured[w][0] > nmin ? s_ured[w][0] : nmin;
        umax = s_ured[w][1] > umax ? s_ured[w][1] : umax;
        bad |= s_ured[w][2];
    }
    if (bad || !(sw > 0.0 && sw < INFINITY)) {                   // a NaN key in a used row, no used row, or an overflowed sum
        if ((int)threadIdx.x < K) out[(int64_t)threadIdx.x * ncols + c] = NAN;
        return;
    }
    const uint64_t umin = ~nmin;

    // ---- bisection: lo[k] .. hi[k] holds the smallest image whose cumulative weight passes request k's test
    uint64_t lo[TRPL_Q_MAX], hi[TRPL_Q_MAX], piv[TRPL_Q_MAX];
    double t[TRPL_Q_MAX], acc[TRPL_Q_MAX];
    bool none[TRPL_Q_MAX];
#pragma unroll
    for (int k = 0; k < TRPL_Q_MAX; k++) {
        lo[k] = hi[k] = umin; t[k] = 0.0; none[k] = true; piv[k] = 0;
        if (k < K) {
            t[k] = rq.q[k] * sw;
            // FIRST_ABOVE looks for S > t; LAST_BELOW for the first point that is NOT below, S >= t, and takes the key before it
            none[k] = !(rq.rule[k] == TRPL_Q_LAST_BELOW ? sw >= t[k] : sw > t[k]);
            if (!none[k]) hi[k] = umax;
        }
    }
    int buf = 1;
    for (;;) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < TRPL_Q_MAX; k++) {
            any |= lo[k] < hi[k];
            piv[k] = lo[k] + ((hi[k] - lo[k]) >> 1);
            acc[k] = 0.0;
        }
        if (!any) break;                                         // the same in every thread: all read the same partials
        for (int64_t j = threadIdx.x; j < n; j += kBlock) {
            uint64_t u;
            double w;
            if (STAGE) { u = s_u[j]; w = s_w[j]; } else fetch(y, Wq, j, u, w);
#pragma unroll
            for (int k = 0; k < TRPL_Q_MAX; k++)
                if (k < K) acc[k] += u <= piv[k] ? w : 0.0;
        }
#pragma unroll
        for (int k = 0; k < TRPL_Q_MAX; k++)
            if (k < K) {
                acc[k] = lane_tree_sum(acc[k]);
                if (lane == 0) s_part[buf][wave][k] = acc[k];
            }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TRPL_Q_MAX; k++)
            if (k < K && lo[k] < hi[k]) {
                double S = s_part[buf][0][k];
#pragma unroll
                for (int w = 1; w < kWaves; w++) S += s_part[buf][w][k];
                if (rq.rule[k] == TRPL_Q_LAST_BELOW ? S >= t[k] : S > t[k]) hi[k] = piv[k];
                else lo[k] = piv[k] + 1;
            }
        buf ^= 1;
    }

    // ---- LAST_BELOW: the largest key below the point found (image 0: there is none)
    bool below = false;
#pragma unroll
    for (int k = 0; k < TRPL_Q_MAX; k++) below |= k < K && rq.rule[k] == TRPL_Q_LAST_BELOW;
    uint64_t prev[TRPL_Q_MAX];
#pragma unroll
    for (int k = 0; k < TRPL_Q_MAX; k++) prev[k] = 0;
    if (below) {
        for (int64_t j = threadIdx.x; j < n; j += kBlock) {
            uint64_t u;
            double w;
            if (STAGE) u = s_u[j]; else fetch(y, Wq, j, u, w);
#pragma unroll
            for (int k = 0; k < TRPL_Q_MAX; k++)
                if (k < K) prev[k] = (u < lo[k] && u > prev[k]) ? u : prev[k];
        }
        __syncthreads();                                         // pass 0's s_ured has been read by everyone
#pragma unroll
        for (int k = 0; k < TRPL_Q_MAX; k++)
            if (k < K) {
                prev[k] = lane_tree_max(prev[k]);
                if (lane == 0) s_ured[wave][k] = prev[k];
            }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TRPL_Q_MAX; k++)
            if (k < K) {
                prev[k] = s_ured[0][k];
#pragma unroll
                for (int w = 1; w < kWaves; w++) prev[k] = s_ured[w][k] > prev[k] ? s_ured[w][k] : prev[k];
            }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < TRPL_Q_MAX; k++)
            if (k < K) {
                double r = NAN;
                if (!none[k]) {
                    if (rq.rule[k] == TRPL_Q_LAST_BELOW) { if (prev[k]) r = number(prev[k]); }
                    else r = number(lo[k]);
                }
                out[(int64_t)k * ncols + c] = r;
            }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) gather_kernel(const T *pl, int64_t rows, int64_t ncol, int64_t ld, const double *mag,
                                                     const double *W, const int32_t *status, uint32_t flags, double *Y, int64_t ldy,
                                                     int64_t row0, double *Wq, int64_t col_tiles)
{
    __shared__ double tile[kTile][kTile + 1];                    // + 1: the transposed read walks a column without bank conflicts
    const int64_t ct = (int64_t)blockIdx.x % col_tiles, rt = (int64_t)blockIdx.x / col_tiles;
    const int64_t i0 = ct * kTile, j0 = rt * kTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool normalize = (flags & TRPL_FLAG_NORMALIZE) != 0, f32 = (flags & TRPL_FLAG_PL_F32) != 0 || sizeof(T) == 4;
    const int64_t i = i0 + lane;
    for (int r = wave; r < kTile; r += 4) {                      // a wave reads 64 consecutive columns of one PL row
        const int64_t j = j0 + r;
        if (j < rows && i < ncol) {
            const T *row = pl + j * ld;
            const T v = row[i], v0 = normalize ? row[0] : (T)1;
            tile[r][lane] = log_pl<T>(v, v0, normalize, f32) + (mag ? mag[j] : 0.0);
        }
    }
    __syncthreads();
    const int64_t jj = j0 + lane;
    for (int r = wave; r < kTile; r += 4) {                      // ... and writes 64 consecutive rows of one column of Y
        const int64_t ii = i0 + r;
        if (ii < ncol && jj < rows) Y[ii * ldy + row0 + jj] = tile[lane][r];
    }
    if (ct == 0 && wave == 0 && jj < rows) {
        const double w = W[jj];
        const bool used = w > 0.0 && w < INFINITY && (!status || status[jj] == 0);
        Wq[row0 + jj] = used ? w : 0.0;
    }
}

}  // namespace quant
}  // namespace trpl

using namespace trpl;

static const int64_t kMaxBlocks = 0x7fffffff;                    // gridDim.x

static int check_select(const void *Y, int64_t ncols, int64_t n, int64_t ldy, const void *Wq, const double *q, const int32_t *rule,
                        int32_t K, uint32_t flags, const void *out)
{
    if (ncols < 1 || ncols > kMaxBlocks) return api_fail(TRPL_ERR_ARG, "ncols=%lld must be in [1, 2^31 - 1]", (long long)ncols);
    if (n < 1) return api_fail(TRPL_ERR_ARG, "n=%lld must be >= 1", (long long)n);
    if (ldy < n) return api_fail(TRPL_ERR_ARG, "ldy=%lld must be >= n=%lld", (long long)ldy, (long long)n);
    if (K < 1 || K > TRPL_Q_MAX) return api_fail(TRPL_ERR_ARG, "K=%d must be in [1, TRPL_Q_MAX = %d]", K, TRPL_Q_MAX);
    if (!Y) return api_fail(TRPL_ERR_ARG, "Y is NULL");
    if (!Wq) return api_fail(TRPL_ERR_ARG, "Wq is NULL");
    if (!q) return api_fail(TRPL_ERR_ARG, "q is NULL");
    if (!rule) return api_fail(TRPL_ERR_ARG, "rule is NULL");
    if (!out) return api_fail(TRPL_ERR_ARG, "out is NULL");
    for (int k = 0; k < K; k++) {
        if (!(q[k] > 0.0 && q[k] < 1.0)) return api_fail(TRPL_ERR_ARG, "q[%d]=%g must lie in (0, 1)", k, q[k]);
        if (rule[k] != TRPL_Q_FIRST_ABOVE && rule[k] != TRPL_Q_LAST_BELOW)
            return api_fail(TRPL_ERR_ARG, "rule[%d]=%d is neither TRPL_Q_FIRST_ABOVE nor TRPL_Q_LAST_BELOW", k, rule[k]);
    }
    if (flags & ~(uint32_t)TRPL_Q_FORCE_STREAM)
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: only TRPL_Q_FORCE_STREAM applies to trpl_weighted_quantiles*", flags);
    return TRPL_OK;
}

extern "C" {

int64_t trpl_quantiles_stage_rows(void) { return quant::kStageRows; }

int trpl_weighted_quantiles_dev(const double *Y, int64_t ncols, int64_t n, int64_t ldy, const double *Wq, const double *q,
                                const int32_t *rule, int32_t K, uint32_t flags, double *out, void *stream)
{
    if (int rc = check_select(Y, ncols, n, ldy, Wq, q, rule, K, flags, out)) return rc;
    quant::Requests rq = {};
    for (int k = 0; k < K; k++) { rq.q[k] = q[k]; rq.rule[k] = rule[k]; }
    const bool stage = n <= quant::kStageRows && !(flags & TRPL_Q_FORCE_STREAM);
    hipStream_t st = (hipStream_t)stream;
    if (stage)
        hipLaunchKernelGGL(quant::select_kernel<true>, dim3((unsigned)ncols), dim3(quant::kBlock), 0, st, Y, n, ldy, Wq, rq, (int)K, ncols, out);
    else
        hipLaunchKernelGGL(quant::select_kernel<false>, dim3((unsigned)ncols), dim3(quant::kBlock), 0, st, Y, n, ldy, Wq, rq, (int)K, ncols, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "weighted quantiles launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_weighted_quantiles(const double *Y, int64_t ncols, int64_t n, int64_t ldy, const double *Wq, const double *q,
                            const int32_t *rule, int32_t K, uint32_t flags, double *out, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_select(Y, ncols, n, ldy, Wq, q, rule, K, flags, out)) return rc;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const double *dY = sg.in(Y, (size_t)(ncols - 1) * (size_t)ldy + (size_t)n), *dW = sg.in(Wq, (size_t)n);   // Y ends with its last column
    double *dOut = sg.out(out, (size_t)K * (size_t)ncols);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_weighted_quantiles_dev(dY, ncols, n, ldy, dW, q, rule, K, flags, dOut, sg.stream())) return rc;
    return sg.finish(seconds);
}

int trpl_predictive_gather_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *mag,
                               const double *W, const int32_t *status, uint32_t flags, double *Y, int64_t ldy, int64_t row0,
                               double *Wq, void *stream)
{
    if (rows < 1) return api_fail(TRPL_ERR_ARG, "rows=%lld must be >= 1", (long long)rows);
    if (ncol < 1) return api_fail(TRPL_ERR_ARG, "ncol=%lld must be >= 1", (long long)ncol);
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes=%d must be 4 or 8", elem_bytes);
    if (ld < ncol) return api_fail(TRPL_ERR_ARG, "ld=%lld must be >= ncol=%lld", (long long)ld, (long long)ncol);
    if (row0 < 0 || ldy < rows || row0 > ldy - rows)
        return api_fail(TRPL_ERR_ARG, "row0=%lld, rows=%lld: the block must lie inside a column of the store, ldy=%lld", (long long)row0,
                        (long long)rows, (long long)ldy);
    if (!plI) return api_fail(TRPL_ERR_ARG, "plI is NULL");
    if (!W) return api_fail(TRPL_ERR_ARG, "W is NULL");
    if (!Y) return api_fail(TRPL_ERR_ARG, "Y is NULL");
    if (!Wq) return api_fail(TRPL_ERR_ARG, "Wq is NULL");
    if (flags & ~(uint32_t)(TRPL_FLAG_PL_F32 | TRPL_FLAG_NORMALIZE))
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: only TRPL_FLAG_PL_F32 and TRPL_FLAG_NORMALIZE apply to trpl_predictive_gather_dev", flags);
    const int64_t col_tiles = (ncol + quant::kTile - 1) / quant::kTile, row_tiles = (rows + quant::kTile - 1) / quant::kTile;
    if (col_tiles > kMaxBlocks / row_tiles)
        return api_fail(TRPL_ERR_ARG, "rows=%lld x ncol=%lld is more than 2^31 - 1 tiles of 64 x 64", (long long)rows, (long long)ncol);
    const dim3 grid((unsigned)(col_tiles * row_tiles));
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4)
        hipLaunchKernelGGL(quant::gather_kernel<float>, grid, dim3(256), 0, st, (const float *)plI, rows, ncol, ld, mag, W, status, flags, Y,
                           ldy, row0, Wq, col_tiles);
    else
        hipLaunchKernelGGL(quant::gather_kernel<double>, grid, dim3(256), 0, st, (const double *)plI, rows, ncol, ld, mag, W, status, flags,
                           Y, ldy, row0, Wq, col_tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "predictive gather launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

}  // extern "C"
