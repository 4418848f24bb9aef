// Instrument-response convolution of a resident PL block (trpl_convolve_irf*, include/trpl.h): every row of pl [rows][ld],
// the output of trpl_solve_pl_dev, convolved with the K taps h of the detection chain's response, tap k0 at time zero:
//     out[r][j] = sum over k = 0 .. K-1, ascending, of  h[k] * (double)pl[r][j + k0 - k]          0 <= j < ncol - k0
// a term whose column j + k0 - k is negative is skipped.  fp64 accumulator from +0.0, one rounded product and one rounded
// addition per term (compiled with -ffp-contract=off), a 4-byte output is the fp64 sum rounded once: the bits of the NumPy loop
// over k, on every run and every device.  No atomics, no cross-lane sums: every output is one thread's own ordered sum.
//
// Tile structure.  A workgroup of kRows waves takes a tile of kRows rows x kTileCols output columns; wave w owns row w.
//   stage    the wave copies the kTileCols + K - 1 input columns its tile reads, j0 + k0 - (K - 1) .. j0 + k0 + kTileCols - 1,
//            into LDS as fp64, 64 consecutive columns per load (rows are only element-aligned: ld = T/plT + 1 is usually odd,
//            so every lane loads one element).  A column outside [0, ncol - 1] is staged as 0.0 (irf_common.hpp's clamp_col and
//            staged_value, which irf_bank.hip stages with too: here the kRun loads go first, then their LDS writes) and never enters a stored sum:
//            left of 0 the term is skipped by a test (tiles that touch column 0 run the EDGE instantiation of the tap loop),
//            right of ncol - 1 only outputs j >= ncol - k0 would read it, and those are not stored.  Each PL element is
//            fetched once per tile; the K - 1 columns two neighbouring tiles share come from L2 the second time.
//   taps     lane l produces the kRun consecutive outputs kRun * l .. kRun * l + kRun - 1 from a sliding window of kRun
//            registers: tap k multiplies the window by h[k] (a wave-uniform scalar load) and adds it to the kRun accumulators,
//            then the window moves one column left with ONE new LDS read.  The k loop is unrolled kRun times, so the move is a
//            renaming.  LDS index s is stored at s + s / kRun: the lanes of a wave read kRun + 1 doubles apart, which spreads a
//            32-lane group over all 64 banks (ds_read_b64, conflict-free).
//   store    the accumulators go back through the wave's LDS row, so that lane l stores columns l, l + 64, ...: 64
//            consecutive elements per store instruction.
// The grid is min(tiles, kGridCap) workgroups; a workgroup walks tiles blockIdx.x, + gridDim.x, ... -- column tiles of one
// row group first, so the tiles resident together share their halo columns.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "irf_common.hpp"

namespace trpl {
namespace irf {

constexpr int kRun = 8;                                // consecutive outputs per lane = the unroll of the tap loop
constexpr int kTileCols = kRun * 64;                   // output columns of a tile: one wave across
constexpr int kRows = TRPL_IRF_TILE_ROWS;              // rows of a tile = waves of a workgroup
constexpr int kThreads = kRows * 64;
constexpr int64_t kGridCap = TRPL_IRF_GRID_CAP;
static_assert(kTileCols == TRPL_IRF_TILE_COLS, "include/trpl.h states the tile");

__host__ __device__ constexpr int phys(int s) { return s + s / kRun; }         // s >= 0
// doubles of one wave's LDS row: local input column i sits at index i + kRun, i = -1 (the read after the last tap, never
// used) .. kTileCols + K - 2
__host__ __device__ constexpr int row_doubles(int K) { return phys(kTileCols + K - 2 + kRun) + 1; }
static_assert(kRows * row_doubles(TRPL_IRF_MAX_TAPS) * 8 <= 64 * 1024, "the staged tile fits the default dynamic LDS limit");
static_assert(row_doubles(1) >= phys(kTileCols - 1) + 1, "the store pass reuses the row");

// the kRun outputs of a lane.  s0: LDS index of the window's first element at tap 0; c0: the input column tap 0 of output 0
// reads (EDGE only: tap k of output v reads column c0 + v - k, skipped when negative)
template <bool EDGE>
__device__ __forceinline__ void taps(const double *xs, const double *__restrict__ h, int K, int s0, int c0, double (&acc)[kRun])
{
    double w[kRun];
#pragma unroll
    for (int v = 0; v < kRun; v++) { w[v] = xs[phys(s0 + v)]; acc[v] = 0.0; }
    auto tap = [&](int k) {
        const double hk = h[k];
#pragma unroll
        for (int v = 0; v < kRun; v++)
            if (!EDGE || c0 + v - k >= 0) acc[v] += hk * w[v];
#pragma unroll
        for (int v = kRun - 1; v > 0; v--) w[v] = w[v - 1];
        w[0] = xs[phys(s0 - k - 1)];
    };
    int k = 0;
    for (; k + kRun <= K; k += kRun) {
#pragma unroll
        for (int u = 0; u < kRun; u++) tap(k + u);
    }
    for (; k < K; k++) tap(k);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) convolve(const T *__restrict__ pl, int64_t rows, int64_t ncol, int64_t ld,
                                                     const double *__restrict__ h, int K, int k0, T *__restrict__ out,
                                                     int64_t out_ld, int64_t col_tiles, int64_t tiles)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *xs = lds + wave * row_doubles(K);
    const int64_t ncol_out = ncol - k0;
    const int n_in = kTileCols + K - 1;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t rg = t / col_tiles, j0 = (t - rg * col_tiles) * kTileCols;
        const int64_t row = rg * kRows + wave;
        const bool live = row < rows;                                   // wave-uniform
        const int64_t c_first = j0 + k0 - (K - 1);                      // input column of local column 0
        if (live) {
            const T *prow = pl + row * ld;
            for (int i0 = lane; i0 < n_in; i0 += 64 * kRun) {            // kRun loads in flight per lane, then their LDS writes
                T x[kRun];
#pragma unroll
                for (int u = 0; u < kRun; u++) {                          // every load is of a column of the row: no branch
                    const int64_t c = c_first + i0 + 64 * u;
                    x[u] = prow[clamp_col(c, ncol)];
                }
#pragma unroll
                for (int u = 0; u < kRun; u++) {
                    const int64_t c = c_first + i0 + 64 * u;
                    if (i0 + 64 * u < n_in) xs[phys(i0 + 64 * u + kRun)] = staged_value<T>(x[u], c, ncol);
                }
            }
            if (lane == 0) xs[phys(kRun - 1)] = 0.0;
        }
        __syncthreads();
        double acc[kRun];
        if (live) {
            const int s0 = kRun * lane + (K - 1) + kRun;
            if (c_first >= 0) taps<false>(xs, h, K, s0, 0, acc);
            else taps<true>(xs, h, K, s0, (int)j0 + kRun * lane + k0, acc);       // j0 < K - 1 here
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int v = 0; v < kRun; v++) xs[phys(kRun * lane + v)] = acc[v];
        }
        __syncthreads();
        if (live) {
            T *orow = out + row * out_ld;
#pragma unroll
            for (int m = 0; m < kRun; m++) {
                const int j = lane + 64 * m;
                if (j0 + j < ncol_out) orow[j0 + j] = (T)xs[phys(j)];
            }
        }
        __syncthreads();
    }
}

}  // namespace irf
}  // namespace trpl

using namespace trpl;

// what both forms refuse before a device is touched, in the order of include/trpl.h
static int check_convolve(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *h, int32_t K,
                          int32_t k0, const void *out, int64_t out_ld)
{
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes=%d must be 4 or 8", elem_bytes);
    if (rows < 0) return api_fail(TRPL_ERR_ARG, "rows=%lld must be >= 0", (long long)rows);
    if (ncol < 1) return api_fail(TRPL_ERR_ARG, "ncol=%lld must be >= 1", (long long)ncol);
    if (ld < ncol) return api_fail(TRPL_ERR_ARG, "ld=%lld must be >= ncol=%lld", (long long)ld, (long long)ncol);
    if (K < 1 || K > TRPL_IRF_MAX_TAPS) return api_fail(TRPL_ERR_ARG, "K=%d must be in [1, TRPL_IRF_MAX_TAPS = %d]", K, TRPL_IRF_MAX_TAPS);
    if (k0 < 0 || k0 > K - 1) return api_fail(TRPL_ERR_ARG, "k0=%d must be in [0, K - 1 = %d]", k0, K - 1);
    if (ncol - k0 < 1) return api_fail(TRPL_ERR_ARG, "ncol=%lld - k0=%d leaves no output column", (long long)ncol, k0);
    if (out_ld < ncol - k0)
        return api_fail(TRPL_ERR_ARG, "out_ld=%lld must be >= ncol - k0 = %lld", (long long)out_ld, (long long)(ncol - k0));
    if (rows > 0) {
        if (!pl) return api_fail(TRPL_ERR_ARG, "pl is NULL");
        if (!h) return api_fail(TRPL_ERR_ARG, "h is NULL");
        if (!out) return api_fail(TRPL_ERR_ARG, "out is NULL");
        if (out == pl) return api_fail(TRPL_ERR_ARG, "out must not be pl: the convolution is not in place");
    }
    return TRPL_OK;
}

extern "C" {

int trpl_irf_max_taps(void) { return TRPL_IRF_MAX_TAPS; }

int trpl_convolve_irf_dev(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *h, int32_t K,
                          int32_t k0, void *out, int64_t out_ld, void *stream)
{
    if (int rc = check_convolve(pl, elem_bytes, rows, ncol, ld, h, K, k0, out, out_ld)) return rc;
    if (rows == 0) return TRPL_OK;
    const int64_t col_tiles = (ncol - k0 + irf::kTileCols - 1) / irf::kTileCols, row_groups = (rows + irf::kRows - 1) / irf::kRows;
    if (col_tiles > INT64_MAX / row_groups)
        return api_fail(TRPL_ERR_ARG, "rows=%lld x ncol=%lld is more tiles than an int64 counts", (long long)rows, (long long)ncol);
    const int64_t tiles = col_tiles * row_groups;
    const dim3 grid((unsigned)(tiles < irf::kGridCap ? tiles : irf::kGridCap));
    const size_t lds = (size_t)irf::kRows * (size_t)irf::row_doubles(K) * sizeof(double);
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4)
        hipLaunchKernelGGL(irf::convolve<float>, grid, dim3(irf::kThreads), lds, st, (const float *)pl, rows, ncol, ld, h, (int)K, (int)k0,
                           (float *)out, out_ld, col_tiles, tiles);
    else
        hipLaunchKernelGGL(irf::convolve<double>, grid, dim3(irf::kThreads), lds, st, (const double *)pl, rows, ncol, ld, h, (int)K, (int)k0,
                           (double *)out, out_ld, col_tiles, tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "convolve_irf launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_convolve_irf(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *h, int32_t K, int32_t k0,
                      void *out, int64_t out_ld, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_convolve(pl, elem_bytes, rows, ncol, ld, h, K, k0, out, out_ld)) return rc;
    if (h)
        for (int k = 0; k < K; k++)
            if (!isfinite(h[k])) return api_fail(TRPL_ERR_ARG, "h[%d]=%g is not finite", k, h[k]);
    if (rows == 0) return TRPL_OK;
    const size_t eb = (size_t)elem_bytes, ncol_out = (size_t)(ncol - k0);
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const void *dPl = sg.in(pl, (size_t)ld * eb, (size_t)ncol * eb, (size_t)rows);          // compact on the device: ld = ncol
    const double *dH = sg.in(h, (size_t)K);
    void *dOut = sg.out(out, (size_t)out_ld * eb, ncol_out * eb, (size_t)rows);             // only ncol - k0 columns come back
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_convolve_irf_dev(dPl, elem_bytes, rows, ncol, ncol, dH, K, k0, dOut, (int64_t)ncol_out, sg.stream())) return rc;
    return sg.finish(seconds);
}

}  // extern "C"
