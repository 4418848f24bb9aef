// Posterior-predictive PL band (trpl_predictive*, include/trpl.h): per time column, the weighted mean, the weighted variance
// and the envelope of the model values  y[j][i] = log10 PL[j][i] + mag[j]  -- log_pl (log_pl.hpp), the values the resident-PL
// likelihood compares with the observations -- over the rows j whose posterior weight W[j] is finite and > 0 and whose solve
// was not flagged.  A streaming pass over a [rows][ncol] PL matrix in HBM with one log10 per element.
//
// Pass structure (no atomics, nothing depends on scheduling):
//   accumulate_partial  grid (column tiles, row chunks), 256 threads = 4 waves, ONE column per lane: a wave reads 64
//       consecutive columns of one row (256 / 512 contiguous bytes; rows are only element-aligned, ld = T/plT + 1 is usually
//       odd, so every lane loads one element).  A wave walks its chunk 64 rows at a time: lane l looks at W, status and mag
//       of row l (one coalesced load each), a ballot gives the used rows, and the wave visits ONLY those, kBatch at a time
//       -- the loads of a batch are issued together, then its log10s are evaluated -- taking each row's W and mag out of the
//       owning lane with a readlane.  An unused row costs 12 bytes of W / status, never a PL load.  Every lane keeps
//       (sw, mean, M2, lo, hi) of its column in registers, updated row after row (West's weighted one-pass update), and
//       writes them to part[chunk][5][ncol].
//   merge_chunks        one thread per column: the chunks' partials in chunk order by Chan's pairwise formula, then the
//       call's result into the running state [5][ncol].
//   finish              state -> out [5][ncol] = mean, var = M2 / sw, lo, hi, sw.
// The chunking (chunks()) is a pure function of (rows, ncol, elem_bytes): the same call gives the same bits on any device.
// Compiled with the FAST contraction flag (-ffp-contract=on).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "log_pl.hpp"

namespace trpl {
namespace pred {

constexpr int kTileCols = 256;        // columns per block: 4 waves x 64 lanes, one column per lane
constexpr int kMinChunkRows = 32;     // no chunk is cut shorter than this
constexpr int kMaxChunks = 64;        // bounds the workspace: kMaxChunks * ncol * 40 B
constexpr int kTargetBlocks = 4096;   // blocks wanted in the grid: 256 CUs x 8 resident 256-thread blocks, twice over
constexpr int kBatch = 8;             // used rows whose loads a wave keeps in flight
constexpr int kFields = 5;            // sw, mean, M2, lo, hi

// rows -> chunks; chunk k covers rows [k * chunk_rows, min((k + 1) * chunk_rows, rows)), chunk_rows = ceil(rows / chunks)
inline int chunks(int64_t rows, int64_t ncol, int elem_bytes)
{
    (void)elem_bytes;                                        // one column per lane for both element sizes
    const int64_t tiles = (ncol + kTileCols - 1) / kTileCols;
    int64_t want = (kTargetBlocks + tiles - 1) / tiles;
    const int64_t by_rows = (rows + kMinChunkRows - 1) / kMinChunkRows;
    if (want > by_rows) want = by_rows;
    if (want > kMaxChunks) want = kMaxChunks;
    if (want < 1) want = 1;
    const int64_t chunk_rows = (rows + want - 1) / want;
    return (int)((rows + chunk_rows - 1) / chunk_rows);      // no empty chunk
}

__device__ __forceinline__ double lane_value(double v, int src)          // v of lane `src` (wave-uniform), in every lane
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// (sw, mean, M2, lo, hi) of A <- A merged with B (Chan et al.); a side without weight passes the other through bit for bit
__device__ __forceinline__ void chan_merge(double &sw, double &mean, double &M2, double &lo, double &hi, double bsw, double bmean,
                                           double bM2, double blo, double bhi)
{
    if (bsw > 0.0) {
        if (!(sw > 0.0)) { sw = bsw; mean = bmean; M2 = bM2; }
        else {
            const double s = sw + bsw, d = bmean - mean;
            mean += d * (bsw / s);
            M2 += bM2 + (d * d) * ((sw * bsw) / s);
            sw = s;
        }
    }
    lo = fmin(lo, blo);
    hi = fmax(hi, bhi);
}

template <typename T>
__global__ void __launch_bounds__(kTileCols) accumulate_partial(const T *pl, int64_t rows, int64_t ncol, int64_t ld,
                                                                 const double *mag, const double *W, const int32_t *status,
                                                                 uint32_t flags, int64_t chunk_rows, double *part)
{
    const int lane = threadIdx.x & 63;
    const int64_t col = (int64_t)blockIdx.x * kTileCols + threadIdx.x;
    if (col - lane >= ncol) return;                            // a whole wave past the last column (wave-uniform)
    const int64_t c = col < ncol ? col : ncol - 1;             // lanes past the end alias the last column: loaded, never stored
    const bool normalize = (flags & TRPL_FLAG_NORMALIZE) != 0, f32 = (flags & TRPL_FLAG_PL_F32) != 0 || sizeof(T) == 4;
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    double sw = 0.0, mean = 0.0, M2 = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int64_t jb = r0; jb < r1; jb += 64) {
        const int64_t j = jb + lane;
        double w = 0.0, m = 0.0;
        bool used = false;
        if (j < r1) {
            w = W[j];
            used = w > 0.0 && w < INFINITY && (!status || status[j] == 0);       // NaN fails the first test
            if (used && mag) m = mag[j];
        }
        unsigned long long todo = __ballot(used);                                 // wave-uniform from here on
        while (todo) {
            int src[kBatch];
            bool on[kBatch];
            T v[kBatch], v0[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                on[k] = todo != 0;
                src[k] = on[k] ? __ffsll((long long)todo) - 1 : 0;
                todo &= todo - 1;                                                 // 0 stays 0
            }
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                v[k] = (T)1; v0[k] = (T)1;
                if (on[k]) {
                    const T *row = pl + (jb + src[k]) * ld;
                    v[k] = row[c];
                    if (normalize) v0[k] = row[0];
                }
            }
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                if (on[k]) {
                    const double wk = lane_value(w, src[k]), mk = lane_value(m, src[k]);
                    const double y = log_pl<T>(v[k], v0[k], normalize, f32) + mk;
                    // West (1979): T += R * SUMW * Q with R = Q * W / (SUMW + W) -- every term of M2 is a product of
                    // non-negative factors and d; the textbook (y - new mean) cancels once a heavy row follows light ones
                    const double s = sw + wk, d = y - mean, r = (wk / s) * d;
                    mean += r;
                    M2 += (r * sw) * d;
                    sw = s;
                    lo = fmin(lo, y);                                             // fmin / fmax skip a NaN
                    hi = fmax(hi, y);
                }
            }
        }
    }
    if (col < ncol) {
        double *p = part + (int64_t)blockIdx.y * kFields * ncol + col;
        p[0] = sw; p[ncol] = mean; p[2 * ncol] = M2; p[3 * ncol] = lo; p[4 * ncol] = hi;
    }
}

__global__ void __launch_bounds__(256) merge_chunks(const double *part, int nchunks, int64_t ncol, double *state)
{
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncol) return;
    double sw = 0.0, mean = 0.0, M2 = 0.0, lo = INFINITY, hi = -INFINITY;          // this call's rows, chunks in order
    for (int k = 0; k < nchunks; k++) {
        const double *p = part + (int64_t)k * kFields * ncol + col;
        chan_merge(sw, mean, M2, lo, hi, p[0], p[ncol], p[2 * ncol], p[3 * ncol], p[4 * ncol]);
    }
    double *q = state + col;
    double asw = q[0], amean = q[ncol], aM2 = q[2 * ncol], alo = q[3 * ncol], ahi = q[4 * ncol];
    chan_merge(asw, amean, aM2, alo, ahi, sw, mean, M2, lo, hi);
    q[0] = asw; q[ncol] = amean; q[2 * ncol] = aM2; q[3 * ncol] = alo; q[4 * ncol] = ahi;
}

__global__ void __launch_bounds__(256) init_state(double *state, int64_t ncol)
{
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncol) return;
    double *q = state + col;
    q[0] = 0.0; q[ncol] = 0.0; q[2 * ncol] = 0.0; q[3 * ncol] = INFINITY; q[4 * ncol] = -INFINITY;
}

// A y that is not finite in a used row (a NaN PL; PL <= 0 in a 4-byte buffer, whose clamp (float)DBL_MIN is 0: y = -inf)
// leaves M2 NaN or infinite whatever the row order (a finite y keeps it far below overflow), and the mean follows it:
// both NaN, by contract.
__global__ void __launch_bounds__(256) finish(const double *state, int64_t ncol, double *out)
{
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncol) return;
    const double *q = state + col;
    const double sw = q[0], M2 = q[2 * ncol];
    const bool ok = sw > 0.0 && M2 < INFINITY;                  // (a NaN fails the comparison)
    double *o = out + col;
    o[0] = ok ? q[ncol] : NAN;
    o[ncol] = ok ? M2 / sw : NAN;
    o[2 * ncol] = q[3 * ncol];
    o[3 * ncol] = q[4 * ncol];
    o[4 * ncol] = sw;
}

inline unsigned col_blocks(int64_t ncol) { return (unsigned)((ncol + 255) / 256); }

}  // namespace pred
}  // namespace trpl

using namespace trpl;

// column tiles ride in gridDim.x, whose limit is far above any ncol; chunks (<= kMaxChunks) in gridDim.y
static const int64_t kMaxNcol = (int64_t)1 << 36;

static int check_shape(int64_t rows, int64_t ncol, int32_t elem_bytes)
{
    if (rows < 1) return api_fail(TRPL_ERR_ARG, "rows=%lld must be >= 1", (long long)rows);
    if (ncol < 1 || ncol > kMaxNcol) return api_fail(TRPL_ERR_ARG, "ncol=%lld must be in [1, 2^36]", (long long)ncol);
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes=%d must be 4 or 8", elem_bytes);
    return TRPL_OK;
}

// what both forms of the accumulation refuse before a device is touched
static int check_accumulate(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const void *W,
                            uint32_t flags)
{
    if (int rc = check_shape(rows, ncol, elem_bytes)) return rc;
    if (ld < ncol) return api_fail(TRPL_ERR_ARG, "ld=%lld must be >= ncol=%lld", (long long)ld, (long long)ncol);
    if (!plI) return api_fail(TRPL_ERR_ARG, "plI is NULL");
    if (!W) return api_fail(TRPL_ERR_ARG, "W is NULL");
    if (flags & ~(uint32_t)(TRPL_FLAG_PL_F32 | TRPL_FLAG_NORMALIZE))
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: only TRPL_FLAG_PL_F32 and TRPL_FLAG_NORMALIZE apply to trpl_predictive*", flags);
    return TRPL_OK;
}

extern "C" {

int64_t trpl_predictive_state_bytes(int64_t ncol)
{
    if (ncol < 1 || ncol > kMaxNcol) return 0;
    return ncol * pred::kFields * (int64_t)sizeof(double);
}

int32_t trpl_predictive_chunks(int64_t rows, int64_t ncol, int32_t elem_bytes)
{
    if (rows < 1 || ncol < 1 || ncol > kMaxNcol || (elem_bytes != 4 && elem_bytes != 8)) return 0;
    return pred::chunks(rows, ncol, elem_bytes);
}

int64_t trpl_predictive_workspace_bytes(int64_t rows, int64_t ncol, int32_t elem_bytes)
{
    return (int64_t)trpl_predictive_chunks(rows, ncol, elem_bytes) * trpl_predictive_state_bytes(ncol);
}

int trpl_predictive_init_dev(void *state, int64_t ncol, void *stream)
{
    if (ncol < 1 || ncol > kMaxNcol) return api_fail(TRPL_ERR_ARG, "ncol=%lld must be in [1, 2^36]", (long long)ncol);
    if (!state) return api_fail(TRPL_ERR_ARG, "state is NULL");
    hipLaunchKernelGGL(pred::init_state, dim3(pred::col_blocks(ncol)), dim3(256), 0, (hipStream_t)stream, (double *)state, ncol);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "predictive init launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_predictive_accumulate_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *mag,
                                   const double *W, const int32_t *status, uint32_t flags, void *state, void *workspace,
                                   int64_t workspace_bytes, void *stream)
{
    if (int rc = check_accumulate(plI, elem_bytes, rows, ncol, ld, W, flags)) return rc;
    if (!state) return api_fail(TRPL_ERR_ARG, "state is NULL");
    if (!workspace) return api_fail(TRPL_ERR_ARG, "workspace is NULL");
    const int64_t need = trpl_predictive_workspace_bytes(rows, ncol, elem_bytes);
    if (workspace_bytes < need)
        return api_fail(TRPL_ERR_ARG, "workspace of %lld bytes is smaller than trpl_predictive_workspace_bytes(rows, ncol, elem_bytes) = %lld",
                        (long long)workspace_bytes, (long long)need);
    const int nch = pred::chunks(rows, ncol, elem_bytes);
    const int64_t chunk_rows = (rows + nch - 1) / nch;
    const dim3 grid((unsigned)((ncol + pred::kTileCols - 1) / pred::kTileCols), (unsigned)nch);
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4)
        hipLaunchKernelGGL(pred::accumulate_partial<float>, grid, dim3(pred::kTileCols), 0, st, (const float *)plI, rows, ncol, ld,
                           mag, W, status, flags, chunk_rows, (double *)workspace);
    else
        hipLaunchKernelGGL(pred::accumulate_partial<double>, grid, dim3(pred::kTileCols), 0, st, (const double *)plI, rows, ncol, ld,
                           mag, W, status, flags, chunk_rows, (double *)workspace);
    hipLaunchKernelGGL(pred::merge_chunks, dim3(pred::col_blocks(ncol)), dim3(256), 0, st, (const double *)workspace, nch, ncol,
                       (double *)state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "predictive accumulate launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_predictive_finish_dev(const void *state, int64_t ncol, double *out, void *stream)
{
    if (ncol < 1 || ncol > kMaxNcol) return api_fail(TRPL_ERR_ARG, "ncol=%lld must be in [1, 2^36]", (long long)ncol);
    if (!state) return api_fail(TRPL_ERR_ARG, "state is NULL");
    if (!out) return api_fail(TRPL_ERR_ARG, "out is NULL");
    hipLaunchKernelGGL(pred::finish, dim3(pred::col_blocks(ncol)), dim3(256), 0, (hipStream_t)stream, (const double *)state, ncol, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "predictive finish launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_predictive(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *mag, const double *W,
                    const int32_t *status, uint32_t flags, double *out, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_accumulate(plI, elem_bytes, rows, ncol, ld, W, flags)) return rc;
    if (!out) return api_fail(TRPL_ERR_ARG, "out is NULL");
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const size_t sb = (size_t)trpl_predictive_state_bytes(ncol), wsb = (size_t)trpl_predictive_workspace_bytes(rows, ncol, elem_bytes);
    const void *dPl = sg.in(plI, (size_t)rows * (size_t)ld * (size_t)elem_bytes);
    const double *dW = sg.in(W, (size_t)rows), *dMag = mag ? sg.in(mag, (size_t)rows) : nullptr;
    const int32_t *dSt = status ? sg.in(status, (size_t)rows) : nullptr;
    void *dState = sg.scratch(sb), *dWs = sg.scratch(wsb);
    double *dOut = (double *)sg.out((void *)out, sb);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_predictive_init_dev(dState, ncol, sg.stream())) return rc;
    if (int rc = trpl_predictive_accumulate_dev(dPl, elem_bytes, rows, ncol, ld, dMag, dW, dSt, flags, dState, dWs, (int64_t)wsb, sg.stream()))
        return rc;
    if (int rc = trpl_predictive_finish_dev(dState, ncol, dOut, sg.stream())) return rc;
    return sg.finish(seconds);
}

}  // extern "C"
