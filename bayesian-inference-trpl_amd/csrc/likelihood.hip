// Stand-alone likelihood kernels for the unfused (drop-in) path: log10 clamp (probs.py:64-75),
// squared-error accumulation (probs.py:20-47) and the curve-order reduction of the fused path.
// All three are HBM-bandwidth bound; arithmetic is fp64.
#include <float.h>
#include <math.h>

#include "log_pl.hpp"
#include "mag_moments.hpp"
#include "pl_score.hpp"
#include "trpl_common.hpp"

namespace trpl {

// x <- log10(max(x, mn)) in the buffer's dtype.  For float the clamp value is stored as
// (float)mn first -- 0.0f for mn = DBL_MIN, hence -inf -- exactly like an assignment into the
// reference's float32 array (probs.py:72-75).  The logarithm is evaluated in fp64 and rounded to
// the buffer's dtype (the CPU oracle's definition).
template <typename T>
__device__ __forceinline__ T log10_clamp_one(T v, double mn)
{
    if ((double)v < mn) v = (T)mn;
    return (T)log10((double)v);
}

// contiguous buffer (ld == cols): 16 bytes per lane per access, no index arithmetic
template <typename T>
__global__ void __launch_bounds__(256) log10_clamp_flat_kernel(T *x, int64_t n, double mn)
{
    constexpr int V = 16 / sizeof(T);
    struct alignas(16) Vec { T v[V]; };
    const int64_t nvec = n / V;
    Vec *xv = reinterpret_cast<Vec *>(x);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        Vec t = xv[i];
#pragma unroll
        for (int k = 0; k < V; k++) t.v[k] = log10_clamp_one<T>(t.v[k], mn);
        xv[i] = t;
    }
    const int64_t tail = nvec * V + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tail < n) x[tail] = log10_clamp_one<T>(x[tail], mn);      // n % V < V <= 4 elements, first lanes of block 0
}

// padded rows (ld > cols): rows over blockIdx.y, columns strided by the block
template <typename T>
__global__ void __launch_bounds__(256) log10_clamp_rows_kernel(T *x, int64_t rows, int64_t cols, int64_t ld, double mn)
{
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        T *row = x + r * ld;
        for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += (int64_t)gridDim.x * blockDim.x)
            row[c] = log10_clamp_one<T>(row[c], mn);
    }
}

template <typename T>
static hipError_t launch_log10_clamp_t(T *x, int64_t rows, int64_t cols, int64_t ld, double mn, hipStream_t stream)
{
    if (ld == cols && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const int64_t n = rows * cols;
        int64_t blocks = (n / (16 / sizeof(T)) + 255) / 256;
        blocks = blocks < 1 ? 1 : (blocks > 256 * 32 ? 256 * 32 : blocks);
        hipLaunchKernelGGL(log10_clamp_flat_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, x, n, mn);
    } else {
        const unsigned bx = (unsigned)((cols + 255) / 256 > 64 ? 64 : (cols + 255) / 256);
        const unsigned by = (unsigned)(rows > 8192 ? 8192 : rows);
        hipLaunchKernelGGL(log10_clamp_rows_kernel<T>, dim3(bx, by), dim3(256), 0, stream, x, rows, cols, ld, mn);
    }
    return hipGetLastError();
}

hipError_t launch_log10_clamp(void *x, int elem_bytes, int64_t rows, int64_t cols, int64_t ld, double mn,
                              hipStream_t stream)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    return elem_bytes == 4 ? launch_log10_clamp_t<float>((float *)x, rows, cols, ld, mn, stream)
                           : launch_log10_clamp_t<double>((double *)x, rows, cols, ld, mn, stream);
}

// P[j] -= sum_i (pl[j][i] + mag[j] - values[i])^2, accumulated in index order in fp64 so the
// result is bit-identical to the reference's serial loop (probs.py:32-44).  The serial chain of
// n_obs dependent fp64 adds per row is the floor of this formulation (~0.2 ms at 80 001 columns);
// everything else is arranged around it: a wavefront owns R rows (R small when there are few
// rows, so that the chip is covered with workgroups), loads [R rows x 64 columns] tiles with the
// lanes along the columns (256/512-byte contiguous segments), squares the residuals in parallel,
// transposes through LDS, and lanes 0..R-1 add their row's 64 values in order while the loads of
// the next tile are already in flight.
// W (trpl_sse_accumulate_w): every squared residual times its column's weight, (e * e) * w[i] -- the weighting line of
// kernel_lnP (probs.py:40) with w = 1 / (2 u^2) formed by the caller -- in its own instantiations, same serial order;
// the W = false kernels are the code they were before.
template <typename T, int R, bool W = false>
__global__ void __launch_bounds__(64) sse_accumulate_kernel(double *P, const T *pl, int64_t rows, int64_t n_obs,
                                                            int64_t ld, const double *values, const double *mag,
                                                            const double *wts = nullptr)
{
    __shared__ double tile[R][65];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    double mg[R];
    const T *rowp[R];
#pragma unroll
    for (int r = 0; r < R; r++) {                 // rows past the end alias the last row: loaded, never stored
        const int64_t rr = row0 + r < rows ? row0 + r : rows - 1;
        mg[r] = mag[rr];
        rowp[r] = pl + rr * ld;
    }
    // D tiles of loads stay in flight per wave: a ring of RAW register tiles, statically indexed.
    // Loads are unconditional (column index clamped) and nothing depends on them until the slot is
    // consumed D tiles later, so the compiler can keep them outstanding (a bounds branch around
    // load+arithmetic made it wait for every single load: 0.1 % of HBM peak).
    constexpr int D = 32 / R;
    T raw[D][R];
    double vraw[D], wraw[W ? D : 1];
    auto issue = [&](int64_t c0, T (&v)[R], double &val, double &wt) {
        int64_t col = c0 + lane;
        col = col < n_obs ? col : n_obs - 1;
        val = values[col];
        if constexpr (W) wt = wts[col];
#pragma unroll
        for (int r = 0; r < R; r++) v[r] = rowp[r][col];
    };
    double acc = 0.0;
    if (n_obs > 0) {
#pragma unroll
        for (int d = 0; d < D; d++) issue((int64_t)d * 64, raw[d], vraw[d], wraw[W ? d : 0]);
    }
    for (int64_t c0 = 0; c0 < n_obs; c0 += 64 * D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const int64_t cc = c0 + (int64_t)d * 64;
            if (cc >= n_obs) break;                                // wave-uniform
#pragma unroll
            for (int r = 0; r < R; r++) {
                double e = (double)raw[d][r] + mg[r];              // probs.py:33
                e -= vraw[d];                                      // :37
                if constexpr (W) tile[r][lane] = (e * e) * wraw[d];   // :39, :40
                else tile[r][lane] = e * e;                        // :39
            }
            issue(cc + 64 * D, raw[d], vraw[d], wraw[W ? d : 0]);                   // refill this slot D tiles ahead
            const int ncol = (int)((n_obs - cc) < 64 ? (n_obs - cc) : 64);
            if (lane < R) {
                const double *t = tile[lane];
                if (ncol == 64) {
#pragma unroll 16
                    for (int k = 0; k < 64; k++) acc += t[k];      // :41, in index order
                } else {
                    for (int k = 0; k < ncol; k++) acc += t[k];    // columns >= n_obs are never read
                }
            }
        }
    }
    if (lane < R && row0 + lane < rows) P[row0 + lane] += (0.0 - acc);   // :44, :57-60
}

template <typename T, bool W = false>
static hipError_t launch_sse_t(double *P, const T *pl, int64_t rows, int64_t n_obs, int64_t ld, const double *values,
                               const double *mag, hipStream_t stream, const double *wts = nullptr)
{
#define TRPL_SSE(RR)                                                                                              \
    hipLaunchKernelGGL((sse_accumulate_kernel<T, RR, W>), dim3((unsigned)((rows + RR - 1) / RR)), dim3(64), 0, stream, \
                       P, pl, rows, n_obs, ld, values, mag, wts)
    if (rows <= 4 * 1024) TRPL_SSE(4);               // >= rows/4 workgroups: cover the 256 CUs
    else if (rows <= 16 * 1024) TRPL_SSE(8);
    else TRPL_SSE(16);
#undef TRPL_SSE
    return hipGetLastError();
}

hipError_t launch_sse_accumulate(double *P, const void *pl, int elem_bytes, int64_t rows, int64_t n_obs,
                                 int64_t ld, const double *values, const double *mag, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    return elem_bytes == 4 ? launch_sse_t<float>(P, (const float *)pl, rows, n_obs, ld, values, mag, stream)
                           : launch_sse_t<double>(P, (const double *)pl, rows, n_obs, ld, values, mag, stream);
}

hipError_t launch_sse_accumulate_w(double *P, const void *pl, int elem_bytes, int64_t rows, int64_t n_obs, int64_t ld,
                                   const double *values, const double *wts, const double *mag, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    return elem_bytes == 4 ? launch_sse_t<float, true>(P, (const float *)pl, rows, n_obs, ld, values, mag, stream, wts)
                           : launch_sse_t<double, true>(P, (const double *)pl, rows, n_obs, ld, values, mag, stream, wts);
}

// P[s] -= sse[c][s] for c = 0..C-1 in curve order (the order bayeslib.simulate calls prob in,
// bayeslib.py:117,:195).
__global__ void __launch_bounds__(256) reduce_curves_kernel(double *P, const double *sse, int64_t S, int C)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (int64_t)gridDim.x * blockDim.x) {
        double p = P[s];
        for (int c = 0; c < C; c++) p += (0.0 - sse[(int64_t)c * S + s]);
        P[s] = p;
    }
}

hipError_t launch_reduce_curves(double *P, const double *sse, int64_t S, int C, hipStream_t stream)
{
    if (S <= 0) return hipSuccess;
    int64_t blocks = (S + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(reduce_curves_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, P, sse, S, C);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Likelihood of PL rows that are already in HBM (the output of trpl_solve_pl_dev) against one set of
// observations, in ONE pass: re-dimensionalised PL -> optional self-normalisation -> clamp -> log10
// (bayeslib.py:150-157) -> observations on the grid or linearly interpolated between the bracketing
// grid points (bayeslib.py:184-191) -> squared error (probs.py:29-44).  This is what lets one solve
// serve several experiments (the reference's loop order curves -> blocks -> experiments) without the
// PL matrix ever crossing PCIe.  One 256-thread block per row (the reference's 1024-row blocks would
// otherwise leave most of the chip idle behind the fp64 log10), threads stride over the observations,
// fixed-order block reduction at the end: the sum is associated differently from probs.prob's serial loop (~1e-16);
// trpl_log10_clamp + trpl_sse_accumulate remain the bit-exact pair.  HBM-bound: n_obs (or 2 n_obs,
// off-grid) PL elements per row.  log_pl (log_pl.hpp) forms the model value; the predictive band shares it.  What follows it --
// the interpolation, the error and its sums, the finish of a row -- is pl_score.hpp, which the bank kernel (irf_bank.hip) shares.
// ---------------------------------------------------------------------------------------------

// MOM (trpl_loglik_moments_from_pl_dev): the sum of the errors beside the sum of their squares, in its own instantiation --
// the MOM = false kernels are the code they were before the moments existed
// WT (trpl_loglik_weighted_from_pl_dev; implies MOM): every term times its observation's weight, (err * err) * w and err * w
template <typename T, bool MOM, bool WT = false>
__global__ void __launch_bounds__(256) pl_loglik_kernel(const T *pl, int64_t rows, int64_t ld, const double *obs,
                                                        const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                                                        int64_t n_obs, const double *mag, const int32_t *status,
                                                        double *P, double *sse_out, uint32_t flags, double *esum_out,
                                                        const double *wts = nullptr)
{
    static_assert(MOM || !WT, "the weighted form emits both sums");
    __shared__ double part[4], part1[MOM ? 4 : 1];
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x;
    const T *r = pl + row * ld;
    const bool normalize = (flags & 0x4u) != 0, f32 = (flags & 0x2u) != 0 || sizeof(T) == 4;
    const T v0 = r[0];
    const double m = mag[row];
    double acc = 0.0, acc1 = 0.0;                // acc1: sum of the errors (esum_out, trpl_loglik_moments_from_pl_dev)
    for (int64_t i = threadIdx.x; i < n_obs; i += 256) {
        double y;
        if (obs_hi) {
            const int64_t hi = obs_hi[i];
            y = interp_log_pl(log_pl<T>(r[hi], v0, normalize, f32), log_pl<T>(r[hi - 1], v0, normalize, f32), obs_h[i], obs_dx[i], f32);
        } else {
            y = log_pl<T>(r[i], v0, normalize, f32);
        }
        double w = 1.0;
        if constexpr (WT) w = wts[i];
        score_add<WT, MOM>(y, m, obs[i], w, acc, acc1);
    }
    wave_add(acc);
    if constexpr (MOM) wave_add(acc1);
    if (lane == 0) { part[threadIdx.x >> 6] = acc; if constexpr (MOM) part1[threadIdx.x >> 6] = acc1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        acc = row_sum(part);
        if constexpr (MOM) acc1 = row_sum(part1);
        row_flag(status && status[row] != 0, acc, acc1);
        if constexpr (MOM) { if (esum_out) esum_out[row] = acc1; }
        if (sse_out) sse_out[row] = acc;
        if (P) P[row] -= acc;                                   // probs.py:44,:60
    }
}

hipError_t launch_pl_loglik(const void *pl, int elem_bytes, int64_t rows, int64_t ld, const double *obs,
                            const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t n_obs,
                            const double *mag, const int32_t *status, double *P, double *sse_out, uint32_t flags,
                            hipStream_t stream, double *esum_out, const double *wts)
{
    if (rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)rows), block(256);
    if (wts) {                                       // trpl_loglik_weighted_from_pl_dev: both sums, weighted
        if (elem_bytes == 4)
            hipLaunchKernelGGL((pl_loglik_kernel<float, true, true>), grid, block, 0, stream, (const float *)pl, rows, ld, obs,
                               obs_hi, obs_dx, obs_h, n_obs, mag, status, P, sse_out, flags, esum_out, wts);
        else
            hipLaunchKernelGGL((pl_loglik_kernel<double, true, true>), grid, block, 0, stream, (const double *)pl, rows, ld, obs,
                               obs_hi, obs_dx, obs_h, n_obs, mag, status, P, sse_out, flags, esum_out, wts);
        return hipGetLastError();
    }
#define TRPL_PLL(TT, MM)                                                                                                  \
    hipLaunchKernelGGL((pl_loglik_kernel<TT, MM>), grid, block, 0, stream, (const TT *)pl, rows, ld, obs, obs_hi, obs_dx, obs_h, \
                       n_obs, mag, status, P, sse_out, flags, esum_out)
    if (elem_bytes == 4) { if (esum_out) TRPL_PLL(float, true); else TRPL_PLL(float, false); }
    else                 { if (esum_out) TRPL_PLL(double, true); else TRPL_PLL(double, false); }
#undef TRPL_PLL
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The mag_grid loop of the reference's older likelihood (probs.lnP, probs.py:5-18) from the two moments the
// TRPL_FLAG_MOMENTS steppers emit: sum_i (e_i + d)^2 = sse + 2 d esum + n d^2.  mag_term, the ordered curve sum and the
// shared-offset profile are mag_moments.hpp, ONE expression each, compiled for the host and for the device in this translation
// unit (-ffp-contract=off: no fused multiply-add on either side, IEEE divide), so that the plain host forms and the kernels agree
// bit for bit; trpl_nuisance_reduce* (nuisance.hip) shares them.
// ---------------------------------------------------------------------------------------------

// P[m][s] -= sum_c mag_term(.., offsets[m]), curves in order
__host__ __device__ inline void mag_grid_one(const double *sse, const double *esum, const double *n, int64_t S, int C, int64_t s,
                                             double d, double *P)
{
    *P = *P - mag_curve_sum(sse + s, esum + s, n, S, C, d);
}

__host__ __device__ inline void mag_profile_one(const double *sse, const double *esum, const double *n, int64_t S, int C, int64_t s,
                                                bool per_curve, double *best, double *P)
{
    double acc = 0.0;
    if (per_curve) {                             // an offset of its own per curve: no sum at one d to share
        for (int c = 0; c < C; c++) {
            const double e = esum[(int64_t)c * S + s];
            // a curve whose weights are all zero (trpl_mag_profile_w; n_obs >= 1 never gets here) has no observation:
            // no best offset, and it contributes nothing
            if (n[c] == 0.0 && sse[(int64_t)c * S + s] < INFINITY) { best[(int64_t)c * S + s] = NAN; continue; }
            const double d = (0.0 - e) / n[c];
            best[(int64_t)c * S + s] = (e - e == 0.0 && sse[(int64_t)c * S + s] < INFINITY) ? d : NAN;
            acc += mag_term(sse[(int64_t)c * S + s], e, n[c], d);
        }
    } else {
        const MagShared p = mag_shared_offset(sse + s, esum + s, n, S, C);
        if (p.empty) { best[s] = NAN; return; }                       // every weight zero: nothing to fit, P stays
        best[s] = p.best;
        acc = mag_curve_sum(sse + s, esum + s, n, S, C, p.d);
    }
    *P = *P - acc;
}

// The quadratic coefficient of a curve is a double everywhere below: (double)n_obs[c] for the unweighted calls, wsum[c] =
// sum_i w_ci for the weighted ones (trpl_mag_grid_w, trpl_mag_profile_w) -- one expression for both.
void mag_grid_host_w(const double *sse, const double *esum, const double *wsum, int64_t S, int C, const double *offsets,
                     int64_t M, double *P)
{
    for (int64_t m = 0; m < M; m++)
        for (int64_t s = 0; s < S; s++) mag_grid_one(sse, esum, wsum, S, C, s, offsets[m], P + m * S + s);
}

void mag_profile_host_w(const double *sse, const double *esum, const double *wsum, int64_t S, int C, bool per_curve,
                        double *best, double *P)
{
    for (int64_t s = 0; s < S; s++) mag_profile_one(sse, esum, wsum, S, C, s, per_curve, best, P + s);
}

struct MagArgs {
    double n[kMagMaxCurves];
    double d[kMagChunk];
};

// One thread per sample; a wavefront's accesses to every array are contiguous.  The curves are the OUTER loop over kMagAcc
// offsets at a time, their sums in registers: a sample's 2 C moments are loaded once per kMagAcc offsets (2 C S 8 B per
// 32 offsets against 32 S 16 B of P traffic) and every P[m][s] sees its curves in order, as mag_grid_one adds them.
constexpr int kMagAcc = 32;
__global__ void __launch_bounds__(256) mag_grid_kernel(const double *sse, const double *esum, int64_t S, int C, int M,
                                                       double *P, const MagArgs g)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (int64_t)gridDim.x * blockDim.x)
        for (int m0 = 0; m0 < M; m0 += kMagAcc) {
            double acc[kMagAcc];
#pragma unroll
            for (int k = 0; k < kMagAcc; k++) acc[k] = 0.0;
            for (int c = 0; c < C; c++) {
                const double q2 = sse[(int64_t)c * S + s], q1 = esum[(int64_t)c * S + s], n = g.n[c];
#pragma unroll
                for (int k = 0; k < kMagAcc; k++) acc[k] += mag_term(q2, q1, n, g.d[m0 + k < M ? m0 + k : M - 1]);
            }
#pragma unroll
            for (int k = 0; k < kMagAcc; k++)
                if (m0 + k < M) { double *p = P + (int64_t)(m0 + k) * S + s; *p = *p - acc[k]; }
        }
}

__global__ void __launch_bounds__(256) mag_profile_kernel(const double *sse, const double *esum, int64_t S, int C, int per_curve,
                                                          double *best, double *P, const MagArgs g)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (int64_t)gridDim.x * blockDim.x)
        mag_profile_one(sse, esum, g.n, S, C, s, per_curve != 0, best, P + s);
}

hipError_t launch_mag_grid_w(const double *sse, const double *esum, const double *wsum, int64_t S, int C,
                             const double *offsets, int64_t M, double *P, hipStream_t stream)
{
    if (S <= 0 || M <= 0) return hipSuccess;
    MagArgs g = {};
    for (int c = 0; c < C; c++) g.n[c] = wsum[c];
    for (int64_t m0 = 0; m0 < M; m0 += kMagChunk) {          // offsets travel as kernel arguments, kMagChunk per launch
        const int mc = (int)(M - m0 < kMagChunk ? M - m0 : kMagChunk);
        for (int m = 0; m < mc; m++) g.d[m] = offsets[m0 + m];
        hipLaunchKernelGGL(mag_grid_kernel, dim3(per_sample_blocks(S)), dim3(256), 0, stream, sse, esum, S, C, mc, P + m0 * S, g);
    }
    return hipGetLastError();
}

hipError_t launch_mag_profile_w(const double *sse, const double *esum, const double *wsum, int64_t S, int C, bool per_curve,
                                double *best, double *P, hipStream_t stream)
{
    if (S <= 0) return hipSuccess;
    MagArgs g = {};
    for (int c = 0; c < C; c++) g.n[c] = wsum[c];
    hipLaunchKernelGGL(mag_profile_kernel, dim3(per_sample_blocks(S)), dim3(256), 0, stream, sse, esum, S, C, per_curve ? 1 : 0,
                       best, P, g);
    return hipGetLastError();
}

// ---- host-side time interpolation of the unfused call sequence (bayeslib.py:184-191) ----
// out[r][i] = ((pl[r][hi_i] - pl[r][hi_i - 1]) / h_i) * dx_i + pl[r][hi_i - 1]: the arithmetic of scipy's interp1d / griddata as
// the reference applies it row by row -- the difference in the matrix's own type (float32 for the reference's buffer), then
// float64, two roundings, no fused multiply-add (this translation unit is compiled with -ffp-contract=off) -- bit for bit what
// driver.interp_rows computed with NumPy, without the interpreter lock: the worker threads of driver.simulate run it side by side
// (NumPy's fancy indexing serialised them: 0.21 s of a 0.60 s task, profiles/r6_levelb_task_phases.txt).  Plain host code.
template <typename T>
static void interp_rows_host(const T *pl, int64_t rows, int64_t ld, const int32_t *hi, const double *dx, const double *h,
                             int64_t n_obs, double *out, int64_t out_ld)
{
    for (int64_t r = 0; r < rows; r++) {
        const T *p = pl + r * ld;
        double *o = out + r * out_ld;
        for (int64_t i = 0; i < n_obs; i++) {
            const T lo = p[hi[i] - 1];
            const T d = p[hi[i]] - lo;
            const double slope = (double)d / h[i];
            const double prod = slope * dx[i];
            o[i] = prod + (double)lo;
        }
    }
}

void interp_rows_any(const void *pl, int elem_bytes, int64_t rows, int64_t ld, const int32_t *hi, const double *dx,
                     const double *h, int64_t n_obs, double *out, int64_t out_ld)
{
    if (elem_bytes == 4) interp_rows_host<float>((const float *)pl, rows, ld, hi, dx, h, n_obs, out, out_ld);
    else interp_rows_host<double>((const double *)pl, rows, ld, hi, dx, h, n_obs, out, out_ld);
}

}  // namespace trpl
