// The likelihood of a resident PL block against a BANK of J instrument responses, from one pass over the block
// (trpl_loglik_irf_bank*, include/trpl.h), and the profile over the bank (trpl_irf_bank_profile*).  For response j and row r the
// kernel forms, at the columns the observations need and nowhere else,
//     cv[c] = sum over k = 0 .. K-1, ascending, of  H[j][k] * (double)pl[r][c + k0 - k]          (csrc/irf.hip's sum, same bits)
// rounds it to the block's element type, takes log_pl of it (log_pl.hpp) and adds the squared error to sse[j][r] and the error to
// esum[j][r] with pl_loglik_kernel's mapping (likelihood.hip): one 256-thread workgroup per row, thread t adds observations
// t, t + 256, ... in ascending order, the xor butterfly inside each wave, then the four wave sums in order.  The kernel shares
// those expressions with pl_loglik_kernel (pl_score.hpp) and the staged column with irf.hip (irf_common.hpp).  The results are the bits of
// trpl_convolve_irf_dev followed by trpl_loglik_moments_from_pl_dev (trpl_loglik_weighted_from_pl_dev with wts), per response;
// the convolved block never exists.  Compiled with -ffp-contract=off like both of those units: one rounded product and one
// rounded addition per term.
//
// Structure.  A pass takes W <= kJB responses through the row: per chunk of 256 observations the workgroup stages the input
// columns the chunk reads in LDS as fp64 (consecutive lanes, consecutive doubles), then per tap every thread does one LDS read
// and W multiply-adds into W accumulators; the taps H[j][k] are wave-uniform scalar loads.  The running sse / esum of the W
// responses stay in registers across the chunks.  Responses beyond W are further passes over the row, from L2.
//   on the grid   thread t of chunk m owns column 256 m + t; the chunk reads the 256 + K - 1 input columns
//                 256 m + k0 - (K - 1) .. 256 m + k0 + 255.
//   off the grid  observation i needs the convolved columns hi - 1 and hi (hi = obs_hi[i], in any order): two accumulators per
//                 response, fed by ONE new read per tap (tap k of column hi - 1 reads what tap k + 1 of column hi reads).  The
//                 chunk's span is max hi - min hi + 2 columns; with its K - 1 halo it is staged when it fits kStage doubles,
//                 otherwise every lane reads its own window through the cache.  Both paths run the same ordered sum.
// A term whose input column is negative is skipped by a test (EDGE instantiations: chunks that touch column 0, and the cache
// path); a staged column outside [0, ncol - 1] holds 0.0 and never enters a stored sum.  No atomics, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "irf_common.hpp"
#include "log_pl.hpp"
#include "pl_score.hpp"

namespace trpl {
namespace irf_bank {

constexpr int kJB = TRPL_IRF_BANK_BLOCK;               // responses that share one pass over the taps
constexpr int kThreads = 256;                          // pl_loglik_kernel's workgroup: the association of the sums
constexpr int kStage = kThreads + TRPL_IRF_MAX_TAPS;   // doubles of the staged window: a chunk's span + K - 1
static_assert(kThreads + TRPL_IRF_MAX_TAPS - 1 <= kStage, "a chunk on the grid is always staged");
static_assert(kJB == 8, "pass_width() below cuts a bank into passes of 8, 4, 2 and 1");

// input column c - d of the thread's window, d = 0 the column tap 0 of the later output reads
struct LdsX {
    const double *p;
    __device__ __forceinline__ double operator()(int d) const { return p[-d]; }
};
template <typename T>
struct MemX {                                          // a column outside the row is never used: any element of the row does
    const T *row;
    int64_t c, ncol;
    __device__ __forceinline__ double operator()(int d) const { return (double)row[clamp_col(c - d, ncol)]; }
};

// NC convolved columns, c - k0 (v = 0) and with NC = 2 the one before it (v = 1), for W responses whose taps start at Hb, K apart:
// acc[v][j] = sum_k Hb[j K + k] * x(c - v - k), ascending k from +0.0, a term with c - v - k < 0 skipped (EDGE)
template <int NC, int W, bool EDGE, typename X>
__device__ __forceinline__ void conv(const X &x, const double *__restrict__ Hb, int K, int64_t c, double (&acc)[NC][W])
{
#pragma unroll
    for (int v = 0; v < NC; v++)
#pragma unroll
        for (int j = 0; j < W; j++) acc[v][j] = 0.0;
    double carry = NC == 2 ? x(0) : 0.0;
    auto tap = [&](int k) {
        double x0, x1 = 0.0;
        if constexpr (NC == 2) { x0 = carry; x1 = x(k + 1); carry = x1; }
        else x0 = x(k);
#pragma unroll
        for (int j = 0; j < W; j++) {
            const double hk = Hb[(int64_t)j * K + k];
            if (!EDGE || c - k >= 0) acc[0][j] += hk * x0;
            if constexpr (NC == 2) { if (!EDGE || c - 1 - k >= 0) acc[1][j] += hk * x1; }
        }
    };
    int k = 0;
    for (; k + 4 <= K; k += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) tap(k + u);
    }
    for (; k < K; k++) tap(k);
}

// the input columns cb .. cb + n_in - 1 of the row as fp64; outside [0, ncol - 1]: 0.0
template <typename T>
__device__ __forceinline__ void stage(double *xs, const T *__restrict__ prow, int64_t cb, int n_in, int64_t ncol)
{
    for (int s = threadIdx.x; s < n_in; s += kThreads) xs[s] = staged_col<T>(prow, cb + s, ncol);
}

// the arguments of the kernel but pl, H, sse and esum, which travel as __restrict__ parameters of their own: the taps are
// wave-uniform loads, and they are scalar loads only where the compiler knows that no store of the kernel reaches them
struct Args {
    int64_t rows, ncol, ld, n_obs;
    int J, K, k0;
    const double *obs;
    const int32_t *obs_hi;
    const double *obs_dx, *obs_h, *wts, *mag;
    const int32_t *status;
    uint32_t flags;
};

// W responses through the row: their taps from Hb on, their sums to sse / esum + w rows + row
template <typename T, bool WT, bool OFFGRID, int W>
__device__ __forceinline__ void pass(const Args &a, const T *__restrict__ prow, const double *__restrict__ Hb, double *__restrict__ sse,
                                     double *__restrict__ esum, double m, bool flagged, double *xs, double (*part)[kJB][4],
                                     int (*span)[4])
{
    constexpr int NC = OFFGRID ? 2 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, k0 = a.k0;
    const int64_t row = blockIdx.x, ncol = a.ncol, ncol_out = ncol - k0, n_obs = a.n_obs;
    const bool f32 = (a.flags & TRPL_FLAG_PL_F32) != 0 || sizeof(T) == 4;
    double s2[W], s1[W];
#pragma unroll
    for (int j = 0; j < W; j++) { s2[j] = 0.0; s1[j] = 0.0; }
    if (!flagged)                                                        // a flagged row scores +inf whatever its PL
        for (int64_t i0 = 0; i0 < n_obs; i0 += kThreads) {
            const int64_t i = i0 + tid;
            const bool live = i < n_obs;
            const int64_t ii = live ? i : n_obs - 1;                     // an idle lane repeats the last observation, and adds nothing
            double acc[NC][W];
            (void)ii;
            if constexpr (!OFFGRID) {
                const int64_t cb = i0 + k0 - (K - 1);
                stage<T>(xs, prow, cb, kThreads + K - 1, ncol);
                __syncthreads();
                const LdsX x{xs + tid + (K - 1)};
                if (cb >= 0) conv<NC, W, false>(x, Hb, K, i + k0, acc);
                else conv<NC, W, true>(x, Hb, K, i + k0, acc);
                __syncthreads();
            } else {
                int64_t hi = a.obs_hi[ii];
                hi = hi < 1 ? 1 : hi < ncol_out ? hi : ncol_out - 1;     // the caller's contract; a bad index must not leave the row
                int lo_w = (int)hi, hi_w = (int)hi;
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const int o0 = __shfl_xor(lo_w, off, 64), o1 = __shfl_xor(hi_w, off, 64);
                    lo_w = o0 < lo_w ? o0 : lo_w;
                    hi_w = o1 > hi_w ? o1 : hi_w;
                }
                if (lane == 0) { span[0][wave] = lo_w; span[1][wave] = hi_w; }
                __syncthreads();
                int hmin = span[0][0], hmax = span[1][0];
#pragma unroll
                for (int w = 1; w < 4; w++) {
                    hmin = span[0][w] < hmin ? span[0][w] : hmin;
                    hmax = span[1][w] > hmax ? span[1][w] : hmax;
                }
                const int64_t cb = (int64_t)hmin - 1 + k0 - (K - 1), n_in = (int64_t)hmax - hmin + 2 + (K - 1);
                if (n_in <= kStage) {                                    // workgroup-uniform
                    stage<T>(xs, prow, cb, (int)n_in, ncol);
                    __syncthreads();
                    const LdsX x{xs + (int)(hi + k0 - cb)};
                    if (cb >= 0) conv<NC, W, false>(x, Hb, K, hi + k0, acc);
                    else conv<NC, W, true>(x, Hb, K, hi + k0, acc);
                } else {
                    const MemX<T> x{prow, hi + k0, ncol};
                    conv<NC, W, true>(x, Hb, K, hi + k0, acc);
                }
                __syncthreads();                                         // xs and span are free for the next chunk
            }
            if (live) {
                const double ob = a.obs[i];
                double w = 1.0, oh = 1.0, odx = 0.0;
                if constexpr (WT) w = a.wts[i];
                if constexpr (OFFGRID) { oh = a.obs_h[i]; odx = a.obs_dx[i]; }
#pragma unroll
                for (int j = 0; j < W; j++) {
                    const T v = (T)acc[0][j];                            // what trpl_convolve_irf_dev stores
                    double y = log_pl<T>(v, v, false, f32);
                    if constexpr (OFFGRID) {
                        const T vl = (T)acc[1][j];
                        y = interp_log_pl(y, log_pl<T>(vl, vl, false, f32), oh, odx, f32);
                    }
                    score_add<WT>(y, m, ob, w, s2[j], s1[j]);
                }
            }
        }
#pragma unroll
    for (int j = 0; j < W; j++) {
        wave_add(s2[j]);
        wave_add(s1[j]);
        if (lane == 0) { part[0][j][wave] = s2[j]; part[1][j][wave] = s1[j]; }
    }
    __syncthreads();
    if (tid < W) {
        double r2 = row_sum(part[0][tid]), r1 = row_sum(part[1][tid]);
        row_flag(flagged, r2, r1);
        sse[(int64_t)tid * a.rows + row] = r2;
        if (esum) esum[(int64_t)tid * a.rows + row] = r1;
    }
    __syncthreads();                                                     // part is free for the next pass
}

// a bank is cut into passes of 8, 4, 2 and 1 responses, so that no pass carries an idle accumulator: the width of the next pass
// when `left` responses remain (never more than `left`)
__host__ __device__ constexpr int pass_width(int left) { return left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1; }

template <typename T, bool WT, bool OFFGRID>
__global__ void __launch_bounds__(kThreads) loglik_bank(const T *__restrict__ pl, const double *__restrict__ H, double *__restrict__ sse,
                                                        double *__restrict__ esum, const Args a)
{
    __shared__ double xs[kStage];
    __shared__ double part[2][kJB][4];
    __shared__ int span[2][4];
    const int64_t row = blockIdx.x;
    const T *__restrict__ prow = pl + row * a.ld;
    const double m = a.mag[row];
    const bool flagged = a.status && a.status[row] != 0;
    for (int j0 = 0; j0 < a.J;) {                                        // workgroup-uniform
        const int w = pass_width(a.J - j0);
        const double *__restrict__ Hj = H + (int64_t)j0 * a.K;
        double *__restrict__ sj = sse + (int64_t)j0 * a.rows, *__restrict__ ej = esum ? esum + (int64_t)j0 * a.rows : nullptr;
        if (w == 8) pass<T, WT, OFFGRID, 8>(a, prow, Hj, sj, ej, m, flagged, xs, part, span);
        else if (w == 4) pass<T, WT, OFFGRID, 4>(a, prow, Hj, sj, ej, m, flagged, xs, part, span);
        else if (w == 2) pass<T, WT, OFFGRID, 2>(a, prow, Hj, sj, ej, m, flagged, xs, part, span);
        else pass<T, WT, OFFGRID, 1>(a, prow, Hj, sj, ej, m, flagged, xs, part, span);
        j0 += w;
    }
}

// One thread per sample, coalesced over s: the greatest Pbank[j][s] and the first j that attains it.  NaN never compares
// greater and -inf is not greater than the start, so a sample whose values are all -inf or NaN keeps best = -1, P = -inf.
__host__ __device__ inline void profile_one(const double *Pbank, int J, int64_t S, int64_t s, int32_t *best, double *P)
{
    double p = -INFINITY;
    int32_t b = -1;
    for (int j = 0; j < J; j++) {
        const double v = Pbank[(int64_t)j * S + s];
        if (v > p) { p = v; b = j; }
    }
    best[s] = b;
    P[s] = p;
}

__global__ void __launch_bounds__(256) profile(const double *__restrict__ Pbank, int J, int64_t S, int32_t *__restrict__ best,
                                               double *__restrict__ P)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (int64_t)gridDim.x * blockDim.x)
        profile_one(Pbank, J, S, s, best, P);
}

}  // namespace irf_bank
}  // namespace trpl

using namespace trpl;

// what both forms of trpl_loglik_irf_bank refuse before a device is touched, in the order of include/trpl.h
static int check_bank(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *H, int32_t J, int32_t K,
                      int32_t k0, const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t n_obs,
                      const double *mag, const double *sse, uint32_t flags)
{
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes=%d must be 4 or 8", elem_bytes);
    if (rows < 0) return api_fail(TRPL_ERR_ARG, "rows=%lld must be >= 0", (long long)rows);
    if (rows > 0x7fffffffLL) return api_fail(TRPL_ERR_ARG, "rows=%lld is more than one launch takes (2^31 - 1)", (long long)rows);
    if (ncol < 1) return api_fail(TRPL_ERR_ARG, "ncol=%lld must be >= 1", (long long)ncol);
    if (ncol > 0x7fffffffLL) return api_fail(TRPL_ERR_ARG, "ncol=%lld must fit obs_hi's int32", (long long)ncol);
    if (ld < ncol) return api_fail(TRPL_ERR_ARG, "ld=%lld must be >= ncol=%lld", (long long)ld, (long long)ncol);
    if (K < 1 || K > TRPL_IRF_MAX_TAPS) return api_fail(TRPL_ERR_ARG, "K=%d must be in [1, TRPL_IRF_MAX_TAPS = %d]", K, TRPL_IRF_MAX_TAPS);
    if (k0 < 0 || k0 > K - 1) return api_fail(TRPL_ERR_ARG, "k0=%d must be in [0, K - 1 = %d]", k0, K - 1);
    if (ncol - k0 < 1) return api_fail(TRPL_ERR_ARG, "ncol=%lld - k0=%d leaves no output column", (long long)ncol, k0);
    if (J < 1 || J > TRPL_IRF_BANK_MAX_RESPONSES)
        return api_fail(TRPL_ERR_ARG, "J=%d must be in [1, TRPL_IRF_BANK_MAX_RESPONSES = %d]", J, TRPL_IRF_BANK_MAX_RESPONSES);
    if (n_obs < 1) return api_fail(TRPL_ERR_ARG, "n_obs=%lld must be >= 1", (long long)n_obs);
    const bool interp = obs_hi || obs_dx || obs_h;
    if (interp && !(obs_hi && obs_dx && obs_h)) return api_fail(TRPL_ERR_ARG, "obs_hi, obs_dx and obs_h go together");
    if (!interp && n_obs > ncol - k0)
        return api_fail(TRPL_ERR_ARG, "n_obs=%lld exceeds the ncol - k0 = %lld convolved columns", (long long)n_obs, (long long)(ncol - k0));
    if (interp && ncol - k0 < 2)
        return api_fail(TRPL_ERR_ARG, "ncol=%lld - k0=%d leaves one convolved column: obs_hi needs two", (long long)ncol, k0);
    if (flags & TRPL_FLAG_NORMALIZE)
        return api_fail(TRPL_ERR_ARG, "flags: TRPL_FLAG_NORMALIZE does not combine with an instrument response (the convolved "
                                      "curve's first column is not PL(0))");
    if (flags & ~(uint32_t)TRPL_FLAG_PL_F32) return api_fail(TRPL_ERR_ARG, "flags=0x%x: only TRPL_FLAG_PL_F32 is taken", flags);
    if (rows > 0) {
        if (!pl) return api_fail(TRPL_ERR_ARG, "pl is NULL");
        if (!H) return api_fail(TRPL_ERR_ARG, "H is NULL");
        if (!obs) return api_fail(TRPL_ERR_ARG, "obs is NULL");
        if (!mag) return api_fail(TRPL_ERR_ARG, "mag is NULL");
        if (!sse) return api_fail(TRPL_ERR_ARG, "sse is NULL");
    }
    return TRPL_OK;
}

static int check_profile(const double *Pbank, int32_t J, int64_t S, const int32_t *best, const double *P)
{
    if (J < 1 || J > TRPL_IRF_BANK_MAX_RESPONSES)
        return api_fail(TRPL_ERR_ARG, "J=%d must be in [1, TRPL_IRF_BANK_MAX_RESPONSES = %d]", J, TRPL_IRF_BANK_MAX_RESPONSES);
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 0", (long long)S);
    if (S > 0) {
        if (!Pbank) return api_fail(TRPL_ERR_ARG, "Pbank is NULL");
        if (!best) return api_fail(TRPL_ERR_ARG, "best is NULL");
        if (!P) return api_fail(TRPL_ERR_ARG, "P is NULL");
    }
    return TRPL_OK;
}

extern "C" {

int trpl_irf_bank_max_responses(void) { return TRPL_IRF_BANK_MAX_RESPONSES; }
int trpl_irf_bank_block(void) { return irf_bank::kJB; }

int trpl_loglik_irf_bank_dev(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *H, int32_t J,
                             int32_t K, int32_t k0, const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                             int64_t n_obs, const double *wts, const double *mag, const int32_t *status, double *sse, double *esum,
                             uint32_t flags, void *stream)
{
    if (int rc = check_bank(pl, elem_bytes, rows, ncol, ld, H, J, K, k0, obs, obs_hi, obs_dx, obs_h, n_obs, mag, sse, flags)) return rc;
    if (rows == 0) return TRPL_OK;
    const irf_bank::Args a = {rows, ncol, ld, n_obs, J, K, k0, obs, obs_hi, obs_dx, obs_h, wts, mag, status, flags};
    const dim3 grid((unsigned)rows), block(irf_bank::kThreads);
    hipStream_t st = (hipStream_t)stream;
#define TRPL_BANK(TT, WW, OO) hipLaunchKernelGGL((irf_bank::loglik_bank<TT, WW, OO>), grid, block, 0, st, (const TT *)pl, H, sse, esum, a)
#define TRPL_BANK_T(TT)                                                        \
    do {                                                                       \
        if (wts) { if (obs_hi) TRPL_BANK(TT, true, true); else TRPL_BANK(TT, true, false); }      \
        else     { if (obs_hi) TRPL_BANK(TT, false, true); else TRPL_BANK(TT, false, false); }    \
    } while (0)
    if (elem_bytes == 4) TRPL_BANK_T(float);
    else TRPL_BANK_T(double);
#undef TRPL_BANK_T
#undef TRPL_BANK
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "loglik_irf_bank launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_loglik_irf_bank(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *H, int32_t J, int32_t K,
                         int32_t k0, const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t n_obs,
                         const double *wts, const double *mag, const int32_t *status, double *sse, double *esum, uint32_t flags,
                         int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_bank(pl, elem_bytes, rows, ncol, ld, H, J, K, k0, obs, obs_hi, obs_dx, obs_h, n_obs, mag, sse, flags)) return rc;
    if (rows == 0) return TRPL_OK;
    // host data: what the _dev form cannot look at
    for (int j = 0; j < J; j++)
        for (int k = 0; k < K; k++)
            if (!isfinite(H[(size_t)j * K + k])) return api_fail(TRPL_ERR_ARG, "H[%d][%d]=%g is not finite", j, k, H[(size_t)j * K + k]);
    if (wts)
        for (int64_t i = 0; i < n_obs; i++)
            if (!(wts[i] >= 0.0) || !(wts[i] < INFINITY))
                return api_fail(TRPL_ERR_ARG, "wts[%lld]=%g: weights must be finite and >= 0", (long long)i, wts[i]);
    if (obs_hi)
        for (int64_t i = 0; i < n_obs; i++)
            if (obs_hi[i] < 1 || obs_hi[i] > ncol - k0 - 1)
                return api_fail(TRPL_ERR_ARG, "obs_hi[%lld]=%d must be in [1, ncol - k0 - 1 = %lld]", (long long)i, obs_hi[i],
                                (long long)(ncol - k0 - 1));
    const size_t eb = (size_t)elem_bytes, n = (size_t)n_obs;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const void *dPl = sg.in(pl, (size_t)ld * eb, (size_t)ncol * eb, (size_t)rows);          // compact on the device: ld = ncol
    const double *dH = sg.in(H, (size_t)J * (size_t)K);
    const double *dObs = sg.in(obs, n);
    const int32_t *dHi = obs_hi ? sg.in(obs_hi, n) : nullptr;
    const double *dDx = obs_hi ? sg.in(obs_dx, n) : nullptr, *dOh = obs_hi ? sg.in(obs_h, n) : nullptr;
    const double *dW = wts ? sg.in(wts, n) : nullptr;
    const double *dMag = sg.in(mag, (size_t)rows);
    const int32_t *dSt = status ? sg.in(status, (size_t)rows) : nullptr;
    double *dSse = sg.out(sse, (size_t)J * (size_t)rows);
    double *dEs = esum ? sg.out(esum, (size_t)J * (size_t)rows) : nullptr;
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_loglik_irf_bank_dev(dPl, elem_bytes, rows, ncol, ncol, dH, J, K, k0, dObs, dHi, dDx, dOh, n_obs, dW, dMag, dSt, dSse,
                                          dEs, flags, sg.stream()))
        return rc;
    return sg.finish(seconds);
}

int trpl_irf_bank_profile_dev(const double *Pbank, int32_t J, int64_t S, int32_t *best, double *P, void *stream)
{
    if (int rc = check_profile(Pbank, J, S, best, P)) return rc;
    if (S == 0) return TRPL_OK;
    hipLaunchKernelGGL(irf_bank::profile, dim3(per_sample_blocks(S)), dim3(256), 0, (hipStream_t)stream, Pbank, (int)J, S, best, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "irf_bank_profile launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

// plain host code, like trpl_mag_profile: the expression the kernel runs
int trpl_irf_bank_profile(const double *Pbank, int32_t J, int64_t S, int32_t *best, double *P)
{
    if (int rc = check_profile(Pbank, J, S, best, P)) return rc;
    for (int64_t s = 0; s < S; s++) irf_bank::profile_one(Pbank, J, S, s, best, P);
    return TRPL_OK;
}

}  // extern "C"
