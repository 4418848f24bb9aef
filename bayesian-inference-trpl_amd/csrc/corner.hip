// The corner: every posterior marginal of a finished run in one device call (trpl_corner*, include/trpl.h) -- what plot() of
// Visualization/marginalization_visual.py:500-609 does between loading a run and drawing it.
//
//   columns_kernel   one thread per sample, one read of its X row: the requested primary columns, the six secondary parameters
//       (secondary_parameters.py:9-57, in their order of operations), log10 where asked, and the exclusion by axis limits
//       (utils.py:145-155) as a NaN in LLk -- the marker the weights kernel already passes through.
//   keys_kernel      the bin of every value of every column, ONCE, one byte per sample and column (kNoBin = dropped), by the rules
//       of posterior.hip's bin_of: edges lo + (hi - lo) * k / bins, left-closed, the computed last edge closed, outside and
//       NaN dropped.
//   hist_kernel<CAP> one workgroup per histogram, its bins in LDS (CAP * CAP doubles for a pair, CAP for a column).  The
//       workgroup walks the samples in tiles of 64, every wave sees every tile, lane l looks at sample tile * 64 + l.  Wave w
//       OWNS the x bins [w * xpw, (w + 1) * xpw): no two waves touch the same word.  Inside a wave, lanes with the same bin
//       are ranked by lane (an emulated match-any over the bits of the local key) and round r adds the lanes of rank r: a
//       bin receives its samples one at a time in rising sample index, starting from +0.0.  That is the whole definition
//       of a bin's bits -- numpy.add.at(out, key, w) on the host -- and it depends on nothing but the inputs.  No
//       floating-point atomics.  A tile in which no owned sample has a weight > 0 is skipped by a ballot (adding +0.0 changes
//       no bit).  The plain counts c1 are integers (LDS integer atomics: exact in any order).
// Compiled with -ffp-contract=off like posterior.hip: the columns are the reference's expressions, one rounding per operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"

namespace trpl {
namespace corner {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNoBin = 255;                                      // key byte of a dropped value (bins <= 128)
constexpr int kUnroll = 8;                                       // tiles whose loads are in flight together

struct ColumnSpec {
    int32_t col[TRPL_CORNER_MAX_COLS];
    int32_t dolog[TRPL_CORNER_MAX_COLS];
    double excl_lo[TRPL_CORNER_PRIMARY], excl_hi[TRPL_CORNER_PRIMARY];
    int32_t D, exclude;
    double thickness;
};
struct Axes {
    double lo[TRPL_CORNER_MAX_COLS], hi[TRPL_CORNER_MAX_COLS];
};

// secondary_parameters.py, evaluated left to right; x**-1 is 1.0 / x and p0**2 is p0 * p0 (what NumPy does for those exponents)
__device__ __forceinline__ double t_rad(double B, double p0) { return 1.0 / (B * p0) * 1e9; }                    // :9-12
__device__ __forceinline__ double t_auger(double CP, double p0) { return 1.0 / (CP * (p0 * p0)) * 1e9; }         // :14-15
__device__ __forceinline__ double mu_eff(double mu_n, double mu_p) { return 2.0 / (1.0 / mu_n + 1.0 / mu_p); }   // :53-54
__device__ __forceinline__ double li_tau_eff(double B, double p0, double tau_n, double Sf, double Sb, double CP, double thickness,
                                             double mu)                                                          // :17-30
{
    const double Dif = mu * 0.0257 / 1.0 * 1e14 / 1e9;
    const double tau_surf = (thickness / ((Sf + Sb) * 0.01)) + (thickness * thickness / ((M_PI * M_PI) * Dif));
    const double t_r = t_rad(B, p0), t_aug = t_auger(CP, p0);
    return 1.0 / (1.0 / t_r + 1.0 / t_aug + 1.0 / tau_surf + 1.0 / tau_n);
}

__global__ void __launch_bounds__(kThreads) columns_kernel(const double *X, int64_t S, int64_t ldx, ColumnSpec sp, const double *LL,
                                                           double *V, double *LLk, unsigned long long *kept)
{
    __shared__ unsigned int s_cnt[kWaves];
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    bool keep = false;
    if (s < S) {
        double x[TRPL_CORNER_PRIMARY];
#pragma unroll
        for (int c = 0; c < TRPL_CORNER_PRIMARY; c++) x[c] = X[s * ldx + c];
        keep = true;
        if (sp.exclude) {
#pragma unroll
            for (int c = 0; c < TRPL_CORNER_PRIMARY; c++)       // a NaN limit: the column is not tested; a NaN value fails the test
                if (sp.excl_lo[c] == sp.excl_lo[c]) keep = keep && (x[c] <= sp.excl_hi[c] && x[c] >= sp.excl_lo[c]);
        }
        const double mu = mu_eff(x[2], x[3]);
        for (int d = 0; d < sp.D; d++) {
            double v;
            switch (sp.col[d]) {
                case TRPL_COL_TAU_EFF:  v = li_tau_eff(x[4], x[1], x[9], x[5], x[6], x[8], sp.thickness, mu); break;
                case TRPL_COL_TAU_RAD:  v = t_rad(x[4], x[1]); break;
                case TRPL_COL_S_SUM:    v = x[5] + x[6]; break;                                                  // s_eff :50-51
                case TRPL_COL_MU_EFF:   v = mu; break;
                case TRPL_COL_EPSILON:  v = 1.0 / x[11]; break;                                                  // epsilon :56-57
                case TRPL_COL_TAU_SUM:  v = x[9] + x[10]; break;                                                 // utils.py:78
                default: {
                    v = x[0];
#pragma unroll
                    for (int c = 1; c < TRPL_CORNER_PRIMARY; c++) v = sp.col[d] == c ? x[c] : v;
                }
            }
            if (sp.dolog[d]) v = log10(v);
            V[(int64_t)d * S + s] = v;
        }
        const double ll = LL ? LL[s] : 0.0;
        if (LLk) LLk[s] = keep ? ll : NAN;
        keep = keep && ll == ll;                                 // the count is that of filter_nan and the exclusion together
    }
    if (kept) {
        const unsigned long long m = __ballot(keep);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (unsigned int)__popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int n = 0;
#pragma unroll
            for (int w = 0; w < kWaves; w++) n += s_cnt[w];
            if (n) atomicAdd(kept, (unsigned long long)n);      // an integer count: exact in any order
        }
    }
}

// posterior.hip's edge and bin_of (without the LDS table), the library's one rule for a bin
__device__ __forceinline__ double edge(double lo, double hi, int k, int bins) { return lo + ((hi - lo) * k) / bins; }
__device__ __forceinline__ int bin_of(double x, double lo, double hi, double last, int bins, double scale)
{
    if (!(x >= lo && x <= last)) return -1;                      // also drops NaN
    int k = (int)((x - lo) * scale);
    k = k < 0 ? 0 : (k > bins - 1 ? bins - 1 : k);
    while (k > 0 && x < edge(lo, hi, k, bins)) k--;
    while (k < bins - 1 && x >= edge(lo, hi, k + 1, bins)) k++;
    return k;
}

__global__ void __launch_bounds__(kThreads) keys_kernel(const double *V, int64_t S, int64_t ldv, Axes ax, int bins, uint8_t *keys)
{
    const int d = blockIdx.y;
    const double lo = ax.lo[d], hi = ax.hi[d], last = edge(lo, hi, bins, bins), scale = bins / (hi - lo);
    for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < S; s += (int64_t)gridDim.x * kThreads) {
        const int k = bin_of(V[(int64_t)d * ldv + s], lo, hi, last, bins, scale);
        keys[(int64_t)d * S + s] = (uint8_t)(k < 0 ? kNoBin : k);
    }
}

// lanes of `pend` whose key equals this lane's (this lane included when it is in pend): a match-any over nbits bits
__device__ __forceinline__ unsigned long long match_key(unsigned long long pend, int key, int nbits)
{
    unsigned long long m = pend;
    for (int b = 0; b < nbits; b++) {
        const bool bit = (key >> b) & 1;
        const unsigned long long has = __ballot(bit);
        m &= bit ? has : ~has;
    }
    return m;
}

// blocks 0 .. D-1: column b (h1, c1); blocks D ..: pair p = b - D in the order of utils.py:103-106 (for i = 1 .. D-1, for j < i:
// x = column j, y = column i), h2[p][x bin][y bin]
template <int CAP>
__global__ void __launch_bounds__(kThreads) hist_kernel(const uint8_t *keys, const double *W, int64_t S, int D, int bins, double *h1,
                                                        double *c1, double *h2)
{
    __shared__ double s_bins[CAP * CAP];
    __shared__ unsigned long long s_cnt[CAP];
    const int b = blockIdx.x;
    const bool pair = b >= D;
    int cx = b, cy = 0;
    if (pair) {
        int p = b - D, i = 1;
        while (p >= i) { p -= i; i++; }
        cx = p; cy = i;
    }
    const int ybins = pair ? bins : 1, nb = bins * ybins;
    const bool count = !pair && c1 != nullptr;
    for (int k = threadIdx.x; k < nb; k += kThreads) s_bins[k] = 0.0;
    if (count) for (int k = threadIdx.x; k < bins; k += kThreads) s_cnt[k] = 0ull;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xpw = (bins + kWaves - 1) / kWaves, x0 = wave * xpw;        // this wave's x bins: [x0, x0 + xpw)
    int nbits = 0;
    while ((1 << nbits) < xpw * ybins) nbits++;                          // bits of the local key (kx - x0) * ybins + ky
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const uint8_t *kxp = keys + (int64_t)cx * S, *kyp = keys + (int64_t)cy * S;
    volatile double *vbins = s_bins;                             // a lane reads what ANOTHER lane stored a round before
    const int64_t tiles = (S + 63) / 64;
    for (int64_t t0 = 0; t0 < tiles; t0 += kUnroll) {
        double w[kUnroll];
        int kx[kUnroll], ky[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {                      // all loads of kUnroll tiles first; beyond S: dropped
            const int64_t s = (t0 + u) * 64 + lane;
            const bool in = s < S;
            const int64_t at = in ? s : 0;
            w[u] = in ? W[at] : NAN;
            kx[u] = in ? kxp[at] : kNoBin;
            ky[u] = pair ? (in ? kyp[at] : kNoBin) : 0;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const bool binned = kx[u] != kNoBin && ky[u] != kNoBin && kx[u] >= x0 && kx[u] < x0 + xpw;
            if (count && binned && w[u] == w[u]) atomicAdd(&s_cnt[kx[u]], 1ull);
            const bool add = binned && w[u] > 0.0 && w[u] < INFINITY;
            const unsigned long long pend = __ballot(add);
            if (!pend) continue;                                 // wave-uniform
            const int key = add ? (kx[u] - x0) * ybins + ky[u] : 0;
            const unsigned long long same = match_key(pend, key, nbits);
            const int rank = add ? __popcll(same & below) : -1;
            const int at = kx[u] * ybins + ky[u];
            for (int r = 0;; r++) {                              // round r: the r-th lane of every bin, so in sample order
                if (rank == r) vbins[at] = vbins[at] + w[u];
                __builtin_amdgcn_wave_barrier();
                if (!__ballot(rank > r)) break;
            }
        }
    }
    __syncthreads();
    double *out = pair ? h2 + (int64_t)(b - D) * nb : h1 + (int64_t)b * bins;
    for (int k = threadIdx.x; k < nb; k += kThreads) out[k] = s_bins[k];
    if (count) for (int k = threadIdx.x; k < bins; k += kThreads) c1[(int64_t)b * bins + k] = (double)s_cnt[k];
}

}  // namespace corner
}  // namespace trpl

using namespace trpl;

static bool is_secondary(int32_t c) { return c >= TRPL_CORNER_PRIMARY; }

static int check_columns(const void *X, int64_t S, int64_t ldx, const int32_t *cols, const int32_t *dolog, int32_t D, double thickness_nm,
                         const double *excl_lo, const double *excl_hi, const void *LL, const void *V, const void *LLk)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 0", (long long)S);
    if (D < 1 || D > TRPL_CORNER_MAX_COLS) return api_fail(TRPL_ERR_ARG, "D=%d must be in [1, TRPL_CORNER_MAX_COLS = %d]", D, TRPL_CORNER_MAX_COLS);
    if (!cols) return api_fail(TRPL_ERR_ARG, "cols is NULL");
    if (!dolog) return api_fail(TRPL_ERR_ARG, "dolog is NULL");
    for (int d = 0; d < D; d++) {
        if (cols[d] < 0 || cols[d] >= TRPL_CORNER_MAX_COLS)
            return api_fail(TRPL_ERR_ARG, "cols[%d]=%d is no column code (0 .. %d)", d, cols[d], TRPL_CORNER_MAX_COLS - 1);
        if (cols[d] == TRPL_COL_TAU_EFF && !(thickness_nm > 0.0 && thickness_nm < INFINITY))
            return api_fail(TRPL_ERR_ARG, "thickness_nm=%g must be finite and > 0 when tau_eff is requested", thickness_nm);
    }
    if ((excl_lo == nullptr) != (excl_hi == nullptr)) return api_fail(TRPL_ERR_ARG, "excl_lo and excl_hi must be given together");
    for (int c = 0; excl_lo && c < TRPL_CORNER_PRIMARY; c++)
        if (excl_lo[c] == excl_lo[c] && excl_hi[c] != excl_hi[c])
            return api_fail(TRPL_ERR_ARG, "excl_hi[%d] is NaN while excl_lo[%d]=%g is not: a tested column needs both limits", c, c, excl_lo[c]);
    if (ldx < TRPL_CORNER_PRIMARY) return api_fail(TRPL_ERR_ARG, "ldx=%lld must be >= %d", (long long)ldx, TRPL_CORNER_PRIMARY);
    if (LLk && !LL) return api_fail(TRPL_ERR_ARG, "LLk needs LL");
    if (!V) return api_fail(TRPL_ERR_ARG, "V is NULL");
    if (S > 0 && !X) return api_fail(TRPL_ERR_ARG, "X is NULL");
    return TRPL_OK;
}

static int check_hist(const void *V, int64_t S, int64_t ldv, int32_t D, const void *W, const double *lo, const double *hi, int32_t bins,
                      const void *h1, const void *h2)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 0", (long long)S);
    if (D < 1 || D > TRPL_CORNER_MAX_COLS) return api_fail(TRPL_ERR_ARG, "D=%d must be in [1, TRPL_CORNER_MAX_COLS = %d]", D, TRPL_CORNER_MAX_COLS);
    if (bins < 1 || bins > TRPL_CORNER_MAX_BINS)
        return api_fail(TRPL_ERR_ARG, "bins=%d must be in [1, TRPL_CORNER_MAX_BINS = %d]", bins, TRPL_CORNER_MAX_BINS);
    if (!lo) return api_fail(TRPL_ERR_ARG, "lo is NULL");
    if (!hi) return api_fail(TRPL_ERR_ARG, "hi is NULL");
    for (int d = 0; d < D; d++)
        if (!(lo[d] > -INFINITY && hi[d] < INFINITY && hi[d] > lo[d]))
            return api_fail(TRPL_ERR_ARG, "lo[%d]=%g, hi[%d]=%g: the limits must be finite with hi > lo", d, lo[d], d, hi[d]);
    if (ldv < S) return api_fail(TRPL_ERR_ARG, "ldv=%lld must be >= S=%lld", (long long)ldv, (long long)S);
    if (!h1) return api_fail(TRPL_ERR_ARG, "h1 is NULL");
    if (S > 0 && !V) return api_fail(TRPL_ERR_ARG, "V is NULL");
    if (S > 0 && !W) return api_fail(TRPL_ERR_ARG, "W is NULL");
    (void)h2;
    return TRPL_OK;
}

extern "C" {

int64_t trpl_corner_workspace_bytes(int64_t S, int32_t D)
{
    if (S < 0 || D < 1 || D > TRPL_CORNER_MAX_COLS) return 0;
    return ((int64_t)D * S + 255) / 256 * 256 + 256;             // one key byte per sample and column
}

int trpl_corner_columns_dev(const double *X, int64_t S, int64_t ldx, const int32_t *cols, const int32_t *dolog, int32_t D,
                            double thickness_nm, const double *excl_lo, const double *excl_hi, const double *LL, double *V, double *LLk,
                            int64_t *kept, void *stream)
{
    if (int rc = check_columns(X, S, ldx, cols, dolog, D, thickness_nm, excl_lo, excl_hi, LL, V, LLk)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (kept) HIP_TRY(hipMemsetAsync(kept, 0, sizeof(int64_t), st));
    if (S == 0) return TRPL_OK;
    const int64_t nblk = (S + corner::kThreads - 1) / corner::kThreads;
    if (nblk > 0x7fffffff) return api_fail(TRPL_ERR_ARG, "S=%lld is more than 2^31 - 1 blocks of %d samples", (long long)S, corner::kThreads);
    corner::ColumnSpec sp = {};
    sp.D = D;
    sp.thickness = thickness_nm;
    sp.exclude = excl_lo != nullptr;
    for (int d = 0; d < D; d++) { sp.col[d] = cols[d]; sp.dolog[d] = dolog[d] != 0; }
    for (int c = 0; c < TRPL_CORNER_PRIMARY; c++) {
        sp.excl_lo[c] = excl_lo ? excl_lo[c] : NAN;
        sp.excl_hi[c] = excl_hi ? excl_hi[c] : NAN;
    }
    hipLaunchKernelGGL(corner::columns_kernel, dim3((unsigned)nblk), dim3(corner::kThreads), 0, st, X, S, ldx, sp, LL, V, LLk,
                       (unsigned long long *)kept);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "corner columns launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_corner_hist_dev(const double *V, int64_t S, int64_t ldv, int32_t D, const double *W, const double *lo, const double *hi,
                         int32_t bins, double *h1, double *c1, double *h2, void *workspace, void *stream)
{
    if (int rc = check_hist(V, S, ldv, D, W, lo, hi, bins, h1, h2)) return rc;
    if (S > 0 && !workspace) return api_fail(TRPL_ERR_ARG, "workspace is NULL");
    hipStream_t st = (hipStream_t)stream;
    uint8_t *keys = (uint8_t *)workspace;
    if (S > 0) {
        corner::Axes ax = {};
        for (int d = 0; d < D; d++) { ax.lo[d] = lo[d]; ax.hi[d] = hi[d]; }
        int64_t nblk = (S + corner::kThreads - 1) / corner::kThreads;
        if (nblk > 1024) nblk = 1024;
        hipLaunchKernelGGL(corner::keys_kernel, dim3((unsigned)nblk, (unsigned)D), dim3(corner::kThreads), 0, st, V, S, ldv, ax, (int)bins, keys);
    }
    const unsigned grid = (unsigned)(D + (h2 ? D * (D - 1) / 2 : 0));
    if (bins <= 64)      hipLaunchKernelGGL(corner::hist_kernel<64>, dim3(grid), dim3(corner::kThreads), 0, st, keys, W, S, (int)D, (int)bins, h1, c1, h2);
    else if (bins <= 96) hipLaunchKernelGGL(corner::hist_kernel<96>, dim3(grid), dim3(corner::kThreads), 0, st, keys, W, S, (int)D, (int)bins, h1, c1, h2);
    else                 hipLaunchKernelGGL(corner::hist_kernel<128>, dim3(grid), dim3(corner::kThreads), 0, st, keys, W, S, (int)D, (int)bins, h1, c1, h2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "corner histogram launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_corner(const double *X, int64_t S, int64_t ldx, const double *LL, double tf, const int32_t *cols, const int32_t *dolog, int32_t D,
                double thickness_nm, const double *excl_lo, const double *excl_hi, const double *lo, const double *hi, int32_t bins,
                double *V, double *W, int64_t *kept, double *h1, double *c1, double *h2, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    // every refusal before a device is touched; V and LLk are the call's own buffers
    if (int rc = check_columns(X, S, ldx, cols, dolog, D, thickness_nm, excl_lo, excl_hi, LL, (const void *)1, LL)) return rc;
    if (int rc = check_hist((const void *)1, S, S, D, (const void *)1, lo, hi, bins, h1, h2)) return rc;
    if (S > 0 && !LL) return api_fail(TRPL_ERR_ARG, "LL is NULL");
    if (!(tf > 0.0)) return api_fail(TRPL_ERR_ARG, "tf=%g must be > 0", tf);
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const int64_t npair = (int64_t)D * (D - 1) / 2, wsb = trpl_posterior_workspace_bytes(1);
    const size_t h1n = (size_t)D * bins, s = (size_t)S;
    const double *dX = sg.in(X, S ? (s - 1) * (size_t)ldx + TRPL_CORNER_PRIMARY : 0), *dLL = sg.in(LL, s);   // X ends with its last row
    double *dLLk = (double *)sg.scratch(s * 8), *dV = sg.out(V, s * D), *dW = sg.out(W, s);
    int64_t *dKept = sg.out(kept, 1);
    double *dH1 = sg.out(h1, h1n), *dC1 = sg.out(c1, h1n), *dH2 = sg.out(h2, (size_t)npair * bins * bins);
    void *dWs = sg.scratch((size_t)wsb), *dKeys = sg.scratch((size_t)trpl_corner_workspace_bytes(S, D));
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_corner_columns_dev(dX, S, ldx, cols, dolog, D, thickness_nm, excl_lo, excl_hi, dLL, dV, dLLk, dKept, sg.stream())) return rc;
    if (int rc = trpl_posterior_weights_dev(dLLk, S, tf, dW, nullptr, dWs, wsb, sg.stream())) return rc;
    if (int rc = trpl_corner_hist_dev(dV, S, S, D, dW, lo, hi, bins, dH1, c1 ? dC1 : nullptr, (h2 && npair) ? dH2 : nullptr, dKeys, sg.stream()))
        return rc;
    return sg.finish(seconds);
}

}  // extern "C"
