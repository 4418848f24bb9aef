// Posterior weights and temperature scan with a per-sample proposal log-ratio kept BESIDE the log-likelihood
// (trpl_posterior_weights_lr*, trpl_posterior_tf_scan_lr*; include/trpl.h).  A refined set (csrc/refine.hip) weights sample s by
// exp(LL[s] / tf) / r(u_s); folding ln r into LL (LLc = LL - tf ln r) fixes the temperature.  Here
//     e_k[s] = LL[s] / tf_k - lnr[s],   m_k = nanmax_s e_k[s],   w_k[s] = exp(((e_k[s] - m_k) + 1000 ln 2) - ln S),
// so one pair (LL, lnr) serves every temperature.
//
// Contract: the same shape as posterior_scan.hip's.  Row k of the scan carries the BITS of trpl_posterior_weights_lr at
// tfs[k] followed by trpl_posterior_moments, and with lnr == +0.0 everywhere both carry the bits of the calls without a
// ratio.  posterior_common.hpp defines what that takes (sample -> (block, thread), rising order within a thread,
// block_reduce, the final_reduce kernel of posterior.hip).
//
// What differs from posterior_scan.hip: the sample that leads at one temperature need not lead at another (a large LL with a
// large ln r wins only while LL / tf outweighs it), so the maximum is taken per temperature, tiled like every other phase;
// the count of usable samples (neither LL nor lnr NaN) is the same at every temperature and rides in tile 0 of that phase.
//
// Phases (each a partial kernel + final_reduce):  max [K] and count  ->  normalising sums [K]  ->  sum W, sum W^2,
// sum W v_d [K][2 + D]  ->  central sums about those means [K][D]  ->  one small kernel forms the outputs.
// Compiled with -ffp-contract=off, like posterior.hip and posterior_scan.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "posterior_common.hpp"

namespace trpl {
namespace post {
namespace lr {

constexpr int kTile = 4;                 // temperatures per thread, as in posterior_scan.hip

// e = LL / tf - lnr rounded to fp64, what its two roundings dropped in `lost`: the remainder of the division (one fma, as in
// tempered_weight) and the error of the subtraction (two_sum), both exact.  lnr = +0.0 leaves q and adds +0.0 to lost.
__device__ __forceinline__ double exponent(double ll, double lnr, double tf, double &lost)
{
    const double q = ll / tf;
    double el;
    const double e = two_sum(q, -lnr, el);
    lost = fma(-q, tf, ll) * __builtin_amdgcn_rcp(tf) + el;
    return e;
}
// tempered_weight (posterior_common.hpp) with the exponent e above in place of LL / tf: m = nanmax(e), and `lost` joins
// the roundings of the three sums in corr.  With lnr = +0.0, e = LL / tf and corr is tempered_weight's (a corr of -0.0 may
// become +0.0, which fma(w, corr, w) does not see): the same bits.  e = -inf (LL = -inf or lnr = +inf) gives exp(-inf) = 0
// exactly, corr then being NaN; a NaN in LL or lnr gives NaN.
__device__ __forceinline__ double weight(double e, double lost, double m, double c_up, double c_size)
{
    double e0, e1, e2;
    const double u = two_sum(two_sum(two_sum(e, -m, e0), c_up, e1), -c_size, e2);
    const double corr = lost + ((e0 + e1) + e2);
    const double w = exp(u);
    return fabs(corr) < 0x1p-30 ? fma(w, corr, w) : w;
}

// the temperatures of this block's tile; a slot beyond K repeats the last temperature and is never stored
struct Tile {
    double tf[kTile];
    int k[kTile];
    __device__ __forceinline__ explicit Tile(const double *tfs, int K)
    {
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            k[j] = blockIdx.y * kTile + j;
            tf[j] = tfs[k[j] < K ? k[j] : K - 1];
        }
    }
    __device__ __forceinline__ int at(int j, int K) const { return k[j] < K ? k[j] : K - 1; }
};

// part[k][b] = the block's max of e_k (fmax ignores NaN, like np.nanmax); tile 0 also leaves the block's count of samples
// with neither LL nor lnr NaN in cnt[b]
__global__ void __launch_bounds__(kThreads) max_count_partial(const double *LL, const double *lnr, int64_t S, const double *tfs,
                                                              int K, double *part, double *cnt)
{
    __shared__ double sm[kThreads / 64];
    const Tile t(tfs, K);
    double m[kTile], n = 0.0;
#pragma unroll
    for (int j = 0; j < kTile; j++) m[j] = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = LL[i], r = lnr[i];
#pragma unroll
        for (int j = 0; j < kTile; j++) m[j] = fmax(m[j], ll / t.tf[j] - r);
        if (ll == ll && r == r) n += 1.0;
    }
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        const double r = block_reduce<true>(m[j], sm);
        if (threadIdx.x == 0 && t.k[j] < K) part[(int64_t)t.k[j] * gridDim.x + blockIdx.x] = r;
    }
    n = block_reduce<false>(n, sm);                    // whole numbers below 2^53: exact in any order
    if (threadIdx.x == 0 && blockIdx.y == 0) cnt[blockIdx.x] = n;
}

// part[k][b] = the block's nansum of the unnormalised weights at tfs[k]
__global__ void __launch_bounds__(kThreads) weights_partial(const double *LL, const double *lnr, int64_t S, const double *tfs,
                                                            int K, const double *mx, double c_up, double c_size, double *part)
{
    __shared__ double sm[kThreads / 64];
    const Tile t(tfs, K);
    double m[kTile], acc[kTile];
#pragma unroll
    for (int j = 0; j < kTile; j++) { m[j] = mx[t.at(j, K)]; acc[j] = 0.0; }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = LL[i], r = lnr[i];
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            double lost;
            const double e = exponent(ll, r, t.tf[j], lost);
            const double w = weight(e, lost, m[j], c_up, c_size);
            if (w == w) acc[j] += w;                                  // np.nansum
        }
    }
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        const double r = block_reduce<false>(acc[j], sm);
        if (threadIdx.x == 0 && t.k[j] < K) part[(int64_t)t.k[j] * gridDim.x + blockIdx.x] = r;
    }
}

// part[k][b][2 + D] = the block's sum W, sum W^2, sum W v_d at tfs[k], W = weight / norm[k]  (V is [D][S])
__global__ void __launch_bounds__(kThreads) moments1_partial(const double *LL, const double *lnr, const double *V, int64_t S,
                                                             int D, const double *tfs, int K, const double *mx,
                                                             const double *norm, double c_up, double c_size, double *part)
{
    __shared__ double sm[kThreads / 64];
    const Tile t(tfs, K);
    double m[kTile], s[kTile], sw[kTile], sw2[kTile], sv[kTile][kMaxDim];
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        m[j] = mx[t.at(j, K)];
        s[j] = norm[t.at(j, K)];
        sw[j] = 0.0; sw2[j] = 0.0;
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) sv[j][d] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = LL[i], r = lnr[i];
        double x[kMaxDim];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) x[d] = d < D ? V[(int64_t)d * S + i] : 0.0;      // wave-uniform
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            double lost;
            const double e = exponent(ll, r, t.tf[j], lost);
            const double w = weight(e, lost, m[j], c_up, c_size) / s[j];                 // utils.py:165
            sw[j] += w;
            sw2[j] += w * w;
#pragma unroll
            for (int d = 0; d < kMaxDim; d++) sv[j][d] += x[d] * w;
        }
    }
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        const bool store = threadIdx.x == 0 && t.k[j] < K;
        double *row = part + ((int64_t)(t.k[j] < K ? t.k[j] : 0) * gridDim.x + blockIdx.x) * (2 + D);
        double r = block_reduce<false>(sw[j], sm);
        if (store) row[0] = r;
        r = block_reduce<false>(sw2[j], sm);
        if (store) row[1] = r;
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) {
            if (d < D) {
                r = block_reduce<false>(sv[j][d], sm);
                if (store) row[2 + d] = r;
            }
        }
    }
}

// part[k][b][D] = the block's sum W (v_d - mean_kd)^2, mean_kd = sums[k][2 + d] / sums[k][0]  (np.average)
__global__ void __launch_bounds__(kThreads) moments2_partial(const double *LL, const double *lnr, const double *V, int64_t S,
                                                             int D, const double *tfs, int K, const double *mx,
                                                             const double *norm, const double *sums, double c_up, double c_size,
                                                             double *part)
{
    __shared__ double sm[kThreads / 64];
    __shared__ double mean[kTile][kMaxDim];
    const Tile t(tfs, K);
    if (threadIdx.x < kTile * kMaxDim) {
        const int j = threadIdx.x / kMaxDim, d = threadIdx.x % kMaxDim;
        const int k = blockIdx.y * kTile + j;                  // (not t.k[j]: a runtime index would move the tile out of registers)
        const double *row = sums + (int64_t)(k < K ? k : K - 1) * (2 + D);
        mean[j][d] = d < D ? row[2 + d] / row[0] : 0.0;
    }
    __syncthreads();
    double m[kTile], s[kTile], c[kTile][kMaxDim];
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        m[j] = mx[t.at(j, K)];
        s[j] = norm[t.at(j, K)];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) c[j][d] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = LL[i], r = lnr[i];
        double x[kMaxDim];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) x[d] = d < D ? V[(int64_t)d * S + i] : 0.0;
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            double lost;
            const double e = exponent(ll, r, t.tf[j], lost);
            const double w = weight(e, lost, m[j], c_up, c_size) / s[j];
#pragma unroll
            for (int d = 0; d < kMaxDim; d++) {
                const double xc = x[d] - mean[j][d];
                c[j][d] += (xc * xc) * w;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        const bool store = threadIdx.x == 0 && t.k[j] < K;
        double *row = part + ((int64_t)(t.k[j] < K ? t.k[j] : 0) * gridDim.x + blockIdx.x) * D;
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) {
            if (d < D) {
                const double r = block_reduce<false>(c[j][d], sm);
                if (store) row[d] = r;
            }
        }
    }
}

// one thread per (k, d), d == D being the statistics of temperature k
__global__ void finish_kernel(int K, int D, const double *mx, const double *cnt, const double *norm, const double *sums,
                              const double *central, double *stats, double *mean, double *var, double *Q)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = idx / (D + 1), d = idx % (D + 1);
    if (k >= K) return;
    const double *row = sums + (int64_t)k * (2 + D);
    if (d == D) {
        stats[6 * k + 0] = mx[k];
        stats[6 * k + 1] = norm[k];
        stats[6 * k + 2] = row[0];
        stats[6 * k + 3] = row[1];
        stats[6 * k + 4] = cnt[0];
        stats[6 * k + 5] = (row[0] * row[0]) / row[1];                // the effective sample size
        return;
    }
    const double v = central[(int64_t)k * D + d] / row[0];            // w_variance, utils.py:202-204
    mean[(int64_t)k * D + d] = row[2 + d] / row[0];                   // w_mean, utils.py:197-199
    var[(int64_t)k * D + d] = v;
    Q[(int64_t)k * D + d] = sqrt(row[1] * v);                         // w_sample_var, utils.py:168-170
}

// doubles of workspace: the block partials [K][kMaxBlocks][2 + D] (the max phase keeps its count partials behind its K rows:
// K nb + nb <= 2 K kMaxBlocks), then max[K], count, norm[K], sums[K][2 + D], central[K][D]
inline size_t part_doubles(int D, int K) { return (size_t)K * kMaxBlocks * (2 + D); }
inline size_t workspace_doubles(int D, int K) { return part_doubles(D, K) + 1 + (size_t)K * (2 + 2 + D + D) + 64; }

hipError_t launch_scan(const double *LL, const double *lnr, int64_t S, const double *V, int D, const double *tfs, int K,
                       double *stats, double *mean, double *var, double *Q, double *ws, hipStream_t st)
{
    const int nb = grid_for(S);
    const dim3 tiles(nb, (K + kTile - 1) / kTile);
    double *part = ws, *mx = ws + part_doubles(D, K), *cnt = mx + K, *norm = cnt + 1, *sums = norm + K,
           *central = sums + (size_t)K * (2 + D);
    const double c_up = 1000.0 * log(2.0), c_size = log((double)S);                   // utils.py:164
    hipLaunchKernelGGL(max_count_partial, tiles, dim3(kThreads), 0, st, LL, lnr, S, tfs, K, part, part + (size_t)K * nb);
    hipLaunchKernelGGL(final_reduce, dim3(1, K), dim3(kThreads), 0, st, part, nb, 1, true, mx);
    hipLaunchKernelGGL(final_reduce, dim3(1, 1), dim3(kThreads), 0, st, part + (size_t)K * nb, nb, 1, false, cnt);
    hipLaunchKernelGGL(weights_partial, tiles, dim3(kThreads), 0, st, LL, lnr, S, tfs, K, mx, c_up, c_size, part);
    hipLaunchKernelGGL(final_reduce, dim3(1, K), dim3(kThreads), 0, st, part, nb, 1, false, norm);
    hipLaunchKernelGGL(moments1_partial, tiles, dim3(kThreads), 0, st, LL, lnr, V, S, D, tfs, K, mx, norm, c_up, c_size, part);
    hipLaunchKernelGGL(final_reduce, dim3(2 + D, K), dim3(kThreads), 0, st, part, nb, 2 + D, false, sums);
    if (D > 0) {
        hipLaunchKernelGGL(moments2_partial, tiles, dim3(kThreads), 0, st, LL, lnr, V, S, D, tfs, K, mx, norm, sums, c_up, c_size,
                           part);
        hipLaunchKernelGGL(final_reduce, dim3(D, K), dim3(kThreads), 0, st, part, nb, D, false, central);
    }
    const int n = K * (D + 1);
    hipLaunchKernelGGL(finish_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, K, D, mx, cnt, norm, sums, central,
                       stats, mean, var, Q);
    return hipGetLastError();
}

// ---- one temperature, the weight vector written: trpl_posterior_weights with the ratio (posterior.hip's five launches) ----
__global__ void __launch_bounds__(kThreads) one_max_partial(const double *LL, const double *lnr, int64_t S, double tf, double *part)
{
    __shared__ double sm[kThreads / 64];
    double m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads)
        m = fmax(m, LL[i] / tf - lnr[i]);
    m = block_reduce<true>(m, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}
__global__ void __launch_bounds__(kThreads) one_weights_partial(const double *LL, const double *lnr, int64_t S, double tf,
                                                                const double *mx, double c_up, double c_size, double *W, double *part)
{
    __shared__ double sm[kThreads / 64];
    const double m = mx[0];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        double lost;
        const double e = exponent(LL[i], lnr[i], tf, lost);
        const double w = weight(e, lost, m, c_up, c_size);
        W[i] = w;
        if (w == w) acc += w;                                 // np.nansum
    }
    acc = block_reduce<false>(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// W /= sum (utils.py:165); thread 0 of block 0 leaves stats = {max, raw sum} where the caller asked for them
__global__ void __launch_bounds__(kThreads) one_scale_kernel(double *W, int64_t S, const double *mx, const double *sum, double *stats)
{
    const double s = sum[0];
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) W[i] = W[i] / s;
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = mx[0]; stats[1] = s; }
}

// ws: >= posterior_workspace_bytes(1), laid out as launch_posterior_weights does
hipError_t launch_weights(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats, double *ws,
                          hipStream_t st)
{
    const int nb = grid_for(S);
    double *part = ws, *mx = ws + kMaxBlocks, *sum = mx + 1;
    const double c_up = 1000.0 * log(2.0), c_size = log((double)S);                   // utils.py:164
    hipLaunchKernelGGL(one_max_partial, dim3(nb), dim3(kThreads), 0, st, LL, lnr, S, tf, part);
    hipLaunchKernelGGL(final_reduce, dim3(1, 1), dim3(kThreads), 0, st, part, nb, 1, true, mx);
    hipLaunchKernelGGL(one_weights_partial, dim3(nb), dim3(kThreads), 0, st, LL, lnr, S, tf, mx, c_up, c_size, W, part);
    hipLaunchKernelGGL(final_reduce, dim3(1, 1), dim3(kThreads), 0, st, part, nb, 1, false, sum);
    hipLaunchKernelGGL(one_scale_kernel, dim3(nb), dim3(kThreads), 0, st, W, S, mx, sum, stats);
    return hipGetLastError();
}

}  // namespace lr
}  // namespace post
}  // namespace trpl

using namespace trpl;

// what both scan forms refuse before a device is touched: check_scan of posterior_scan.hip, and lnr; tfs_host: the temperatures
// where the caller's pointer is host memory
static int check_scan_lr(const void *LL, const void *lnr, int64_t S, const void *V, int32_t D, const double *tfs,
                         const double *tfs_host, int32_t K, const void *stats, const void *mean, const void *var, const void *Q)
{
    if (S < 1) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 1", (long long)S);
    if (D < 0 || D > post::kMaxDim) return api_fail(TRPL_ERR_ARG, "D=%d must be in [0, %d]", D, post::kMaxDim);
    if (K < 1 || K > TRPL_TF_SCAN_MAX) return api_fail(TRPL_ERR_ARG, "K=%d must be in [1, TRPL_TF_SCAN_MAX = %d]", K, TRPL_TF_SCAN_MAX);
    if (!LL) return api_fail(TRPL_ERR_ARG, "LL is NULL");
    if (!lnr) return api_fail(TRPL_ERR_ARG, "lnr is NULL");
    if (!tfs) return api_fail(TRPL_ERR_ARG, "tfs is NULL");
    if (D > 0 && !V) return api_fail(TRPL_ERR_ARG, "V is NULL with D=%d (only D = 0 takes no columns)", D);
    if (!stats) return api_fail(TRPL_ERR_ARG, "stats is NULL");
    if (D > 0 && !mean) return api_fail(TRPL_ERR_ARG, "mean is NULL");
    if (D > 0 && !var) return api_fail(TRPL_ERR_ARG, "var is NULL");
    if (D > 0 && !Q) return api_fail(TRPL_ERR_ARG, "Q is NULL");
    if (tfs_host)
        for (int k = 0; k < K; k++)
            if (!(tfs_host[k] > 0) || !(tfs_host[k] < INFINITY))
                return api_fail(TRPL_ERR_ARG, "tfs[%d]=%g must be finite and > 0", k, tfs_host[k]);
    return TRPL_OK;
}

static int check_weights_lr(const void *LL, const void *lnr, int64_t S, double tf, const void *W)
{
    if (S < 1) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 1", (long long)S);
    if (!LL) return api_fail(TRPL_ERR_ARG, "LL is NULL");
    if (!lnr) return api_fail(TRPL_ERR_ARG, "lnr is NULL");
    if (!W) return api_fail(TRPL_ERR_ARG, "W is NULL");
    if (!(tf > 0) || !(tf < INFINITY)) return api_fail(TRPL_ERR_ARG, "tf=%g must be finite and > 0", tf);
    return TRPL_OK;
}

extern "C" {

int trpl_posterior_weights_lr_dev(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats,
                                  void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = check_weights_lr(LL, lnr, S, tf, W)) return rc;
    if (!workspace) return api_fail(TRPL_ERR_ARG, "workspace is NULL");
    if (workspace_bytes < (int64_t)posterior_workspace_bytes(1))
        return api_fail(TRPL_ERR_ARG, "workspace of %lld bytes is smaller than trpl_posterior_workspace_bytes(1) = %lld",
                        (long long)workspace_bytes, (long long)posterior_workspace_bytes(1));
    hipError_t e = post::lr::launch_weights(LL, lnr, S, tf, W, stats, (double *)workspace, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "posterior weights (log-ratio) launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_posterior_weights_lr(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats, int32_t device,
                              double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_weights_lr(LL, lnr, S, tf, W)) return rc;
    if (int rc = select_device(device)) return rc;
    CallScope cs;
    HIP_TRY(cs.open());
    DevBuf dL, dR, dW, dSt, ws;
    const size_t wsb = posterior_workspace_bytes(1);
    HIP_TRY(dL.alloc((size_t)S * 8, cs.st)); HIP_TRY(dR.alloc((size_t)S * 8, cs.st)); HIP_TRY(dW.alloc((size_t)S * 8, cs.st));
    HIP_TRY(dSt.alloc(16, cs.st)); HIP_TRY(ws.alloc(wsb, cs.st));
    HIP_TRY(hipMemcpyAsync(dL.p, LL, (size_t)S * 8, hipMemcpyHostToDevice, cs.st));
    HIP_TRY(hipMemcpyAsync(dR.p, lnr, (size_t)S * 8, hipMemcpyHostToDevice, cs.st));
    const double t0 = now_s();
    if (int rc = trpl_posterior_weights_lr_dev(dL.as<double>(), dR.as<double>(), S, tf, dW.as<double>(), dSt.as<double>(), ws.p,
                                               (int64_t)wsb, cs.st))
        return rc;
    HIP_TRY(hipStreamSynchronize(cs.st));
    if (seconds) *seconds = now_s() - t0;
    HIP_TRY(hipMemcpyAsync(W, dW.p, (size_t)S * 8, hipMemcpyDeviceToHost, cs.st));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, dSt.p, 16, hipMemcpyDeviceToHost, cs.st));
    HIP_TRY(hipStreamSynchronize(cs.st));        // the copies back have landed (and their errors surface here)
    return TRPL_OK;
}

int64_t trpl_posterior_tf_scan_lr_workspace(int64_t S, int32_t D, int32_t K)
{
    if (S < 1 || D < 0 || D > post::kMaxDim || K < 1 || K > TRPL_TF_SCAN_MAX) return 0;
    return (int64_t)(sizeof(double) * post::lr::workspace_doubles(D, K));
}

int trpl_posterior_tf_scan_lr_dev(const double *LL, const double *lnr, int64_t S, const double *V, int32_t D, const double *tfs,
                                  int32_t K, double *stats, double *mean, double *var, double *Q, void *workspace,
                                  int64_t workspace_bytes, void *stream)
{
    if (int rc = check_scan_lr(LL, lnr, S, V, D, tfs, nullptr, K, stats, mean, var, Q)) return rc;
    if (!workspace) return api_fail(TRPL_ERR_ARG, "workspace is NULL");
    if (workspace_bytes < trpl_posterior_tf_scan_lr_workspace(S, D, K))
        return api_fail(TRPL_ERR_ARG, "workspace of %lld bytes is smaller than trpl_posterior_tf_scan_lr_workspace(S, D, K) = %lld",
                        (long long)workspace_bytes, (long long)trpl_posterior_tf_scan_lr_workspace(S, D, K));
    hipError_t e = post::lr::launch_scan(LL, lnr, S, V, D, tfs, K, stats, mean, var, Q, (double *)workspace, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "posterior tf scan (log-ratio) launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_posterior_tf_scan_lr(const double *LL, const double *lnr, int64_t S, const double *V, int32_t D, const double *tfs,
                              int32_t K, double *stats, double *mean, double *var, double *Q, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_scan_lr(LL, lnr, S, V, D, tfs, tfs, K, stats, mean, var, Q)) return rc;
    if (int rc = select_device(device)) return rc;
    CallScope cs;
    HIP_TRY(cs.open());
    DevBuf dL, dR, dV, dT, dSt, dM, dVar, dQ, ws;
    const size_t wsb = (size_t)trpl_posterior_tf_scan_lr_workspace(S, D, K), kd = (size_t)K * D * 8;
    HIP_TRY(dL.alloc((size_t)S * 8, cs.st)); HIP_TRY(dR.alloc((size_t)S * 8, cs.st)); HIP_TRY(dV.alloc((size_t)S * D * 8, cs.st));
    HIP_TRY(dT.alloc((size_t)K * 8, cs.st)); HIP_TRY(dSt.alloc((size_t)K * 48, cs.st)); HIP_TRY(dM.alloc(kd, cs.st));
    HIP_TRY(dVar.alloc(kd, cs.st)); HIP_TRY(dQ.alloc(kd, cs.st)); HIP_TRY(ws.alloc(wsb, cs.st));
    HIP_TRY(hipMemcpyAsync(dL.p, LL, (size_t)S * 8, hipMemcpyHostToDevice, cs.st));
    HIP_TRY(hipMemcpyAsync(dR.p, lnr, (size_t)S * 8, hipMemcpyHostToDevice, cs.st));
    if (D > 0) HIP_TRY(hipMemcpyAsync(dV.p, V, (size_t)S * D * 8, hipMemcpyHostToDevice, cs.st));
    HIP_TRY(hipMemcpyAsync(dT.p, tfs, (size_t)K * 8, hipMemcpyHostToDevice, cs.st));
    const double t0 = now_s();
    if (int rc = trpl_posterior_tf_scan_lr_dev(dL.as<double>(), dR.as<double>(), S, D > 0 ? dV.as<double>() : nullptr, D,
                                               dT.as<double>(), K, dSt.as<double>(), dM.as<double>(), dVar.as<double>(),
                                               dQ.as<double>(), ws.p, (int64_t)wsb, cs.st))
        return rc;
    HIP_TRY(hipStreamSynchronize(cs.st));
    if (seconds) *seconds = now_s() - t0;
    HIP_TRY(hipMemcpyAsync(stats, dSt.p, (size_t)K * 48, hipMemcpyDeviceToHost, cs.st));
    if (D > 0) {
        HIP_TRY(hipMemcpyAsync(mean, dM.p, kd, hipMemcpyDeviceToHost, cs.st));
        HIP_TRY(hipMemcpyAsync(var, dVar.p, kd, hipMemcpyDeviceToHost, cs.st));
        HIP_TRY(hipMemcpyAsync(Q, dQ.p, kd, hipMemcpyDeviceToHost, cs.st));
    }
    HIP_TRY(hipStreamSynchronize(cs.st));        // the copies back have landed (and their errors surface here)
    return TRPL_OK;
}

}  // extern "C"
