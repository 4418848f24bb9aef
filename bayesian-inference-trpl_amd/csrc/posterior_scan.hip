// Temperature scan of the posterior core: for K temperatures tfs[k] at once, what trpl_posterior_weights(LL, S, tfs[k])
// followed by trpl_posterior_moments(V, S, D, W_k) returns -- the maximum, the normalising sum, sum W^2, the weighted means
// and variances of the D columns and Q = sqrt(sum W^2 * variance), the objective of the reference's tf_driver
// (Visualization/utils.py:168-179) -- without ever writing a weight vector: the weights at K temperatures are K exponentials
// of the same LL[s], recomputed in registers by every phase that needs them.
//
// Contract: row k carries the BITS of the two existing calls.  posterior_common.hpp defines what that takes: a sample
// belongs to the same (block, thread) as there, a thread adds its samples in the same order, blocks combine through the same
// block_reduce and the same final_reduce kernel.  So every (thread, temperature, column) keeps an accumulator of its own;
// a thread holds kTile temperatures of them in registers and gridDim.y covers the K / kTile tiles.  The maximum of LL / tf_k is
// max(LL) / tf_k (IEEE division by a positive number is monotone): one max phase serves all K.
//
// Phases (each a partial kernel + final_reduce):  max and count of LL  ->  normalising sums [K]  ->  sum W, sum W^2,
// sum W v_d [K][2 + D]  ->  central sums about those means [K][D]  ->  one small kernel forms the outputs.
// Compiled with -ffp-contract=off, like posterior.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "api_util.hpp"
#include "posterior_common.hpp"

namespace trpl {
namespace post {
namespace scan {

constexpr int kTile = 4;                 // temperatures per thread

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
};

// part[0][b] = max of the block's LL (fmax ignores NaN, like np.nanmax), part[1][b] = its count of non-NaN entries
__global__ void __launch_bounds__(kThreads) max_count_partial(const double *LL, int64_t S, double *part)
{
    __shared__ double sm[kThreads / 64];
    double m = -INFINITY, n = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = LL[i];
        m = fmax(m, ll);
        if (ll == ll) n += 1.0;
    }
    m = block_reduce<true>(m, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
    n = block_reduce<false>(n, sm);                    // whole numbers below 2^53: exact in any order
    if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = n;
}

// part[k][b] = the block's nansum of the unnormalised weights at tfs[k]
__global__ void __launch_bounds__(kThreads) weights_partial(const double *LL, int64_t S, const double *tfs, int K,
                                                            const double *mxc, double c_up, double c_size, double *part)
{
    __shared__ double sm[kThreads / 64];
    const Tile t(tfs, K);
    double m[kTile], acc[kTile];
#pragma unroll
    for (int j = 0; j < kTile; j++) { m[j] = mxc[0] / t.tf[j]; acc[j] = 0.0; }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = LL[i];
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const double w = tempered_weight(ll, t.tf[j], m[j], c_up, c_size);
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
__global__ void __launch_bounds__(kThreads) moments1_partial(const double *LL, const double *V, int64_t S, int D,
                                                             const double *tfs, int K, const double *mxc, const double *norm,
                                                             double c_up, double c_size, double *part)
{
    __shared__ double sm[kThreads / 64];
    const Tile t(tfs, K);
    double m[kTile], s[kTile], sw[kTile], sw2[kTile], sv[kTile][kMaxDim];
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        m[j] = mxc[0] / t.tf[j];
        s[j] = norm[t.k[j] < K ? t.k[j] : K - 1];
        sw[j] = 0.0; sw2[j] = 0.0;
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) sv[j][d] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = LL[i];
        double x[kMaxDim];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) x[d] = d < D ? V[(int64_t)d * S + i] : 0.0;      // wave-uniform
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const double w = tempered_weight(ll, t.tf[j], m[j], c_up, c_size) / s[j];     // utils.py:165
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
__global__ void __launch_bounds__(kThreads) moments2_partial(const double *LL, const double *V, int64_t S, int D,
                                                             const double *tfs, int K, const double *mxc, const double *norm,
                                                             const double *sums, double c_up, double c_size, double *part)
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
        m[j] = mxc[0] / t.tf[j];
        s[j] = norm[t.k[j] < K ? t.k[j] : K - 1];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) c[j][d] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = LL[i];
        double x[kMaxDim];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) x[d] = d < D ? V[(int64_t)d * S + i] : 0.0;
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const double w = tempered_weight(ll, t.tf[j], m[j], c_up, c_size) / s[j];
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
__global__ void finish_kernel(const double *tfs, int K, int D, const double *mxc, const double *norm, const double *sums,
                              const double *central, double *stats, double *mean, double *var, double *Q)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = idx / (D + 1), d = idx % (D + 1);
    if (k >= K) return;
    const double *row = sums + (int64_t)k * (2 + D);
    if (d == D) {
        stats[4 * k + 0] = mxc[0] / tfs[k];
        stats[4 * k + 1] = norm[k];
        stats[4 * k + 2] = row[1];
        stats[4 * k + 3] = mxc[1];
        return;
    }
    const double v = central[(int64_t)k * D + d] / row[0];            // w_variance, utils.py:202-204
    mean[(int64_t)k * D + d] = row[2 + d] / row[0];                   // w_mean, utils.py:197-199
    var[(int64_t)k * D + d] = v;
    Q[(int64_t)k * D + d] = sqrt(row[1] * v);                         // w_sample_var, utils.py:168-170
}

// doubles of workspace: the block partials [K][kMaxBlocks][2 + D], then {max, count}, norm[K], sums[K][2 + D], central[K][D]
inline size_t part_doubles(int D, int K) { return (size_t)K * kMaxBlocks * (2 + D); }
inline size_t workspace_doubles(int D, int K) { return part_doubles(D, K) + 2 + (size_t)K * (1 + 2 + D + D) + 64; }

hipError_t launch(const double *LL, int64_t S, const double *V, int D, const double *tfs, int K, double *stats, double *mean,
                  double *var, double *Q, double *ws, hipStream_t st)
{
    const int nb = grid_for(S);
    const dim3 tiles(nb, (K + kTile - 1) / kTile);
    double *part = ws, *mxc = ws + part_doubles(D, K), *norm = mxc + 2, *sums = norm + K, *central = sums + (size_t)K * (2 + D);
    const double c_up = 1000.0 * log(2.0), c_size = log((double)S);                   // utils.py:164
    hipLaunchKernelGGL(max_count_partial, dim3(nb), dim3(kThreads), 0, st, LL, S, part);
    hipLaunchKernelGGL(final_reduce, dim3(1, 1), dim3(kThreads), 0, st, part, nb, 1, true, mxc);
    hipLaunchKernelGGL(final_reduce, dim3(1, 1), dim3(kThreads), 0, st, part + nb, nb, 1, false, mxc + 1);
    hipLaunchKernelGGL(weights_partial, tiles, dim3(kThreads), 0, st, LL, S, tfs, K, mxc, c_up, c_size, part);
    hipLaunchKernelGGL(final_reduce, dim3(1, K), dim3(kThreads), 0, st, part, nb, 1, false, norm);
    hipLaunchKernelGGL(moments1_partial, tiles, dim3(kThreads), 0, st, LL, V, S, D, tfs, K, mxc, norm, c_up, c_size, part);
    hipLaunchKernelGGL(final_reduce, dim3(2 + D, K), dim3(kThreads), 0, st, part, nb, 2 + D, false, sums);
    if (D > 0) {
        hipLaunchKernelGGL(moments2_partial, tiles, dim3(kThreads), 0, st, LL, V, S, D, tfs, K, mxc, norm, sums, c_up, c_size, part);
        hipLaunchKernelGGL(final_reduce, dim3(D, K), dim3(kThreads), 0, st, part, nb, D, false, central);
    }
    const int n = K * (D + 1);
    hipLaunchKernelGGL(finish_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, tfs, K, D, mxc, norm, sums,
                       central, stats, mean, var, Q);
    return hipGetLastError();
}

}  // namespace scan
}  // namespace post
}  // namespace trpl

using namespace trpl;

// what both forms refuse before a device is touched; tfs_host: the temperatures where the caller's pointer is host memory
static int check_scan(const void *LL, int64_t S, const void *V, int32_t D, const double *tfs, const double *tfs_host, int32_t K,
                      const void *stats, const void *mean, const void *var, const void *Q)
{
    if (S < 1) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 1", (long long)S);
    if (D < 0 || D > post::kMaxDim) return api_fail(TRPL_ERR_ARG, "D=%d must be in [0, %d]", D, post::kMaxDim);
    if (K < 1 || K > TRPL_TF_SCAN_MAX) return api_fail(TRPL_ERR_ARG, "K=%d must be in [1, TRPL_TF_SCAN_MAX = %d]", K, TRPL_TF_SCAN_MAX);
    if (!LL) return api_fail(TRPL_ERR_ARG, "LL is NULL");
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

extern "C" {

int64_t trpl_posterior_tf_scan_workspace(int64_t S, int32_t D, int32_t K)
{
    if (S < 1 || D < 0 || D > post::kMaxDim || K < 1 || K > TRPL_TF_SCAN_MAX) return 0;
    return (int64_t)(sizeof(double) * post::scan::workspace_doubles(D, K));
}

int trpl_posterior_tf_scan_dev(const double *LL, int64_t S, const double *V, int32_t D, const double *tfs, int32_t K,
                               double *stats, double *mean, double *var, double *Q, void *workspace, int64_t workspace_bytes,
                               void *stream)
{
    if (int rc = check_scan(LL, S, V, D, tfs, nullptr, K, stats, mean, var, Q)) return rc;
    if (!workspace) return api_fail(TRPL_ERR_ARG, "workspace is NULL");
    if (workspace_bytes < trpl_posterior_tf_scan_workspace(S, D, K))
        return api_fail(TRPL_ERR_ARG, "workspace of %lld bytes is smaller than trpl_posterior_tf_scan_workspace(S, D, K) = %lld",
                        (long long)workspace_bytes, (long long)trpl_posterior_tf_scan_workspace(S, D, K));
    hipError_t e = post::scan::launch(LL, S, V, D, tfs, K, stats, mean, var, Q, (double *)workspace, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "posterior tf scan launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_posterior_tf_scan(const double *LL, int64_t S, const double *V, int32_t D, const double *tfs, int32_t K, double *stats,
                           double *mean, double *var, double *Q, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_scan(LL, S, V, D, tfs, tfs, K, stats, mean, var, Q)) return rc;
    if (int rc = select_device(device)) return rc;
    CallScope cs;
    HIP_TRY(cs.open());
    DevBuf dL, dV, dT, dSt, dM, dVar, dQ, ws;
    const size_t wsb = (size_t)trpl_posterior_tf_scan_workspace(S, D, K), kd = (size_t)K * D * 8;
    HIP_TRY(dL.alloc((size_t)S * 8, cs.st)); HIP_TRY(dV.alloc((size_t)S * D * 8, cs.st)); HIP_TRY(dT.alloc((size_t)K * 8, cs.st));
    HIP_TRY(dSt.alloc((size_t)K * 32, cs.st)); HIP_TRY(dM.alloc(kd, cs.st)); HIP_TRY(dVar.alloc(kd, cs.st));
    HIP_TRY(dQ.alloc(kd, cs.st)); HIP_TRY(ws.alloc(wsb, cs.st));
    HIP_TRY(hipMemcpyAsync(dL.p, LL, (size_t)S * 8, hipMemcpyHostToDevice, cs.st));
    if (D > 0) HIP_TRY(hipMemcpyAsync(dV.p, V, (size_t)S * D * 8, hipMemcpyHostToDevice, cs.st));
    HIP_TRY(hipMemcpyAsync(dT.p, tfs, (size_t)K * 8, hipMemcpyHostToDevice, cs.st));
    const double t0 = now_s();
    if (int rc = trpl_posterior_tf_scan_dev(dL.as<double>(), S, D > 0 ? dV.as<double>() : nullptr, D, dT.as<double>(), K,
                                            dSt.as<double>(), dM.as<double>(), dVar.as<double>(), dQ.as<double>(), ws.p,
                                            (int64_t)wsb, cs.st))
        return rc;
    HIP_TRY(hipStreamSynchronize(cs.st));
    if (seconds) *seconds = now_s() - t0;
    HIP_TRY(hipMemcpyAsync(stats, dSt.p, (size_t)K * 32, hipMemcpyDeviceToHost, cs.st));
    if (D > 0) {
        HIP_TRY(hipMemcpyAsync(mean, dM.p, kd, hipMemcpyDeviceToHost, cs.st));
        HIP_TRY(hipMemcpyAsync(var, dVar.p, kd, hipMemcpyDeviceToHost, cs.st));
        HIP_TRY(hipMemcpyAsync(Q, dQ.p, kd, hipMemcpyDeviceToHost, cs.st));
    }
    HIP_TRY(hipStreamSynchronize(cs.st));        // the copies back have landed (and their errors surface here)
    return TRPL_OK;
}

}  // extern "C"
