// Temperature scan of the posterior core: for K temperatures tfs[k] at once, what trpl_posterior_weights(LL, S, tfs[k])
// followed by trpl_posterior_moments(V, S, D, W_k) returns -- the maximum, the normalising sum, sum W^2, the weighted means
// and variances of the D columns and Q = sqrt(sum W^2 * variance), the objective of the reference's tf_driver
// (Visualization/utils.py:168-179) -- without ever writing a weight vector: the weights at K temperatures are K exponentials
// of the same LL[s], recomputed in registers by every phase that needs them.  With a proposal log-ratio lnr kept beside LL
// (trpl_posterior_tf_scan_lr*; a refined set, csrc/refine.hip), the same for trpl_posterior_weights_lr:
//     e_k[s] = LL[s] / tf_k - lnr[s],   m_k = nanmax_s e_k[s],   w_k[s] = exp(((e_k[s] - m_k) + 1000 ln 2) - ln S),
// so one pair (LL, lnr) serves every temperature.  Both scans are the kernels below, instantiated for the source of their
// samples (Plain or Ratio, posterior_common.hpp).
//
// Contract: row k carries the BITS of the two existing calls, and with lnr == +0.0 everywhere the scan with a ratio carries the
// bits of the scan without.  posterior_common.hpp defines what that takes: a sample belongs to the same (block, thread) as
// there, a thread adds its samples in the same order, blocks combine through the same block_reduce and the same final_reduce
// kernel.  So every (thread, temperature, column) keeps an accumulator of its own; a thread holds kTile temperatures of them
// in registers and gridDim.y covers the K / kTile tiles.
//
// Phases (each a partial kernel + final_reduce):  max and count  ->  normalising sums [K]  ->  sum W, sum W^2,
// sum W v_d [K][2 + D]  ->  central sums about those means [K][D]  ->  one small kernel forms the outputs.  The max phase is
// the one that differs by source, see its two kernels.
// Compiled with -ffp-contract=off, like posterior.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

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
    __device__ __forceinline__ int at(int j, int K) const { return k[j] < K ? k[j] : K - 1; }
};

// Without a ratio the maximum of LL / tf_k is max(LL) / tf_k (IEEE division by a positive number is monotone), so one untiled
// max phase serves all K:  part[0][b] = max of the block's LL (fmax ignores NaN, like np.nanmax), part[1][b] = its count of
// non-NaN entries
__global__ void __launch_bounds__(kThreads) max_count_partial(Plain src, int64_t S, double *part)
{
    __shared__ double sm[kThreads / 64];
    double m = -INFINITY, n = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const double ll = src.load(i);
        m = fmax(m, ll);
        if (Plain::usable(ll)) n += 1.0;
    }
    m = block_reduce<true>(m, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
    n = block_reduce<false>(n, sm);                    // whole numbers below 2^53: exact in any order
    if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = n;
}
// With a ratio the sample that leads at one temperature need not lead at another (a large LL with a large ln r wins only while
// LL / tf outweighs it), so the maximum is taken per temperature, tiled like every other phase:  part[k][b] = the block's max
// of e_k.  The count of usable samples is the same at every temperature: tile 0 leaves the block's in cnt[b]
__global__ void __launch_bounds__(kThreads) tiled_max_count_partial(Ratio src, int64_t S, const double *tfs, int K, double *part,
                                                                    double *cnt)
{
    __shared__ double sm[kThreads / 64];
    const Tile t(tfs, K);
    double m[kTile], n = 0.0;
#pragma unroll
    for (int j = 0; j < kTile; j++) m[j] = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const Ratio::Sample x = src.load(i);
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            double lost;                     // not needed for the maximum
            m[j] = fmax(m[j], Ratio::exponent(x, t.tf[j], lost));
        }
        if (Ratio::usable(x)) n += 1.0;
    }
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        const double r = block_reduce<true>(m[j], sm);
        if (threadIdx.x == 0 && t.k[j] < K) part[(int64_t)t.k[j] * gridDim.x + blockIdx.x] = r;
    }
    n = block_reduce<false>(n, sm);                    // whole numbers below 2^53: exact in any order
    if (threadIdx.x == 0 && blockIdx.y == 0) cnt[blockIdx.x] = n;
}
// the maximum of the exponent at tf = tfs[k], from what the source's max phase left in mx: max(LL), or the K maxima
__device__ __forceinline__ double max_at(Plain, const double *mx, double tf, int) { return mx[0] / tf; }
__device__ __forceinline__ double max_at(Ratio, const double *mx, double, int k) { return mx[k]; }

// part[k][b] = the block's nansum of the unnormalised weights at tfs[k]
template <class Src>
__global__ void __launch_bounds__(kThreads) weights_partial(Src src, int64_t S, const double *tfs, int K, const double *mx,
                                                            double c_up, double c_size, double *part)
{
    __shared__ double sm[kThreads / 64];
    const Tile t(tfs, K);
    double m[kTile], acc[kTile];
#pragma unroll
    for (int j = 0; j < kTile; j++) { m[j] = max_at(src, mx, t.tf[j], t.at(j, K)); acc[j] = 0.0; }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const auto x = src.load(i);
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const double w = tempered_weight<Src>(x, t.tf[j], m[j], c_up, c_size);
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
template <class Src>
__global__ void __launch_bounds__(kThreads) moments1_partial(Src src, const double *V, int64_t S, int D, const double *tfs, int K,
                                                             const double *mx, const double *norm, double c_up, double c_size,
                                                             double *part)
{
    __shared__ double sm[kThreads / 64];
    const Tile t(tfs, K);
    double m[kTile], s[kTile], sw[kTile], sw2[kTile], sv[kTile][kMaxDim];
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        m[j] = max_at(src, mx, t.tf[j], t.at(j, K));
        s[j] = norm[t.at(j, K)];
        sw[j] = 0.0; sw2[j] = 0.0;
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) sv[j][d] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const auto x = src.load(i);
        double v[kMaxDim];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) v[d] = d < D ? V[(int64_t)d * S + i] : 0.0;      // wave-uniform
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const double w = tempered_weight<Src>(x, t.tf[j], m[j], c_up, c_size) / s[j];     // utils.py:165
            sw[j] += w;
            sw2[j] += w * w;
#pragma unroll
            for (int d = 0; d < kMaxDim; d++) sv[j][d] += v[d] * w;
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
template <class Src>
__global__ void __launch_bounds__(kThreads) moments2_partial(Src src, const double *V, int64_t S, int D, const double *tfs, int K,
                                                             const double *mx, const double *norm, const double *sums,
                                                             double c_up, double c_size, double *part)
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
        m[j] = max_at(src, mx, t.tf[j], t.at(j, K));
        s[j] = norm[t.at(j, K)];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) c[j][d] = 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < S; i += (int64_t)gridDim.x * kThreads) {
        const auto x = src.load(i);
        double v[kMaxDim];
#pragma unroll
        for (int d = 0; d < kMaxDim; d++) v[d] = d < D ? V[(int64_t)d * S + i] : 0.0;
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const double w = tempered_weight<Src>(x, t.tf[j], m[j], c_up, c_size) / s[j];
#pragma unroll
            for (int d = 0; d < kMaxDim; d++) {
                const double vc = v[d] - mean[j][d];
                c[j][d] += (vc * vc) * w;
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

// one thread per (k, d), d == D being the statistics of temperature k: stats[K][4] without a ratio, [K][6] with one
template <class Src>
__global__ void finish_kernel(const double *tfs, int K, int D, const double *mx, const double *cnt, const double *norm,
                              const double *sums, const double *central, double *stats, double *mean, double *var, double *Q)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = idx / (D + 1), d = idx % (D + 1);
    if (k >= K) return;
    const double *row = sums + (int64_t)k * (2 + D);
    if (d == D) {
        const double m = max_at(Src{}, mx, tfs[k], k);
        if constexpr (std::is_same<Src, Plain>::value) {
            stats[4 * k + 0] = m;
            stats[4 * k + 1] = norm[k];
            stats[4 * k + 2] = row[1];
            stats[4 * k + 3] = cnt[0];
        } else {
            stats[6 * k + 0] = m;
            stats[6 * k + 1] = norm[k];
            stats[6 * k + 2] = row[0];
            stats[6 * k + 3] = row[1];
            stats[6 * k + 4] = cnt[0];
            stats[6 * k + 5] = (row[0] * row[0]) / row[1];                // the effective sample size
        }
        return;
    }
    const double v = central[(int64_t)k * D + d] / row[0];            // w_variance, utils.py:202-204
    mean[(int64_t)k * D + d] = row[2 + d] / row[0];                   // w_mean, utils.py:197-199
    var[(int64_t)k * D + d] = v;
    Q[(int64_t)k * D + d] = sqrt(row[1] * v);                         // w_sample_var, utils.py:168-170
}

// doubles of workspace: the block partials [K][kMaxBlocks][2 + D] (the max phase keeps its count partials behind its rows of
// maxima: nb + nb and K nb + nb are both <= 2 K kMaxBlocks), then max (one, or [K] with a ratio), count, norm[K],
// sums[K][2 + D], central[K][D]
inline size_t part_doubles(int D, int K) { return (size_t)K * kMaxBlocks * (2 + D); }
inline size_t workspace_doubles(int D, int K, bool ratio)
{
    return part_doubles(D, K) + (ratio ? K : 1) + 1 + (size_t)K * (1 + 2 + D + D) + 64;
}

template <class Src>
hipError_t launch(Src src, int64_t S, const double *V, int D, const double *tfs, int K, double *stats, double *mean, double *var,
                  double *Q, double *ws, hipStream_t st)
{
    constexpr bool ratio = std::is_same<Src, Ratio>::value;
    const int nb = grid_for(S), nmax = ratio ? K : 1;
    const dim3 tiles(nb, (K + kTile - 1) / kTile);
    double *part = ws, *mx = ws + part_doubles(D, K), *cnt = mx + nmax, *norm = cnt + 1, *sums = norm + K,
           *central = sums + (size_t)K * (2 + D);
    double *cnt_part = part + (size_t)nmax * nb;
    const double c_up = 1000.0 * log(2.0), c_size = log((double)S);                   // utils.py:164
    if constexpr (ratio) hipLaunchKernelGGL(tiled_max_count_partial, tiles, dim3(kThreads), 0, st, src, S, tfs, K, part, cnt_part);
    else                 hipLaunchKernelGGL(max_count_partial, dim3(nb), dim3(kThreads), 0, st, src, S, part);
    hipLaunchKernelGGL(final_reduce, dim3(1, nmax), dim3(kThreads), 0, st, part, nb, 1, true, mx);
    hipLaunchKernelGGL(final_reduce, dim3(1, 1), dim3(kThreads), 0, st, cnt_part, nb, 1, false, cnt);
    hipLaunchKernelGGL(weights_partial<Src>, tiles, dim3(kThreads), 0, st, src, S, tfs, K, mx, c_up, c_size, part);
    hipLaunchKernelGGL(final_reduce, dim3(1, K), dim3(kThreads), 0, st, part, nb, 1, false, norm);
    hipLaunchKernelGGL(moments1_partial<Src>, tiles, dim3(kThreads), 0, st, src, V, S, D, tfs, K, mx, norm, c_up, c_size, part);
    hipLaunchKernelGGL(final_reduce, dim3(2 + D, K), dim3(kThreads), 0, st, part, nb, 2 + D, false, sums);
    if (D > 0) {
        hipLaunchKernelGGL(moments2_partial<Src>, tiles, dim3(kThreads), 0, st, src, V, S, D, tfs, K, mx, norm, sums, c_up, c_size,
                           part);
        hipLaunchKernelGGL(final_reduce, dim3(D, K), dim3(kThreads), 0, st, part, nb, D, false, central);
    }
    const int n = K * (D + 1);
    hipLaunchKernelGGL(finish_kernel<Src>, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, tfs, K, D, mx, cnt, norm,
                       sums, central, stats, mean, var, Q);
    return hipGetLastError();
}

}  // namespace scan
}  // namespace post
}  // namespace trpl

using namespace trpl;

// The entry points with and without a ratio (`ratio`: the _lr ones, which take lnr) share everything below.
// What all forms refuse before a device is touched; tfs_host: the temperatures where the caller's pointer is host memory
static int check_scan(const void *LL, const void *lnr, bool ratio, int64_t S, const void *V, int32_t D, const double *tfs,
                      const double *tfs_host, int32_t K, const void *stats, const void *mean, const void *var, const void *Q)
{
    if (S < 1) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 1", (long long)S);
    if (D < 0 || D > post::kMaxDim) return api_fail(TRPL_ERR_ARG, "D=%d must be in [0, %d]", D, post::kMaxDim);
    if (K < 1 || K > TRPL_TF_SCAN_MAX) return api_fail(TRPL_ERR_ARG, "K=%d must be in [1, TRPL_TF_SCAN_MAX = %d]", K, TRPL_TF_SCAN_MAX);
    if (!LL) return api_fail(TRPL_ERR_ARG, "LL is NULL");
    if (ratio && !lnr) return api_fail(TRPL_ERR_ARG, "lnr is NULL");
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

static int64_t scan_workspace(int64_t S, int32_t D, int32_t K, bool ratio)
{
    if (S < 1 || D < 0 || D > post::kMaxDim || K < 1 || K > TRPL_TF_SCAN_MAX) return 0;
    return (int64_t)(sizeof(double) * post::scan::workspace_doubles(D, K, ratio));
}

// the device form
static int scan_dev(const double *LL, const double *lnr, bool ratio, int64_t S, const double *V, int32_t D, const double *tfs,
                    int32_t K, double *stats, double *mean, double *var, double *Q, void *workspace, int64_t workspace_bytes,
                    void *stream)
{
    if (int rc = check_scan(LL, lnr, ratio, S, V, D, tfs, nullptr, K, stats, mean, var, Q)) return rc;
    if (!workspace) return api_fail(TRPL_ERR_ARG, "workspace is NULL");
    if (workspace_bytes < scan_workspace(S, D, K, ratio))
        return api_fail(TRPL_ERR_ARG, "workspace of %lld bytes is smaller than trpl_posterior_tf_scan%s_workspace(S, D, K) = %lld",
                        (long long)workspace_bytes, ratio ? "_lr" : "", (long long)scan_workspace(S, D, K, ratio));
    double *ws = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = ratio ? post::scan::launch(post::Ratio{LL, lnr}, S, V, D, tfs, K, stats, mean, var, Q, ws, st)
                         : post::scan::launch(post::Plain{LL}, S, V, D, tfs, K, stats, mean, var, Q, ws, st);
    if (e != hipSuccess)
        return api_fail(TRPL_ERR_HIP, "posterior tf scan%s launch: %s", ratio ? " (log-ratio)" : "", hipGetErrorString(e));
    return TRPL_OK;
}

// the host-buffer form: stages the inputs, runs the device form, copies the outputs back
static int scan_staged(const double *LL, const double *lnr, bool ratio, int64_t S, const double *V, int32_t D, const double *tfs,
                       int32_t K, double *stats, double *mean, double *var, double *Q, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_scan(LL, lnr, ratio, S, V, D, tfs, tfs, K, stats, mean, var, Q)) return rc;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const size_t wsb = (size_t)scan_workspace(S, D, K, ratio), kd = (size_t)K * D;
    const double *dL = sg.in(LL, (size_t)S), *dR = ratio ? sg.in(lnr, (size_t)S) : nullptr, *dV = sg.in(V, (size_t)S * D);
    const double *dT = sg.in(tfs, (size_t)K);
    double *dSt = sg.out(stats, (size_t)K * (ratio ? 6 : 4)), *dM = sg.out(mean, kd), *dVar = sg.out(var, kd), *dQ = sg.out(Q, kd);
    void *ws = sg.scratch(wsb);
    if (int rc = sg.begin()) return rc;
    if (int rc = scan_dev(dL, dR, ratio, S, D > 0 ? dV : nullptr, D, dT, K, dSt, dM, dVar, dQ, ws, (int64_t)wsb, sg.stream())) return rc;
    return sg.finish(seconds);
}

extern "C" {

int64_t trpl_posterior_tf_scan_workspace(int64_t S, int32_t D, int32_t K) { return scan_workspace(S, D, K, false); }
int64_t trpl_posterior_tf_scan_lr_workspace(int64_t S, int32_t D, int32_t K) { return scan_workspace(S, D, K, true); }

int trpl_posterior_tf_scan_dev(const double *LL, int64_t S, const double *V, int32_t D, const double *tfs, int32_t K,
                               double *stats, double *mean, double *var, double *Q, void *workspace, int64_t workspace_bytes,
                               void *stream)
{
    return scan_dev(LL, nullptr, false, S, V, D, tfs, K, stats, mean, var, Q, workspace, workspace_bytes, stream);
}
int trpl_posterior_tf_scan_lr_dev(const double *LL, const double *lnr, int64_t S, const double *V, int32_t D, const double *tfs,
                                  int32_t K, double *stats, double *mean, double *var, double *Q, void *workspace,
                                  int64_t workspace_bytes, void *stream)
{
    return scan_dev(LL, lnr, true, S, V, D, tfs, K, stats, mean, var, Q, workspace, workspace_bytes, stream);
}

int trpl_posterior_tf_scan(const double *LL, int64_t S, const double *V, int32_t D, const double *tfs, int32_t K, double *stats,
                           double *mean, double *var, double *Q, int32_t device, double *seconds)
{
    return scan_staged(LL, nullptr, false, S, V, D, tfs, K, stats, mean, var, Q, device, seconds);
}
int trpl_posterior_tf_scan_lr(const double *LL, const double *lnr, int64_t S, const double *V, int32_t D, const double *tfs,
                              int32_t K, double *stats, double *mean, double *var, double *Q, int32_t device, double *seconds)
{
    return scan_staged(LL, lnr, true, S, V, D, tfs, K, stats, mean, var, Q, device, seconds);
}

}  // extern "C"
