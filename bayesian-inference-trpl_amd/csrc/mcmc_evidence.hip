// The sums of the log-evidence estimates of a tempered run (trpl_mcmc_evidence_sums*, include/trpl.h): from the
// kept LL [K][n][C] of the K rungs, over the steps [t0, t1) cut into B blocks of w consecutive steps, the extrema of every rung and,
// per (rung, block), the sum of LL, the two stepping-stone sums towards the neighbouring rungs with their squares, and the count.
// What the estimator on top (trpl_amd.mcmc.log_evidence_ratios) needs of a history, in two passes over it and no other solve.
//
//   evidence_extrema_block_kernel   pass 1a, one workgroup per (k, b): the maximum and the minimum of the block's w C values, NaN when
//       one of them is NaN, left in slots 0 and 1 of the block's own row of `sums` -- the outputs are the only memory the call owns.
//   evidence_extrema_kernel         pass 1b, one workgroup per rung: the extrema over the rung's B rows -> ext [K][2].  Maximum and
//       minimum do not depend on the order but for the sign of a zero, and a zero extremum is stored as +0.0 (m + 0.0).
//   evidence_sums_kernel            pass 2, one workgroup per (k, b), after ext is final: the six sums of the block.  Thread j adds the
//       elements j, j + 256, .. of the block in (t, c) row-major order, ascending from +0.0; the 256 partials are added by the halving
//       tree p[j] = p[j] + p[j + s], s = 128 .. 1, in LDS: the association is a function of (w, C) alone.  No atomics.
// The term of a value x with coefficient c and centre a (evidence_term): exp(c * (x - a)), the subtraction and the product one
// rounding each; x = -inf is never put through the expression, it gives +0.0 for c >= 0 and +inf for c < 0; c = +-0.0 gives 1.0 for
// every x above -inf, which is the expression's value wherever it has one.  A rung with a NaN has NaN extrema, and every sum of
// every block of it is NaN.
// Adjacent threads read adjacent addresses; nothing outside the rows [t0, t1) is read and nothing outside ext and sums is written.
// Compiled with -ffp-contract=off like mcmc.hip: every result is its expression with one rounding per operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "mcmc_common.hpp"
#include "refine_common.hpp"

namespace trpl {
namespace mcmc {

using refine::kThreads;

constexpr int kEvidenceSums = TRPL_MCMC_EVIDENCE_SUMS;           // the columns of a row of `sums`

// p[j] = op(p[j], p[j + s]), s = 128 .. 1, on NV arrays of kThreads values at once; the result is p[v][0], read after the last barrier
template <int NV, class Op>
__device__ __forceinline__ void halving_tree(double (&p)[NV][kThreads], Op op)
{
    const int j = threadIdx.x;
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s >>= 1) {
        if (j < s) {
#pragma unroll
            for (int v = 0; v < NV; v++) p[v][j] = op(v, p[v][j], p[v][j + s]);
        }
        __syncthreads();
    }
}

// slot 0 is a maximum, slot 1 a minimum, slot 2 the number of NaN seen (a sum of small integers: exact)
struct ExtremaOp {
    __device__ double operator()(int v, double a, double b) const { return v == 0 ? (b > a ? b : a) : v == 1 ? (b < a ? b : a) : a + b; }
};
struct SumOp {
    __device__ double operator()(int, double a, double b) const { return a + b; }
};

__global__ void __launch_bounds__(kThreads) evidence_extrema_block_kernel(const double *LL, int64_t n, int64_t C, int64_t t0, int64_t B,
                                                                          int64_t w, double *sums)
{
    __shared__ double p[3][kThreads];
    const int64_t kb = blockIdx.x, k = kb / B, b = kb % B;
    const double *x = LL + ((k * n + t0) + b * w) * C;
    const int64_t m = w * C;
    double mx = -INFINITY, mn = INFINITY, bad = 0.0;
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < m; i += kThreads) {
        const double v = x[i];
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
        bad = v != v ? 1.0 : bad;
    }
    p[0][threadIdx.x] = mx;
    p[1][threadIdx.x] = mn;
    p[2][threadIdx.x] = bad;
    halving_tree(p, ExtremaOp());
    if (threadIdx.x == 0) {
        const bool nan = p[2][0] > 0.0;
        sums[kb * kEvidenceSums + 0] = nan ? NAN : p[0][0];
        sums[kb * kEvidenceSums + 1] = nan ? NAN : p[1][0];
    }
}

__global__ void __launch_bounds__(kThreads) evidence_extrema_kernel(const double *sums, int64_t B, double *ext)
{
    __shared__ double p[3][kThreads];
    const int64_t k = blockIdx.x;
    double mx = -INFINITY, mn = INFINITY, bad = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += kThreads) {
        const double hi = sums[(k * B + b) * kEvidenceSums + 0], lo = sums[(k * B + b) * kEvidenceSums + 1];
        mx = hi > mx ? hi : mx;
        mn = lo < mn ? lo : mn;
        bad = hi != hi ? 1.0 : bad;
    }
    p[0][threadIdx.x] = mx;
    p[1][threadIdx.x] = mn;
    p[2][threadIdx.x] = bad;
    halving_tree(p, ExtremaOp());
    if (threadIdx.x == 0) {
        const bool nan = p[2][0] > 0.0;
        ext[2 * k + 0] = nan ? NAN : p[0][0] + 0.0;             // a zero extremum is +0.0 whatever the order found
        ext[2 * k + 1] = nan ? NAN : p[1][0] + 0.0;
    }
}

__device__ __forceinline__ double evidence_term(double x, double c, double a)
{
    if (c == 0.0) return x > -INFINITY ? 1.0 : 0.0;
    if (x == -INFINITY) return c < 0.0 ? INFINITY : 0.0;
    return exp(c * (x - a));
}

__global__ void __launch_bounds__(kThreads) evidence_sums_kernel(const double *LL, int32_t K, int64_t n, int64_t C, int64_t t0, int64_t B,
                                                                 int64_t w, const Ladder tf, const double *ext, double *sums)
{
    __shared__ double p[kEvidenceSums][kThreads];
    const int64_t kb = blockIdx.x, b = kb % B;
    const int32_t k = (int32_t)(kb / B);
    double *out = sums + kb * kEvidenceSums;
    const double hi = ext[2 * k + 0], lo = ext[2 * k + 1];
    if (hi != hi) {                                              // a NaN in the rung: every sum of every block of it
        if (threadIdx.x < kEvidenceSums) out[threadIdx.x] = NAN;
        return;
    }
    const bool has_up = k > 0, has_down = k + 1 < K;
    // delta_k = 1 / tf[k] - 1 / tf[k + 1], swap_kernel's expression; up has the coefficient delta_{k - 1}, down -delta_k
    const double cu = has_up ? 1.0 / tf.tf[k - 1] - 1.0 / tf.tf[k] : 0.0;
    const double cd = has_down ? -(1.0 / tf.tf[k] - 1.0 / tf.tf[k + 1]) : 0.0;
    const double au = cu >= 0.0 ? hi : lo;                       // the exponent is never positive
    const double ad = cd <= 0.0 ? lo : hi;                       // delta_k >= 0: the minimum
    const double *x = LL + (((int64_t)k * n + t0) + b * w) * C;
    const int64_t m = w * C;
    double sx = 0.0, up = 0.0, up2 = 0.0, dn = 0.0, dn2 = 0.0, cnt = 0.0;
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < m; i += kThreads) {
        const double v = x[i];
        sx = sx + v;
        cnt = cnt + (v > -INFINITY ? 1.0 : 0.0);
        if (has_up) {
            const double e = evidence_term(v, cu, au);
            up = up + e;
            up2 = up2 + e * e;
        }
        if (has_down) {
            const double e = evidence_term(v, cd, ad);
            dn = dn + e;
            dn2 = dn2 + e * e;
        }
    }
    p[0][threadIdx.x] = sx;
    p[1][threadIdx.x] = up;
    p[2][threadIdx.x] = up2;
    p[3][threadIdx.x] = dn;
    p[4][threadIdx.x] = dn2;
    p[5][threadIdx.x] = cnt;
    halving_tree(p, SumOp());
    if (threadIdx.x < kEvidenceSums) out[threadIdx.x] = p[threadIdx.x][0];
}

}  // namespace mcmc
}  // namespace trpl

using namespace trpl;

namespace {                                                      // the host half: mcmc.hip's file comment has its structure

struct EvidenceCall {
    const double *LL; int32_t K; int64_t n, C, t0, t1, B; const double *tf; double *ext, *sums;
    mcmc::Ladder lad = {};
};

// every refusal of the call, before a device is touched; copies the ladder into the kernel argument
int check(EvidenceCall &k)
{
    if (int rc = check_not_null({{"LL", k.LL}, {"tf", k.tf}, {"ext", k.ext}, {"sums", k.sums}})) return rc;
    if (k.K < 1 || k.K > TRPL_MCMC_MAX_RUNGS) return api_fail(TRPL_ERR_ARG, "K=%d must be in [1, %d]", k.K, TRPL_MCMC_MAX_RUNGS);
    if (k.n < 1) return api_fail(TRPL_ERR_ARG, "n=%lld must be >= 1", (long long)k.n);
    if (k.C < 1) return api_fail(TRPL_ERR_ARG, "C=%lld must be >= 1", (long long)k.C);
    if (k.C > (INT64_MAX >> 3) / k.n / k.K)
        return api_fail(TRPL_ERR_ARG, "n=%lld steps of C=%lld values on K=%d rungs are more than 2^60 - 1 values", (long long)k.n, (long long)k.C, k.K);
    if (!(0 <= k.t0 && k.t0 < k.t1 && k.t1 <= k.n))
        return api_fail(TRPL_ERR_ARG, "t0=%lld, t1=%lld: the range must satisfy 0 <= t0 < t1 <= n=%lld", (long long)k.t0, (long long)k.t1,
                        (long long)k.n);
    if (k.B < 1 || (k.t1 - k.t0) % k.B)
        return api_fail(TRPL_ERR_ARG, "B=%lld must be >= 1 and divide t1 - t0 = %lld", (long long)k.B, (long long)(k.t1 - k.t0));
    for (int r = 0; r < k.K; r++) {
        if (!(isfinite(k.tf[r]) && k.tf[r] > 0.0)) return api_fail(TRPL_ERR_ARG, "tf[%d]=%g must be finite and > 0", r, k.tf[r]);
        k.lad.tf[r] = k.tf[r];
    }
    if (k.B > kRefineMaxBlocks / k.K)
        return api_fail(TRPL_ERR_ARG, "B=%lld blocks on K=%d rungs are more than 2^31 - 1 workgroups", (long long)k.B, k.K);
    return TRPL_OK;
}

int launch(const EvidenceCall &k, hipStream_t stream)
{
    const int64_t w = (k.t1 - k.t0) / k.B;
    const dim3 grid((unsigned)(k.K * k.B)), block(refine::kThreads);
    hipLaunchKernelGGL(mcmc::evidence_extrema_block_kernel, grid, block, 0, stream, k.LL, k.n, k.C, k.t0, k.B, w, k.sums);
    hipLaunchKernelGGL(mcmc::evidence_extrema_kernel, dim3((unsigned)k.K), block, 0, stream, k.sums, k.B, k.ext);
    hipLaunchKernelGGL(mcmc::evidence_sums_kernel, grid, block, 0, stream, k.LL, k.K, k.n, k.C, k.t0, k.B, w, k.lad, k.ext, k.sums);
    return refine_launched("mcmc evidence sums");
}

// the steps of the range only, compact on the device: [K][t1 - t0][C]
void stage(EvidenceCall &k, Staged &sg)
{
    const int64_t steps = k.t1 - k.t0;
    k.LL = sg.in(k.LL + k.t0 * k.C, (size_t)(k.n * k.C), (size_t)(steps * k.C), (size_t)k.K);
    k.n = steps;
    k.t0 = 0;
    k.t1 = steps;
    k.ext = sg.out(k.ext, (size_t)k.K * 2);
    k.sums = sg.out(k.sums, (size_t)(k.K * k.B) * mcmc::kEvidenceSums);
}

}  // namespace

extern "C" {

int trpl_mcmc_evidence_sums_dev(const double *LL, int32_t K, int64_t n, int64_t C, int64_t t0, int64_t t1, int64_t B, const double *tf,
                                double *ext, double *sums, void *stream)
{
    return on_stream(EvidenceCall{LL, K, n, C, t0, t1, B, tf, ext, sums}, stream);
}

int trpl_mcmc_evidence_sums(const double *LL, int32_t K, int64_t n, int64_t C, int64_t t0, int64_t t1, int64_t B, const double *tf,
                            double *ext, double *sums, int32_t device, double *seconds)
{
    return staged(EvidenceCall{LL, K, n, C, t0, t1, B, tf, ext, sums}, device, seconds);
}

}  // extern "C"
