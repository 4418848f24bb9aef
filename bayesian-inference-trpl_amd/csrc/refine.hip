// Refinement generations (trpl_refine_*, include/trpl.h): draw a further generation of samples around the posterior of the ones
// at hand and weight the union exactly.  All sampling happens in UNIT coordinates: an active column of the parameter box maps to
// u in [0, 1] (linear, or linear in log10), the prior is uniform on the cube.
//
//   unit_kernel        X -> U for existing samples, one thread per sample (device log10: not bit-pinned).
//   chunk_sums_kernel, chunk_prefix_kernel, resample_kernel    systematic resampling.  The cumulative weight is ONE function of S:
//       a chunk is kChunk = kThreads * kRows rows; thread t of a chunk adds its kRows consecutive rows one after the other
//       (partial sums s_0 .. s_15), thread 0 adds the 256 thread totals one after the other (bases b_0 = 0, b_t+1 = b_t + total_t,
//       chunk total T = b_256), one thread adds the chunk totals one after the other (prefix p_0 = 0, p_c+1 = p_c + T_c), and
//           cum[i] = p_c + (b_t + s_j)      for row i = c * kChunk + t * kRows + j.
//       Every level adds non-negative terms in a fixed order and rounding is monotone, so cum never decreases in i, and the last
//       cum of a chunk IS p_c+1, bit for bit; a row of weight 0 leaves cum where it was.  resample_kernel: one workgroup per
//       chunk finds the draws whose threshold lies in [p_c, p_c+1) by bisection over k (thresholds rise with k), rebuilds the
//       chunk's cum in LDS and bisects it for each of them.  No atomics; nothing depends on the grid or the schedule.
//   draw_kernel        one thread per child: Philox4x32-10 (Salmon et al. 2011) keyed by the seed, counter (child, call, generation),
//       two 53-bit uniforms per call in the sampler's genrand_res53 form, u = min(b, a + (b - a) * xi), then X by the sampler's
//       expressions.
//   density_kernel<A>  B[s] = sum over the parents k whose closed box holds u_s of inv_vol[k], one thread per sample, the parents
//       staged through LDS in tiles of kTile as (a, b) pairs (one 16-byte read per dimension, the same address in every lane of a
//       wave: a broadcast, no bank conflict), the sum taken in ascending k with one fp64 add per member box starting from
//       +0.0: the plain sequential loop, bit for bit.  A lane leaves a box at its first failing dimension, but that is
//       predication inside an unrolled loop: the wave goes on reading the box's dimensions from LDS while ANY of its 64 lanes is
//       still inside, so what is saved is the compares of the lanes that left, and the reads only once all of them have.
// Compiled with -ffp-contract=off like posterior.hip and corner.hip: every result is its expression with one rounding per operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "refine_common.hpp"

namespace trpl {
namespace refine {

constexpr int kRows = 16;                                        // consecutive rows one thread adds
constexpr int kChunk = kThreads * kRows;                         // rows of one chunk: 32 KiB of cumulative weights in LDS
constexpr int kTile = 128;                                       // parents per LDS tile: (2 * 16 + 1) * 8 * 128 = 33 KiB at A = 16
constexpr int kPrefixTile = 1024;                                // chunk totals staged per round of the prefix kernel

__device__ __forceinline__ double used(double w) { return w > 0.0 ? w : 0.0; }      // NaN and <= 0 count as 0

// the chunk's thread-level sums: w[j] = this thread's j-th row as it counts, part[j] = its running sum after that row; s_tot[t] <-
// the base of thread t, s_tot[256] <- the chunk total.  The rows are read once; a caller that needs only one of w and part leaves
// the other to the compiler.
__device__ __forceinline__ void chunk_partials(const double *W, int64_t S, int64_t c, double (&w)[kRows], double (&part)[kRows], double *s_tot)
{
    const int t = threadIdx.x;
    const int64_t i0 = c * kChunk + (int64_t)t * kRows;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kRows; j++) {
        w[j] = i0 + j < S ? used(W[i0 + j]) : 0.0;
        s = s + w[j];
        part[j] = s;
    }
    s_tot[t] = s;
    __syncthreads();
    if (t == 0) {
        double base = 0.0;
        for (int k = 0; k < kThreads; k++) {
            const double v = s_tot[k];
            s_tot[k] = base;
            base = base + v;
        }
        s_tot[kThreads] = base;
    }
    __syncthreads();
}

constexpr double kNoExponent = -1.0e9;                           // a chunk without weight

// The sum of squares is kept as a pair: ex = the binary exponent of the chunk's largest weight, sq = sum (w * 2^-ex)^2 in the order of
// the sums (a thread's rows, then the threads).  Scaling by a power of two is exact, the largest term is in [1, 4), so neither a
// vector of weights near 1e-200 nor one near 1e+200 loses its sum of squares -- and the effective sample size, a ratio, with it.
__global__ void __launch_bounds__(kThreads) chunk_sums_kernel(const double *W, int64_t S, double *tot, double *sq, double *ex)
{
    __shared__ double s_tot[kThreads + 1], s_sq[kThreads + 1];
    double w[kRows], part[kRows];
    chunk_partials(W, S, blockIdx.x, w, part, s_tot);
    const int t = threadIdx.x;
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < kRows; j++) mx = w[j] > mx ? w[j] : mx;
    s_sq[t] = mx;
    __syncthreads();
    if (t == 0) {
        double m = 0.0;
        for (int k = 0; k < kThreads; k++) m = s_sq[k] > m ? s_sq[k] : m;
        s_sq[kThreads] = m;
    }
    __syncthreads();
    const double m = s_sq[kThreads];
    __syncthreads();                                             // everyone has read the maximum before s_sq is written again
    const int e = m > 0.0 ? ilogb(m) : 0;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < kRows; j++) {
        const double v = ldexp(w[j], -e);
        q = q + v * v;
    }
    s_sq[t] = q;
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int k = 0; k < kThreads; k++) sum = sum + s_sq[k];
        tot[blockIdx.x] = s_tot[kThreads];
        sq[blockIdx.x] = sum;
        ex[blockIdx.x] = m > 0.0 ? (double)e : kNoExponent;
    }
}

// one workgroup: prefix[0] = 0, prefix[c + 1] = prefix[c] + tot[c], one add after the other; the chunks' scaled sums of squares are
// brought to the largest exponent E and added one after the other; stats = {sw, sum w^2, sw^2 / sum w^2}, the ratio formed from the
// scaled numbers
__global__ void __launch_bounds__(kThreads) chunk_prefix_kernel(const double *tot, const double *sq, const double *ex, int64_t nchunks,
                                                                double *prefix, double *stats)
{
    __shared__ double s_t[kPrefixTile], s_q[kPrefixTile];
    __shared__ double s_carry[3];
    double emax = kNoExponent;
    for (int64_t c = threadIdx.x; c < nchunks; c += kThreads) emax = ex[c] > emax ? ex[c] : emax;
    s_q[threadIdx.x] = emax;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = kNoExponent;
        for (int k = 0; k < kThreads; k++) m = s_q[k] > m ? s_q[k] : m;
        s_carry[0] = 0.0; s_carry[1] = 0.0; s_carry[2] = m; prefix[0] = 0.0;
    }
    __syncthreads();
    const double E = s_carry[2];
    for (int64_t c0 = 0; c0 < nchunks; c0 += kPrefixTile) {
        const int n = (int)(nchunks - c0 < kPrefixTile ? nchunks - c0 : kPrefixTile);
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += kThreads) {
            s_t[e] = tot[c0 + e];
            const double d = 2.0 * (ex[c0 + e] - E);             // <= 0; a chunk without weight has sq = 0
            s_q[e] = d < -2200.0 ? 0.0 : ldexp(sq[c0 + e], (int)d);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double p = s_carry[0], q = s_carry[1];
            for (int e = 0; e < n; e++) {
                p = p + s_t[e];
                q = q + s_q[e];
                s_t[e] = p;
            }
            s_carry[0] = p; s_carry[1] = q;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += kThreads) prefix[c0 + 1 + e] = s_t[e];
    }
    __syncthreads();
    if (threadIdx.x == 0 && stats) {
        const double sw = s_carry[0], q = s_carry[1];
        const int e = q > 0.0 ? (int)E : 0;
        const double sws = ldexp(sw, -e);
        stats[0] = sw; stats[1] = ldexp(q, 2 * e); stats[2] = q > 0.0 ? sws * sws / q : 0.0;
    }
}

// threshold of draw k: (k + offset) / K * sw, left to right; one that rounds up to sw is the largest double below sw, so that
// every draw has a row.  Non-decreasing in k.
__device__ __forceinline__ double threshold(int64_t k, double offset, int64_t K, double sw)
{
    const double t = ((double)k + offset) / (double)K * sw;
    return t < sw ? t : __longlong_as_double(__double_as_longlong(sw) - 1);
}
// first k in [0, K] whose threshold is >= v (K: none)
__device__ __forceinline__ int64_t first_draw_at(double v, double offset, int64_t K, double sw)
{
    int64_t lo = 0, hi = K;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (threshold(mid, offset, K, sw) >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kThreads) resample_kernel(const double *W, int64_t S, int64_t K, double offset, const double *prefix,
                                                            int64_t nchunks, int64_t *idx)
{
    __shared__ double s_cum[kChunk];
    __shared__ double s_tot[kThreads + 1];
    const int64_t c = blockIdx.x;
    const double sw = prefix[nchunks];
    if (!(sw > 0.0)) {                                           // no weight at all: every draw is -1
        if (c == 0) for (int64_t k = threadIdx.x; k < K; k += kThreads) idx[k] = -1;
        return;
    }
    if (c >= nchunks) return;
    const double p0 = prefix[c], p1 = prefix[c + 1];
    if (!(p1 > p0)) return;                                      // a chunk without weight holds no draw
    const int64_t k0 = first_draw_at(p0, offset, K, sw), k1 = first_draw_at(p1, offset, K, sw);
    if (k0 >= k1) return;                                        // the same in every thread
    double w[kRows], part[kRows];
    chunk_partials(W, S, c, w, part, s_tot);
    const double base = s_tot[threadIdx.x];
#pragma unroll
    for (int j = 0; j < kRows; j++) s_cum[threadIdx.x * kRows + j] = p0 + (base + part[j]);
    __syncthreads();
    for (int64_t k = k0 + threadIdx.x; k < k1; k += kThreads) {
        const double t = threshold(k, offset, K, sw);
        int lo = 0, hi = kChunk - 1;                             // s_cum[kChunk - 1] == p1 > t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_cum[mid] > t) hi = mid; else lo = mid + 1;
        }
        idx[k] = c * kChunk + lo;                                // its weight is > 0 (cum rose there), so it is a row below S
    }
}

// Philox4x32-10, genrand_res53 and the expressions of a row of X: refine_common.hpp, shared with the oriented draw
__global__ void __launch_bounds__(kThreads) draw_kernel(const double *a, const double *b, int64_t K, int64_t n_uniform, int64_t total,
                                                        uint32_t seed_lo, uint32_t seed_hi, uint32_t generation, const Box bx, double *U2,
                                                        double *X2)
{
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (n >= total) return;
    const bool uni = n < n_uniform;
    const int64_t par = uni ? 0 : (n - n_uniform) % K;
    const double *pa = a + par * bx.A, *pb = b + par * bx.A;
    double *row = X2 + n * bx.ncol;
    put_fixed(bx, row);
    for (int j = 0; 2 * j < bx.A; j++) {
        uint32_t r[4];
        philox4x32_10((uint32_t)n, (uint32_t)((uint64_t)n >> 32), (uint32_t)j, generation, seed_lo, seed_hi, r);
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int d = 2 * j + e;
            if (d >= bx.A) break;
            const double xi = res53(r[2 * e], r[2 * e + 1]);
            const double lo = uni ? 0.0 : pa[d], hi = uni ? 1.0 : pb[d];
            double u = lo + (hi - lo) * xi;
            u = u < hi ? u : hi;                                 // min(b, .)
            U2[n * bx.A + d] = u;
            const int c = bx.act[d];
            row[c] = column_value(bx, c, u);
        }
    }
    put_overrides(bx, row);
}

__global__ void __launch_bounds__(kThreads) unit_kernel(const double *X, int64_t S, int64_t ldx, const Box bx, double *U)
{
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    for (int d = 0; d < bx.A; d++) {
        const int c = bx.act[d];
        const double x = X[s * ldx + c];
        U[s * bx.A + d] = bx.do_log[c] ? (log10(x) - bx.l[c]) / (bx.lh[c] - bx.l[c]) : (x - bx.lo[c]) / (bx.hi[c] - bx.lo[c]);
    }
}

template <int A>
__global__ void __launch_bounds__(kThreads) density_kernel(const double *U, int64_t S, int64_t ldu, const double *a, const double *b,
                                                           const double *inv_vol, int64_t K, double *B)
{
    __shared__ double2 s_ab[kTile * A];
    __shared__ double s_iv[kTile];
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double u[A];
#pragma unroll
    for (int d = 0; d < A; d++) u[d] = s < S ? U[s * ldu + d] : NAN;         // a NaN lies in no box
    double acc = 0.0;
    for (int64_t k0 = 0; k0 < K; k0 += kTile) {
        const int n = (int)(K - k0 < kTile ? K - k0 : kTile);
        __syncthreads();                                         // everyone has left the tile before
        for (int e = threadIdx.x; e < n * A; e += kThreads) s_ab[e] = make_double2(a[k0 * A + e], b[k0 * A + e]);
        for (int e = threadIdx.x; e < n; e += kThreads) s_iv[e] = inv_vol[k0 + e];
        __syncthreads();
        for (int k = 0; k < n; k++) {
            bool in = true;
#pragma unroll
            for (int d = 0; d < A; d++)
                if (in) {
                    const double2 ab = s_ab[k * A + d];
                    in = u[d] >= ab.x && u[d] <= ab.y;
                }
            if (in) acc = acc + s_iv[k];
        }
    }
    if (s < S) B[s] = acc;
}

}  // namespace refine
}  // namespace trpl

using namespace trpl;

static int check_resample(const void *W, int64_t S, int64_t K, double offset, const void *idx)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 0", (long long)S);
    if (K < 1 || K > TRPL_REFINE_MAX_PARENTS)
        return api_fail(TRPL_ERR_ARG, "K=%lld must be in [1, TRPL_REFINE_MAX_PARENTS = %d]", (long long)K, TRPL_REFINE_MAX_PARENTS);
    if (!(offset >= 0.0 && offset < 1.0)) return api_fail(TRPL_ERR_ARG, "offset=%g must lie in [0, 1)", offset);
    if (S > 0 && !W) return api_fail(TRPL_ERR_ARG, "W is NULL");
    if (!idx) return api_fail(TRPL_ERR_ARG, "idx is NULL");
    return TRPL_OK;
}

static int check_draw(const void *a, const void *b, int64_t K, int32_t A, int64_t m, int64_t n_uniform, const void *U2, const void *X2)
{
    if (int rc = refine_check_counts(K, A)) return rc;
    if (int rc = refine_check_children(K, m, n_uniform)) return rc;
    if (!a) return api_fail(TRPL_ERR_ARG, "a is NULL");
    if (!b) return api_fail(TRPL_ERR_ARG, "b is NULL");
    if (!U2) return api_fail(TRPL_ERR_ARG, "U2 is NULL");
    if (!X2) return api_fail(TRPL_ERR_ARG, "X2 is NULL");
    return TRPL_OK;
}

static int check_density(const void *U, int64_t S, int64_t ldu, int32_t A, const void *a, const void *b, const void *inv_vol, int64_t K,
                         const void *B)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 0", (long long)S);
    if (int rc = refine_check_counts(K, A)) return rc;
    if (ldu < A) return api_fail(TRPL_ERR_ARG, "ldu=%lld must be >= A=%d", (long long)ldu, A);
    if (int rc = refine_check_blocks("S", S, "samples")) return rc;
    if (!a) return api_fail(TRPL_ERR_ARG, "a is NULL");
    if (!b) return api_fail(TRPL_ERR_ARG, "b is NULL");
    if (!inv_vol) return api_fail(TRPL_ERR_ARG, "inv_vol is NULL");
    if (S > 0 && !U) return api_fail(TRPL_ERR_ARG, "U is NULL");
    if (S > 0 && !B) return api_fail(TRPL_ERR_ARG, "B is NULL");
    return TRPL_OK;
}

static int check_unit(const void *X, int64_t S, int64_t ldx, int32_t ncol, int32_t A, const void *U)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 0", (long long)S);
    if (A < 1 || A > TRPL_REFINE_MAX_DIMS) return api_fail(TRPL_ERR_ARG, "A=%d must be in [1, %d]", A, TRPL_REFINE_MAX_DIMS);
    if (ldx < ncol) return api_fail(TRPL_ERR_ARG, "ldx=%lld must be >= ncol=%d", (long long)ldx, ncol);
    if (int rc = refine_check_blocks("S", S, "samples")) return rc;
    if (S > 0 && !X) return api_fail(TRPL_ERR_ARG, "X is NULL");
    if (S > 0 && !U) return api_fail(TRPL_ERR_ARG, "U is NULL");
    return TRPL_OK;
}

static int64_t chunks_of(int64_t S) { return (S + refine::kChunk - 1) / refine::kChunk; }

extern "C" {

int64_t trpl_refine_chunk_rows(void) { return refine::kChunk; }
int64_t trpl_refine_tile_parents(void) { return refine::kTile; }

int64_t trpl_refine_workspace_bytes(int64_t S)
{
    if (S < 0) return 0;
    return (4 * chunks_of(S) + 1) * 8 + 256;                     // chunk totals, scaled sums of squares and their exponents, the prefix
}

int trpl_refine_resample_dev(const double *W, int64_t S, int64_t K, double offset, int64_t *idx, double *stats, void *workspace,
                             int64_t workspace_bytes, void *stream)
{
    if (int rc = check_resample(W, S, K, offset, idx)) return rc;
    if (!workspace) return api_fail(TRPL_ERR_ARG, "workspace is NULL");
    if (workspace_bytes < trpl_refine_workspace_bytes(S))
        return api_fail(TRPL_ERR_ARG, "workspace_bytes=%lld is less than trpl_refine_workspace_bytes(S) = %lld", (long long)workspace_bytes,
                        (long long)trpl_refine_workspace_bytes(S));
    const int64_t nch = chunks_of(S);
    if (nch > kRefineMaxBlocks) return api_fail(TRPL_ERR_ARG, "S=%lld is more than 2^31 - 1 chunks", (long long)S);
    hipStream_t st = (hipStream_t)stream;
    double *tot = (double *)workspace, *sq = tot + nch, *ex = sq + nch, *prefix = ex + nch;
    if (nch) hipLaunchKernelGGL(refine::chunk_sums_kernel, dim3((unsigned)nch), dim3(refine::kThreads), 0, st, W, S, tot, sq, ex);
    hipLaunchKernelGGL(refine::chunk_prefix_kernel, dim3(1), dim3(refine::kThreads), 0, st, tot, sq, ex, nch, prefix, stats);
    hipLaunchKernelGGL(refine::resample_kernel, dim3((unsigned)(nch ? nch : 1)), dim3(refine::kThreads), 0, st, W, S, K, offset, prefix, nch, idx);
    return refine_launched("refine resample");
}

int trpl_refine_resample(const double *W, int64_t S, int64_t K, double offset, int64_t *idx, double *stats, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_resample(W, S, K, offset, idx)) return rc;
    for (int64_t i = 0; i < S; i++)
        if (W[i] == INFINITY) return api_fail(TRPL_ERR_ARG, "W[%lld] is +inf: a weight must be finite", (long long)i);
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const int64_t wsb = trpl_refine_workspace_bytes(S);
    const double *dW = sg.in(W, (size_t)S);
    int64_t *dIdx = sg.out(idx, (size_t)K);
    double *dStats = sg.out(stats, 3);
    void *dWs = sg.scratch((size_t)wsb);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_refine_resample_dev(dW, S, K, offset, dIdx, dStats, dWs, wsb, sg.stream())) return rc;
    return sg.finish(seconds);
}

int trpl_refine_draw_dev(const double *a, const double *b, int64_t K, int32_t A, int64_t m, int64_t n_uniform, uint64_t seed,
                         uint32_t generation, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log, uint32_t flags,
                         double *U2, double *X2, void *stream)
{
    if (int rc = check_draw(a, b, K, A, m, n_uniform, U2, X2)) return rc;
    refine::Box bx;
    if (int rc = refine_make_box(ncol, lo, hi, do_log, flags, A, bx)) return rc;
    const int64_t total = n_uniform + K * m;
    if (total == 0) return TRPL_OK;
    hipLaunchKernelGGL(refine::draw_kernel, dim3(refine_blocks(total)), dim3(refine::kThreads), 0, (hipStream_t)stream, a, b, K, n_uniform,
                       total, (uint32_t)seed, (uint32_t)(seed >> 32), generation, bx, U2, X2);
    return refine_launched("refine draw");
}

int trpl_refine_draw(const double *a, const double *b, int64_t K, int32_t A, int64_t m, int64_t n_uniform, uint64_t seed, uint32_t generation,
                     int32_t ncol, const double *lo, const double *hi, const int32_t *do_log, uint32_t flags, double *U2, double *X2,
                     int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_draw(a, b, K, A, m, n_uniform, U2, X2)) return rc;
    refine::Box bx;
    if (int rc = refine_make_box(ncol, lo, hi, do_log, flags, A, bx)) return rc;
    const int64_t total = n_uniform + K * m;
    if (total == 0) return TRPL_OK;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const double *dA = sg.in(a, (size_t)K * A), *dB = sg.in(b, (size_t)K * A);
    double *dU = sg.out(U2, (size_t)total * A), *dX = sg.out(X2, (size_t)total * ncol);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_refine_draw_dev(dA, dB, K, A, m, n_uniform, seed, generation, ncol, lo, hi, do_log, flags, dU, dX, sg.stream())) return rc;
    return sg.finish(seconds);
}

int trpl_refine_density_dev(const double *U, int64_t S, int64_t ldu, int32_t A, const double *a, const double *b, const double *inv_vol,
                            int64_t K, double *B, void *stream)
{
    if (int rc = check_density(U, S, ldu, A, a, b, inv_vol, K, B)) return rc;
    if (S == 0) return TRPL_OK;
    const dim3 grid(refine_blocks(S)), block(refine::kThreads);
    switch (A) {
#define TRPL_CASE(n) case n: hipLaunchKernelGGL(refine::density_kernel<n>, grid, block, 0, (hipStream_t)stream, U, S, ldu, a, b, inv_vol, K, B); break;
        TRPL_REFINE_DIMS(TRPL_CASE)
#undef TRPL_CASE
    }
    return refine_launched("refine density");
}

int trpl_refine_density(const double *U, int64_t S, int64_t ldu, int32_t A, const double *a, const double *b, const double *inv_vol, int64_t K,
                        double *B, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_density(U, S, ldu, A, a, b, inv_vol, K, B)) return rc;
    if (S == 0) return TRPL_OK;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const double *dU = sg.in(U, (size_t)(S - 1) * (size_t)ldu + A);                      // the last row ends after its A entries
    const double *dA = sg.in(a, (size_t)K * A), *dB = sg.in(b, (size_t)K * A), *dV = sg.in(inv_vol, (size_t)K);
    double *dOut = sg.out(B, (size_t)S);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_refine_density_dev(dU, S, ldu, A, dA, dB, dV, K, dOut, sg.stream())) return rc;
    return sg.finish(seconds);
}

int trpl_refine_unit_dev(const double *X, int64_t S, int64_t ldx, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log,
                         uint32_t flags, int32_t A, double *U, void *stream)
{
    refine::Box bx;
    if (int rc = refine_make_box(ncol, lo, hi, do_log, flags, A, bx)) return rc;
    if (int rc = check_unit(X, S, ldx, ncol, A, U)) return rc;
    if (S == 0) return TRPL_OK;
    hipLaunchKernelGGL(refine::unit_kernel, dim3(refine_blocks(S)), dim3(refine::kThreads), 0, (hipStream_t)stream, X, S, ldx, bx, U);
    return refine_launched("refine unit");
}

int trpl_refine_unit(const double *X, int64_t S, int64_t ldx, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log,
                     uint32_t flags, int32_t A, double *U, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    refine::Box bx;
    if (int rc = refine_make_box(ncol, lo, hi, do_log, flags, A, bx)) return rc;
    if (int rc = check_unit(X, S, ldx, ncol, A, U)) return rc;
    if (S == 0) return TRPL_OK;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const double *dX = sg.in(X, (size_t)(S - 1) * (size_t)ldx + ncol);                   // the last row ends after its ncol entries
    double *dU = sg.out(U, (size_t)S * A);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_refine_unit_dev(dX, S, ldx, ncol, lo, hi, do_log, flags, A, dU, sg.stream())) return rc;
    return sg.finish(seconds);
}

}  // extern "C"
