// Ensemble Metropolis sampling (trpl_mcmc_propose*, trpl_mcmc_accept*, trpl_mcmc_chain_stats*, include/trpl.h): the cheap half of a
// Markov-chain sampler whose expensive half, the likelihood of every chain's proposal, is one launch of the fused likelihood.
//
//   propose_kernel<A>     one thread per chain.  The uniforms are the refinement draws' (Philox4x32-10, genrand_res53:
//       refine_common.hpp) with the counter's third word moved to 0x100 + j: call j < 8 gives xi[2j], xi[2j + 1], call 8 the two
//       partner uniforms.  With partners (differential evolution, ter Braak 2006): u'_d = (u_d + gamma (pa_d - pb_d)) + scale_d (2
//       xi_d - 1); without (random walk): u'_d = u_d + scale_d (2 xi_d - 1).  inside = every u'_d in [0, 1]; X by the sampler's
//       expressions from u', inside or not, as draw_oriented_kernel forms it.  The body is propose_body<A, FOLD, RUNGS>; propose_kernel
//       is FOLD = false.
//   propose_fold_kernel<A>  the same body with FOLD = true (TRPL_MCMC_FOLD, include/trpl.h): each u'_d that fails the range test
//       is reflected back into [0, 1] before it is stored and turned into X; inside = 0 (a NaN is left), 2 (folded) or 1 (untouched).
//   accept_kernel<A>      one thread per chain.  xi of counter word 0x109; the chain takes its proposal's U, X and LL when the
//       proposal is inside, its LLp is neither NaN nor -inf, and the chain stands on a likelihood that is not above -inf, or
//       d = (LLp - LL) / tf >= 0, or log(xi) < d.
//   levels_kernel         one thread per chain.  The accept step's xi (the same counter word, res53 and log), turned into the level of
//       trpl_loglik_cut_levels above which a proposal's running sse makes its rejection by accept_kernel certain: -(LL + tf log(xi)),
//       or that plus a few ulps, whichever the accept step's own expression confirms; +inf (never cut) when neither does.
//   chain_stats_kernel    one thread per column q of a history H [n][ldh]: the mean and the centred sum of squares over the steps
//       [t0, t1), both sums in ascending t from +0.0.  Adjacent threads read adjacent addresses.
// Autocovariance sums (trpl_mcmc_autocov*, include/trpl.h): what the effective sample size is formed from.
//   autocov_mean_kernel   chain_stats_kernel's first pass alone: mean[q], the bits of chain_stats.
//   autocov_kernel<TL>    one thread per column q and tile of TL consecutive lags [l0, l0 + TL): s[l][q] = sum over t of e[t] e[t + l],
//       e = H - mean, t ascending from +0.0.  The thread walks u = t + l upward and pairs e[u] with the TL centred values before it,
//       kept in a register window that rotates with static indices (the time loop is unrolled by TL): per step two loads, two
//       subtracts, TL multiplies and TL adds.  u upward is t upward for every lag, and the product commutes: the definition's bits.
//   autocov_pool_kernel   one thread per (l, a): pooled[l][a] = sum over c < M of s[l][c A + a], c ascending from +0.0; 16 loads ahead.
// Parallel tempering (trpl_mcmc_*_rungs*, trpl_mcmc_swap*, include/trpl.h): K rungs of `group` chains each in one
// contiguous block, row k group + c chain c of rung k, advanced by one launch each.
//   propose_rungs_kernel<A>, propose_rungs_fold_kernel<A>   propose_body with the partners of chain i narrowed to the rows
//       [(i / group) group, + group) of `partners` and P = group in the index expressions: a rung's slice is propose_kernel's bits.
//   accept_rungs_kernel<A>, levels_rungs_kernel   accept_body and levels_body with tf = ladder[i / group]; the ladder travels by value.
//   hastings_accept_kernel<A>, hastings_levels_kernel   (trpl_mcmc_accept_h*, trpl_mcmc_levels_h*) the same
//       two bodies with H = true, an untempered log term h[i] per chain: d = (LLp - LL) / tf[i / group] + h[i], and the level that goes
//       with that d.  At h = +-0.0 they give the rung kernels' bits: the quotient is the same source line, and the sum changes no value
//       but -0.0, which no comparison sees.  What produces h, the stretch move and the prior term, is mcmc_hastings.hip.
//   swap_kernel<A>        one thread per row of the block; the thread of the lower row a of a pair (k, k + 1), k = parity, parity + 2, ..,
//       decides it: xi of counter word 0x10a keyed by row a, d = (LL[b] - LL[a]) * (1 / tf[k] - 1 / tf[k + 1]), the rows of U, X and LL
//       exchanged when neither LL is NaN and d >= 0 or log(xi) < d.  The thread of an upper row writes nothing; an unpaired row's
//       writes swapped = 0 only.
// The host half, after the kernels.  Propose, accept, levels and swap have one argument record each (ProposeCall, AcceptCall,
// LevelsCall, SwapCall: the entry point's arguments in its order; `rungs` marks a *_rungs call, whose group, K and ladder are read
// only then, `with_h` a *_h call, a rung call whose h is read only then) and three functions on it: check (every refusal of the
// operation, for each of its forms in the order the entry points have always had; it makes the kernel arguments Scale, Box, Ladder),
// launch (the kernel of the record, on a stream) and stage (the record's buffers through a Staged).  on_stream is every _dev form:
// check, launch.  staged is every host-buffer form: check before a device is opened, stage, launch -- the record is checked once.  An
// extern "C" entry point fills a record and returns one of the two.  A new argument goes into the record, its refusal into check, its
// buffer into stage; a new operation is a record with these three.  on_stream and staged, the shared checks and the Philox call
// indices are mcmc_common.hpp's, shared with mcmc_hastings.hip, which has the stretch move and the prior term in the same structure.
// chain_stats and the autocovariance calls are a kernel or two each and stay written out; their refusals share check_history.
// Compiled with -ffp-contract=off like refine.hip: every result is its expression with one rounding per operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "api_util.hpp"
#include "mcmc_common.hpp"
#include "refine_common.hpp"

namespace trpl {
namespace mcmc {                                                 // the kernels of this unit; the box, Philox and X are trpl::refine's

using namespace refine;

struct Scale {
    double s[16];
};

// fold_outside, the reflection of TRPL_MCMC_FOLD, is mcmc_common.hpp's, shared with mcmc_subspace.hip.
// RUNGS: the partners of chain i are the `group` rows of its rung, [(i / group) group, + group) of `partners`
template <int A, bool FOLD, bool RUNGS>
__device__ __forceinline__ void propose_body(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, double gamma,
                                             const Scale &sc, int64_t chain0, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, const Box &bx,
                                             double *Up, double *Xp, int32_t *inside)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    if (RUNGS) {
        partners += (i / group) * group * A;
        P = group;
    }
    const uint64_t n = (uint64_t)(chain0 + i);
    double xi[A];
#pragma unroll
    for (int j = 0; 2 * j < A; j++) {
        uint32_t r[4];
        philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + (uint32_t)j, step, seed_lo, seed_hi, r);
        xi[2 * j] = res53(r[0], r[1]);
        if (2 * j + 1 < A) xi[2 * j + 1] = res53(r[2], r[3]);
    }
    double u[A];
#pragma unroll
    for (int d = 0; d < A; d++) u[d] = U[i * A + d];
    if (P >= 2) {
        uint32_t r[4];
        philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kPartnerCall, step, seed_lo, seed_hi, r);
        const double xa = res53(r[0], r[1]), xb = res53(r[2], r[3]);
        int64_t a = (int64_t)(xa * (double)P), b = (int64_t)(xb * (double)(P - 1));
        a = a < P - 1 ? a : P - 1;
        b = b < P - 2 ? b : P - 2;
        b += b >= a;
        const double *pa = partners + a * A, *pb = partners + b * A;
#pragma unroll
        for (int d = 0; d < A; d++) u[d] = u[d] + gamma * (pa[d] - pb[d]);
    }
    bool in = true, folded = false;
    double *row = Xp + i * bx.ncol;
    put_fixed(bx, row);
#pragma unroll
    for (int d = 0; d < A; d++) {
        u[d] = u[d] + sc.s[d] * (2.0 * xi[d] - 1.0);
        if (FOLD) {
            if (!(u[d] >= 0.0 && u[d] <= 1.0)) {
                u[d] = fold_outside(u[d]);
                folded = true;
            }
            in = in && u[d] == u[d];                             // after the fold only a NaN is left outside
        } else {
            in = in && u[d] >= 0.0 && u[d] <= 1.0;               // a NaN is outside
        }
        Up[i * A + d] = u[d];
        const int c = bx.act[d];
        row[c] = column_value(bx, c, u[d]);
    }
    put_overrides(bx, row);
    inside[i] = !in ? 0 : folded ? 2 : 1;
}

#define TRPL_PROPOSE_PARAMS                                                                                                            \
    const double *U, const double *partners, int64_t count, int64_t P, double gamma, const Scale sc, int64_t chain0, uint32_t seed_lo,  \
        uint32_t seed_hi, uint32_t step, const Box bx, double *Up, double *Xp, int32_t *inside
#define TRPL_PROPOSE_ARGS(group) U, partners, count, P, group, gamma, sc, chain0, seed_lo, seed_hi, step, bx, Up, Xp, inside

template <int A>
__global__ void __launch_bounds__(kThreads) propose_kernel(TRPL_PROPOSE_PARAMS)
{
    propose_body<A, false, false>(TRPL_PROPOSE_ARGS(0));
}

template <int A>
__global__ void __launch_bounds__(kThreads) propose_fold_kernel(TRPL_PROPOSE_PARAMS)
{
    propose_body<A, true, false>(TRPL_PROPOSE_ARGS(0));
}

template <int A>
__global__ void __launch_bounds__(kThreads) propose_rungs_kernel(TRPL_PROPOSE_PARAMS, int64_t group)
{
    propose_body<A, false, true>(TRPL_PROPOSE_ARGS(group));
}

template <int A>
__global__ void __launch_bounds__(kThreads) propose_rungs_fold_kernel(TRPL_PROPOSE_PARAMS, int64_t group)
{
    propose_body<A, true, true>(TRPL_PROPOSE_ARGS(group));
}

#undef TRPL_PROPOSE_PARAMS
#undef TRPL_PROPOSE_ARGS

// The accept step of all three forms.  H: the call has a Hastings term (include/trpl.h, trpl_mcmc_accept_h), an untempered h[i] added
// to d; a proposal whose term is NaN or -inf is not taken.  Without it h is not read and d is the quotient alone.  tf() gives the
// chain's temperature where d is formed.
template <int A, bool H, class TF>
__device__ __forceinline__ void accept_body(int64_t i, double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp,
                                            const int32_t *inside, const double *h, int32_t ncol, TF tf, int64_t chain0, uint32_t seed_lo,
                                            uint32_t seed_hi, uint32_t step, int32_t *accepted)
{
    const uint64_t n = (uint64_t)(chain0 + i);
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kAcceptCall, step, seed_lo, seed_hi, r);
    const double xi = res53(r[0], r[1]);
    const double ll = LL[i], llp = LLp[i];
    double hv = 0.0;
    if constexpr (H) hv = h[i];
    const double d0 = (llp - ll) / tf();
    const double d = H ? d0 + hv : d0;
    const bool take = inside[i] != 0 && !(llp != llp) && llp > -INFINITY && (!H || (!(hv != hv) && hv > -INFINITY)) &&
                      (!(ll > -INFINITY) || d >= 0.0 || log(xi) < d);
    accepted[i] = take ? 1 : 0;
    if (!take) return;
#pragma unroll
    for (int k = 0; k < A; k++) U[i * A + k] = Up[i * A + k];
    for (int c = 0; c < ncol; c++) X[i * ncol + c] = Xp[i * ncol + c];
    LL[i] = llp;
}

#define TRPL_ACCEPT_PARAMS(tf_type)                                                                                                    \
    double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside, int64_t count,        \
        int32_t ncol, tf_type tf, int64_t chain0, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, int32_t *accepted
#define TRPL_ACCEPT_ARGS(h, tf) i, U, X, LL, Up, Xp, LLp, inside, h, ncol, tf, chain0, seed_lo, seed_hi, step, accepted

template <int A>
__global__ void __launch_bounds__(kThreads) accept_kernel(TRPL_ACCEPT_PARAMS(double))
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    accept_body<A, false>(TRPL_ACCEPT_ARGS(nullptr, [tf] { return tf; }));
}

template <int A>
__global__ void __launch_bounds__(kThreads) accept_rungs_kernel(TRPL_ACCEPT_PARAMS(const Ladder), int64_t group)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const double t = tf.tf[i / group];
    accept_body<A, false>(TRPL_ACCEPT_ARGS(nullptr, [t] { return t; }));
}

template <int A>
__global__ void __launch_bounds__(kThreads) hastings_accept_kernel(double *U, double *X, double *LL, const double *Up, const double *Xp,
                                                                   const double *LLp, const int32_t *inside, const double *h, int64_t count,
                                                                   int32_t ncol, const Ladder tf, int64_t group, int64_t chain0,
                                                                   uint32_t seed_lo, uint32_t seed_hi, uint32_t step, int32_t *accepted)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    accept_body<A, true>(TRPL_ACCEPT_ARGS(h, [&] { return tf.tf[i / group]; }));
}

#undef TRPL_ACCEPT_PARAMS
#undef TRPL_ACCEPT_ARGS

// Early rejection (include/trpl.h, trpl_mcmc_levels): a candidate level l is taken only if the accept step's own d, formed for a proposal
// with LLp = -l, is negative and not above log(xi) -- then every LLp <= -l has a d no larger (subtraction and division by tf > 0 are
// monotone) and the accept kernel rejects it with the same (seed, chain, step).  The argument is per chain -- it never compares two
// chains -- so it holds with a temperature per rung.  With a Hastings term (H; trpl_mcmc_levels_h) it survives the added constant:
// every LLp <= -l has (LLp - LL) / tf <= (-l - LL) / tf as before, and adding the same h to both sides is monotone under
// round-to-nearest, so d <= dq < 0 and log(xi) < d is false: hastings_accept_kernel rejects with the same (seed, chain, step, h).  The
// level is +inf (never cut) where neither candidate is confirmed, and where h is NaN or infinite.
template <bool H, class TF>
__device__ __forceinline__ void levels_body(int64_t i, const double *LL, const double *h, TF tf, int64_t chain0, uint32_t seed_lo,
                                            uint32_t seed_hi, uint32_t step, double *level)
{
    const uint64_t n = (uint64_t)(chain0 + i);
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kAcceptCall, step, seed_lo, seed_hi, r);
    const double xi = res53(r[0], r[1]);
    const double ll = LL[i];
    double hv = 0.0;
    if constexpr (H) hv = h[i];
    const double t = tf();
    double lv = INFINITY;
    if (!(ll != ll) && ll > -INFINITY && xi != 0.0 && (!H || (!(hv != hv) && fabs(hv) < INFINITY))) {
        const double lx = log(xi);
        const double l0 = H ? -(ll + t * (lx - hv)) : -(ll + t * lx);
        double cand = l0;
        for (int k = 0; k < 2; k++) {
            const double q = -cand;
            const double dq0 = (q - ll) / t;
            const double dq = H ? dq0 + hv : dq0;
            if (dq < 0.0 && !(lx < dq)) { lv = cand; break; }
            cand = l0 + (fabs(ll) + l0) * 0x1p-40;
        }
    }
    level[i] = lv;
}

__global__ void __launch_bounds__(kThreads) levels_kernel(const double *LL, int64_t count, double tf, int64_t chain0, uint32_t seed_lo,
                                                          uint32_t seed_hi, uint32_t step, double *level)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    levels_body<false>(i, LL, nullptr, [tf] { return tf; }, chain0, seed_lo, seed_hi, step, level);
}

__global__ void __launch_bounds__(kThreads) levels_rungs_kernel(const double *LL, int64_t count, const Ladder tf, int64_t group,
                                                                int64_t chain0, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                                double *level)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const double t = tf.tf[i / group];
    levels_body<false>(i, LL, nullptr, [t] { return t; }, chain0, seed_lo, seed_hi, step, level);
}

__global__ void __launch_bounds__(kThreads) hastings_levels_kernel(const double *LL, const double *h, int64_t count, const Ladder tf,
                                                                   int64_t group, int64_t chain0, uint32_t seed_lo, uint32_t seed_hi,
                                                                   uint32_t step, double *level)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    levels_body<true>(i, LL, h, [&] { return tf.tf[i / group]; }, chain0, seed_lo, seed_hi, step, level);
}

// Replica exchange (include/trpl.h, trpl_mcmc_swap): count = K group rows.  Row i belongs to rung k = i / group; it is the lower row of a
// pair when k - parity is even and not negative and k + 1 < K, the upper row when k - parity is odd and positive, else unpaired.
template <int A>
__global__ void __launch_bounds__(kThreads) swap_kernel(double *U, double *X, double *LL, int64_t count, int32_t K, int64_t group,
                                                        int32_t ncol, const Ladder tf, int32_t parity, int64_t chain0, uint32_t seed_lo,
                                                        uint32_t seed_hi, uint32_t step, int32_t *swapped)
{
    const int64_t a = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (a >= count) return;
    const int32_t k = (int32_t)(a / group);
    const int32_t rel = k - parity;
    if (rel > 0 && (rel & 1)) return;                            // the upper row of a pair: its lower row's thread writes it
    if (rel < 0 || k + 1 >= K) {                                 // unpaired
        swapped[a] = 0;
        return;
    }
    const int64_t b = a + group;
    const uint64_t n = (uint64_t)(chain0 + a);
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kSwapCall, step, seed_lo, seed_hi, r);
    const double xi = res53(r[0], r[1]);
    const double la = LL[a], lb = LL[b];
    const double d = (lb - la) * (1.0 / tf.tf[k] - 1.0 / tf.tf[k + 1]);
    const bool take = !(la != la) && !(lb != lb) && (d >= 0.0 || log(xi) < d);
    swapped[a] = swapped[b] = take ? 1 : 0;
    if (!take) return;
#pragma unroll
    for (int j = 0; j < A; j++) {
        const double ua = U[a * A + j], ub = U[b * A + j];
        U[a * A + j] = ub;
        U[b * A + j] = ua;
    }
    for (int c = 0; c < ncol; c++) {
        const double xa = X[a * ncol + c], xb = X[b * ncol + c];
        X[a * ncol + c] = xb;
        X[b * ncol + c] = xa;
    }
    LL[a] = lb;
    LL[b] = la;
}

__global__ void __launch_bounds__(kThreads) chain_stats_kernel(const double *H, int64_t ldh, int64_t Q, int64_t t0, int64_t t1,
                                                               double *mean, double *m2)
{
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= Q) return;
    double s = 0.0;
    for (int64_t t = t0; t < t1; t++) s = s + H[t * ldh + q];
    const double mu = s / (double)(t1 - t0);
    double v = 0.0;
    for (int64_t t = t0; t < t1; t++) {
        const double e = H[t * ldh + q] - mu;
        v = v + e * e;
    }
    mean[q] = mu;
    m2[q] = v;
}

// ---- autocovariance sums.  kAutocovTile is trpl_mcmc_autocov_tile(): with 8 lags per thread the kernel takes 72 VGPRs, 7 waves per
// SIMD and no scratch; 16 lags take 166 and leave 3 waves.
constexpr int kAutocovTile = 8;

__global__ void __launch_bounds__(kThreads) autocov_mean_kernel(const double *H, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, double *mean)
{
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= Q) return;
    double s = 0.0;
    for (int64_t t = t0; t < t1; t++) s = s + H[t * ldh + q];
    mean[q] = s / (double)(t1 - t0);
}

// TL steps r = base .. base + TL - 1 of a thread's walk: e[r] (row hw) enters slot r % TL = j of the window, e[l0 + r] (row hu) multiplies
// the window's e[r - k] into the sum of lag l0 + k.  FIRST (base = 0): e[r - k] exists from r = k on.  PARTIAL: only `left` < TL steps
// remain.  Every index of w and acc is a constant after unrolling.
template <int TL, bool FIRST, bool PARTIAL>
__device__ __forceinline__ void autocov_chunk(const double *hw, const double *hu, int64_t ldh, double mu, int64_t left, double (&w)[TL],
                                              double (&acc)[TL])
{
    double hv[TL], uv[TL];                                       // the chunk's 2 TL loads are issued before its arithmetic
#pragma unroll
    for (int j = 0; j < TL; j++) {
        if (PARTIAL && j >= left) break;
        hv[j] = hw[j * ldh];
        uv[j] = hu[j * ldh];
    }
#pragma unroll
    for (int j = 0; j < TL; j++) {
        if (PARTIAL && j >= left) break;
        w[j] = hv[j] - mu;
        const double eu = uv[j] - mu;
#pragma unroll
        for (int k = 0; k < TL; k++) {
            if (FIRST && k > j) continue;
            acc[k] = acc[k] + eu * w[(j - k + TL) % TL];
        }
    }
}

// Block b serves the lag tile b / qblocks and the columns (b % qblocks) kThreads + thread: the tiles go out in ascending l0, the
// longest walks first.  (Measured, DESIGN.md section 28: the other order, the tiles of one block of columns adjacent so that they share
// their rows of H in a cache, is 1.6 x faster where H is far larger than the caches and 1.4 x slower where it fits, the usual case.)  A
// block's R = m - l0 steps are the same for all its threads, so no branch diverges.  Reads stay inside the rows [t0, t1): hw reads
// t0 + r and hu reads t0 + l0 + r for r < R = (t1 - t0) - l0, whatever k; a lag l0 + k >= L of the edge tile is summed and not stored.
template <int TL>
__global__ void __launch_bounds__(kThreads) autocov_kernel(const double *H, int64_t ldh, int64_t Q, int64_t qblocks, int64_t t0, int64_t t1,
                                                           int64_t L, const double *mean, double *s, int64_t lds)
{
    const int64_t tile = (int64_t)blockIdx.x / qblocks;
    const int64_t q = ((int64_t)blockIdx.x % qblocks) * kThreads + threadIdx.x;
    if (q >= Q) return;
    const int64_t l0 = tile * TL, R = (t1 - t0) - l0;
    const double mu = mean[q];
    const double *hw = H + t0 * ldh + q, *hu = hw + l0 * ldh;
    double w[TL], acc[TL];
#pragma unroll
    for (int k = 0; k < TL; k++) w[k] = acc[k] = 0.0;
    if (R >= TL) autocov_chunk<TL, true, false>(hw, hu, ldh, mu, TL, w, acc);
    else autocov_chunk<TL, true, true>(hw, hu, ldh, mu, R, w, acc);
    int64_t base = TL;
    for (; base + TL <= R; base += TL) autocov_chunk<TL, false, false>(hw + base * ldh, hu + base * ldh, ldh, mu, TL, w, acc);
    if (base < R) autocov_chunk<TL, false, true>(hw + base * ldh, hu + base * ldh, ldh, mu, R - base, w, acc);
#pragma unroll
    for (int k = 0; k < TL; k++)
        if (l0 + k < L) s[(l0 + k) * lds + q] = acc[k];
}

// One sum is sequential in c by definition, so a thread is as fast as its loads: kPoolAhead of them are issued before they are added,
// in order, and the L A threads go out in blocks of one wavefront, over as many compute units as there are.
constexpr int kPoolThreads = 64, kPoolAhead = 16;

__global__ void __launch_bounds__(kPoolThreads) autocov_pool_kernel(const double *s, int64_t L, int64_t lds, int64_t M, int32_t A, double *pooled)
{
    const int64_t i = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x;
    if (i >= L * A) return;
    const double *row = s + (i / A) * lds + i % A;
    double p = 0.0;
    int64_t c = 0;
    for (; c + kPoolAhead <= M; c += kPoolAhead) {
        double v[kPoolAhead];
#pragma unroll
        for (int k = 0; k < kPoolAhead; k++) v[k] = row[(c + k) * A];
#pragma unroll
        for (int k = 0; k < kPoolAhead; k++) p = p + v[k];
    }
    for (; c < M; c++) p = p + row[c * A];
    pooled[i] = p;
}

}  // namespace mcmc
}  // namespace trpl

using namespace trpl;

namespace {                                                      // the host half: the file comment has its structure

// ---- the records: an entry point's arguments in its order, then what check() makes of them for the kernel.  rungs marks a *_rungs
// call: group, K and ladder are read only then, and tf only without.  with_h marks a *_h call, which is a rung call (K = 1: one
// temperature): h is read only then.
struct ProposeCall {
    const double *U, *partners; int64_t count, P; bool rungs; int64_t group; int32_t A; double gamma; const double *scale;
    int64_t chain0; uint64_t seed; uint32_t step; int32_t ncol; const double *lo, *hi; const int32_t *do_log; uint32_t flags;
    double *Up, *Xp; int32_t *inside;
    mcmc::Scale sc = {}; refine::Box bx = {};
};
struct AcceptCall {
    double *U, *X, *LL; const double *Up, *Xp, *LLp; const int32_t *inside; const double *h; int64_t count; int32_t A, ncol; double tf;
    bool rungs, with_h; int32_t K; int64_t group; const double *ladder; int64_t chain0; uint64_t seed; uint32_t step; int32_t *accepted;
    mcmc::Ladder lad = {};
};
struct LevelsCall {
    const double *LL, *h; int64_t count; double tf; bool rungs, with_h; int32_t K; int64_t group; const double *ladder; int64_t chain0;
    uint64_t seed; uint32_t step; double *level;
    mcmc::Ladder lad = {};
};
struct SwapCall {                                                // count: K group, the rows of one block; check() sets it
    double *U, *X, *LL; int64_t count; int32_t K; int64_t group; int32_t A, ncol; const double *tf; int32_t parity; int64_t chain0;
    uint64_t seed; uint32_t step; int32_t *swapped;
    mcmc::Ladder lad = {};
};

// ---- check: every refusal of an operation, in the order its entry points have always had
int check(ProposeCall &k)
{
    if (int rc = check_chains(k.count, k.A, k.chain0)) return rc;
    if (k.P < 0 || k.P == 1) return api_fail(TRPL_ERR_ARG, "P=%lld must be 0 (random walk) or >= 2", (long long)k.P);
    if (k.P > 0 && !k.partners) return api_fail(TRPL_ERR_ARG, "partners is NULL with P=%lld", (long long)k.P);
    if (int rc = check_not_null({{"U", k.U}, {"scale", k.scale}, {"Up", k.Up}, {"Xp", k.Xp}, {"inside", k.inside}})) return rc;
    if (!isfinite(k.gamma)) return api_fail(TRPL_ERR_ARG, "gamma=%g must be finite", k.gamma);
    if (k.flags & ~(uint32_t)(TRPL_BOX_EQUAL_MU | TRPL_BOX_EQUAL_S | TRPL_BOX_EQUAL_AUGER | TRPL_MCMC_FOLD))
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: only the TRPL_BOX_EQUAL_* bits and TRPL_MCMC_FOLD apply", k.flags);
    for (int d = 0; d < k.A; d++) {
        if (!(isfinite(k.scale[d]) && k.scale[d] >= 0.0)) return api_fail(TRPL_ERR_ARG, "scale[%d]=%g must be finite and >= 0", d, k.scale[d]);
        k.sc.s[d] = k.scale[d];
    }
    if (k.rungs && k.group < 2) return api_fail(TRPL_ERR_ARG, "group=%lld must be >= 2", (long long)k.group);
    if (k.rungs && (k.P < k.group || k.P % k.group))
        return api_fail(TRPL_ERR_ARG, "P=%lld must be a positive multiple of group=%lld", (long long)k.P, (long long)k.group);
    if (k.rungs && k.count > k.P) return api_fail(TRPL_ERR_ARG, "count=%lld must be <= P=%lld", (long long)k.count, (long long)k.P);
    return refine_make_box(k.ncol, k.lo, k.hi, k.do_log, k.flags & ~(uint32_t)TRPL_MCMC_FOLD, k.A, k.bx);
}

int check(AcceptCall &k)
{
    if (k.rungs) {                                               // a rung call refuses its ladder first and its count last
        if (int rc = check_ladder(k.K, k.group, k.ladder, k.lad)) return rc;
        k.tf = k.lad.tf[0];
    }
    if (int rc = check_chains(k.count, k.A, k.chain0)) return rc;
    if (k.ncol < 1 || k.ncol > 16) return api_fail(TRPL_ERR_ARG, "ncol=%d must be in [1, 16]", k.ncol);
    if (!(isfinite(k.tf) && k.tf > 0.0)) return api_fail(TRPL_ERR_ARG, "tf=%g must be finite and > 0", k.tf);
    if (int rc = check_not_null({{"U", k.U}, {"X", k.X}, {"LL", k.LL}, {"Up", k.Up}, {"Xp", k.Xp}, {"LLp", k.LLp}, {"inside", k.inside}}))
        return rc;
    if (k.with_h && !k.h) return api_fail(TRPL_ERR_ARG, "h is NULL");
    if (int rc = check_not_null({{"accepted", k.accepted}})) return rc;
    if (k.rungs && k.count != (int64_t)k.K * k.group)
        return api_fail(TRPL_ERR_ARG, "count=%lld must be K * group = %d * %lld", (long long)k.count, k.K, (long long)k.group);
    return TRPL_OK;
}

int check(LevelsCall &k)
{
    if (k.rungs) {                                               // a rung call refuses its ladder first and its count last
        if (int rc = check_ladder(k.K, k.group, k.ladder, k.lad)) return rc;
        k.tf = k.lad.tf[0];
    }
    if (int rc = check_count(k.count)) return rc;
    if (!(isfinite(k.tf) && k.tf > 0.0)) return api_fail(TRPL_ERR_ARG, "tf=%g must be finite and > 0", k.tf);
    if (k.chain0 < 0) return api_fail(TRPL_ERR_ARG, "chain0=%lld must be >= 0", (long long)k.chain0);
    if (int rc = check_not_null({{"LL", k.LL}})) return rc;
    if (k.with_h && !k.h) return api_fail(TRPL_ERR_ARG, "h is NULL");
    if (int rc = check_not_null({{"level", k.level}})) return rc;
    if (k.rungs && k.count != (int64_t)k.K * k.group)
        return api_fail(TRPL_ERR_ARG, "count=%lld must be K * group = %d * %lld", (long long)k.count, k.K, (long long)k.group);
    return TRPL_OK;
}

int check(SwapCall &k)
{
    if (int rc = check_ladder(k.K, k.group, k.tf, k.lad)) return rc;
    k.count = (int64_t)k.K * k.group;
    if (int rc = check_chains(k.count, k.A, k.chain0)) return rc;
    if (k.ncol < 1 || k.ncol > 16) return api_fail(TRPL_ERR_ARG, "ncol=%d must be in [1, 16]", k.ncol);
    if (k.parity != 0 && k.parity != 1) return api_fail(TRPL_ERR_ARG, "parity=%d must be 0 or 1", k.parity);
    return check_not_null({{"U", k.U}, {"X", k.X}, {"LL", k.LL}, {"swapped", k.swapped}});
}

// ---- launch: the kernel of a checked record on a stream, through TRPL_MCMC_LAUNCH (mcmc_common.hpp)
int launch(const ProposeCall &k, hipStream_t stream)
{
    const bool fold = (k.flags & TRPL_MCMC_FOLD) != 0;
    if (k.rungs) {
        TRPL_MCMC_LAUNCH(k.A, fold ? mcmc::propose_rungs_fold_kernel<n> : mcmc::propose_rungs_kernel<n>, k.count, stream, k.U, k.partners,
                         k.count, k.P, k.gamma, k.sc, k.chain0, (uint32_t)k.seed, (uint32_t)(k.seed >> 32), k.step, k.bx, k.Up, k.Xp,
                         k.inside, k.group)
        return refine_launched("mcmc propose rungs");
    }
    TRPL_MCMC_LAUNCH(k.A, fold ? mcmc::propose_fold_kernel<n> : mcmc::propose_kernel<n>, k.count, stream, k.U, k.partners, k.count, k.P,
                     k.gamma, k.sc, k.chain0, (uint32_t)k.seed, (uint32_t)(k.seed >> 32), k.step, k.bx, k.Up, k.Xp, k.inside)
    return refine_launched("mcmc propose");
}

int launch(const AcceptCall &k, hipStream_t stream)
{
    const uint32_t lo = (uint32_t)k.seed, hi = (uint32_t)(k.seed >> 32);
    if (k.with_h) {
        TRPL_MCMC_LAUNCH(k.A, mcmc::hastings_accept_kernel<n>, k.count, stream, k.U, k.X, k.LL, k.Up, k.Xp, k.LLp, k.inside, k.h, k.count,
                         k.ncol, k.lad, k.group, k.chain0, lo, hi, k.step, k.accepted)
        return refine_launched("mcmc accept h");
    }
    if (k.rungs) {
        TRPL_MCMC_LAUNCH(k.A, mcmc::accept_rungs_kernel<n>, k.count, stream, k.U, k.X, k.LL, k.Up, k.Xp, k.LLp, k.inside, k.count, k.ncol,
                         k.lad, k.chain0, lo, hi, k.step, k.accepted, k.group)
        return refine_launched("mcmc accept rungs");
    }
    TRPL_MCMC_LAUNCH(k.A, mcmc::accept_kernel<n>, k.count, stream, k.U, k.X, k.LL, k.Up, k.Xp, k.LLp, k.inside, k.count, k.ncol, k.tf,
                     k.chain0, lo, hi, k.step, k.accepted)
    return refine_launched("mcmc accept");
}

int launch(const LevelsCall &k, hipStream_t stream)
{
    const dim3 grid(refine_blocks(k.count)), block(refine::kThreads);
    const uint32_t lo = (uint32_t)k.seed, hi = (uint32_t)(k.seed >> 32);
    if (k.with_h)
        hipLaunchKernelGGL(mcmc::hastings_levels_kernel, grid, block, 0, stream, k.LL, k.h, k.count, k.lad, k.group, k.chain0, lo, hi, k.step,
                           k.level);
    else if (k.rungs)
        hipLaunchKernelGGL(mcmc::levels_rungs_kernel, grid, block, 0, stream, k.LL, k.count, k.lad, k.group, k.chain0, lo, hi, k.step, k.level);
    else
        hipLaunchKernelGGL(mcmc::levels_kernel, grid, block, 0, stream, k.LL, k.count, k.tf, k.chain0, lo, hi, k.step, k.level);
    return refine_launched(k.with_h ? "mcmc levels h" : k.rungs ? "mcmc levels rungs" : "mcmc levels");
}

int launch(const SwapCall &k, hipStream_t stream)
{
    TRPL_MCMC_LAUNCH(k.A, mcmc::swap_kernel<n>, k.count, stream, k.U, k.X, k.LL, k.count, k.K, k.group, k.ncol, k.lad, k.parity, k.chain0,
                     (uint32_t)k.seed, (uint32_t)(k.seed >> 32), k.step, k.swapped)
    return refine_launched("mcmc swap");
}

// ---- stage: the record's buffers through a Staged, host pointers replaced by their device copies
void stage(ProposeCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    const double *partners = sg.in(k.partners, (size_t)k.P * k.A);
    k.U = sg.in(k.U, n * k.A); k.partners = k.P > 0 ? partners : nullptr;
    k.Up = sg.out(k.Up, n * k.A); k.Xp = sg.out(k.Xp, n * k.ncol); k.inside = sg.out(k.inside, n);
}

void stage(AcceptCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    k.U = sg.inout(k.U, n * k.A); k.X = sg.inout(k.X, n * k.ncol); k.LL = sg.inout(k.LL, n);
    k.Up = sg.in(k.Up, n * k.A); k.Xp = sg.in(k.Xp, n * k.ncol); k.LLp = sg.in(k.LLp, n);
    k.inside = sg.in(k.inside, n);
    if (k.with_h) k.h = sg.in(k.h, n);
    k.accepted = sg.out(k.accepted, n);
}

void stage(LevelsCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    k.LL = sg.in(k.LL, n);
    if (k.with_h) k.h = sg.in(k.h, n);
    k.level = sg.out(k.level, n);
}

void stage(SwapCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    k.U = sg.inout(k.U, n * k.A); k.X = sg.inout(k.X, n * k.ncol); k.LL = sg.inout(k.LL, n); k.swapped = sg.out(k.swapped, n);
}

// the two forms of an entry point, on_stream and staged, are mcmc_common.hpp's

// ---- the histories of chain_stats and the autocovariance sums
int check_history(int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1)
{
    if (n < 1) return api_fail(TRPL_ERR_ARG, "n=%lld must be >= 1", (long long)n);
    if (Q < 1) return api_fail(TRPL_ERR_ARG, "Q=%lld must be >= 1", (long long)Q);
    if (int rc = refine_check_blocks("Q", Q, "columns")) return rc;
    if (ldh < Q) return api_fail(TRPL_ERR_ARG, "ldh=%lld must be >= Q=%lld", (long long)ldh, (long long)Q);
    if (!(0 <= t0 && t0 < t1 && t1 <= n))
        return api_fail(TRPL_ERR_ARG, "t0=%lld, t1=%lld: the range must satisfy 0 <= t0 < t1 <= n=%lld", (long long)t0, (long long)t1,
                        (long long)n);
    return TRPL_OK;
}

int check_chain_stats(const void *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, const void *mean, const void *m2)
{
    if (int rc = check_history(n, ldh, Q, t0, t1)) return rc;
    return check_not_null({{"H", H}, {"mean", mean}, {"m2", m2}});
}

// the shape of an autocovariance call: the history, then the lags and the grid
int check_autocov_shape(int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, int64_t L)
{
    if (int rc = check_history(n, ldh, Q, t0, t1)) return rc;
    if (L < 1 || L > t1 - t0) return api_fail(TRPL_ERR_ARG, "L=%lld must be in [1, t1 - t0 = %lld]", (long long)L, (long long)(t1 - t0));
    const int64_t tiles = (L + mcmc::kAutocovTile - 1) / mcmc::kAutocovTile;
    if (tiles > kRefineMaxBlocks / (int64_t)refine_blocks(Q))
        return api_fail(TRPL_ERR_ARG, "L=%lld: %lld tiles of %d lags for Q=%lld are more than 2^31 - 1 blocks of %d columns", (long long)L,
                        (long long)tiles, mcmc::kAutocovTile, (long long)Q, refine::kThreads);
    return TRPL_OK;
}

int check_autocov(const void *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, int64_t L, const void *mean, const void *s,
                  int64_t lds)
{
    if (int rc = check_autocov_shape(n, ldh, Q, t0, t1, L)) return rc;
    if (lds < Q) return api_fail(TRPL_ERR_ARG, "lds=%lld must be >= Q=%lld", (long long)lds, (long long)Q);
    return check_not_null({{"H", H}, {"mean", mean}, {"s", s}});
}

// M sequences of A columns each: M A fits an int64 once M has passed the grid's limit
int check_autocov_groups(int64_t M, int32_t A)
{
    if (M < 1) return api_fail(TRPL_ERR_ARG, "M=%lld must be >= 1", (long long)M);
    if (int rc = refine_check_blocks("M", M, "sequences")) return rc;
    if (A < 1 || A > TRPL_REFINE_MAX_DIMS) return api_fail(TRPL_ERR_ARG, "A=%d must be in [1, %d]", A, TRPL_REFINE_MAX_DIMS);
    return TRPL_OK;
}

int check_autocov_pool(const void *s, int64_t L, int64_t lds, int64_t M, int32_t A, const void *pooled)
{
    if (L < 1) return api_fail(TRPL_ERR_ARG, "L=%lld must be >= 1", (long long)L);
    if (int rc = check_autocov_groups(M, A)) return rc;
    if (L > kRefineMaxBlocks * (int64_t)mcmc::kPoolThreads / A)
        return api_fail(TRPL_ERR_ARG, "L=%lld lags of A=%d columns are more than 2^31 - 1 blocks of %d sums", (long long)L, A, mcmc::kPoolThreads);
    if (lds < M * A) return api_fail(TRPL_ERR_ARG, "lds=%lld must be >= M * A = %lld", (long long)lds, (long long)(M * A));
    return check_not_null({{"s", s}, {"pooled", pooled}});
}

}  // namespace

extern "C" {

int trpl_mcmc_propose_dev(const double *U, const double *partners, int64_t count, int64_t P, int32_t A, double gamma, const double *scale,
                          int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo, const double *hi,
                          const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside, void *stream)
{
    return on_stream(ProposeCall{U, partners, count, P, false, 0, A, gamma, scale, chain0, seed, step, ncol, lo, hi, do_log, flags, Up, Xp,
                                 inside}, stream);
}

int trpl_mcmc_propose(const double *U, const double *partners, int64_t count, int64_t P, int32_t A, double gamma, const double *scale,
                      int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log,
                      uint32_t flags, double *Up, double *Xp, int32_t *inside, int32_t device, double *seconds)
{
    return staged(ProposeCall{U, partners, count, P, false, 0, A, gamma, scale, chain0, seed, step, ncol, lo, hi, do_log, flags, Up, Xp,
                              inside}, device, seconds);
}

int trpl_mcmc_accept_dev(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                         int64_t count, int32_t A, int32_t ncol, double tf, int64_t chain0, uint64_t seed, uint32_t step,
                         int32_t *accepted, void *stream)
{
    return on_stream(AcceptCall{U, X, LL, Up, Xp, LLp, inside, nullptr, count, A, ncol, tf, false, false, 0, 0, nullptr, chain0, seed, step,
                                accepted}, stream);
}

int trpl_mcmc_accept(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                     int64_t count, int32_t A, int32_t ncol, double tf, int64_t chain0, uint64_t seed, uint32_t step, int32_t *accepted,
                     int32_t device, double *seconds)
{
    return staged(AcceptCall{U, X, LL, Up, Xp, LLp, inside, nullptr, count, A, ncol, tf, false, false, 0, 0, nullptr, chain0, seed, step,
                             accepted}, device, seconds);
}

int trpl_mcmc_levels_dev(const double *LL, int64_t count, double tf, int64_t chain0, uint64_t seed, uint32_t step, double *level,
                         void *stream)
{
    return on_stream(LevelsCall{LL, nullptr, count, tf, false, false, 0, 0, nullptr, chain0, seed, step, level}, stream);
}

int trpl_mcmc_levels(const double *LL, int64_t count, double tf, int64_t chain0, uint64_t seed, uint32_t step, double *level,
                     int32_t device, double *seconds)
{
    return staged(LevelsCall{LL, nullptr, count, tf, false, false, 0, 0, nullptr, chain0, seed, step, level}, device, seconds);
}

int trpl_mcmc_propose_rungs_dev(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double gamma,
                                const double *scale, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo,
                                const double *hi, const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside, void *stream)
{
    return on_stream(ProposeCall{U, partners, count, P, true, group, A, gamma, scale, chain0, seed, step, ncol, lo, hi, do_log, flags, Up,
                                 Xp, inside}, stream);
}

int trpl_mcmc_propose_rungs(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double gamma,
                            const double *scale, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo,
                            const double *hi, const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside,
                            int32_t device, double *seconds)
{
    return staged(ProposeCall{U, partners, count, P, true, group, A, gamma, scale, chain0, seed, step, ncol, lo, hi, do_log, flags, Up, Xp,
                              inside}, device, seconds);
}

int trpl_mcmc_accept_rungs_dev(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp,
                               const int32_t *inside, int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group, const double *tf,
                               int64_t chain0, uint64_t seed, uint32_t step, int32_t *accepted, void *stream)
{
    return on_stream(AcceptCall{U, X, LL, Up, Xp, LLp, inside, nullptr, count, A, ncol, 0.0, true, false, K, group, tf, chain0, seed, step,
                                accepted}, stream);
}

int trpl_mcmc_accept_rungs(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                           int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group, const double *tf, int64_t chain0,
                           uint64_t seed, uint32_t step, int32_t *accepted, int32_t device, double *seconds)
{
    return staged(AcceptCall{U, X, LL, Up, Xp, LLp, inside, nullptr, count, A, ncol, 0.0, true, false, K, group, tf, chain0, seed, step,
                             accepted}, device, seconds);
}

int trpl_mcmc_levels_rungs_dev(const double *LL, int64_t count, int32_t K, int64_t group, const double *tf, int64_t chain0, uint64_t seed,
                               uint32_t step, double *level, void *stream)
{
    return on_stream(LevelsCall{LL, nullptr, count, 0.0, true, false, K, group, tf, chain0, seed, step, level}, stream);
}

int trpl_mcmc_levels_rungs(const double *LL, int64_t count, int32_t K, int64_t group, const double *tf, int64_t chain0, uint64_t seed,
                           uint32_t step, double *level, int32_t device, double *seconds)
{
    return staged(LevelsCall{LL, nullptr, count, 0.0, true, false, K, group, tf, chain0, seed, step, level}, device, seconds);
}

int trpl_mcmc_accept_h_dev(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                           const double *h, int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group, const double *tf,
                           int64_t chain0, uint64_t seed, uint32_t step, int32_t *accepted, void *stream)
{
    return on_stream(AcceptCall{U, X, LL, Up, Xp, LLp, inside, h, count, A, ncol, 0.0, true, true, K, group, tf, chain0, seed, step, accepted},
                     stream);
}

int trpl_mcmc_accept_h(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                       const double *h, int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group, const double *tf, int64_t chain0,
                       uint64_t seed, uint32_t step, int32_t *accepted, int32_t device, double *seconds)
{
    return staged(AcceptCall{U, X, LL, Up, Xp, LLp, inside, h, count, A, ncol, 0.0, true, true, K, group, tf, chain0, seed, step, accepted},
                  device, seconds);
}

int trpl_mcmc_levels_h_dev(const double *LL, const double *h, int64_t count, int32_t K, int64_t group, const double *tf, int64_t chain0,
                           uint64_t seed, uint32_t step, double *level, void *stream)
{
    return on_stream(LevelsCall{LL, h, count, 0.0, true, true, K, group, tf, chain0, seed, step, level}, stream);
}

int trpl_mcmc_levels_h(const double *LL, const double *h, int64_t count, int32_t K, int64_t group, const double *tf, int64_t chain0,
                       uint64_t seed, uint32_t step, double *level, int32_t device, double *seconds)
{
    return staged(LevelsCall{LL, h, count, 0.0, true, true, K, group, tf, chain0, seed, step, level}, device, seconds);
}

int trpl_mcmc_swap_dev(double *U, double *X, double *LL, int32_t K, int64_t group, int32_t A, int32_t ncol, const double *tf,
                       int32_t parity, int64_t chain0, uint64_t seed, uint32_t step, int32_t *swapped, void *stream)
{
    return on_stream(SwapCall{U, X, LL, 0, K, group, A, ncol, tf, parity, chain0, seed, step, swapped}, stream);
}

int trpl_mcmc_swap(double *U, double *X, double *LL, int32_t K, int64_t group, int32_t A, int32_t ncol, const double *tf, int32_t parity,
                   int64_t chain0, uint64_t seed, uint32_t step, int32_t *swapped, int32_t device, double *seconds)
{
    return staged(SwapCall{U, X, LL, 0, K, group, A, ncol, tf, parity, chain0, seed, step, swapped}, device, seconds);
}

int trpl_mcmc_chain_stats_dev(const double *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, double *mean, double *m2,
                              void *stream)
{
    if (int rc = check_chain_stats(H, n, ldh, Q, t0, t1, mean, m2)) return rc;
    hipLaunchKernelGGL(mcmc::chain_stats_kernel, dim3(refine_blocks(Q)), dim3(refine::kThreads), 0, (hipStream_t)stream, H, ldh, Q, t0, t1,
                       mean, m2);
    return refine_launched("mcmc chain stats");
}

int trpl_mcmc_chain_stats(const double *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, double *mean, double *m2,
                          int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_chain_stats(H, n, ldh, Q, t0, t1, mean, m2)) return rc;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const int64_t steps = t1 - t0;
    const double *dH = sg.in(H + t0 * ldh, (size_t)ldh, (size_t)Q, (size_t)steps);      // the steps of the range only, compact on the device
    double *dM = sg.out(mean, (size_t)Q), *dV = sg.out(m2, (size_t)Q);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_mcmc_chain_stats_dev(dH, steps, Q, Q, 0, steps, dM, dV, sg.stream())) return rc;
    return sg.finish(seconds);
}

int trpl_mcmc_autocov_tile(void) { return mcmc::kAutocovTile; }

int trpl_mcmc_autocov_dev(const double *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, int64_t L, double *mean, double *s,
                          int64_t lds, void *stream)
{
    if (int rc = check_autocov(H, n, ldh, Q, t0, t1, L, mean, s, lds)) return rc;
    const int64_t qblocks = refine_blocks(Q), tiles = (L + mcmc::kAutocovTile - 1) / mcmc::kAutocovTile;
    hipLaunchKernelGGL(mcmc::autocov_mean_kernel, dim3((unsigned)qblocks), dim3(refine::kThreads), 0, (hipStream_t)stream, H, ldh, Q, t0, t1,
                       mean);
    hipLaunchKernelGGL(mcmc::autocov_kernel<mcmc::kAutocovTile>, dim3((unsigned)(qblocks * tiles)), dim3(refine::kThreads), 0,
                       (hipStream_t)stream, H, ldh, Q, qblocks, t0, t1, L, mean, s, lds);
    return refine_launched("mcmc autocov");
}

int trpl_mcmc_autocov(const double *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, int64_t L, double *mean, double *s,
                      int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_autocov(H, n, ldh, Q, t0, t1, L, mean, s, Q)) return rc;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const int64_t steps = t1 - t0;
    const double *dH = sg.in(H + t0 * ldh, (size_t)ldh, (size_t)Q, (size_t)steps);      // the steps of the range only, compact on the device
    double *dM = sg.out(mean, (size_t)Q), *dS = sg.out(s, (size_t)L * Q);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_mcmc_autocov_dev(dH, steps, Q, Q, 0, steps, L, dM, dS, Q, sg.stream())) return rc;
    return sg.finish(seconds);
}

int trpl_mcmc_autocov_pool_dev(const double *s, int64_t L, int64_t lds, int64_t M, int32_t A, double *pooled, void *stream)
{
    if (int rc = check_autocov_pool(s, L, lds, M, A, pooled)) return rc;
    hipLaunchKernelGGL(mcmc::autocov_pool_kernel, dim3((unsigned)((L * A + mcmc::kPoolThreads - 1) / mcmc::kPoolThreads)),
                       dim3(mcmc::kPoolThreads), 0, (hipStream_t)stream, s, L, lds, M, A, pooled);
    return refine_launched("mcmc autocov pool");
}

int trpl_mcmc_autocov_pool(const double *s, int64_t L, int64_t lds, int64_t M, int32_t A, double *pooled, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_autocov_pool(s, L, lds, M, A, pooled)) return rc;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const int64_t Q = M * A;
    const double *dS = sg.in(s, (size_t)lds, (size_t)Q, (size_t)L);
    double *dP = sg.out(pooled, (size_t)L * A);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_mcmc_autocov_pool_dev(dS, L, Q, M, A, dP, sg.stream())) return rc;
    return sg.finish(seconds);
}

int trpl_mcmc_autocov_chains(const double *H, int64_t n, int64_t ldh, int64_t M, int32_t A, int64_t t0, int64_t t1, int64_t L, double *mean,
                             double *m2, double *pooled, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_autocov_groups(M, A)) return rc;
    const int64_t Q = M * A;
    if (int rc = check_autocov_shape(n, ldh, Q, t0, t1, L)) return rc;
    if (int rc = check_not_null({{"H", H}, {"mean", mean}, {"m2", m2}, {"pooled", pooled}})) return rc;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const int64_t steps = t1 - t0;
    const double *dH = sg.in(H + t0 * ldh, (size_t)ldh, (size_t)Q, (size_t)steps);
    double *dM = sg.out(mean, (size_t)Q), *dP = sg.out(pooled, (size_t)L * A);
    double *dS = (double *)sg.scratch((size_t)L * Q * sizeof(double));                  // s stays on the device: only its row 0 goes back
    sg.down(dS, m2, 0, (size_t)Q * sizeof(double), 1);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_mcmc_autocov_dev(dH, steps, Q, Q, 0, steps, L, dM, dS, Q, sg.stream())) return rc;
    if (int rc = trpl_mcmc_autocov_pool_dev(dS, L, Q, M, A, dP, sg.stream())) return rc;
    return sg.finish(seconds);
}

}  // extern "C"
