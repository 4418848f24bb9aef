// The Metropolis-Hastings half of the ensemble sampler (trpl_mcmc_propose_stretch*, trpl_mcmc_accept_h*, trpl_mcmc_levels_h*,
// trpl_mcmc_prior_term*, include/trpl.h): an untempered additive log term h per chain in the accept rule and in
// the early-rejection level, and the two users of it -- the affine-invariant stretch move, whose h is ln z^(A - 1), and an independent
// Gaussian prior in unit coordinates, whose h is ln p(u') - ln p(u).  Everything is for a ladder of temperatures; K = 1 is the single
// temperature.
//
//   hastings_accept_kernel<A>   accept_body of mcmc.hip with h: the same Philox call (0x100 + 9, key (seed; chain0 + i, step)), the
//       same copy of the rows, the same `accepted`.  d = (LLp - LL) / tf[i / group] + h[i]; the proposal is taken when it is inside,
//       LLp and h are neither NaN nor -inf, and the chain stands on a likelihood that is not above -inf, or d >= 0, or log(xi) < d.
//       With h = +0.0 the sum changes no value but -0.0, which no comparison sees: accept_rungs_kernel's outputs bit for bit.
//   hastings_levels_kernel      levels_body of mcmc.hip with h: l0 = -(LL + tf (log(xi) - h)), then l0 + (fabs(LL) + l0) 2^-40; a
//       candidate l is taken only if the accept kernel's own dq = (-l - LL) / tf + h satisfies dq < 0 && !(log(xi) < dq).  +inf where
//       levels_body gives +inf, and where h is NaN or infinite.  The monotonicity argument of mcmc.hip survives the added constant:
//       every LLp <= -l has (LLp - LL) / tf <= (-l - LL) / tf as before, and adding the same h to both sides is monotone under
//       round-to-nearest, so d <= dq: d < 0 and log(xi) < d is false, and hastings_accept_kernel rejects with the same (seed, chain,
//       step, h).  The argument never compares two chains, so it holds with a temperature per rung.  With h = +0.0, lx - 0.0 is lx and
//       dq + 0.0 compares as dq: levels_rungs_kernel's bits.
//   stretch_kernel<A>           one stretch proposal per chain (Goodman & Weare 2010, in the split-ensemble form of Foreman-Mackey
//       et al. 2013): the partner row p = partners[(i / group) group + a], a = min((int64)(xa group), group - 1), xa the first uniform
//       of the partner call 0x100 + 8; xi the first uniform of call 0x100 + 11; s = (a_par - 1) xi + 1, z = s s / a_par (the density
//       proportional to 1 / sqrt(z) on [1 / a_par, a_par]); u'_d = p_d + z (u_d - p_d).  inside = every u'_d in [0, 1] (a NaN is
//       outside); X from u' either way; z and lnq = (double)(A - 1) log(z), the Hastings term of the move.  No jitter and no fold: a
//       stretch reflected at a face is not reversible through the same partner (the reverse move from the folded point along its
//       line through p does not lead back to u), so z^(A - 1) would no longer be its ratio.
//   prior_term_kernel<A>        h_out = h_in + (lnp(u') - lnp(u)), lnp(u) = sum over d ascending from +0.0 of (-0.5 t) t,
//       t = (u_d - m_d) / sd_d; a column with sd_d = +inf adds exactly +0.0.  h_in NULL is +0.0.  m and sd travel by value.
// The host half has mcmc.hip's structure: one argument record per operation with check, launch and stage, and the two forms of an
// entry point from mcmc_common.hpp.
// Compiled with -ffp-contract=off like mcmc.hip: every result is its expression with one rounding per operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "mcmc_common.hpp"
#include "refine_common.hpp"

namespace trpl {
namespace mcmc {

using namespace refine;

struct Prior {                                                   // the Gaussian of every active column, by value like Scale
    double m[16], sd[16];
};

template <int A>
__global__ void __launch_bounds__(kThreads) stretch_kernel(const double *U, const double *partners, int64_t count, int64_t group,
                                                           double a_par, int64_t chain0, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                           const Box bx, double *Up, double *Xp, int32_t *inside, double *z_out, double *lnq)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const uint64_t n = (uint64_t)(chain0 + i);
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kPartnerCall, step, seed_lo, seed_hi, r);
    const double xa = res53(r[0], r[1]);
    int64_t a = (int64_t)(xa * (double)group);
    a = a < group - 1 ? a : group - 1;
    const double *p = partners + ((i / group) * group + a) * A;  // count <= P and P a multiple of group: the row is below P
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kStretchCall, step, seed_lo, seed_hi, r);
    const double xi = res53(r[0], r[1]);
    const double s = (a_par - 1.0) * xi + 1.0;
    const double z = s * s / a_par;
    bool in = true;
    double *row = Xp + i * bx.ncol;
    put_fixed(bx, row);
#pragma unroll
    for (int d = 0; d < A; d++) {
        const double pd = p[d];
        const double u = pd + z * (U[i * A + d] - pd);
        in = in && u >= 0.0 && u <= 1.0;                         // a NaN is outside
        Up[i * A + d] = u;
        const int c = bx.act[d];
        row[c] = column_value(bx, c, u);
    }
    put_overrides(bx, row);
    inside[i] = in ? 1 : 0;
    z_out[i] = z;
    lnq[i] = (double)(A - 1) * log(z);
}

template <int A>
__global__ void __launch_bounds__(kThreads) hastings_accept_kernel(double *U, double *X, double *LL, const double *Up, const double *Xp,
                                                                   const double *LLp, const int32_t *inside, const double *h, int64_t count,
                                                                   int32_t ncol, const Ladder tf, int64_t group, int64_t chain0,
                                                                   uint32_t seed_lo, uint32_t seed_hi, uint32_t step, int32_t *accepted)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const uint64_t n = (uint64_t)(chain0 + i);
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kAcceptCall, step, seed_lo, seed_hi, r);
    const double xi = res53(r[0], r[1]);
    const double ll = LL[i], llp = LLp[i], hv = h[i];
    const double d = (llp - ll) / tf.tf[i / group] + hv;
    const bool take = inside[i] != 0 && !(llp != llp) && llp > -INFINITY && !(hv != hv) && hv > -INFINITY &&
                      (!(ll > -INFINITY) || d >= 0.0 || log(xi) < d);
    accepted[i] = take ? 1 : 0;
    if (!take) return;
#pragma unroll
    for (int k = 0; k < A; k++) U[i * A + k] = Up[i * A + k];
    for (int c = 0; c < ncol; c++) X[i * ncol + c] = Xp[i * ncol + c];
    LL[i] = llp;
}

__global__ void __launch_bounds__(kThreads) hastings_levels_kernel(const double *LL, const double *h, int64_t count, const Ladder tf,
                                                                   int64_t group, int64_t chain0, uint32_t seed_lo, uint32_t seed_hi,
                                                                   uint32_t step, double *level)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const uint64_t n = (uint64_t)(chain0 + i);
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kAcceptCall, step, seed_lo, seed_hi, r);
    const double xi = res53(r[0], r[1]);
    const double ll = LL[i], hv = h[i], t = tf.tf[i / group];
    double lv = INFINITY;
    if (!(ll != ll) && ll > -INFINITY && xi != 0.0 && !(hv != hv) && fabs(hv) < INFINITY) {
        const double lx = log(xi);
        const double l0 = -(ll + t * (lx - hv));
        double cand = l0;
        for (int k = 0; k < 2; k++) {
            const double q = -cand;
            const double dq = (q - ll) / t + hv;
            if (dq < 0.0 && !(lx < dq)) { lv = cand; break; }
            cand = l0 + (fabs(ll) + l0) * 0x1p-40;
        }
    }
    level[i] = lv;
}

template <int A>
__device__ __forceinline__ double log_prior(const double *u, const Prior &pr)
{
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < A; d++) {
        const double t = (u[d] - pr.m[d]) / pr.sd[d];
        s = s + (pr.sd[d] == INFINITY ? 0.0 : (-0.5 * t) * t);   // a flat column adds exactly +0.0, whatever u is
    }
    return s;
}

template <int A>
__global__ void __launch_bounds__(kThreads) prior_term_kernel(const double *U, const double *Up, int64_t count, const Prior pr,
                                                              const double *h_in, double *h_out)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const double h0 = h_in ? h_in[i] : 0.0;
    h_out[i] = h0 + (log_prior<A>(Up + i * A, pr) - log_prior<A>(U + i * A, pr));
}

}  // namespace mcmc
}  // namespace trpl

using namespace trpl;

namespace {                                                      // the host half: mcmc.hip's file comment has its structure

struct StretchCall {
    const double *U, *partners; int64_t count, P, group; int32_t A; double a; int64_t chain0; uint64_t seed; uint32_t step; int32_t ncol;
    const double *lo, *hi; const int32_t *do_log; uint32_t flags; double *Up, *Xp; int32_t *inside; double *z, *lnq;
    refine::Box bx = {};
};
struct AcceptHCall {
    double *U, *X, *LL; const double *Up, *Xp, *LLp; const int32_t *inside; const double *h; int64_t count; int32_t A, ncol, K;
    int64_t group; const double *ladder; int64_t chain0; uint64_t seed; uint32_t step; int32_t *accepted;
    mcmc::Ladder lad = {};
};
struct LevelsHCall {
    const double *LL, *h; int64_t count; int32_t K; int64_t group; const double *ladder; int64_t chain0; uint64_t seed; uint32_t step;
    double *level;
    mcmc::Ladder lad = {};
};
struct PriorCall {
    const double *U, *Up; int64_t count; int32_t A; const double *mean, *sd, *h_in; double *h_out;
    mcmc::Prior pr = {};
};

// ---- check: the refusals of the *_rungs counterpart in its order, then the call's own
int check(StretchCall &k)
{
    if (int rc = check_chains(k.count, k.A, k.chain0)) return rc;
    if (k.P < 1) return api_fail(TRPL_ERR_ARG, "P=%lld must be >= 1", (long long)k.P);
    if (int rc = check_not_null({{"partners", k.partners}, {"U", k.U}, {"Up", k.Up}, {"Xp", k.Xp}, {"inside", k.inside}, {"z", k.z},
                                 {"lnq", k.lnq}}))
        return rc;
    if (!(isfinite(k.a) && k.a > 1.0)) return api_fail(TRPL_ERR_ARG, "a=%g must be finite and > 1", k.a);
    if (k.flags & TRPL_MCMC_FOLD)
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: TRPL_MCMC_FOLD does not apply to the stretch move, whose reflection is not reversible",
                        k.flags);
    if (k.flags & ~(uint32_t)(TRPL_BOX_EQUAL_MU | TRPL_BOX_EQUAL_S | TRPL_BOX_EQUAL_AUGER))
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: only the TRPL_BOX_EQUAL_* bits apply", k.flags);
    if (k.group < 1) return api_fail(TRPL_ERR_ARG, "group=%lld must be >= 1", (long long)k.group);
    if (k.P % k.group) return api_fail(TRPL_ERR_ARG, "P=%lld must be a positive multiple of group=%lld", (long long)k.P, (long long)k.group);
    if (k.count > k.P) return api_fail(TRPL_ERR_ARG, "count=%lld must be <= P=%lld", (long long)k.count, (long long)k.P);
    return refine_make_box(k.ncol, k.lo, k.hi, k.do_log, k.flags, k.A, k.bx);
}

int check(AcceptHCall &k)
{
    if (int rc = check_ladder(k.K, k.group, k.ladder, k.lad)) return rc;
    if (int rc = check_chains(k.count, k.A, k.chain0)) return rc;
    if (k.ncol < 1 || k.ncol > 16) return api_fail(TRPL_ERR_ARG, "ncol=%d must be in [1, 16]", k.ncol);
    if (int rc = check_not_null({{"U", k.U}, {"X", k.X}, {"LL", k.LL}, {"Up", k.Up}, {"Xp", k.Xp}, {"LLp", k.LLp}, {"inside", k.inside},
                                 {"h", k.h}, {"accepted", k.accepted}}))
        return rc;
    if (k.count != (int64_t)k.K * k.group)
        return api_fail(TRPL_ERR_ARG, "count=%lld must be K * group = %d * %lld", (long long)k.count, k.K, (long long)k.group);
    return TRPL_OK;
}

int check(LevelsHCall &k)
{
    if (int rc = check_ladder(k.K, k.group, k.ladder, k.lad)) return rc;
    if (int rc = check_count(k.count)) return rc;
    if (k.chain0 < 0) return api_fail(TRPL_ERR_ARG, "chain0=%lld must be >= 0", (long long)k.chain0);
    if (int rc = check_not_null({{"LL", k.LL}, {"h", k.h}, {"level", k.level}})) return rc;
    if (k.count != (int64_t)k.K * k.group)
        return api_fail(TRPL_ERR_ARG, "count=%lld must be K * group = %d * %lld", (long long)k.count, k.K, (long long)k.group);
    return TRPL_OK;
}

int check(PriorCall &k)
{
    if (int rc = check_count(k.count)) return rc;
    if (k.A < 1 || k.A > TRPL_REFINE_MAX_DIMS) return api_fail(TRPL_ERR_ARG, "A=%d must be in [1, %d]", k.A, TRPL_REFINE_MAX_DIMS);
    if (int rc = check_not_null({{"U", k.U}, {"Up", k.Up}, {"mean", k.mean}, {"sd", k.sd}, {"h_out", k.h_out}})) return rc;
    for (int d = 0; d < k.A; d++) {
        if (!isfinite(k.mean[d])) return api_fail(TRPL_ERR_ARG, "mean[%d]=%g must be finite", d, k.mean[d]);
        if (!(k.sd[d] > 0.0)) return api_fail(TRPL_ERR_ARG, "sd[%d]=%g must be > 0 (+inf: a flat column)", d, k.sd[d]);
        k.pr.m[d] = k.mean[d];
        k.pr.sd[d] = k.sd[d];
    }
    return TRPL_OK;
}

// ---- launch
int launch(const StretchCall &k, hipStream_t stream)
{
    TRPL_MCMC_LAUNCH(k.A, mcmc::stretch_kernel<n>, k.count, stream, k.U, k.partners, k.count, k.group, k.a, k.chain0, (uint32_t)k.seed,
                     (uint32_t)(k.seed >> 32), k.step, k.bx, k.Up, k.Xp, k.inside, k.z, k.lnq)
    return refine_launched("mcmc propose stretch");
}

int launch(const AcceptHCall &k, hipStream_t stream)
{
    TRPL_MCMC_LAUNCH(k.A, mcmc::hastings_accept_kernel<n>, k.count, stream, k.U, k.X, k.LL, k.Up, k.Xp, k.LLp, k.inside, k.h, k.count, k.ncol,
                     k.lad, k.group, k.chain0, (uint32_t)k.seed, (uint32_t)(k.seed >> 32), k.step, k.accepted)
    return refine_launched("mcmc accept h");
}

int launch(const LevelsHCall &k, hipStream_t stream)
{
    hipLaunchKernelGGL(mcmc::hastings_levels_kernel, dim3(refine_blocks(k.count)), dim3(refine::kThreads), 0, stream, k.LL, k.h, k.count, k.lad,
                       k.group, k.chain0, (uint32_t)k.seed, (uint32_t)(k.seed >> 32), k.step, k.level);
    return refine_launched("mcmc levels h");
}

int launch(const PriorCall &k, hipStream_t stream)
{
    TRPL_MCMC_LAUNCH(k.A, mcmc::prior_term_kernel<n>, k.count, stream, k.U, k.Up, k.count, k.pr, k.h_in, k.h_out)
    return refine_launched("mcmc prior term");
}

// ---- stage
void stage(StretchCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    k.partners = sg.in(k.partners, (size_t)k.P * k.A); k.U = sg.in(k.U, n * k.A);
    k.Up = sg.out(k.Up, n * k.A); k.Xp = sg.out(k.Xp, n * k.ncol); k.inside = sg.out(k.inside, n);
    k.z = sg.out(k.z, n); k.lnq = sg.out(k.lnq, n);
}

void stage(AcceptHCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    k.U = sg.inout(k.U, n * k.A); k.X = sg.inout(k.X, n * k.ncol); k.LL = sg.inout(k.LL, n);
    k.Up = sg.in(k.Up, n * k.A); k.Xp = sg.in(k.Xp, n * k.ncol); k.LLp = sg.in(k.LLp, n);
    k.inside = sg.in(k.inside, n); k.h = sg.in(k.h, n); k.accepted = sg.out(k.accepted, n);
}

void stage(LevelsHCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    k.LL = sg.in(k.LL, n); k.h = sg.in(k.h, n); k.level = sg.out(k.level, n);
}

void stage(PriorCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    k.U = sg.in(k.U, n * k.A); k.Up = sg.in(k.Up, n * k.A);
    if (k.h_in) k.h_in = sg.in(k.h_in, n);                       // NULL stays NULL: the kernel reads +0.0
    k.h_out = sg.out(k.h_out, n);
}

}  // namespace

extern "C" {

int trpl_mcmc_propose_stretch_dev(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double a,
                                  int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo, const double *hi,
                                  const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside, double *z, double *lnq,
                                  void *stream)
{
    return on_stream(StretchCall{U, partners, count, P, group, A, a, chain0, seed, step, ncol, lo, hi, do_log, flags, Up, Xp, inside, z, lnq},
                     stream);
}

int trpl_mcmc_propose_stretch(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double a,
                              int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo, const double *hi,
                              const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside, double *z, double *lnq,
                              int32_t device, double *seconds)
{
    return staged(StretchCall{U, partners, count, P, group, A, a, chain0, seed, step, ncol, lo, hi, do_log, flags, Up, Xp, inside, z, lnq},
                  device, seconds);
}

int trpl_mcmc_accept_h_dev(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                           const double *h, int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group, const double *tf,
                           int64_t chain0, uint64_t seed, uint32_t step, int32_t *accepted, void *stream)
{
    return on_stream(AcceptHCall{U, X, LL, Up, Xp, LLp, inside, h, count, A, ncol, K, group, tf, chain0, seed, step, accepted}, stream);
}

int trpl_mcmc_accept_h(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                       const double *h, int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group, const double *tf, int64_t chain0,
                       uint64_t seed, uint32_t step, int32_t *accepted, int32_t device, double *seconds)
{
    return staged(AcceptHCall{U, X, LL, Up, Xp, LLp, inside, h, count, A, ncol, K, group, tf, chain0, seed, step, accepted}, device, seconds);
}

int trpl_mcmc_levels_h_dev(const double *LL, const double *h, int64_t count, int32_t K, int64_t group, const double *tf, int64_t chain0,
                           uint64_t seed, uint32_t step, double *level, void *stream)
{
    return on_stream(LevelsHCall{LL, h, count, K, group, tf, chain0, seed, step, level}, stream);
}

int trpl_mcmc_levels_h(const double *LL, const double *h, int64_t count, int32_t K, int64_t group, const double *tf, int64_t chain0,
                       uint64_t seed, uint32_t step, double *level, int32_t device, double *seconds)
{
    return staged(LevelsHCall{LL, h, count, K, group, tf, chain0, seed, step, level}, device, seconds);
}

int trpl_mcmc_prior_term_dev(const double *U, const double *Up, int64_t count, int32_t A, const double *mean, const double *sd,
                             const double *h_in, double *h_out, void *stream)
{
    return on_stream(PriorCall{U, Up, count, A, mean, sd, h_in, h_out}, stream);
}

int trpl_mcmc_prior_term(const double *U, const double *Up, int64_t count, int32_t A, const double *mean, const double *sd,
                         const double *h_in, double *h_out, int32_t device, double *seconds)
{
    return staged(PriorCall{U, Up, count, A, mean, sd, h_in, h_out}, device, seconds);
}

}  // extern "C"
