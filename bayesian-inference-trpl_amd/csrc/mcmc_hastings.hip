// The two producers of a Hastings term (trpl_mcmc_propose_stretch*, trpl_mcmc_prior_term*, include/trpl.h): the
// untempered additive log term h per chain that trpl_mcmc_accept_h and trpl_mcmc_levels_h (mcmc.hip: hastings_accept_kernel,
// hastings_levels_kernel) take into the accept rule and the early-rejection level.  The affine-invariant stretch move's h is ln z^(A - 1); an
// independent Gaussian prior's, in unit coordinates, is ln p(u') - ln p(u).  Both are for a ladder of temperatures; K = 1 is the
// single temperature.
//
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
struct PriorCall {
    const double *U, *Up; int64_t count; int32_t A; const double *mean, *sd, *h_in; double *h_out;
    mcmc::Prior pr = {};
};

// ---- check: the stretch refuses what trpl_mcmc_propose_rungs refuses, in its order, then its own
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
