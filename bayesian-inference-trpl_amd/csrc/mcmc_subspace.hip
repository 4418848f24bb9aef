// The subspace differential-evolution proposal (trpl_mcmc_propose_subspace*, include/trpl.h): DREAM's move
// (Vrugt et al. 2009) on the split ensemble -- a random subset of the coordinates is moved along the sum of up to
// TRPL_MCMC_MAX_PAIRS difference vectors of the other half, with a gamma chosen for the subset's size and the number of pairs and a
// small multiplicative jitter on the jump.  It is symmetric, so trpl_mcmc_accept* and trpl_mcmc_levels* take it as they stand.  For a
// ladder of rungs; K = 1 is the single temperature.
//
//   subspace_kernel<A, FOLD>    one thread per chain i, keyed n = chain0 + i.  Call 0x100 + 28: xi_m = res53(x0, x1) picks the
//       crossover class m, the first index with xi_m < cdf[m] (the last class if none), CR = (m + 1) / ncr; t = res53(x2, x3) pairs,
//       delta = min((int)t, pairs - 1) + 1 the number of pairs and xi_f = t - (delta - 1), the fraction of the same uniform, which is
//       independent of its integer part, the fallback's.  Calls 0x100 + 12 + j: c_2j, c_2j+1; coordinate d is selected when c_d < CR,
//       and if none is, coordinate min((int)(xi_f A), A - 1) alone.  Pair 0 is propose_body's partner call 0x100 + 8, pair p >= 1 call
//       0x100 + 28 + p, each by propose_body's index expressions on P = group, inside the chain's rung of `partners`.  D_d = the sum
//       over p < delta, ascending from the first term, of (pa_p[d] - pb_p[d]); g = tab[delta - 1][dsel - 1]; for a selected d, with
//       v_d of calls 0x100 + 20 + j and xi_d of the draws' calls 0x100 + j,
//           u'_d = (u_d + (g (1 + e_width (2 v_d - 1))) D_d) + scale_d (2 xi_d - 1)
//       then propose_body's range test or fold; an unselected d keeps u_d's bits and takes no part in `inside`.  X from u' as
//       propose_body forms it.  mask = the selected bits, sel = delta | m << 8.
//   With ncr = 1, pairs = 1, e_width = 0 and a table filled with gamma every output is propose_rungs_kernel's bit for bit: CR = 1
//   selects every coordinate (c_d < 1 always), pair 0 and the jitter are the same calls, 1.0 + (+-0.0) = 1.0 and g * 1.0 = g.
// Per-coordinate arrays are indexed by unrolled loop counters only, so they stay in registers; the table and the class boundaries
// travel by value and are read from the kernel argument.
// The host half has mcmc.hip's structure: one argument record with check, launch and stage, and the two forms of an entry point from
// mcmc_common.hpp.
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

struct Subspace {                                                // what the move takes by value, like Scale and Ladder
    double s[16];                                                // the additive jitter's half-width per coordinate
    double cdf[TRPL_MCMC_MAX_CR];                                // cumulative class probabilities; cdf[ncr - 1] is never read
    double g[TRPL_MCMC_MAX_PAIRS][16];                           // gamma by (delta - 1, dsel - 1)
    double e_width;
    int32_t pairs, ncr;
};

// the two distinct rows (a, b) of a rung of `group` partners from one Philox call: propose_body's expressions with P = group
__device__ __forceinline__ void partner_pair(uint64_t n, uint32_t call, uint32_t step, uint32_t seed_lo, uint32_t seed_hi, int64_t group,
                                             int64_t &a, int64_t &b)
{
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + call, step, seed_lo, seed_hi, r);
    const double xa = res53(r[0], r[1]), xb = res53(r[2], r[3]);
    a = (int64_t)(xa * (double)group);
    b = (int64_t)(xb * (double)(group - 1));
    a = a < group - 1 ? a : group - 1;
    b = b < group - 2 ? b : group - 2;
    b += b >= a;
}

template <int A, bool FOLD>
__global__ void __launch_bounds__(kThreads) subspace_kernel(const double *U, const double *partners, int64_t count, int64_t group,
                                                            const Subspace sp, int64_t chain0, uint32_t seed_lo, uint32_t seed_hi,
                                                            uint32_t step, const Box bx, double *Up, double *Xp, int32_t *inside,
                                                            int32_t *mask, int32_t *sel)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    partners += (i / group) * group * A;                         // count <= P and P a multiple of group: the rung is below P
    const uint64_t n = (uint64_t)(chain0 + i);
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kSelectCall, step, seed_lo, seed_hi, r);
    const double xm = res53(r[0], r[1]);
    int m = sp.ncr - 1;
#pragma unroll
    for (int k = TRPL_MCMC_MAX_CR - 2; k >= 0; k--)
        if (k < sp.ncr - 1 && xm < sp.cdf[k]) m = k;             // descending: the first class with xm < cdf[k] is left standing
    const double cr = (double)(m + 1) / (double)sp.ncr;
    const double t = res53(r[2], r[3]) * (double)sp.pairs;
    int delta = (int)t;
    delta = (delta < sp.pairs - 1 ? delta : sp.pairs - 1) + 1;
    const double xf = t - (double)(delta - 1);
    int f = (int)(xf * (double)A);
    f = f < A - 1 ? f : A - 1;
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; 2 * j < A; j++) {
        philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kCrossCall + (uint32_t)j, step, seed_lo, seed_hi, r);
        if (res53(r[0], r[1]) < cr) bits |= 1u << (2 * j);
        if (2 * j + 1 < A && res53(r[2], r[3]) < cr) bits |= 1u << (2 * j + 1);
    }
    if (bits == 0) bits = 1u << f;
    const int dsel = __popc(bits);
    double u[A], D[A];
#pragma unroll
    for (int d = 0; d < A; d++) u[d] = U[i * A + d];
    {
        int64_t a, b;
        partner_pair(n, kPartnerCall, step, seed_lo, seed_hi, group, a, b);
        const double *pa = partners + a * A, *pb = partners + b * A;
#pragma unroll
        for (int d = 0; d < A; d++) D[d] = pa[d] - pb[d];
    }
#pragma unroll
    for (int p = 1; p < TRPL_MCMC_MAX_PAIRS; p++) {
        if (p < delta) {
            int64_t a, b;
            partner_pair(n, kPairCall + (uint32_t)p, step, seed_lo, seed_hi, group, a, b);
            const double *pa = partners + a * A, *pb = partners + b * A;
#pragma unroll
            for (int d = 0; d < A; d++) D[d] = D[d] + (pa[d] - pb[d]);
        }
    }
    const double g = sp.g[delta - 1][dsel - 1];
    bool in = true, folded = false;
    double *row = Xp + i * bx.ncol;
    put_fixed(bx, row);
#pragma unroll
    for (int j = 0; 2 * j < A; j++) {
        uint32_t rx[4], rv[4];
        philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + (uint32_t)j, step, seed_lo, seed_hi, rx);
        philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), kStream + kJumpCall + (uint32_t)j, step, seed_lo, seed_hi, rv);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int d = 2 * j + h;
            if (d < A) {
                if (bits >> d & 1u) {
                    const double xi = res53(rx[2 * h], rx[2 * h + 1]), v = res53(rv[2 * h], rv[2 * h + 1]);
                    double w = (u[d] + (g * (1.0 + sp.e_width * (2.0 * v - 1.0))) * D[d]) + sp.s[d] * (2.0 * xi - 1.0);
                    if (FOLD) {
                        if (!(w >= 0.0 && w <= 1.0)) {
                            w = fold_outside(w);
                            folded = true;
                        }
                        in = in && w == w;                       // after the fold only a NaN is left outside
                    } else {
                        in = in && w >= 0.0 && w <= 1.0;         // a NaN is outside
                    }
                    u[d] = w;
                }
                Up[i * A + d] = u[d];
                const int c = bx.act[d];
                row[c] = column_value(bx, c, u[d]);
            }
        }
    }
    put_overrides(bx, row);
    inside[i] = !in ? 0 : folded ? 2 : 1;
    mask[i] = (int32_t)bits;
    sel[i] = delta | m << 8;
}

}  // namespace mcmc
}  // namespace trpl

using namespace trpl;

namespace {                                                      // the host half: mcmc.hip's file comment has its structure

struct SubspaceCall {
    const double *U, *partners; int64_t count, P, group; int32_t A; double gamma; const double *scale; int64_t chain0; uint64_t seed;
    uint32_t step; int32_t ncol; const double *lo, *hi; const int32_t *do_log; uint32_t flags; double *Up, *Xp; int32_t *inside;
    int32_t pairs, ncr; const double *pcr, *gamma_tab; double e_width; int32_t *mask, *sel;
    mcmc::Subspace sp = {}; refine::Box bx = {};
};

// ---- check: what trpl_mcmc_propose_rungs refuses, in its order, then the move's own
int check(SubspaceCall &k)
{
    if (int rc = check_chains(k.count, k.A, k.chain0)) return rc;
    if (k.P < 0 || k.P == 1) return api_fail(TRPL_ERR_ARG, "P=%lld must be >= 2", (long long)k.P);
    if (k.P > 0 && !k.partners) return api_fail(TRPL_ERR_ARG, "partners is NULL with P=%lld", (long long)k.P);
    if (int rc = check_not_null({{"U", k.U}, {"scale", k.scale}, {"Up", k.Up}, {"Xp", k.Xp}, {"inside", k.inside}})) return rc;
    if (!isfinite(k.gamma)) return api_fail(TRPL_ERR_ARG, "gamma=%g must be finite", k.gamma);
    if (k.flags & ~(uint32_t)(TRPL_BOX_EQUAL_MU | TRPL_BOX_EQUAL_S | TRPL_BOX_EQUAL_AUGER | TRPL_MCMC_FOLD))
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: only the TRPL_BOX_EQUAL_* bits and TRPL_MCMC_FOLD apply", k.flags);
    for (int d = 0; d < k.A; d++) {
        if (!(isfinite(k.scale[d]) && k.scale[d] >= 0.0)) return api_fail(TRPL_ERR_ARG, "scale[%d]=%g must be finite and >= 0", d, k.scale[d]);
        k.sp.s[d] = k.scale[d];
    }
    if (k.group < 2) return api_fail(TRPL_ERR_ARG, "group=%lld must be >= 2", (long long)k.group);
    if (k.P < k.group || k.P % k.group)
        return api_fail(TRPL_ERR_ARG, "P=%lld must be a positive multiple of group=%lld", (long long)k.P, (long long)k.group);
    if (k.count > k.P) return api_fail(TRPL_ERR_ARG, "count=%lld must be <= P=%lld", (long long)k.count, (long long)k.P);
    if (k.pairs < 1 || k.pairs > TRPL_MCMC_MAX_PAIRS)
        return api_fail(TRPL_ERR_ARG, "pairs=%d must be in [1, TRPL_MCMC_MAX_PAIRS = %d]", k.pairs, TRPL_MCMC_MAX_PAIRS);
    if (k.ncr < 1 || k.ncr > TRPL_MCMC_MAX_CR) return api_fail(TRPL_ERR_ARG, "ncr=%d must be in [1, TRPL_MCMC_MAX_CR = %d]", k.ncr, TRPL_MCMC_MAX_CR);
    if (k.pcr) {
        double sum = 0.0;
        for (int m = 0; m < k.ncr; m++) {
            if (!(isfinite(k.pcr[m]) && k.pcr[m] >= 0.0)) return api_fail(TRPL_ERR_ARG, "pcr[%d]=%g must be finite and >= 0", m, k.pcr[m]);
            sum = sum + k.pcr[m];
        }
        if (!(sum > 0.0 && isfinite(sum))) return api_fail(TRPL_ERR_ARG, "pcr: the sum %g of the %d shares must be > 0", sum, k.ncr);
        double c = 0.0;
        for (int m = 0; m < k.ncr; m++) {
            c = c + k.pcr[m];
            k.sp.cdf[m] = c / sum;
        }
    } else {
        for (int m = 0; m < k.ncr; m++) k.sp.cdf[m] = (double)(m + 1) / (double)k.ncr;
    }
    for (int p = 0; k.gamma_tab && p < k.pairs; p++)
        for (int d = 0; d < k.A; d++) {
            const double g = k.gamma_tab[p * k.A + d];
            if (!isfinite(g)) return api_fail(TRPL_ERR_ARG, "gamma_tab[%d][%d]=%g must be finite", p, d, g);
            k.sp.g[p][d] = g;
        }
    if (!(k.e_width >= 0.0 && k.e_width < 1.0)) return api_fail(TRPL_ERR_ARG, "e_width=%g must be in [0, 1)", k.e_width);
    if (int rc = check_not_null({{"gamma_tab", k.gamma_tab}, {"mask", k.mask}, {"sel", k.sel}})) return rc;
    k.sp.e_width = k.e_width; k.sp.pairs = k.pairs; k.sp.ncr = k.ncr;
    return refine_make_box(k.ncol, k.lo, k.hi, k.do_log, k.flags & ~(uint32_t)TRPL_MCMC_FOLD, k.A, k.bx);
}

// ---- launch
int launch(const SubspaceCall &k, hipStream_t stream)
{
    const bool fold = (k.flags & TRPL_MCMC_FOLD) != 0;
    TRPL_MCMC_LAUNCH(k.A, (fold ? mcmc::subspace_kernel<n, true> : mcmc::subspace_kernel<n, false>), k.count, stream, k.U, k.partners, k.count,
                     k.group, k.sp, k.chain0, (uint32_t)k.seed, (uint32_t)(k.seed >> 32), k.step, k.bx, k.Up, k.Xp, k.inside, k.mask, k.sel)
    return refine_launched("mcmc propose subspace");
}

// ---- stage
void stage(SubspaceCall &k, Staged &sg)
{
    const size_t n = (size_t)k.count;
    k.partners = sg.in(k.partners, (size_t)k.P * k.A); k.U = sg.in(k.U, n * k.A);
    k.Up = sg.out(k.Up, n * k.A); k.Xp = sg.out(k.Xp, n * k.ncol); k.inside = sg.out(k.inside, n);
    k.mask = sg.out(k.mask, n); k.sel = sg.out(k.sel, n);
}

}  // namespace

extern "C" {

int trpl_mcmc_propose_subspace_dev(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double gamma,
                                   const double *scale, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo,
                                   const double *hi, const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside,
                                   int32_t pairs, int32_t ncr, const double *pcr, const double *gamma_tab, double e_width, int32_t *mask,
                                   int32_t *sel, void *stream)
{
    return on_stream(SubspaceCall{U, partners, count, P, group, A, gamma, scale, chain0, seed, step, ncol, lo, hi, do_log, flags, Up, Xp, inside,
                                  pairs, ncr, pcr, gamma_tab, e_width, mask, sel}, stream);
}

int trpl_mcmc_propose_subspace(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double gamma,
                               const double *scale, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo,
                               const double *hi, const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside,
                               int32_t pairs, int32_t ncr, const double *pcr, const double *gamma_tab, double e_width, int32_t *mask,
                               int32_t *sel, int32_t device, double *seconds)
{
    return staged(SubspaceCall{U, partners, count, P, group, A, gamma, scale, chain0, seed, step, ncol, lo, hi, do_log, flags, Up, Xp, inside,
                               pairs, ncr, pcr, gamma_tab, e_width, mask, sel}, device, seconds);
}

}  // extern "C"
