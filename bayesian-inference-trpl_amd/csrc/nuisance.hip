// One reduction over the nuisance grid of an experiment (trpl_nuisance_reduce*, include/trpl.h): the J responses of a bank x M
// magnitude offsets, from the moments sse, esum [C][J][S] that trpl_loglik_irf_bank* left in HBM.  The value of a cell shares
// mag_term, the ordered curve sum and the shared-offset profile with likelihood.hip's trpl_mag_grid* and trpl_mag_profile*
// (mag_moments.hpp) and restates irf.loglik_bank's P -= sse; the maximum restates irf_bank.hip's profile_one.  ONE body, compiled
// for the host and for the device in this translation unit (-ffp-contract=off: no fused multiply-add on either side, IEEE divide),
// so that the plain host form and the kernel agree bit for bit wherever no exp or log is taken.
//
// Loop order.  One thread per sample, a wavefront's loads contiguous along s.  Per thread the responses j are the outer loop; under
// GRID the offsets go kTile at a time with their sums in registers and the curves inside, so that a sample's 2 C moments of response j
// are loaded once per kTile offsets and every cell sees its curves in ascending c; the cells reach the reduction in ascending
// i = j M + m.  Nothing is held per curve or per cell.  The marginal runs the loop twice -- the greatest a, then the sum of
// exp(a - mx) -- and reads the moments again instead of keeping J M values.  No atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "mag_moments.hpp"

namespace trpl {
namespace nuisance {

constexpr int kTile = 8;                       // offsets of one pass over a response's curves (GRID)
constexpr int kFixed = (int)TRPL_NUISANCE_MAG_FIXED, kGrid = (int)TRPL_NUISANCE_MAG_GRID, kProfile = (int)TRPL_NUISANCE_MAG_PROFILE;
static_assert(TRPL_NUISANCE_MAX_OFFSETS % kTile == 0, "a tile never reads past d[]");

// the host arrays, as kernel arguments (1 KiB)
struct Args {
    double n[TRPL_MAG_MAX_CURVES];             // wsum
    double d[TRPL_NUISANCE_MAX_OFFSETS];       // offsets
};

// f(i, v, d) for every cell of sample s in ascending i = j M + m: its value and the offset it stands for
template <int MODE, typename F>
__host__ __device__ inline void visit(const double *__restrict__ sse, const double *__restrict__ esum, const Args &g, int64_t S, int C,
                                      int J, int M, int64_t s, F &f)
{
    const int64_t JS = (int64_t)J * S;
    for (int j = 0; j < J; j++) {
        const int64_t o = (int64_t)j * S + s;                            // curve c of response j: o + c JS
        if constexpr (MODE == kFixed) {
            double acc = 0.0;
            for (int c = 0; c < C; c++) acc += sse[o + c * JS];
            f(j, 0.0 - acc, 0.0);
        } else if constexpr (MODE == kProfile) {                         // mag_profile_one, one offset for all curves
            const MagShared p = mag_shared_offset(sse + o, esum + o, g.n, JS, C);
            if (p.empty) { f(j, 0.0, (double)NAN); continue; }           // every weight zero: nothing to fit
            f(j, 0.0 - mag_curve_sum(sse + o, esum + o, g.n, JS, C, p.d), p.best);
        } else {
            for (int m0 = 0; m0 < M; m0 += kTile) {
                double acc[kTile];
#pragma unroll
                for (int k = 0; k < kTile; k++) acc[k] = 0.0;
                for (int c = 0; c < C; c++) {
                    const double q2 = sse[o + c * JS], q1 = esum[o + c * JS], n = g.n[c];
#pragma unroll
                    for (int k = 0; k < kTile; k++) acc[k] += mag_term(q2, q1, n, g.d[m0 + k]);       // past M: 0.0, never used
                }
#pragma unroll
                for (int k = 0; k < kTile; k++)
                    if (m0 + k < M) f(j * M + m0 + k, 0.0 - acc[k], g.d[m0 + k]);
            }
        }
    }
}

// the greatest value and the first cell that attains it; with MARGINAL of a = v / tf + logw.  NaN never compares greater and -inf is
// not greater than the start, so a sample whose cells are all -inf or NaN keeps best = -1, p = -inf, mag = NaN.
template <bool MARGINAL>
struct Greatest {
    const double *__restrict__ logw;
    double tf;
    double p = -INFINITY, mag = NAN;
    int32_t b = -1;
    __host__ __device__ inline void operator()(int i, double v, double d)
    {
        double a = v;
        if constexpr (MARGINAL) a = v / tf + (logw ? logw[i] : 0.0);
        if (a > p) { p = a; b = i; mag = d; }
    }
};

struct ExpSum {
    const double *__restrict__ logw;
    double tf, mx;
    double sum = 0.0;
    __host__ __device__ inline void operator()(int i, double v, double)
    {
        const double a = v / tf + (logw ? logw[i] : 0.0);
        const double t = a - mx;
        if (t == t) sum += exp(t);
    }
};

template <int MODE, bool MARGINAL>
__host__ __device__ inline void reduce_one(const double *__restrict__ sse, const double *__restrict__ esum, const Args &g, int64_t S, int C,
                                           int J, int M, const double *__restrict__ logw, double tf, int64_t s, double *__restrict__ P,
                                           int32_t *__restrict__ best, double *__restrict__ best_mag)
{
    Greatest<MARGINAL> top{logw, tf};
    visit<MODE>(sse, esum, g, S, C, J, M, s, top);
    double p = top.p;
    if constexpr (MARGINAL) {
        if (top.b >= 0) {
            ExpSum es{logw, tf, top.p};
            visit<MODE>(sse, esum, g, S, C, J, M, s, es);
            p = tf * (top.p + log(es.sum));
        }
    }
    P[s] = p;
    if (best) best[s] = top.b;
    if (best_mag) best_mag[s] = top.mag;
}

template <int MODE, bool MARGINAL>
__global__ void __launch_bounds__(256) reduce(const double *__restrict__ sse, const double *__restrict__ esum, int64_t S, int C, int J, int M,
                                              const double *__restrict__ logw, double tf, double *__restrict__ P,
                                              int32_t *__restrict__ best, double *__restrict__ best_mag, const Args g)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (int64_t)gridDim.x * blockDim.x)
        reduce_one<MODE, MARGINAL>(sse, esum, g, S, C, J, M, logw, tf, s, P, best, best_mag);
}

template <int MODE, bool MARGINAL>
static void reduce_host(const double *sse, const double *esum, const Args &g, int64_t S, int C, int J, int M, const double *logw, double tf,
                        double *P, int32_t *best, double *best_mag)
{
    for (int64_t s = 0; s < S; s++) reduce_one<MODE, MARGINAL>(sse, esum, g, S, C, J, M, logw, tf, s, P, best, best_mag);
}

}  // namespace nuisance
}  // namespace trpl

using namespace trpl;

// what both forms refuse before a device is touched, in the order of include/trpl.h; logw_host: the entries can be looked at
static int check_nuisance(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C, int32_t J, const double *offsets,
                          int32_t M, const double *logw, bool logw_host, double tf, uint32_t flags, const double *P)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 0", (long long)S);
    if (C < 1 || C > TRPL_MAG_MAX_CURVES) return api_fail(TRPL_ERR_ARG, "C=%d must be in [1, TRPL_MAG_MAX_CURVES = %d]", C, TRPL_MAG_MAX_CURVES);
    if (J < 1 || J > TRPL_IRF_BANK_MAX_RESPONSES)
        return api_fail(TRPL_ERR_ARG, "J=%d must be in [1, TRPL_IRF_BANK_MAX_RESPONSES = %d]", J, TRPL_IRF_BANK_MAX_RESPONSES);
    const uint32_t mode = flags & TRPL_NUISANCE_MAG_MASK;
    if (mode > TRPL_NUISANCE_MAG_PROFILE || (flags & ~(TRPL_NUISANCE_MAG_MASK | TRPL_NUISANCE_MARGINAL)))
        return api_fail(TRPL_ERR_ARG, "flags=0x%x: an unknown mag mode or flag bit", flags);
    const bool grid = mode == TRPL_NUISANCE_MAG_GRID, marginal = (flags & TRPL_NUISANCE_MARGINAL) != 0;
    if (grid && (M < 1 || M > TRPL_NUISANCE_MAX_OFFSETS))
        return api_fail(TRPL_ERR_ARG, "M=%d must be in [1, TRPL_NUISANCE_MAX_OFFSETS = %d]", M, TRPL_NUISANCE_MAX_OFFSETS);
    if (!grid && M != 1) return api_fail(TRPL_ERR_ARG, "M=%d must be 1 without TRPL_NUISANCE_MAG_GRID", M);
    if (grid && !offsets) return api_fail(TRPL_ERR_ARG, "offsets is NULL with TRPL_NUISANCE_MAG_GRID");
    if (!grid && offsets) return api_fail(TRPL_ERR_ARG, "offsets must be NULL without TRPL_NUISANCE_MAG_GRID");
    if (!esum && mode != TRPL_NUISANCE_MAG_FIXED) return api_fail(TRPL_ERR_ARG, "esum is NULL: only TRPL_NUISANCE_MAG_FIXED does without it");
    if (wsum)
        for (int c = 0; c < C; c++)
            if (!(wsum[c] >= 0.0) || !(wsum[c] < INFINITY)) return api_fail(TRPL_ERR_ARG, "wsum[%d]=%g must be finite and >= 0", c, wsum[c]);
    if (grid)
        for (int m = 0; m < M; m++)
            if (!isfinite(offsets[m])) return api_fail(TRPL_ERR_ARG, "offsets[%d]=%g is not finite", m, offsets[m]);
    if (marginal) {
        if (!(tf > 0.0) || !(tf < INFINITY)) return api_fail(TRPL_ERR_ARG, "tf=%g must be finite and > 0", tf);
        if (logw && logw_host)
            for (int64_t i = 0; i < (int64_t)J * M; i++)
                if (!(logw[i] < INFINITY)) return api_fail(TRPL_ERR_ARG, "logw[%lld]=%g must not be NaN or +inf", (long long)i, logw[i]);
    } else if (logw) {
        return api_fail(TRPL_ERR_ARG, "logw must be NULL without TRPL_NUISANCE_MARGINAL");
    }
    if (S > 0) {
        if (!sse) return api_fail(TRPL_ERR_ARG, "sse is NULL");
        if (!wsum) return api_fail(TRPL_ERR_ARG, "wsum is NULL");
        if (!P) return api_fail(TRPL_ERR_ARG, "P is NULL");
    }
    return TRPL_OK;
}

static nuisance::Args pack(const double *wsum, int C, const double *offsets, int M)
{
    nuisance::Args g = {};
    for (int c = 0; c < C; c++) g.n[c] = wsum[c];
    for (int m = 0; offsets && m < M; m++) g.d[m] = offsets[m];
    return g;
}

// one line per (mode, reduction): X(MODE, MARGINAL)
#define TRPL_NUISANCE_DISPATCH(X)                                                              \
    do {                                                                                       \
        const uint32_t mode_ = flags & TRPL_NUISANCE_MAG_MASK;                                 \
        if (flags & TRPL_NUISANCE_MARGINAL) {                                                  \
            if (mode_ == TRPL_NUISANCE_MAG_FIXED) X(nuisance::kFixed, true);                   \
            else if (mode_ == TRPL_NUISANCE_MAG_GRID) X(nuisance::kGrid, true);                \
            else X(nuisance::kProfile, true);                                                  \
        } else {                                                                               \
            if (mode_ == TRPL_NUISANCE_MAG_FIXED) X(nuisance::kFixed, false);                  \
            else if (mode_ == TRPL_NUISANCE_MAG_GRID) X(nuisance::kGrid, false);               \
            else X(nuisance::kProfile, false);                                                 \
        }                                                                                      \
    } while (0)

extern "C" {

int trpl_nuisance_max_offsets(void) { return TRPL_NUISANCE_MAX_OFFSETS; }

double trpl_nuisance_bound(double tf, double B, int32_t n, double R) { return TRPL_NUISANCE_BOUND(tf, B, n, R); }

int trpl_nuisance_reduce_dev(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C, int32_t J, const double *offsets,
                             int32_t M, const double *logw, double tf, uint32_t flags, double *P, int32_t *best, double *best_mag,
                             void *stream)
{
    if (int rc = check_nuisance(sse, esum, wsum, S, C, J, offsets, M, logw, false, tf, flags, P)) return rc;
    if (S == 0) return TRPL_OK;
    const nuisance::Args g = pack(wsum, C, offsets, M);
#define TRPL_NUISANCE_LAUNCH(MM, GG)                                                                                               \
    hipLaunchKernelGGL((nuisance::reduce<MM, GG>), dim3(per_sample_blocks(S)), dim3(256), 0, (hipStream_t)stream, sse, esum, S, (int)C, \
                       (int)J, (int)M, logw, tf, P, best, best_mag, g)
    TRPL_NUISANCE_DISPATCH(TRPL_NUISANCE_LAUNCH);
#undef TRPL_NUISANCE_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "nuisance_reduce launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

// plain host code, like trpl_mag_profile: the body the kernel runs
int trpl_nuisance_reduce(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C, int32_t J, const double *offsets,
                         int32_t M, const double *logw, double tf, uint32_t flags, double *P, int32_t *best, double *best_mag)
{
    if (int rc = check_nuisance(sse, esum, wsum, S, C, J, offsets, M, logw, true, tf, flags, P)) return rc;
    if (S == 0) return TRPL_OK;
    const nuisance::Args g = pack(wsum, C, offsets, M);
#define TRPL_NUISANCE_HOST(MM, GG) nuisance::reduce_host<MM, GG>(sse, esum, g, S, (int)C, (int)J, (int)M, logw, tf, P, best, best_mag)
    TRPL_NUISANCE_DISPATCH(TRPL_NUISANCE_HOST);
#undef TRPL_NUISANCE_HOST
    return TRPL_OK;
}

}  // extern "C"
