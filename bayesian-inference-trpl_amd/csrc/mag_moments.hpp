// The likelihood at a magnitude offset from the two moments of a curve -- the mag_grid loop of the reference's older likelihood
// (probs.lnP, probs.py:5-18) from what the TRPL_FLAG_MOMENTS steppers and trpl_loglik_irf_bank* emit: sum_i (e_i + d)^2 = sse +
// 2 d esum + n d^2.  ONE definition of each expression, compiled for the host and for the device in the translation units that
// include it (likelihood.hip: trpl_mag_grid*, trpl_mag_profile*; nuisance.hip: trpl_nuisance_reduce*), all of them with
// -ffp-contract=off: no fused multiply-add on either side, IEEE divide, so that the plain host forms and the kernels agree bit
// for bit, and so do the calls of the two units.
//
// A sample's moments of curve c are sse[c * stride], esum[c * stride] from the pointers handed in: stride S from sse + s for the
// [C][S] arrays of trpl_mag_*, stride J S from sse + j S + s for the [C][J][S] arrays of trpl_nuisance_reduce*.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace trpl {

// the squared error of a curve at offset d, +inf for a flagged system or NaN / inf moments
__host__ __device__ inline double mag_term(double sse, double esum, double n, double d)
{
    const double t1 = (2.0 * d) * esum;
    const double t2 = n * (d * d);
    const double v = (sse + t1) + t2;
    if (!(sse < INFINITY) || !(esum - esum == 0.0) || !(v == v)) return INFINITY;
    return v < 0.0 ? 0.0 : v;
}

// sum_c mag_term(.., d), curves in order from +0.0
__host__ __device__ inline double mag_curve_sum(const double *sse, const double *esum, const double *n, int64_t stride, int C, double d)
{
    double acc = 0.0;
    for (int c = 0; c < C; c++) acc += mag_term(sse[c * stride], esum[c * stride], n[c], d);
    return acc;
}

// The likelihood-maximising offset the curves of a sample share: d = -sum_c esum / sum_c n.  best is d, or NaN where a curve is
// flagged or the moments are not finite.  empty: every weight is zero and no curve is flagged -- nothing to fit, d means nothing;
// what the cell is then is the caller's.
struct MagShared {
    double d, best;
    bool empty;
};
__host__ __device__ inline MagShared mag_shared_offset(const double *sse, const double *esum, const double *n, int64_t stride, int C)
{
    double E = 0.0, N = 0.0;
    bool ok = true;
    for (int c = 0; c < C; c++) { E += esum[c * stride]; N += n[c]; ok = ok && sse[c * stride] < INFINITY; }
    const double d = (0.0 - E) / N;
    return {d, (ok && E - E == 0.0) ? d : (double)NAN, N == 0.0 && ok};
}

}  // namespace trpl
