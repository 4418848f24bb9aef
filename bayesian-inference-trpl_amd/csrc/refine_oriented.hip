// Oriented refinement proposals (trpl_refine_affine*, trpl_refine_draw_oriented*, include/trpl.h): the boxes of a generation are
// axis-parallel in whitened coordinates z = M (u - c), M the inverse of the lower Cholesky factor L of the population's shrunk
// weighted covariance, so they follow a ridge of the posterior that lies across the axes of the unit cube.
//
//   affine_kernel<A>         Z[s] = M (U[s] - c), one thread per sample with its row in registers.  M (the lower triangle, packed by
//       rows) and c are kernel arguments: every index is a compile-time constant after unrolling, so they are read as scalars, the
//       same in every lane.  z_i = sum_{j <= i} M_ij * (u_j - c_j), j ascending from +0.0: subtract, multiply, add.  Memory-bound:
//       16 A bytes per sample.
//   draw_oriented_kernel<A>  one thread per child.  The uniforms are draw_kernel's (Philox4x32-10, counter (child, call, generation),
//       genrand_res53: refine_common.hpp).  A box child of parent k: z_d = zc_kd + h_d * (2 xi_d - 1), u_i = c_i + sum_{j <= i}
//       L_ij * z_j (j ascending from +0.0), inside = every u_i in [0, 1]; a uniform child: u_d = xi_d, no z (NaN), inside.  X by the
//       sampler's expressions from u, inside or not: a child outside the cube keeps a finite X slightly beyond the prior box; the
//       caller does not solve it.
// The density of the oriented boxes is trpl_refine_density (refine.hip) on the Z of affine_kernel, unchanged.
// Compiled with -ffp-contract=off like refine.hip: every result is its expression with one rounding per operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "api_util.hpp"
#include "refine_common.hpp"

namespace trpl {
namespace refine_oriented {                                      // the kernels of this unit; the box, Philox and X are trpl::refine's

using namespace refine;

constexpr int kTri = 16 * 17 / 2;

// a lower-triangular matrix packed by rows, t[i (i + 1) / 2 + j] = T_ij for j <= i, and a vector: at most 152 doubles of kernel arguments
struct Affine {
    double t[kTri];
    double c[16];
};
struct HalfWidths {
    double h[16];
};

__host__ __device__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

template <int A>
__global__ void __launch_bounds__(kThreads) affine_kernel(const double *U, int64_t S, int64_t ldu, const Affine mc, double *Z, int64_t ldz)
{
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    double d[A];
#pragma unroll
    for (int j = 0; j < A; j++) d[j] = U[s * ldu + j] - mc.c[j];
#pragma unroll
    for (int i = 0; i < A; i++) {
        double z = 0.0;
#pragma unroll
        for (int j = 0; j <= i; j++) z = z + mc.t[tri(i, j)] * d[j];
        Z[s * ldz + i] = z;
    }
}

template <int A>
__global__ void __launch_bounds__(kThreads) draw_oriented_kernel(const double *zc, int64_t K, int64_t n_uniform, int64_t total,
                                                                 uint32_t seed_lo, uint32_t seed_hi, uint32_t generation, const Affine lc,
                                                                 const HalfWidths hw, const Box bx, double *Z2, double *U2, double *X2,
                                                                 int32_t *inside)
{
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (n >= total) return;
    const bool uni = n < n_uniform;
    const int64_t par = uni ? 0 : (n - n_uniform) % K;
    const double *pz = zc + par * A;
    double xi[A];
#pragma unroll
    for (int j = 0; 2 * j < A; j++) {
        uint32_t r[4];
        philox4x32_10((uint32_t)n, (uint32_t)((uint64_t)n >> 32), (uint32_t)j, generation, seed_lo, seed_hi, r);
        xi[2 * j] = res53(r[0], r[1]);
        if (2 * j + 1 < A) xi[2 * j + 1] = res53(r[2], r[3]);
    }
    double z[A], u[A];
    bool in = true;
#pragma unroll
    for (int d = 0; d < A; d++) z[d] = uni ? (double)NAN : pz[d] + hw.h[d] * (2.0 * xi[d] - 1.0);
#pragma unroll
    for (int i = 0; i < A; i++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j <= i; j++) s = s + lc.t[tri(i, j)] * z[j];
        u[i] = uni ? xi[i] : lc.c[i] + s;
        in = in && u[i] >= 0.0 && u[i] <= 1.0;                   // a NaN is outside
    }
    double *row = X2 + n * bx.ncol;
    put_fixed(bx, row);
#pragma unroll
    for (int d = 0; d < A; d++) {
        Z2[n * A + d] = z[d];
        U2[n * A + d] = u[d];
        const int c = bx.act[d];
        row[c] = column_value(bx, c, u[d]);
    }
    put_overrides(bx, row);
    inside[n] = in ? 1 : 0;
}

}  // namespace refine_oriented
}  // namespace trpl

using namespace trpl;

// a host lower-triangular [A][A] row-major matrix and a host vector -> the kernels' packed arguments; only j <= i is read.
// Refuses a non-finite entry and a diagonal that is not positive.
static int pack_affine(const char *mname, const double *T, const double *c, int32_t A, refine_oriented::Affine &out)
{
    out = refine_oriented::Affine();
    for (int i = 0; i < A; i++) {
        if (!isfinite(c[i])) return api_fail(TRPL_ERR_ARG, "c[%d] is not finite", i);
        out.c[i] = c[i];
        for (int j = 0; j <= i; j++) {
            const double v = T[i * A + j];
            if (!isfinite(v)) return api_fail(TRPL_ERR_ARG, "%s[%d][%d] is not finite", mname, i, j);
            out.t[refine_oriented::tri(i, j)] = v;
        }
        if (!(T[i * A + i] > 0.0)) return api_fail(TRPL_ERR_ARG, "%s[%d][%d]=%g: the diagonal must be positive", mname, i, i, T[i * A + i]);
    }
    return TRPL_OK;
}

static int check_affine(const void *U, int64_t S, int64_t ldu, int32_t A, const void *M, const void *c, const void *Z, int64_t ldz)
{
    if (S < 1) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 1", (long long)S);
    if (A < 1 || A > TRPL_REFINE_MAX_DIMS) return api_fail(TRPL_ERR_ARG, "A=%d must be in [1, %d]", A, TRPL_REFINE_MAX_DIMS);
    if (ldu < A) return api_fail(TRPL_ERR_ARG, "ldu=%lld must be >= A=%d", (long long)ldu, A);
    if (ldz < A) return api_fail(TRPL_ERR_ARG, "ldz=%lld must be >= A=%d", (long long)ldz, A);
    if (int rc = refine_check_blocks("S", S, "samples")) return rc;
    if (!U) return api_fail(TRPL_ERR_ARG, "U is NULL");
    if (!M) return api_fail(TRPL_ERR_ARG, "M is NULL");
    if (!c) return api_fail(TRPL_ERR_ARG, "c is NULL");
    if (!Z) return api_fail(TRPL_ERR_ARG, "Z is NULL");
    return TRPL_OK;
}

static int check_draw_oriented(const void *zc, const double *h, const void *L, const void *c, int64_t K, int32_t A, int64_t m,
                               int64_t n_uniform, const void *Z2, const void *U2, const void *X2, const void *inside,
                               refine_oriented::HalfWidths &hw)
{
    if (int rc = refine_check_counts(K, A)) return rc;
    if (int rc = refine_check_children(K, m, n_uniform)) return rc;
    if (!zc) return api_fail(TRPL_ERR_ARG, "zc is NULL");
    if (!h) return api_fail(TRPL_ERR_ARG, "h is NULL");
    if (!L) return api_fail(TRPL_ERR_ARG, "L is NULL");
    if (!c) return api_fail(TRPL_ERR_ARG, "c is NULL");
    if (!Z2) return api_fail(TRPL_ERR_ARG, "Z2 is NULL");
    if (!U2) return api_fail(TRPL_ERR_ARG, "U2 is NULL");
    if (!X2) return api_fail(TRPL_ERR_ARG, "X2 is NULL");
    if (!inside) return api_fail(TRPL_ERR_ARG, "inside is NULL");
    hw = refine_oriented::HalfWidths();
    for (int d = 0; d < A; d++) {
        if (!(isfinite(h[d]) && h[d] > 0.0)) return api_fail(TRPL_ERR_ARG, "h[%d]=%g must be finite and > 0", d, h[d]);
        hw.h[d] = h[d];
    }
    return TRPL_OK;
}

extern "C" {

int trpl_refine_affine_dev(const double *U, int64_t S, int64_t ldu, int32_t A, const double *M, const double *c, double *Z, int64_t ldz,
                           void *stream)
{
    if (int rc = check_affine(U, S, ldu, A, M, c, Z, ldz)) return rc;
    refine_oriented::Affine mc;
    if (int rc = pack_affine("M", M, c, A, mc)) return rc;
    const dim3 grid(refine_blocks(S)), block(refine::kThreads);
    switch (A) {
#define TRPL_CASE(n) case n: hipLaunchKernelGGL(refine_oriented::affine_kernel<n>, grid, block, 0, (hipStream_t)stream, U, S, ldu, mc, Z, ldz); break;
        TRPL_REFINE_DIMS(TRPL_CASE)
#undef TRPL_CASE
    }
    return refine_launched("refine affine");
}

int trpl_refine_affine(const double *U, int64_t S, int64_t ldu, int32_t A, const double *M, const double *c, double *Z, int64_t ldz,
                       int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_affine(U, S, ldu, A, M, c, Z, ldz)) return rc;
    refine_oriented::Affine mc;
    if (int rc = pack_affine("M", M, c, A, mc)) return rc;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const double *dU = sg.in(U, (size_t)ldu, (size_t)A, (size_t)S);                      // both compact on the device: the rows' padding
    double *dZ = sg.out(Z, (size_t)ldz, (size_t)A, (size_t)S);                           // stays on the host
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_refine_affine_dev(dU, S, A, A, M, c, dZ, A, sg.stream())) return rc;
    return sg.finish(seconds);
}

int trpl_refine_draw_oriented_dev(const double *zc, const double *h, const double *L, const double *c, int64_t K, int32_t A, int64_t m,
                                  int64_t n_uniform, uint64_t seed, uint32_t generation, int32_t ncol, const double *lo, const double *hi,
                                  const int32_t *do_log, uint32_t flags, double *Z2, double *U2, double *X2, int32_t *inside, void *stream)
{
    refine_oriented::HalfWidths hw;
    if (int rc = check_draw_oriented(zc, h, L, c, K, A, m, n_uniform, Z2, U2, X2, inside, hw)) return rc;
    refine::Box bx;
    if (int rc = refine_make_box(ncol, lo, hi, do_log, flags, A, bx)) return rc;
    refine_oriented::Affine lc;
    if (int rc = pack_affine("L", L, c, A, lc)) return rc;
    const int64_t total = n_uniform + K * m;
    if (total == 0) return TRPL_OK;
    const dim3 grid(refine_blocks(total)), block(refine::kThreads);
    switch (A) {
#define TRPL_CASE(n)                                                                                                                   \
    case n:                                                                                                                            \
        hipLaunchKernelGGL(refine_oriented::draw_oriented_kernel<n>, grid, block, 0, (hipStream_t)stream, zc, K, n_uniform, total,         \
                           (uint32_t)seed, (uint32_t)(seed >> 32), generation, lc, hw, bx, Z2, U2, X2, inside);                        \
        break;
        TRPL_REFINE_DIMS(TRPL_CASE)
#undef TRPL_CASE
    }
    return refine_launched("refine oriented draw");
}

int trpl_refine_draw_oriented(const double *zc, const double *h, const double *L, const double *c, int64_t K, int32_t A, int64_t m,
                              int64_t n_uniform, uint64_t seed, uint32_t generation, int32_t ncol, const double *lo, const double *hi,
                              const int32_t *do_log, uint32_t flags, double *Z2, double *U2, double *X2, int32_t *inside, int32_t device,
                              double *seconds)
{
    if (seconds) *seconds = 0.0;
    refine_oriented::HalfWidths hw;
    if (int rc = check_draw_oriented(zc, h, L, c, K, A, m, n_uniform, Z2, U2, X2, inside, hw)) return rc;
    refine::Box bx;
    if (int rc = refine_make_box(ncol, lo, hi, do_log, flags, A, bx)) return rc;
    refine_oriented::Affine lc;
    if (int rc = pack_affine("L", L, c, A, lc)) return rc;
    const int64_t total = n_uniform + K * m;
    if (total == 0) return TRPL_OK;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const double *dC = sg.in(zc, (size_t)K * A);
    double *dZ = sg.out(Z2, (size_t)total * A), *dU = sg.out(U2, (size_t)total * A), *dX = sg.out(X2, (size_t)total * ncol);
    int32_t *dIn = sg.out(inside, (size_t)total);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_refine_draw_oriented_dev(dC, h, L, c, K, A, m, n_uniform, seed, generation, ncol, lo, hi, do_log, flags, dZ, dU, dX, dIn,
                                               sg.stream()))
        return rc;
    return sg.finish(seconds);
}

}  // extern "C"
