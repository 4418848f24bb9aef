// extern "C" entry points of libtrpl_hip.so (declared in include/trpl.h).  Host-side glue only:
// argument checks, the per-curve constants of pvSim (pvSimPCR.py:314-331), staging for the
// host-buffer calls, launches.  Nothing here throws across the ABI.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "api_util.hpp"
#include "crosslane.hpp"      // TRPL_PAIR_OPTIMISTIC (classify_stepper)

namespace trpl {

namespace { thread_local char g_err[512] = ""; }

int api_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

const RoctxApi &roctx()
{
    static const RoctxApi api = [] {
        RoctxApi a;
        void *push = dlsym(RTLD_DEFAULT, "roctxRangePushA"), *pop = dlsym(RTLD_DEFAULT, "roctxRangePop");
        if (!push || !pop) {
            void *dl = nullptr;
            for (const char *n : {"libroctx64.so.4", "libroctx64.so"})
                if ((dl = dlopen(n, RTLD_NOW | RTLD_LOCAL)) != nullptr) break;
            push = dl ? dlsym(dl, "roctxRangePushA") : nullptr;
            pop = dl ? dlsym(dl, "roctxRangePop") : nullptr;
        }
        if (push && pop) {
            a.push = (int (*)(const char *))push;
            a.pop = (int (*)())pop;
        }
        return a;
    }();
    return api;
}

int check_grid(int32_t L, int64_t T, int32_t plT, int32_t max_iter, double time_ns)
{
    if (!pow2(L) || L < 4 || L > 512) return api_fail(TRPL_ERR_ARG, "L=%d must be a power of two in [4, 512]", L);
    if (T < 1) return api_fail(TRPL_ERR_ARG, "T=%lld must be >= 1", (long long)T);
    // the steppers keep steps and PL columns in 32-bit scalars: with T <= 2^30 - 16 and plT clamped to T + 1 (kernel_plT)
    // none of t + plT, pl_col * plT or (t0 + plT - 1) / plT can leave the int32 range
    if (T > 0x3ffffff0LL) return api_fail(TRPL_ERR_ARG, "T=%lld is too large (at most 2^30 - 16 steps)", (long long)T);
    if (plT < 1) return api_fail(TRPL_ERR_ARG, "plT=%d must be >= 1", plT);
    if (max_iter < 1) return api_fail(TRPL_ERR_ARG, "max_iter=%d must be >= 1", max_iter);
    if (!(time_ns > 0)) return api_fail(TRPL_ERR_ARG, "time_ns must be > 0");
    return TRPL_OK;
}

int check_batch(const LoglikCall &k)
{
    if (int rc = check_grid(k.L, k.T, k.plT, k.max_iter, k.time_ns)) return rc;
    if (k.S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (k.C < 1 || k.C > TRPL_MAX_CURVES) return api_fail(TRPL_ERR_ARG, "C=%d must be in [1, %d]", k.C, TRPL_MAX_CURVES);
    return TRPL_OK;
}

int check_interp(const void *obs_hi, const void *obs_dx, const void *obs_h, int32_t plT)
{
    const bool interp = obs_hi || obs_dx || obs_h;
    if (interp && !(obs_hi && obs_dx && obs_h)) return api_fail(TRPL_ERR_ARG, "obs_hi, obs_dx and obs_h go together");
    if (interp && plT != 1) return api_fail(TRPL_ERR_ARG, "off-grid observations need plT = 1");
    return TRPL_OK;
}

// plT as the kernels see it: a stride beyond the window stores column 0 only, whatever its size
static inline int32_t kernel_plT(int32_t plT, int64_t T) { return (int64_t)plT > T + 1 ? (int32_t)(T + 1) : plT; }

int check_brackets(const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int32_t C, int64_t obs_ld,
                   const int64_t *n_obs, int64_t T)
{
    for (int c = 0; c < C; c++)
        for (int64_t i = 0; i < n_obs[c] && i < obs_ld; i++) {
            const int64_t at = (int64_t)c * obs_ld + i;
            const int32_t h = obs_hi[at];
            if (h < 1 || h > T || (i && h < obs_hi[at - 1]))
                return api_fail(TRPL_ERR_ARG, "obs_hi[%d][%lld]=%d must be sorted and in [1, T]", c, (long long)i, h);
            if (!(obs_h[at] > 0) || !(obs_dx[at] >= 0) || !(obs_dx[at] <= obs_h[at]))
                return api_fail(TRPL_ERR_ARG, "observation %lld of curve %d: need 0 <= obs_dx <= obs_h and obs_h > 0",
                                (long long)i, c);
        }
    return TRPL_OK;
}

int64_t loglik_steps(bool interp, int32_t C, const int64_t *n_obs, int32_t plT, int64_t T)
{
    if (interp) return T;                            // the kernel stops at the last observation (PlSink::t_last)
    int64_t steps = 0;
    for (int c = 0; c < C; c++) steps = std::max<int64_t>(steps, (n_obs[c] - 1) * (int64_t)plT);
    return steps;
}

namespace {

// pvSim's non-dimensionalisation (pvSimPCR.py:314-331, :393).  Python's float `**` is C pow().
void curve_const(double length, double time_ns, int L, int64_t T, trpl::CurveConst &cc)
{
    const double dx = length / L, dt = time_ns / (double)T;
    const double dx3 = pow(dx, 3.0), dtdx = dt / dx, dtdx2 = dtdx / dx;
    const double dtdx6 = dt / pow(dx, 6.0);
    const double s[12] = {dx3, dx3, dtdx2, dtdx2, dtdx2 / dx, dtdx, dtdx, dtdx6, dtdx6, 1 / dt, 1 / dt, 1 / dx};
    memcpy(cc.scales, s, sizeof s);
    cc.dx3 = dx3;
    cc.plnorm = pow(dx, 2.0) * dt;
    cc.dx = dx;
    cc.n_obs = 0;
}

// FAST, L = 128 has two kernels: one system per wavefront (3 waves per SIMD: 12 systems per CU in
// flight) and two systems per wavefront (2 waves per SIMD: 16 systems per CU, +25..40 % throughput once
// the chip is kept full, but ~15 % slower per wave when it is not).  A launch's duration is set by its slowest
// chain of systems, so the paired kernel only pays when the chip stays full for most of the launch: more
// systems than the one-system kernel holds at once, and -- for short windows, where the first time steps'
// 20-900 inner iterations make the work per system very uneven -- at least two and a half such fills.
// Measured crossover (MI355X, Power_scan, round-2 kernels, tools/small_launch_probe.py; pair / single time):
//   steps = 8000:  1024 systems 1.15, 3072: 1.01, 4096: 0.91, 8192: 0.86, 12 288: 0.82
//   steps = 1000:  4096: 0.96, 6144: 0.99, 8192: 0.92, 12 288: 0.88
// TRPL_FLAG_KERNEL_PAIR / _SINGLE force the choice per call.
bool use_pair_kernel(int64_t nsys, int64_t steps)
{
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        static thread_local int cached_dev = -1, cached_cus = 256;
        if (cached_dev != dev) {
            int n = 0;
            if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cached_cus = n;
            cached_dev = dev;
        }
        cus = cached_cus;
    }
    const int64_t fill = (int64_t)cus * 12;
    return nsys > fill && (steps >= 4000 || 2 * nsys >= 5 * fill);
}

constexpr uint32_t kVariantBits = TRPL_FLAG_KERNEL_PAIR | TRPL_FLAG_KERNEL_SINGLE;

// Who shares a wavefront in the paired kernel.  Two curves of ONE sample have the same material parameters and need
// similar iteration counts step by step, which is what a pair pays for (max of the two per time step); adjacent
// samples of one curve do not.  Curves are grouped by identical grid (thickness) and observation count; inside a
// group consecutive curves -- neighbouring excitation powers in the reference's files -- are paired for each of the
// two samples of a period; the first curve of a group of odd size pairs with itself across the two samples.  Every
// (curve, sample) of the period appears exactly once.  A system's bits do not depend on its partner (tested), so the
// table is purely a scheduling matter; TRPL_FLAG_PAIR_ADJACENT switches it off for A/B measurements.
void build_pair_table(trpl::StepArgs &a)
{
    a.pair_n = 0;
    if ((a.flags & TRPL_FLAG_PAIR_ADJACENT) || a.C < 2 || a.obs_hi != nullptr || a.pl != nullptr) return;
    bool used[trpl::kMaxCurves] = {};
    int k = 0;
    for (int c0 = 0; c0 < a.C; c0++) {
        if (used[c0]) continue;
        int group[trpl::kMaxCurves], n = 0;
        for (int c = c0; c < a.C; c++)
            if (!used[c] && memcmp(a.curve[c].scales, a.curve[c0].scales, sizeof a.curve[c].scales) == 0 &&
                a.curve[c].plnorm == a.curve[c0].plnorm && a.curve[c].n_obs == a.curve[c0].n_obs) {
                group[n++] = c;
                used[c] = true;
            }
        for (int i = n & 1; i + 1 < n; i += 2)
            for (int off = 0; off < 2; off++) {
                a.pair_cA[k] = (uint8_t)group[i]; a.pair_oA[k] = (uint8_t)off;
                a.pair_cB[k] = (uint8_t)group[i + 1]; a.pair_oB[k] = (uint8_t)off;
                k++;
            }
        if (n & 1) {
            a.pair_cA[k] = a.pair_cB[k] = (uint8_t)group[0]; a.pair_oA[k] = 0; a.pair_oB[k] = 1;
            k++;
        }
    }
    a.pair_n = k;                                   // == a.C
}

// Which stepper instantiation a launch runs: the kernel family and the template arguments of its kernel.
struct StepperChoice {
    enum Family { Single, Pair, F32 } family;        // trpl::stepper_kernel / pair::stepper_pair_kernel / f32::stepper_kernel
    int32_t L, bundle;                               // bundle: m of TRPL_FLAG_BUNDLE(m)
    bool strict, snap, mixed, hist32;                // template arguments of the one-system kernel, with bundle > 1
    bool predict;                                    // TRPL_FLAG_PREDICT: the instantiation in namespace ...::predict
    trpl::Variant::Sink sink;                        // TRPL_FLAG_MOMENTS / _WEIGHTED / _CUT: the instantiation in namespace trpl::<sink>
    bool optimistic;                                 // paired kernel: the optimistic seam (not TRPL_FLAG_PAIR_ALWAYS_SEAM)
};

// The likelihood sinks a flag selects, indexed by Variant::Sink: all of them exist for the plain fp64 steppers (FAST, paired
// and, where `strict` says so, STRICT) in likelihood mode only.  A sink excludes the ones before it in this table.
const struct SinkInfo {
    uint32_t flag;
    const char *name, *ns;                           // ns: its level of the kernels' namespace
    bool strict;                                     // has STRICT units (the cut sink is batched: another granularity than STRICT's emit)
} kSinks[trpl::Variant::kSinks] = {
    {0, "", "", true},
    {TRPL_FLAG_MOMENTS, "TRPL_FLAG_MOMENTS", "moments::", true},
    {TRPL_FLAG_WEIGHTED, "TRPL_FLAG_WEIGHTED", "weighted::", true},      // emits both sums itself
    {TRPL_FLAG_CUT, "TRPL_FLAG_CUT", "cut::", false},                    // tests the plain sse
};

// THE function that maps a call to a kernel: launch(), trpl_kernel_name, trpl_kernel_variant and pin_variant read its answer.
// It does not validate (check_launch does); on what check_launch accepts at most one of FP32 / STRICT / MIXED / HIST32 is
// set, and the precedence below is what trpl_kernel_variant answers for the rest (STRICT | FP32 -> FP32, KERNEL_PAIR | STRICT
// -> STRICT).  HIST32 leaves the paired-or-single rung alone: launches accept it at L = 256 / 512 only, and pin_variant
// pins by launch size whatever it is.  snap: state snapshots or a resume (their own instantiation).
StepperChoice classify_stepper(uint32_t flags, int32_t L, int64_t nsys, int64_t steps, bool snap)
{
    StepperChoice c = {StepperChoice::Single, L, flags_bundle(flags)};
    c.snap = snap;
    c.predict = (flags & TRPL_FLAG_PREDICT) != 0;
    c.sink = trpl::Variant::plain;
    for (int k = 1; k < trpl::Variant::kSinks; k++)
        if (flags & kSinks[k].flag) c.sink = (trpl::Variant::Sink)k;        // check_launch accepts at most one
    c.optimistic = TRPL_PAIR_OPTIMISTIC != 0 && !(flags & TRPL_FLAG_PAIR_ALWAYS_SEAM);
    if (flags & TRPL_FLAG_FP32) c.family = StepperChoice::F32;
    else if (flags & TRPL_FLAG_STRICT) c.strict = true;
    else if (flags & TRPL_FLAG_MIXED) c.mixed = true;
    else {
        c.hist32 = (flags & TRPL_FLAG_HIST32) != 0;
        if (L == 128 && c.bundle == 1 &&                                             // a bundle is one system per wavefront
            ((flags & TRPL_FLAG_KERNEL_PAIR) || (!(flags & TRPL_FLAG_KERNEL_SINGLE) && use_pair_kernel(nsys, steps))))
            c.family = StepperChoice::Pair;
    }
    return c;
}

// The launcher of a choice, or nullptr where none is built: the table has exactly the lines of stepper_variants.hpp.
typedef hipError_t StepperLauncher(const trpl::StepArgs &, hipStream_t);
trpl::Variant::Unit unit_of(const StepperChoice &c)
{
    if (c.family == StepperChoice::F32) return trpl::Variant::f32;
    if (c.mixed) return trpl::Variant::mixed;
    if (c.hist32) return trpl::Variant::hist32;
    if (c.family == StepperChoice::Pair) return trpl::Variant::pair;
    return c.strict ? trpl::Variant::strict : trpl::Variant::fast;
}
StepperLauncher *find_launcher(const StepperChoice &c)
{
    static const struct Table {
        StepperLauncher *fn[trpl::Variant::kSinks][2][trpl::Variant::kUnits] = {};
        Table()
        {
#define TRPL_VARIANT(sink, predict, unit) \
    fn[trpl::Variant::sink][predict][trpl::Variant::unit] = trpl::launch_variant<trpl::Variant::sink, predict, trpl::Variant::unit>;
#include "stepper_variants.hpp"
#undef TRPL_VARIANT
        }
    } table;
    return table.fn[c.sink][c.predict][unit_of(c)];
}

int check_variant_flags(uint32_t flags, int32_t L)
{
    if ((flags & kVariantBits) == kVariantBits)
        return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_KERNEL_PAIR and TRPL_FLAG_KERNEL_SINGLE exclude each other");
    if ((flags & TRPL_FLAG_KERNEL_PAIR) && (L != 128 || (flags & (TRPL_FLAG_STRICT | TRPL_FLAG_FP32 | TRPL_FLAG_MIXED))))
        return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_KERNEL_PAIR needs L = 128 (got %d) without TRPL_FLAG_STRICT / _FP32 / _MIXED", L);
    return TRPL_OK;
}

uint32_t pin_variant(uint32_t flags, int64_t nsys, int32_t L, int64_t steps)
{
    if (flags & kVariantBits) return flags;
    return flags | (classify_stepper(flags, L, nsys, steps, false).family == StepperChoice::Pair ? TRPL_FLAG_KERNEL_PAIR : TRPL_FLAG_KERNEL_SINGLE);
}

// What sink k refuses by the flags alone: the sinks before it (kSinks) and the steppers it is not built for.
int check_sink_flags(int k, uint32_t flags)
{
    const SinkInfo &s = kSinks[k];
    if (!(flags & s.flag)) return TRPL_OK;
    for (int j = 1; j < k; j++)
        if (flags & kSinks[j].flag)
            return api_fail(TRPL_ERR_ARG, "%s does not combine with %s (one sink per launch)", s.name, kSinks[j].name);
    if (!s.strict && (flags & TRPL_FLAG_STRICT)) return api_fail(TRPL_ERR_UNSUPPORTED, "%s is not built for TRPL_FLAG_STRICT", s.name);
    if (flags & (TRPL_FLAG_FP32 | TRPL_FLAG_MIXED | TRPL_FLAG_HIST32))
        return api_fail(TRPL_ERR_UNSUPPORTED, "%s is not built for TRPL_FLAG_FP32, TRPL_FLAG_MIXED or TRPL_FLAG_HIST32", s.name);
    if (flags_bundle(flags) > 1) return api_fail(TRPL_ERR_UNSUPPORTED, "%s is not built for TRPL_FLAG_BUNDLE(m > 1)", s.name);
    return TRPL_OK;
}

// TRPL_FLAG_CUT: what the cut sink does not combine with.  Flags only, so that trpl_loglik_cut[_dev] can answer before they touch a device.
int check_cut_flags(uint32_t flags) { return check_sink_flags(trpl::Variant::cut, flags); }

// Everything a stepper launch refuses because of its flags and shape: launch() and trpl_kernel_name run the same checks
// before they classify, so a kernel name is only ever returned for an instantiation that exists and that the launch would run.
// snap: state snapshots requested; resume: the launch continues from a checkpoint.
int check_launch(uint32_t flags, int32_t L, int64_t steps, bool snap, bool resume)
{
    if (!pow2(L) || L < 4 || L > 512) return api_fail(TRPL_ERR_ARG, "L=%d must be a power of two in [4, 512]", L);
    if (int rc = check_variant_flags(flags, L)) return rc;
    if (flags_bdf_order(flags) > 5u) return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_BDF_ORDER(%u): the order cap must be 1 .. 5 (0: the reference's ramp)", flags_bdf_order(flags));
    const int32_t bundle = flags_bundle(flags);
    for (int k = 1; k < trpl::Variant::kSinks; k++) {                       // the sinks, in the table's order
        if (int rc = check_sink_flags(k, flags)) return rc;
        if ((flags & kSinks[k].flag) && (snap || resume))
            return api_fail(TRPL_ERR_UNSUPPORTED, "%s has no snapshot / resume instantiations (likelihood mode only)", kSinks[k].name);
    }
    if (flags & TRPL_FLAG_PREDICT) {                                        // the extrapolated start: plain fp64 steppers only
        if (flags & (TRPL_FLAG_FP32 | TRPL_FLAG_MIXED | TRPL_FLAG_HIST32))
            return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_PREDICT excludes TRPL_FLAG_FP32, TRPL_FLAG_MIXED and TRPL_FLAG_HIST32");
        if (bundle > 1) return api_fail(TRPL_ERR_UNSUPPORTED, "TRPL_FLAG_PREDICT is not built for TRPL_FLAG_BUNDLE(m > 1)");
    }
#ifndef TRPL_EXPERIMENTAL
    if (flags & (TRPL_FLAG_MIXED | TRPL_FLAG_HIST32))
        return api_fail(TRPL_ERR_UNSUPPORTED, "%s: this library was built without the experimental steppers (measured and rejected, "
                        "DESIGN.md section 7); rebuild with `make EXPERIMENTAL=1` to run them",
                        (flags & TRPL_FLAG_MIXED) ? "TRPL_FLAG_MIXED" : "TRPL_FLAG_HIST32");
#endif
    if (flags & TRPL_FLAG_HIST32) {
        if (flags & (TRPL_FLAG_STRICT | TRPL_FLAG_FP32 | TRPL_FLAG_MIXED | TRPL_FLAG_KERNEL_PAIR))
            return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_HIST32 excludes TRPL_FLAG_STRICT, TRPL_FLAG_FP32, TRPL_FLAG_MIXED and TRPL_FLAG_KERNEL_PAIR");
        if (L != 256 && L != 512) return api_fail(TRPL_ERR_UNSUPPORTED, "TRPL_FLAG_HIST32: the fp32-difference history is built for L = 256 and 512 (got %d)", L);
        if (snap || resume || bundle > 1)
            return api_fail(TRPL_ERR_UNSUPPORTED, "snapshots, resume and bundles are not available with TRPL_FLAG_HIST32");
    }
    if (bundle > 1 && (flags & (TRPL_FLAG_FP32 | TRPL_FLAG_MIXED | TRPL_FLAG_KERNEL_PAIR)))
        return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_BUNDLE goes with TRPL_FLAG_STRICT or the plain fp64 one-system stepper only");
    if (bundle > 1 && !(flags & TRPL_FLAG_STRICT) && L > 128)
        return api_fail(TRPL_ERR_UNSUPPORTED, "TRPL_FLAG_BUNDLE without TRPL_FLAG_STRICT is built for L <= 128 (got %d)", L);
    if (bundle > trpl::bundle_cap(L))
        return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_BUNDLE(%d): at most %d systems per bundle at L = %d", bundle, trpl::bundle_cap(L), L);
    if (flags & TRPL_FLAG_FP32) {
        if (flags & (TRPL_FLAG_STRICT | TRPL_FLAG_MIXED)) return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_FP32 excludes TRPL_FLAG_STRICT and TRPL_FLAG_MIXED");
        if (L < 128) return api_fail(TRPL_ERR_UNSUPPORTED, "the fp32 stepper is built for L >= 128 (got %d)", L);
        if (snap) return api_fail(TRPL_ERR_UNSUPPORTED, "state snapshots are not available with TRPL_FLAG_FP32");
        if (steps > TRPL_FP32_MAX_STEPS && !(flags & TRPL_FLAG_FP32_LONG))
            return api_fail(TRPL_ERR_UNSUPPORTED, "TRPL_FLAG_FP32 over %lld time steps: an fp32 state loses the decay beyond ~%d steps "
                            "(PL errors of percents, then tens of percents: include/trpl.h); use the fp64 path, or add "
                            "TRPL_FLAG_FP32_LONG (Python wrappers: fp32=\"long\") for a screening pass", (long long)steps, TRPL_FP32_MAX_STEPS);
    }
    if (flags & TRPL_FLAG_MIXED) {
        if (flags & TRPL_FLAG_STRICT) return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_MIXED and TRPL_FLAG_STRICT exclude each other");
        if (L < 128) return api_fail(TRPL_ERR_UNSUPPORTED, "the mixed-precision stepper is built for L >= 128 (got %d)", L);
    }
    return TRPL_OK;
}

}  // namespace

int pin_sharded_batch(uint32_t &flags, int64_t S, int32_t C, int32_t L, int64_t T, int32_t plT, bool interp, const int64_t *n_obs, int64_t obs_ld)
{
    if (int rc = check_variant_flags(flags, L)) return rc;
    if (flags_bundle(flags) > 1) return api_fail(TRPL_ERR_UNSUPPORTED, "TRPL_FLAG_BUNDLE couples neighbouring samples: a sharded batch would depend on where it is cut");
    for (int c = 0; c < C; c++)
        if (n_obs[c] < 1 || n_obs[c] > obs_ld)
            return api_fail(TRPL_ERR_ARG, "n_obs[%d]=%lld out of range (obs_ld %lld)", c, (long long)n_obs[c], (long long)obs_ld);
    flags = pin_variant(flags, S * (int64_t)C, L, loglik_steps(interp, C, n_obs, plT, T));
    return TRPL_OK;
}

// TRPL_FLAG_MOMENTS belongs to trpl_loglik_moments[_dev], which set it themselves: the other entry points have no esum output
// ... and TRPL_FLAG_WEIGHTED to trpl_loglik_weighted[_dev]: the other entry points take no weights
// ... and TRPL_FLAG_CUT to trpl_loglik_cut[_levels][_dev]: the other entry points have no sse_cut and no cut_level
static int no_cut_flag(uint32_t flags)
{
    if (flags & TRPL_FLAG_CUT)
        return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_CUT is set by trpl_loglik_cut[_dev] only: this entry point has no sse_cut");
    return TRPL_OK;
}

int no_weighted_flag(uint32_t flags)
{
    if (int rc = no_cut_flag(flags)) return rc;      // every entry point without an sse_cut passes here
    if (flags & TRPL_FLAG_WEIGHTED)
        return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_WEIGHTED is set by trpl_loglik_weighted[_dev] only: this entry point takes no weights");
    return TRPL_OK;
}

int no_moments_flag(uint32_t flags)
{
    if (int rc = no_weighted_flag(flags)) return rc;
    if (flags & TRPL_FLAG_MOMENTS)
        return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_MOMENTS is set by trpl_loglik_moments[_dev] only: this entry point has no esum output");
    return TRPL_OK;
}

int select_device(int32_t device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return api_fail(TRPL_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return api_fail(TRPL_ERR_ARG, "device %d out of range (%d visible)", device, n);
    HIP_TRY(hipSetDevice(device));
    return TRPL_OK;
}

std::atomic<int64_t> g_pair_launch_info[3];

}  // namespace trpl

using namespace trpl;

namespace {

#if TRPL_SLOT_TIMELINE
// measurement build only: where the paired kernel's waves record their blocks, and whether its launch stays one block per wave
uint64_t *g_slot_timeline = nullptr;
int32_t g_slot_timeline_classic = 0;
#endif

// steps: how many time steps the launch will take (T, or up to the last observation in likelihood mode)
int launch(const trpl::StepArgs &a_in, uint32_t flags, hipStream_t st, int64_t steps)
{
    if (int rc = check_launch(flags, a_in.L, steps, a_in.n_snap > 0, a_in.resN != nullptr)) return rc;
    const StepperChoice c = classify_stepper(flags, a_in.L, a_in.S * a_in.C, steps, a_in.n_snap > 0 || a_in.resN != nullptr);
    trpl::StepArgs a = a_in;
    a.bundle = c.bundle;
    if (c.family == StepperChoice::Pair) build_pair_table(a);
#if TRPL_SLOT_TIMELINE
    a.timeline = g_slot_timeline; a.timeline_classic = g_slot_timeline_classic;
#endif
    static const char *const kWord[trpl::Variant::kUnits] = {"", "", "pair ", "fp32 ", "mixed ", "hist32 "};   // what the error message starts with
    StepperLauncher *const fn = find_launcher(c);
    if (!fn) return api_fail(TRPL_ERR_UNSUPPORTED, "no stepper is built for this combination of flags (flags 0x%x, L = %d)", flags, a.L);
    const hipError_t e = fn(a, st);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "%sstepper launch: %s", kWord[unit_of(c)], hipGetErrorString(e));
    return TRPL_OK;
}

}  // namespace

extern "C" {

int trpl_abi_version(void) { return TRPL_ABI_VERSION; }
int trpl_has_experimental(void)
{
#ifdef TRPL_EXPERIMENTAL
    return 1;
#else
    return 0;
#endif
}
const char *trpl_last_error(void) { return g_err; }

// Tests and tools (not in include/trpl.h): out[0] paired-stepper launches of this process with persistent waves on a ticket, out[1]
// those of one block per wave, out[2] the resident waves R the last persistent-capable launch compared its blocks with
void trpl_pair_launch_info(int64_t *out)
{
    for (int i = 0; i < 3; i++) out[i] = trpl::g_pair_launch_info[i].load(std::memory_order_relaxed);
}

#if TRPL_SLOT_TIMELINE
// measurement build only (tools/slot_timeline.py; not in include/trpl.h): every later paired-stepper launch records into
// buf, a device buffer of 4 x 8 bytes per block of the launch (NULL: none); classic != 0 keeps one block per wave
void trpl_debug_slot_timeline(void *buf, int32_t classic) { g_slot_timeline = (uint64_t *)buf; g_slot_timeline_classic = classic; }
#endif

int trpl_kernel_variant(int64_t nsys, int32_t L, int64_t steps, uint32_t flags)
{
    const StepperChoice c = classify_stepper(flags, L, nsys, steps, false);
    if (c.family == StepperChoice::F32) return TRPL_KERNEL_FP32;
    if (c.strict) return TRPL_KERNEL_STRICT;
    if (c.mixed) return TRPL_KERNEL_MIXED;
    if (c.hist32) return TRPL_KERNEL_HIST32;
    return c.family == StepperChoice::Pair ? TRPL_KERNEL_FAST_PAIR : TRPL_KERNEL_FAST;
}

int trpl_kernel_name(int64_t nsys, int32_t L, int64_t steps, uint32_t flags, int32_t snapshots, char *buf, int64_t buflen)
{
    if (!buf || buflen < 1) return api_fail(TRPL_ERR_ARG, "buf must hold at least one byte");
    buf[0] = 0;
    // the checks of a launch: no name for a combination launch() refuses or for an instantiation that does not exist
    // (`snapshots` covers snapshots AND resume; the fp32 stepper has one instantiation and accepts a resume)
    if (int rc = check_launch(flags, L, steps, snapshots != 0 && !(flags & TRPL_FLAG_FP32), false)) return rc;
    const StepperChoice c = classify_stepper(flags, L, nsys, steps, snapshots != 0);
    if (!find_launcher(c)) return api_fail(TRPL_ERR_UNSUPPORTED, "no stepper is built for this combination of flags (flags 0x%x, L = %d)", flags, L);
    const char *tf[2] = {"false", "true"};
    char ns[64];                                     // trpl::[<sink>::][predict::] (stepper_impl.hpp: TRPL_VARIANT_NS_BEGIN)
    snprintf(ns, sizeof ns, "trpl::%s%s", kSinks[c.sink].ns, c.predict ? "predict::" : "");
    int n;
    if (c.family == StepperChoice::F32)
        n = snprintf(buf, (size_t)buflen, "%sf32::stepper_kernel<%d>", ns, c.L);
    else if (c.family == StepperChoice::Pair)
        n = snprintf(buf, (size_t)buflen, "%spair::stepper_pair_kernel<true, %s, %s>", ns, tf[c.snap], tf[c.optimistic]);
    else
        n = snprintf(buf, (size_t)buflen, "%sstepper_kernel<%d, %s, %s, %s, %s, %s>", ns, c.L, tf[c.strict], tf[c.snap],
                     tf[c.mixed], tf[c.bundle > 1], tf[c.hist32]);
    if (n < 0 || n >= buflen) return api_fail(TRPL_ERR_ARG, "buflen=%lld is too small for the kernel name", (long long)buflen);
    return TRPL_OK;
}

int trpl_pair_table(const double *lengths_nm, const int64_t *n_obs, int32_t C, int32_t L, int64_t T, double time_ns,
                    int32_t *cA, int32_t *oA, int32_t *cB, int32_t *oB)
{
    if (C < 1 || C > trpl::kMaxCurves) return -api_fail(TRPL_ERR_ARG, "C=%d must be in [1, %d]", C, trpl::kMaxCurves);
    if (!lengths_nm || !n_obs || !cA || !oA || !cB || !oB) return -api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    if (int rc = check_grid(L, T, 1, 1, time_ns)) return -rc;
    trpl::StepArgs a;
    memset(&a, 0, sizeof a);
    a.C = C; a.L = L; a.T = T;
    for (int c = 0; c < C; c++) {
        if (!(lengths_nm[c] > 0)) return -api_fail(TRPL_ERR_ARG, "lengths_nm[%d] must be > 0", c);
        curve_const(lengths_nm[c], time_ns, L, T, a.curve[c]);
        a.curve[c].n_obs = n_obs[c];
    }
    build_pair_table(a);
    for (int k = 0; k < a.pair_n; k++) { cA[k] = a.pair_cA[k]; oA[k] = a.pair_oA[k]; cB[k] = a.pair_cB[k]; oB[k] = a.pair_oB[k]; }
    return a.pair_n;
}

int trpl_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* ------------------------------------------------------------------ solve_pl ------------ */
// what both forms check alike; the rest of the head runs in each form's own order, as it always has
static int check_solve_counts(int64_t S, int32_t n_snap)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (n_snap < 0 || n_snap > trpl::kMaxSnaps) return api_fail(TRPL_ERR_ARG, "n_snap=%d must be in [0, %d]", n_snap, trpl::kMaxSnaps);
    return TRPL_OK;
}

static int solve_pl_dev_impl(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L, int64_t T,
                             int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, int64_t t0,
                             const double *resN, const double *resP, const double *resE, void *plI,
                             int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status, int64_t *iters_total,
                             const int64_t *snap_steps, int32_t n_snap, double *plN, double *plP, double *plE,
                             uint32_t flags, void *stream)
{
    const bool resume = resN || resP || resE;
    if (int rc = no_moments_flag(flags)) return rc;
    if (int rc = check_grid(L, T, plT, max_iter, time_ns)) return rc;
    if (int rc = check_solve_counts(S, n_snap)) return rc;
    if (n_snap > 0 && !snap_steps) return api_fail(TRPL_ERR_ARG, "snap_steps must not be NULL when n_snap > 0");
    if (resume && !(resN && resP && resE)) return api_fail(TRPL_ERR_ARG, "resN, resP and resE go together");
    if (resume && (t0 < 4 || t0 > T)) return api_fail(TRPL_ERR_ARG, "t0=%lld must be in [4, T]: a resume needs five BDF levels", (long long)t0);
    if (resume && (flags & TRPL_FLAG_FP32)) return api_fail(TRPL_ERR_UNSUPPORTED, "resume is not available with TRPL_FLAG_FP32");
    if (S == 0) return TRPL_OK;
    if (!matpar || (!dN && !resume) || !plI) return api_fail(TRPL_ERR_ARG, "matpar, dN and plI must not be NULL");
    if (pl_elem_bytes != 4 && pl_elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "pl_elem_bytes must be 4 or 8");
    if (pl_ld < T / plT + 1) return api_fail(TRPL_ERR_ARG, "pl_ld=%lld < T/plT+1", (long long)pl_ld);
    if (!(length_nm > 0)) return api_fail(TRPL_ERR_ARG, "length_nm must be > 0");
    if (S > 0x7fffffffLL) return api_fail(TRPL_ERR_ARG, "S too large for one launch");
    trpl::StepArgs a;
    memset(&a, 0, sizeof a);
    a.X = matpar; a.xld = 12; a.dN = dN;      // NULL on a resume: the kernels take the state from res* and never read it
    a.pl = plI; a.pl_bytes = pl_elem_bytes; a.pl_ld = pl_ld;
    a.status = status; a.iters_total = iters_total;
    a.S = S; a.C = 1; a.L = L; a.T = T; a.plT = kernel_plT(plT, T); a.MAX = max_iter; a.flags = flags;
    a.TOL = pow(10.0, -(double)tol_exp);                        /* pvSimPCR.py:112 */
    curve_const(length_nm, time_ns, L, T, a.curve[0]);
    if (resume) { a.resN = resN; a.resP = resP; a.resE = resE; a.t0 = t0; }
    if (n_snap > 0 && (plN || plP || plE)) {
        // (step, slot) pairs, steps strictly ascending: the slot of a step is its FIRST position in the
        // caller's list (Legacy/pvSim.py:122 `pT.index(t)`); steps outside [t0, T] are never reached
        a.snapN = plN; a.snapP = plP; a.snapE = plE; a.snap_ld = n_snap;
        for (int i = 0; i < n_snap; i++) {
            const int64_t st = snap_steps[i];
            if (st < (resume ? t0 : 0) || st > T) continue;
            bool seen = false;
            for (int k = 0; k < a.n_snap; k++) seen = seen || a.snap_t[k] == (int32_t)st;
            if (seen) continue;
            int at = a.n_snap++;
            while (at > 0 && a.snap_t[at - 1] > (int32_t)st) {
                a.snap_t[at] = a.snap_t[at - 1]; a.snap_slot[at] = a.snap_slot[at - 1]; at--;
            }
            a.snap_t[at] = (int32_t)st; a.snap_slot[at] = i;
        }
    }
    return launch(a, flags, (hipStream_t)stream, T - (resume ? t0 : 0));
}

int trpl_solve_pl_snap_dev(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L, int64_t T,
                           int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, void *plI,
                           int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status, int64_t *iters_total,
                           const int64_t *snap_steps, int32_t n_snap, double *plN, double *plP, double *plE,
                           uint32_t flags, void *stream)
{
    return solve_pl_dev_impl(matpar, S, length_nm, time_ns, L, T, plT, tol_exp, max_iter, dN, 0, nullptr, nullptr, nullptr,
                             plI, pl_elem_bytes, pl_ld, status, iters_total, snap_steps, n_snap, plN, plP, plE, flags, stream);
}

int trpl_solve_pl_resume_dev(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L, int64_t T,
                             int32_t plT, int32_t tol_exp, int32_t max_iter, int64_t t0, const double *resN,
                             const double *resP, const double *resE, void *plI, int32_t pl_elem_bytes, int64_t pl_ld,
                             int32_t *status, int64_t *iters_total, const int64_t *snap_steps, int32_t n_snap,
                             double *plN, double *plP, double *plE, uint32_t flags, void *stream)
{
    if (!resN || !resP || !resE) return api_fail(TRPL_ERR_ARG, "resN, resP and resE must not be NULL");
    return solve_pl_dev_impl(matpar, S, length_nm, time_ns, L, T, plT, tol_exp, max_iter, nullptr, t0, resN, resP, resE, plI,
                             pl_elem_bytes, pl_ld, status, iters_total, snap_steps, n_snap, plN, plP, plE, flags, stream);
}

int trpl_solve_pl_dev(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L, int64_t T,
                      int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, void *plI,
                      int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status, int64_t *iters_total, uint32_t flags,
                      void *stream)
{
    return trpl_solve_pl_snap_dev(matpar, S, length_nm, time_ns, L, T, plT, tol_exp, max_iter, dN, plI, pl_elem_bytes,
                                  pl_ld, status, iters_total, nullptr, 0, nullptr, nullptr, nullptr, flags, stream);
}

static int solve_pl_host_impl(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L, int64_t T,
                              int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, int64_t t0,
                              const double *resN, const double *resP, const double *resE, void *plI,
                              int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status, int64_t *iters_total,
                              const int64_t *snap_steps, int32_t n_snap, double *plN, double *plP, double *plE,
                              uint32_t flags, int32_t device, double *seconds)
{
    const bool resume = resN || resP || resE;
    if (int rc = no_moments_flag(flags)) return rc;
    if (resume && !(resN && resP && resE)) return api_fail(TRPL_ERR_ARG, "resN, resP and resE go together");
    if (int rc = check_grid(L, T, plT, max_iter, time_ns)) return rc;
    if (pl_elem_bytes != 4 && pl_elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "pl_elem_bytes must be 4 or 8");
    if (int rc = check_solve_counts(S, n_snap)) return rc;
    if (seconds) *seconds = 0.0;
    if (S == 0) return TRPL_OK;
    if (!matpar || (!dN && !resume) || !plI) return api_fail(TRPL_ERR_ARG, "matpar, dN and plI must not be NULL");
    const int64_t ncol = T / plT + 1;
    if (pl_ld < ncol) return api_fail(TRPL_ERR_ARG, "pl_ld=%lld < T/plT+1", (long long)pl_ld);
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    // A large PL matrix is written by the kernel STRAIGHT INTO the caller's buffer (pinned and mapped for
    // the duration of the call): the stores cross PCIe while the time-stepping goes on (a 1024 x 80 001 fp32
    // block is 328 MB over a ~0.3 s kernel, ~1 GB/s), so there is no device copy of the matrix and no
    // device-to-host copy after the kernel.  Small or unmappable buffers are staged through device memory:
    // on a resume as a copy of the caller's matrix, because columns before t0 are kept.
    const size_t eb = (size_t)pl_elem_bytes;
    void *dpl = sg.map(plI, ((size_t)(S - 1) * pl_ld + ncol) * eb);
    const int64_t dpl_ld = dpl ? pl_ld : ncol;
    if (!dpl) dpl = resume ? sg.inout(plI, pl_ld * eb, ncol * eb, (size_t)S) : sg.out(plI, pl_ld * eb, ncol * eb, (size_t)S);
    const double *dm = sg.in(matpar, (size_t)S * 12), *dn = sg.in(dN, (size_t)L);
    // the five BDF levels of every system, solver units
    const size_t rNP = (size_t)S * 5 * L, rE = (size_t)S * 5 * (L + 1);
    const double *rN = resume ? sg.in(resN, rNP) : nullptr, *rP = resume ? sg.in(resP, rNP) : nullptr;
    const double *rEd = resume ? sg.in(resE, rE) : nullptr;
    int32_t *ds = sg.out(status, (size_t)S);
    int64_t *di = sg.out(iters_total, (size_t)S);
    // snapshot buffers start as copies of the caller's (pvSimPCR.py:366-368): unfilled slots keep their contents
    const size_t nNP = (size_t)S * n_snap * L, nE = (size_t)S * n_snap * (L + 1);
    double *sN = n_snap > 0 && plN ? sg.inout(plN, nNP) : nullptr, *sP = n_snap > 0 && plP ? sg.inout(plP, nNP) : nullptr;
    double *sE = n_snap > 0 && plE ? sg.inout(plE, nE) : nullptr;
    if (int rc = sg.begin()) return rc;
    if (int rc = solve_pl_dev_impl(dm, S, length_nm, time_ns, L, T, plT, tol_exp, max_iter, dn, t0, rN, rP, rEd, dpl, pl_elem_bytes,
                                   dpl_ld, ds, di, snap_steps, n_snap, sN, sP, sE, flags, sg.stream()))
        return rc;
    return sg.finish(seconds);                                  /* pvSimPCR.py:378-381 */
}

int trpl_solve_pl_snap(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L, int64_t T,
                       int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, void *plI,
                       int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status, int64_t *iters_total,
                       const int64_t *snap_steps, int32_t n_snap, double *plN, double *plP, double *plE,
                       uint32_t flags, int32_t device, double *seconds)
{
    ProfRange range("trpl_solve_pl (pvSim)");
    return solve_pl_host_impl(matpar, S, length_nm, time_ns, L, T, plT, tol_exp, max_iter, dN, 0, nullptr, nullptr, nullptr,
                              plI, pl_elem_bytes, pl_ld, status, iters_total, snap_steps, n_snap, plN, plP, plE, flags,
                              device, seconds);
}

int trpl_solve_pl_resume(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L, int64_t T,
                         int32_t plT, int32_t tol_exp, int32_t max_iter, int64_t t0, const double *resN,
                         const double *resP, const double *resE, void *plI, int32_t pl_elem_bytes, int64_t pl_ld,
                         int32_t *status, int64_t *iters_total, const int64_t *snap_steps, int32_t n_snap, double *plN,
                         double *plP, double *plE, uint32_t flags, int32_t device, double *seconds)
{
    ProfRange range("trpl_solve_pl_resume (pvSim, init_mode continue)");
    if (!resN || !resP || !resE) return api_fail(TRPL_ERR_ARG, "resN, resP and resE must not be NULL");
    if (t0 < 4 || t0 > T) return api_fail(TRPL_ERR_ARG, "t0=%lld must be in [4, T]: a resume needs five BDF levels", (long long)t0);
    return solve_pl_host_impl(matpar, S, length_nm, time_ns, L, T, plT, tol_exp, max_iter, nullptr, t0, resN, resP, resE, plI,
                              pl_elem_bytes, pl_ld, status, iters_total, snap_steps, n_snap, plN, plP, plE, flags, device,
                              seconds);
}

int trpl_solve_pl(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L, int64_t T,
                  int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, void *plI,
                  int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status, int64_t *iters_total, uint32_t flags,
                  int32_t device, double *seconds)
{
    return trpl_solve_pl_snap(matpar, S, length_nm, time_ns, L, T, plT, tol_exp, max_iter, dN, plI, pl_elem_bytes, pl_ld,
                              status, iters_total, nullptr, 0, nullptr, nullptr, nullptr, flags, device, seconds);
}

/* ------------------------------------------------------------------ log10 clamp --------- */
// both forms: the host form's message names no numbers; its seconds are zeroed once the shape is accepted
static int check_log10_clamp(const void *x, int32_t elem_bytes, int64_t rows, int64_t cols, int64_t ld, bool numbers, double *seconds)
{
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes must be 4 or 8");
    if (rows < 0 || cols < 0 || ld < cols)
        return numbers ? api_fail(TRPL_ERR_ARG, "bad shape rows=%lld cols=%lld ld=%lld", (long long)rows, (long long)cols, (long long)ld)
                       : api_fail(TRPL_ERR_ARG, "bad shape");
    if (seconds) *seconds = 0.0;
    if (rows == 0 || cols == 0) return TRPL_OK;
    if (!x) return api_fail(TRPL_ERR_ARG, "x must not be NULL");
    return TRPL_OK;
}

int trpl_log10_clamp_dev(void *x, int32_t elem_bytes, int64_t rows, int64_t cols, int64_t ld, double min,
                         void *stream)
{
    if (int rc = check_log10_clamp(x, elem_bytes, rows, cols, ld, true, nullptr)) return rc;
    if (rows == 0 || cols == 0) return TRPL_OK;
    hipError_t e = trpl::launch_log10_clamp(x, elem_bytes, rows, cols, ld, min, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "log10_clamp launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_log10_clamp(void *x, int32_t elem_bytes, int64_t rows, int64_t cols, int64_t ld, double min,
                     int32_t device, double *seconds)
{
    ProfRange range("trpl_log10_clamp (fastlog)");
    if (int rc = check_log10_clamp(x, elem_bytes, rows, cols, ld, false, seconds)) return rc;
    if (rows == 0 || cols == 0) return TRPL_OK;
    Staged sg;
    if (int rc = sg.open(device, true)) return rc;               /* probs.py:79: the clock includes the copy in */
    const size_t eb = (size_t)elem_bytes;
    sg.pin(x, ((size_t)(rows - 1) * ld + cols) * eb);
    void *dx = sg.inout(x, ld * eb, cols * eb, (size_t)rows);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_log10_clamp_dev(dx, elem_bytes, rows, cols, cols, min, sg.stream())) return rc;
    return sg.finish(seconds);
}

/* ------------------------------------------------------------------ sse accumulate ------ */
// all four forms (weighted: trpl_sse_accumulate_w[_dev], probs.py:40); the host forms' seconds are zeroed once the shape is accepted
static int check_sse_accumulate(const double *P, const void *plI, int32_t elem_bytes, int64_t rows, int64_t n_obs, int64_t ld,
                                const double *values, const double *wts, bool weighted, const double *mag, double *seconds)
{
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes must be 4 or 8");
    if (rows < 0 || n_obs < 0 || ld < n_obs) return api_fail(TRPL_ERR_ARG, "bad shape");
    if (seconds) *seconds = 0.0;
    if (rows == 0) return TRPL_OK;
    if (!P || !mag || (n_obs && (!plI || !values || (weighted && !wts)))) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    return TRPL_OK;
}

int trpl_sse_accumulate_dev(double *P, const void *plI, int32_t elem_bytes, int64_t rows, int64_t n_obs,
                            int64_t ld, const double *values, const double *mag, void *stream)
{
    if (int rc = check_sse_accumulate(P, plI, elem_bytes, rows, n_obs, ld, values, nullptr, false, mag, nullptr)) return rc;
    if (rows == 0) return TRPL_OK;
    hipError_t e = trpl::launch_sse_accumulate(P, plI, elem_bytes, rows, n_obs, ld, values, mag, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "sse_accumulate launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_sse_accumulate_w_dev(double *P, const void *plI, int32_t elem_bytes, int64_t rows, int64_t n_obs, int64_t ld,
                              const double *values, const double *wts, const double *mag, void *stream)
{
    if (int rc = check_sse_accumulate(P, plI, elem_bytes, rows, n_obs, ld, values, wts, true, mag, nullptr)) return rc;
    if (rows == 0) return TRPL_OK;
    hipError_t e = trpl::launch_sse_accumulate_w(P, plI, elem_bytes, rows, n_obs, ld, values, wts, mag, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "sse_accumulate_w launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

// the host-buffer form of both, the arguments checked, rows > 0
static int sse_accumulate_staged(double *P, const void *plI, int32_t elem_bytes, int64_t rows, int64_t n_obs, int64_t ld,
                                 const double *values, const double *wts, bool weighted, const double *mag, int32_t device,
                                 double *seconds)
{
    Staged sg;
    if (int rc = sg.open(device, true)) return rc;               /* probs.py:51: the clock includes the copies in */
    const size_t eb = (size_t)elem_bytes;
    if (n_obs) sg.pin(plI, ((size_t)(rows - 1) * ld + n_obs) * eb);
    double *dP = sg.inout(P, (size_t)rows);
    const void *dpl = sg.in(plI, ld * eb, n_obs * eb, (size_t)rows);
    const double *dv = sg.in(values, (size_t)n_obs), *dw = weighted ? sg.in(wts, (size_t)n_obs) : nullptr, *dm = sg.in(mag, (size_t)rows);
    if (int rc = sg.begin()) return rc;
    if (int rc = weighted ? trpl_sse_accumulate_w_dev(dP, dpl, elem_bytes, rows, n_obs, n_obs, dv, dw, dm, sg.stream())
                          : trpl_sse_accumulate_dev(dP, dpl, elem_bytes, rows, n_obs, n_obs, dv, dm, sg.stream()))
        return rc;
    return sg.finish(seconds);
}

int trpl_sse_accumulate(double *P, const void *plI, int32_t elem_bytes, int64_t rows, int64_t n_obs, int64_t ld,
                        const double *values, const double *mag, int32_t device, double *seconds)
{
    ProfRange range("trpl_sse_accumulate (prob)");
    if (int rc = check_sse_accumulate(P, plI, elem_bytes, rows, n_obs, ld, values, nullptr, false, mag, seconds)) return rc;
    if (rows == 0) return TRPL_OK;
    return sse_accumulate_staged(P, plI, elem_bytes, rows, n_obs, ld, values, nullptr, false, mag, device, seconds);
}

// the weights of one curve, host data: finite and >= 0
static int check_weights(const double *w, int64_t n, int c)
{
    for (int64_t i = 0; i < n; i++)
        if (!(w[i] >= 0.0) || !(w[i] < INFINITY))
            return api_fail(TRPL_ERR_ARG, "weight of curve %d, index %lld is %g: weights must be finite and >= 0", c, (long long)i, w[i]);
    return TRPL_OK;
}

int trpl_sse_accumulate_w(double *P, const void *plI, int32_t elem_bytes, int64_t rows, int64_t n_obs, int64_t ld,
                          const double *values, const double *wts, const double *mag, int32_t device, double *seconds)
{
    ProfRange range("trpl_sse_accumulate_w (prob, uncertainty-weighted)");
    if (int rc = check_sse_accumulate(P, plI, elem_bytes, rows, n_obs, ld, values, wts, true, mag, seconds)) return rc;
    if (rows == 0) return TRPL_OK;
    if (int rc = check_weights(wts, n_obs, 0)) return rc;
    return sse_accumulate_staged(P, plI, elem_bytes, rows, n_obs, ld, values, wts, true, mag, device, seconds);
}

/* ------------------------------------------------------------------ loglik from stored PL */
static int loglik_from_pl_impl(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                               const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                               int64_t n_obs, const double *mag, const int32_t *status, double *P, double *sse,
                               double *esum, uint32_t flags, void *stream, const double *wts = nullptr)
{
    if (int rc = no_moments_flag(flags)) return rc;
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes must be 4 or 8");
    if (rows < 0 || ncol < 1 || ld < ncol || n_obs < 0) return api_fail(TRPL_ERR_ARG, "bad shape");
    const bool interp = obs_hi || obs_dx || obs_h;
    if (interp && !(obs_hi && obs_dx && obs_h)) return api_fail(TRPL_ERR_ARG, "obs_hi, obs_dx and obs_h go together");
    if (!interp && n_obs > ncol) return api_fail(TRPL_ERR_ARG, "n_obs=%lld exceeds the %lld PL columns", (long long)n_obs, (long long)ncol);
    if (rows > 0x7fffffffLL) return api_fail(TRPL_ERR_ARG, "too many rows for one launch");
    if (rows == 0) return TRPL_OK;
    if (!plI || !mag || (n_obs && !obs) || (!P && !sse && !esum)) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    hipError_t e = trpl::launch_pl_loglik(plI, elem_bytes, rows, ld, obs, obs_hi, obs_dx, obs_h, n_obs, mag, status, P, sse, flags,
                                          (hipStream_t)stream, esum, wts);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "pl_loglik launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_loglik_from_pl_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                            const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                            int64_t n_obs, const double *mag, const int32_t *status, double *P, double *sse,
                            uint32_t flags, void *stream)
{
    return loglik_from_pl_impl(plI, elem_bytes, rows, ncol, ld, obs, obs_hi, obs_dx, obs_h, n_obs, mag, status, P, sse, nullptr,
                               flags, stream);
}

int trpl_loglik_moments_from_pl_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                                    const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                                    int64_t n_obs, const double *mag, const int32_t *status, double *P, double *sse,
                                    double *esum, uint32_t flags, void *stream)
{
    return loglik_from_pl_impl(plI, elem_bytes, rows, ncol, ld, obs, obs_hi, obs_dx, obs_h, n_obs, mag, status, P, sse, esum,
                               flags, stream);
}

int trpl_loglik_weighted_from_pl_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                                     const double *obs, const double *wts, const int32_t *obs_hi, const double *obs_dx,
                                     const double *obs_h, int64_t n_obs, const double *mag, const int32_t *status, double *P,
                                     double *sse, double *esum, uint32_t flags, void *stream)
{
    if (rows > 0 && n_obs > 0 && !wts) return api_fail(TRPL_ERR_ARG, "wts must not be NULL");
    return loglik_from_pl_impl(plI, elem_bytes, rows, ncol, ld, obs, obs_hi, obs_dx, obs_h, n_obs, mag, status, P, sse, esum,
                               flags, stream, n_obs > 0 ? wts : nullptr);
}

/* ------------------------------------------------------------------ fused loglik -------- */
// Which of the two flags the entry points set themselves a call may carry: wts -- the weighted entry points (they set
// TRPL_FLAG_WEIGHTED; with TRPL_FLAG_MOMENTS: refused, the weighted sink already emits both sums); esum alone -- the moments entry
// points (they set TRPL_FLAG_MOMENTS); every other caller must carry neither.
static int entry_flags(uint32_t &flags, bool esum, bool wts, bool cut = false)
{
    if (cut) {                                       // trpl_loglik_cut[_dev]: they set TRPL_FLAG_CUT
        flags |= TRPL_FLAG_CUT;
        return check_cut_flags(flags);
    }
    if (wts) {
        if (int rc = no_cut_flag(flags)) return rc;
        if (flags & TRPL_FLAG_MOMENTS)
            return api_fail(TRPL_ERR_ARG, "TRPL_FLAG_MOMENTS does not combine with TRPL_FLAG_WEIGHTED: the weighted sink already emits both sums");
        flags |= TRPL_FLAG_WEIGHTED;
        return TRPL_OK;
    }
    if (esum) {
        if (int rc = no_weighted_flag(flags)) return rc;
        flags |= TRPL_FLAG_MOMENTS;
        return TRPL_OK;
    }
    return no_moments_flag(flags);
}

// the sink flag of the record's optional pointers and the sse_cut range: the first checks of both forms
static int check_sink(const LoglikCall &k, uint32_t &flags)
{
    // sse_cut, or cut_level in its place: the cut entry points (both NULL everywhere else)
    if (int rc = entry_flags(flags, k.esum != nullptr, k.wts != nullptr, k.sse_cut != nullptr || k.cut_level != nullptr)) return rc;
    if (k.sse_cut && !(*k.sse_cut >= 0.0)) return api_fail(TRPL_ERR_ARG, "sse_cut=%g must be >= 0 or +inf", *k.sse_cut);
    return TRPL_OK;
}

}  // extern "C": trpl::loglik_dev is called from trpl_multi.hip too

int trpl::loglik_dev(const LoglikCall &k, hipStream_t stream)
{
    uint32_t flags = k.flags;
    if (int rc = check_sink(k, flags)) return rc;
    if (int rc = check_batch(k)) return rc;
    const int64_t S = k.S, T = k.T, obs_ld = k.obs_ld;
    const int32_t C = k.C, L = k.L;
    if (S == 0) return TRPL_OK;
    if (!k.X || !k.lengths_nm || !k.dN || !k.obs || !k.n_obs || !k.P || !k.sse) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    if (int rc = check_interp(k.obs_hi, k.obs_dx, k.obs_h, k.plT)) return rc;
    const bool interp = k.obs_hi != nullptr;
    const int64_t ncol = T / k.plT + 1;
    for (int c = 0; c < C; c++) {
        if (!(k.lengths_nm[c] > 0)) return api_fail(TRPL_ERR_ARG, "lengths_nm[%d] must be > 0", c);
        if (k.n_obs[c] < 1 || k.n_obs[c] > obs_ld || (!interp && k.n_obs[c] > ncol))
            return api_fail(TRPL_ERR_ARG, "n_obs[%d]=%lld out of range (obs_ld %lld, grid columns %lld)", c,
                        (long long)k.n_obs[c], (long long)obs_ld, (long long)ncol);
    }
    // A launch carries the constants of at most kMaxCurves curves in its argument block; bayeslib.simulate loops over any
    // number of curves (bayeslib.py:117), so more are run as consecutive launches of up to kMaxCurves on the same stream,
    // each writing its own rows of the [C][S] outputs, before ONE reduction over all C in curve order (probs.py:44).  The
    // stepper variant is chosen once from the whole batch, so a system's bits do not depend on the grouping.
    // trpl_loglik_cut_budget[_dev] (k.budget): groups of curves_per_launch curves instead, and before each group the kernel of
    // cut_budget.hip writes the group's rows of cut_level from the budget and the sse rows the earlier groups have reported
    // (stream order: a group's sinks read levels that are complete, and its sse is complete before the next group's levels).
    const int64_t steps = loglik_steps(interp, C, k.n_obs, k.plT, T);
    const int group = k.budget ? k.curves_per_launch : trpl::kMaxCurves;
    if (k.budget && (group < 1 || group > trpl::kMaxCurves || !k.cut_level))
        return api_fail(TRPL_ERR_ARG, "curves_per_launch=%d must be in [1, %d], with a cut_level to fill", group, trpl::kMaxCurves);
    if (C > group) flags = pin_variant(flags, S * (int64_t)C, L, steps);
    for (int c0 = 0; c0 < C; c0 += group) {
        const int Cg = C - c0 < group ? C - c0 : group;
        if (S * (int64_t)Cg > 0x7fffffffLL) return api_fail(TRPL_ERR_ARG, "S*C too large for one launch");
        if (k.budget) {
            hipError_t e = trpl::launch_budget_level(k.budget, k.sse, const_cast<double *>(k.cut_level), S, c0, Cg, stream);
            if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "budget level launch: %s", hipGetErrorString(e));
        }
        trpl::StepArgs a;
        memset(&a, 0, sizeof a);
        a.X = k.X; a.xld = 13; a.dN = k.dN + (int64_t)c0 * L; a.obs = k.obs + (int64_t)c0 * obs_ld;
        a.obs_hi = k.obs_hi ? k.obs_hi + (int64_t)c0 * obs_ld : nullptr;
        a.obs_dx = k.obs_dx ? k.obs_dx + (int64_t)c0 * obs_ld : nullptr;
        a.obs_h = k.obs_h ? k.obs_h + (int64_t)c0 * obs_ld : nullptr;
        a.obs_ld = obs_ld; a.sse = k.sse + (int64_t)c0 * S;
        a.esum = k.esum ? k.esum + (int64_t)c0 * S : nullptr;
        a.wts = k.wts ? k.wts + (int64_t)c0 * obs_ld : nullptr;
        a.sse_cut = k.sse_cut ? *k.sse_cut : 0.0;
        a.cut_col = k.cut_col ? k.cut_col + (int64_t)c0 * S : nullptr;
        a.cut_level = k.cut_level ? k.cut_level + (int64_t)c0 * S : nullptr;
        a.status = k.status ? k.status + (int64_t)c0 * S : nullptr;
        a.iters_total = k.iters_total ? k.iters_total + (int64_t)c0 * S : nullptr;
        a.floor_col = k.floor_col ? k.floor_col + (int64_t)c0 * S : nullptr;
        a.S = S; a.C = Cg; a.L = L; a.T = T; a.plT = kernel_plT(k.plT, T); a.MAX = k.max_iter; a.flags = flags;
        a.TOL = pow(10.0, -(double)k.tol_exp);
        for (int c = 0; c < Cg; c++) {
            curve_const(k.lengths_nm[c0 + c], k.time_ns, L, T, a.curve[c]);
            a.curve[c].n_obs = k.n_obs[c0 + c];
        }
        if (int rc = launch(a, flags, stream, steps)) return rc;
    }
    hipError_t e = trpl::launch_reduce_curves(k.P, k.sse, S, C, stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "reduce_curves launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

// the host-buffer form of loglik_dev: the record's pointers are the caller's host arrays
static int loglik_host(const LoglikCall &k, int32_t device, double *seconds)
{
    { uint32_t f = k.flags; if (int rc = check_sink(k, f)) return rc; }
    if (int rc = check_batch(k)) return rc;
    if (seconds) *seconds = 0.0;
    if (k.S == 0) return TRPL_OK;
    if (!k.X || !k.lengths_nm || !k.dN || !k.obs || !k.n_obs || !k.P) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    if (k.obs_ld < 1) return api_fail(TRPL_ERR_ARG, "obs_ld must be >= 1");
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const bool interp = k.obs_hi != nullptr;
    if (interp) {                                    // the brackets are host data here: validate them
        if (int rc = check_brackets(k.obs_hi, k.obs_dx, k.obs_h, k.C, k.obs_ld, k.n_obs, k.T)) return rc;
    }
    // sse, status and iters_total are the _dev form's whether the caller takes them or not; floor_col, esum and cut_col only on request
    const size_t nsys = (size_t)k.S * k.C, nobs = (size_t)k.C * k.obs_ld;
    LoglikCall d = k;
    d.X = sg.in(k.X, (size_t)k.S * 13); d.dN = sg.in(k.dN, (size_t)k.C * k.L); d.obs = sg.in(k.obs, nobs);
    d.wts = k.wts ? sg.in(k.wts, nobs) : nullptr;
    d.obs_hi = interp ? sg.in(k.obs_hi, nobs) : nullptr;
    d.obs_dx = interp ? sg.in(k.obs_dx, nobs) : nullptr; d.obs_h = interp ? sg.in(k.obs_h, nobs) : nullptr;
    d.P = sg.inout(k.P, (size_t)k.S); d.sse = sg.out(k.sse, nsys); d.esum = k.esum ? sg.out(k.esum, nsys) : nullptr;
    d.status = sg.out(k.status, nsys); d.floor_col = k.floor_col ? sg.out(k.floor_col, nsys) : nullptr;
    d.cut_col = k.cut_col ? sg.out(k.cut_col, nsys) : nullptr;
    if (k.budget) {                                  // the budget in, the levels every system ran at out
        d.budget = sg.in(k.budget, (size_t)k.S);
        d.cut_level = sg.out(const_cast<double *>(k.cut_level), nsys);
    } else {
        d.cut_level = k.cut_level ? sg.in(k.cut_level, nsys) : nullptr;
    }
    d.iters_total = sg.out(k.iters_total, nsys);
    if (int rc = sg.begin()) return rc;
    if (int rc = loglik_dev(d, sg.stream())) return rc;
    return sg.finish(seconds);
}

/* ------------------------------------------------------------------ magnitude grid and profile from the moments */
// trpl_mag_grid[_w][_dev] and trpl_mag_profile[_w][_dev]: one body per operation.  The per-curve coefficient is a count (N = int64_t:
// n_obs, >= 1, converted exactly) or a sum of weights (N = double: wsum, finite and >= 0); either way likelihood.hip gets doubles.
// on_device: the kernels on `stream`; else the host loop.
template <typename N>
static int check_mag(const double *sse, const double *esum, const N *v, int64_t S, int32_t C, const double *P, bool need_P, double *n)
{
    constexpr bool counts = std::is_same_v<N, int64_t>;
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (C < 1 || C > TRPL_MAG_MAX_CURVES) return api_fail(TRPL_ERR_ARG, "C=%d must be in [1, %d]", C, TRPL_MAG_MAX_CURVES);
    if (!v) return api_fail(TRPL_ERR_ARG, "%s must not be NULL", counts ? "n_obs" : "wsum");
    for (int c = 0; c < C; c++) {
        if constexpr (counts) {
            if (v[c] < 1) return api_fail(TRPL_ERR_ARG, "n_obs[%d]=%lld must be >= 1", c, (long long)v[c]);
        } else {
            if (!(v[c] >= 0.0) || !(v[c] < INFINITY)) return api_fail(TRPL_ERR_ARG, "wsum[%d]=%g must be finite and >= 0", c, v[c]);
        }
        n[c] = (double)v[c];
    }
    if (S > 0 && (!sse || !esum || (need_P && !P))) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    return TRPL_OK;
}

template <typename N>
static int mag_grid(const double *sse, const double *esum, const N *v, int64_t S, int32_t C, const double *offsets, int64_t M,
                    double *P, bool on_device, void *stream)
{
    double n[trpl::kMagMaxCurves];
    if (M < 0) return api_fail(TRPL_ERR_ARG, "M must be >= 0");
    if (int rc = check_mag(sse, esum, v, S, C, P, M > 0, n)) return rc;
    if (S == 0 || M == 0) return TRPL_OK;
    if (!offsets) return api_fail(TRPL_ERR_ARG, "offsets must not be NULL");
    if (!on_device) { trpl::mag_grid_host_w(sse, esum, n, S, C, offsets, M, P); return TRPL_OK; }
    hipError_t e = trpl::launch_mag_grid_w(sse, esum, n, S, C, offsets, M, P, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "mag_grid%s launch: %s", std::is_same_v<N, double> ? "_w" : "", hipGetErrorString(e));
    return TRPL_OK;
}

template <typename N>
static int mag_profile(const double *sse, const double *esum, const N *v, int64_t S, int32_t C, uint32_t flags, double *best,
                       double *P, bool on_device, void *stream)
{
    const char *w = std::is_same_v<N, double> ? "_w" : "";
    double n[trpl::kMagMaxCurves];
    if (flags & ~(uint32_t)TRPL_MAG_PER_CURVE) return api_fail(TRPL_ERR_ARG, "trpl_mag_profile%s: unknown flag bits 0x%x", w, flags);
    if (int rc = check_mag(sse, esum, v, S, C, P, true, n)) return rc;
    if (S == 0) return TRPL_OK;
    if (!best) return api_fail(TRPL_ERR_ARG, "best must not be NULL");
    const bool per_curve = (flags & TRPL_MAG_PER_CURVE) != 0;
    if (!on_device) { trpl::mag_profile_host_w(sse, esum, n, S, C, per_curve, best, P); return TRPL_OK; }
    hipError_t e = trpl::launch_mag_profile_w(sse, esum, n, S, C, per_curve, best, P, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "mag_profile%s launch: %s", w, hipGetErrorString(e));
    return TRPL_OK;
}

extern "C" {

int trpl_loglik_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                    int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                    const double *obs, int64_t obs_ld, const int64_t *n_obs, double *P, double *sse,
                    int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags, void *stream)
{
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    return loglik_dev(k, (hipStream_t)stream);
}

int trpl_loglik_obs_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                        int64_t T, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                        const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                        const int64_t *n_obs, double *P, double *sse, int32_t *status, int64_t *iters_total,
                        int32_t *floor_col, uint32_t flags, void *stream)
{
    if (!obs_hi || !obs_dx || !obs_h) return api_fail(TRPL_ERR_ARG, "obs_hi, obs_dx and obs_h must not be NULL");
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = 1; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h;
    return loglik_dev(k, (hipStream_t)stream);
}

int trpl_loglik(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                int64_t obs_ld, const int64_t *n_obs, double *P, double *sse, int32_t *status,
                int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device, double *seconds)
{
    ProfRange range("trpl_loglik (pvSim + fastlog + prob, fused)");
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    return loglik_host(k, device, seconds);
}

int trpl_loglik_obs(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                    int64_t T, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                    const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                    const int64_t *n_obs, double *P, double *sse, int32_t *status, int64_t *iters_total,
                    int32_t *floor_col, uint32_t flags, int32_t device, double *seconds)
{
    ProfRange range("trpl_loglik_obs (pvSim + fastlog + griddata + prob, fused)");
    if (!obs_hi || !obs_dx || !obs_h) return api_fail(TRPL_ERR_ARG, "obs_hi, obs_dx and obs_h must not be NULL");
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = 1; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h;
    return loglik_host(k, device, seconds);
}

/* ------------------------------------------------------------------ moments + magnitude grid (probs.py:5-18) */
int trpl_loglik_moments_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                            int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                            const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                            const int64_t *n_obs, double *P, double *sse, double *esum, int32_t *status,
                            int64_t *iters_total, int32_t *floor_col, uint32_t flags, void *stream)
{
    if (S > 0 && !esum) return api_fail(TRPL_ERR_ARG, "esum must not be NULL");
    if (S == 0) flags &= ~(uint32_t)TRPL_FLAG_MOMENTS;            // nothing is launched; the common checks still run
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.esum = esum;
    return loglik_dev(k, (hipStream_t)stream);
}

int trpl_loglik_moments(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                        int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                        const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                        const int64_t *n_obs, double *P, double *sse, double *esum, int32_t *status, int64_t *iters_total,
                        int32_t *floor_col, uint32_t flags, int32_t device, double *seconds)
{
    ProfRange range("trpl_loglik_moments (pvSim + fastlog + lnP's mag_grid moments, fused)");
    if (S > 0 && !esum) return api_fail(TRPL_ERR_ARG, "esum must not be NULL");
    if (int rc = check_interp(obs_hi, obs_dx, obs_h, plT)) return rc;
    if (S == 0) flags &= ~(uint32_t)TRPL_FLAG_MOMENTS;
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.esum = esum;
    return loglik_host(k, device, seconds);
}

/* ------------------------------------------------------------------ fused loglik with early stop (probs.py:5-18 bval_cutoff) */
int trpl_loglik_cut_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                        int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                        const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                        const int64_t *n_obs, double sse_cut, double *P, double *sse, int32_t *cut_col, int32_t *status,
                        int64_t *iters_total, int32_t *floor_col, uint32_t flags, void *stream)
{
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.sse_cut = &sse_cut; k.cut_col = cut_col;
    return loglik_dev(k, (hipStream_t)stream);
}

int trpl_loglik_cut(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                    int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                    const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                    const int64_t *n_obs, double sse_cut, double *P, double *sse, int32_t *cut_col, int32_t *status,
                    int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device, double *seconds)
{
    ProfRange range("trpl_loglik_cut (pvSim + fastlog + prob with early stop, fused)");
    if (int rc = check_interp(obs_hi, obs_dx, obs_h, plT)) return rc;
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.sse_cut = &sse_cut; k.cut_col = cut_col;
    return loglik_host(k, device, seconds);
}

/* ------------------------------------------------------------------ the early stop with a level per system (MCMC early rejection) */
// the host form sees its levels: each >= 0 or +inf, checked before a device is touched
static int check_levels(const double *cut_level, int64_t S, int32_t C)
{
    for (int32_t c = 0; c < C; c++)
        for (int64_t s = 0; s < S; s++)
            if (!(cut_level[(int64_t)c * S + s] >= 0.0))
                return api_fail(TRPL_ERR_ARG, "cut_level[c=%d][s=%lld]=%g must be >= 0 or +inf", c, (long long)s, cut_level[(int64_t)c * S + s]);
    return TRPL_OK;
}

int trpl_loglik_cut_levels_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                               int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                               const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                               const int64_t *n_obs, const double *cut_level, double *P, double *sse, int32_t *cut_col,
                               int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags, void *stream)
{
    if (S > 0 && !cut_level) return api_fail(TRPL_ERR_ARG, "cut_level must not be NULL");
    const double none = INFINITY;                                 // S == 0: nothing is launched; the common checks still run
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.cut_col = cut_col;
    if (S > 0) k.cut_level = cut_level; else k.sse_cut = &none;
    return loglik_dev(k, (hipStream_t)stream);
}

int trpl_loglik_cut_levels(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                           int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                           const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                           const int64_t *n_obs, const double *cut_level, double *P, double *sse, int32_t *cut_col,
                           int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device,
                           double *seconds)
{
    ProfRange range("trpl_loglik_cut_levels (pvSim + fastlog + prob with a stop level per system, fused)");
    if (S > 0 && !cut_level) return api_fail(TRPL_ERR_ARG, "cut_level must not be NULL");
    if (int rc = check_interp(obs_hi, obs_dx, obs_h, plT)) return rc;
    const double none = INFINITY;
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.cut_col = cut_col;
    if (S > 0) k.cut_level = cut_level; else k.sse_cut = &none;
    { uint32_t f = flags; if (int rc = check_sink(k, f)) return rc; }       // the flag refusals before the levels are read
    if (int rc = check_batch(k)) return rc;                                  // S >= 0 and C in range: the extent of cut_level
    if (S > 0) { if (int rc = check_levels(cut_level, S, C)) return rc; }
    return loglik_host(k, device, seconds);
}

/* ------------------------------------------------------------------ the early stop on a sample's total: a budget carried across the curves */
// what both forms refuse before anything else: the two arrays and the group size
static int check_budget_args(int64_t S, const double *budget, int32_t curves_per_launch, const double *cut_level)
{
    if (S > 0 && !budget) return api_fail(TRPL_ERR_ARG, "budget must not be NULL");
    if (S > 0 && !cut_level) return api_fail(TRPL_ERR_ARG, "cut_level must not be NULL");
    if (curves_per_launch < 1 || curves_per_launch > trpl::kMaxCurves)
        return api_fail(TRPL_ERR_ARG, "curves_per_launch=%d must be in [1, %d]", curves_per_launch, trpl::kMaxCurves);
    return TRPL_OK;
}

int trpl_loglik_cut_budget_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                               int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                               const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                               const int64_t *n_obs, const double *budget, int32_t curves_per_launch, double *cut_level, double *P,
                               double *sse, int32_t *cut_col, int32_t *status, int64_t *iters_total, int32_t *floor_col,
                               uint32_t flags, void *stream)
{
    if (int rc = check_budget_args(S, budget, curves_per_launch, cut_level)) return rc;
    const double none = INFINITY;                                 // S == 0: nothing is launched; the common checks still run
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.cut_col = cut_col;
    if (S > 0) { k.budget = budget; k.curves_per_launch = curves_per_launch; k.cut_level = cut_level; } else k.sse_cut = &none;
    return loglik_dev(k, (hipStream_t)stream);
}

int trpl_loglik_cut_budget(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                           int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                           const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t obs_ld,
                           const int64_t *n_obs, const double *budget, int32_t curves_per_launch, double *cut_level, double *P,
                           double *sse, int32_t *cut_col, int32_t *status, int64_t *iters_total, int32_t *floor_col,
                           uint32_t flags, int32_t device, double *seconds)
{
    ProfRange range("trpl_loglik_cut_budget (pvSim + fastlog + prob with a stop budget per sample, fused)");
    if (int rc = check_budget_args(S, budget, curves_per_launch, cut_level)) return rc;
    if (int rc = check_interp(obs_hi, obs_dx, obs_h, plT)) return rc;
    const double none = INFINITY;
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.cut_col = cut_col;
    if (S > 0) { k.budget = budget; k.curves_per_launch = curves_per_launch; k.cut_level = cut_level; } else k.sse_cut = &none;
    { uint32_t f = flags; if (int rc = check_sink(k, f)) return rc; }       // the flag refusals before the budgets are read
    if (int rc = check_batch(k)) return rc;
    for (int64_t s = 0; s < S; s++)                                          // the host form sees its budgets: each >= 0 or +inf
        if (!(budget[s] >= 0.0)) return api_fail(TRPL_ERR_ARG, "budget[s=%lld]=%g must be >= 0 or +inf", (long long)s, budget[s]);
    return loglik_host(k, device, seconds);
}

/* ------------------------------------------------------------------ uncertainty-weighted fused loglik (probs.py:40) */
int trpl_loglik_weighted_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                             int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                             const double *wts, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                             int64_t obs_ld, const int64_t *n_obs, double *P, double *sse, double *esum, int32_t *status,
                             int64_t *iters_total, int32_t *floor_col, uint32_t flags, void *stream)
{
    if (S > 0 && (!esum || !wts)) return api_fail(TRPL_ERR_ARG, "esum and wts must not be NULL");
    if (S == 0) flags &= ~(uint32_t)TRPL_FLAG_WEIGHTED;           // nothing is launched; the common checks still run
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.esum = esum; k.wts = S > 0 ? wts : nullptr;
    return loglik_dev(k, (hipStream_t)stream);
}

int trpl_loglik_weighted(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns, int32_t L,
                         int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN, const double *obs,
                         const double *wts, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                         int64_t obs_ld, const int64_t *n_obs, double *P, double *sse, double *esum, int32_t *status,
                         int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device, double *seconds)
{
    ProfRange range("trpl_loglik_weighted (pvSim + fastlog + uncertainty-weighted prob, fused)");
    if (S > 0 && (!esum || !wts)) return api_fail(TRPL_ERR_ARG, "esum and wts must not be NULL");
    if (int rc = check_interp(obs_hi, obs_dx, obs_h, plT)) return rc;
    if (S == 0) flags &= ~(uint32_t)TRPL_FLAG_WEIGHTED;
    if (S > 0 && n_obs && C >= 1 && C <= TRPL_MAX_CURVES && obs_ld >= 1)      // the weights are host data here: validate them
        for (int c = 0; c < C; c++)
            if (n_obs[c] >= 1 && n_obs[c] <= obs_ld)
                if (int rc = check_weights(wts + (int64_t)c * obs_ld, n_obs[c], c)) return rc;
    LoglikCall k;
    k.X = X; k.S = S; k.C = C; k.lengths_nm = lengths_nm; k.time_ns = time_ns; k.L = L; k.T = T; k.plT = plT; k.tol_exp = tol_exp;
    k.max_iter = max_iter; k.dN = dN; k.obs = obs; k.obs_ld = obs_ld; k.n_obs = n_obs; k.P = P; k.sse = sse; k.status = status;
    k.iters_total = iters_total; k.floor_col = floor_col; k.flags = flags;
    k.obs_hi = obs_hi; k.obs_dx = obs_dx; k.obs_h = obs_h; k.esum = esum; k.wts = S > 0 ? wts : nullptr;
    return loglik_host(k, device, seconds);
}

int trpl_mag_grid_w(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C, const double *offsets,
                    int64_t M, double *P)
{
    return mag_grid(sse, esum, wsum, S, C, offsets, M, P, false, nullptr);
}

int trpl_mag_grid_w_dev(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C, const double *offsets,
                        int64_t M, double *P, void *stream)
{
    return mag_grid(sse, esum, wsum, S, C, offsets, M, P, true, stream);
}

int trpl_mag_profile_w(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C, uint32_t flags,
                       double *best, double *P)
{
    return mag_profile(sse, esum, wsum, S, C, flags, best, P, false, nullptr);
}

int trpl_mag_profile_w_dev(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C, uint32_t flags,
                           double *best, double *P, void *stream)
{
    return mag_profile(sse, esum, wsum, S, C, flags, best, P, true, stream);
}

int trpl_mag_grid(const double *sse, const double *esum, const int64_t *n_obs, int64_t S, int32_t C, const double *offsets,
                  int64_t M, double *P)
{
    return mag_grid(sse, esum, n_obs, S, C, offsets, M, P, false, nullptr);
}

int trpl_mag_grid_dev(const double *sse, const double *esum, const int64_t *n_obs, int64_t S, int32_t C, const double *offsets,
                      int64_t M, double *P, void *stream)
{
    return mag_grid(sse, esum, n_obs, S, C, offsets, M, P, true, stream);
}

int trpl_mag_profile(const double *sse, const double *esum, const int64_t *n_obs, int64_t S, int32_t C, uint32_t flags,
                     double *best, double *P)
{
    return mag_profile(sse, esum, n_obs, S, C, flags, best, P, false, nullptr);
}

int trpl_mag_profile_dev(const double *sse, const double *esum, const int64_t *n_obs, int64_t S, int32_t C, uint32_t flags,
                         double *best, double *P, void *stream)
{
    return mag_profile(sse, esum, n_obs, S, C, flags, best, P, true, stream);
}

/* ------------------------------------------------------------------ host interpolation --- */
int trpl_interp_rows(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const int32_t *hi,
                     const double *dx, const double *h, int64_t n_obs, double *out, int64_t out_ld)
{
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes must be 4 or 8");
    if (rows < 0 || n_obs < 0 || ncol < 2 || ld < ncol || out_ld < n_obs) return api_fail(TRPL_ERR_ARG, "bad shape");
    if (rows == 0 || n_obs == 0) return TRPL_OK;
    if (!pl || !hi || !dx || !h || !out) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    for (int64_t i = 0; i < n_obs; i++)
        if (hi[i] < 1 || hi[i] >= ncol) return api_fail(TRPL_ERR_ARG, "hi[%lld]=%d must be in [1, ncol - 1]", (long long)i, hi[i]);
    trpl::interp_rows_any(pl, elem_bytes, rows, ld, hi, dx, h, n_obs, out, out_ld);
    return TRPL_OK;
}

/* ------------------------------------------------------------------ posterior core ------ */
int64_t trpl_posterior_workspace_bytes(int32_t D) { return (int64_t)trpl::posterior_workspace_bytes(D); }

// The weights with and without a proposal log-ratio lnr are one call path below the argument checks, which differ: the plain
// call accepts S == 0 (nothing to do) and has one message for its pointers, the log-ratio call refuses S < 1 and names the pointer.
static int check_post_weights(const void *LL, int64_t S, double tf, const void *W, bool have_workspace)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (S == 0) return TRPL_OK;
    if (!LL || !W || !have_workspace) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    if (!(tf > 0)) return api_fail(TRPL_ERR_ARG, "tf must be > 0");
    return TRPL_OK;
}

static int check_post_weights_lr(const void *LL, const void *lnr, int64_t S, double tf, const void *W)
{
    if (S < 1) return api_fail(TRPL_ERR_ARG, "S=%lld must be >= 1", (long long)S);
    if (!LL) return api_fail(TRPL_ERR_ARG, "LL is NULL");
    if (!lnr) return api_fail(TRPL_ERR_ARG, "lnr is NULL");
    if (!W) return api_fail(TRPL_ERR_ARG, "W is NULL");
    if (!(tf > 0) || !(tf < INFINITY)) return api_fail(TRPL_ERR_ARG, "tf=%g must be finite and > 0", tf);
    return TRPL_OK;
}

static int weights_launch(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats, void *workspace,
                          void *stream)
{
    hipError_t e = trpl::launch_posterior_weights(LL, lnr, S, tf, W, stats, (double *)workspace, (hipStream_t)stream);
    if (e != hipSuccess)
        return api_fail(TRPL_ERR_HIP, "posterior weights%s launch: %s", lnr ? " (log-ratio)" : "", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_posterior_weights_dev(const double *LL, int64_t S, double tf, double *W, double *stats, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    if (int rc = check_post_weights(LL, S, tf, W, workspace != nullptr)) return rc;
    if (S == 0) return TRPL_OK;
    if (workspace_bytes < (int64_t)trpl::posterior_workspace_bytes(1)) return api_fail(TRPL_ERR_ARG, "workspace too small");
    return weights_launch(LL, nullptr, S, tf, W, stats, workspace, stream);
}

int trpl_posterior_weights_lr_dev(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats,
                                  void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = check_post_weights_lr(LL, lnr, S, tf, W)) return rc;
    if (!workspace) return api_fail(TRPL_ERR_ARG, "workspace is NULL");
    if (workspace_bytes < (int64_t)trpl::posterior_workspace_bytes(1))
        return api_fail(TRPL_ERR_ARG, "workspace of %lld bytes is smaller than trpl_posterior_workspace_bytes(1) = %lld",
                        (long long)workspace_bytes, (long long)trpl::posterior_workspace_bytes(1));
    return weights_launch(LL, lnr, S, tf, W, stats, workspace, stream);
}

// the host-buffer form of both, the arguments checked: stages LL (and lnr), runs the device form, copies W and stats back
static int weights_staged(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats, int32_t device,
                          double *seconds)
{
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const size_t wsb = trpl::posterior_workspace_bytes(1);
    const double *dL = sg.in(LL, (size_t)S), *dR = lnr ? sg.in(lnr, (size_t)S) : nullptr;
    double *dW = sg.out(W, (size_t)S), *dSt = sg.out(stats, 2);
    void *ws = sg.scratch(wsb);
    if (int rc = sg.begin()) return rc;
    if (int rc = lnr ? trpl_posterior_weights_lr_dev(dL, dR, S, tf, dW, dSt, ws, (int64_t)wsb, sg.stream())
                     : trpl_posterior_weights_dev(dL, S, tf, dW, dSt, ws, (int64_t)wsb, sg.stream()))
        return rc;
    return sg.finish(seconds);
}

int trpl_posterior_weights(const double *LL, int64_t S, double tf, double *W, double *stats, int32_t device,
                           double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_post_weights(LL, S, tf, W, true)) return rc;
    if (S == 0) return TRPL_OK;
    return weights_staged(LL, nullptr, S, tf, W, stats, device, seconds);
}

int trpl_posterior_weights_lr(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats, int32_t device,
                              double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_post_weights_lr(LL, lnr, S, tf, W)) return rc;
    return weights_staged(LL, lnr, S, tf, W, stats, device, seconds);
}

int trpl_posterior_moments_dev(const double *V, int64_t S, int32_t D, const double *W, const double *mean_in, double *sums,
                               double *central, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (D < 1 || D > 16) return api_fail(TRPL_ERR_ARG, "D=%d must be in [1, 16]", D);
    if (S == 0) return TRPL_OK;
    if (!V || !W || !sums || !central || !workspace) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    if (workspace_bytes < (int64_t)trpl::posterior_workspace_bytes(D)) return api_fail(TRPL_ERR_ARG, "workspace too small");
    hipError_t e = trpl::launch_posterior_moments(V, W, S, D, mean_in, sums, central, (double *)workspace, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "posterior moments launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_posterior_moments(const double *V, int64_t S, int32_t D, const double *W, const double *mean_in, double *sums,
                           double *central, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (D < 1 || D > 16) return api_fail(TRPL_ERR_ARG, "D=%d must be in [1, 16]", D);
    if (!sums || !central) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    memset(sums, 0, sizeof(double) * (2 + D));
    memset(central, 0, sizeof(double) * D * (D + 2));
    if (S == 0) return TRPL_OK;
    if (!V || !W) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const size_t wsb = trpl::posterior_workspace_bytes(D);
    const double *dV = sg.in(V, (size_t)S * D), *dW = sg.in(W, (size_t)S), *dM = mean_in ? sg.in(mean_in, (size_t)D) : nullptr;
    double *dS = sg.out(sums, (size_t)(2 + D)), *dC = sg.out(central, (size_t)D * (D + 2));
    void *ws = sg.scratch(wsb);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_posterior_moments_dev(dV, S, D, dW, dM, dS, dC, ws, (int64_t)wsb, sg.stream())) return rc;
    return sg.finish(seconds);
}

static int check_hist(int64_t S, double xlo, double xhi, int32_t xb, const double *y, double ylo, double yhi, int32_t yb)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (xb < 1 || !(xhi > xlo)) return api_fail(TRPL_ERR_ARG, "x axis needs bins >= 1 and hi > lo");
    if (y && (yb < 1 || !(yhi > ylo))) return api_fail(TRPL_ERR_ARG, "y axis needs bins >= 1 and hi > lo");
    if ((int64_t)xb * (y ? yb : 1) > (1 << 24)) return api_fail(TRPL_ERR_ARG, "too many bins");
    return TRPL_OK;
}

int trpl_posterior_hist_dev(const double *x, const double *y, const double *W, int64_t S, double xlo, double xhi,
                            int32_t xbins, double ylo, double yhi, int32_t ybins, double *out, void *stream)
{
    if (int rc = check_hist(S, xlo, xhi, xbins, y, ylo, yhi, ybins)) return rc;
    if (S == 0) return TRPL_OK;
    if (!x || !out) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    hipError_t e = trpl::launch_posterior_hist(x, y, W, S, xlo, xhi, xbins, ylo, yhi, ybins, out, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "posterior histogram launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_posterior_hist(const double *x, const double *y, const double *W, int64_t S, double xlo, double xhi,
                        int32_t xbins, double ylo, double yhi, int32_t ybins, double *out, int32_t device,
                        double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_hist(S, xlo, xhi, xbins, y, ylo, yhi, ybins)) return rc;
    if (!out) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    const size_t nb = (size_t)xbins * (y ? ybins : 1);
    memset(out, 0, nb * 8);
    if (S == 0) return TRPL_OK;
    if (!x) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const double *dx = sg.in(x, (size_t)S), *dy = y ? sg.in(y, (size_t)S) : nullptr, *dW = W ? sg.in(W, (size_t)S) : nullptr;
    double *dO = sg.inout(out, nb);                              // the kernel adds into it: up as zeros
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_posterior_hist_dev(dx, dy, dW, S, xlo, xhi, xbins, ylo, yhi, ybins, dO, sg.stream())) return rc;
    return sg.finish(seconds);
}

/* ------------------------------------------------------------------ sampler -------------- */
static int check_box(int64_t S, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log)
{
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (ncol < 1 || ncol > 16) return api_fail(TRPL_ERR_ARG, "ncol=%d must be in [1, 16]", ncol);
    if (!lo || !hi || !do_log) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    for (int c = 0; c < ncol; c++) {
        if (!(lo[c] <= hi[c])) return api_fail(TRPL_ERR_ARG, "column %d: lo must be <= hi", c);
        if (do_log[c] && lo[c] != hi[c] && !(lo[c] > 0)) return api_fail(TRPL_ERR_ARG, "column %d: log-uniform needs lo > 0", c);
    }
    return TRPL_OK;
}

int trpl_sample_box_dev(uint32_t seed, int64_t S, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log,
                        uint32_t flags, double *X, void *stream)
{
    if (int rc = check_box(S, ncol, lo, hi, do_log)) return rc;
    if (S == 0) return TRPL_OK;
    if (!X) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    hipError_t e = trpl::launch_sample_box(seed, S, ncol, lo, hi, do_log, flags, X, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "sampler launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_sample_box(uint32_t seed, int64_t S, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log,
                    uint32_t flags, double *X, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check_box(S, ncol, lo, hi, do_log)) return rc;
    if (S == 0) return TRPL_OK;
    if (!X) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    double *dX = sg.out(X, (size_t)S * ncol);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_sample_box_dev(seed, S, ncol, lo, hi, do_log, flags, dX, sg.stream())) return rc;
    return sg.finish(seconds);
}

/* ------------------------------------------------------------------ batched PCR --------- */
int trpl_pcr_solve_batched_dev(const void *ld, const void *d, const void *ud, const void *b, void *x, int64_t S,
                               int32_t L, int32_t elem_bytes, uint32_t flags, void *stream)
{
    if (!pow2(L) || L < 4 || L > 512) return api_fail(TRPL_ERR_ARG, "L=%d must be a power of two in [4, 512]", L);
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes must be 4 or 8");
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (S == 0) return TRPL_OK;
    if (!ld || !d || !ud || !b || !x) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    hipError_t e = (flags & TRPL_FLAG_STRICT)
                       ? trpl::launch_pcr_batched_strict(ld, d, ud, b, x, S, L, elem_bytes, (hipStream_t)stream)
                       : trpl::launch_pcr_batched_fast(ld, d, ud, b, x, S, L, elem_bytes, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail(TRPL_ERR_HIP, "pcr_batched launch: %s", hipGetErrorString(e));
    return TRPL_OK;
}

int trpl_pcr_solve_batched(const void *ld, const void *d, const void *ud, const void *b, void *x, int64_t S,
                           int32_t L, int32_t elem_bytes, uint32_t flags, int32_t device, double *seconds)
{
    if (!pow2(L) || L < 4 || L > 512) return api_fail(TRPL_ERR_ARG, "L=%d must be a power of two in [4, 512]", L);
    if (elem_bytes != 4 && elem_bytes != 8) return api_fail(TRPL_ERR_ARG, "elem_bytes must be 4 or 8");
    if (S < 0) return api_fail(TRPL_ERR_ARG, "S must be >= 0");
    if (seconds) *seconds = 0.0;
    if (S == 0) return TRPL_OK;
    if (!ld || !d || !ud || !b || !x) return api_fail(TRPL_ERR_ARG, "NULL pointer argument");
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    const size_t n = (size_t)S * L * elem_bytes;
    const void *bl = sg.in(ld, n), *bd = sg.in(d, n), *bu = sg.in(ud, n), *bb = sg.in(b, n);
    void *bx = sg.out(x, n);
    if (int rc = sg.begin()) return rc;
    if (int rc = trpl_pcr_solve_batched_dev(bl, bd, bu, bb, bx, S, L, elem_bytes, flags, sg.stream())) return rc;
    return sg.finish(seconds);
}

}  // extern "C"
