// What the units of the ensemble sampler share (mcmc.hip: the symmetric proposals, the Metropolis step with and without a
// Hastings term, tempering, the chain sums; mcmc_hastings.hip: what produces the term, the stretch move and the prior term;
// mcmc_subspace.hip: the subspace differential-evolution proposal): the Philox stream and its call indices, the fold of
// TRPL_MCMC_FOLD, the ladder as a kernel argument, the host checks of the chains and the ladder, the switch over
// the instantiations and the two forms of an entry point.  One definition of each, so a call index is taken once.  All units are
// compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>
#include <utility>

#include "api_util.hpp"
#include "refine_common.hpp"

namespace trpl {
namespace mcmc {

constexpr uint32_t kStream = 0x100;                              // third counter word: 0x100 + j, apart from the draws' j < 8
constexpr uint32_t kPartnerCall = 8, kAcceptCall = 9, kSwapCall = 10, kStretchCall = 11;
// the subspace move (mcmc_subspace.hip): the crossover uniforms c_d are calls 12 + j, the jump-jitter uniforms v_d calls 20 + j (j < 8:
// coordinates 2j and 2j + 1, as the draws' calls), call 28 the class and the number of pairs with the fallback coordinate, call
// 28 + p the partners of pair p = 1 .. TRPL_MCMC_MAX_PAIRS - 1 (pair 0 is kPartnerCall)
constexpr uint32_t kCrossCall = 12, kJumpCall = 20, kSelectCall = 28, kPairCall = 28;

// fold (include/trpl.h, TRPL_MCMC_FOLD): v reflected at the faces of [0, 1] as often as needed.  Called only for a v that failed the
// range test, so the fmod is off the common path; fmod is exact, the add and the subtract round once each.  NaN and +-inf give NaN.
__device__ __forceinline__ double fold_outside(double v)
{
    double r = fmod(v, 2.0);
    if (r < 0.0) r = r + 2.0;
    if (r > 1.0) r = 2.0 - r;
    return r;
}

struct Ladder {                                                  // the temperatures of the rungs, by value like Scale
    double tf[TRPL_MCMC_MAX_RUNGS];
};

}  // namespace mcmc

// "<name> is NULL" for the first pointer of the list that is
static inline int check_not_null(std::initializer_list<std::pair<const char *, const void *>> ptrs)
{
    for (const auto &q : ptrs)
        if (!q.second) return api_fail(TRPL_ERR_ARG, "%s is NULL", q.first);
    return TRPL_OK;
}

static inline int check_count(int64_t count)
{
    if (count < 1) return api_fail(TRPL_ERR_ARG, "count=%lld must be >= 1", (long long)count);
    return refine_check_blocks("count", count, "chains");
}

static inline int check_chains(int64_t count, int32_t A, int64_t chain0)
{
    if (int rc = check_count(count)) return rc;
    if (A < 1 || A > TRPL_REFINE_MAX_DIMS) return api_fail(TRPL_ERR_ARG, "A=%d must be in [1, %d]", A, TRPL_REFINE_MAX_DIMS);
    if (chain0 < 0) return api_fail(TRPL_ERR_ARG, "chain0=%lld must be >= 0", (long long)chain0);
    return TRPL_OK;
}

// the ladder of the *_rungs calls and of the swap: K, group and the K temperatures, copied into the kernel argument
static inline int check_ladder(int32_t K, int64_t group, const double *tf, mcmc::Ladder &lad)
{
    if (K < 1 || K > TRPL_MCMC_MAX_RUNGS) return api_fail(TRPL_ERR_ARG, "K=%d must be in [1, %d]", K, TRPL_MCMC_MAX_RUNGS);
    if (group < 1) return api_fail(TRPL_ERR_ARG, "group=%lld must be >= 1", (long long)group);
    if (int rc = refine_check_blocks("group", group, "chains")) return rc;
    if (!tf) return api_fail(TRPL_ERR_ARG, "tf is NULL");
    for (int k = 0; k < K; k++) {
        if (!(isfinite(tf[k]) && tf[k] > 0.0)) return api_fail(TRPL_ERR_ARG, "tf[%d]=%g must be finite and > 0", k, tf[k]);
        lad.tf[k] = tf[k];
    }
    return TRPL_OK;
}

// TRPL_MCMC_LAUNCH is the switch (A) over kernel<1> .. kernel<16>: its kernel argument names the instantiation by `n`.  A kernel<A>
// is emitted where its launch stands.
#define TRPL_MCMC_CASE(v, ...)                                                                                                         \
    case v: {                                                                                                                          \
        constexpr int n = v;                                                                                                           \
        hipLaunchKernelGGL(__VA_ARGS__);                                                                                               \
    } break;
#define TRPL_MCMC_CASES(...)                                                                                                           \
    TRPL_MCMC_CASE(1, __VA_ARGS__) TRPL_MCMC_CASE(2, __VA_ARGS__) TRPL_MCMC_CASE(3, __VA_ARGS__) TRPL_MCMC_CASE(4, __VA_ARGS__)        \
    TRPL_MCMC_CASE(5, __VA_ARGS__) TRPL_MCMC_CASE(6, __VA_ARGS__) TRPL_MCMC_CASE(7, __VA_ARGS__) TRPL_MCMC_CASE(8, __VA_ARGS__)        \
    TRPL_MCMC_CASE(9, __VA_ARGS__) TRPL_MCMC_CASE(10, __VA_ARGS__) TRPL_MCMC_CASE(11, __VA_ARGS__) TRPL_MCMC_CASE(12, __VA_ARGS__)     \
    TRPL_MCMC_CASE(13, __VA_ARGS__) TRPL_MCMC_CASE(14, __VA_ARGS__) TRPL_MCMC_CASE(15, __VA_ARGS__) TRPL_MCMC_CASE(16, __VA_ARGS__)
#define TRPL_MCMC_LAUNCH(A, kernel, count, ...)                                                                                        \
    switch (A) { TRPL_MCMC_CASES(kernel, dim3(refine_blocks(count)), dim3(refine::kThreads), 0, __VA_ARGS__) }

// ---- the two forms of an entry point on an argument record with check(record &), launch(const record &, stream) and
// stage(record &, Staged &) beside it (found through the record's namespace).  on_stream is a _dev form: every check, then the
// launch on the caller's stream.  staged is a host-buffer form: every check before a device is opened, then the launch of the same
// record on its staged buffers.
template <class Call>
static int on_stream(Call k, void *stream)
{
    if (int rc = check(k)) return rc;
    return launch(k, (hipStream_t)stream);
}

template <class Call>
static int staged(Call k, int32_t device, double *seconds)
{
    if (seconds) *seconds = 0.0;
    if (int rc = check(k)) return rc;
    Staged sg;
    if (int rc = sg.open(device)) return rc;
    stage(k, sg);
    if (int rc = sg.begin()) return rc;
    if (int rc = launch(k, sg.stream())) return rc;
    return sg.finish(seconds);
}

}  // namespace trpl
