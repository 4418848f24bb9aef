// TRPL_FLAG_WEIGHTED, STRICT: the likelihood-mode stepper whose sink emits sse = sum w_i e_i^2 and esum = sum w_i e_i,
// trpl::weighted::stepper_kernel<L, true, ...>.  A translation unit of its own, compiled like
// stepper_strict.hip (-ffp-contract=off): the existing kernels' objects do not change.
#define TRPL_STEPPER_WEIGHTED 1
#include "stepper_impl.hpp"

namespace trpl {
hipError_t launch_stepper_weighted_strict(const StepArgs &a, hipStream_t stream) { return weighted::launch_stepper<true>(a, stream); }
}  // namespace trpl
