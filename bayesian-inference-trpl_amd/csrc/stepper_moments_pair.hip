// TRPL_FLAG_MOMENTS, FAST, two systems per wavefront: the likelihood-mode stepper whose sink emits esum = sum e_i beside sse = sum e_i^2,
// trpl::moments::pair::stepper_pair_kernel<true, false, OPT>.  A translation unit of its own, compiled like
// stepper_pair.hip (-ffp-contract=on): the existing kernels' objects do not change.
#define TRPL_STEPPER_MOMENTS 1
#include "stepper_pair_impl.hpp"

namespace trpl {
hipError_t launch_stepper_moments_pair(const StepArgs &a, hipStream_t stream) { return moments::launch_stepper_pair_t<true>(a, stream); }
}  // namespace trpl
