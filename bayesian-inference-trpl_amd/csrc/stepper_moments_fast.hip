// TRPL_FLAG_MOMENTS, FAST: the likelihood-mode stepper whose sink emits esum = sum e_i beside sse = sum e_i^2,
// trpl::moments::stepper_kernel<L, false, ...>.  A translation unit of its own, compiled like
// stepper_fast.hip (-ffp-contract=on): the existing kernels' objects do not change.
#define TRPL_STEPPER_MOMENTS 1
#include "stepper_impl.hpp"

namespace trpl {
hipError_t launch_stepper_moments_fast(const StepArgs &a, hipStream_t stream) { return moments::launch_stepper<false>(a, stream); }
}  // namespace trpl
