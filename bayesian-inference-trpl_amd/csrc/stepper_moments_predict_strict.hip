// TRPL_FLAG_MOMENTS, STRICT with TRPL_FLAG_PREDICT: the likelihood-mode stepper whose sink emits esum = sum e_i beside sse = sum e_i^2,
// trpl::moments::predict::stepper_kernel<L, true, ...>.  A translation unit of its own, compiled like
// stepper_predict_strict.hip (-ffp-contract=off): the existing kernels' objects do not change.
#define TRPL_STEPPER_MOMENTS 1
#define TRPL_STEPPER_PREDICT 1
#include "stepper_impl.hpp"

namespace trpl {
hipError_t launch_stepper_moments_predict_strict(const StepArgs &a, hipStream_t stream) { return moments::predict::launch_stepper<true>(a, stream); }
}  // namespace trpl
