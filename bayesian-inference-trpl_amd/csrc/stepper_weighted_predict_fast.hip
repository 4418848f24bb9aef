// TRPL_FLAG_WEIGHTED, FAST with TRPL_FLAG_PREDICT: the likelihood-mode stepper whose sink emits sse = sum w_i e_i^2 and esum = sum w_i e_i,
// trpl::weighted::predict::stepper_kernel<L, false, ...>.  A translation unit of its own, compiled like
// stepper_predict_fast.hip (-ffp-contract=on): the existing kernels' objects do not change.
#define TRPL_STEPPER_WEIGHTED 1
#define TRPL_STEPPER_PREDICT 1
#include "stepper_impl.hpp"

namespace trpl {
hipError_t launch_stepper_weighted_predict_fast(const StepArgs &a, hipStream_t stream) { return weighted::predict::launch_stepper<false>(a, stream); }
}  // namespace trpl
