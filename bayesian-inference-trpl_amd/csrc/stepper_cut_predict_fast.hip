// TRPL_FLAG_CUT, FAST with TRPL_FLAG_PREDICT: the likelihood-mode stepper whose sink stops a system once its running sse is above
// StepArgs::sse_cut, trpl::cut::predict::stepper_kernel<L, false, ...>.  A translation unit of its own, compiled like
// stepper_predict_fast.hip (-ffp-contract=on): the existing kernels' objects do not change.
#define TRPL_STEPPER_CUT 1
#define TRPL_STEPPER_PREDICT 1
#include "stepper_impl.hpp"

namespace trpl {
hipError_t launch_stepper_cut_predict_fast(const StepArgs &a, hipStream_t stream) { return cut::predict::launch_stepper<false>(a, stream); }
}  // namespace trpl
