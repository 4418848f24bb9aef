// TRPL_FLAG_CUT, FAST: the likelihood-mode stepper whose sink stops a system once its running sse is above
// StepArgs::sse_cut, trpl::cut::stepper_kernel<L, false, ...>.  A translation unit of its own, compiled like
// stepper_fast.hip (-ffp-contract=on): the existing kernels' objects do not change.
#define TRPL_STEPPER_CUT 1
#include "stepper_impl.hpp"

namespace trpl {
hipError_t launch_stepper_cut_fast(const StepArgs &a, hipStream_t stream) { return cut::launch_stepper<false>(a, stream); }
}  // namespace trpl
