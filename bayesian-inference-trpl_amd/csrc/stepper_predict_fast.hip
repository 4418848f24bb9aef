// TRPL_FLAG_PREDICT, FAST arithmetic: the one-system stepper with the extrapolated start of every time step,
// trpl::predict::stepper_kernel<L, false, SNAP, false, false, false>.  A translation unit of its own, compiled like
// stepper_fast.hip (-ffp-contract=on): the default kernels' machine code does not depend on the mode's existence.
#define TRPL_STEPPER_PREDICT 1
#include "stepper_impl.hpp"

namespace trpl {
hipError_t launch_stepper_predict_fast(const StepArgs &a, hipStream_t stream) { return predict::launch_stepper<false>(a, stream); }
}  // namespace trpl
