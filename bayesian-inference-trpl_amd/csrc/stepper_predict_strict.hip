// TRPL_FLAG_PREDICT, STRICT arithmetic: the one-system stepper with the extrapolated start of every time step,
// trpl::predict::stepper_kernel<L, true, SNAP, false, false, false>, compiled like stepper_strict.hip
// (-ffp-contract=off).  The start is no longer the reference's, so neither is the iteration path: what STRICT keeps
// here is its arithmetic (IEEE divides, the reference's operation order) -- the yardstick of FAST + predict.
#define TRPL_STEPPER_PREDICT 1
#include "stepper_impl.hpp"

namespace trpl {
hipError_t launch_stepper_predict_strict(const StepArgs &a, hipStream_t stream) { return predict::launch_stepper<true>(a, stream); }
}  // namespace trpl
