// TRPL_FLAG_PREDICT on the two-systems-per-wavefront stepper (L = 128, FAST, isolated; optimistic seam, or the
// always-voiding one under TRPL_FLAG_PAIR_ALWAYS_SEAM): trpl::predict::pair::stepper_pair_kernel<true, SNAP, OPT>.
// Compiled like stepper_pair.hip (-ffp-contract=on).
#define TRPL_STEPPER_PREDICT 1
#include "stepper_pair_impl.hpp"

namespace trpl {
hipError_t launch_stepper_pair_predict(const StepArgs &a, hipStream_t stream) { return predict::launch_stepper_pair_t<true>(a, stream); }
}  // namespace trpl
