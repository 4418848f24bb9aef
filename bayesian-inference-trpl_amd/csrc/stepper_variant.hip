// The one-system fp64 stepper of one line of stepper_variants.hpp: this file is compiled once per (sink, predict, fast | strict)
// beside the plain units stepper_fast.hip / stepper_strict.hip, each time into an object of its own (stepper_moments_predict_strict.o
// ...) with that line's switches -- TRPL_STEPPER_MOMENTS / _WEIGHTED / _CUT, _PREDICT, _STRICT -- and its arithmetic's
// -ffp-contract (Makefile), so the objects of the other variants do not change when one is added.  The kernels are
// trpl::[<sink>::][predict::]stepper_kernel<L, STRICT, false> (stepper_impl.hpp).
#ifndef TRPL_STEPPER_STRICT
#define TRPL_STEPPER_STRICT 0
#endif
#include "stepper_impl.hpp"

namespace trpl {
template <>
hipError_t launch_variant<Variant::TRPL_VARIANT_SINK, TRPL_STEPPER_PREDICT, TRPL_STEPPER_STRICT ? Variant::strict : Variant::fast>(
    const StepArgs &a, hipStream_t stream)
{
    return TRPL_VARIANT_NS launch_stepper<TRPL_STEPPER_STRICT != 0>(a, stream);
}
}  // namespace trpl
