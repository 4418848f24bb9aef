// The paired stepper (two L = 128 systems per wavefront, FAST) of one line of stepper_variants.hpp: this file is compiled once per
// (sink, predict) beside the plain unit stepper_pair.hip, each time into an object of its own (stepper_cut_predict_pair.o ...) with
// that line's switches (Makefile) and -ffp-contract=on.  The kernels are trpl::[<sink>::][predict::]pair::stepper_pair_kernel<true,
// false, OPT> (stepper_pair_impl.hpp); only the isolated form is shipped (stepper_pair.hip).
#include "stepper_pair_impl.hpp"

namespace trpl {
template <>
hipError_t launch_variant<Variant::TRPL_VARIANT_SINK, TRPL_STEPPER_PREDICT, Variant::pair>(const StepArgs &a, hipStream_t stream)
{
    return TRPL_VARIANT_NS launch_stepper_pair_t<true>(a, stream);
}
}  // namespace trpl
