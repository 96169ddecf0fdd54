// Step Jacobian kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_step_jac.hpp"
namespace excenv {
template <> int step_jac_entry<CartPole>(const StepJacCall& jc) { return launch_step_jac_any<CartPole>(jc); }
}  // namespace excenv
