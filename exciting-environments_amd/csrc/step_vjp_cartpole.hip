// Reverse-mode step kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_step_vjp.hpp"
namespace excenv {
template <> int step_vjp_entry<CartPole>(const StepVjpCall& sc) { return launch_step_vjp_any<CartPole>(sc); }
}  // namespace excenv
