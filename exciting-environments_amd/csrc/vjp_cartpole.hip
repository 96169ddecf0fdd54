// Reverse-mode kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_vjp.hpp"
namespace excenv {
template <> int vjp_entry<CartPole>(const VjpCall& vc) { return launch_vjp_any<CartPole>(vc); }
}  // namespace excenv
