// Reverse-mode kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_vjp.hpp"
namespace excenv {
template <> int vjp_entry<Pmsm>(const VjpCall& vc) { return launch_vjp_any<Pmsm>(vc); }
template <> int vjp_entry<PmsmSat>(const VjpCall&) {
  set_error("excenv_sim_ahead_vjp: the saturated PMSM (pmsm_lut) has no reverse mode");
  return EXCENV_EUNSUPPORTED;
}
}  // namespace excenv
