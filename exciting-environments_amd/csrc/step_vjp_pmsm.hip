// Reverse-mode step kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_step_vjp.hpp"
namespace excenv {
template <> int step_vjp_entry<Pmsm>(const StepVjpCall& sc) { return launch_step_vjp_any<Pmsm>(sc); }
template <> int step_vjp_entry<PmsmSat>(const StepVjpCall&) {
  set_error("excenv_step_vjp: the saturated PMSM (pmsm_lut) has no reverse mode");
  return EXCENV_EUNSUPPORTED;
}
}  // namespace excenv
