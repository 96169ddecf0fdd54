// Step Jacobian kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_step_jac.hpp"
namespace excenv {
template <> int step_jac_entry<Pmsm>(const StepJacCall& jc) { return launch_step_jac_any<Pmsm>(jc); }
template <> int step_jac_entry<PmsmSat>(const StepJacCall&) {
  set_error("excenv_step_jacobian: the saturated PMSM (pmsm_lut) has no reverse mode");
  return EXCENV_EUNSUPPORTED;
}
}  // namespace excenv
