// The transposed reward of a stored trajectory (excenv_rew_vjp): rew_vjp_kernel for the six models, both element types and both
// forms, in a translation unit of its own. The reward does not read the saturated model's tables: its entry is the linear PMSM's.
#include "kernels_rew_vjp.hpp"
namespace excenv {
template <template <typename> class MT> static int rew_vjp_any(const RewVjpCall& rc) {
  return rc.dtype == EXCENV_F32 ? launch_rew_vjp<MT<float>, float>(rc) : launch_rew_vjp<MT<double>, double>(rc);
}
template <> int rew_vjp_entry<Pendulum>(const RewVjpCall& rc) { return rew_vjp_any<Pendulum>(rc); }
template <> int rew_vjp_entry<MassSpringDamper>(const RewVjpCall& rc) { return rew_vjp_any<MassSpringDamper>(rc); }
template <> int rew_vjp_entry<CartPole>(const RewVjpCall& rc) { return rew_vjp_any<CartPole>(rc); }
template <> int rew_vjp_entry<Acrobot>(const RewVjpCall& rc) { return rew_vjp_any<Acrobot>(rc); }
template <> int rew_vjp_entry<FluidTank>(const RewVjpCall& rc) { return rew_vjp_any<FluidTank>(rc); }
template <> int rew_vjp_entry<Pmsm>(const RewVjpCall& rc) { return rew_vjp_any<Pmsm>(rc); }
template <> int rew_vjp_entry<PmsmSat>(const RewVjpCall& rc) { return rew_vjp_any<Pmsm>(rc); }
}  // namespace excenv
