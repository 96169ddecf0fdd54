// The transposed reward of a stored trajectory (excenv_rew_vjp): rew_vjp_kernel for the six models, both element types and both
// forms, in a translation unit of its own.
#include "kernels_rew_vjp.hpp"
template int excenv::rew_vjp_entry<excenv::Pendulum>(const excenv::RewVjpCall&);
template int excenv::rew_vjp_entry<excenv::MassSpringDamper>(const excenv::RewVjpCall&);
template int excenv::rew_vjp_entry<excenv::CartPole>(const excenv::RewVjpCall&);
template int excenv::rew_vjp_entry<excenv::Acrobot>(const excenv::RewVjpCall&);
template int excenv::rew_vjp_entry<excenv::FluidTank>(const excenv::RewVjpCall&);
template int excenv::rew_vjp_entry<excenv::Pmsm>(const excenv::RewVjpCall&);
template int excenv::rew_vjp_entry<excenv::PmsmSat>(const excenv::RewVjpCall&);
