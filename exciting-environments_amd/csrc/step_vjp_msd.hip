// Reverse-mode step kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_step_vjp.hpp"
template int excenv::step_vjp_entry<excenv::MassSpringDamper>(const excenv::StepVjpCall&);
