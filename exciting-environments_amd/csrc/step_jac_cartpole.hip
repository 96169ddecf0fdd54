// Step Jacobian kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_step_jac.hpp"
template int excenv::step_jac_entry<excenv::CartPole>(const excenv::StepJacCall&);
