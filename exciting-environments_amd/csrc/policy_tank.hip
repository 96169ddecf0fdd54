// Policy rollout kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_policy.hpp"
template int excenv::policy_entry<excenv::FluidTank>(const excenv::PolicyCall&);
