// Policy reverse-mode kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_policy_vjp.hpp"
template int excenv::policy_vjp_entry<excenv::Pendulum>(const excenv::PolicyVjpCall&);
