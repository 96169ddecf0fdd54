// Reverse-mode kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_vjp.hpp"
template int excenv::vjp_entry<excenv::FluidTank>(const excenv::VjpCall&);
