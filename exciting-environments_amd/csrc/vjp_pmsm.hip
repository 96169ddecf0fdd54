// Reverse-mode kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_vjp.hpp"
template int excenv::vjp_entry<excenv::Pmsm>(const excenv::VjpCall&);
template int excenv::vjp_entry<excenv::PmsmSat>(const excenv::VjpCall&);  // the refusal: no kernel
