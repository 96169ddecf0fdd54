// Closed-loop reverse-mode kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_feedback_vjp.hpp"
template int excenv::feedback_vjp_entry<excenv::CartPole>(const excenv::FeedbackVjpCall&);
