// Closed-loop trajectory kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_feedback.hpp"
template int excenv::feedback_entry<excenv::Pendulum>(const excenv::FeedbackCall&);
