// Closed-loop trajectory kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_feedback.hpp"
template int excenv::feedback_entry<excenv::Pmsm>(const excenv::FeedbackCall&);
template int excenv::feedback_entry<excenv::PmsmSat>(const excenv::FeedbackCall&);  // the saturated model: tables in global memory
