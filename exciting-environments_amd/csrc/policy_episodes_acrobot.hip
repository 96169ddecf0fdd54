// Episode rollout kernel instantiations for one environment (its own translation unit so the six compile in parallel).
#include "kernels_policy_episodes.hpp"
template int excenv::policy_episodes_entry<excenv::Acrobot>(const excenv::EpisodeCall&);
