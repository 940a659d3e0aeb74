// The translation unit of the candle DQN's split-k head forward (cdqn_head_fwd.hpp): k_cdqn_head_fwd and its launcher.
#define BDR_CDQN_HEAD_FWD_KERNELS
#include "cdqn_head_fwd.hpp"
