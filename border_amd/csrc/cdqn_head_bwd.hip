// The translation unit of the candle DQN's fused head backward (cdqn_head_bwd.hpp): k_cdqn_head_bwd and its launcher.
#define BDR_CDQN_HEAD_BWD_KERNELS
#include "cdqn_head_bwd.hpp"
