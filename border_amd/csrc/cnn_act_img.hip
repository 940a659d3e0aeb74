// The translation unit of the AtariCnn candle DQN's acting kernels (cnn_act_img.hpp): k_cnn_act_trunk, k_cnn_act_head, the group entries
// k_cnn_act_trunk_group / k_cnn_act_head_group and their launchers.
#define BDR_CNN_ACT_IMG_KERNELS
#include "cnn_act_img.hpp"
