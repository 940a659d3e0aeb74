// ================================================================================================
// A group of candle DQN agents in the AtariCnn form (candle_dqn_cnn_group.hpp), the part without HIP in it: which agents may form a
// group, and the launches of one update round - kernel, layer, instances and grid for a shape and P members.
// The round is the launch sequence Dqn::opt_ (dqn/base.rs:172-189) enqueues for ONE member through CandleDqnCnn::opt / update_cnn
// (candle_dqn.hip): the gather of u8 rows of 84 * 84 * n_stack bytes; conv1, conv2 and conv3 forward with the passes (p, obs),
// (p_tgt, next_obs) and - double_dqn - (p, next_obs) as the instances of one launch per layer; l1 and l2 forward; the TD launch; l2's
// input gradient; l1's input gradient into dy3 under conv3's ReLU mask; the head's grouped dW; the head's reduce + Adam; conv3 dW,
// conv3 dX, conv2 dW, conv2 dX, conv1 dW; the conv reduce + Adam, the last reader of the step slot: CQC_LAUNCHES = 17 whatever P is.
// The member is grid dimension y of every launch, the instance of a conv2 / conv3 / head forward grid dimension z, and x the member's
// own grid: conv1's workgroups of all instances (conv1_forward's rule, instance = x % nz), (M + 63) / 64 row tiles, conv_dw_plan's
// wgs * chunks, and - the input gradients, whose own grid is (tiles, positions) - tiles * positions with the position as x / tiles, so
// that the long position classes are still dispatched first.
// The Mlp form's rule (candle_dqn_group_plan.hpp, cq_*) is untouched: that group keeps refusing an AtariCnn member by name.
#pragma once
#include <cstdint>

#include "conv_layout.hpp"
#include "group_plan_common.hpp"

namespace bdr {

constexpr int CQC_LAUNCHES = 17, CQC_MAX_LAUNCHES = CQC_LAUNCHES;
constexpr int CQC_MAX_STACK = 6;        // conv1's staged-image forward (conv1_bf16_img.hpp: C1IMG_MAX_STACK), the form with a member entry
constexpr int CQC_MAX_BATCH = 65536, CQC_MAX_ACTIONS = 4096;   // bdr_candle_dqn_cnn_create's limits (cdqn_check)
constexpr int CQC_CUS = 256;            // conv1_forward's default

// obs_dim: the u8 row of 84 * 84 * n_stack bytes in 4-byte words (what the gather's grid is computed from); net: the head [3136 -> 512 -> A]
struct CqcShape { int obs_dim, n_stack, n_actions, batch, double_dqn, dxc3_kloop; GpNet net; };
// kind_cdqn_cnn: the agent is a candle DQN agent with the AtariCnn Q-network; n_updates: its n_updates_per_opt
// split_arith: it was switched to BDR_ARITH_BF16X3_6 (bdr_candle_dqn_cnn_set_arithmetic)
// head_splitk: it was switched to BDR_HEAD_FORM_SPLITK (bdr_candle_dqn_cnn_set_head_form)
// head_bwd_fused: it was switched to BDR_HEAD_BWD_FUSED (bdr_candle_dqn_cnn_set_head_bwd_form)
struct CqcMember { CqcShape shape; int kind_cdqn_cnn; uint64_t n_updates; int device, prof, grad_comm; const void* agent; int split_arith, head_splitk, head_bwd_fused; };

inline bool cqc_same_shape(const CqcShape& a, const CqcShape& b)
{
    return a.n_stack == b.n_stack && a.n_actions == b.n_actions && a.batch == b.batch && (a.double_dqn != 0) == (b.double_dqn != 0) && gp_same_net(a.net, b.net);
}
inline unsigned cqc_instances(const CqcShape& s) { return s.double_dqn ? 3u : 2u; }

// why an AtariCnn candle DQN agent of this shape cannot be a member of any group (nullptr: it can)
inline const char* cqc_shape_ineligible(const CqcShape& s)
{
    if (s.n_stack < 1 || s.n_stack > CQC_MAX_STACK) return "n_stack beyond 6: conv1's direct forward has no member entry (the staged-image form serves n_stack 1 .. 6)";
    if (s.net.n_layers != 2) return "the AtariCnn head has two layers (l1, l2)";
    if (s.batch < 1 || s.batch > CQC_MAX_BATCH) return "batch size out of range";
    if (s.n_actions < 1 || s.n_actions > CQC_MAX_ACTIONS || s.obs_dim != 1764 * s.n_stack) return "bad number of actions or row width";
    return nullptr;
}

// gather, forward and dX under GpKernel's numbers, the kind's own launches behind them, the head's weight gradient and reduce + Adam last
enum CqcKernel {
    CQC_K_GATHER = GP_K_GATHER, CQC_K_PACK = GP_K_PACK /* (no pack launch: the trunk reads the gathered u8 rows) */, CQC_K_FWD = GP_K_FWD, CQC_K_DX = GP_K_DX,
    CQC_K_CONV1_FWD = GP_K_OWN, CQC_K_CONV2_FWD, CQC_K_CONV3_FWD, CQC_K_TD, CQC_K_CONV3_DW, CQC_K_CONV3_DX, CQC_K_CONV2_DW, CQC_K_CONV2_DX, CQC_K_CONV1_DW,
    CQC_K_CONV_REDUCE_ADAM, CQC_K_DW, CQC_K_REDUCE_ADAM, CQC_K_COUNT
};
enum CqcNetId { CQC_NET_NONE = GP_NET_NONE, CQC_NET_Q = 0 };
inline const char* cqc_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "-", "k_dense_small_members_z<fwd>", "k_dense_small_members_z<dx>", "k_conv1_img_members",
                                        "k_igemm_members<FwdC2>", "k_igemm_members<FwdC3>", "k_cdqn_td_group", "k_igemm_red_members<DwC3>",
                                        "k_igemm_members<DxC3Pos>", "k_igemm_red_members<DwC2>", "k_igemm_members<DxC2MPos>", "k_conv1_dw_members",
                                        "k_cdqn_conv_reduce_adam_group", "k_dense_dw_small_members", "k_cdqn_head_reduce_adam_group"};
    return k >= 0 && k < CQC_K_COUNT ? names[k] : "?";
}
using CqcLaunch = GpLaunch;

inline int cqc_launch_count() { return CQC_LAUNCHES; }
// forward and dX launches of the head: l1, l2, l2's dX, l1's dX into dy3
inline int cqc_dense_launches() { return 4; }
// conv1_forward's rule (conv1_bf16_img.hpp) for the staged-image form: images per workgroup pass and workgroups per instance
inline int cqc_conv1_ipw(const CqcShape& s)
{
    const int per_inst = std::max(1, CQC_CUS / (int)cqc_instances(s));
    return (s.n_stack <= 4 && s.batch > per_inst) ? 2 : 1;
}
inline unsigned cqc_conv1_grid(const CqcShape& s)
{
    const int nz = (int)cqc_instances(s), per_inst = std::max(1, CQC_CUS / nz), ipw = cqc_conv1_ipw(s);
    return (unsigned)(std::max(1, std::min(per_inst, (s.batch + ipw - 1) / ipw)) * nz);
}
// tiles along x of the position-class input gradients (cnn_layers.hpp: dxc3_pos_grid, dxc2_pos_grid): 64 images per tile; conv3 has one
// 64-column tile and 81 positions, conv2's merged classes two and 100 positions
constexpr unsigned CQC_DXC3_POS = 81, CQC_DXC2_POS = 100;
inline unsigned cqc_dxc3_tiles(int batch) { return (unsigned)((batch + 63) / 64); }
inline unsigned cqc_dxc2_tiles(int batch) { return (unsigned)((batch + 63) / 64) * 2; }
// the conv weight gradients: conv_dw_plan's workgroups per chunk x chunks of this batch (layer 0 conv1, 1 conv2, 2 conv3)
inline unsigned cqc_conv_dw_grid(const CqcShape& s, int layer)
{
    const ConvDwLayer l = conv_dw_plan(make_arena(1, s.n_stack), s.batch).layer[layer];
    return (unsigned)(l.wgs * l.chunks(s.batch));
}
inline uint64_t cqc_conv_floats(int n_stack) { return make_arena(1, n_stack).w4; }

// The launches of one update round of P members of shape `s`, in stream order; returns their number (0: no group of that shape).
inline int cqc_round_plan(const CqcShape& s, unsigned P, CqcLaunch* out)
{
    if (cqc_shape_ineligible(s) || P < 1) return 0;
    const unsigned nz = cqc_instances(s), B = (unsigned)s.batch;
    GpPlan p{out, 0, s.batch, P, CQC_K_DW, CQC_K_REDUCE_ADAM};
    p.gather(s.obs_dim);
    p.one(CQC_K_CONV1_FWD, CQC_NET_NONE, -1, cqc_conv1_grid(s), 512);                               // the instance is x % nz
    out[p.n++] = GpLaunch{CQC_K_CONV2_FWD, CQC_NET_NONE, -1, (B * 81 + 63) / 64, P, nz, 256};
    out[p.n++] = GpLaunch{CQC_K_CONV3_FWD, CQC_NET_NONE, -1, (B * 49 + 63) / 64, P, nz, 256};
    p.fwd(s.net, CQC_NET_Q, nz);                                                                    // l1, l2
    p.one(CQC_K_TD, CQC_NET_Q, -1, 1, 1024);                                                        // one workgroup per member
    p.dx(s.net, CQC_NET_Q, 1, 0);                                                                   // l2's dX, then l1's into dy3 (dx0 / mask0)
    out[p.n++] = GpLaunch{CQC_K_DW, CQC_NET_Q, -1, gp_dw_tiles(s.net, s.batch), P, 1, 256};
    out[p.n++] = GpLaunch{CQC_K_REDUCE_ADAM, CQC_NET_Q, -1, (unsigned)((gp_arena_floats(s.net) / 4 + 255) / 256), P, 1, 256};
    p.one(CQC_K_CONV3_DW, CQC_NET_NONE, -1, cqc_conv_dw_grid(s, 2), 256);
    p.one(CQC_K_CONV3_DX, CQC_NET_NONE, -1, cqc_dxc3_tiles(s.batch) * CQC_DXC3_POS, 512);           // two teams of four waves
    p.one(CQC_K_CONV2_DW, CQC_NET_NONE, -1, cqc_conv_dw_grid(s, 1), 256);
    p.one(CQC_K_CONV2_DX, CQC_NET_NONE, -1, cqc_dxc2_tiles(s.batch) * CQC_DXC2_POS, 256);
    p.one(CQC_K_CONV1_DW, CQC_NET_NONE, -1, cqc_conv_dw_grid(s, 0), 512);
    p.one(CQC_K_CONV_REDUCE_ADAM, CQC_NET_NONE, -1, (unsigned)((cqc_conv_floats(s.n_stack) / 4 + 31) / 32), 256);   // the last reader of the step slot
    return p.n;
}

// May these n agents form a group?  CQC_OK: yes.  Otherwise *why says so; the return value is the first member the reason names, or
// CQC_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).
constexpr int CQC_OK = GP_OK, CQC_NO_MEMBER = GP_NO_MEMBER;
inline int cqc_group_refusal(const CqcMember* m, unsigned n, const char** why, int* kernel = nullptr)
{
    const auto own = [&](const CqcMember& x) -> const char* {
        if (!x.kind_cdqn_cnn) return "not a candle DQN agent with the AtariCnn Q-network (agents in the Mlp form make a candle DQN group)";
        if (x.split_arith) return "its arithmetic is BDR_ARITH_BF16X3_6: the grouped round is built for BDR_ARITH_F32_EXACT members (conv2 / conv3 on the FP32 MFMA)";
        if (x.head_splitk) return "its head form is BDR_HEAD_FORM_SPLITK: the grouped round is built for BDR_HEAD_FORM_LAYERS members (l1 and l2 as two grouped launches)";
        if (x.head_bwd_fused) return "its head backward form is BDR_HEAD_BWD_FUSED: the grouped round is built for BDR_HEAD_BWD_LAYERS members (the head's dX and dW as grouped launches)";
        if (const char* w = cqc_shape_ineligible(x.shape)) return w;
        if (!cqc_same_shape(x.shape, m[0].shape)) return "its shape (n_stack, n_actions, batch_size, double_dqn) differs from member 0's: one shape per group";
        if (x.n_updates != 1) return "n_updates_per_opt != 1 is not built for a group";
        if ((x.shape.dxc3_kloop != 0) != (m[0].shape.dxc3_kloop != 0)) return "its dxc3_kloop differs from member 0's: one form of conv3's input gradient per group";
        return nullptr;
    };
    return gp_group_refusal<GpLaunch, CQC_MAX_LAUNCHES>(m, n, why, kernel, own, [&](GpLaunch* out) { return cqc_round_plan(m[0].shape, n, out); });
}

}  // namespace bdr
