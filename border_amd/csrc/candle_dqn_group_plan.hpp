// ================================================================================================
// A group of candle DQN agents (candle_dqn_group.hpp), the part without HIP in it: which agents may form a group, and the launches of
// one update round - kernel, layer, instances and grid for a shape and P members.  The group's host round, bdr_candle_dqn_create (the
// batch and action limits) and tests/test_candle_dqn_group_host.py (compiled with the host compiler alone) read the rule from here.
// The round is the launch sequence Dqn::opt_ (dqn/base.rs:172-189) enqueues for ONE member through CandleDqn::opt / update
// (candle_dqn.hip) - the gather of replay_sample_on_stream, k_cdqn_pack, the L forward layers (the passes (p, obs), (p_tgt, next_obs)
// and - double_dqn - (p, next_obs) are the 2 or 3 instances of one launch per layer), the TD launch, the L - 1 input gradients, the
// grouped weight gradient, reduce + Adam with the soft update riding on it - with the member index as grid dimension y of every launch
// and the network instance of a forward launch as grid dimension z: 2 L + 4 launches whatever P is, 10 at the dqn_cartpole shape.
#pragma once
#include <cstdint>

#include "group_plan_common.hpp"

namespace bdr {

constexpr int CQ_SHAPE_LAYERS = GP_SHAPE_LAYERS;
constexpr int CQ_FORM_MLP = 0, CQ_FORM_ATARI_CNN = 1;   // the Q-network of a candle DQN agent
// the limits bdr_candle_dqn_create accepts (cdqn_check): the TD launch indexes B x Np elements with 32 bits
constexpr int CQ_MAX_BATCH = 65536, CQ_MAX_ACTIONS = 4096;

// ---- what the rule reads of a member ------------------------------------------------------------------------------------------------
using CqNet = GpNet;   // the Q-network (group_plan_common.hpp); activation_out is the Mlp's output activation
// double_dqn decides grid z of the forward launches: 2 or 3 network instances
struct CqShape { int obs_dim, n_actions, batch, double_dqn, form; CqNet net; };
// kind_cdqn: the agent is a candle DQN agent; n_updates: its n_updates_per_opt
struct CqMember { CqShape shape; int kind_cdqn; uint64_t n_updates; int device, prof, grad_comm; const void* agent; };

inline bool cq_same_shape(const CqShape& a, const CqShape& b)
{
    return a.obs_dim == b.obs_dim && a.n_actions == b.n_actions && a.batch == b.batch && (a.double_dqn != 0) == (b.double_dqn != 0) && a.form == b.form &&
           gp_same_net(a.net, b.net);
}
// network instances of a forward launch
inline unsigned cq_instances(const CqShape& s) { return s.double_dqn ? 3u : 2u; }

// why a candle DQN agent of this shape cannot be a member of any group (nullptr: it can)
inline const char* cq_shape_ineligible(const CqShape& s)
{
    if (s.form != CQ_FORM_MLP) return "the AtariCnn Q-network is not grouped: a group steps candle DQN agents in the Mlp form";
    if (s.net.n_layers < 1 || s.net.n_layers > CQ_SHAPE_LAYERS || s.net.n_layers > GP_DW_GROUP || s.net.n_layers > GP_RA_SEGS)
        return "more layers than one grouped weight-gradient launch (16) or one reduce + Adam launch (12 segments) holds";
    if (s.batch < 1 || s.batch > CQ_MAX_BATCH) return "batch size out of range";
    if (s.obs_dim < 1 || s.n_actions < 1 || s.n_actions > CQ_MAX_ACTIONS) return "bad obs dim or number of actions";
    return nullptr;
}

// gather .. dX under GpKernel's numbers, the TD launch behind them, the weight gradient and reduce + Adam last
enum CqKernel { CQ_K_GATHER = GP_K_GATHER, CQ_K_PACK = GP_K_PACK, CQ_K_FWD = GP_K_FWD, CQ_K_DX = GP_K_DX, CQ_K_TD = GP_K_OWN, CQ_K_DW, CQ_K_REDUCE_ADAM, CQ_K_COUNT };
enum CqNetId { CQ_NET_NONE = GP_NET_NONE, CQ_NET_Q = 0 };
inline const char* cq_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "k_cdqn_pack_group", "k_dense_small_members_z<fwd>", "k_dense_small_members_z<dx>",
                                        "k_cdqn_td_group", "k_dense_dw_small_members", "k_cdqn_reduce_adam_group"};
    return k >= 0 && k < CQ_K_COUNT ? names[k] : "?";
}
using CqLaunch = GpLaunch;
constexpr int CQ_MAX_LAUNCHES = 2 * CQ_SHAPE_LAYERS + 4;

// launches of one round, whatever P is
inline int cq_launch_count(int n_layers) { return 2 * n_layers + 4; }
// forward and dX launches of one round: the entries of the dense argument array are (this) x P
inline int cq_dense_launches(int n_layers) { return 2 * n_layers - 1; }
// k_cdqn_pack's grid: one thread per element of [B][obs_dim] (the body does not stride)
inline unsigned cq_pack_grid(const CqShape& s) { return (unsigned)(((uint64_t)s.batch * (uint64_t)s.obs_dim + 255) / 256); }

// The launches of one update round of P members of shape `s`, in stream order; returns their number (0: no group of that shape).
inline int cq_round_plan(const CqShape& s, unsigned P, CqLaunch* out)
{
    if (cq_shape_ineligible(s) || P < 1) return 0;
    GpPlan p{out, 0, s.batch, P, CQ_K_DW, CQ_K_REDUCE_ADAM};
    p.gather(s.obs_dim);
    p.one(CQ_K_PACK, CQ_NET_NONE, -1, cq_pack_grid(s), 256);
    p.fwd(s.net, CQ_NET_Q, cq_instances(s));               // (p, obs), (p_tgt, next_obs) and, double_dqn, (p, next_obs)
    p.one(CQ_K_TD, CQ_NET_Q, -1, 1, 1024);                 // one workgroup per member
    p.step(s.net, CQ_NET_Q, 1, gp_arena_floats(s.net));    // the last reader of the step slot
    return p.n;
}

inline bool cq_grid_ok(const CqLaunch& l) { return gp_grid_ok(l); }

// May these n agents form a group?  CQ_OK: yes.  Otherwise *why says so; the return value is the first member the reason names,
// or CQ_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).
constexpr int CQ_OK = GP_OK, CQ_NO_MEMBER = GP_NO_MEMBER;
inline int cq_group_refusal(const CqMember* m, unsigned n, const char** why, int* kernel = nullptr)
{
    return gp_dense_group_refusal<CQ_MAX_LAUNCHES>(
        m, n, why, kernel, &CqMember::kind_cdqn, "not a candle DQN agent",
        "its shape (obs_dim, n_actions, units and activation_out, batch_size, double_dqn) differs from member 0's: one shape per group",
        cq_shape_ineligible, cq_same_shape, cq_round_plan);
}

}  // namespace bdr
