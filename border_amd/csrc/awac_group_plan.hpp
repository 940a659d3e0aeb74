// ================================================================================================
// A group of AWAC agents (awac_group.hpp), the part without HIP in it: which agents may form a group, and the launches of one update
// round - kernel, network, layer, instances and grid for a shape and P members.  The group's host round and
// tests/test_awac_group_host.py (compiled with the host compiler alone) read the rule from here.
// The round is the launch sequence Awac::opt_ (awac/base.rs:170-215) enqueues for ONE member through Awac::update (awac.hip) - the
// gather of replay_sample_on_stream, pack, the actor on obs, the sample of act_, the online critics on (obs | act) and (obs | act_),
// the actor loss and the actor's step, the UPDATED actor on next_obs, the sample of next_act, the target critics on
// (next_obs | next_act), the critic loss and the critics' step with the soft update - with the member index as grid dimension y of
// every launch and the network instance, where the standalone launch has one, as grid dimension z.  With Lp, Lq the layer counts of
// actor and critic: 3 (Lp + Lq) + 8 launches whatever P is.
#pragma once
#include <cstdint>

#include "group_plan_common.hpp"

namespace bdr {

constexpr int AG_SHAPE_LAYERS = GP_SHAPE_LAYERS;
constexpr int AG_DW_GROUP = 16;     // jobs of one grouped weight-gradient launch (dense.hpp DW_GROUP)
constexpr int AG_RA_SEGS = 12;      // segments of k_dense_reduce_adam (dense.hpp RA_SEGS)
constexpr int AG_MAXZ = 4;          // instances of one dense launch (dense.hpp DenseArgsZ, RA_INST)
constexpr unsigned AG_MAX_MEMBERS = GP_MAX_MEMBERS;

// ---- what the rule reads of a member ------------------------------------------------------------------------------------------------
using AgNet = GpNet;   // one network (group_plan_common.hpp)
struct AgShape { int obs_dim, act_dim, batch, n_critics; AgNet critic, actor; };
// kind_awac: the agent is an AWAC agent; n_updates: its n_updates_per_opt
struct AgMember { AgShape shape; int kind_awac; uint64_t n_updates; int device, prof, grad_comm; const void* agent; };

inline bool ag_same_shape(const AgShape& a, const AgShape& b)
{
    return a.obs_dim == b.obs_dim && a.act_dim == b.act_dim && a.batch == b.batch && a.n_critics == b.n_critics && gp_same_net(a.critic, b.critic) &&
           gp_same_net(a.actor, b.actor);
}

// why an AWAC agent of this shape cannot be a member of any group (nullptr: it can)
inline const char* ag_shape_ineligible(const AgShape& s)
{
    for (const AgNet* n : {&s.critic, &s.actor})
        if (n->n_layers < 1 || n->n_layers > AG_SHAPE_LAYERS) return "a network has no layer, or more than 16";
    if (s.n_critics < 1) return "n_critics must be positive";
    if (2 * s.n_critics > AG_MAXZ)
        return "n_critics > 2: the online critics on (obs | act) and on (obs | act_) run as the 2 n_critics instances of one launch per layer, and a launch holds four";
    if (s.n_critics * s.critic.n_layers > AG_DW_GROUP) return "n_critics x critic layers beyond the 16 jobs of one grouped weight-gradient launch";
    if (s.critic.n_layers > AG_RA_SEGS || s.actor.n_layers + 1 > AG_RA_SEGS)
        return "more layers than one reduce + Adam launch has segments (12; the actor's head2 is one more)";
    if (s.batch < 2 || s.batch > 65536) return "batch size out of range (AWAC needs at least 2 rows)";
    if (s.obs_dim < 1 || s.act_dim < 1) return "bad obs/act dims";
    return nullptr;
}

enum AgKernel { AG_K_GATHER = 0, AG_K_PACK, AG_K_FWD, AG_K_DX, AG_K_SAMPLE, AG_K_ACTOR_LOSS, AG_K_CRITIC_LOSS, AG_K_DW, AG_K_REDUCE_ADAM, AG_K_COUNT };
enum AgNetId { AG_NET_NONE = -1, AG_NET_ACTOR = 0, AG_NET_CRITIC = 1 };
inline const char* ag_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "k_awac_pack_group", "k_dense_small_members_z<fwd>", "k_dense_small_members_z<dx>", "k_awac_sample_group",
                                        "k_awac_actor_loss_group", "k_awac_critic_loss_group", "k_dense_dw_small_members", "k_awac_reduce_adam_group"};
    return k >= 0 && k < AG_K_COUNT ? names[k] : "?";
}
// net: the network a dense / dW / reduce / loss launch serves (AgNetId), layer: the layer a forward / dX launch serves, the draw (0:
// act_, 1: next_act) of a sample launch, else -1; gz = the instances nz of the launch
struct AgLaunch { int kernel, net, layer; unsigned gx, gy, gz, threads; };
constexpr int AG_MAX_LAUNCHES = 6 * AG_SHAPE_LAYERS + 8;

// launches of one round, whatever P is
inline int ag_launch_count(int Lq, int Lp) { return 3 * (Lp + Lq) + 8; }
// forward and dX launches of one round: the entries of the dense argument array are (this) x P
inline int ag_dense_launches(int Lq, int Lp) { return 3 * (Lp + Lq) - 2; }
// k_awac_pack's grid (Awac::update): one thread per element of [B][obs + act], at most 2048 workgroups (the body strides by the grid)
inline unsigned ag_pack_grid(const AgShape& s)
{
    const uint64_t g = ((uint64_t)s.batch * (uint64_t)(s.obs_dim + s.act_dim) + 255) / 256;
    return (unsigned)(g < 2048 ? g : 2048);
}
// k_candle_sample's grid (CandleAgent::sample_pack): one thread per element of [B][act]
inline unsigned ag_sample_grid(const AgShape& s) { return (unsigned)(((uint64_t)s.batch * (uint64_t)s.act_dim + 255) / 256); }

// The launches of one update round of P members of shape `s`, in stream order; returns their number (0: no group of that shape).
// x is the member's own grid everywhere, y the member, z the network instance.
inline int ag_round_plan(const AgShape& s, unsigned P, AgLaunch* out)
{
    if (ag_shape_ineligible(s) || P < 1) return 0;
    const int B = s.batch, NC = s.n_critics;
    const unsigned RB = (unsigned)((B + 31) / 32);
    int n = 0;
    const auto fwd = [&](const AgNet& net, int id, unsigned nz) {
        for (int i = 0; i < net.n_layers; ++i) out[n++] = AgLaunch{AG_K_FWD, id, i, RB * (unsigned)(net.Np[i] / 32), P, nz, 256};
    };
    // mlp_backward_step: the input gradients down to layer 1, the grouped weight gradient, reduce + Adam over `arena` floats
    const auto step = [&](const AgNet& net, int id, unsigned nz, uint64_t arena) {
        for (int i = net.n_layers - 1; i > 0; --i) out[n++] = AgLaunch{AG_K_DX, id, i, RB * (unsigned)(net.Kp[i] / 32), P, nz, 256};
        out[n++] = AgLaunch{AG_K_DW, id, -1, nz * gp_dw_tiles(net, B), P, 1, 256};
        out[n++] = AgLaunch{AG_K_REDUCE_ADAM, id, -1, (unsigned)((arena / 4 + 255) / 256), P, nz, 256};
    };
    out[n++] = AgLaunch{AG_K_GATHER, AG_NET_NONE, -1, (unsigned)B * gp_gather_chunks((uint64_t)s.obs_dim * 4), P, 1, 256};
    out[n++] = AgLaunch{AG_K_PACK, AG_NET_NONE, -1, ag_pack_grid(s), P, 1, 256};
    // ---- update_actor
    fwd(s.actor, AG_NET_ACTOR, 1);                                                          // the actor on obs
    out[n++] = AgLaunch{AG_K_SAMPLE, AG_NET_ACTOR, 0, ag_sample_grid(s), P, 1, 256};        // act_
    fwd(s.critic, AG_NET_CRITIC, 2u * (unsigned)NC);                                        // the online critics on (obs | act) and (obs | act_)
    out[n++] = AgLaunch{AG_K_ACTOR_LOSS, AG_NET_ACTOR, -1, (unsigned)s.act_dim + 1, P, 1, 1024};
    step(s.actor, AG_NET_ACTOR, 1, gp_arena_floats(s.actor) + (uint64_t)((s.act_dim + 63) / 64 * 64));   // head2 behind the layers
    // ---- update_critic
    fwd(s.actor, AG_NET_ACTOR, 1);                                                          // the updated actor on next_obs
    out[n++] = AgLaunch{AG_K_SAMPLE, AG_NET_ACTOR, 1, ag_sample_grid(s), P, 1, 256};        // next_act
    fwd(s.critic, AG_NET_CRITIC, (unsigned)NC);                                             // the target critics on (next_obs | next_act)
    out[n++] = AgLaunch{AG_K_CRITIC_LOSS, AG_NET_CRITIC, -1, 1, P, 1, 1024};
    step(s.critic, AG_NET_CRITIC, (unsigned)NC, gp_arena_floats(s.critic));                 // the last reader of the step slot
    return n;
}

inline bool ag_grid_ok(const AgLaunch& l) { return gp_grid_ok(l); }

// May these n agents form a group?  AG_OK: yes.  Otherwise *why says so; the return value is the first member the reason names,
// or AG_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).
constexpr int AG_OK = GP_OK, AG_NO_MEMBER = GP_NO_MEMBER;
inline int ag_group_refusal(const AgMember* m, unsigned n, const char** why, int* kernel = nullptr)
{
    const auto own = [&](const AgMember& x) -> const char* {
        if (!x.kind_awac) return "not an AWAC agent";
        if (const char* w = ag_shape_ineligible(x.shape)) return w;
        if (!ag_same_shape(x.shape, m[0].shape))
            return "its shape (obs_dim, act_dim, both networks' units and activation_out, n_critics, batch_size) differs from member 0's: one shape per group";
        if (x.n_updates != 1) return "n_updates_per_opt != 1 is not built for a group";
        return nullptr;
    };
    return gp_group_refusal<AgLaunch, AG_MAX_LAUNCHES>(m, n, why, kernel, own, [&](AgLaunch* out) { return ag_round_plan(m[0].shape, n, out); });
}

}  // namespace bdr
