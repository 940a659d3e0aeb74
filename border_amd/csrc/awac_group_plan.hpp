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
    GpShapeOwn own{};
    own.two_nc = "n_critics > 2: the online critics on (obs | act) and on (obs | act_) run as the 2 n_critics instances of one launch per layer, and a launch holds four";
    if (s.critic.n_layers > GP_RA_SEGS || s.actor.n_layers + 1 > GP_RA_SEGS)
        own.segs = "more layers than one reduce + Adam launch has segments (12; the actor's head2 is one more)";
    if (s.batch < 2 || s.batch > 65536) own.batch = "batch size out of range (AWAC needs at least 2 rows)";
    return gp_shape_ineligible({&s.critic, &s.actor}, s.n_critics, s.critic.n_layers, s.obs_dim, s.act_dim, own);
}

// gather .. dX under GpKernel's numbers, AWAC's own behind them, the weight gradient and reduce + Adam last
enum AgKernel {
    AG_K_GATHER = GP_K_GATHER, AG_K_PACK = GP_K_PACK, AG_K_FWD = GP_K_FWD, AG_K_DX = GP_K_DX,
    AG_K_SAMPLE = GP_K_OWN, AG_K_ACTOR_LOSS, AG_K_CRITIC_LOSS, AG_K_DW, AG_K_REDUCE_ADAM, AG_K_COUNT
};
enum AgNetId { AG_NET_NONE = GP_NET_NONE, AG_NET_ACTOR = 0, AG_NET_CRITIC = 1 };
inline const char* ag_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "k_awac_pack_group", "k_dense_small_members_z<fwd>", "k_dense_small_members_z<dx>", "k_awac_sample_group",
                                        "k_awac_actor_loss_group", "k_awac_critic_loss_group", "k_dense_dw_small_members", "k_awac_reduce_adam_group"};
    return k >= 0 && k < AG_K_COUNT ? names[k] : "?";
}
using AgLaunch = GpLaunch;   // net: AgNetId; layer of a sample launch: the draw (0: act_, 1: next_act)
constexpr int AG_MAX_LAUNCHES = 6 * AG_SHAPE_LAYERS + 8;

// launches of one round, whatever P is
inline int ag_launch_count(int Lq, int Lp) { return 3 * (Lp + Lq) + 8; }
// forward and dX launches of one round: the entries of the dense argument array are (this) x P
inline int ag_dense_launches(int Lq, int Lp) { return 3 * (Lp + Lq) - 2; }
// k_candle_sample's grid (CandleAgent::sample_pack): one thread per element of [B][act]
inline unsigned ag_sample_grid(const AgShape& s) { return (unsigned)(((uint64_t)s.batch * (uint64_t)s.act_dim + 255) / 256); }

// The launches of one update round of P members of shape `s`, in stream order; returns their number (0: no group of that shape).
inline int ag_round_plan(const AgShape& s, unsigned P, AgLaunch* out)
{
    if (ag_shape_ineligible(s) || P < 1) return 0;
    const unsigned NC = (unsigned)s.n_critics;
    GpPlan p{out, 0, s.batch, P, AG_K_DW, AG_K_REDUCE_ADAM};
    p.gather(s.obs_dim);
    p.pack(s.obs_dim + s.act_dim);
    // ---- update_actor
    p.fwd(s.actor, AG_NET_ACTOR, 1);                                          // the actor on obs
    p.one(AG_K_SAMPLE, AG_NET_ACTOR, 0, ag_sample_grid(s), 256);              // act_
    p.fwd(s.critic, AG_NET_CRITIC, 2 * NC);                                   // the online critics on (obs | act) and (obs | act_)
    p.one(AG_K_ACTOR_LOSS, AG_NET_ACTOR, -1, (unsigned)s.act_dim + 1, 1024);
    p.step(s.actor, AG_NET_ACTOR, 1, gp_arena_floats(s.actor) + (uint64_t)((s.act_dim + 63) / 64 * 64));   // head2 behind the layers
    // ---- update_critic
    p.fwd(s.actor, AG_NET_ACTOR, 1);                                          // the updated actor on next_obs
    p.one(AG_K_SAMPLE, AG_NET_ACTOR, 1, ag_sample_grid(s), 256);              // next_act
    p.fwd(s.critic, AG_NET_CRITIC, NC);                                       // the target critics on (next_obs | next_act)
    p.one(AG_K_CRITIC_LOSS, AG_NET_CRITIC, -1, 1, 1024);
    p.step(s.critic, AG_NET_CRITIC, NC, gp_arena_floats(s.critic));           // the last reader of the step slot
    return p.n;
}

inline bool ag_grid_ok(const AgLaunch& l) { return gp_grid_ok(l); }

// May these n agents form a group?  AG_OK: yes.  Otherwise *why says so; the return value is the first member the reason names,
// or AG_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).
constexpr int AG_OK = GP_OK, AG_NO_MEMBER = GP_NO_MEMBER;
inline int ag_group_refusal(const AgMember* m, unsigned n, const char** why, int* kernel = nullptr)
{
    return gp_dense_group_refusal<AG_MAX_LAUNCHES>(
        m, n, why, kernel, &AgMember::kind_awac, "not an AWAC agent",
        "its shape (obs_dim, act_dim, both networks' units and activation_out, n_critics, batch_size) differs from member 0's: one shape per group",
        ag_shape_ineligible, ag_same_shape, ag_round_plan);
}

}  // namespace bdr
