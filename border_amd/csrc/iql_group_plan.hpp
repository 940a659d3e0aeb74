// ================================================================================================
// A group of IQL agents (iql_group.hpp), the part without HIP in it: which agents may form a group, and the launches of one update
// round - kernel, network, layer, instances and grid for a shape and P members.  The group's host round and
// tests/test_iql_group_host.py (compiled with the host compiler alone) read the rule from here.
// The round is the launch sequence Iql::opt_ (iql/base.rs:157-188) enqueues for ONE member through Iql::update (iql.hip) - the gather of
// replay_sample_on_stream, pack, the forwards of target + online critics, actor and value, the value loss and the value step, V'(obs)
// and V'(next_obs), the critic loss and the critics' step with the soft update, the target critics again, the actor loss and the
// actor's step - with the member index as grid dimension y of every launch and the network instance, where the standalone launch has
// one, as grid dimension z.  With Lv, Lq, Lp the layer counts: 3 (Lq + Lv) + 2 Lp + 8 launches whatever P is.
#pragma once
#include <cstdint>

#include "group_plan_common.hpp"

namespace bdr {

constexpr int IG_SHAPE_LAYERS = GP_SHAPE_LAYERS;

// ---- what the rule reads of a member ------------------------------------------------------------------------------------------------
// one network (group_plan_common.hpp, shared with awac_group_plan.hpp)
using IgNet = GpNet;
struct IgShape { int obs_dim, act_dim, batch, n_critics; IgNet value, critic, actor; };
// kind_iql: the agent is an IQL agent; n_updates: its n_updates_per_opt
struct IgMember { IgShape shape; int kind_iql; uint64_t n_updates; int device, prof, grad_comm; const void* agent; };

inline bool ig_same_shape(const IgShape& a, const IgShape& b)
{
    return a.obs_dim == b.obs_dim && a.act_dim == b.act_dim && a.batch == b.batch && a.n_critics == b.n_critics && gp_same_net(a.value, b.value) &&
           gp_same_net(a.critic, b.critic) && gp_same_net(a.actor, b.actor);
}

// why an IQL agent of this shape cannot be a member of any group (nullptr: it can)
inline const char* ig_shape_ineligible(const IgShape& s)
{
    GpShapeOwn own{};
    own.two_nc = "n_critics > 2: target and online critics run as the 2 n_critics instances of one launch per layer, and a launch holds four";
    if (s.critic.n_layers > GP_RA_SEGS || s.actor.n_layers + 1 > GP_RA_SEGS || s.value.n_layers > GP_RA_SEGS)
        own.segs = "more layers than one reduce + Adam launch has segments (12; the actor's head2 is one more)";
    if (s.batch < 1 || s.batch > 65536) own.batch = "batch size out of range";
    return gp_shape_ineligible({&s.value, &s.critic, &s.actor}, s.n_critics, s.critic.n_layers, s.obs_dim, s.act_dim, own);
}

// gather .. dX under GpKernel's numbers, IQL's own behind them, the weight gradient and reduce + Adam last
enum IgKernel {
    IG_K_GATHER = GP_K_GATHER, IG_K_PACK = GP_K_PACK, IG_K_FWD = GP_K_FWD, IG_K_DX = GP_K_DX,
    IG_K_VALUE_LOSS = GP_K_OWN, IG_K_CRITIC_LOSS, IG_K_ACTOR_LOSS, IG_K_DW, IG_K_REDUCE_ADAM, IG_K_COUNT
};
enum IgNetId { IG_NET_NONE = GP_NET_NONE, IG_NET_VALUE = 0, IG_NET_CRITIC = 1, IG_NET_ACTOR = 2 };
inline const char* ig_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "k_iql_pack_group", "k_dense_small_members_z<fwd>", "k_dense_small_members_z<dx>", "k_iql_value_loss_group",
                                        "k_iql_critic_loss_group", "k_iql_actor_loss_group", "k_dense_dw_small_members", "k_iql_reduce_adam_group"};
    return k >= 0 && k < IG_K_COUNT ? names[k] : "?";
}
using IgLaunch = GpLaunch;   // net: IgNetId
constexpr int IG_MAX_LAUNCHES = 8 * IG_SHAPE_LAYERS + 8;

// launches of one round, whatever P is
inline int ig_launch_count(int Lv, int Lq, int Lp) { return 3 * (Lq + Lv) + 2 * Lp + 8; }
// forward and dX launches of one round: the entries of the dense argument array are (this) x P
inline int ig_dense_launches(int Lv, int Lq, int Lp) { return 3 * (Lq + Lv) + 2 * Lp - 3; }

// The launches of one update round of P members of shape `s`, in stream order; returns their number (0: no group of that shape).
inline int ig_round_plan(const IgShape& s, unsigned P, IgLaunch* out)
{
    if (ig_shape_ineligible(s) || P < 1) return 0;
    const unsigned NC = (unsigned)s.n_critics;
    GpPlan p{out, 0, s.batch, P, IG_K_DW, IG_K_REDUCE_ADAM};
    p.gather(s.obs_dim);
    p.pack(s.obs_dim + s.act_dim);
    p.fwd(s.critic, IG_NET_CRITIC, 2 * NC);            // target and online critics
    p.fwd(s.actor, IG_NET_ACTOR, 1);
    p.fwd(s.value, IG_NET_VALUE, 1);
    p.one(IG_K_VALUE_LOSS, IG_NET_VALUE, -1, 1, 1024);
    p.step(s.value, IG_NET_VALUE, 1, gp_arena_floats(s.value));
    p.fwd(s.value, IG_NET_VALUE, 2);                   // V'(obs), V'(next_obs)
    p.one(IG_K_CRITIC_LOSS, IG_NET_CRITIC, -1, 1, 1024);
    p.step(s.critic, IG_NET_CRITIC, NC, gp_arena_floats(s.critic));
    p.fwd(s.critic, IG_NET_CRITIC, NC);                // the target critics after the soft update
    p.one(IG_K_ACTOR_LOSS, IG_NET_ACTOR, -1, 1, 1024);
    p.step(s.actor, IG_NET_ACTOR, 1, gp_arena_floats(s.actor) + (uint64_t)((s.act_dim + 63) / 64 * 64));   // head2 behind the layers
    return p.n;
}

inline bool ig_grid_ok(const IgLaunch& l) { return gp_grid_ok(l); }

// May these n agents form a group?  IG_OK: yes.  Otherwise *why says so; the return value is the first member the reason names,
// or IG_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).
constexpr int IG_OK = GP_OK, IG_NO_MEMBER = GP_NO_MEMBER;
inline int ig_group_refusal(const IgMember* m, unsigned n, const char** why, int* kernel = nullptr)
{
    return gp_dense_group_refusal<IG_MAX_LAUNCHES>(
        m, n, why, kernel, &IgMember::kind_iql, "not an IQL agent",
        "its shape (obs_dim, act_dim, the three networks' units and activation_out, n_critics, batch_size) differs from member 0's: one shape per group",
        ig_shape_ineligible, ig_same_shape, ig_round_plan);
}

}  // namespace bdr
