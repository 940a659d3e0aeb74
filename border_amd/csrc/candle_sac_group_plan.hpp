// ================================================================================================
// A group of candle SAC agents (candle_sac_group.hpp), the part without HIP in it: which agents may form a group, and the launches of
// one update round - kernel, network, layer, instances and grid for a shape and P members.  The group's host round and
// tests/test_candle_sac_group_host.py (compiled with the host compiler alone) read the rule from here.
// The round is the launch sequence Sac::opt_ (sac/base.rs:124-134) enqueues for ONE member through CandleSac::update (candle_sac.hip)
// behind the gather of replay_sample_on_stream - pack, the actor on obs, sample + logp of a with its partials, the entropy
// coefficient's step, the online critics on (obs | act) and (obs | a), qmin, the critics' input-gradient chain down to d(-q/B)/da
// (the input layer without a mask), the actor's output gradient and its step, the UPDATED actor on next_obs, sample + logp of
// next_a, the target critics on (next_obs | next_a), the critic loss and the critics' step with the soft update - with the member
// index as grid dimension y of every launch and the network instance, where the standalone launch has one, as grid dimension z.
// With Lp, Lq the layer counts of actor and critic: 3 Lp + 4 Lq + 10 launches whatever P is.
#pragma once
#include <cstdint>

#include "group_plan_common.hpp"

namespace bdr {

constexpr int CS_SHAPE_LAYERS = GP_SHAPE_LAYERS;
constexpr int CS_ACTOR_MLP3 = 0, CS_ACTOR_MLP2 = 1;   // BDR_ACTOR_* (include/border_amd.h)

// ---- what the rule reads of a member ------------------------------------------------------------------------------------------------
using CsNet = GpNet;   // one network (group_plan_common.hpp)
// actor: the layers of the actor's Mlp; with actor_kind Mlp2 its last layer is [mean | s], 2 act_dim wide, and there is no head2
struct CsShape { int obs_dim, act_dim, batch, n_critics, actor_kind; CsNet critic, actor; };
// kind_csac: the agent is a candle SAC agent; n_updates: its n_updates_per_opt
struct CsMember { CsShape shape; int kind_csac; uint64_t n_updates; int device, prof, grad_comm; const void* agent; };

inline bool cs_same_shape(const CsShape& a, const CsShape& b)
{
    return a.obs_dim == b.obs_dim && a.act_dim == b.act_dim && a.batch == b.batch && a.n_critics == b.n_critics && a.actor_kind == b.actor_kind &&
           gp_same_net(a.critic, b.critic) && gp_same_net(a.actor, b.actor);
}
// segments of the actor's reduce + Adam launch: its layers, and Mlp3's head2
inline int cs_actor_segs(const CsShape& s) { return s.actor.n_layers + (s.actor_kind == CS_ACTOR_MLP2 ? 0 : 1); }

// why a candle SAC agent of this shape cannot be a member of any group (nullptr: it can)
inline const char* cs_shape_ineligible(const CsShape& s)
{
    GpShapeOwn own{};
    if (s.actor_kind != CS_ACTOR_MLP3 && s.actor_kind != CS_ACTOR_MLP2) own.first = "unknown actor kind";
    own.two_nc = "n_critics > 2: the online critics on (obs | act) and on (obs | a) run as the 2 n_critics instances of one launch per layer, and a launch holds four";
    if (s.critic.n_layers > GP_RA_SEGS || cs_actor_segs(s) > GP_RA_SEGS)
        own.segs = "more layers than one reduce + Adam launch has segments (12; an Mlp3 actor's head2 is one more)";
    if (s.batch < 2 || s.batch > 65536) own.batch = "batch size out of range (SAC needs at least 2 rows)";
    return gp_shape_ineligible({&s.critic, &s.actor}, s.n_critics, s.critic.n_layers, s.obs_dim, s.act_dim, own);
}

// gather .. dX under GpKernel's numbers, SAC's own behind them, the weight gradient and reduce + Adam last
enum CsKernel {
    CS_K_GATHER = GP_K_GATHER, CS_K_PACK = GP_K_PACK, CS_K_FWD = GP_K_FWD, CS_K_DX = GP_K_DX,
    CS_K_SAMPLE_LOGP = GP_K_OWN, CS_K_ALPHA, CS_K_QMIN, CS_K_ACTOR_GRAD, CS_K_CRITIC_LOSS, CS_K_DW, CS_K_REDUCE_ADAM, CS_K_COUNT
};
enum CsNetId { CS_NET_NONE = GP_NET_NONE, CS_NET_ACTOR = 0, CS_NET_CRITIC = 1 };
inline const char* cs_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "k_csac_pack_group", "k_dense_small_members_z<fwd>", "k_dense_small_members_z<dx>",
                                        "k_csac_sample_logp_group", "k_csac_alpha_group", "k_csac_qmin_group", "k_csac_actor_grad_group",
                                        "k_csac_critic_loss_group", "k_dense_dw_small_members", "k_csac_reduce_adam_group"};
    return k >= 0 && k < CS_K_COUNT ? names[k] : "?";
}
using CsLaunch = GpLaunch;   // net: CsNetId; layer of a sample + logp launch: the draw (0: a, 1: next_a)
constexpr int CS_MAX_LAUNCHES = 7 * CS_SHAPE_LAYERS + 10;

// launches of one round, whatever P is
inline int cs_launch_count(int Lq, int Lp) { return 3 * Lp + 4 * Lq + 10; }
// forward and dX launches of one round: the entries of the dense argument array are (this) x P
inline int cs_dense_launches(int Lq, int Lp) { return 3 * Lp + 4 * Lq - 2; }
// lanes per row of k_csac_sample_logp (CandleSac::sample_logp): the smallest power of two that holds act_dim, at most 64
inline int cs_sample_lanes(int act_dim)
{
    int G = 1;
    while (G < act_dim && G < 64) G *= 2;
    return G;
}
// ... and its grid: 256 / G rows per workgroup
inline unsigned cs_sample_grid(const CsShape& s)
{
    const int rows = 256 / cs_sample_lanes(s.act_dim);
    return (unsigned)((s.batch + rows - 1) / rows);
}
// floats of the actor's arena: its layers, and Mlp3's head2 padded to 64 behind them
inline uint64_t cs_actor_arena(const CsShape& s)
{
    return gp_arena_floats(s.actor) + (s.actor_kind == CS_ACTOR_MLP2 ? 0 : (uint64_t)((s.act_dim + 63) / 64 * 64));
}

// The launches of one update round of P members of shape `s`, in stream order; returns their number (0: no group of that shape).
inline int cs_round_plan(const CsShape& s, unsigned P, CsLaunch* out)
{
    if (cs_shape_ineligible(s) || P < 1) return 0;
    const unsigned NC = (unsigned)s.n_critics;
    GpPlan p{out, 0, s.batch, P, CS_K_DW, CS_K_REDUCE_ADAM};
    p.gather(s.obs_dim);
    p.pack(s.obs_dim + s.act_dim);
    // ---- update_actor
    p.fwd(s.actor, CS_NET_ACTOR, 1);                                              // the actor on obs
    p.one(CS_K_SAMPLE_LOGP, CS_NET_ACTOR, 0, cs_sample_grid(s), 256);             // a, logp, the partials
    p.one(CS_K_ALPHA, CS_NET_NONE, -1, 1, 1024);
    p.fwd(s.critic, CS_NET_CRITIC, 2 * NC);                                       // the online critics on (obs | act) and (obs | a)
    p.one(CS_K_QMIN, CS_NET_CRITIC, -1, (unsigned)((s.batch + 255) / 256), 256);
    p.dx(s.critic, CS_NET_CRITIC, NC, 0);                                         // dq/da: down to the input layer, which has no mask
    p.one(CS_K_ACTOR_GRAD, CS_NET_ACTOR, -1, (unsigned)s.act_dim + 1, 1024);
    p.step(s.actor, CS_NET_ACTOR, 1, cs_actor_arena(s));
    // ---- update_critic
    p.fwd(s.actor, CS_NET_ACTOR, 1);                                              // the updated actor on next_obs
    p.one(CS_K_SAMPLE_LOGP, CS_NET_ACTOR, 1, cs_sample_grid(s), 256);             // next_a, next_logp
    p.fwd(s.critic, CS_NET_CRITIC, NC);                                           // the target critics on (next_obs | next_a)
    p.one(CS_K_CRITIC_LOSS, CS_NET_CRITIC, -1, 1, 1024);
    p.step(s.critic, CS_NET_CRITIC, NC, gp_arena_floats(s.critic));               // the last reader of the step slot
    return p.n;
}

inline bool cs_grid_ok(const CsLaunch& l) { return gp_grid_ok(l); }

// May these n agents form a group?  CS_OK: yes.  Otherwise *why says so; the return value is the first member the reason names,
// or CS_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).
constexpr int CS_OK = GP_OK, CS_NO_MEMBER = GP_NO_MEMBER;
inline int cs_group_refusal(const CsMember* m, unsigned n, const char** why, int* kernel = nullptr)
{
    return gp_dense_group_refusal<CS_MAX_LAUNCHES>(
        m, n, why, kernel, &CsMember::kind_csac, "not a candle SAC agent",
        "its shape (obs_dim, act_dim, both networks' units and activation_out, actor_kind, n_critics, batch_size) differs from member 0's: one shape per group",
        cs_shape_ineligible, cs_same_shape, cs_round_plan);
}

}  // namespace bdr
