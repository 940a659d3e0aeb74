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
constexpr int IG_DW_GROUP = 16;     // jobs of one grouped weight-gradient launch (dense.hpp DW_GROUP)
constexpr int IG_RA_SEGS = 12;      // segments of k_dense_reduce_adam (dense.hpp RA_SEGS)
constexpr int IG_MAXZ = 4;          // instances of one dense launch (dense.hpp DenseArgsZ, RA_INST)
constexpr unsigned IG_MAX_MEMBERS = GP_MAX_MEMBERS;

// ---- what the rule reads of a member ------------------------------------------------------------------------------------------------
// one network (group_plan_common.hpp, shared with awac_group_plan.hpp)
using IgNet = GpNet;
struct IgShape { int obs_dim, act_dim, batch, n_critics; IgNet value, critic, actor; };
// kind_iql: the agent is an IQL agent; n_updates: its n_updates_per_opt
struct IgMember { IgShape shape; int kind_iql; uint64_t n_updates; int device, prof, grad_comm; const void* agent; };

inline bool ig_same_net(const IgNet& a, const IgNet& b) { return gp_same_net(a, b); }
inline bool ig_same_shape(const IgShape& a, const IgShape& b)
{
    return a.obs_dim == b.obs_dim && a.act_dim == b.act_dim && a.batch == b.batch && a.n_critics == b.n_critics && ig_same_net(a.value, b.value) &&
           ig_same_net(a.critic, b.critic) && ig_same_net(a.actor, b.actor);
}

// why an IQL agent of this shape cannot be a member of any group (nullptr: it can)
inline const char* ig_shape_ineligible(const IgShape& s)
{
    for (const IgNet* n : {&s.value, &s.critic, &s.actor})
        if (n->n_layers < 1 || n->n_layers > IG_SHAPE_LAYERS) return "a network has no layer, or more than 16";
    if (s.n_critics < 1) return "n_critics must be positive";
    if (2 * s.n_critics > IG_MAXZ)
        return "n_critics > 2: target and online critics run as the 2 n_critics instances of one launch per layer, and a launch holds four";
    if (s.n_critics * s.critic.n_layers > IG_DW_GROUP) return "n_critics x critic layers beyond the 16 jobs of one grouped weight-gradient launch";
    if (s.critic.n_layers > IG_RA_SEGS || s.actor.n_layers + 1 > IG_RA_SEGS || s.value.n_layers > IG_RA_SEGS)
        return "more layers than one reduce + Adam launch has segments (12; the actor's head2 is one more)";
    if (s.batch < 1 || s.batch > 65536) return "batch size out of range";
    if (s.obs_dim < 1 || s.act_dim < 1) return "bad obs/act dims";
    return nullptr;
}

enum IgKernel { IG_K_GATHER = 0, IG_K_PACK, IG_K_FWD, IG_K_DX, IG_K_VALUE_LOSS, IG_K_CRITIC_LOSS, IG_K_ACTOR_LOSS, IG_K_DW, IG_K_REDUCE_ADAM, IG_K_COUNT };
enum IgNetId { IG_NET_NONE = -1, IG_NET_VALUE = 0, IG_NET_CRITIC = 1, IG_NET_ACTOR = 2 };
inline const char* ig_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "k_iql_pack_group", "k_dense_small_members_z<fwd>", "k_dense_small_members_z<dx>", "k_iql_value_loss_group",
                                        "k_iql_critic_loss_group", "k_iql_actor_loss_group", "k_dense_dw_small_members", "k_iql_reduce_adam_group"};
    return k >= 0 && k < IG_K_COUNT ? names[k] : "?";
}
// net: the network a dense / dW / reduce launch serves (IgNetId), layer: the layer a forward / dX launch serves, else -1; gz = the
// instances nz of the launch
struct IgLaunch { int kernel, net, layer; unsigned gx, gy, gz, threads; };
constexpr int IG_MAX_LAUNCHES = 8 * IG_SHAPE_LAYERS + 8;

// launches of one round, whatever P is
inline int ig_launch_count(int Lv, int Lq, int Lp) { return 3 * (Lq + Lv) + 2 * Lp + 8; }
// forward and dX launches of one round: the entries of the dense argument array are (this) x P
inline int ig_dense_launches(int Lv, int Lq, int Lp) { return 3 * (Lq + Lv) + 2 * Lp - 3; }
// (the rules every plan shares: group_plan_common.hpp)
inline int ig_dw_chunks(int batch) { return gp_dw_chunks(batch); }
inline unsigned ig_gather_chunks(uint64_t obs_bytes) { return gp_gather_chunks(obs_bytes); }
inline uint64_t ig_arena_floats(const IgNet& n) { return gp_arena_floats(n); }
inline unsigned ig_dw_tiles(const IgNet& n, int batch) { return gp_dw_tiles(n, batch); }
// k_iql_pack's grid (Iql::update): one thread per element of [B][obs + act], at most 2048 workgroups (the body strides by the grid)
inline unsigned ig_pack_grid(const IgShape& s)
{
    const uint64_t g = ((uint64_t)s.batch * (uint64_t)(s.obs_dim + s.act_dim) + 255) / 256;
    return (unsigned)(g < 2048 ? g : 2048);
}

// The launches of one update round of P members of shape `s`, in stream order; returns their number (0: no group of that shape).
// x is the member's own grid everywhere, y the member, z the network instance.
inline int ig_round_plan(const IgShape& s, unsigned P, IgLaunch* out)
{
    if (ig_shape_ineligible(s) || P < 1) return 0;
    const int B = s.batch, NC = s.n_critics;
    const unsigned RB = (unsigned)((B + 31) / 32);
    int n = 0;
    const auto fwd = [&](const IgNet& net, int id, unsigned nz) {
        for (int i = 0; i < net.n_layers; ++i) out[n++] = IgLaunch{IG_K_FWD, id, i, RB * (unsigned)(net.Np[i] / 32), P, nz, 256};
    };
    // mlp_backward_step: the input gradients down to layer 1, the grouped weight gradient, reduce + Adam over `arena` floats
    const auto step = [&](const IgNet& net, int id, unsigned nz, uint64_t arena) {
        for (int i = net.n_layers - 1; i > 0; --i) out[n++] = IgLaunch{IG_K_DX, id, i, RB * (unsigned)(net.Kp[i] / 32), P, nz, 256};
        out[n++] = IgLaunch{IG_K_DW, id, -1, nz * ig_dw_tiles(net, B), P, 1, 256};
        out[n++] = IgLaunch{IG_K_REDUCE_ADAM, id, -1, (unsigned)((arena / 4 + 255) / 256), P, nz, 256};
    };
    out[n++] = IgLaunch{IG_K_GATHER, IG_NET_NONE, -1, (unsigned)B * ig_gather_chunks((uint64_t)s.obs_dim * 4), P, 1, 256};
    out[n++] = IgLaunch{IG_K_PACK, IG_NET_NONE, -1, ig_pack_grid(s), P, 1, 256};
    fwd(s.critic, IG_NET_CRITIC, 2u * (unsigned)NC);   // target and online critics
    fwd(s.actor, IG_NET_ACTOR, 1);
    fwd(s.value, IG_NET_VALUE, 1);
    out[n++] = IgLaunch{IG_K_VALUE_LOSS, IG_NET_VALUE, -1, 1, P, 1, 1024};
    step(s.value, IG_NET_VALUE, 1, ig_arena_floats(s.value));
    fwd(s.value, IG_NET_VALUE, 2);                     // V'(obs), V'(next_obs)
    out[n++] = IgLaunch{IG_K_CRITIC_LOSS, IG_NET_CRITIC, -1, 1, P, 1, 1024};
    step(s.critic, IG_NET_CRITIC, (unsigned)NC, ig_arena_floats(s.critic));
    fwd(s.critic, IG_NET_CRITIC, (unsigned)NC);        // the target critics after the soft update
    out[n++] = IgLaunch{IG_K_ACTOR_LOSS, IG_NET_ACTOR, -1, 1, P, 1, 1024};
    step(s.actor, IG_NET_ACTOR, 1, ig_arena_floats(s.actor) + (uint64_t)((s.act_dim + 63) / 64 * 64));   // head2 behind the layers
    return n;
}

inline bool ig_grid_ok(const IgLaunch& l) { return gp_grid_ok(l); }

// May these n agents form a group?  IG_OK: yes.  Otherwise *why says so; the return value is the first member the reason names,
// or IG_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).
constexpr int IG_OK = GP_OK, IG_NO_MEMBER = GP_NO_MEMBER;
inline int ig_group_refusal(const IgMember* m, unsigned n, const char** why, int* kernel = nullptr)
{
    const auto own = [&](const IgMember& x) -> const char* {
        if (!x.kind_iql) return "not an IQL agent";
        if (const char* w = ig_shape_ineligible(x.shape)) return w;
        if (!ig_same_shape(x.shape, m[0].shape))
            return "its shape (obs_dim, act_dim, the three networks' units and activation_out, n_critics, batch_size) differs from member 0's: one shape per group";
        if (x.n_updates != 1) return "n_updates_per_opt != 1 is not built for a group";
        return nullptr;
    };
    return gp_group_refusal<IgLaunch, IG_MAX_LAUNCHES>(m, n, why, kernel, own, [&](IgLaunch* out) { return ig_round_plan(m[0].shape, n, out); });
}

}  // namespace bdr
