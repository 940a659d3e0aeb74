// ================================================================================================
// A group of BC agents (bc_group.hpp), the part without HIP in it: the kernel form a BC agent takes, which agents may form a group,
// and the launches of one update round - kernel and grid for a shape and P members.  Bc itself (bdr_bc_create), the group's host
// round and tests/test_bc_group_host.py (compiled with the host compiler alone) all read the rule from here.
// The round is the launch sequence Bc::opt enqueues for ONE member - the gather of replay_sample_on_stream, pack, the forward layers,
// the loss (general form) or the MFMA head, the input gradients, the grouped weight gradient, reduce + Adam - with the member index as
// grid dimension y of every launch.
#pragma once
#include <cstdint>

#include "group_plan_common.hpp"

namespace bdr {

constexpr int BG_SHAPE_LAYERS = 16;
constexpr int BG_DW_GROUP = 16;     // jobs of one grouped weight-gradient launch (dense.hpp DW_GROUP)
constexpr int BG_RA_SEGS = 12;      // segments of k_dense_reduce_adam (dense.hpp RA_SEGS)
constexpr unsigned BG_MAX_MEMBERS = GP_MAX_MEMBERS;
// the kernel forms and action types of include/border_amd.h (bc_group.hpp checks that they are the same numbers)
enum BgForm { BG_FORM_DEFAULT = 0, BG_FORM_GENERAL = 1, BG_FORM_FUSED = 2, BG_FORM_FUSED_MFMA = 3 };
enum BgAction { BG_ACTION_DISCRETE = 0, BG_ACTION_CONTINUOUS = 1 };

// ---- the form decision (bdr_bc_create) --------------------------------------------------------------------------------------------
// the MFMA head: one padded column block and a hidden layer under it
inline bool bc_can_mfma(int act_dim, int n_units) { return act_dim <= 64 && n_units >= 1; }
// BDR_BC_KERNEL_DEFAULT: the MFMA head where it applies and the update is launch-bound.  Measured at the bc_pen shape (B = 256,
// profiles/bench_bc_pen.json): 23 200-23 600 updates/s against 21 800-22 000 (general) and 22 600-23 000 (k_bc_head, 8 rows) in five
// alternating rounds.  Nothing was measured above a few hundred rows, where the launches stop being the bound: the general form there.
inline int bc_default_form(int batch, bool can_mfma) { return can_mfma && batch <= 1024 ? BG_FORM_FUSED_MFMA : BG_FORM_GENERAL; }
inline int bc_resolve_form(int kernel_form, int batch, int act_dim, int n_units)
{
    return kernel_form != BG_FORM_DEFAULT ? kernel_form : bc_default_form(batch, bc_can_mfma(act_dim, n_units));
}

// ---- what the rule reads of a member ------------------------------------------------------------------------------------------------
// padded sizes (multiples of 64: make_mlp) and logical output width of every layer, the logical input and output widths, the batch
// size, the RESOLVED kernel form
struct BgShape {
    int obs_dim, n_layers;
    int Kp[BG_SHAPE_LAYERS], Np[BG_SHAPE_LAYERS], out[BG_SHAPE_LAYERS];
    int act_dim, batch, activation_out, form, action_type;
};
struct BgMember { BgShape shape; int device, prof, grad_comm; const void* agent; };

// (two layer counts beyond BG_SHAPE_LAYERS differ: such a member is refused before its shape is compared)
inline bool bg_same_shape(const BgShape& a, const BgShape& b)
{
    if (a.obs_dim != b.obs_dim || a.n_layers != b.n_layers || a.act_dim != b.act_dim || a.batch != b.batch || a.activation_out != b.activation_out ||
        a.form != b.form || a.action_type != b.action_type) return false;
    for (int i = 0; i < a.n_layers && i < BG_SHAPE_LAYERS; ++i) if (a.Kp[i] != b.Kp[i] || a.Np[i] != b.Np[i] || a.out[i] != b.out[i]) return false;
    return true;
}

// why a BC agent of this shape cannot be a member of any group (nullptr: it can)
inline const char* bg_shape_ineligible(const BgShape& s)
{
    if (s.action_type != BG_ACTION_CONTINUOUS) return "a Discrete BC agent has no update (the reference's opt_ panics there, bc/base.rs:174)";
    if (s.form == BG_FORM_FUSED) return "the LDS head k_bc_head (kernel_form \"fused\") is not grouped: use \"general\" or \"fused_mfma\"";
    if (s.form != BG_FORM_GENERAL && s.form != BG_FORM_FUSED_MFMA) return "its kernel form is not resolved";
    if (s.n_layers < 1 || s.n_layers > BG_DW_GROUP || s.n_layers > BG_RA_SEGS || s.n_layers > BG_SHAPE_LAYERS)
        return "more layers than one grouped weight-gradient launch (16) or one reduce + Adam launch (12 segments) holds";
    if (s.form == BG_FORM_FUSED_MFMA && (s.n_layers < 2 || s.act_dim > 64)) return "the MFMA head needs a hidden layer and act_dim <= 64";
    if (s.act_dim < 1 || s.act_dim > 256 || s.Np[s.n_layers - 1] > 256) return "act_dim beyond 256: k_bc_loss keeps 32 padded rows in LDS";
    if (s.batch < 1 || s.batch > 65536) return "batch size out of range";
    return nullptr;
}

enum BgKernel { BG_K_GATHER = 0, BG_K_PACK, BG_K_FWD, BG_K_LOSS, BG_K_HEAD, BG_K_DX, BG_K_DW, BG_K_REDUCE_ADAM, BG_K_COUNT };
inline const char* bg_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "k_pack_rows_group", "k_bc_dense_small_group<fwd>", "k_bc_loss_group", "k_bc_head_mfma_group",
                                        "k_bc_dense_small_group<dx>", "k_bc_dense_dw_small_group", "k_bc_reduce_adam_group"};
    return k >= 0 && k < BG_K_COUNT ? names[k] : "?";
}
struct BgLaunch { int kernel, layer; unsigned gx, gy, gz, threads; };   // layer: the layer a forward / dX launch serves, else -1
constexpr int BG_MAX_LAUNCHES = 2 * BG_SHAPE_LAYERS + 4;

// launches of one round, whatever P is: 2L + 4 (general), 2L + 2 (MFMA head)
inline int bg_launch_count(int n_layers, int form) { return form == BG_FORM_GENERAL ? 2 * n_layers + 4 : 2 * n_layers + 2; }
// (the rules every plan shares: group_plan_common.hpp)
inline int bg_dw_chunks(int batch) { return gp_dw_chunks(batch); }
inline unsigned bg_gather_chunks(uint64_t obs_bytes) { return gp_gather_chunks(obs_bytes); }
inline uint64_t bg_arena_floats(const BgShape& s)
{
    uint64_t total = 0;
    for (int i = 0; i < s.n_layers; ++i) total += (uint64_t)s.Kp[i] * s.Np[i] + s.Np[i];
    return total;
}

// The launches of one update round of P members of shape `s`, in stream order; returns their number (0: no group of that shape).
// x is the member's own grid everywhere - the loss and the head count gridDim.x workgroups on the member's own ticket - and y the member.
inline int bg_round_plan(const BgShape& s, unsigned P, BgLaunch* out)
{
    if (bg_shape_ineligible(s) || P < 1) return 0;
    const int L = s.n_layers, B = s.batch;
    const bool head = s.form == BG_FORM_FUSED_MFMA;
    const unsigned RB = (unsigned)((B + 31) / 32);
    int n = 0;
    out[n++] = BgLaunch{BG_K_GATHER, -1, (unsigned)B * bg_gather_chunks((uint64_t)s.obs_dim * 4), P, 1, 256};
    out[n++] = BgLaunch{BG_K_PACK, -1, (unsigned)((B * s.obs_dim + 255) / 256), P, 1, 256};
    for (int i = 0; i < (head ? L - 1 : L); ++i) out[n++] = BgLaunch{BG_K_FWD, i, RB * (unsigned)(s.Np[i] / 32), P, 1, 256};
    out[n++] = BgLaunch{head ? BG_K_HEAD : BG_K_LOSS, -1, RB, P, 1, 256};
    for (int i = head ? L - 2 : L - 1; i > 0; --i) out[n++] = BgLaunch{BG_K_DX, i, RB * (unsigned)(s.Kp[i] / 32), P, 1, 256};
    unsigned dw = 0;
    for (int i = 0; i < L; ++i) dw += (unsigned)((s.Kp[i] / 32) * (s.Np[i] / 32) * bg_dw_chunks(B));
    out[n++] = BgLaunch{BG_K_DW, -1, dw, P, 1, 256};
    out[n++] = BgLaunch{BG_K_REDUCE_ADAM, -1, (unsigned)((bg_arena_floats(s) / 4 + 255) / 256), P, 1, 256};
    return n;
}

inline bool bg_grid_ok(const BgLaunch& l) { return gp_grid_ok(l); }

// May these n agents form a group?  BG_OK: yes.  Otherwise *why says so; the return value is the first member the reason names,
// or BG_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).
constexpr int BG_OK = GP_OK, BG_NO_MEMBER = GP_NO_MEMBER;
inline int bg_group_refusal(const BgMember* m, unsigned n, const char** why, int* kernel = nullptr)
{
    const auto own = [&](const BgMember& x) -> const char* {
        if (const char* w = bg_shape_ineligible(x.shape)) return w;
        if (!bg_same_shape(x.shape, m[0].shape))
            return "its shape (obs_dim, units, act_dim, activation_out, batch_size, resolved kernel form) differs from member 0's: one shape per group";
        return nullptr;
    };
    return gp_group_refusal<BgLaunch, BG_MAX_LAUNCHES>(m, n, why, kernel, own, [&](BgLaunch* out) { return bg_round_plan(m[0].shape, n, out); });
}

}  // namespace bdr
