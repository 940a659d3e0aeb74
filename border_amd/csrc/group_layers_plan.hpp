// ================================================================================================
// The layer form of an agent group (group_layers.hpp), the part without HIP in it: which step an Mlp DQN member takes, whether it may
// join a layer-form group, and the launches of one update round - kernel and grid for a shape and P members.  DqnMlp::fused_ok, the
// group's host round and tests/test_group_layers_host.py (compiled with the host compiler alone) all read the rule from here.
// The round is the launch sequence DqnMlp::update_critic enqueues for ONE member on its latency-shaped layer path, behind the gather
// of replay_sample_on_stream, with the member index as one more grid dimension of every launch.
#pragma once
#include <cstdint>

#include "group_plan_common.hpp"

namespace bdr {

constexpr int GL_MAXL = 4;        // layers the acting kernel covers (mlp_fused.hpp MF_MAXL)
constexpr int GL_RA_SEGS = 12;    // segments of k_dense_reduce_adam (dense.hpp RA_SEGS)
constexpr int GL_MAX_WIDTH = 256; // padded width mf_act_body keeps in LDS
constexpr int GL_SHAPE_LAYERS = 16;

// what the rule reads of a member: padded sizes (multiples of 64), batch size, the switches of its environment
struct GlShape {
    int in_dim, n_layers;
    int Kp[GL_SHAPE_LAYERS], Np[GL_SHAPE_LAYERS];
    int out_dim, batch, double_dqn, activation_out;
    int fused, small_gemm, head_fuse, head_fuse_wide;   // BDR_NO_MLP_FUSED / BDR_NO_SMALL_GEMM / BDR_NO_MLP_HEAD_FUSE / BDR_MLP_HEAD_FUSE_WIDE
};

inline bool gl_same_shape(const GlShape& a, const GlShape& b)
{
    if (a.in_dim != b.in_dim || a.n_layers != b.n_layers || a.out_dim != b.out_dim || a.batch != b.batch || a.double_dqn != b.double_dqn ||
        a.activation_out != b.activation_out || a.head_fuse != b.head_fuse || a.head_fuse_wide != b.head_fuse_wide) return false;
    for (int i = 0; i < a.n_layers && i < GL_SHAPE_LAYERS; ++i) if (a.Kp[i] != b.Kp[i] || a.Np[i] != b.Np[i]) return false;
    return true;
}

// DqnMlp::fused_ok: the one-workgroup step (mlp_fused.hpp) while every phase is a single pass of eight waves over its 32x32 blocks
inline bool gl_fused_ok(const GlShape& s)
{
    if (!s.fused || s.n_layers > GL_MAXL || s.batch > 128 || s.out_dim > 64) return false;
    for (int i = 0; i < s.n_layers; ++i) if (s.Kp[i] > 256 || s.Np[i] > 256) return false;
    const int nz = s.double_dqn ? 3 : 2, RB = (s.batch + 31) / 32;
    for (int i = 0; i < s.n_layers; ++i) if (nz * RB * (s.Np[i] / 32) > 8 || RB * (s.Kp[i] / 32) * (s.Np[i] / 32) > 8) return false;
    return true;
}

// the row-block head (k_mlp_head_td) on uniform rings: DqnMlp::update_critic's head_fused
inline bool gl_head_fused(const GlShape& s)
{
    const int L = s.n_layers;
    return s.head_fuse && L >= 2 && s.out_dim <= 32 && s.Kp[L - 1] <= (s.head_fuse_wide ? 4096 : 128);
}

// why a member that does not take the one-workgroup step cannot join a layer-form group (nullptr: it can)
inline const char* gl_layers_ineligible(const GlShape& s)
{
    if (!s.small_gemm) return "the latency-shaped layer path is switched off (BDR_NO_SMALL_GEMM)";
    if (s.n_layers > GL_MAXL || s.n_layers > GL_RA_SEGS) return "more than 4 layers: the acting kernel and the reduce + Adam kernel do not cover it";
    for (int i = 0; i < s.n_layers; ++i)
        if (s.Kp[i] > GL_MAX_WIDTH || s.Np[i] > GL_MAX_WIDTH) return "a layer wider than 256: the acting kernel does not cover it";
    if (s.batch < 1 || s.batch >= (1 << 20)) return "batch size out of range";
    return nullptr;
}

enum GlForm { GL_FORM_ONE_WORKGROUP = 0, GL_FORM_LAYERS = 1 };

enum GlKernel { GL_K_GATHER = 0, GL_K_PACK, GL_K_FWD, GL_K_HEAD_TD, GL_K_TD_DENSE, GL_K_MEAN_ROWS, GL_K_DX, GL_K_DW, GL_K_REDUCE_ADAM, GL_K_STEP };
inline const char* gl_kernel_name(int k)
{
    static const char* const names[] = {"k_gather_group", "k_mlp_pack_z_group", "k_dense_small_group<fwd>", "k_mlp_head_td_group", "k_td_dense_group",
                                        "k_mean_rows_group", "k_dense_small_group<dx>", "k_dense_dw_small_group_members", "k_dense_reduce_adam_group",
                                        "k_dqn_mlp_step_group"};
    return k >= 0 && k < 10 ? names[k] : "?";
}
struct GlLaunch { int kernel, layer; unsigned gx, gy, gz, threads; };   // layer: the layer a forward / dX launch serves, else -1
constexpr int GL_MAX_LAUNCHES = 2 + GL_MAXL + 2 + GL_MAXL + 2;

// (the rules every plan shares: group_plan_common.hpp)
inline int gl_dw_chunks(int batch) { return gp_dw_chunks(batch); }
inline unsigned gl_gather_chunks(uint64_t obs_bytes) { return gp_gather_chunks(obs_bytes); }

// The launches of one update round of P members of shape `s` on uniform rings, in stream order; returns their number (0: a member of
// that shape does not take the layer form).  The member index is grid y everywhere but in the two kernels that already use y or z:
// the row-block head (x row blocks, y column groups, z member) and the layers (x tiles, y member, z network instance).
inline int gl_round_plan(const GlShape& s, unsigned P, GlLaunch* out)
{
    if (gl_fused_ok(s)) { out[0] = GlLaunch{GL_K_STEP, -1, P, 1, 1, 512}; return 1; }
    if (gl_layers_ineligible(s)) return 0;
    const int L = s.n_layers, B = s.batch, nz = s.double_dqn ? 3 : 2;
    const bool head = gl_head_fused(s);
    const unsigned RB = (unsigned)((B + 31) / 32);
    int n = 0;
    out[n++] = GlLaunch{GL_K_GATHER, -1, (unsigned)B * gl_gather_chunks((uint64_t)s.in_dim * 4), P, 1, 256};
    out[n++] = GlLaunch{GL_K_PACK, -1, (unsigned)((nz * B * s.in_dim + 255) / 256), P, 1, 256};
    for (int i = 0; i < (head ? L - 1 : L); ++i) out[n++] = GlLaunch{GL_K_FWD, i, RB * (unsigned)(s.Np[i] / 32), P, (unsigned)nz, 256};
    if (head) out[n++] = GlLaunch{GL_K_HEAD_TD, -1, RB, (unsigned)(s.Kp[L - 1] / 64), P, 512};
    else {
        out[n++] = GlLaunch{GL_K_TD_DENSE, -1, (unsigned)((B + 3) / 4), P, 1, 256};
        out[n++] = GlLaunch{GL_K_MEAN_ROWS, -1, 1, P, 1, 256};
    }
    for (int i = head ? L - 2 : L - 1; i > 0; --i) out[n++] = GlLaunch{GL_K_DX, i, RB * (unsigned)(s.Kp[i] / 32), P, 1, 256};
    unsigned dw = 0;
    for (int i = 0; i < L; ++i) dw += (unsigned)((s.Kp[i] / 32) * (s.Np[i] / 32) * gl_dw_chunks(B));
    out[n++] = GlLaunch{GL_K_DW, -1, dw, P, 1, 256};
    uint64_t total = 0;
    for (int i = 0; i < L; ++i) total += (uint64_t)s.Kp[i] * s.Np[i] + s.Np[i];
    out[n++] = GlLaunch{GL_K_REDUCE_ADAM, -1, (unsigned)((total / 4 + 255) / 256), P, 1, 256};
    return n;
}

inline bool gl_grid_ok(const GlLaunch& l) { return gp_grid_ok(l); }

}  // namespace bdr
