// ================================================================================================
// The group entries of the Nature-CNN trunk's kernels (igemm.hpp, conv1_bf16_img.hpp, conv1_dw_bf16.hpp; policies: cnn_layers.hpp) with
// the member as grid dimension y, for launch groupings of agents that run the trunk layer by layer (candle_dqn_cnn_group.hpp), and the
// host writers of one member's entries - what trunk_conv1 / trunk_conv23 / trunk_backward (conv_trunk.hpp) hand the standalone launches.
// Each entry runs the body of the kernel it groups on the member's entry of a device array, read in place through the constant address
// space: the member comes from blockIdx.y, so it is uniform and the entry's fields are scalar loads, as they are from the
// kernel-argument segment of the standalone kernel.  The conv1 bodies read the entry directly; the igemm bodies hand their arguments to
// the policies' hooks, so there the fields are copied into an argument struct in registers (as dg_step_scalars hands over a member's
// optimizer scalars), with the network instance of a forward entry already selected: no run-time index reaches a register array.
// The bodies are the *_body_inc.hpp texts the standalone kernels compile (igemm_body_inc.hpp, conv1_bf16_img_body_inc.hpp,
// conv1_dw_bf16_body_inc.hpp) and igemm_red_body: same tiles, same k order, same bits - and the standalone kernels' own code is
// token for token what it was.
//   k_igemm_members<P, TEAMS, PEEL>   k_igemm's body on the member.  Forward (FwdC2, FwdC3; Args = FwdArgs): grid (row tiles, P, nz), z the
//                                     instance.  Input gradients (DxC3Pos / DxC3PosL with two teams, DxC2MPos; Args = DxArgs): grid
//                                     (tiles * positions, P): the standalone grid (tiles, positions) folded into x, position = x / tiles
//                                     - the positions stay ordered by decreasing tap count -, tile = x % tiles; `tiles` is a kernel argument.
//   k_igemm_red_members<P>            igemm_red_body (DwC3, DwC2) on the member's DwArgs: grid (wgs * chunks, P); the body's own
//                                     (workgroup, grid) pair is (blockIdx.x, gridDim.x), the member's own grid.
//   k_conv1_img_members<NS, IPW>      k_conv1_bf16_img's body with 512 threads: grid (workgroups per instance * nz, P), instance = x % nz.
//   k_conv1_dw_members<NS>            k_conv1_dw_bf16's body: grid (chunks, P), dynamic LDS c1dw_lds_bytes(NS).
// Launch bounds, LDS and wave counts are those of the standalone kernels (the bodies declare the LDS).
// Bounds of every new index: member = blockIdx.y < gridDim.y = P = the length of every argument array here; the instance
// z = blockIdx.z < gridDim.z = nz <= MAXZ = the instances of a FwdArgs; conv1's instance x % nz < nz = the entry's nz <= 3; a dX
// entry's position x / tiles < gridDim.x / tiles = the policy's positions (81 / 100: the host launches tiles * positions
// workgroups) and tile x % tiles < tiles.  Inside a member every index is the body's own, with the bounds of the standalone kernel
// (rows < M = the member's batch x rows per image, clamped or predicated by the body).
// No workgroup waits for another; memory traffic is the bodies' plain vector loads and stores.
#pragma once
#include "conv_trunk.hpp"
#include "candle_dqn_cnn_group_plan.hpp"

namespace {

// ---- a member's entry -> the body's argument struct, field by field -----------------------------------------------------------------
__device__ __forceinline__ FwdArgs cg_args(const BDR_CONST_AS FwdArgs& e, unsigned z)
{
    FwdArgs a{};
    a.x[0] = e.x[z]; a.w[0] = e.w[z]; a.bias[0] = e.bias[z]; a.out[0] = e.out[z]; a.M = e.M; a.nkt_per_split = e.nkt_per_split;
    return a;
}
__device__ __forceinline__ DxArgs cg_args(const BDR_CONST_AS DxArgs& e, unsigned)
{
    return DxArgs{e.dy, e.w, e.mask, e.out, e.M, nullptr, 0};
}
__device__ __forceinline__ DwArgs cg_args(const BDR_CONST_AS DwArgs& e)
{
    return DwArgs{e.x, e.dy, e.part, e.part_stride, e.M, nullptr, 0};
}

// ---- the group entries: grid dimension y is the member ------------------------------------------------------------------------------
template <class P, int TEAMS = 1, bool PEEL = false>
__global__ __launch_bounds__(64 * P::WM * P::WN * TEAMS) void k_igemm_members(const BDR_CONST_AS typename P::Args* member_args, unsigned tiles)
{
    const typename P::Args args = cg_args(member_args[blockIdx.y], blockIdx.z);   // (a forward entry's instance is slot 0 of `args`)
    // input gradients: the standalone grid (tiles, positions) folded into x
#define IGEMM_BX (has_vrow_y<P>::value ? blockIdx.x % tiles : blockIdx.x)
#define IGEMM_BY (has_vrow_y<P>::value ? blockIdx.x / tiles : 0u)
#define IGEMM_BZ 0u
#include "igemm_body_inc.hpp"
#undef IGEMM_BX
#undef IGEMM_BY
#undef IGEMM_BZ
}
template <class P>
__global__ __launch_bounds__(256) void k_igemm_red_members(const BDR_CONST_AS typename P::Args* args)
{
    const typename P::Args a = cg_args(args[blockIdx.y]);
    igemm_red_body<P>(a, (int)blockIdx.x, (int)gridDim.x);
}
template <int NS, int IPW>
__global__ __launch_bounds__(512, 2) void k_conv1_img_members(const BDR_CONST_AS Conv1Args* args)
{
    constexpr int NT = 512;
    const BDR_CONST_AS Conv1Args& a = args[blockIdx.y];
#include "conv1_bf16_img_body_inc.hpp"
}
template <int NS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NS <= 4 ? C1DW_WAVES_PER_EU : 2, NS <= 4 ? C1DW_WAVES_PER_EU : 2))) void k_conv1_dw_members(
    const BDR_CONST_AS Conv1DwArgs* args)
{
    const BDR_CONST_AS Conv1DwArgs& a = args[blockIdx.y];
#include "conv1_dw_bf16_body_inc.hpp"
}

// ---- host: one member's entries, what conv_trunk.hpp hands the standalone launches ----------------------------------------------------
struct ConvMemberArgs {
    Conv1Args c1; FwdArgs f2, f3;
    DwArgs dw3, dw2; DxArgs dx3, dx2; Conv1DwArgs dw1;
    int dw_chunks[3];              // chunks of this batch per layer (conv1, conv2, conv3)
    ConvDwLayer layer[3];          // conv_dw_plan's entries at the member's capacity: where its partials lie
};
// trunk_conv1 + trunk_conv23 of nz (parameters, u8 rows) pairs, then trunk_backward from dy3: Bn images, cap = the capacity part_conv
// was allocated for
inline void cg_member_static(const Arena& conv, int nz, const float* const* pp, const uint8_t* const* rows, float* const* a1, float* const* a2, float* const* a3,
                             const float* dy3, float* dy2, float* dy1, float* part_conv, int Bn, int cap, ConvMemberArgs& o)
{
    o = ConvMemberArgs{};
    o.c1.M = Bn * 400; o.c1.nz = nz; o.f2.M = Bn * 81; o.f3.M = Bn * 49;
    for (int z = 0; z < nz; ++z) {
        o.c1.x[z] = rows[z]; o.c1.w1[z] = pp[z] + conv.w1; o.c1.bias[z] = pp[z] + conv.b1; o.c1.out[z] = a1[z];
        o.f2.x[z] = a1[z]; o.f2.w[z] = pp[z] + conv.w2; o.f2.bias[z] = pp[z] + conv.b2; o.f2.out[z] = a2[z];
        o.f3.x[z] = a2[z]; o.f3.w[z] = pp[z] + conv.w3; o.f3.bias[z] = pp[z] + conv.b3; o.f3.out[z] = a3[z];
    }
    const ConvDwPlan pl = conv_dw_plan(conv, cap);
    for (int k = 0; k < 3; ++k) { o.layer[k] = pl.layer[k]; o.dw_chunks[k] = pl.layer[k].chunks(Bn); }
    const float* p = pp[0];   // the online parameters
    o.dw3 = DwArgs{a2[0], dy3, part_conv + pl.layer[2].off, pl.layer[2].stride, Bn * 49, nullptr, 0};
    o.dx3 = DxArgs{dy3, p + conv.w3, a2[0], dy2, Bn * 81, nullptr, 0};
    o.dw2 = DwArgs{a1[0], dy2, part_conv + pl.layer[1].off, pl.layer[1].stride, Bn * 81, nullptr, 0};
    o.dx2 = DxArgs{dy2, p + conv.w2, a1[0], dy1, Bn * 100, nullptr, 0};
    o.dw1 = Conv1DwArgs{rows[0], dy1, part_conv + pl.layer[0].off, pl.layer[0].stride, Bn, nullptr, 0};
}

// the staged arrays of the trunk's launches, [P] each
struct ConvRound {
    StagedArray<Conv1Args> c1; StagedArray<FwdArgs> f2, f3;
    StagedArray<DwArgs> dw3, dw2; StagedArray<DxArgs> dx3, dx2; StagedArray<Conv1DwArgs> dw1;
    hipError_t resize(size_t P) { return staged_resize(P, c1, f2, f3, dw3, dx3, dw2, dx2, dw1); }
    void stage(size_t p, const ConvMemberArgs& o)
    {
        c1[p] = o.c1; f2[p] = o.f2; f3[p] = o.f3; dw3[p] = o.dw3; dx3[p] = o.dx3; dw2[p] = o.dw2; dx2[p] = o.dx2; dw1[p] = o.dw1;
    }
    hipError_t upload() { return staged_upload(c1, f2, f3, dw3, dx3, dw2, dx2, dw1); }
};

// the dynamic LDS of conv1's weight-gradient entry, allowed once per device (launch_conv1_dw_bf16 does the same for the standalone kernel)
template <int NS>
inline hipError_t cg_conv1_dw_allow()
{
    static bool allowed[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (allowed[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv1_dw_members<NS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c1dw_lds_bytes(NS));
    if (e == hipSuccess) allowed[dev] = true;
    return e;
}

// One trunk launch of a round: kernel k of candle_dqn_cnn_group_plan.hpp at the plan's grid.  ns: n_stack (1 .. CQC_MAX_STACK);
// ipw: conv1's images per workgroup pass (cqc_conv1_ipw); kloop: the members' dxc3_kloop.  hipErrorInvalidValue: no such entry.
inline hipError_t cg_launch(const ConvRound& r, int k, int ns, int ipw, bool kloop, dim3 grid, dim3 block, hipStream_t st)
{
    switch (k) {
    case CQC_K_CONV1_FWD: {
        const auto* a = (const BDR_CONST_AS Conv1Args*)r.c1.d.get();
        switch (ns * 2 + (ipw - 1)) {
#define BDR_CG_C1(N) case N * 2: hipLaunchKernelGGL((k_conv1_img_members<N, 1>), grid, block, 0, st, a); break;
#define BDR_CG_C1X(N) BDR_CG_C1(N) case N * 2 + 1: hipLaunchKernelGGL((k_conv1_img_members<N, 2>), grid, block, 0, st, a); break;
            BDR_CG_C1X(1) BDR_CG_C1X(2) BDR_CG_C1X(3) BDR_CG_C1X(4) BDR_CG_C1(5) BDR_CG_C1(6)
#undef BDR_CG_C1X
#undef BDR_CG_C1
            default: return hipErrorInvalidValue;
        }
        break;
    }
    case CQC_K_CONV2_FWD: hipLaunchKernelGGL((k_igemm_members<FwdC2>), grid, block, 0, st, (const BDR_CONST_AS FwdArgs*)r.f2.d.get(), grid.x); break;
    case CQC_K_CONV3_FWD: hipLaunchKernelGGL((k_igemm_members<FwdC3>), grid, block, 0, st, (const BDR_CONST_AS FwdArgs*)r.f3.d.get(), grid.x); break;
    case CQC_K_CONV3_DW: hipLaunchKernelGGL((k_igemm_red_members<DwC3>), grid, block, 0, st, (const BDR_CONST_AS DwArgs*)r.dw3.d.get()); break;
    case CQC_K_CONV3_DX:
        if (kloop) hipLaunchKernelGGL((k_igemm_members<DxC3PosL, 2, true>), grid, block, 0, st, (const BDR_CONST_AS DxArgs*)r.dx3.d.get(), grid.x / CQC_DXC3_POS);
        else hipLaunchKernelGGL((k_igemm_members<DxC3Pos, 2>), grid, block, 0, st, (const BDR_CONST_AS DxArgs*)r.dx3.d.get(), grid.x / CQC_DXC3_POS);
        break;
    case CQC_K_CONV2_DW: hipLaunchKernelGGL((k_igemm_red_members<DwC2>), grid, block, 0, st, (const BDR_CONST_AS DwArgs*)r.dw2.d.get()); break;
    case CQC_K_CONV2_DX: hipLaunchKernelGGL((k_igemm_members<DxC2MPos, 1>), grid, block, 0, st, (const BDR_CONST_AS DxArgs*)r.dx2.d.get(), grid.x / CQC_DXC2_POS); break;
    case CQC_K_CONV1_DW: {
        const auto* a = (const BDR_CONST_AS Conv1DwArgs*)r.dw1.d.get();
        switch (ns) {
#define BDR_CG_C1DW(N) case N: { const hipError_t e = cg_conv1_dw_allow<N>(); if (e != hipSuccess) return e; \
            hipLaunchKernelGGL(k_conv1_dw_members<N>, grid, block, c1dw_lds_bytes(N), st, a); break; }
            BDR_CG_C1DW(1) BDR_CG_C1DW(2) BDR_CG_C1DW(3) BDR_CG_C1DW(4) BDR_CG_C1DW(5) BDR_CG_C1DW(6)
#undef BDR_CG_C1DW
            default: return hipErrorInvalidValue;
        }
        break;
    }
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

static_assert(CQC_MAX_STACK == C1IMG_MAX_STACK && CQC_MAX_STACK <= C1_MAX_STACK, "candle_dqn_cnn_group_plan.hpp restates conv1's staged-image limit");
static_assert(CQC_DXC3_POS == DxC3Pos::G::IH * DxC3Pos::G::IW && CQC_DXC2_POS == DxC2MPos::NPOS && n_tiles<DxC3Pos>() == 1 && n_tiles<DxC2MPos>() == 2 &&
                  DxC3Pos::WM * DxC3Pos::TM * 32 == 64 && DxC2MPos::WM * DxC2MPos::TM * 32 == 64,
              "candle_dqn_cnn_group_plan.hpp restates the grids of the position-class input gradients");

}  // namespace
