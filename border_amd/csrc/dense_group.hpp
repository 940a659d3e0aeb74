// ================================================================================================
// The group entries of dense.hpp's generic kernels with the member as grid dimension y and the network instance as grid dimension z,
// for launch groupings whose launches have instances (iql_group.hpp: IQL; the end-of-round ticket both groupings share is group_done.hpp).
// Each entry runs the body of the kernel it groups on the member's entry of a device array, read in place through the constant address
// space: member and instance come from blockIdx, so they are uniform and the entry's fields are scalar loads, as they are from the
// kernel-argument segment of the standalone kernel.  Same bodies, same bits.  (BC's own entries, with one instance, stay in bc_group.hpp,
// which does not include this header.)
// Bounds: member = blockIdx.y < gridDim.y = P; launch i of the dense family is handed args + i * P, so it reads entry i * P + member of an
// array of (launches of the family) * P entries; z = blockIdx.z < gridDim.z = nz <= DG_MAXZ, the instances an entry holds.  Inside an
// instance every index is the body's own, with the bounds of the standalone kernel.
#pragma once
#include "dense.hpp"
#include "group_done.hpp"

namespace {

constexpr int DG_MAXZ = 4;
static_assert(DG_MAXZ == RA_INST, "an entry holds the instances of one DenseArgsZ / ReduceAdamArgs launch");
// one member's arguments of one layer (or input-gradient) launch: instance z = blockIdx.z, as DenseArgsZ::a of the standalone launch
struct DenseGroupEntry { DenseArgs a[DG_MAXZ]; };

// a layer (DX = false) or an input gradient (DX = true) of every member's nz networks: grid (the member's own tiles, P, nz)
template <bool DX>
__global__ __launch_bounds__(256) void k_dense_small_members_z(const BDR_CONST_AS DenseGroupEntry* args)
{
    __shared__ float red[4][32][33];
    dense_small_body<DX>(args[blockIdx.y].a[blockIdx.z], red);
}
// the grouped weight gradient of every member: grid (the member's own dW tiles - all jobs of all its instances -, P)
__global__ __launch_bounds__(256) void k_dense_dw_small_members(const BDR_CONST_AS DenseDwSmallGroup* args) { dense_dw_small_group_body(args[blockIdx.y]); }

}  // namespace
