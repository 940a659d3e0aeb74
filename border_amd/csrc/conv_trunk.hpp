// Host driver of the Nature-CNN trunk on ONE stream, for the agents that run it layer by layer (iqn.hip's psi, candle_dqn.hip's
// AtariCnn form): the forward of nz network instances with one launch per layer, and the backward chain conv3 dW, conv3 dX,
// conv2 dW, conv2 dX, conv1 dW.  Kernels, policies and the dW chunk plan are cnn_layers.hpp's; the buffers are the caller's
// (CONV_A1_ROW / CONV_A2_ROW / CONV_A3_ROW floats per image, dw_plan(B, ns).total floats of partials).
#pragma once
#include "conv1_bf16_img.hpp"
#include "cnn_layers.hpp"

namespace {

// conv1 of nz (parameters, u8 rows) instances into a1[z]
inline int32_t trunk_conv1(bdr_agent* a, const Arena& conv, int nz, const float* const* pp, const uint8_t* const* rows, float* const* a1, int Bn, const char* label)
{
    Conv1Args c{}; c.M = Bn * 400; c.nz = nz;
    for (int z = 0; z < nz; ++z) { c.x[z] = rows[z]; c.w1[z] = pp[z] + conv.w1; c.bias[z] = pp[z] + conv.b1; c.out[z] = a1[z]; }
    Bracket br(a, label);
    BDR_HIP(conv1_forward(conv.ns, Bn, a->stream, c));
    return BDR_OK;
}
// conv2 and conv3 behind it: a1[z] -> a2[z] -> a3[z]  (apart from conv1: IQN's small acting batches take act_small.hpp's kernels here)
inline int32_t trunk_conv23(bdr_agent* a, const Arena& conv, int nz, const float* const* pp, float* const* a1, float* const* a2, float* const* a3, int Bn,
                            const char* label2, const char* label3)
{
    FwdArgs f2{}, f3{}; f2.M = Bn * 81; f3.M = Bn * 49;
    for (int z = 0; z < nz; ++z) {
        f2.x[z] = a1[z]; f2.w[z] = pp[z] + conv.w2; f2.bias[z] = pp[z] + conv.b2; f2.out[z] = a2[z];
        f3.x[z] = a2[z]; f3.w[z] = pp[z] + conv.w3; f3.bias[z] = pp[z] + conv.b3; f3.out[z] = a3[z];
    }
    { Bracket br(a, label2); LAUNCH(k_igemm<FwdC2>, dim3((f2.M + 63) / 64, 1, nz), f2); }
    { Bracket br(a, label3); LAUNCH(k_igemm<FwdC3>, dim3((f3.M + 63) / 64, 1, nz), f3); }
    return BDR_OK;
}

// The backward of Bn images: dy3 (in) is the gradient at conv3's pre-activation; dy2 / dy1 are scratch; p the online parameters; B the
// capacity part_conv was allocated for (dw_plan).  after_dw(k, chunks, part, stride) runs right behind layer k's dW launch (k = 2, 1, 0
// for conv3, conv2, conv1) with that layer's partial sums: part[chunk * stride + i], a chunk = the layer's weights, then its bias.
// Brackets: <prefix>conv3_dw, conv3_dx, conv2_dw, conv2_dx, conv1_dw.
template <class Hook>
inline int32_t trunk_backward(bdr_agent* a, const Arena& conv, const float* p, const uint8_t* obs, const float* a1, const float* a2, const float* dy3, float* dy2,
                              float* dy1, float* part_conv, int Bn, int B, const char* prefix, Hook&& after_dw)
{
    const DwPlan pl = dw_plan(B, conv.ns);
    auto label = [&](const char* s) { return std::string(prefix) + s; };
    {
        const int Mr = Bn * 49, chunks = std::min(pl.chunks_c3, (Mr + 31) / 32);
        DwArgs d{a2, dy3, part_conv + pl.off_c3, pl.stride_c3, Mr};
        { Bracket br(a, label("conv3_dw").c_str()); LAUNCH(k_igemm_red<DwC3>, dim3(9 * chunks), d); }
        BDR_TRY(after_dw(2, chunks, part_conv + pl.off_c3, pl.stride_c3));
    }
    {   // position-class tiles (cnn_layers.hpp DxC3PosP: only the taps that reach a valid output; bit-identical to the flat row tiles)
        DxArgs d{dy3, p + conv.w3, a2, dy2, Bn * 81, nullptr, 0};
        Bracket br(a, label("conv3_dx").c_str());
        BDR_HIP((launch_igemm<DxC3Pos, 2>(a->stream, dxc3_pos_grid<DxC3Pos>(Bn), d)));
    }
    {
        const int Mr = Bn * 81, chunks = std::min(pl.chunks_c2, (Mr + 31) / 32);
        DwArgs d{a1, dy2, part_conv + pl.off_c2, pl.stride_c2, Mr};
        { Bracket br(a, label("conv2_dw").c_str()); LAUNCH(k_igemm_red<DwC2>, dim3(8 * chunks), d); }
        BDR_TRY(after_dw(1, chunks, part_conv + pl.off_c2, pl.stride_c2));
    }
    {   // the four parity classes as one GEMM over position-class tiles (DxC2MPosP), as the tch DQN's step
        DxArgs d{dy2, p + conv.w2, a1, dy1, Bn * 100, nullptr, 0};
        Bracket br(a, label("conv2_dx").c_str());
        BDR_HIP((launch_igemm<DxC2MPos, 1>(a->stream, dxc2_pos_grid<DxC2MPos>(Bn), d)));
    }
    {
        const int chunks = std::min(pl.chunks_c1, Bn);
        Conv1DwArgs d{obs, dy1, part_conv + pl.off_c1, pl.stride_c1, Bn};
        { Bracket br(a, label("conv1_dw").c_str()); BDR_HIP(launch_conv1_dw_bf16(conv.ns, dim3(chunks), a->stream, d)); }
        BDR_TRY(after_dw(0, chunks, part_conv + pl.off_c1, pl.stride_c1));
    }
    return BDR_OK;
}

}  // namespace
