// Host driver of the Nature-CNN trunk on ONE stream, for the agents that run it layer by layer (iqn.hip's psi, candle_dqn.hip's
// AtariCnn form): the forward of nz network instances with one launch per layer, and the backward chain conv3 dW, conv3 dX,
// conv2 dW, conv2 dX, conv1 dW.  Kernels and policies are cnn_layers.hpp's, the plan of the dW partials is conv_layout.hpp's; the
// buffers are the caller's (CONV_A1_ROW / CONV_A2_ROW / CONV_A3_ROW floats per image, conv_dw_plan(conv, B).total floats of partials).
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
// capacity part_conv was allocated for (conv_dw_plan).  after_dw(layer, chunks, part) runs right behind each layer's dW launch (conv3,
// conv2, conv1) with the plan's entry of that layer and its partial sums: part[chunk * layer.stride + i], chunk < chunks.
// Brackets: <prefix>conv3_dw, conv3_dx, conv2_dw, conv2_dx, conv1_dw.
template <class Hook>
inline int32_t trunk_backward(bdr_agent* a, const Arena& conv, const float* p, const uint8_t* obs, const float* a1, const float* a2, const float* dy3, float* dy2,
                              float* dy1, float* part_conv, int Bn, int B, const char* prefix, Hook&& after_dw)
{
    const ConvDwPlan pl = conv_dw_plan(conv, B);
    auto label = [&](const char* s) { return std::string(prefix) + s; };
    {
        const ConvDwLayer& l = pl.layer[2];
        DwArgs d{a2, dy3, part_conv + l.off, l.stride, Bn * 49};
        { Bracket br(a, label("conv3_dw").c_str()); LAUNCH(k_igemm_red<DwC3>, dim3(l.wgs * l.chunks(Bn)), d); }
        BDR_TRY(after_dw(l, l.chunks(Bn), d.part));
    }
    {   // position-class tiles (cnn_layers.hpp DxC3PosP: only the taps that reach a valid output; bit-identical to the flat row tiles)
        DxArgs d{dy3, p + conv.w3, a2, dy2, Bn * 81, nullptr, 0};
        Bracket br(a, label("conv3_dx").c_str());
        if (a->dxc3_kloop) BDR_HIP((launch_igemm<DxC3PosL, 2, true>(a->stream, dxc3_pos_grid<DxC3PosL>(Bn), d)));   // (igemm.hpp: ADxS1PosLean, PEEL; BDR_DXC3_KLOOP=0: the form before them)
        else BDR_HIP((launch_igemm<DxC3Pos, 2>(a->stream, dxc3_pos_grid<DxC3Pos>(Bn), d)));
    }
    {
        const ConvDwLayer& l = pl.layer[1];
        DwArgs d{a1, dy2, part_conv + l.off, l.stride, Bn * 81};
        { Bracket br(a, label("conv2_dw").c_str()); LAUNCH(k_igemm_red<DwC2>, dim3(l.wgs * l.chunks(Bn)), d); }
        BDR_TRY(after_dw(l, l.chunks(Bn), d.part));
    }
    {   // the four parity classes as one GEMM over position-class tiles (DxC2MPosP), as the tch DQN's step
        DxArgs d{dy2, p + conv.w2, a1, dy1, Bn * 100, nullptr, 0};
        Bracket br(a, label("conv2_dx").c_str());
        BDR_HIP((launch_igemm<DxC2MPos, 1>(a->stream, dxc2_pos_grid<DxC2MPos>(Bn), d)));
    }
    {
        const ConvDwLayer& l = pl.layer[0];
        Conv1DwArgs d{obs, dy1, part_conv + l.off, l.stride, Bn};
        { Bracket br(a, label("conv1_dw").c_str()); BDR_HIP(launch_conv1_dw_bf16(conv.ns, dim3(l.wgs * l.chunks(Bn)), a->stream, d)); }
        BDR_TRY(after_dw(l, l.chunks(Bn), d.part));
    }
    return BDR_OK;
}

}  // namespace
