// Parameter arena of the Nature-CNN trunk (conv1 8x8/4, conv2 4x4/2, conv3 3x3/1; border-tch-agent/src/cnn/base.rs:23-36) and the
// conversion of its six conv tensors between the reference's layout and the internal one, and the plan of the conv layers'
// weight-gradient partials (conv_dw_plan).  No HIP in here: the three agents that run
// the trunk (dqn.hip, iqn.hip, candle_dqn.hip) share this one copy, and it is tested on its own with the host compiler
// (tests/test_conv_layout_host.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

namespace bdr {

// floats per image of the trunk's activations (NHWC): conv1 [20][20][32], conv2 [9][9][64], conv3 [7][7][64]
constexpr size_t CONV_A1_ROW = 400 * 32, CONV_A2_ROW = 81 * 64, CONV_A3_ROW = 49 * 64;

// ---- flat parameter arena (internal layouts; every segment 16-byte aligned) ----------------------
//   W1 [64 * n_stack][32]  k=(c,kh,kw)      b1[32]      (n_stack = 4: [256][32])
//   W2 [512][64]  k=(kh,kw,c)      b2[64]
//   W3 [576][64]  k=(kh,kw,c)      b3[64]
//   W4 [3136][512] k=(h,w,c)       b4[512]      (NHWC flatten of conv3's output)
//   W5 [A][512]  (= the reference's [out][in]: k_head reads a lane's 8 columns of an action as two f32x4)   b5[A]
// W4 ... b5 are the tch DQN's head; IQN and the candle DQN use the conv offsets alone (w4 = the conv floats = where their own tail begins).
struct Arena {
    size_t w1, b1, w2, b2, w3, b3, w4, b4, w5, b5, total;  // offsets in floats
    int A;
    int ns;        // AtariCnnConfig::n_stack (cnn/config.rs:14-24): conv1 has 64 * ns rows
    size_t n_w1() const { return (size_t)64 * ns * 32; }
};
inline Arena make_arena(int A, int ns = 4)
{
    Arena a{};
    size_t o = 0;
    auto seg = [&](size_t n) { size_t r = o; o += (n + 3) / 4 * 4; return r; };
    a.ns = ns;
    a.w1 = seg((size_t)64 * ns * 32); a.b1 = seg(32);
    a.w2 = seg(512 * 64); a.b2 = seg(64);
    a.w3 = seg(576 * 64); a.b3 = seg(64);
    a.w4 = seg((size_t)3136 * 512); a.b4 = seg(512);
    a.w5 = seg((size_t)512 * A); a.b5 = seg(A);
    a.total = o; a.A = A;
    return a;
}

// reference order: c1.weight[32][n_stack][8][8] c1.bias c2.weight[64][32][4][4] c2.bias c3.weight[64][64][3][3] c3.bias
inline size_t conv_ref_floats(int ns) { return (size_t)2048 * ns + 32 + 32768 + 64 + 36864 + 64; }

// Every (reference index, internal index) pair of the six conv tensors, in reference order; returns conv_ref_floats(ar.ns).  The one
// place that knows both layouts: conv_to_internal and conv_to_reference below are this walk with the assignment turned round.
template <class F>
inline size_t conv_layout_walk(const Arena& ar, F f)
{
    size_t r = 0;
    const int K1 = 64 * ar.ns;   // (c, kh, kw) of c1.weight[o] is the internal k order
    for (int o = 0; o < 32; ++o) for (int k = 0; k < K1; ++k) f(r + (size_t)o * K1 + k, ar.w1 + (size_t)k * 32 + o);
    r += (size_t)32 * K1; for (int o = 0; o < 32; ++o) f(r + o, ar.b1 + o);
    r += 32;
    for (int o = 0; o < 64; ++o) for (int c = 0; c < 32; ++c) for (int kh = 0; kh < 4; ++kh) for (int kw = 0; kw < 4; ++kw)
        f(r + ((size_t)(o * 32 + c) * 4 + kh) * 4 + kw, ar.w2 + (size_t)((kh * 4 + kw) * 32 + c) * 64 + o);
    r += 32768; for (int o = 0; o < 64; ++o) f(r + o, ar.b2 + o);
    r += 64;
    for (int o = 0; o < 64; ++o) for (int c = 0; c < 64; ++c) for (int kh = 0; kh < 3; ++kh) for (int kw = 0; kw < 3; ++kw)
        f(r + ((size_t)(o * 64 + c) * 3 + kh) * 3 + kw, ar.w3 + (size_t)((kh * 3 + kw) * 64 + c) * 64 + o);
    r += 36864; for (int o = 0; o < 64; ++o) f(r + o, ar.b3 + o);
    return r + 64;
}
// the caller's own tail (l1 / head / cos layer) continues at the returned count of reference floats
inline size_t conv_to_internal(const Arena& ar, const float* ref, float* in) { return conv_layout_walk(ar, [&](size_t r, size_t i) { in[i] = ref[r]; }); }
inline size_t conv_to_reference(const Arena& ar, const float* in, float* ref) { return conv_layout_walk(ar, [&](size_t r, size_t i) { ref[r] = in[i]; }); }

// ---- weight-gradient partials of the three conv layers -------------------------------------------
// A conv layer's dW kernel splits its rows across workgroups and leaves one partial sum per chunk: part[off + chunk * stride + i],
// a chunk = the layer's weights, then its bias (the layer's gradient segment of the arena, n floats at w).  The buffer is laid out
// for the batch CAPACITY; a batch of Bn <= capacity images fills the first chunks(Bn) chunks of each layer, and the reduction behind
// the dW launch sums exactly those.  The one place that knows the split: the dW launches and every reduction read it from here.
constexpr float INV255 = 1.0f / 255.0f;   // cnn/base.rs:26 "/ 255": conv1's kernels multiply raw u8 operands
struct ConvDwLayer {
    size_t off, stride;   // floats: the layer's partials in the partial buffer, and one chunk of them
    int allocated;        // chunks the buffer holds
    int rows;             // GEMM rows per image that 32-row tiles split into chunks (0: conv1, one partial per workgroup, workgroups stride over the images)
    int n, n_weights;     // floats of the gradient segment (= stride), the weights among them
    size_t w;             // arena offset of the segment
    float wscale;         // applied to the weights' sums
    int wgs;              // dW workgroups per chunk
    int chunks(int Bn) const { return std::min(allocated, rows ? (Bn * rows + 31) / 32 : Bn); }
};
struct ConvDwPlan { ConvDwLayer layer[3]; size_t total; };   // [0] conv1, [1] conv2, [2] conv3; total floats of the partial buffer
inline ConvDwPlan conv_dw_plan(const Arena& ar, int B)
{
    ConvDwPlan p{};
    const int cap[3] = {256, 64, 56}, rows[3] = {0, 81, 49}, nw[3] = {(int)ar.n_w1(), 512 * 64, 576 * 64}, nb[3] = {32, 64, 64}, wgs[3] = {1, 8, 9};
    const size_t seg[3] = {ar.w1, ar.w2, ar.w3};
    // diagnostics (A/B of the partial-sum traffic): BDR_DW_CHUNKS="c1,c2,c3" caps the three counts (c2 / c3: multiples of 8 keep the XCD map)
    int env[3] = {0, 0, 0};
    if (const char* e = getenv("BDR_DW_CHUNKS")) { if (sscanf(e, "%d,%d,%d", &env[0], &env[1], &env[2]) != 3) env[0] = env[1] = env[2] = 0; }
    for (int k = 0; k < 3; ++k) {
        ConvDwLayer& l = p.layer[k];
        l.rows = rows[k]; l.allocated = cap[k];
        l.allocated = l.chunks(B);
        if (env[k] > 0) l.allocated = std::min(l.allocated, env[k]);
        l.n_weights = nw[k]; l.n = nw[k] + nb[k]; l.stride = (size_t)l.n;
        l.w = seg[k]; l.wscale = k == 0 ? INV255 : 1.0f; l.wgs = wgs[k];
        l.off = p.total;
        p.total += l.allocated * l.stride;
    }
    return p;
}

}  // namespace bdr
