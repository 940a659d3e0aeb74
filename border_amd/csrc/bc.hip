// BC (behaviour cloning) agent on MI355X: Bc::opt_ (border-candle-agent/src/bc/base.rs:167-198): loss = mse(policy(obs), act) - the mean of
// the squared differences over all B x A elements - backward and one optimizer step on the policy, a plain Mlp (mlp/base.rs,
// mlp.rs:14-24: ReLU after every layer but the last, activation_out after the last; lib.rs:58-74 None | ReLU | Tanh | Sigmoid).  No
// critic, no target, no noise; the record holds "loss" (:191-193).  Policy::sample (:49-59): Continuous returns the network output,
// Discrete the argmax over the last dimension as i64; the Discrete update is a panic in the reference (:174) and an error here.
// train() / eval() do nothing and is_train() is false (:104-112).
// Hidden layers, the grouped weight gradient and the fused reduce + Adam are dense.hpp's FP32-MFMA kernels, unchanged, driven by
// DenseAgent (dense_agent.hpp), the host core BC shares with IQL and AWAC: this file holds BC's kernels, the dispatch of its three
// kernel forms, its record, its sample and its entry points.  BC's own kernels:
//   k_bc_loss   (general form) y = act_out(z), the loss, dL/dz from the last layer's pre-activation z [B][Np]
//   k_bc_head   (fused form, out_dim <= 64) the last layer's forward, y, the loss, dL/dz and the last layer's input gradient in one
//               row-block launch, the layer's weights staged in LDS once per workgroup
//   k_bc_head_mfma  the same on the FP32 MFMA: 32 rows per workgroup, dense.hpp's 32 x 32 tiles, the weights read from L2
//   k_bc_act    Policy::sample: the output activation (Continuous) or the row-wise argmax (Discrete)
// One update, general form: pack, L forwards, k_bc_loss, L-1 input gradients, the grouped dW, reduce + Adam (3L + 2 launches);
// fused form: pack, L-1 forwards, k_bc_head, L-2 input gradients, the grouped dW, reduce + Adam (3L - 1 launches).
// Every sum has one order, so an update gives the same bits run to run and agent to agent.  The loss: per row the squared
// differences added in column order; then candle_actor.hpp's batch order (rows in blocks of 32, a butterfly per block, the block
// partials added in block order), formed by the launch's last workgroup from per-row sums - no workgroup waits for another, and no
// float atomics.  The two forms form the last layer's dot products in different orders and need not agree bitwise.
// k_bc_loss, k_bc_head_mfma (and dense.hpp's k_pack_rows) are bodies over their argument structs with the entries calling them: bc_group.hpp
// (included below) runs the same bodies for P agents of one shape per launch, the member index in grid dimension y.
#include <algorithm>
#include <cstdlib>

#include "candle_actor.hpp"
#include "bc_group_plan.hpp"

using namespace bdr;

namespace {

// one output element: y = act_out(z), d = y - a; sq = d^2; dz = 2 d inv_n * act_out'(z)
__device__ __forceinline__ void bc_elem(int kind, float z, float a, float inv_n, float& y, float& dz, float& sq)
{
#pragma clang fp contract(off)
    float gp = 1.f;
    y = z;
    if (kind == BDR_ACTIVATION_RELU) { y = z > 0.f ? z : 0.f; gp = z > 0.f ? 1.f : 0.f; }
    else if (kind == BDR_ACTIVATION_TANH) { y = tanhf(z); const float yy = y * y; gp = 1.f - yy; }
    else if (kind == BDR_ACTIVATION_SIGMOID) { const float e = expf(-z); y = 1.f / (1.f + e); gp = y * (1.f - y); }
    const float d = y - a;
    sq = d * d;
    const float g = 2.f * d;
    const float gs = g * inv_n;
    dz = gs * gp;
}
// (bc_act_out and bc_argmax, the element code of Policy::sample, live in dense_act.hpp: k_dense_act calls them too)

// The launch's last workgroup (256 threads): the per-row sums in candle::row_sum's order - blocks of 32 rows, a butterfly per
// block, the partials added in block order (the order does not depend on the workgroup's size) - into the record slot.
// rowsq was written with agent-scope stores by every workgroup before its ticket (dense.hpp last_workgroup).
__device__ __forceinline__ void bc_finish_loss(const float* rowsq, int B, float* scal, int accumulate, float inv_n, float* red8)
{
    float total = 0.f;
    for (int base = 0; base < B; base += 256) {
        const int b = base + (int)threadIdx.x;
        const float part = candle::butterfly32(b < B ? ld_agent(rowsq + b) : 0.f);
        if ((threadIdx.x & 31) == 0) red8[threadIdx.x >> 5] = part;
        __syncthreads();
        const int nb = min(8, (B - base + 31) / 32);
        for (int k = 0; k < nb; ++k) total += red8[k];
        __syncthreads();
    }
    if (threadIdx.x == 0) scal[0] = candle::acc(accumulate ? scal[0] : 0.f, total, inv_n);
}

// ---- general form -----------------------------------------------------------------------------------------------------------------
// z [B][ld] (ld = pad64(A)), act [B][A].  Workgroup w owns rows [32 w, 32 w + 32): y -> pred, dL/dz -> dz (both [B][ld], padding
// columns zero), the row sums -> rowsq.  Bounds: rows b < B and columns j < ld only; sq holds 32 x (ld + 1) floats, ld <= 256.
struct BcLossArgs {
    const float* z; int ld; const float* act; int A, B, kind;
    float* pred; float* dz; float* rowsq; unsigned* ticket; float* scal; int accumulate; float inv_n;
};
// (the body over its argument struct: the kernel argument, or a member's entry of a device array read in place - bc_group.hpp, where
// gridDim.x is still the member's own workgroup count and the ticket the member's own)
template <class Args>
__device__ __forceinline__ void bc_loss_body(const Args& p)
{
    __shared__ float sq[32 * 257];
    __shared__ float red8[8];
    __shared__ unsigned s_flag;
    const int r0 = (int)blockIdx.x * 32, ls = p.ld + 1;
    for (int t = threadIdx.x; t < 32 * p.ld; t += 256) {
        const int r = t / p.ld, j = t % p.ld, b = r0 + r;
        float y = 0.f, g = 0.f, s = 0.f;
        if (b < p.B && j < p.A) bc_elem(p.kind, p.z[(size_t)b * p.ld + j], p.act[(size_t)b * p.A + j], p.inv_n, y, g, s);
        sq[r * ls + j] = s;
        if (b < p.B) { p.pred[(size_t)b * p.ld + j] = y; p.dz[(size_t)b * p.ld + j] = g; }
    }
    __syncthreads();
    if (threadIdx.x < 32 && r0 + (int)threadIdx.x < p.B) {
        float s = 0.f;
        for (int j = 0; j < p.A; ++j) s += sq[threadIdx.x * ls + j];
        st_agent(p.rowsq + r0 + threadIdx.x, s);
    }
    if (last_workgroup(p.ticket, gridDim.x, &s_flag)) bc_finish_loss(p.rowsq, p.B, p.scal, p.accumulate, p.inv_n, red8);
}
__global__ __launch_bounds__(256) void k_bc_loss(BcLossArgs p) { bc_loss_body(p); }

// ---- fused form -------------------------------------------------------------------------------------------------------------------
// h [B][K] the last hidden activation (post-ReLU, K = its padded width), w [K][64] + bias [64] the last layer (out_dim <= 64).
// Workgroup g owns rows [R g, R g + R):  z = h w + bias (k ascending, then the bias), y, dL/dz, the row sums, and
// dL/dh[b][k] = [h > 0] sum_n dz[b][n] w[k][n] (n ascending).  y -> pred, dL/dz -> dz ([B][64], padding columns zero: the grouped
// dW launch reads them), dL/dh -> dx [B][K].
// LDS (dynamic, floats): ws [K][65] the weights (row stride 65: the forward reads a row across lanes, dX a column across lanes, both
// without bank conflicts) | hs [R][K] | dzt [64][R] | sq [R][65] | red8 [8] | flag.  bc_head_lds() is the size; the host refuses
// shapes beyond 160 KB.  Bounds: rows are clamped to B - 1 when loaded and stored only for b < B; k < K; n < 64.
struct BcHeadArgs {
    const float* h; int K; const float* w; const float* bias; const float* act; int A, B, kind;
    float* pred; float* dz; float* dx; float* rowsq; unsigned* ticket; float* scal; int accumulate; float inv_n;
};
constexpr int BC_HEAD_ROWS_DEFAULT = 8;   // measured at the bc_pen shape: 8 rows 22.9k updates/s, 16 rows 21.1k, 32 rows 17.1k (profiles/bench_bc_pen.json)
// (BDR_BC_KERNEL_DEFAULT and the MFMA head's conditions: bc_resolve_form / bc_can_mfma, bc_group_plan.hpp - the group reads the same rule)
inline size_t bc_head_lds(int K, int R) { return ((size_t)K * 65 + (size_t)R * K + 64 * (size_t)R + (size_t)R * 65 + 8 + 4) * sizeof(float) + 64; }
template <int R>
__global__ __launch_bounds__(256) void k_bc_head(BcHeadArgs p)
{
    extern __shared__ __attribute__((aligned(16))) float bc_lds[];
    const int K = p.K, tid = threadIdx.x;
    // carve: hs first (16-byte aligned rows for the b128 broadcast reads), then dzt (also read as b128), then the scalar-read parts
    float* hs = bc_lds;
    float* dzt = hs + (size_t)R * K;
    float* ws = dzt + 64 * R;
    float* sq = ws + (size_t)K * 65;
    float* red8 = sq + R * 65;
    unsigned* s_flag = reinterpret_cast<unsigned*>(red8 + 8);
    const int r0 = (int)blockIdx.x * R;
    for (int i = tid; i < K * 16; i += 256) {   // K x 64 weights, four columns per load
        const f32x4 v = *reinterpret_cast<const f32x4*>(p.w + (size_t)i * 4);
        float* d = ws + (i >> 4) * 65 + (i & 15) * 4;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    const int K4 = K / 4;
    for (int i = tid; i < R * K4; i += 256) {
        const int r = i / K4, q = i % K4;
        *reinterpret_cast<f32x4*>(hs + (size_t)r * K + q * 4) = *reinterpret_cast<const f32x4*>(p.h + (size_t)min(r0 + r, p.B - 1) * K + q * 4);
    }
    __syncthreads();
    // forward: lane -> column n, wave -> RW rows
    constexpr int RW = R / 4;
    const int n = tid & 63, rw0 = (tid >> 6) * RW;
    float acc[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) acc[i] = 0.f;
    for (int k = 0; k < K; k += 4) {
        const float w0 = ws[(k + 0) * 65 + n], w1 = ws[(k + 1) * 65 + n], w2 = ws[(k + 2) * 65 + n], w3 = ws[(k + 3) * 65 + n];
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(hs + (size_t)(rw0 + i) * K + k);
            acc[i] = fmaf(hv[0], w0, acc[i]); acc[i] = fmaf(hv[1], w1, acc[i]); acc[i] = fmaf(hv[2], w2, acc[i]); acc[i] = fmaf(hv[3], w3, acc[i]);
        }
    }
    const float bias = p.bias[n];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        const int r = rw0 + i, b = r0 + r;
        float y = 0.f, g = 0.f, s = 0.f;
        if (b < p.B && n < p.A) bc_elem(p.kind, acc[i] + bias, p.act[(size_t)b * p.A + n], p.inv_n, y, g, s);
        dzt[n * R + r] = g;
        sq[r * 65 + n] = s;
        if (b < p.B) { p.pred[(size_t)b * 64 + n] = y; p.dz[(size_t)b * 64 + n] = g; }
    }
    __syncthreads();
    if (tid < R && r0 + tid < p.B) {
        float s = 0.f;
        for (int j = 0; j < p.A; ++j) s += sq[tid * 65 + j];
        st_agent(p.rowsq + r0 + tid, s);
    }
    ticket_take(p.ticket, gridDim.x, s_flag);   // the answer is read after the input gradient: the ticket's round trip hides behind it
    // input gradient: thread -> column k of the hidden layer, all R rows
    for (int k = tid; k < K; k += 256) {
        float dxv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) dxv[r] = 0.f;
        for (int j = 0; j < p.A; ++j) {
            const float wv = ws[k * 65 + j];
#pragma unroll
            for (int r4 = 0; r4 < R; r4 += 4) {
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(dzt + j * R + r4);
#pragma unroll
                for (int u = 0; u < 4; ++u) dxv[r4 + u] = fmaf(g4[u], wv, dxv[r4 + u]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r0 + r < p.B) p.dx[(size_t)(r0 + r) * K + k] = hs[(size_t)r * K + k] > 0.f ? dxv[r] : 0.f;
    }
    if (ticket_last(s_flag)) bc_finish_loss(p.rowsq, p.B, p.scal, p.accumulate, p.inv_n, red8);
}

// ---- fused form on the FP32 MFMA ----------------------------------------------------------------------------------------------------
// The same work as k_bc_head for a block of 32 rows, both products as dense.hpp's 32 x 32 MFMA tiles and the weights read from
// global memory (L2) instead of staged in LDS.  Forward: NT column tiles (NT = 1 for act_dim <= 32, else 2) through
// dense_small_tile / dense_small_sum - the tile k_dense_small forms, so z has the general form's bits - then the bias.  Input
// gradient: wave w owns the 32-column tiles w, w + 4, ... of the hidden layer; A = dz rows from LDS, B = weight rows (contiguous
// in n), reduced over n ascending in quads, the two lane halves taking alternate quads.
// Bounds: rows clamped to B - 1 when loaded, stored for b < B only; k < K (K % 64 == 0); n < 32 NT <= 64.
// (the body over its argument struct, as bc_loss_body)
template <int NT, class Args>
__device__ __forceinline__ void bc_head_mfma_body(const Args& p)
{
    constexpr int NC = NT * 32;
    __shared__ float red[4][32][33];
    __shared__ __attribute__((aligned(16))) float dzs[32][NC + 4];
    __shared__ float sq[32][NC + 1];
    __shared__ float red8[8];
    __shared__ unsigned s_flag;
    const int K = p.K, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int r0 = (int)blockIdx.x * 32;
    const float* arow = p.h + (size_t)min(r0 + i, p.B - 1) * K;
    const int r = tid >> 3, c4 = (tid & 7) * 4, b = r0 + r;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        dense_small_tile<false>([&](int k) { return *reinterpret_cast<const f32x4*>(arow + k); }, p.w, 64, t * 32, K, wave, lane, red);
        __syncthreads();
        f32x4 y4 = {0.f, 0.f, 0.f, 0.f}, g4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = t * 32 + c4 + q;
            const float z = dense_small_sum(red, r, c4 + q) + p.bias[n];
            float y = 0.f, g = 0.f, s = 0.f;
            if (b < p.B && n < p.A) bc_elem(p.kind, z, p.act[(size_t)b * p.A + n], p.inv_n, y, g, s);
            dzs[r][n] = g; sq[r][n] = s; y4[q] = y; g4[q] = g;
        }
        if (b < p.B) {
            *reinterpret_cast<f32x4*>(p.pred + (size_t)b * 64 + t * 32 + c4) = y4;
            *reinterpret_cast<f32x4*>(p.dz + (size_t)b * 64 + t * 32 + c4) = g4;
            if (NT == 1) {   // columns 32 .. 63 of the padded rows: zero (the grouped dW launch reads them)
                const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(p.pred + (size_t)b * 64 + 32 + c4) = z4;
                *reinterpret_cast<f32x4*>(p.dz + (size_t)b * 64 + 32 + c4) = z4;
            }
        }
        __syncthreads();   // red is the next tile's
    }
    if (tid < 32 && r0 + tid < p.B) {
        float s = 0.f;
        for (int j = 0; j < p.A; ++j) s += sq[tid][j];
        st_agent(p.rowsq + r0 + tid, s);
    }
    ticket_take(p.ticket, gridDim.x, &s_flag);   // the answer is read after the input gradient
    for (int kt = wave; kt < K / 32; kt += 4) {
        const float* wrow = p.w + (size_t)(kt * 32 + i) * 64;
        f32x4 av[NC / 8], bv[NC / 8];
#pragma unroll
        for (int c = 0; c < NC / 8; ++c) {
            bv[c] = *reinterpret_cast<const f32x4*>(wrow + 8 * c + 4 * h);
            av[c] = *reinterpret_cast<const f32x4*>(&dzs[i][8 * c + 4 * h]);
        }
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int c = 0; c < NC / 8; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c][q], bv[c][q], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int bb = r0 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (bb < p.B) {
                const size_t o = (size_t)bb * K + kt * 32 + i;
                p.dx[o] = p.h[o] > 0.f ? acc[e] : 0.f;
            }
        }
    }
    if (ticket_last(&s_flag)) bc_finish_loss(p.rowsq, p.B, p.scal, p.accumulate, p.inv_n, red8);
}
template <int NT>
__global__ __launch_bounds__(256) void k_bc_head_mfma(BcHeadArgs p) { bc_head_mfma_body<NT>(p); }

// Policy::sample (bc/base.rs:49-59) from the last layer's pre-activation z [n][ld].  Continuous: out [n][A] = act_out(z).  Discrete:
// idx [n] = argmax_j act_out(z[b][j]), the lowest index among equal values (candle's tie order is not pinned by anything that can be
// run against; ReLU outputs tie at 0).
struct BcActArgs { const float* z; int ld, A, n, kind, discrete; float* out; long long* idx; };
__global__ __launch_bounds__(256) void k_bc_act(BcActArgs p)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (p.discrete) {
        if (t >= p.n) return;
        p.idx[t] = bc_argmax(p.kind, p.z + (size_t)t * p.ld, p.A);
        return;
    }
    if (t >= p.n * p.A) return;
    const int b = t / p.A, j = t % p.A;
    p.out[t] = bc_act_out(p.kind, p.z[(size_t)b * p.ld + j]);
}

}  // namespace

// ================================================================================================
// The buffer lifetimes, the layer-by-layer forward, the backward step, the observation rows of an acting call and the reference
// layout are DenseAgent's (dense_agent.hpp); BC adds its one model, the loss / head kernels' dispatch, its record and its sample.
struct Bc : DenseAgent {
    bdr_bc_config cfg;
    MlpLayout net;                     // the policy; its last layer is built without activation (z), act_out is applied by BC's kernels
    float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;   // arenas: parameters, gradients, exp_avg, exp_avg_sq
    uint64_t step = 0;
    int form = BDR_BC_KERNEL_GENERAL; bool head_attr = false; int head_rows = 0; size_t head_lds = 0;
    // batch buffers
    int B = 0; uint64_t batch_gen = 0;          // batch_gen: bumped whenever the batch buffers are re-allocated (bc_group.hpp keys its static arguments on it)
    float* x0 = nullptr;                        // [B][Kp] padded observations
    std::vector<float*> act, dy;                // activations (the last: z) and gradients per layer
    float *pred = nullptr, *rowsq = nullptr, *part = nullptr, *samp = nullptr; long long* samp_idx = nullptr;
    std::vector<size_t> off;
    unsigned* ticket = nullptr;
    float* scal = nullptr;                      // [0] loss
    float *u_obs = nullptr, *u_act = nullptr; uint64_t u_cap = 0;
    int last_B = 0;

    int32_t ensure_batch(int Bn)
    {
        if (Bn <= B) return BDR_OK;
        BDR_HIP(hipStreamSynchronize(stream));
        release(BATCH);
        B = 0;
        BDR_TRY(alloc(&x0, (size_t)Bn * net.L[0].Kp, BATCH));
        BDR_TRY(layer_bufs(net, Bn, act)); BDR_TRY(layer_bufs(net, Bn, dy));
        BDR_TRY(alloc(&pred, (size_t)Bn * net.L.back().Np, BATCH));
        BDR_TRY(alloc(&rowsq, Bn, BATCH));
        BDR_TRY(alloc(&part, plan(net, Bn, off), BATCH));
        BDR_TRY(alloc(&samp, (size_t)Bn * A, BATCH));
        BDR_TRY(alloc(&samp_idx, Bn, BATCH));
        B = Bn; batch_gen += 1;
        return BDR_OK;
    }
    // layers [0, upto) of Bn rows of x0
    int32_t forward(int upto, int Bn, const char* name)
    {
        const float* pp[1] = {p}; const float* xs[1] = {x0}; std::vector<float*>* as[1] = {&act};
        return mlp_forward(net, 1, pp, xs, as, Bn, name, upto);
    }
    template <int R>
    int32_t launch_head(const BcHeadArgs& a, int Bn)
    {
        if (!head_attr) {   // more than 64 KB of dynamic LDS has to be asked for, once per agent (and so per device)
            BDR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bc_head<R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)head_lds));
            head_attr = true;
        }
        hipLaunchKernelGGL(k_bc_head<R>, dim3((Bn + R - 1) / R), dim3(256), head_lds, stream, a);
        BDR_HIP(hipGetLastError());
        return BDR_OK;
    }
    // Bc::opt_ (bc/base.rs:167-198) on device-resident rows: obs [Bn][O], data [Bn][A]
    int32_t update(int Bn, const float* obs, const float* data)
    {
        BDR_TRY(ensure_batch(Bn));
        const int L = (int)net.L.size();
        const DenseLayer& last = net.L[L - 1];
        const float inv_n = (float)(1.0 / ((double)Bn * (double)A));
        { Bracket br(this, "pack"); BDR_TRY(pack_rows(stream, obs, O, O, x0, net.L[0].Kp, 0, Bn)); }
        int lo;   // input gradients still to form: layers lo .. 1
        if (form != BDR_BC_KERNEL_GENERAL) {
            BDR_TRY(forward(L - 1, Bn, "fwd"));
            BcHeadArgs a{act[L - 2], last.Kp, p + last.w, p + last.b, data, A, Bn, cfg.policy.activation_out,
                         pred, dy[L - 1], dy[L - 2], rowsq, ticket, scal, 0, inv_n};
            Bracket br(this, "bc_head");
            if (form == BDR_BC_KERNEL_FUSED_MFMA) {
                if (A <= 32) BDR_HIP(step_launch(stream, false, k_bc_head_mfma<1>, dim3((Bn + 31) / 32), dim3(256), a));
                else BDR_HIP(step_launch(stream, false, k_bc_head_mfma<2>, dim3((Bn + 31) / 32), dim3(256), a));
            } else {
                BDR_TRY(head_rows == 8 ? launch_head<8>(a, Bn) : head_rows == 32 ? launch_head<32>(a, Bn) : launch_head<16>(a, Bn));
            }
            lo = L - 2;
        } else {
            BDR_TRY(forward(L, Bn, "fwd"));
            BcLossArgs a{act[L - 1], last.Np, data, A, Bn, cfg.policy.activation_out, pred, dy[L - 1], rowsq, ticket, scal, 0, inv_n};
            Bracket br(this, "bc_loss");
            BDR_HIP(step_launch(stream, false, k_bc_loss, dim3((Bn + 31) / 32), dim3(256), a));
            lo = L - 1;
        }
        step += 1;
        const AdamScalars sc = opt_scalars(cfg.opt, cfg.lr, step);
        std::vector<float*>* acts[1] = {&act}; std::vector<float*>* dys[1] = {&dy};
        // no targets: nz = 1, no instance stride, track == 0, and a tau the kernel does not read (dense.hpp k_dense_reduce_adam)
        BDR_TRY(mlp_backward_step(net, 1, &p, &g, &m, &v, nullptr, x0, acts, dys, part, 0, off, &sc, Bn, {"dx", "dw", "reduce_adam"}, net.total, 0.0, lo));
        n_opts += 1;
        last_B = Bn;
        return BDR_OK;
    }
    int32_t refuse_discrete() const
    {
        return cfg.action_type == BDR_BC_ACTION_DISCRETE
                   ? fail(BDR_ERR_INVALID, "BC has no update for BcActionType::Discrete: the reference's opt_ panics there (bc/base.rs:174)")
                   : BDR_OK;
    }

    bool has_train_mode() const override { return false; }   // bc/base.rs:104-112
    const char* kind() const override { return "bc"; }
    int32_t opt(bdr_replay* r) override
    {
        BDR_TRY(refuse_discrete());
        BDR_TRY(check_replay(r, "BC"));
        const int Bn = (int)cfg.batch_size;
        BDR_TRY(ensure_batch(Bn));
        { Bracket br(this, "sample"); BDR_TRY(replay_sample_on_stream(r, Bn, stream)); }
        return update(Bn, (const float*)r->b_obs, (const float*)r->b_act);
    }
    void record_keys(std::vector<std::string>& keys) override { keys = {"loss"}; }
    int32_t record(float* out, int cap, int* n) override
    {
        if (cap < 1) return fail(BDR_ERR_INVALID, "BC record needs 1 slot");
        BDR_HIP(hipMemcpyAsync(out, scal, 4, hipMemcpyDeviceToHost, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        *n = 1;
        return BDR_OK;
    }

    // Policy::sample of n observation rows (host rows, or device rows inside sample_device)
    int32_t sample(uint64_t n, const float* obs, float* act_out, int64_t* idx_out)
    {
        const bool disc = cfg.action_type == BDR_BC_ACTION_DISCRETE;
        BDR_REQUIRE(disc ? idx_out != nullptr : act_out != nullptr, "BC sample: a %s agent writes %s", disc ? "Discrete" : "Continuous", disc ? "idx_out" : "act_out");
        BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
        if (act_fused_on()) return act_fused(nullptr, n, obs, BDR_DTYPE_F32, obs_rows_on_device, obs_rows_on_device ? obs_row_stride : (uint64_t)O * 4, act_out, idx_out);
        BDR_HIP(hipSetDevice(device));
        BDR_TRY(ensure_batch((int)n));
        int32_t st = pack_acting_obs(obs, n, x0, net.L[0].Kp);
        if (st == BDR_OK) st = forward((int)net.L.size(), (int)n, "sample_fwd");
        if (st == BDR_OK) {
            BcActArgs a{act.back(), net.L.back().Np, A, (int)n, cfg.policy.activation_out, disc ? 1 : 0, samp, samp_idx};
            const int tot = disc ? (int)n : (int)n * A;
            Bracket br(this, "bc_act");
            const hipError_t e = step_launch(stream, false, k_bc_act, dim3((tot + 255) / 256), dim3(256), a);
            if (e != hipSuccess) st = fail(BDR_ERR_HIP, "k_bc_act: %s", hipGetErrorString(e));
        }
        // (an i64 row travels as two f32 words: the copy moves bits)
        if (st == BDR_OK) st = disc ? rows_to_host(reinterpret_cast<const float*>(samp_idx), reinterpret_cast<float*>(idx_out), n * 2) : rows_to_host(samp, act_out, n * A);
        slot_cursor = 0;
        return st;
    }
    int32_t sample_device(uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out, int64_t* idx_out)
    {
        return with_device_rows(obs_dev, row_stride, [&](const float* rows) { return sample(n, rows, act_out, idx_out); });
    }
    // ---- DenseAgent's acting hooks (dense_agent.hpp) ----
    const MlpLayout& act_net() const override { return net; }
    const float* act_params() const override { return p; }
    int32_t act_check_out(const float* act_out, const int64_t* idx_out) const override
    {
        const bool disc = cfg.action_type == BDR_BC_ACTION_DISCRETE;
        BDR_REQUIRE(disc ? idx_out != nullptr : act_out != nullptr, "BC sample: a %s agent writes %s", disc ? "Discrete" : "Continuous", disc ? "idx_out" : "act_out");
        return BDR_OK;
    }
    int32_t act_epilogue(DenseActArgs& a, uint64_t n) override
    {
        BDR_TRY(ensure_batch((int)n));
        a.mode = cfg.action_type == BDR_BC_ACTION_DISCRETE ? DA_BC_DISCRETE : DA_BC; a.kind = cfg.policy.activation_out;
        a.out = samp; a.idx = samp_idx;
        return BDR_OK;
    }
    int32_t act_results(uint64_t n, float* act_out, int64_t* idx_out) override
    {
        // (an i64 row travels as two f32 words: the copy moves bits)
        return cfg.action_type == BDR_BC_ACTION_DISCRETE ? rows_to_host(reinterpret_cast<const float*>(samp_idx), reinterpret_cast<float*>(idx_out), n * 2)
                                                         : rows_to_host(samp, act_out, n * A);
    }
    int32_t act_layers(uint64_t n, const void* rows, bool on_device, uint64_t stride, float* act_out, int64_t* idx_out) override
    {
        return on_device ? sample_device(n, rows, stride, act_out, idx_out) : sample(n, static_cast<const float*>(rows), act_out, idx_out);
    }
    // the compiled trainers take f32 action rows: Continuous only
    bool sample_f32(uint64_t n, const void* obs, bool on_device, uint64_t stride, float* out, int32_t* st) override
    {
        *st = !obs || !out ? fail(BDR_ERR_INVALID, "null argument")
            : cfg.action_type != BDR_BC_ACTION_CONTINUOUS ? fail(BDR_ERR_INVALID, "the compiled trainers take f32 action rows: a Discrete BC agent is sampled through bdr_bc_sample")
            : on_device ? sample_device(n, obs, stride, out, nullptr) : sample(n, static_cast<const float*>(obs), out, nullptr);
        return true;
    }

    // ---- parameter views: model 0; +100 grad, +200 exp_avg, +300 exp_avg_sq ----
    bool param_view(int which, ParamView* pv) override
    {
        if (which < 0 || which % 100 != 0 || which / 100 > 3) return false;
        float* r[4] = {p, g, m, v};
        *pv = mlp_view(net, r[which / 100]);
        return true;
    }
    // ---- group copies and hyperparameters (dense_agent.hpp) ----
    void state_arenas(std::vector<StateArena>& out) override { out = {{p, net.total}, {g, net.total}, {m, net.total}, {v, net.total}}; }
    void adopt_steps(const DenseAgent& src) override { step = static_cast<const Bc&>(src).step; }
    double* hyper_field(int32_t id) override { return id <= BDR_HYPER_WEIGHT_DECAY ? opt_field(cfg.opt, cfg.lr, id) : nullptr; }
    // ---- checkpoint: policy_model.pt (bc/base.rs:138-153), variables mlp.ln{i}.weight / .bias from the VarMap's root (bc/model.rs:130-133)
    void checkpoint_files(std::vector<CheckpointFile>& files) override
    {
        std::vector<NamedTensor> mt;
        candle::mlp_meta(net, "", mt);
        files = {{"policy_model", mt, {0}, {0}}};
    }
};

namespace {

constexpr size_t BC_LDS_MAX = 160 * 1024;

int32_t bc_check(const bdr_bc_config& c)
{
    BDR_REQUIRE(c.device >= 0, "No device is given for BC agent");
    BDR_REQUIRE(c.obs_dim >= 1 && c.obs_dim <= 4096 && c.act_dim >= 1 && c.act_dim <= 256, "bad obs/act dims");
    const bdr_mlp_config& m = c.policy;
    BDR_REQUIRE(m.n_units >= 0 && m.n_units <= BDR_MAX_UNITS, "policy: bad layer count");
    for (int i = 0; i < m.n_units; ++i) BDR_REQUIRE(m.units[i] >= 1 && m.units[i] <= 4096, "policy: bad layer width");
    BDR_REQUIRE(m.activation_out >= BDR_ACTIVATION_NONE && m.activation_out <= BDR_ACTIVATION_SIGMOID, "policy: unknown activation_out %d", m.activation_out);
    BDR_REQUIRE(c.action_type == BDR_BC_ACTION_DISCRETE || c.action_type == BDR_BC_ACTION_CONTINUOUS, "unknown BC action type %d", c.action_type);
    BDR_REQUIRE(c.batch_size >= 1 && c.batch_size <= 65536, "bad batch size");
    BDR_TRY(check_opt(c.opt, "policy"));
    BDR_REQUIRE(c.kernel_form >= BDR_BC_KERNEL_DEFAULT && c.kernel_form <= BDR_BC_KERNEL_FUSED_MFMA, "unknown BC kernel form %d", c.kernel_form);
    BDR_REQUIRE(c.head_rows == 0 || c.head_rows == 8 || c.head_rows == 16 || c.head_rows == 32, "head_rows must be 0, 8, 16 or 32");
    return BDR_OK;
}

}  // namespace

#include "bc_group.hpp"

extern "C" {

void bdr_bc_config_default(bdr_bc_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof *c);
    // bc/config.rs:66-75
    c->batch_size = 1; c->action_type = BDR_BC_ACTION_DISCRETE; c->device = -1; c->record_verbose_level = 0;
    c->policy.activation_out = BDR_ACTIVATION_NONE;
    // BcModelConfig (bc/model.rs:33-43): opt_config = OptimizerConfig::default() = AdamW with candle's ParamsAdamW defaults (opt.rs:100-111)
    c->lr = 1e-3;
    c->opt.opt_kind = BDR_OPT_ADAMW; c->opt.beta1 = 0.9; c->opt.beta2 = 0.999; c->opt.weight_decay = 0.01; c->opt.eps = 1e-8;
    c->kernel_form = BDR_BC_KERNEL_DEFAULT;
}

int32_t bdr_bc_create(const bdr_bc_config* cfg, bdr_agent** out)
{
    BDR_REQUIRE(cfg && out, "null argument");
    const bdr_bc_config& c = *cfg;
    BDR_TRY(bc_check(c));
    MlpLayout net = make_mlp(c.obs_dim, c.policy.units, c.policy.n_units, c.act_dim, false);
    // the fused head: one padded column block, a hidden layer under it, and its LDS plan within the CU's 160 KB
    const int R = c.head_rows ? c.head_rows : BC_HEAD_ROWS_DEFAULT;
    const bool can_fuse = c.act_dim <= 64 && c.policy.n_units >= 1 && bc_head_lds(net.L.back().Kp, R) <= BC_LDS_MAX;
    BDR_REQUIRE(c.kernel_form != BDR_BC_KERNEL_FUSED || can_fuse,
                "the fused BC head needs act_dim <= 64, a hidden layer, and the last layer's weights plus %d rows within 160 KB of LDS "
                "(act_dim %d, %d hidden layers, last hidden width %d): use BDR_BC_KERNEL_GENERAL", R, c.act_dim, c.policy.n_units,
                c.policy.n_units ? c.policy.units[c.policy.n_units - 1] : 0);
    const bool can_mfma = bc_can_mfma(c.act_dim, c.policy.n_units);
    BDR_REQUIRE(c.kernel_form != BDR_BC_KERNEL_FUSED_MFMA || can_mfma,
                "the fused BC head needs act_dim <= 64 and a hidden layer (act_dim %d, %d hidden layers): use BDR_BC_KERNEL_GENERAL", c.act_dim, c.policy.n_units);
    BDR_TRY(ensure_device(c.device));
    Bc* a = new Bc();
    a->cfg = c; a->device = c.device; a->train = false;
    a->O = c.obs_dim; a->A = c.act_dim; a->net = net;
    a->form = bc_resolve_form(c.kernel_form, (int)c.batch_size, c.act_dim, c.policy.n_units);
    a->head_rows = R; a->head_lds = bc_head_lds(net.L.back().Kp, R);
    const int32_t st = [&]() -> int32_t {
        BDR_HIP(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
        BDR_TRY(a->err_init());
        for (auto q : {&a->p, &a->g, &a->m, &a->v}) BDR_TRY(a->alloc(q, net.total, Bc::AGENT));
        BDR_TRY(a->alloc(&a->scal, 4, Bc::AGENT));
        BDR_TRY(a->alloc(&a->ticket, 4, Bc::AGENT));
        std::vector<float> ref(net.ref_total, 0.f);
        mlp_init_reference(net, c.seed * 7 + 1, ref.data());
        BDR_TRY(a->set_params(0, ref.data(), ref.size()));
        return a->ensure_batch((int)c.batch_size);
    }();
    if (st != BDR_OK) { delete a; return st; }
    *out = a;
    return BDR_OK;
}

int32_t bdr_bc_update_on_batch(bdr_agent* base, uint64_t n, const float* obs, const float* act, float* rec_out)
{
    BDR_REQUIRE(base && obs && act, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "bc"), "not a BC agent");
    Bc* a = static_cast<Bc*>(base);
    BDR_TRY(a->refuse_discrete());
    BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
    BDR_HIP(hipSetDevice(a->device));
    BDR_TRY(a->ensure_batch((int)n));
    if (n > a->u_cap) {
        BDR_HIP(hipStreamSynchronize(a->stream));
        a->release(Bc::STAGING);
        a->u_cap = 0;
        BDR_TRY(a->alloc(&a->u_obs, n * a->O, Bc::STAGING)); BDR_TRY(a->alloc(&a->u_act, n * a->A, Bc::STAGING));
        a->u_cap = n;
    }
    BDR_HIP(hipMemcpyAsync(a->u_obs, obs, n * a->O * 4, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_act, act, n * a->A * 4, hipMemcpyHostToDevice, a->stream));
    BDR_TRY(a->update((int)n, a->u_obs, a->u_act));
    prof_collect(a);
    if (rec_out) BDR_HIP(hipMemcpyAsync(rec_out, a->scal, 4, hipMemcpyDeviceToHost, a->stream));
    BDR_HIP(hipStreamSynchronize(a->stream));
    return a->err_check();
}

// Parity probes of the LAST update (see include/border_amd.h)
int32_t bdr_bc_probe(bdr_agent* base, int32_t what, float* out, uint64_t n)
{
    BDR_REQUIRE(base && out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "bc"), "not a BC agent");
    Bc* a = static_cast<Bc*>(base);
    BDR_HIP(hipSetDevice(a->device));
    const int Bn = a->last_B;
    BDR_REQUIRE(Bn > 0, "no update has run yet");
    BDR_REQUIRE(what == 0 || what == 1, "unknown BC probe %d", what);
    BDR_REQUIRE(n == (uint64_t)Bn * a->A, "this probe holds batch x act_dim values");
    BDR_HIP(hipStreamSynchronize(a->stream));
    const int ld = a->net.L.back().Np;
    std::vector<float> h((size_t)Bn * ld);
    BDR_HIP(hipMemcpy(h.data(), what == 0 ? a->pred : a->dy.back(), h.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < Bn; ++b) memcpy(out + (size_t)b * a->A, h.data() + (size_t)b * ld, (size_t)a->A * 4);
    return BDR_OK;
}

int32_t bdr_bc_sample(bdr_agent* base, uint64_t n, const float* obs, float* act_out, int64_t* idx_out)
{
    BDR_REQUIRE(base && obs, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "bc"), "not a BC agent");
    return static_cast<Bc*>(base)->sample(n, obs, act_out, idx_out);
}

int32_t bdr_bc_sample_device(bdr_agent* base, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out, int64_t* idx_out)
{
    BDR_REQUIRE(base && obs_dev, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "bc"), "not a BC agent");
    return static_cast<Bc*>(base)->sample_device(n, obs_dev, row_stride, act_out, idx_out);
}

}  // extern "C"
