// DenseAgent: the host core under every agent whose models are Mlps trained on dense.hpp's FP32-MFMA kernels (BC: bc.hip; the candle
// DQN: candle_dqn.hip; IQL, AWAC and the candle SAC through CandleAgent, candle_actor.hpp).  It knows how such a network is allocated, run forward, stepped (input gradients,
// the grouped dW, the fused reduce + Adam), fed the observation rows of an acting call, and copied to and from the reference
// layout (mlp_view, dense.hpp) - and nothing about which models an agent has: an agent brings its arenas, its batch buffers, its loss kernels and its
// update schedule.  Host code only; with it the checkpoint helpers of candle VarMaps and the optimizer check the agents share.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "dense.hpp"
#include "dense_act.hpp"

namespace bdr {
namespace candle {

// ---- checkpoints of candle VarMaps (host) ----
// the variables of an Mlp under `prefix`: mlp.ln{i}.weight [out][in], mlp.ln{i}.bias [out]
inline void mlp_meta(const MlpLayout& net, const std::string& prefix, std::vector<NamedTensor>& mt) { mlp_tensors(net, prefix + "mlp.ln", mt); }
}  // namespace candle
}  // namespace bdr

namespace {
using namespace bdr;

int32_t check_opt(const bdr_adamw_config& o, const char* what)
{
    BDR_REQUIRE(o.opt_kind == BDR_OPT_ADAM || o.opt_kind == BDR_OPT_ADAMW, "%s: unknown optimizer", what);
    BDR_REQUIRE(!(o.opt_kind == BDR_OPT_ADAMW && o.amsgrad), "%s: candle's AdamW has no amsgrad", what);
    return BDR_OK;
}

struct DenseAgent : bdr_agent {
    int O = 0, A = 0;   // f32 observation and action row widths
    bool candle_checkpoints() const override { return true; }   // every agent on this core mirrors a candle agent: VarMap files

    // Every device buffer is registered by its lifetime when it is allocated and freed here: the agent's (arenas, record values),
    // those of one batch size (the agent's ensure_batch) and the staging rows of update_on_batch
    enum Life { AGENT, BATCH, STAGING };
    std::vector<void*> owned[3];
    template <class T>
    int32_t alloc(T** p, size_t n, Life life, bool zero = true)
    {
        const size_t bytes = std::max<size_t>(n, 4) * sizeof(T);
        BDR_HIP(hipMalloc((void**)p, bytes));
        owned[life].push_back(*p);
        if (zero) BDR_HIP(hipMemsetAsync(*p, 0, bytes, stream));
        return BDR_OK;
    }
    void release(Life life)
    {
        for (void* p : owned[life]) (void)hipFree(p);
        owned[life].clear();
    }
    ~DenseAgent() override
    {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        for (Life l : {AGENT, BATCH, STAGING}) release(l);
        (void)hipFree(raw_f32);
    }
    int32_t layer_bufs(const MlpLayout& net, int Bn, std::vector<float*>& out)
    {
        out.assign(net.L.size(), nullptr);
        for (size_t l = 0; l < net.L.size(); ++l) BDR_TRY(alloc(&out[l], (size_t)Bn * net.L[l].Np, BATCH));
        return BDR_OK;
    }
    // row chunks of the grouped dW launch (k_dense_dw_small_group: 256 rows per workgroup, at most 16 chunks)
    static int chunks_for(int Bn) { return std::max(1, std::min(16, Bn / 256)); }
    // per-layer offsets of one network's dW partials; returns their size
    static size_t plan(const MlpLayout& net, int Bn, std::vector<size_t>& off)
    {
        off.clear();
        size_t o = 0;
        for (const auto& l : net.L) { off.push_back(o); o += (size_t)chunks_for(Bn) * ((size_t)l.Kp * l.Np + l.Np); }
        return o;
    }

    // forward of n (parameters, input) pairs of one architecture, up to 4 per launch: pass j runs params[j] on x[j] into
    // (*acts[j])[layer]; layers [0, upto), all of them by default.  One profile bracket `name` per launch.
    int32_t mlp_forward(const MlpLayout& net, int n, const float* const* params, const float* const* x, std::vector<float*>* const* acts, int Bn, const char* name,
                        int upto = -1)
    {
        const size_t layers = upto < 0 ? net.L.size() : (size_t)upto;
        for (int j0 = 0; j0 < n; j0 += 4) {
            const int nz = std::min(4, n - j0);
            DenseSrc in[4]; float* out[4];
            for (int j = 0; j < nz; ++j) in[j] = DenseSrc{x[j0 + j], net.L[0].Kp};
            for (size_t l = 0; l < layers; ++l) {
                for (int j = 0; j < nz; ++j) out[j] = (*acts[j0 + j])[l];
                Bracket br(this, name);
                BDR_TRY(dense_forward_z(stream, net.L[l], nz, params + j0, in, out, Bn, true));
                for (int j = 0; j < nz; ++j) in[j] = DenseSrc{out[j], net.L[l].Np};
            }
        }
        return BDR_OK;
    }
    static AdamScalars opt_scalars(const bdr_adamw_config& o, double lr, uint64_t step)
    {
        return adam_scalars_for(o.opt_kind == BDR_OPT_ADAMW, lr, o.beta1, o.beta2, o.eps, o.weight_decay, step);
    }
    // the profile brackets of mlp_backward_step, one per launch: the input gradients, the grouped dW, the reduce + Adam
    struct StepNames {
        const char *dx, *dw, *adam;
        StepNames(const char* one) : dx(one), dw(one), adam(one) {}
        StepNames(const char* dx_, const char* dw_, const char* adam_) : dx(dx_), dw(dw_), adam(adam_) {}
    };
    // backward of nz networks of one layout from the output gradient dy[z][lo] of layer lo (the last layer, or below it where the
    // agent's own kernel has already formed the gradients above: BC's fused head): input gradients down to layer 1 (one launch per
    // layer for all nz), every weight gradient in one grouped launch, then the fused reduce + Adam (+ tracking into tgt at rate tau).
    // poison (optional): a device word that, when non-zero, makes the reduce + Adam launch leave everything alone (the candle DQN's
    // out-of-range action flag); applied / step: *applied = step by a launch that was not skipped.
    // dx0 / mask0 (optional): one more input-gradient launch below layer 0, d(x0) of network z into dx0[z] ([Bn][Kp of layer 0]),
    // zero where mask0[z] - the post-ReLU activation that produced x0 - is not positive (the candle DQN's conv trunk feeds layer 0).
    int32_t mlp_backward_step(const MlpLayout& net, int nz, float* const* p, float* const* g, float* const* m, float* const* v, float* const* tgt,
                              const float* x0, std::vector<float*>* const* acts, std::vector<float*>* const* dys, float* part, size_t part_stride,
                              const std::vector<size_t>& off, const AdamScalars* sc, int Bn, const StepNames& names, size_t total, double tau, int lo,
                              const DenseReduceSeg* extra = nullptr, const unsigned* poison = nullptr, unsigned long long* applied = nullptr,
                              unsigned long long step = 0, float* const* dx0 = nullptr, const float* const* mask0 = nullptr)
    {
        const int L = (int)net.L.size();
        for (int l = lo; l >= 1; --l) {
            const float* pb[4]; const float* dy[4]; float* dx[4]; const float* mask[4];
            for (int z = 0; z < nz; ++z) { pb[z] = p[z]; dy[z] = (*dys[z])[l]; dx[z] = (*dys[z])[l - 1]; mask[z] = (*acts[z])[l - 1]; }
            Bracket br(this, names.dx);
            BDR_TRY(dense_dx_z(stream, net.L[l], nz, pb, dy, dx, mask, Bn, true));
        }
        if (dx0) {
            const float* pb[4]; const float* dy[4];
            for (int z = 0; z < nz; ++z) { pb[z] = p[z]; dy[z] = (*dys[z])[0]; }
            Bracket br(this, names.dx);
            BDR_TRY(dense_dx_z(stream, net.L[0], nz, pb, dy, dx0, mask0, Bn, true));
        }
        std::vector<DenseDwJob> jobs;
        const int c = chunks_for(Bn);
        for (int z = 0; z < nz; ++z)
            for (int l = 0; l < L; ++l)
                jobs.push_back(DenseDwJob{&net.L[l], l == 0 ? DenseSrc{x0, net.L[0].Kp} : DenseSrc{(*acts[z])[l - 1], net.L[l - 1].Np}, (*dys[z])[l],
                                          part + (size_t)z * part_stride + off[l], c});
        { Bracket br(this, names.dw); BDR_TRY(dense_dw_small_group(stream, jobs.data(), (int)jobs.size(), Bn)); }
        ReduceAdamArgs ra{};
        ra.nseg = L; ra.inst_part_stride = part_stride;
        for (int l = 0; l < L; ++l) {
            const DenseLayer& ly = net.L[l];
            const size_t nfl = (size_t)ly.Kp * ly.Np + ly.Np;
            ra.seg[l] = DenseReduceSeg{part + off[l], nfl, c, (unsigned)(ly.w / 4), (unsigned)(nfl / 4)};
        }
        if (extra) ra.seg[ra.nseg++] = *extra;
        for (int z = 0; z < nz; ++z) { ra.p[z] = p[z]; ra.g[z] = g[z]; ra.m[z] = m[z]; ra.v[z] = v[z]; ra.tgt[z] = tgt ? tgt[z] : nullptr; ra.s[z] = sc[z]; ra.vmax[z] = nullptr; }
        // without targets (track == 0) k_dense_reduce_adam reads neither tau nor omt: an agent that has none passes any tau
        ra.n4 = (unsigned)(total / 4); ra.track = tgt ? 1 : 0; ra.tau = (float)tau; ra.omt = (float)(1.0 - tau);
        ra.poison = poison; ra.applied = applied; ra.step = step;
        Bracket br(this, names.adam);
        BDR_HIP(step_launch(stream, true, k_dense_reduce_adam, dim3((ra.n4 + 255) / 256, nz), dim3(256), ra));
        return BDR_OK;
    }

    // Agent::opt's checks of the replay buffer: f32 rows of the agent's widths on the agent's device
    int32_t check_replay(const bdr_replay* r, const char* name) const
    {
        BDR_REQUIRE(r->obs_bytes == (uint64_t)O * 4 && r->act_bytes == (uint64_t)A * 4, "replay rows do not match %s obs/act dims (f32 rows)", name);
        BDR_REQUIRE(r->device == device, "agent and replay buffer live on different devices");
        BDR_REQUIRE(!r->frame_stack, "%s reads f32 observation rows, not a frame-stack store", name);
        return BDR_OK;
    }

    // ---- training state as a group copy moves it (group_copy.hpp) ----
    // state_arenas: every arena the agent's model table serves, each once, in one order for every agent of a kind and shape (an
    // agent lists its allocations, not its views: the candle SAC's one-float views share a block).  state_adopt: the host half of a
    // copy from `src`, an agent of the same kind and shape - the optimizer step counters, and with `hypers` every settable
    // hyperparameter both have; seed, noise counter, mode, act path, n_opts and everything about buffers stay this agent's.
    struct StateArena { float* p; size_t n; };
    virtual void state_arenas(std::vector<StateArena>& out) { out.clear(); }   // (the candle DQN's group, candle_dqn_group.hpp, has no copy between members: it lists none)
    virtual void adopt_steps(const DenseAgent&) {}
    void state_adopt(const DenseAgent& src, bool hypers)
    {
        adopt_steps(src);
        if (hypers)
            for (int32_t id = 0; id <= HYPER_ID_MAX; ++id) {
                double* d = hyper_field(id);
                const double* s = const_cast<DenseAgent&>(src).hyper_field(id);
                if (d && s && *d != *s) { *d = *s; hyper_gen += 1; }
            }
    }

    // ---- hyperparameters by id (bdr_agent_hyper_get / _set) ----
    // hyper_field: the config field behind BDR_HYPER_* `id`, null where the kind (or the agent's entropy mode) has none.  hyper_gen
    // moves with every change: the groups key their staged static arguments on it (group_core.hpp), the per-step words and the
    // agent's own update read the config afresh.
    static constexpr int32_t HYPER_ID_MAX = BDR_HYPER_TARGET_ENTROPY;
    uint64_t hyper_gen = 0;
    virtual double* hyper_field(int32_t) { return nullptr; }
    static double* opt_field(bdr_adamw_config& o, double& lr, int k)   // k: BDR_HYPER_LR .. BDR_HYPER_WEIGHT_DECAY
    {
        double* f[5] = {&lr, &o.beta1, &o.beta2, &o.eps, &o.weight_decay};
        return k >= 0 && k < 5 ? f[k] : nullptr;
    }
    static int32_t hyper_check(int32_t id, double v)
    {
        const int k = id < BDR_HYPER_GAMMA ? id % 10 : -1;
        BDR_REQUIRE(std::isfinite(v), "hyperparameter %d: %g is not finite", id, v);
        if (k == BDR_HYPER_LR || id == BDR_HYPER_ENT_COEF_LR) BDR_REQUIRE(v >= 0.0, "hyperparameter %d: a learning rate is >= 0, got %g", id, v);
        else if (k == BDR_HYPER_BETA1 || k == BDR_HYPER_BETA2) BDR_REQUIRE(v >= 0.0 && v < 1.0, "hyperparameter %d: a beta lies in [0, 1), got %g", id, v);
        else if (k == BDR_HYPER_EPS || k == BDR_HYPER_WEIGHT_DECAY) BDR_REQUIRE(v >= 0.0, "hyperparameter %d: eps and weight decay are >= 0, got %g", id, v);
        else if (id == BDR_HYPER_GAMMA || id == BDR_HYPER_CRITIC_TAU) BDR_REQUIRE(v >= 0.0 && v <= 1.0, "hyperparameter %d: gamma and critic_tau lie in [0, 1], got %g", id, v);
        else if (id == BDR_HYPER_TAU_IQL) BDR_REQUIRE(v > 0.0 && v < 1.0, "hyperparameter %d: tau_iql lies in (0, 1), got %g", id, v);
        else if (id == BDR_HYPER_INV_LAMBDA || id == BDR_HYPER_EXP_ADV_MAX) BDR_REQUIRE(v >= 0.0, "hyperparameter %d: inv_lambda and exp_adv_max are >= 0, got %g", id, v);
        return BDR_OK;
    }
    int32_t hyper(int32_t id, bool set, double* v) override
    {
        double* f = id >= 0 && id <= HYPER_ID_MAX ? hyper_field(id) : nullptr;
        BDR_REQUIRE(f, "%s agent has no hyperparameter %d (include/border_amd.h, BDR_HYPER_*)", kind(), id);
        if (!set) { *v = *f; return BDR_OK; }
        BDR_TRY(hyper_check(id, *v));
        if (*f != *v) { *f = *v; hyper_gen += 1; }
        return BDR_OK;
    }

    // ---- acting calls (Policy::sample) ----
    // n observation rows (host rows, or device rows inside with_device_rows) -> the zero-padded first-layer input x [n][Kp].  On an
    // error the profile's slot cursor is reset, as the caller does when the call ends, and the status returned.
    int32_t pack_acting_obs(const float* obs, uint64_t n, float* x, int Kp)
    {
        const uint8_t* d = nullptr;
        int32_t st = acting_rows(obs, (size_t)O * 4, n, &d);
        if (st == BDR_OK) st = pack_rows(stream, reinterpret_cast<const float*>(d), O, O, x, Kp, 0, (int)n);
        if (st != BDR_OK) slot_cursor = 0;
        return st;
    }
    // an acting call on rows that already live in HBM, row_stride bytes apart: sample(rows) is the agent's host-row call
    template <class F>
    int32_t with_device_rows(const void* obs_dev, uint64_t row_stride, F&& sample)
    {
        BDR_REQUIRE(row_stride >= (uint64_t)O * 4 && row_stride % 4 == 0, "row_stride must be >= the row size and a multiple of 4");
        BDR_HIP(hipSetDevice(device));
        BDR_TRY(check_device_rows(obs_dev, row_stride));
        DeviceRowsScope rows(this, row_stride);
        return sample(static_cast<const float*>(obs_dev));
    }

    // ---- the acting path (bdr_agent_set_act_path) and raw rows (bdr_agent_sample_raw) ----
    // An agent names the network it acts with (act_net / act_params), checks its output pointers (act_check_out), fills the epilogue
    // of k_dense_act for n rows (act_epilogue: its result buffers, the element code's operands, the draws it takes), copies the
    // results out (act_results) and runs its layer-by-layer call on f32 rows (act_layers).
    virtual const MlpLayout& act_net() const = 0;
    virtual const float* act_params() const = 0;
    virtual int32_t act_check_out(const float* act_out, const int64_t* idx_out) const = 0;
    virtual int32_t act_epilogue(DenseActArgs& a, uint64_t n) = 0;
    virtual int32_t act_results(uint64_t n, float* act_out, int64_t* idx_out) = 0;
    virtual int32_t act_layers(uint64_t n, const void* rows, bool on_device, uint64_t stride, float* act_out, int64_t* idx_out) = 0;

    int32_t act_path = BDR_ACT_PATH_DEFAULT;
    bool act_attr[2] = {false, false};   // k_dense_act<1>, <2>: the dynamic LDS size was asked for (once per agent, and so per device)
    float* raw_f32 = nullptr; size_t raw_cap = 0;   // the layer path's f32 rows of a raw call
    // widest padded layer input / output of the acting network
    int act_width() const
    {
        int W = 0;
        for (const auto& l : act_net().L) W = std::max(W, std::max(l.Kp, l.Np));
        return W;
    }
    // BDR_ACT_PATH_DEFAULT is the layer path: nothing has shown the fused kernel faster in every round for any shape class yet
    // (DESIGN.md 14); BDR_ACT_PATH_FUSED asks for it
    bool act_fused_on() const { return act_path == BDR_ACT_PATH_FUSED; }
    int32_t set_act_path(int32_t path) override
    {
        BDR_REQUIRE(path == BDR_ACT_PATH_DEFAULT || path == BDR_ACT_PATH_LAYERS || path == BDR_ACT_PATH_FUSED, "unknown act path %d", path);
        const int W = act_width();
        BDR_REQUIRE(path != BDR_ACT_PATH_FUSED || (W <= DA_MAX_W && dense_act_lds(W, 1) <= DA_LDS_MAX),
                    "the fused acting kernel keeps two [32][W + 4] activation buffers and its reduction block in 160 KB of LDS: W <= %d, "
                    "this agent's widest padded layer is %d: use BDR_ACT_PATH_LAYERS", DA_MAX_W, W);
        act_path = path;
        return BDR_OK;
    }
    // one launch: raw rows -> (normalise) -> every layer -> the action, then the results to the host
    int32_t act_fused(const bdr_obs_norm* norm, uint64_t n, const void* rows, int32_t dtype, bool on_device, uint64_t stride, float* act_out, int64_t* idx_out)
    {
        BDR_TRY(act_check_out(act_out, idx_out));
        BDR_HIP(hipSetDevice(device));
        const MlpLayout& net = act_net();
        const uint64_t eb = dtype == BDR_DTYPE_F64 ? 8 : 4;
        DenseActArgs a{};
        const uint8_t* src = static_cast<const uint8_t*>(rows);
        uint64_t rs = stride;
        if (!on_device) {   // host rows: the pinned area the kernel reads in place, or (large) the staging buffer
            rs = (uint64_t)O * eb;
            if (n * rs <= HOST_ROWS_PINNED_MAX) BDR_TRY(host_rows_pinned(rows, n * rs, &src));
            else {
                void* stage = nullptr;
                BDR_TRY(act_buffer(n * rs, &stage));
                BDR_HIP(hipMemcpyAsync(stage, rows, n * rs, hipMemcpyHostToDevice, stream));
                src = static_cast<const uint8_t*>(stage);
            }
        }
        a.rows = src; a.row_stride = rs; a.f64 = dtype == BDR_DTYPE_F64 ? 1 : 0;
        a.n = (int)n; a.O = O; a.A = A; a.nl = (int)net.L.size(); a.W = act_width();
        a.mean = norm ? norm->d_meanf : nullptr; a.std = norm ? norm->d_stdf : nullptr;
        const float* pb = act_params();
        for (int l = 0; l < a.nl; ++l) a.L[l] = DenseActLayer{pb + net.L[l].w, pb + net.L[l].b, net.L[l].Kp, net.L[l].Np, net.L[l].relu};
        BDR_TRY(act_epilogue(a, n));
        const int teams = dense_act_lds(a.W, 2) <= DA_LDS_MAX ? 2 : 1;
        const size_t lds = dense_act_lds(a.W, teams);
        int32_t st = BDR_OK;
        {
            Bracket br(this, "dense_act");
            hipError_t e = hipSuccess;
            if (!act_attr[teams - 1]) {   // more than 64 KB of dynamic LDS has to be asked for
                e = teams == 2 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dense_act<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DA_LDS_MAX)
                               : hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dense_act<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DA_LDS_MAX);
                act_attr[teams - 1] = e == hipSuccess;
            }
            if (e == hipSuccess) {
                const dim3 grid((unsigned)((n + 31) / 32));
                if (teams == 2) hipLaunchKernelGGL(k_dense_act<2>, grid, dim3(512), lds, stream, a);
                else hipLaunchKernelGGL(k_dense_act<1>, grid, dim3(256), lds, stream, a);
                e = hipGetLastError();
            }
            if (e != hipSuccess) st = fail(BDR_ERR_HIP, "k_dense_act: %s", hipGetErrorString(e));
        }
        if (st == BDR_OK) st = act_results(n, act_out, idx_out);
        if (st == BDR_OK) prof_collect(this);
        slot_cursor = 0;
        return st;
    }
    // Policy::sample on raw environment rows (bdr_agent_sample_raw): fused, one launch; layers, the rows' f32 / z form into
    // contiguous device rows (obs_norm_z, the expression of bdr_obs_norm_apply) followed by the agent's call on those
    int32_t sample_raw(const bdr_obs_norm* norm, uint64_t n, const void* rows, int32_t dtype, bool on_device, uint64_t stride, float* act_out,
                       int64_t* idx_out) override
    {
        BDR_REQUIRE(rows, "null argument");
        BDR_TRY(act_check_out(act_out, idx_out));
        BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
        BDR_REQUIRE(dtype == BDR_DTYPE_F32 || dtype == BDR_DTYPE_F64, "dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64");
        const uint64_t eb = dtype == BDR_DTYPE_F64 ? 8 : 4;
        if (norm) {
            BDR_REQUIRE(norm->ready, "the normaliser has no statistics yet (bdr_obs_norm_finish / bdr_obs_norm_set)");
            BDR_REQUIRE(norm->dim == (uint64_t)O, "the normaliser's dim (%llu) is not the agent's obs dim (%d)", (unsigned long long)norm->dim, O);
            BDR_REQUIRE(norm->device == device, "agent and normaliser live on different devices");
        }
        BDR_HIP(hipSetDevice(device));
        if (on_device) {
            BDR_REQUIRE(stride >= (uint64_t)O * eb && stride % eb == 0 && (uintptr_t)rows % eb == 0,
                        "row_stride must be a multiple of the element size and >= the row size, rows aligned to the element size");
            BDR_TRY(check_device_rows(rows, stride));
        }
        if (act_fused_on()) return act_fused(norm, n, rows, dtype, on_device, stride, act_out, idx_out);
        if (!norm && dtype == BDR_DTYPE_F32) return act_layers(n, rows, on_device, stride, act_out, idx_out);
        const uint8_t* src = static_cast<const uint8_t*>(rows);
        uint64_t rs = stride;
        if (!on_device) {
            rs = (uint64_t)O * eb;
            BDR_TRY(acting_rows(rows, (size_t)rs, n, &src));
        }
        if (n * O > raw_cap) {
            BDR_HIP(hipStreamSynchronize(stream));
            (void)hipFree(raw_f32); raw_f32 = nullptr; raw_cap = 0;
            const size_t cap = std::max<size_t>(n * O, 4096);
            BDR_HIP(hipMalloc((void**)&raw_f32, cap * 4));
            raw_cap = cap;
        }
        const dim3 grid((unsigned)((n * O + 255) / 256));
        const float* mean = norm ? norm->d_meanf : nullptr; const float* sd = norm ? norm->d_stdf : nullptr;
        {
            Bracket br(this, "raw_rows");
            if (dtype == BDR_DTYPE_F64) hipLaunchKernelGGL(k_act_raw_rows<double>, grid, dim3(256), 0, stream, src, (unsigned long long)rs, (unsigned long long)n, O, mean, sd, raw_f32);
            else hipLaunchKernelGGL(k_act_raw_rows<float>, grid, dim3(256), 0, stream, src, (unsigned long long)rs, (unsigned long long)n, O, mean, sd, raw_f32);
        }
        BDR_HIP(hipGetLastError());
        return act_layers(n, raw_f32, true, (uint64_t)O * 4, act_out, idx_out);
    }
};

}  // namespace
