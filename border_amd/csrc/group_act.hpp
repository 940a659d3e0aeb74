// ================================================================================================
// Group acting, the host half, once: Policy::sample of the selected members of a group on n host rows each in ONE launch of a group
// entry over dense_act_body (k_bc_act_group, bc_group.hpp: BC; k_candle_act_group, candle_act_group.hpp: Gaussian actors).  The rule
// without HIP in it - selection, the staged offsets, the cap, the draws - is group_act_plan.hpp's; this header adds the state and the
// call.  A group (group_core.hpp: bdr_bc_group, bdr_iql_group, bdr_awac_group) holds a GroupAct<Call> as `act` beside device, stream, members, shape (obs_dim,
// act_dim), ticket, seq, launches and kernel_launches, and hands group_act_sample a Kind that says what differs:
//   Kind::Call                          the words of one member's call (BcActCall, CandleActCall: the common words by name)
//   Kind::arena(m)                      the parameter arena the member acts with: the key of its static arguments
//   Kind::write_static(m, a)            the member's DenseActArgs: the network on that arena and the static half of the epilogue
//   Kind::noise(m, &train, &counter)    the member's mode and noise counter, for the draws rule of group_act_plan.hpp (BC: no stream)
//   Kind::call_words(m, c, train, start, counter)   what the call struct holds beyond the common words (train, and the counter the
//                                       call draws at) and the member's counter after the call; runs after every refusal, once per call
//   Kind::set_lds_attr(teams), launch(teams, grid, lds, stream, args, calls, sel, ticket, seq_host, seq)   GroupActEntry's, over the
//                                       one-team and the two-team instantiation of the kind's entry
//   static per member   d_act, rewritten when the member's arena has moved (keys), behind a stream synchronise
//   per call            calls / sel and the staged rows and results, ONE pinned, device-mapped area each - an acting call is
//                       synchronous, so the areas are free again whenever the next call fills them; rows and results grow on demand
//                       behind a stream synchronise; every member's block of rows is 16-byte aligned; one call stages at most 64 MiB
// The launch takes the next number of the group's one counter - opt rounds and acting calls are ordered on the group's stream - ends
// with the ticket and publishes that number; the host waits for it (wait_seq_word) and copies the actions out.  Everything is checked
// before anything is staged, enqueued or advanced; every refusal names the member.
#pragma once
#include <atomic>
#include <chrono>
#include <cstring>
#include <vector>

#include "slot_ring.hpp"
#include "device_arrays.hpp"
#include "group_act_plan.hpp"

static_assert(GA_MAX_ROWS == 65536, "group_act_plan.hpp restates the row limit of an acting call");

namespace {

template <class Call>
struct GroupAct {
    int W = 0, teams = 0; bool attr = false;
    std::vector<const float*> keys;                                 // [P] the arena d_act[p] was written for (null: not yet)
    std::vector<DenseActArgs> h_act; DeviceArray<DenseActArgs> d_act;   // [P]
    PinnedArray<Call> calls; PinnedArray<unsigned> sel;             // [P], [P]
    PinnedArray<uint8_t> rows; size_t rows_cap = 0;                 // bytes
    PinnedArray<float> res; size_t res_cap = 0;                     // floats
};

// the attribute and launch halves of a Kind: K1 / K2 are its entry with one team of 256 threads / two teams
template <class C> using GroupActKernel = void (*)(const BDR_CONST_AS DenseActArgs*, const BDR_CONST_AS C*, const BDR_CONST_AS unsigned*, unsigned*, unsigned*, unsigned);
template <class C, GroupActKernel<C> K1, GroupActKernel<C> K2>
struct GroupActEntry {
    using Call = C;
    // The result step of a call, what the four float-action kinds do; a kind whose members act otherwise (the candle DQN:
    // candle_dqn_group.hpp) shadows these.  Out: the element of act_out; act_cols(shape): the action width A; res_cols(A): the floats
    // a member's result block holds per row; result(m, block, n, A, out): the member's block -> its act_out rows, after the launch
    // has arrived, in selection order.
    using Out = float;
    template <class Shape> int act_cols(const Shape& s) const { return s.act_dim; }
    int res_cols(int A) const { return A; }
    template <class M> int32_t result(M*, const float* block, uint64_t n, int A, float* out) const
    {
        memcpy(out, block, (size_t)n * A * sizeof(float));
        return BDR_OK;
    }
    hipError_t set_lds_attr(int teams) const
    {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(teams == 2 ? K2 : K1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DA_LDS_MAX);
    }
    void launch(int teams, dim3 grid, size_t lds, hipStream_t stream, const BDR_CONST_AS DenseActArgs* args, const BDR_CONST_AS C* calls,
                const BDR_CONST_AS unsigned* sel, unsigned* ticket, unsigned* seq_host, unsigned seq) const
    {
        if (teams == 2) hipLaunchKernelGGL(K2, grid, dim3(512), lds, stream, args, calls, sel, ticket, seq_host, seq);
        else hipLaunchKernelGGL(K1, grid, dim3(256), lds, stream, args, calls, sel, ticket, seq_host, seq);
    }
};

// Policy::sample of the selected members (members == nullptr: all of them) on n host rows each, ONE launch
template <class Group, class Kind>
int32_t group_act_sample(Group* g, Kind kind, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows,
                         const int32_t* dtypes, typename Kind::Out* const* act_out)
{
    using Call = typename Kind::Call;
    auto& s = g->act;
    const uint32_t P = (uint32_t)g->members.size();
    const GaSelect pick = ga_select(members, n_sel, P);
    BDR_REQUIRE(pick.refusal != GA_EMPTY, "the member list is empty");
    BDR_REQUIRE(pick.refusal != GA_RANGE, "member %u (entry %u of the member list) of a group of %u", members[pick.entry], pick.entry, P);
    BDR_REQUIRE(pick.refusal != GA_ORDER, "member %u (entry %u of the member list): the list must be strictly ascending", members[pick.entry], pick.entry);
    BDR_REQUIRE(pick.refusal != GA_COUNT, "%u rows for a group of %u", n_sel, P);
    const auto at = [&](uint32_t b) { return ga_member_at(members, b); };
    BDR_REQUIRE(n >= 1 && n <= GA_MAX_ROWS, "batch size out of range");
    const int O = g->shape.obs_dim, A = kind.act_cols(g->shape), RC = kind.res_cols(A);
    if (!s.W) {
        s.W = g->members[0]->act_width();
        s.teams = dense_act_lds(s.W, 2) <= DA_LDS_MAX ? 2 : 1;
    }
    std::vector<int> f64(P, 0);
    for (uint32_t b = 0; b < n_sel; ++b) {
        const uint32_t p = at(b);
        BDR_REQUIRE(rows[p], "member %u: null observation rows", p);
        BDR_REQUIRE(act_out[p], "member %u: null act_out", p);
        const int32_t dt = dtypes[p];
        BDR_REQUIRE(dt == BDR_DTYPE_F32 || dt == BDR_DTYPE_F64, "member %u: dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64", p);
        if (const bdr_obs_norm* nm = norms ? norms[p] : nullptr) {
            BDR_REQUIRE(nm->ready, "member %u: the normaliser has no statistics yet (bdr_obs_norm_finish / bdr_obs_norm_set)", p);
            BDR_REQUIRE(nm->dim == (uint64_t)O, "member %u: the normaliser's dim (%llu) is not the agent's obs dim (%d)", p, (unsigned long long)nm->dim, O);
            BDR_REQUIRE(nm->device == g->device, "member %u: agent and normaliser live on different devices", p);
        }
        BDR_REQUIRE(s.W <= DA_MAX_W && dense_act_lds(s.W, 1) <= DA_LDS_MAX,
                    "member %u: the group acting kernel keeps two [32][W + 4] activation buffers in LDS: W <= %d, this member's widest padded layer is %d: "
                    "such members keep acting standalone (bdr_agent_sample_raw)", p, DA_MAX_W, s.W);
        f64[p] = dt == BDR_DTYPE_F64 ? 1 : 0;
    }
    const GaPlan plan = ga_plan(members, n_sel, P, n, O, RC, f64.data());   // (RC = A for every kind but the candle DQN)
    const size_t staged = plan.staged, res_floats = plan.res_floats;
    BDR_REQUIRE(plan.refusal == GA_OK,
                "member %u .. %u: %zu bytes of rows and %zu bytes of actions in one group acting call, more than the staging area's %zu: split the call",
                at(0), at(n_sel - 1), staged, res_floats * 4, GA_STAGE_MAX);
    BDR_HIP(hipSetDevice(g->device));
    // ---- the areas (first call, growth) and the static arguments (first call, a moved arena): rare, behind whatever the stream holds
    if (!s.d_act) {   // (d_act last: a failure before it leaves the first call to be made again)
        BDR_HIP(pinned_array(s.calls, P));
        BDR_HIP(pinned_array(s.sel, P));
        s.h_act.assign(P, DenseActArgs{});
        s.keys.assign(P, nullptr);
        BDR_HIP(device_array(s.d_act, P));
    }
    if (staged > s.rows_cap) {
        BDR_HIP(hipStreamSynchronize(g->stream));
        const size_t cap = std::max(staged, (size_t)64 * 1024);
        s.rows_cap = 0;
        BDR_HIP(pinned_array(s.rows, cap));
        s.rows_cap = cap;
    }
    if (res_floats > s.res_cap) {
        BDR_HIP(hipStreamSynchronize(g->stream));
        const size_t cap = std::max(res_floats, (size_t)16 * 1024);
        s.res_cap = 0;
        BDR_HIP(pinned_array(s.res, cap));
        s.res_cap = cap;
    }
    bool dirty = false;
    for (uint32_t b = 0; b < n_sel; ++b) {
        const uint32_t p = at(b);
        const auto* m = g->members[p];
        if (s.keys[p] == kind.arena(m)) continue;
        DenseActArgs& a = s.h_act[p];
        a = DenseActArgs{};
        a.O = O; a.A = A; a.W = s.W;
        kind.write_static(m, a);
        s.keys[p] = kind.arena(m);
        dirty = true;
    }
    if (dirty) {
        hipError_t e = hipStreamSynchronize(g->stream);
        if (e == hipSuccess) e = hipMemcpy(s.d_act.get(), s.h_act.data(), (size_t)P * sizeof(DenseActArgs), hipMemcpyHostToDevice);
        if (e != hipSuccess) s.keys.assign(P, nullptr);   // (nothing is known to be on the device: the next call writes it again)
        BDR_HIP(e);
    }
    if (!s.attr) {   // more than 64 KB of dynamic LDS has to be asked for, once per group (and so per device)
        BDR_HIP(kind.set_lds_attr(s.teams));
        s.attr = true;
    }
    // ---- this call's words, rows and selection; the draws (ga_apply_draws): a selected member in train mode draws at its own counter,
    // which advances by n * A
    std::vector<int> train(P, 0);
    std::vector<uint64_t> counters(P, 0), start(n_sel, 0);
    for (uint32_t b = 0; b < n_sel; ++b) kind.noise(g->members[at(b)], &train[at(b)], &counters[at(b)]);
    ga_apply_draws(plan, members, n_sel, n, A, train.data(), counters.data(), start.data());
    for (uint32_t b = 0; b < n_sel; ++b) {
        const uint32_t p = at(b);
        const size_t off = plan.row_off[b], row = ga_row_bytes(O, f64[p] != 0), bytes = (size_t)n * row;
        memcpy(s.rows.host.get() + off, rows[p], bytes);
        const bdr_obs_norm* nm = norms ? norms[p] : nullptr;
        Call c{};
        c.rows = s.rows.dev + off; c.row_stride = row; c.mean = nm ? nm->d_meanf : nullptr; c.std = nm ? nm->d_stdf : nullptr;
        c.out = s.res.dev + plan.res_off[b]; c.idx = nullptr; c.n = (int)n; c.f64 = f64[p];
        kind.call_words(g->members[p], c, train[p], start[b], counters[p]);
        s.calls.host.get()[p] = c;
        s.sel.host.get()[b] = p;
    }
    std::atomic_thread_fence(std::memory_order_release);
    // the launch takes the next number of the group's one counter: opt rounds and acting calls are ordered on the group's stream
    const uint64_t k = g->launches + 1;
    g->launches = k;
    const dim3 grid((unsigned)((n + 31) / 32), n_sel);
    const size_t lds = dense_act_lds(s.W, s.teams);
    kind.launch(s.teams, grid, lds, g->stream, (const BDR_CONST_AS DenseActArgs*)s.d_act.get(), (const BDR_CONST_AS Call*)s.calls.dev,
                (const BDR_CONST_AS unsigned*)s.sel.dev, g->ticket.get(), g->seq.dev, (unsigned)k);
    BDR_HIP(hipGetLastError());
    g->kernel_launches += 1;
    bool arrived = false;
    BDR_TRY(wait_seq_word(g->seq.host.get(), (unsigned)k, g->stream, std::chrono::steady_clock::now(), &arrived));
    if (!arrived) return fail(BDR_ERR_HIP, "the actions of a group acting call never arrived in host memory");
    std::atomic_thread_fence(std::memory_order_acquire);
    for (uint32_t b = 0; b < n_sel; ++b) BDR_TRY(kind.result(g->members[at(b)], s.res.host.get() + plan.res_off[b], n, A, act_out[at(b)]));
    return BDR_OK;
}

}  // namespace
