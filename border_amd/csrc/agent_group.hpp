// ================================================================================================
// A group of DqnMlp agents: Agent::opt of every member in ONE launch per update round (k_dqn_mlp_step[_lds]_group, workgroup p =
// member p) and Policy::sample of every member in one launch (k_dqn_mlp_act_group).  A launch grouping, not an agent kind: the
// members stay ordinary bdr_agents on the group's stream (DESIGN.md "Agent groups").  This file is a part of mlp_agents.hip's
// translation unit (it needs DqnMlp, and the kernels of mlp_fused.hpp are compiled once), included where the code stood.
//   static arguments   d_args[P] (MlpFusedArgs without its per-step words), rewritten only when a member's buffers or ring change
//                      (`key` below) - synchronously, behind a stream synchronise: rare
//   per launch         three pinned, device-mapped staging rings the kernels read in place: MfStep[P] per step, PerGroupWords[P] per
//                      round with prioritized members, [GroupPushDesc[P] | P records | words] per push
// so one group step is one launch per update round and no copy command, whatever P is.
// A group whose members do NOT take the one-workgroup step (one shape for all, Mlp[256, 256] at batch 64 among them) takes the layer
// form instead: group_layers.hpp - the layer path's launches of one member, each serving all members, on the same rings and rule.
// The one rule of the three rings (slot_ring.hpp): every launch that ends with mf_group_done / per_group_done takes the next number of
// `launches` and publishes it to the pinned word `seq`; a ring takes its slots in turn by its own use count, records per slot the
// number published by the last kernel that reads it - a step or a push its own number k, the words of a prioritized round and a push
// onto prioritized rings k + 1, the number of the last tree kernel behind them - and the host rewrites a slot only once `seq` has
// reached the number recorded for it.
#pragma once
#include "slot_ring.hpp"
#include "device_arrays.hpp"
#include "gp_copy.hpp"

#include "group_layers.hpp"

struct bdr_agent_group {
    enum { STEP_SLOTS = 8, PUSH_SLOTS = 8 };
    using StepRing = SlotRing<STEP_SLOTS>;
    using PushRing = SlotRing<PUSH_SLOTS>;
    int32_t device = 0;
    hipStream_t stream = nullptr;
    // (bdr_agent_group_destroy has synchronised the stream and destroyed the members; a failed create has adopted nobody.)  The stream
    // goes first, the buffers - the members below - after it.
    ~bdr_agent_group() { if (stream) { stream_retire(stream); (void)hipStreamDestroy(stream); } }
    std::vector<DqnMlp*> members;
    uint64_t n_updates = 1;
    // the form: every member takes the one-workgroup step (layers == nullptr, everything below as it always was), or none does and all
    // have one shape on the latency-shaped layer path (group_layers.hpp: its device arrays; `keys`, `steps`, `seq`, `ticket` are shared)
    std::unique_ptr<GroupLayers> layers;
    uint64_t kernel_launches = 0;                                       // every kernel launch the group's own calls have enqueued (bdr_agent_group_info)
    // opt
    struct StaticKey { bool valid = false; uint64_t batch_gen = 0; const void* td_abs = nullptr; uint64_t r_uid = 0, r_batch_gen = 0;
                       const void* weight = nullptr; int per_j = -1; };   // (prioritized ring: its weight array, its place in d_per)
    std::vector<StaticKey> keys;
    std::vector<MlpFusedArgs> h_args; DeviceArray<MlpFusedArgs> d_args;
    std::vector<size_t> lds_bytes; size_t lds_attr = 0;
    PinnedArray<MfStep> steps; StepRing step_ring;                      // [STEP_SLOTS][P]
    PinnedArray<unsigned> seq;                                          // pinned word: the launch number published last
    DeviceArray<unsigned> ticket;
    uint64_t launches = 0;                                              // launch numbers given out so far (1-based; the word carries them as unsigned)
    std::vector<bdr_replay*> last_buffers;                              // the buffers of the last accepted opt (distinctness checked once)
    uint64_t poll_count = 0; DeviceArray<MfErrRef> d_err_refs;
    // acting
    DeviceArray<MfActArgs> d_act; std::vector<unsigned> obs_off; unsigned obs_floats = 0;
    PinnedArray<float> obs_pin, act_pin; unsigned act_seq = 0;
    // acting for a subset (k_dqn_mlp_act_group_sel): the selected member indices, pinned and mapped, read in place by the launch.  ONE
    // buffer, no staging ring: group_act returns only after every launched member's sequence word has arrived, so no launch is in
    // flight when the host writes the next selection.
    PinnedArray<unsigned> sel_pin;
    // push (bdr_agent_group_push): PUSH_SLOTS slots of [GroupPushDesc[P] | the P packed records | the words of the prioritized rings];
    // k_group_push and the tree kernels behind it read a slot in place
    PinnedArray<uint8_t> push; size_t push_slot_bytes = 0; PushRing push_ring;
    std::vector<bdr_replay*> last_push_buffers;                         // the buffers of the last accepted push (distinctness checked once)
    // prioritized rings (bdr_agent_group_set_prioritized; per.hip k_per_*_group).  Member p on a prioritized ring is entry keys[p].per_j
    // of d_per (static descriptors, rewritten with d_args) and of a slot of per_words (STEP_SLOTS slots of P entries): the kernels that
    // read the slot run before AND after the step, so the round's last tree kernel publishes for it.
    bool prioritized = false;
    std::vector<PerGroupMember> h_per; DeviceArray<PerGroupMember> d_per;
    PinnedArray<PerGroupWords> per_words; StepRing per_ring;
    std::vector<PerGroupMember> h_per_push; DeviceArray<PerGroupMember> d_per_push;
    std::vector<uint64_t> per_push_uids;                                // uid of every prioritized ring of the last push, in member order
};

// ---- bdr_agent_group_push: one transition per member, one launch ------------------------------------------------------------------
// Member p's record sits in the slot exactly as bdr_replay_push lays it out for that ring (obs | next_obs | act | reward, flags at the
// ring's own offsets), 16-byte aligned like its destination `ring + head * stride`, so source and destination of every field share
// their alignment.  One wave per member - a CartPole record is 46 bytes in four fields, a quarter of one wave's 16-byte lanes - and
// four members per workgroup.  Exactly the bytes a standalone push defines are written: the two rows, act_bytes, reward and two flags.
struct GroupPushDesc { uint8_t* dst; uint32_t src_off, obs_bytes, next_off, act_off, tail_off, act_bytes; };
static_assert(sizeof(GroupPushDesc) == 32, "GroupPushDesc is read as two 16-byte halves");

__global__ __launch_bounds__(256) void k_group_push(const uint8_t* __restrict__ slot, unsigned P, unsigned* ticket, unsigned* seq_host, unsigned seq)
{
    const int lane = threadIdx.x & 63;
    const unsigned p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p < P) {
        const GroupPushDesc d = reinterpret_cast<const GroupPushDesc*>(slot)[p];
        const uint8_t* rec = slot + d.src_off;
        gp_copy(d.dst, rec, d.obs_bytes, lane);
        gp_copy(d.dst + d.next_off, rec + d.next_off, d.obs_bytes, lane);
        gp_copy(d.dst + d.act_off, rec + d.act_off, d.act_bytes, lane);
        gp_copy(d.dst + d.tail_off, rec + d.tail_off, 6, lane);   // reward f32, is_terminated, is_truncated
    }
    mf_group_done(ticket, seq_host, seq);   // every wave's loads of the slot have returned: their data went into the stores above
}

namespace {

// a slot may be rewritten: the launch numbered `launch` has published (0: the slot was never read).  Behind the fallback's stream
// synchronise nothing reads the slot any more, whatever the word says.
int32_t group_wait_seq(bdr_agent_group* g, uint64_t launch)
{
    bool arrived = false;
    return launch ? wait_seq_word(g->seq.host.get(), (unsigned)launch, g->stream, std::chrono::steady_clock::now(), &arrived) : BDR_OK;
}

// members[b] of a member list, b of all members (members == nullptr)
inline uint32_t group_member_at(const uint32_t* members, uint32_t b) { return members ? members[b] : b; }

// a list of buffers other than the one accepted last (`accepted`) must name P different rings; `accepted` is then cleared, and set
// again by the caller once its call is enqueued
int32_t group_distinct_buffers(std::vector<bdr_replay*>& accepted, bdr_replay* const* buffers, uint32_t P)
{
    if (accepted.size() == P && memcmp(accepted.data(), buffers, P * sizeof(bdr_replay*)) == 0) return BDR_OK;
    std::vector<const bdr_replay*> s(buffers, buffers + P);
    std::sort(s.begin(), s.end());
    BDR_REQUIRE(std::adjacent_find(s.begin(), s.end()) == s.end(), "two members share one replay buffer: every member needs its own");
    accepted.clear();
    return BDR_OK;
}

// a member's deferred report (its error words, its ring's NaN flag) under the member's number; the deferred mark stays
int32_t group_name_member(int32_t st, uint32_t p)
{
    const int deferred = bdr::g_err_deferred;
    const std::string msg = bdr::g_err;
    (void)fail(st, "member %u: %s", p, msg.c_str());
    bdr::g_err_deferred = deferred;
    return st;
}

// The form follows member 0: the layer form when it is an Mlp DQN agent whose one-workgroup step is ON and whose network / batch size
// does not take it; every other member 0 is judged by the one-workgroup rules, with their messages, as before.
bool group_takes_layer_form(const bdr_agent* a)
{
    if (strcmp(a->kind(), "dqn_mlp") != 0) return false;
    const DqnMlp* m = static_cast<const DqnMlp*>(a);
    return m->fused && m->gather_in_step && !m->fused_ok((int)m->cfg.batch_size);
}

// why `a` cannot be a member (nullptr: it can)
// layer_form: the group takes the layer form (group_takes_layer_form of member 0)
const char* group_ineligible(const bdr_agent* a, const DqnMlp** out, bool layer_form)
{
    if (strcmp(a->kind(), "dqn_mlp") != 0) return "not an Mlp DQN agent (kind dqn_mlp)";
    const DqnMlp* m = static_cast<const DqnMlp*>(a);
    *out = m;
    if (m->group) return "already a member of a group";
    if (layer_form) {   // (member 0 does not take the one-workgroup step: the layer form, one shape for all)
        if (m->fused_ok((int)m->cfg.batch_size)) return "it takes the one-workgroup step, member 0 the layer path: one form per group";
        if (const char* why = gl_layers_ineligible(m->gl_shape((int)m->cfg.batch_size))) return why;
    } else {
        if (!m->fused) return "the one-workgroup step is switched off (BDR_NO_MLP_FUSED)";
        if (!m->gather_in_step) return "the in-step sample is switched off (BDR_NO_STEP_GATHER)";
        if (!m->fused_ok((int)m->cfg.batch_size)) return "its network / batch size does not take the one-workgroup step (at most 4 layers up to 256 wide, batch <= 128, at most 8 32x32 blocks per phase)";
    }
    if (m->amsgrad) return "amsgrad";
    if (m->grad_comm) return "a gradient communicator is installed";
    if (m->prof) return "profiling is on";
    return nullptr;
}

// the in_kernel conditions of DqnMlp::opt_enqueue + the checks of DqnMlp::opt, without touching anything
int32_t group_check_buffers(bdr_agent_group* g, bdr_replay* const* buffers)
{
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {
        const DqnMlp* m = g->members[p];
        const bdr_replay* r = buffers[p];
        BDR_REQUIRE(r, "member %u: null buffer", p);
        BDR_REQUIRE(!m->prof && !m->grad_comm, "member %u: profiling or a gradient communicator was switched on after the group was created", p);
        BDR_REQUIRE(r->obs_bytes == (uint64_t)m->net.in_dim * 4, "member %u: replay obs rows (%llu B) do not match the Mlp input (%d f32)", p,
                    (unsigned long long)r->obs_bytes, m->net.in_dim);
        BDR_REQUIRE(r->act_bytes >= 8, "member %u: discrete actions are stored as i64", p);
        BDR_REQUIRE(r->device == g->device, "member %u: its replay buffer lives on another device", p);
        BDR_REQUIRE(!r->per || !g->layers, "member %u: a prioritized buffer cannot be stepped by a layer-form group (prioritized replay under the layer form is not built)", p);
        BDR_REQUIRE(!r->per || g->prioritized, "member %u: a prioritized buffer cannot be stepped by a group (the in-step sample covers the uniform ring)", p);
        BDR_REQUIRE(!r->frame_stack, "member %u: a single-frame store cannot be stepped by a group", p);
        BDR_REQUIRE(r->index_rng == BDR_RNG_STDRNG, "member %u: the in-step sample draws the StdRng index stream only", p);
        if (r->size == 0) return fail(BDR_ERR_EMPTY, "member %u: batch() on an empty replay buffer", p);
    }
    return group_distinct_buffers(g->last_buffers, buffers, P);   // workgroups run side by side: one ring (its batch arrays) per member
}

// one update round of every member: fill, advance the host state, one launch
int32_t group_round(bdr_agent_group* g, bdr_replay* const* buffers, bool last_round)
{
    const uint32_t P = (uint32_t)g->members.size();
    const uint64_t k = g->launches + 1;
    const unsigned seq = (unsigned)k;
    const auto step_slot = g->step_ring.next();
    BDR_TRY(group_wait_seq(g, step_slot.wait));
    MfStep* steps = g->steps.host.get() + (size_t)step_slot.slot * P;
    // prioritized rings (accepted by group_check_buffers only when the group is switched on): their words go into a slot of their own
    uint32_t n_per = 0;
    for (uint32_t p = 0; p < P; ++p) n_per += buffers[p]->per ? 1u : 0u;
    const auto per_slot = g->per_ring.next();
    PerGroupWords* per_words = nullptr;
    if (n_per) {
        BDR_TRY(group_wait_seq(g, per_slot.wait));
        per_words = g->per_words.host.get() + (size_t)per_slot.slot * P;
    }
    bool dirty = false, per_need_mm = false, per_any_all = false;
    uint64_t per_max_capacity = 0;
    uint32_t j = 0;
    for (uint32_t p = 0; p < P; ++p) {
        DqnMlp* m = g->members[p];
        bdr_replay* r = buffers[p];
        const int bs = (int)m->cfg.batch_size;
        BDR_TRY(m->ensure_batch(bs));
        BDR_TRY(m->td_buffer(bs));
        GatherArgs plan{};
        PerGroupMember pm{};
        if (r->per) {   // the head of replay_sample_on_stream; the sample itself is k_per_sample_group's
            BDR_TRY(replay_prepare_sample(r, bs, g->stream));
            BDR_TRY(per_group_describe(r->per, bs, &pm));
        } else {
            BDR_TRY(replay_sample_plan(r, bs, g->stream, &plan));
        }
        m->last_reward = r->b_reward; m->last_B = bs;
        m->defer_adam = false;
        m->track_with_next = last_round && m->soft_update_counter + 1 == m->cfg.soft_update_interval;
        bdr_agent_group::StaticKey& key = g->keys[p];
        const int per_j = r->per ? (int)j : -1;
        if (!key.valid || key.batch_gen != m->batch_gen || key.td_abs != m->td_abs || key.r_uid != r->uid || key.r_batch_gen != r->batch_gen ||
            key.weight != (const void*)pm.w || key.per_j != per_j) {
            // a prioritized member takes the step as update_critic_fused gives it standalone: no in-step sample, weight and td_abs set
            g->lds_bytes[p] = m->fused_static(g->h_args[p], bs, r->b_obs, r->b_next, r->b_act, (int)r->act_bytes, r->b_reward, r->b_term, pm.w,
                                              r->per ? nullptr : &plan);
            if (r->per) {
                pm.td = m->td_abs; pm.ixs = r->b_ixs;
                pm.ring = r->ring; pm.stride = (uint32_t)r->stride; pm.obs_bytes = (uint32_t)r->obs_bytes; pm.act_bytes = (uint32_t)r->act_bytes;
                pm.next_off = (uint32_t)r->next_off; pm.act_off = (uint32_t)r->act_off; pm.tail_off = (uint32_t)r->tail_off;
                pm.b_obs = r->b_obs; pm.b_next = r->b_next; pm.b_act = r->b_act; pm.b_reward = r->b_reward; pm.b_term = r->b_term; pm.b_trunc = r->b_trunc;
                memcpy(pm.key.k, r->key, sizeof pm.key.k);
                g->h_per[j] = pm;
            }
            key.valid = true; key.batch_gen = m->batch_gen; key.td_abs = m->td_abs; key.r_uid = r->uid; key.r_batch_gen = r->batch_gen;
            key.weight = pm.w; key.per_j = per_j;
            dirty = true;
        }
        if (r->per) {   // what replay_sample_on_stream advances, with per_sample's state
            PerGroupWords w = per_group_sample_advance(r->per);
            w.word_pos = r->word_pos;
            r->word_pos += (uint64_t)bs;   // one next_u32() per index
            r->read_pending = true; r->read_stream = g->stream;
            r->batch_n = (uint64_t)bs;
            per_words[j] = w;
            per_need_mm = per_need_mm || w.need_mm != 0;
            per_any_all = per_any_all || per_normalizes_all(r->per);
            per_max_capacity = std::max(per_max_capacity, per_capacity(r->per));
            ++j;
        }
        steps[p] = m->fused_step_advance(r->per ? nullptr : &plan);
    }
    if (dirty) {   // rare (first step, a reallocation, another ring): behind everything the stream still holds
        BDR_HIP(hipStreamSynchronize(g->stream));
        BDR_HIP(hipMemcpy(g->d_args.get(), g->h_args.data(), P * sizeof(MlpFusedArgs), hipMemcpyHostToDevice));
        if (n_per) BDR_HIP(hipMemcpy(g->d_per.get(), g->h_per.data(), n_per * sizeof(PerGroupMember), hipMemcpyHostToDevice));
    }
    PerGroupMember* const d_per = g->d_per.get();
    unsigned* const ticket = g->ticket.get();
    const PerGroupWords* per_words_dev = g->per_words.dev + (size_t)per_slot.slot * P;
    if (n_per) {   // every prioritized member's sample, weights and rows: one launch (two when a minimum has to be recomputed first)
        std::atomic_thread_fence(std::memory_order_release);
        if (per_need_mm) BDR_TRY(per_group_minmax(g->stream, d_per, per_words_dev, n_per, per_max_capacity, 0, PerGroupPublish{nullptr, nullptr, 0u}));
        BDR_TRY(per_group_sample(g->stream, d_per, per_words_dev, n_per));
        g->kernel_launches += per_need_mm ? 2 : 1;
    }
    // the LDS form only when every member has a plan: otherwise all take the global-memory form (same bits)
    size_t lds = 0;
    bool all_lds = true;
    for (uint32_t p = 0; p < P; ++p) { all_lds = all_lds && g->lds_bytes[p] != 0; lds = std::max(lds, g->lds_bytes[p]); }
    for (uint32_t p = 0; p < P; ++p) { g->members[p]->probe_form = all_lds ? BDR_DQN_MLP_FORM_LDS : BDR_DQN_MLP_FORM_GLOBAL; g->members[p]->probe_chunks = 0; }   // bdr_dqn_mlp_layer_probe
    const auto* args = (const MF_CONST_AS MlpFusedArgs*)g->d_args.get();
    const auto* st = (const MF_CONST_AS MfStep*)(g->steps.dev + (size_t)step_slot.slot * P);
    if (all_lds) {
        if (lds > g->lds_attr) {
            BDR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_dqn_mlp_step_lds_group), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            g->lds_attr = lds;
        }
        hipLaunchKernelGGL(k_dqn_mlp_step_lds_group, dim3(P), dim3(512), lds, g->stream, args, st, ticket, g->seq.dev, seq);
    } else {
        hipLaunchKernelGGL(k_dqn_mlp_step_group, dim3(P), dim3(512), 0, g->stream, args, st, ticket, g->seq.dev, seq);
    }
    g->launches = k; g->step_ring.record(k);
    BDR_HIP(hipGetLastError());
    g->kernel_launches += 1;
    if (n_per) {   // update_priority of every prioritized member (and the minimum the next `All` batch needs): the last of them publishes
        const PerGroupPublish pub{ticket, g->seq.dev, (unsigned)(k + 1)}, none{nullptr, nullptr, 0u};
        BDR_TRY(per_group_update(g->stream, d_per, n_per, per_any_all ? none : pub));
        if (per_any_all) BDR_TRY(per_group_minmax(g->stream, d_per, per_words_dev, n_per, per_max_capacity, 1, pub));
        g->kernel_launches += per_any_all ? 2 : 1;
        g->launches = k + 1; g->per_ring.record(k + 1);
        for (uint32_t p = 0; p < P; ++p) {
            if (!buffers[p]->per) continue;
            per_group_update_advance(buffers[p]->per);
            replay_end_write_on_stream(buffers[p], g->stream, 0);   // a tree update is a write of the ring: the group's stream is its last writer
        }
    }
    return BDR_OK;
}

// group_round for the layer form: per member what DqnMlp::opt_enqueue / update_critic do on the host for one update on the layer
// path, then the round's launches (GroupLayers::launch), the last of which publishes the round's number
int32_t group_round_layers(bdr_agent_group* g, bdr_replay* const* buffers, bool last_round)
{
    GroupLayers& gl = *g->layers;
    const uint32_t P = (uint32_t)g->members.size();
    const uint64_t k = g->launches + 1;
    const auto step_slot = g->step_ring.next();
    BDR_TRY(group_wait_seq(g, step_slot.wait));
    MfStep* steps = g->steps.host.get() + (size_t)step_slot.slot * P;
    bool dirty = false;
    for (uint32_t p = 0; p < P; ++p) {
        DqnMlp* m = g->members[p];
        bdr_replay* r = buffers[p];
        const int bs = (int)m->cfg.batch_size;
        BDR_TRY(m->ensure_batch(bs));
        BDR_TRY(m->td_buffer(bs));
        GatherArgs plan{};
        BDR_TRY(replay_sample_plan(r, bs, g->stream, &plan));   // the host half of replay_sample_on_stream; the rows are k_gather_group's
        m->last_reward = r->b_reward; m->last_B = bs;
        m->defer_adam = false;
        m->head_fused = gl.head != 0;
        m->probe_form = gl.head ? BDR_DQN_MLP_FORM_LAYERS_HEAD : BDR_DQN_MLP_FORM_LAYERS_TD;   // bdr_dqn_mlp_layer_probe
        m->probe_chunks = std::min(m->dw_chunks_l[0], std::max(1, bs / 256));
        m->track_with_next = last_round && m->soft_update_counter + 1 == m->cfg.soft_update_interval;
        bdr_agent_group::StaticKey& key = g->keys[p];
        if (!key.valid || key.batch_gen != m->batch_gen || key.td_abs != m->td_abs || key.r_uid != r->uid || key.r_batch_gen != r->batch_gen) {
            GlMemberArgs o;
            gl_member_static(m, bs, r, plan, o);
            BDR_REQUIRE(o.dw_grid == (int)gl.plan[gl.n_launches - 2].gx, "member %u: the weight-gradient grid (%d) differs from the plan's (%u)", p, o.dw_grid,
                        gl.plan[gl.n_launches - 2].gx);
            gl.stage(p, P, o);
            key.valid = true; key.batch_gen = m->batch_gen; key.td_abs = m->td_abs; key.r_uid = r->uid; key.r_batch_gen = r->batch_gen;
            dirty = true;
        }
        steps[p] = m->fused_step_advance(&plan);   // word_pos / size, adam_step and its scalars, the soft update riding on this round
    }
    if (dirty) {   // rare (first step, a reallocation, another ring): behind everything the stream still holds
        BDR_HIP(hipStreamSynchronize(g->stream));
        BDR_HIP(gl.upload(P));
    }
    std::atomic_thread_fence(std::memory_order_release);
    // (should a launch fail, k is the number of whatever the group launches next - later than every reader of the slot)
    g->launches = k; g->step_ring.record(k);
    BDR_TRY(gl.launch(g->stream, P, g->steps.dev + (size_t)step_slot.slot * P, g->ticket.get(), g->seq.dev, (unsigned)k));
    g->kernel_launches += (uint64_t)gl.n_launches;
    return BDR_OK;
}

// what bdr_agent_opt does around opt(), for every member, then the rounds
int32_t group_opt(bdr_agent_group* g, bdr_replay* const* buffers)
{
    BDR_HIP(hipSetDevice(g->device));
    BDR_TRY(group_check_buffers(g, buffers));
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {   // asynchronous: a device-side failure of an earlier step surfaces here without a synchronisation
        DqnMlp* m = g->members[p];
        unsigned w[bdr_agent::ERR_WORDS];
        m->err_mirror_read(w);
        BDR_TRY(m->err_report(w));
    }
    if (++g->poll_count % bdr_agent::ERR_POLL_INTERVAL == 0) {   // every member's error words -> its pinned mirror, one launch
        hipLaunchKernelGGL(k_group_err_mirror, dim3(P), dim3(64), 0, g->stream, (const MfErrRef*)g->d_err_refs.get(), (int)bdr_agent::ERR_WORDS);
        BDR_HIP(hipGetLastError());
        g->kernel_launches += 1;
    }
    for (uint32_t p = 0; p < P; ++p) g->members[p]->last_replay_uid = buffers[p]->uid;
    for (uint64_t u = 0; u < g->n_updates; ++u) BDR_TRY(g->layers ? group_round_layers(g, buffers, u + 1 == g->n_updates) : group_round(g, buffers, u + 1 == g->n_updates));
    for (uint32_t p = 0; p < P; ++p) BDR_TRY(g->members[p]->after_updates());   // (the soft update rode on the last round's launch: nothing is enqueued here)
    g->last_buffers.assign(buffers, buffers + P);
    return BDR_OK;
}

// one observation row per selected member -> those members' action values in the pinned result area (and each one's view of its error
// words).  members == nullptr: all of them, through the full entry; otherwise members[0..n) (checked by the caller: strictly
// ascending, every index < P, rows not NULL) - a full list takes the full entry too, so the default path enqueues what it always did.
int32_t group_act(bdr_agent_group* g, const void* const* obs, const uint32_t* members = nullptr, uint32_t n = 0)
{
    BDR_HIP(hipSetDevice(g->device));
    const uint32_t P = (uint32_t)g->members.size();
    if (members && n == P) members = nullptr;   // strictly ascending and n == P: every member
    const uint32_t N = members ? n : P;
    for (uint32_t b = 0; b < N; ++b) {
        const uint32_t p = group_member_at(members, b);
        BDR_REQUIRE(p < P, "member %u of a group of %u", p, P);   // (the kernel indexes the members' arrays with it)
        BDR_REQUIRE(obs[p], "member %u: null observation row", p);
    }
    for (uint32_t b = 0; b < N; ++b) {
        const uint32_t p = group_member_at(members, b);
        memcpy(g->obs_pin.host.get() + g->obs_off[p], obs[p], (size_t)g->members[p]->net.in_dim * 4);
        if (members) g->sel_pin.host.get()[b] = p;
    }
    const unsigned seq = ++g->act_seq;
    const auto* act_args = (const MF_CONST_AS MfActArgs*)g->d_act.get();
    if (members) {
        std::atomic_thread_fence(std::memory_order_release);
        hipLaunchKernelGGL(k_dqn_mlp_act_group_sel, dim3(N), dim3(512), 0, g->stream, act_args, (const MF_CONST_AS unsigned*)g->sel_pin.dev,
                           (const float*)g->obs_pin.dev, g->act_pin.dev, seq);
    } else {
        hipLaunchKernelGGL(k_dqn_mlp_act_group, dim3(P), dim3(512), 0, g->stream, act_args, (const float*)g->obs_pin.dev, g->act_pin.dev, seq);
    }
    BDR_HIP(hipGetLastError());
    g->kernel_launches += 1;
    const auto slot_words = [&](uint32_t b) { return reinterpret_cast<const volatile unsigned*>(g->act_pin.host.get() + (size_t)group_member_at(members, b) * MF_ACT_SLOT); };
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t b = 0; b < N; ++b) {
        bool arrived = false;
        BDR_TRY(wait_seq_word(slot_words(b), seq, g->stream, t0, &arrived));
        if (!arrived) return fail(BDR_ERR_HIP, "the action values of a group acting call never arrived in host memory");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    for (uint32_t b = 0; b < N; ++b) g->members[group_member_at(members, b)]->err_adopt(slot_words(b) + 4);
    return BDR_OK;
}

// the per-member tail of Policy::sample behind group_act, for the members members[0..n) (nullptr: all), in member order
int32_t group_sample_tail(bdr_agent_group* g, const uint32_t* members, uint32_t n, int64_t* act_out, bdr_sample_info* info)
{
    const uint32_t N = members ? n : (uint32_t)g->members.size();
    for (uint32_t b = 0; b < N; ++b) {   // the forward brought each member's error words along: report from them, as bdr_agent_sample does
        const uint32_t p = group_member_at(members, b);
        DqnMlp* m = g->members[p];
        unsigned w[bdr_agent::ERR_WORDS];
        m->err_mirror_read(w);
        BDR_TRY(m->err_report(w));
        bool alive = false;
        const int32_t st = replay_per_check(m->last_replay_uid, &alive);
        if (!alive) m->last_replay_uid = 0;
        if (st != BDR_OK) return g->prioritized ? group_name_member(st, p) : st;
    }
    for (uint32_t b = 0; b < N; ++b) {
        const uint32_t p = group_member_at(members, b);
        DqnMlp* m = g->members[p];
        BDR_TRY(bdr::explore_actions(m, 1, g->act_pin.host.get() + (size_t)p * MF_ACT_SLOT + 16, m->net.out_dim, act_out + p, info ? info + p : nullptr));
    }
    return BDR_OK;
}

// every refusal of a grouped push, before anything moves
int32_t group_check_push(bdr_agent_group* g, bdr_replay* const* buffers, const void* const* obs, const void* const* next_obs)
{
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {
        const DqnMlp* m = g->members[p];
        const bdr_replay* r = buffers[p];
        BDR_REQUIRE(r, "member %u: null buffer", p);
        BDR_REQUIRE(obs[p] && next_obs[p], "member %u: null observation row", p);
        BDR_REQUIRE(r->device == g->device, "member %u: its replay buffer lives on another device", p);
        BDR_REQUIRE(!r->per || !g->layers, "member %u: a prioritized buffer cannot take the push of a layer-form group (prioritized replay under the layer form is not built)", p);
        BDR_REQUIRE(!r->per || g->prioritized, "member %u: a prioritized buffer cannot take a grouped push (its sum tree is updated by bdr_replay_push)", p);
        BDR_REQUIRE(!r->frame_stack, "member %u: a single-frame store cannot take a grouped push", p);
        BDR_REQUIRE(r->obs_bytes == (uint64_t)m->net.in_dim * 4, "member %u: replay obs rows (%llu B) do not match the Mlp input (%d f32)", p,
                    (unsigned long long)r->obs_bytes, m->net.in_dim);
        BDR_REQUIRE(r->act_bytes == 8, "member %u: a grouped push stores one i64 action per row (act_row_bytes %llu)", p, (unsigned long long)r->act_bytes);
    }
    return group_distinct_buffers(g->last_push_buffers, buffers, P);   // waves run side by side, and every ring's head moves by one
}

int32_t group_push(bdr_agent_group* g, bdr_replay* const* buffers, const void* const* obs, const int64_t* act, const void* const* next_obs,
                   const float* reward, const int8_t* term, const int8_t* trunc)
{
    BDR_HIP(hipSetDevice(g->device));
    BDR_TRY(group_check_push(g, buffers, obs, next_obs));
    const uint32_t P = (uint32_t)g->members.size();
    // the slot: descriptors, then the records (each a multiple of 16 bytes)
    size_t need = (size_t)P * sizeof(GroupPushDesc);
    for (uint32_t p = 0; p < P; ++p) need += (size_t)round_up(buffers[p]->tail_off + 8, 16);
    uint32_t n_per = 0;   // prioritized rings: their words follow the records
    for (uint32_t p = 0; p < P; ++p) n_per += buffers[p]->per ? 1u : 0u;
    const size_t words_off = need;
    need += (size_t)n_per * sizeof(PerGroupWords);
    if (need > g->push_slot_bytes) {   // first push, or wider rings than before: rare, behind everything the stream still holds
        BDR_HIP(hipStreamSynchronize(g->stream));
        const size_t bytes = (size_t)round_up((uint64_t)need, 256);
        BDR_HIP(pinned_array(g->push, bdr_agent_group::PUSH_SLOTS * bytes));
        g->push_slot_bytes = bytes;
        g->push_ring.reset();
    }
    const auto push_slot = g->push_ring.next();
    BDR_TRY(group_wait_seq(g, push_slot.wait));
    // order the group's stream behind each ring's last reader and writer: nothing to do when both were this stream
    for (uint32_t p = 0; p < P; ++p) BDR_TRY(replay_begin_write_on_stream(buffers[p], g->stream));
    const size_t slot_off = (size_t)push_slot.slot * g->push_slot_bytes;
    uint8_t* base = g->push.host.get() + slot_off;
    GroupPushDesc* desc = reinterpret_cast<GroupPushDesc*>(base);
    size_t off = (size_t)P * sizeof(GroupPushDesc);
    for (uint32_t p = 0; p < P; ++p) {
        const bdr_replay* r = buffers[p];
        uint8_t* rec = base + off;
        memcpy(rec, obs[p], r->obs_bytes);
        memcpy(rec + r->next_off, next_obs[p], r->obs_bytes);
        memcpy(rec + r->act_off, &act[p], 8);
        memcpy(rec + r->tail_off, &reward[p], 4);
        rec[r->tail_off + 4] = (uint8_t)term[p];
        rec[r->tail_off + 5] = (uint8_t)trunc[p];
        desc[p] = GroupPushDesc{r->ring + r->i * r->stride, (uint32_t)off, (uint32_t)r->obs_bytes, (uint32_t)r->next_off, (uint32_t)r->act_off,
                                (uint32_t)r->tail_off, 8u};
        off += (size_t)round_up(r->tail_off + 8, 16);
    }
    bool per_need_mm = false;
    uint64_t per_max_capacity = 0;
    if (n_per) {   // set_priority(1) of every prioritized ring (base.rs:227-235): the tree descriptors, then this push's words
        bool same = g->per_push_uids.size() == n_per;
        uint32_t j = 0;
        for (uint32_t p = 0; p < P && same; ++p) if (buffers[p]->per) same = g->per_push_uids[j++] == buffers[p]->uid;
        if (!same) {   // rare (first push, other rings): behind everything the stream still holds
            g->per_push_uids.clear();
            j = 0;
            for (uint32_t p = 0; p < P; ++p) {
                if (!buffers[p]->per) continue;
                PerGroupMember pm{};
                BDR_TRY(per_group_describe(buffers[p]->per, 1, &pm));
                g->h_per_push[j++] = pm;
            }
            BDR_HIP(hipStreamSynchronize(g->stream));
            BDR_HIP(hipMemcpy(g->d_per_push.get(), g->h_per_push.data(), n_per * sizeof(PerGroupMember), hipMemcpyHostToDevice));
            for (uint32_t p = 0; p < P; ++p) if (buffers[p]->per) g->per_push_uids.push_back(buffers[p]->uid);
        }
        PerGroupWords* words = reinterpret_cast<PerGroupWords*>(base + words_off);
        j = 0;
        for (uint32_t p = 0; p < P; ++p) {
            bdr_replay* r = buffers[p];
            if (!r->per) continue;
            PerGroupWords w = per_group_push_advance(r->per);
            w.head = (uint32_t)r->i;
            words[j++] = w;
            per_need_mm = per_need_mm || w.need_mm != 0;
            per_max_capacity = std::max(per_max_capacity, per_capacity(r->per));
        }
    }
    std::atomic_thread_fence(std::memory_order_release);
    const uint64_t k = g->launches + 1;
    hipLaunchKernelGGL(k_group_push, dim3((P + 3) / 4), dim3(256), 0, g->stream, (const uint8_t*)(g->push.dev + slot_off), P, g->ticket.get(), g->seq.dev,
                       (unsigned)k);
    BDR_HIP(hipGetLastError());
    // the tree kernels read the slot too: the last of them publishes, under a launch number of its own.  (Should one of them fail to
    // launch, k + 1 is the number of whatever the group launches next - later than every reader of the slot.)
    g->kernel_launches += 1;
    g->launches = k; g->push_ring.record(n_per ? k + 1 : k);
    if (n_per) {
        const PerGroupWords* words_dev = reinterpret_cast<const PerGroupWords*>(g->push.dev + slot_off + words_off);
        PerGroupMember* const d_per_push = g->d_per_push.get();
        if (per_need_mm) BDR_TRY(per_group_minmax(g->stream, d_per_push, words_dev, n_per, per_max_capacity, 0, PerGroupPublish{nullptr, nullptr, 0u}));
        BDR_TRY(per_group_push(g->stream, d_per_push, words_dev, n_per, PerGroupPublish{g->ticket.get(), g->seq.dev, (unsigned)(k + 1)}));
        g->kernel_launches += per_need_mm ? 2 : 1;
        g->launches = k + 1;
    }
    for (uint32_t p = 0; p < P; ++p) replay_end_write_on_stream(buffers[p], g->stream, 1);
    g->last_push_buffers.assign(buffers, buffers + P);
    return BDR_OK;
}

}  // namespace

extern "C" {

int32_t bdr_agent_group_create(bdr_agent* const* agents, uint32_t n, bdr_agent_group** out)
{
    BDR_REQUIRE(agents && out, "null argument");
    BDR_REQUIRE(n >= 1 && n <= 65535, "a group has 1 .. 65535 members");
    std::vector<DqnMlp*> ms;
    BDR_REQUIRE(agents[0], "member 0: null agent");
    const bool layer_form = group_takes_layer_form(agents[0]);
    for (uint32_t p = 0; p < n; ++p) {
        BDR_REQUIRE(agents[p], "member %u: null agent", p);
        const DqnMlp* m = nullptr;
        const char* why = group_ineligible(agents[p], &m, layer_form);
        BDR_REQUIRE(!why, "member %u cannot join a group: %s", p, why);
        if (layer_form) {
            const DqnMlp* m0 = static_cast<const DqnMlp*>(agents[0]);
            BDR_REQUIRE(gl_same_shape(m->gl_shape((int)m->cfg.batch_size), m0->gl_shape((int)m0->cfg.batch_size)),
                        "member %u cannot join a group: its shape (in_dim, units, out_dim, activation_out, batch_size, double_dqn) differs from member 0's - one shape per layer-form group", p);
        }
        BDR_REQUIRE(m->device == agents[0]->device, "member %u lives on device %d, member 0 on device %d", p, m->device, agents[0]->device);
        BDR_REQUIRE(m->cfg.n_updates_per_opt == static_cast<const DqnMlp*>(agents[0])->cfg.n_updates_per_opt,
                    "member %u has n_updates_per_opt %llu, member 0 has %llu: one value per group", p, (unsigned long long)m->cfg.n_updates_per_opt,
                    (unsigned long long)static_cast<const DqnMlp*>(agents[0])->cfg.n_updates_per_opt);
        for (uint32_t o = 0; o < p; ++o) BDR_REQUIRE(agents[o] != agents[p], "member %u is member %u once more", p, o);
        ms.push_back(static_cast<DqnMlp*>(agents[p]));
    }
    std::unique_ptr<bdr_agent_group> g(new bdr_agent_group());
    g->device = ms[0]->device; g->n_updates = ms[0]->cfg.n_updates_per_opt;
    BDR_HIP(hipSetDevice(g->device));
    const size_t P = n;
    // acting arguments: fixed for the members' lifetime (the arenas and the error words are never reallocated)
    std::vector<MfActArgs> act(P);
    std::vector<MfErrRef> refs(P);
    g->obs_off.resize(P);
    for (size_t p = 0; p < P; ++p) {
        DqnMlp* m = ms[p];
        MfActArgs& a = act[p];
        memset(&a, 0, sizeof a);
        a.L = (int)m->net.L.size(); a.A = m->net.out_dim; a.in_dim = m->net.in_dim;
        for (int i = 0; i < a.L; ++i) { a.Kp[i] = m->net.L[i].Kp; a.Np[i] = m->net.L[i].Np; a.relu[i] = m->net.L[i].relu; a.w[i] = m->net.L[i].w; a.b[i] = m->net.L[i].b; }
        a.params = m->q; a.dev_err = m->dev_err;
        g->obs_off[p] = g->obs_floats; a.obs_off = g->obs_floats;
        g->obs_floats += (unsigned)round_up((uint64_t)m->net.in_dim, 4);
        if (!m->host_err_dev) BDR_HIP(hipHostGetDevicePointer((void**)&m->host_err_dev, m->host_err, 0));
        refs[p] = MfErrRef{m->dev_err, m->host_err_dev};
    }
    // (a failure below leaves nothing adopted: the partially built group releases what it holds)
    BDR_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    if (layer_form) {   // the layer form's argument arrays instead of d_args
        g->layers.reset(new GroupLayers());
        BDR_HIP(g->layers->allocate(ms[0]->gl_shape((int)ms[0]->cfg.batch_size), P));
        BDR_REQUIRE(g->layers->n_launches >= 3, "the layer-form launch plan is empty");
        for (int i = 0; i < g->layers->n_launches; ++i)
            BDR_REQUIRE(gl_grid_ok(g->layers->plan[i]), "%u members of this shape: the grid of %s exceeds the launch limits", n, gl_kernel_name(g->layers->plan[i].kernel));
    } else {
        BDR_HIP(device_array(g->d_args, P));
    }
    BDR_HIP(device_array(g->d_act, P));
    BDR_HIP(device_array(g->d_err_refs, P));
    BDR_HIP(device_array(g->ticket, 1));
    BDR_HIP(hipMemset(g->ticket.get(), 0, sizeof(unsigned)));
    BDR_HIP(hipMemcpy(g->d_act.get(), act.data(), P * sizeof(MfActArgs), hipMemcpyHostToDevice));
    BDR_HIP(hipMemcpy(g->d_err_refs.get(), refs.data(), P * sizeof(MfErrRef), hipMemcpyHostToDevice));
    BDR_HIP(pinned_array(g->steps, bdr_agent_group::STEP_SLOTS * P));
    BDR_HIP(pinned_array(g->seq, 16));   // (one word, a cache line of its own)
    BDR_HIP(pinned_array(g->obs_pin, g->obs_floats));
    BDR_HIP(pinned_array(g->act_pin, P * MF_ACT_SLOT));
    BDR_HIP(pinned_array(g->sel_pin, P));
    g->keys.resize(P); g->h_args.resize(P); g->lds_bytes.assign(P, 0);
    // adopt: the member's own stream is drained, retired and destroyed; the member enqueues on the group's stream from now on
    for (size_t p = 0; p < P; ++p) BDR_HIP(hipStreamSynchronize(ms[p]->stream));
    for (size_t p = 0; p < P; ++p) {
        DqnMlp* m = ms[p];
        hipStream_t old = m->stream;
        m->stream = g->stream; m->group = g.get();
        if (old) { stream_retire(old); (void)hipStreamDestroy(old); }
    }
    g->members = std::move(ms);
    *out = g.release();
    return BDR_OK;
}

int32_t bdr_agent_group_destroy(bdr_agent_group* g)
{
    if (!g) return BDR_OK;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->stream);
    for (DqnMlp* m : g->members) {   // the group owns its members; their stream is the group's, destroyed once below
        m->group = nullptr; m->stream = nullptr;
        (void)bdr_agent_destroy(m);
    }
    delete g;   // retires and destroys the stream, then releases the buffers
    return BDR_OK;
}

int32_t bdr_agent_group_size(const bdr_agent_group* g, uint32_t* n)
{
    BDR_REQUIRE(g && n, "null argument");
    *n = (uint32_t)g->members.size();
    return BDR_OK;
}

int32_t bdr_agent_group_member(const bdr_agent_group* g, uint32_t i, bdr_agent** out)
{
    BDR_REQUIRE(g && out, "null argument");
    BDR_REQUIRE(i < g->members.size(), "member %u of a group of %u", i, (unsigned)g->members.size());
    *out = g->members[i];
    return BDR_OK;
}

int32_t bdr_agent_group_info(const bdr_agent_group* g, bdr_group_info* out)
{
    BDR_REQUIRE(g && out, "null argument");
    memset(out, 0, sizeof *out);
    out->form = g->layers ? BDR_GROUP_FORM_LAYERS : BDR_GROUP_FORM_ONE_WORKGROUP;
    out->n_members = (uint32_t)g->members.size();
    out->launches_per_round = g->layers ? (uint32_t)g->layers->n_launches : 1u;
    out->kernel_launches = g->kernel_launches;
    return BDR_OK;
}

int32_t bdr_agent_group_set_prioritized(bdr_agent_group* g, int32_t on)
{
    BDR_REQUIRE(g, "null group");
    BDR_REQUIRE(on == 0 || on == 1, "on must be 0 or 1 (got %d)", on);
    BDR_REQUIRE(!on || !g->layers, "prioritized replay under a layer-form group is not built: its members step prioritized rings standalone");
    if (on && !g->d_per) {   // the arrays of the tree kernels, once
        BDR_HIP(hipSetDevice(g->device));
        const size_t P = g->members.size();
        DeviceArray<PerGroupMember> d, dp;   // all three or none
        PinnedArray<PerGroupWords> w;
        hipError_t e = device_array(d, P);
        if (e == hipSuccess) e = device_array(dp, P);
        if (e == hipSuccess) e = pinned_array(w, bdr_agent_group::STEP_SLOTS * P);
        if (e != hipSuccess) return fail(BDR_ERR_HIP, "allocating the group's prioritized-replay arrays failed: %s", hipGetErrorString(e));
        g->d_per = std::move(d); g->d_per_push = std::move(dp); g->per_words = std::move(w);
        g->h_per.resize(P); g->h_per_push.resize(P);
    }
    g->prioritized = on != 0;
    return BDR_OK;
}

int32_t bdr_agent_group_opt(bdr_agent_group* g, bdr_replay* const* buffers)
{
    BDR_REQUIRE(g && buffers, "null argument");
    return group_opt(g, buffers);
}

int32_t bdr_agent_group_push(bdr_agent_group* g, bdr_replay* const* buffers, const void* const* obs, const int64_t* act, const void* const* next_obs,
                             const float* reward, const int8_t* is_terminated, const int8_t* is_truncated)
{
    BDR_REQUIRE(g && buffers && obs && act && next_obs && reward && is_terminated && is_truncated, "null argument");
    return group_push(g, buffers, obs, act, next_obs, reward, is_terminated, is_truncated);
}

int32_t bdr_agent_group_opt_with_scalars(bdr_agent_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    BDR_REQUIRE(g && buffers && out && n_out, "null argument");
    BDR_REQUIRE(cap_per_member >= 1, "cap_per_member must be positive");
    BDR_TRY(group_opt(g, buffers));
    BDR_HIP(hipStreamSynchronize(g->stream));   // the one synchronisation: every record() below finds the stream idle
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {
        DqnMlp* m = g->members[p];
        int n = 0;
        m->rec_opt = true;
        const int32_t st = m->record(out + (size_t)p * cap_per_member, cap_per_member, &n);
        m->rec_opt = false;
        BDR_TRY(st);
        n_out[p] = n;
    }
    for (uint32_t p = 0; p < P; ++p) {   // the records are complete whatever the error words say about the step that produced them
        const int32_t st = g->members[p]->err_check();
        if (st != BDR_OK) { if (bdr::g_err_deferred) bdr::g_err_deferred = 2; return st; }
    }
    return BDR_OK;
}

int32_t bdr_agent_group_qvalues(bdr_agent_group* g, const void* const* obs, float* const* q_out)
{
    BDR_REQUIRE(g && obs && q_out, "null argument");
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) BDR_REQUIRE(q_out[p], "member %u: null output row", p);
    BDR_TRY(group_act(g, obs));
    for (uint32_t p = 0; p < P; ++p) memcpy(q_out[p], g->act_pin.host.get() + (size_t)p * MF_ACT_SLOT + 16, (size_t)g->members[p]->net.out_dim * 4);
    return BDR_OK;
}

int32_t bdr_agent_group_sample(bdr_agent_group* g, const void* const* obs, int64_t* act_out, bdr_sample_info* info)
{
    BDR_REQUIRE(g && obs && act_out, "null argument");
    BDR_TRY(group_act(g, obs));
    return group_sample_tail(g, nullptr, 0, act_out, info);
}

int32_t bdr_agent_group_sample_members(bdr_agent_group* g, const uint32_t* members, uint32_t n, const void* const* obs, int64_t* act_out,
                                       bdr_sample_info* info)
{
    BDR_REQUIRE(g && members && obs && act_out, "null argument");
    const uint32_t P = (uint32_t)g->members.size();
    BDR_REQUIRE(n >= 1, "an empty member list");
    for (uint32_t b = 0; b < n; ++b) {   // everything is refused before anything moves
        BDR_REQUIRE(members[b] < P, "member %u of a group of %u", members[b], P);
        BDR_REQUIRE(b == 0 || members[b] > members[b - 1], "the member list must be strictly ascending (%u follows %u)", members[b], members[b - 1]);
        BDR_REQUIRE(obs[members[b]], "member %u: null observation row", members[b]);
    }
    BDR_TRY(group_act(g, obs, members, n));
    return group_sample_tail(g, members, n, act_out, info);
}

int32_t bdr_agent_group_sync(bdr_agent_group* g)
{
    BDR_REQUIRE(g, "null group");
    BDR_HIP(hipSetDevice(g->device));
    BDR_HIP(hipStreamSynchronize(g->stream));
    for (size_t p = 0; p < g->members.size(); ++p) {
        DqnMlp* m = g->members[p];
        BDR_TRY(m->after_sync());
        const int32_t st = m->err_check();
        if (st != BDR_OK) return g->prioritized ? group_name_member(st, (uint32_t)p) : st;
    }
    return BDR_OK;
}

}  // extern "C"
