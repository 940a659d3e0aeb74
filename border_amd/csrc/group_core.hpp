// ================================================================================================
// A launch grouping of dense agents, the host half, once (bc_group.hpp: BC; iql_group.hpp: IQL; awac_group.hpp: AWAC): Agent::opt of every member in the
// launch sequence the agent enqueues for ONE member, every launch serving ALL members - the member index is grid dimension y.  A launch
// grouping, not an agent kind: the members stay ordinary agents on the group's stream.  The protocol: adopt the members onto one
// stream, check the buffers, take a slot of the pinned step ring, re-stage the static arguments of the members whose key has moved,
// walk the launch plan, publish the launch number, collect records, sync, destroy.
//   static arguments   one device array per kernel family (the Kind's StagedArrays), rewritten only when a member's batch buffers or
//                      its ring change, or a hyperparameter of it is set (`keys`: the member's batch_gen and hyper_gen, the ring's uid
//                      and batch_gen), synchronously, behind a stream synchronise: rare
//   per step           Kind::Step[P] in a slot of the pinned, device-mapped step ring: the gather reads word_pos and size of the
//                      member's entry (GatherStepWords at its start), the reduce + Adam launches its AdamScalars
// The slot rule (slot_ring.hpp): the LAST launch of a round that reads the slot - the kind's final reduce + Adam - ends with the ticket
// and publishes the round's launch number (bg_group_done, group_done.hpp - all workgroups of its grid counted, behind a barrier every
// thread reaches).  The host rewrites a slot only once the pinned word has reached the number recorded for it: no copy command, event
// or synchronise in the steady loop.  Acting calls (group_act.hpp) take their numbers from the same counter.
// The grouped push of the online kinds (AWAC, candle SAC: group_push below, k_cgroup_push in group_push.hpp) has a pinned ring of its
// own under the same rule - PUSH_SLOTS slots of PUSH_SLOT_BYTES, a slot = [CGroupPushDesc[P] | every member's n records] - and takes
// its numbers from the same counter; the push kernel is the only reader of its slot and publishes its own number.
// Copies of training state between members (group_copy.hpp: group_copy_members, k_group_copy) have a third ring under the same rule -
// GC_SLOTS slots of segment tables - and take their numbers from the same counter.
// Bounds: a slot and every per-member argument array hold P = members.size() entries, the length of `keys` and of the buffer list of
// an opt; slot.slot < STEP_SLOTS, and `steps` holds STEP_SLOTS * P entries.  The bounds of the indices a kind's launches add (its
// dense, dW and reduce arrays) are stated in the kind's file, those of the kinds on dense_group.hpp once, there.
// A Kind says what differs:
//   Member, Shape, Launch, Step, MemberArgs, PlanMember, Act        the types (Act: the acting kind of group_act.hpp)
//   KIND, A, NAME                                                   the member's kind() string and its name in messages ("a BC", "BC")
//   MAX_LAUNCHES, K_GATHER, FORM, MIN_CAP, CAP_MSG                  the plan's capacity and gather kernel, the bdr_group_info form, the
//                                                                   least cap_per_member of opt_with_scalars and its message
//   describe(m), refusal(..), kernel_name(k), round_plan(..), launch_count(shape)   the rule of its plan header
//   fill_step(m, bs, plan)                                          this step's words; advances the member's step counters, n_opts, last_B (AWAC: and
//                                                                   reads its mode and takes the round's draws of its noise counter)
//   member_static(m, bs, r, plan, o)                                one member's static arguments
//   allocate(shape, P), stage(p, P, o), upload()                    its StagedArrays
//   check_static(plan, n, o, p)                                     the plan's weight-gradient grids against the member's
//   launch(g, P, steps_dev, seq_no)                                 one round's launches (the switch over its own kernels)
// For the kinds with network instances (IQL, AWAC, candle SAC) the dense half of the last four is written once: dense_group.hpp's DenseRound.
#pragma once
#include <algorithm>
#include <atomic>
#include <memory>
#include <vector>

#include "slot_ring.hpp"
#include "device_arrays.hpp"
#include "group_done.hpp"
#include "group_act.hpp"
#include "group_push.hpp"
#include "group_copy.hpp"
#include "group_plan_common.hpp"

namespace {

template <class K>
struct GroupCore {
    using Kind = K;
    enum { STEP_SLOTS = 8, PUSH_SLOTS = 8, PUSH_SLOT_BYTES = 64 * 1024 };
    int32_t device = 0;
    hipStream_t stream = nullptr;
    // (group_destroy has synchronised the stream and destroyed the members; a failed create has adopted nobody.)  The stream goes
    // first, the buffers - the members below - after it.
    ~GroupCore() { if (stream) { stream_retire(stream); (void)hipStreamDestroy(stream); } }
    std::vector<typename K::Member*> members;
    typename K::Shape shape{};       // the one shape of all members
    typename K::Launch plan[K::MAX_LAUNCHES]; int n_launches = 0;
    uint64_t kernel_launches = 0;    // every kernel launch the group's own calls have enqueued (bdr_*_group_info)
    struct StaticKey { bool valid = false; uint64_t batch_gen = 0, hyper_gen = 0, r_uid = 0, r_batch_gen = 0; };
    std::vector<StaticKey> keys;
    K kind;                                                             // the static arguments of its kernel families
    PinnedArray<typename K::Step> steps; SlotRing<STEP_SLOTS> step_ring;   // [STEP_SLOTS][P]
    PinnedArray<unsigned> seq;                                          // pinned word: the launch number published last
    DeviceArray<unsigned> ticket;
    uint64_t launches = 0;                                              // launch numbers given out so far (1-based)
    std::vector<bdr_replay*> last_buffers;                              // the buffers of the last accepted opt (distinctness checked once)
    GroupAct<typename K::Act::Call> act;                                // group acting (group_act.hpp): static arguments, call words, staging areas
    // push (group_push below): PUSH_SLOTS slots of PUSH_SLOT_BYTES, [CGroupPushDesc[P] | every member's n records]; allocated by the
    // first push, read in place by k_cgroup_push (group_push.hpp)
    PinnedArray<uint8_t> push; SlotRing<PUSH_SLOTS> push_ring;
    std::vector<bdr_replay*> last_push_buffers;                         // the buffers of the last accepted push (distinctness checked once)
    // copies between members (group_copy.hpp): GC_SLOTS slots of min(65535, (P - 1) x arenas) segments; allocated by the first copy,
    // read in place by k_group_copy
    PinnedArray<GroupCopySeg> copy; SlotRing<GC_SLOTS> copy_ring;

    hipError_t allocate(size_t P)
    {
        keys.resize(P);
        hipError_t e = kind.allocate(shape, P);
        if (e == hipSuccess) e = device_array(ticket, 1);
        if (e == hipSuccess) e = hipMemset(ticket.get(), 0, sizeof(unsigned));
        if (e == hipSuccess) e = pinned_array(steps, (size_t)STEP_SLOTS * P);
        if (e == hipSuccess) e = pinned_array(seq, 16);   // (one word, a cache line of its own)
        return e;
    }
};

// ---- create: every refusal, then stream, arrays, and the adoption with nothing adopted on failure -------------------------------------
template <class G>
int32_t group_create(bdr_agent* const* agents, uint32_t n, G** out)
{
    using K = typename G::Kind;
    BDR_REQUIRE(agents && out, "null argument");
    BDR_REQUIRE(n >= 1 && n <= bdr::GP_MAX_MEMBERS, "a group has 1 .. 65535 members");
    std::vector<typename K::Member*> ms;
    std::vector<typename K::PlanMember> desc;
    for (uint32_t p = 0; p < n; ++p) {
        BDR_REQUIRE(agents[p], "member %u: null agent", p);
        BDR_REQUIRE(!strcmp(agents[p]->kind(), K::KIND), "member %u cannot join %s group: not %s agent (kind %s)", p, K::A, K::A, agents[p]->kind());
        BDR_REQUIRE(!agents[p]->group, "member %u cannot join %s group: already a member of a group", p, K::A);
        ms.push_back(static_cast<typename K::Member*>(agents[p]));
        desc.push_back(K::describe(ms.back()));
    }
    const char* why = nullptr;
    int kernel = -1;
    const int who = K::refusal(desc.data(), n, &why, &kernel);
    if (who == bdr::GP_NO_MEMBER) return kernel >= 0 ? fail(BDR_ERR_INVALID, "%u members of this shape: %s (%s)", n, why, K::kernel_name(kernel)) : fail(BDR_ERR_INVALID, "%s", why);
    BDR_REQUIRE(who == bdr::GP_OK, "member %d cannot join %s group: %s", who, K::A, why);
    std::unique_ptr<G> g(new G());
    g->device = ms[0]->device;
    BDR_HIP(hipSetDevice(g->device));
    g->shape = desc[0].shape;
    g->n_launches = K::round_plan(g->shape, n, g->plan);
    BDR_REQUIRE(g->n_launches == K::launch_count(g->shape), "the %s group launch plan is incomplete", K::NAME);
    {   // the gather's grid is replay_gather_group's own: it must be the one the plan has checked against the limits
        uint32_t chunks = 1, vec_per_chunk = 0;
        replay_gather_shape((uint64_t)g->shape.obs_dim * 4, &chunks, &vec_per_chunk);
        BDR_REQUIRE((unsigned)g->shape.batch * chunks == g->plan[0].gx && g->plan[0].kernel == K::K_GATHER,
                    "the gather's grid (%u workgroups per row) differs from the plan's (is BDR_GATHER_CHUNKS set?): no %s group", chunks, K::NAME);
    }
    // (a failure below leaves nothing adopted: the partially built group releases what it holds)
    BDR_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    BDR_HIP(g->allocate(n));
    // adopt: the member's own stream is drained, retired and destroyed; the member enqueues on the group's stream from now on
    for (auto* m : ms) BDR_HIP(hipStreamSynchronize(m->stream));
    for (auto* m : ms) {
        hipStream_t old = m->stream;
        m->stream = g->stream; m->group = g.get();
        if (old) { stream_retire(old); (void)hipStreamDestroy(old); }
    }
    g->members = std::move(ms);
    *out = g.release();
    return BDR_OK;
}

template <class G>
int32_t group_destroy(G* g)
{
    if (!g) return BDR_OK;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->stream);
    for (auto* m : g->members) {   // the group owns its members; their stream is the group's, destroyed once below
        m->group = nullptr; m->stream = nullptr;
        (void)bdr_agent_destroy(m);
    }
    delete g;   // retires and destroys the stream, then releases the buffers
    return BDR_OK;
}

template <class G>
int32_t group_size(const G* g, uint32_t* n)
{
    BDR_REQUIRE(g && n, "null argument");
    *n = (uint32_t)g->members.size();
    return BDR_OK;
}

template <class G>
int32_t group_member(const G* g, uint32_t i, bdr_agent** out)
{
    BDR_REQUIRE(g && out, "null argument");
    BDR_REQUIRE(i < g->members.size(), "member %u of a group of %u", i, (unsigned)g->members.size());
    *out = g->members[i];
    return BDR_OK;
}

template <class G>
int32_t group_info(const G* g, bdr_group_info* out)
{
    BDR_REQUIRE(g && out, "null argument");
    memset(out, 0, sizeof *out);
    out->form = G::Kind::FORM;
    out->n_members = (uint32_t)g->members.size();
    out->launches_per_round = (uint32_t)g->n_launches;
    out->kernel_launches = g->kernel_launches;
    return BDR_OK;
}

// the action width of a member, for the group evaluator's check of act_row_bytes (trainer.hip); 0: no such member
template <class G>
int group_act_dim(const void* group, uint32_t member)
{
    const auto* g = static_cast<const G*>(group);
    return g && member < g->members.size() ? g->members[member]->A : 0;
}
// its observation width, for the online loop's check of obs_row_bytes (trainer.hip); 0: no such member
template <class G>
int group_obs_dim(const void* group, uint32_t member)
{
    const auto* g = static_cast<const G*>(group);
    return g && member < g->members.size() ? g->members[member]->O : 0;
}

// the bytes of one action row of a member's ring: A f32 values, unless the kind says otherwise (K::act_row_bytes - the candle DQN: one i64)
template <class K, class M> auto group_act_row_bytes(const M* m, int) -> decltype(K::act_row_bytes(m)) { return K::act_row_bytes(m); }
template <class K, class M> uint64_t group_act_row_bytes(const M* m, long) { return (uint64_t)m->A * 4; }

// the second of two members that name one bdr_replay (P: the P handles are all different)
inline uint32_t group_shared_buffer(bdr_replay* const* buffers, uint32_t P)
{
    std::vector<const bdr_replay*> s(buffers, buffers + P);
    std::sort(s.begin(), s.end());
    const auto dup = std::adjacent_find(s.begin(), s.end());
    if (dup == s.end()) return P;
    for (uint32_t p = 0, seen = 0; p < P; ++p) if (buffers[p] == *dup && seen++ == 1) return p;
    return P;
}

// every refusal of a grouped opt, before anything moves: the checks of the agent's own opt, and what the grouped gather covers
template <class G>
int32_t group_check_buffers(G* g, bdr_replay* const* buffers)
{
    using K = typename G::Kind;
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {
        const auto* m = g->members[p];
        const bdr_replay* r = buffers[p];
        BDR_REQUIRE(r, "member %u: null buffer", p);
        BDR_REQUIRE(!m->prof && !m->grad_comm, "member %u: profiling or a gradient communicator was switched on after the group was created", p);
        BDR_REQUIRE(r->obs_bytes == (uint64_t)m->O * 4 && r->act_bytes == group_act_row_bytes<K>(m, 0), "member %u: replay rows do not match %s obs/act dims (f32 rows)", p, K::NAME);
        BDR_REQUIRE(r->device == g->device, "member %u: its replay buffer lives on another device", p);
        BDR_REQUIRE(!r->per, "member %u: a prioritized buffer cannot be stepped by %s group (the grouped gather covers the uniform ring)", p, K::A);
        BDR_REQUIRE(!r->frame_stack, "member %u: a single-frame store cannot be stepped by %s group", p, K::A);
        BDR_REQUIRE(r->index_rng == BDR_RNG_STDRNG, "member %u: the grouped gather draws the StdRng index stream only", p);
        if (r->size == 0) return fail(BDR_ERR_EMPTY, "member %u: batch() on an empty replay buffer", p);
    }
    if (g->last_buffers.size() == P && memcmp(g->last_buffers.data(), buffers, P * sizeof(bdr_replay*)) == 0) return BDR_OK;
    // workgroups run side by side: one bdr_replay (its batch arrays, its stream position) per member
    const uint32_t second = group_shared_buffer(buffers, P);
    if (second != P)
        return fail(BDR_ERR_INVALID, "member %u: it shares its replay buffer with an earlier member: every member needs a bdr_replay of its own (a view of one ring will do)", second);
    g->last_buffers.clear();
    return BDR_OK;
}

// one update round: per member what the agent's opt / update do on the host, in their order, then the round's launches, the last of
// which publishes its number
template <class G>
int32_t group_round(G* g, bdr_replay* const* buffers)
{
    using K = typename G::Kind;
    const uint32_t P = (uint32_t)g->members.size();
    const uint64_t k = g->launches + 1;
    const auto slot = g->step_ring.next();
    if (slot.wait) {   // the slot's last reader has published (bounded: wait_seq_word)
        bool arrived = false;
        BDR_TRY(wait_seq_word(g->seq.host.get(), (unsigned)slot.wait, g->stream, std::chrono::steady_clock::now(), &arrived));
    }
    typename K::Step* steps = g->steps.host.get() + (size_t)slot.slot * P;
    bool dirty = false;
    typename K::MemberArgs o;
    for (uint32_t p = 0; p < P; ++p) {
        auto* m = g->members[p];
        bdr_replay* r = buffers[p];
        const int bs = (int)m->cfg.batch_size;
        BDR_TRY(m->ensure_batch(bs));
        GatherArgs plan{};
        BDR_TRY(replay_sample_plan(r, bs, g->stream, &plan));   // the host half of replay_sample_on_stream; the rows are k_gather_group's
        const typename K::Step st = K::fill_step(m, bs, plan);
        auto& key = g->keys[p];
        if (!key.valid || key.batch_gen != m->batch_gen || key.hyper_gen != m->hyper_gen || key.r_uid != r->uid || key.r_batch_gen != r->batch_gen) {
            K::member_static(m, bs, r, plan, o);
            BDR_TRY(g->kind.check_static(g->plan, g->n_launches, o, p));
            g->kind.stage(p, P, o);
            key.valid = true; key.batch_gen = m->batch_gen; key.hyper_gen = m->hyper_gen; key.r_uid = r->uid; key.r_batch_gen = r->batch_gen;
            dirty = true;
        }
        steps[p] = st;
    }
    if (dirty) {   // rare (first step, a reallocation, another ring): behind everything the stream still holds
        BDR_HIP(hipStreamSynchronize(g->stream));
        BDR_HIP(g->kind.upload());
    }
    std::atomic_thread_fence(std::memory_order_release);
    // (should a launch fail, k is the number of whatever the group launches next - later than every reader of the slot)
    g->launches = k; g->step_ring.record(k);
    BDR_TRY(g->kind.launch(*g, P, g->steps.dev + (size_t)slot.slot * P, (unsigned)k));
    g->kernel_launches += (uint64_t)g->n_launches;
    return BDR_OK;
}

// what bdr_agent_opt does around opt(), for every member, then the round
template <class G>
int32_t group_opt(G* g, bdr_replay* const* buffers)
{
    BDR_REQUIRE(g && buffers, "null argument");
    BDR_HIP(hipSetDevice(g->device));
    BDR_TRY(group_check_buffers(g, buffers));
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {   // asynchronous: what an earlier synchronising call of the member read back surfaces here
        unsigned w[bdr_agent::ERR_WORDS];
        g->members[p]->err_mirror_read(w);
        BDR_TRY(g->members[p]->err_report(w));
    }
    for (uint32_t p = 0; p < P; ++p) g->members[p]->last_replay_uid = buffers[p]->uid;
    BDR_TRY(group_round(g, buffers));
    g->last_buffers.assign(buffers, buffers + P);
    return BDR_OK;
}

template <class G>
int32_t group_opt_with_scalars(G* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    BDR_REQUIRE(g && buffers && out && n_out, "null argument");
    BDR_REQUIRE(cap_per_member >= G::Kind::MIN_CAP, "%s", G::Kind::CAP_MSG);
    BDR_TRY(group_opt(g, buffers));
    BDR_HIP(hipStreamSynchronize(g->stream));   // the one synchronisation: every record() below finds the stream idle
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {
        auto* m = g->members[p];
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

// Policy::sample of the selected members (members == nullptr: all of them) on n host rows each, ONE launch (group_act.hpp)
template <class G>
int32_t group_sample(G* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows, const int32_t* dtypes, typename G::Kind::Act::Out* const* act_out)
{
    BDR_REQUIRE(g && rows && dtypes && act_out, "null argument");
    return group_act_sample(g, typename G::Kind::Act{}, nullptr, (uint32_t)g->members.size(), norms, n, rows, dtypes, act_out);
}
template <class G>
int32_t group_sample_members(G* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows,
                             const int32_t* dtypes, typename G::Kind::Act::Out* const* act_out)
{
    BDR_REQUIRE(g && members && rows && dtypes && act_out, "null argument");
    return group_act_sample(g, typename G::Kind::Act{}, members, n_sel, norms, n, rows, dtypes, act_out);
}

// ---- the grouped push (group_push.hpp has the kernel and the slot's layout) -----------------------------------------------------------
// the staged record of one transition of a ring, F32 or F64 observation rows
struct GroupPushLayout { uint32_t s_next_off, s_act_off, s_tail_off, rec_bytes; };
inline GroupPushLayout group_push_layout(const bdr_replay* r, bool f64)
{
    GroupPushLayout l{};
    if (!f64) {   // the ring's own record
        l.s_next_off = (uint32_t)r->next_off; l.s_act_off = (uint32_t)r->act_off; l.s_tail_off = (uint32_t)r->tail_off;
    } else {      // two raw float64 rows, then act and the tail at the ring's offsets modulo 16
        l.s_next_off = (uint32_t)round_up(2 * r->obs_bytes, 16);
        l.s_act_off = 2 * l.s_next_off + (uint32_t)(r->act_off & 15);
        l.s_tail_off = l.s_act_off + (uint32_t)(r->tail_off - r->act_off);
    }
    l.rec_bytes = (uint32_t)round_up((uint64_t)l.s_tail_off + 8, 16);
    return l;
}

// every refusal of a grouped push, before anything moves; *need: the bytes of the slot the call fills
template <class G>
int32_t group_check_push(G* g, bdr_replay* const* buffers, uint64_t n, const void* const* obs, const void* const* next_obs, const int32_t* dtypes,
                         const float* const* act, const float* const* reward, const int8_t* const* term, const int8_t* const* trunc, uint64_t* need)
{
    using K = typename G::Kind;
    const uint32_t P = (uint32_t)g->members.size();
    BDR_REQUIRE(n >= 1, "a grouped push takes at least one row per member (n = 0)");
    uint64_t bytes = (uint64_t)P * sizeof(CGroupPushDesc);
    for (uint32_t p = 0; p < P; ++p) {
        const auto* m = g->members[p];
        const bdr_replay* r = buffers[p];
        BDR_REQUIRE(r, "member %u: null buffer", p);
        BDR_REQUIRE(obs[p] && next_obs[p], "member %u: null observation rows", p);
        BDR_REQUIRE(act[p] && reward[p] && term[p] && trunc[p], "member %u: null act, reward or flag rows", p);
        const int32_t dt = dtypes ? dtypes[p] : BDR_DTYPE_F32;
        BDR_REQUIRE(dt == BDR_DTYPE_F32 || dt == BDR_DTYPE_F64, "member %u: dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64", p);
        BDR_REQUIRE(r->device == g->device, "member %u: its replay buffer lives on another device", p);
        BDR_REQUIRE(!r->view_of, "member %u: a grouped push on a view: a view is read-only (it borrows its owner's rows)", p);
        BDR_REQUIRE(r->n_views == 0, "member %u: a grouped push on a ring with %u live view(s): its rows stay as they are until the views are destroyed", p, r->n_views);
        BDR_REQUIRE(!r->per, "member %u: a prioritized buffer cannot take the push of %s group (its sum tree is updated by bdr_replay_push)", p, K::A);
        BDR_REQUIRE(!r->frame_stack, "member %u: a single-frame store cannot take the push of %s group", p, K::A);
        BDR_REQUIRE(r->index_rng == BDR_RNG_STDRNG, "member %u: %s group steps rings on the StdRng index stream only", p, K::A);
        BDR_REQUIRE(r->obs_bytes == (uint64_t)m->O * 4 && r->act_bytes == group_act_row_bytes<K>(m, 0), "member %u: replay rows do not match %s obs/act dims (f32 rows)", p, K::NAME);
        bytes += n * (uint64_t)group_push_layout(r, dt == BDR_DTYPE_F64).rec_bytes;
        BDR_REQUIRE(bytes <= (uint64_t)G::PUSH_SLOT_BYTES,
                    "member %u: %llu rows per member do not fit one staging slot of %d bytes (descriptors and records of all members): split the call", p,
                    (unsigned long long)n, (int)G::PUSH_SLOT_BYTES);
    }
    *need = bytes;
    if (g->last_push_buffers.size() == P && memcmp(g->last_push_buffers.data(), buffers, P * sizeof(bdr_replay*)) == 0) return BDR_OK;
    const uint32_t second = group_shared_buffer(buffers, P);   // waves run side by side, and every ring's head moves once
    BDR_REQUIRE(second == P, "member %u: it shares its replay buffer with an earlier member: every member pushes into a ring of its own", second);
    g->last_push_buffers.clear();
    return BDR_OK;
}

// the largest n a grouped push of these rings and dtypes takes (0: not even one row fits)
template <class G>
int32_t group_push_max_rows(G* g, bdr_replay* const* buffers, const int32_t* dtypes, uint64_t* n_max)
{
    BDR_REQUIRE(g && buffers && n_max, "null argument");
    const uint32_t P = (uint32_t)g->members.size();
    uint64_t per_row = 0;
    for (uint32_t p = 0; p < P; ++p) {
        BDR_REQUIRE(buffers[p], "member %u: null buffer", p);
        const int32_t dt = dtypes ? dtypes[p] : BDR_DTYPE_F32;
        BDR_REQUIRE(dt == BDR_DTYPE_F32 || dt == BDR_DTYPE_F64, "member %u: dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64", p);
        per_row += group_push_layout(buffers[p], dt == BDR_DTYPE_F64).rec_bytes;
    }
    const uint64_t head = (uint64_t)P * sizeof(CGroupPushDesc);
    *n_max = head >= (uint64_t)G::PUSH_SLOT_BYTES ? 0 : ((uint64_t)G::PUSH_SLOT_BYTES - head) / per_row;
    return BDR_OK;
}

// ExperienceBufferBase::push of n transitions per member, ONE launch; does not synchronise
template <class G>
int32_t group_push(G* g, bdr_replay* const* buffers, uint64_t n, const void* const* obs, const void* const* next_obs, const int32_t* dtypes,
                   const float* const* act, const float* const* reward, const int8_t* const* term, const int8_t* const* trunc)
{
    BDR_REQUIRE(g && buffers && obs && next_obs && act && reward && term && trunc, "null argument");
    uint64_t need = 0;
    BDR_TRY(group_check_push(g, buffers, n, obs, next_obs, dtypes, act, reward, term, trunc, &need));
    BDR_HIP(hipSetDevice(g->device));
    const uint32_t P = (uint32_t)g->members.size();
    if (!g->push.host) BDR_HIP(pinned_array(g->push, (size_t)G::PUSH_SLOTS * G::PUSH_SLOT_BYTES));   // the first push
    const auto slot = g->push_ring.next();
    if (slot.wait) {   // the slot's last reader has published (bounded: wait_seq_word)
        bool arrived = false;
        BDR_TRY(wait_seq_word(g->seq.host.get(), (unsigned)slot.wait, g->stream, std::chrono::steady_clock::now(), &arrived));
    }
    // order the group's stream behind each ring's last reader and writer: nothing to do when both were this stream
    for (uint32_t p = 0; p < P; ++p) BDR_TRY(replay_begin_write_on_stream(buffers[p], g->stream));
    const size_t slot_off = (size_t)slot.slot * G::PUSH_SLOT_BYTES;
    uint8_t* base = g->push.host.get() + slot_off;
    CGroupPushDesc* desc = reinterpret_cast<CGroupPushDesc*>(base);
    size_t off = (size_t)P * sizeof(CGroupPushDesc);
    for (uint32_t p = 0; p < P; ++p) {
        const bdr_replay* r = buffers[p];
        const bool f64 = dtypes && dtypes[p] == BDR_DTYPE_F64;
        const GroupPushLayout l = group_push_layout(r, f64);
        const size_t row = (size_t)r->obs_bytes * (f64 ? 2 : 1);
        const uint8_t* o = (const uint8_t*)obs[p]; const uint8_t* x = (const uint8_t*)next_obs[p]; const uint8_t* a = (const uint8_t*)act[p];
        for (uint64_t j = 0; j < n; ++j) {
            uint8_t* rec = base + off + (size_t)j * l.rec_bytes;
            memcpy(rec, o + j * row, row);
            memcpy(rec + l.s_next_off, x + j * row, row);
            memcpy(rec + l.s_act_off, a + j * r->act_bytes, r->act_bytes);
            memcpy(rec + l.s_tail_off, &reward[p][j], 4);
            rec[l.s_tail_off + 4] = (uint8_t)term[p][j];
            rec[l.s_tail_off + 5] = (uint8_t)trunc[p][j];
        }
        CGroupPushDesc d{};
        d.ring = r->ring; d.head = r->i; d.capacity = r->capacity; d.stride = r->stride;
        d.src_off = (uint32_t)off; d.rec_bytes = l.rec_bytes;
        d.obs_bytes = (uint32_t)r->obs_bytes; d.act_bytes = (uint32_t)r->act_bytes;
        d.next_off = (uint32_t)r->next_off; d.act_off = (uint32_t)r->act_off; d.tail_off = (uint32_t)r->tail_off;
        d.s_next_off = l.s_next_off; d.s_act_off = l.s_act_off; d.s_tail_off = l.s_tail_off; d.f64 = f64 ? 1u : 0u;
        desc[p] = d;
        off += (size_t)n * l.rec_bytes;
    }
    std::atomic_thread_fence(std::memory_order_release);
    // (should the launch fail, k is the number of whatever the group launches next - later than every reader of the slot)
    const uint64_t k = g->launches + 1;
    g->launches = k; g->push_ring.record(k);
    const unsigned waves = P * (unsigned)n;
    hipLaunchKernelGGL(k_cgroup_push, dim3((waves + 3) / 4), dim3(256), 0, g->stream, (const uint8_t*)(g->push.dev + slot_off), (unsigned)P, (unsigned)n,
                       g->ticket.get(), g->seq.dev, (unsigned)k);
    BDR_HIP(hipGetLastError());
    g->kernel_launches += 1;
    for (uint32_t p = 0; p < P; ++p) replay_end_write_on_stream(buffers[p], g->stream, n);
    g->last_push_buffers.assign(buffers, buffers + P);
    return BDR_OK;
}

template <class G>
int32_t group_sync(G* g)
{
    BDR_REQUIRE(g, "null group");
    BDR_HIP(hipSetDevice(g->device));
    BDR_HIP(hipStreamSynchronize(g->stream));
    for (auto* m : g->members) {
        BDR_TRY(m->after_sync());
        BDR_TRY(m->err_check());
    }
    return BDR_OK;
}

}  // namespace
