// Host-side driver of the opt-step loops: the reference's Trainer is compiled Rust, so its counterpart
// above the C ABI is compiled C++ (the Python mirror in border_amd/trainer.py binds the same rules for tests and bench.py).
//   Trainer::train_step      border-core/src/trainer.rs:197-228   warm-up rule, opt_interval, opt vs opt_with_record, timer
//   Trainer::train           trainer.rs:267-327                   sample_and_push, train_step, cost record, stop at max_opts
//   Trainer::train_offline   trainer.rs:330-384                   warmup_period = 0, opt_interval = 1
//   Sampler::sample_and_push trainer/sampler.rs:99-144            reset on first use, Policy::sample, step_with_reset, push
//   SimpleStepProcessor      generic_replay_buffer/step_proc.rs:62-137   (prev_obs, act, obs, ...) transitions
//   Trainer::post_process   trainer.rs:231-264                   evaluate every eval_interval opt steps, keep the best model, save
//   DefaultEvaluator        evaluator/default_evaluator.rs:64-88  (MinariEvaluator, border-minari/src/evaluator.rs:25-62, is the same loop)
// Recorders are out of scope: an observer callback receives what the reference would store.  Pure host code: the agent, buffer and environment are reached through function tables, so the loop itself runs
// (and is tested) without a GPU.
#include <sys/stat.h>

#include <cerrno>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "agent_base.hpp"
#include "common.hpp"

using namespace bdr;

namespace bdr {
int bc_group_act_dim(const void* group, uint32_t member);    // bc.hip (bc_group.hpp), iql.hip (iql_group.hpp): group_core.hpp's group_act_dim of the kind
int iql_group_act_dim(const void* group, uint32_t member);
int awac_group_act_dim(const void* group, uint32_t member);   // awac.hip (awac_group.hpp)
int candle_sac_group_act_dim(const void* group, uint32_t member);   // candle_sac.hip (candle_sac_group.hpp)
int awac_group_obs_dim(const void* group, uint32_t member);
int candle_sac_group_obs_dim(const void* group, uint32_t member);
}

namespace {
using Clock = std::chrono::steady_clock;

struct State {
    const bdr_trainer_config* c;
    const bdr_trainer_ops* ops;
    uint64_t env_steps = 0, opt_steps = 0, opt_steps_counter = 0, samples_counter = 0, n_records = 0, n_episodes = 0;
    double timer_for_opt_steps = 0, timer_for_samples = 0, total_opt = 0, total_sample = 0;
    float scalars[128];
    int32_t n_scalars = 0;
    float max_eval_reward = -FLT_MAX;   // f32::MIN (trainer.rs: max_eval_reward)
};

// trainer.rs:197-228
int32_t train_step(State& s, bool* is_opt, bool* with_record)
{
    const bdr_trainer_config& c = *s.c;
    *is_opt = false; *with_record = false; s.n_scalars = 0;
    if (s.env_steps < c.warmup_period) return BDR_OK;
    if (s.env_steps % c.opt_interval != 0) return BDR_OK;
    const auto t0 = Clock::now();
    if (c.record_agent_info_interval != 0 && (s.opt_steps + 1) % c.record_agent_info_interval == 0) {
        BDR_TRY(s.ops->agent_opt_with_record(s.ops->agent, s.ops->buffer, s.scalars, 128, &s.n_scalars));
        *with_record = true;
        s.n_records += 1;
    } else {
        BDR_TRY(s.ops->agent_opt(s.ops->agent, s.ops->buffer));
    }
    s.opt_steps += 1;
    const double dt = std::chrono::duration<double>(Clock::now() - t0).count();
    s.timer_for_opt_steps += dt; s.total_opt += dt;
    s.opt_steps_counter += 1;
    *is_opt = true;
    return BDR_OK;
}

// trainer.rs:164-181: average_time() / reset_counters() at every record_compute_cost_interval-th opt step
void cost_record(State& s, bdr_trainer_observer obs, void* ctx)
{
    const bdr_trainer_config& c = *s.c;
    if (c.record_compute_cost_interval == 0 || s.opt_steps % c.record_compute_cost_interval != 0) return;
    // `timer.as_millis() as f32 / n as f32`: the accumulated time is truncated to whole milliseconds first (trainer.rs:164-174)
    const float avr[2] = {s.opt_steps_counter ? (float)std::floor(1000.0 * s.timer_for_opt_steps) / (float)s.opt_steps_counter : -1.0f,
                          s.samples_counter ? (float)std::floor(1000.0 * s.timer_for_samples) / (float)s.samples_counter : -1.0f};
    if (obs) obs(ctx, s.env_steps, s.opt_steps, BDR_TRAINER_EVENT_COST, avr, 2);
    s.timer_for_opt_steps = 0; s.opt_steps_counter = 0; s.timer_for_samples = 0; s.samples_counter = 0;
}

void fill_stats(const State& s, bdr_trainer_stats* out)
{
    if (!out) return;
    out->env_steps = s.env_steps; out->opt_steps = s.opt_steps; out->n_records = s.n_records; out->n_episodes = s.n_episodes;
    out->opt_seconds = s.total_opt; out->sample_seconds = s.total_sample;
}

int32_t check(const bdr_trainer_config* c, const bdr_trainer_ops* ops)
{
    BDR_REQUIRE(c && ops, "null argument");
    BDR_REQUIRE(c->max_opts >= 1, "max_opts must be >= 1");
    BDR_REQUIRE(c->opt_interval >= 1, "opt_interval must be >= 1");
    BDR_REQUIRE(ops->agent_set_train && ops->agent_opt && ops->agent_opt_with_record, "agent function table is incomplete");
    return BDR_OK;
}

// defaults: the library's own handles
int32_t d_set_train(void* a, int32_t on) { return bdr_agent_set_train((bdr_agent*)a, on); }
int32_t d_opt(void* a, void* b) { return bdr_agent_opt((bdr_agent*)a, (bdr_replay*)b); }
int32_t d_opt_rec(void* a, void* b, float* out, int32_t cap, int32_t* n) { return bdr_agent_opt_with_scalars((bdr_agent*)a, (bdr_replay*)b, out, cap, n); }
int32_t d_push(void* b, uint64_t n, const void* obs, const void* act, const void* next_obs, const float* rew, const int8_t* term, const int8_t* trunc)
{
    return bdr_replay_push((bdr_replay*)b, n, obs, act, next_obs, rew, term, trunc);
}
// bdr_replay_push for device-resident observations (bdr_env_vtable::obs_on_device); the single-frame store has its own device push
int32_t d_push_dev(void* b, uint64_t n, const void* obs_dev, uint64_t os, const void* act, const void* next_dev, uint64_t ns, const float* rew,
                   const int8_t* term, const int8_t* trunc)
{
    if (((bdr_replay*)b)->frame_stack) return bdr_replay_push_device_frames((bdr_replay*)b, n, obs_dev, os, act, next_dev, ns, rew, term, trunc);
    return bdr_replay_push_device((bdr_replay*)b, n, obs_dev, os, act, next_dev, ns, rew, term, trunc);
}
// defaults of the evaluator and the post-processing
int32_t d_sample_raw(void* a, const bdr_obs_norm* norm, uint64_t n, const void* rows, int32_t dtype, int32_t on_device, uint64_t row_stride, void* act)
{
    // one buffer for both result kinds: a Discrete BC agent writes i64 indices, every other agent f32 rows
    return bdr_agent_sample_raw((bdr_agent*)a, norm, n, rows, dtype, on_device, row_stride, (float*)act, (int64_t*)act);
}
int32_t mkdir_p(const std::string& dir)
{
    for (size_t i = 1; i <= dir.size(); ++i) {
        if (i != dir.size() && dir[i] != '/') continue;
        const std::string part = dir.substr(0, i);
        if (mkdir(part.c_str(), 0777) != 0 && errno != EEXIST) return fail(BDR_ERR_IO, "cannot create directory %s: %s", part.c_str(), strerror(errno));
    }
    return BDR_OK;
}
int32_t d_save(void* a, const char* dir)
{
    BDR_TRY(mkdir_p(dir));
    return bdr_agent_save_params((bdr_agent*)a, dir);
}

int32_t check_post(const bdr_trainer_post* post)
{
    if (!post) return BDR_OK;
    BDR_REQUIRE(!post->eval_interval || post->evaluator, "eval_interval is set: post-processing needs an evaluator");
    BDR_REQUIRE(!(post->eval_interval || post->save_interval) || post->model_dir, "post-processing saves models: model_dir must be set");
    return BDR_OK;
}

// trainer.rs:231-264, after an iteration that took an opt step
int32_t post_process(State& s, const bdr_trainer_post* post, bdr_trainer_observer obs, void* ctx)
{
    if (!post) return BDR_OK;
    const auto save = post->save_params ? post->save_params : d_save;
    if (post->eval_interval && s.opt_steps % post->eval_interval == 0) {
        BDR_TRY(s.ops->agent_set_train(s.ops->agent, 0));
        bdr_eval_result r{};
        BDR_TRY(bdr_evaluate(post->evaluator, s.ops->agent, &r));
        BDR_TRY(s.ops->agent_set_train(s.ops->agent, 1));
        const float sc[2] = {r.score, r.normalized};
        if (obs) obs(ctx, s.env_steps, s.opt_steps, BDR_TRAINER_EVENT_EVAL, sc, r.has_normalized ? 2 : 1);
        if (r.score > s.max_eval_reward) {
            s.max_eval_reward = r.score;
            BDR_TRY(save(s.ops->agent, (std::string(post->model_dir) + "/best").c_str()));
        }
    }
    if (post->save_interval > 0 && s.opt_steps % post->save_interval == 0)
        BDR_TRY(save(s.ops->agent, (std::string(post->model_dir) + "/" + std::to_string(s.opt_steps)).c_str()));
    return BDR_OK;
}

// what follows the sampling of an iteration in both loops: train_step, its event, post_process, the cost record; *stop: max_opts reached
int32_t step_and_records(State& s, const bdr_trainer_post* post, bdr_trainer_observer obs, void* obs_ctx, bool* stop)
{
    bool is_opt = false, with_record = false;
    BDR_TRY(train_step(s, &is_opt, &with_record));
    if (obs) obs(obs_ctx, s.env_steps, s.opt_steps, is_opt ? (with_record ? BDR_TRAINER_EVENT_OPT_RECORD : BDR_TRAINER_EVENT_OPT) : BDR_TRAINER_EVENT_SKIP,
                 s.scalars, s.n_scalars);
    if (is_opt) BDR_TRY(post_process(s, post, obs, obs_ctx));
    cost_record(s, obs, obs_ctx);
    *stop = s.opt_steps == s.c->max_opts;   // trainer.rs:323-325
    return BDR_OK;
}

// ---- the group loop: bdr_trainer_ops over a group, so that State / train_step / cost_record serve it unchanged ---------------------
// `agent` is this adapter: opt is one group opt, opt_with_record one group opt_with_record whose Records stay here per member
// (the entries both group tables have - bdr_group_trainer_ops: i64 actions, bdr_cgroup_trainer_ops: f32 action rows - by value)
struct GroupAdapter {
    void* group; void* const* buffers;
    int32_t (*set_train)(void*, int32_t);
    int32_t (*opt)(void*, void* const*);
    int32_t (*opt_with_record)(void*, void* const*, float*, int32_t, int32_t*);
    std::vector<float> scalars;      // [n_members][128]
    std::vector<int32_t> n_scalars;  // [n_members]
    template <class Ops>
    GroupAdapter(const Ops* o, uint32_t P)
        : group(o->group), buffers(o->buffers), set_train(o->set_train), opt(o->opt), opt_with_record(o->opt_with_record), scalars((size_t)P * 128), n_scalars(P, 0) {}
};
int32_t ga_set_train(void* a, int32_t on) { const auto* ga = (GroupAdapter*)a; return ga->set_train(ga->group, on); }
int32_t ga_opt(void* a, void*) { const auto* ga = (GroupAdapter*)a; return ga->opt(ga->group, ga->buffers); }
int32_t ga_opt_rec(void* a, void*, float* out, int32_t cap, int32_t* n)
{
    auto* ga = (GroupAdapter*)a;
    BDR_TRY(ga->opt_with_record(ga->group, ga->buffers, ga->scalars.data(), 128, ga->n_scalars.data()));
    *n = std::min(ga->n_scalars[0], cap);   // (State::scalars mirrors member 0's; the loop hands every member its own)
    memcpy(out, ga->scalars.data(), (size_t)*n * sizeof(float));
    return BDR_OK;
}
// defaults: the library's own group
int32_t dg_set_train(void* g, int32_t on)
{
    uint32_t n = 0;
    BDR_TRY(bdr_agent_group_size((bdr_agent_group*)g, &n));
    for (uint32_t i = 0; i < n; ++i) {
        bdr_agent* m = nullptr;
        BDR_TRY(bdr_agent_group_member((bdr_agent_group*)g, i, &m));
        BDR_TRY(bdr_agent_set_train(m, on));
    }
    return BDR_OK;
}
int32_t dg_sample(void* g, const void* const* obs, int64_t* act) { return bdr_agent_group_sample((bdr_agent_group*)g, obs, act, nullptr); }
int32_t dg_push(void* g, void* const* b, const void* const* obs, const int64_t* act, const void* const* next_obs, const float* rew, const int8_t* term,
                const int8_t* trunc)
{
    return bdr_agent_group_push((bdr_agent_group*)g, (bdr_replay* const*)b, obs, act, next_obs, rew, term, trunc);
}
int32_t dg_opt(void* g, void* const* b) { return bdr_agent_group_opt((bdr_agent_group*)g, (bdr_replay* const*)b); }
int32_t dg_opt_rec(void* g, void* const* b, float* out, int32_t cap, int32_t* n)
{
    return bdr_agent_group_opt_with_scalars((bdr_agent_group*)g, (bdr_replay* const*)b, out, cap, n);
}
int32_t dg_sample_members(void* g, const uint32_t* members, uint32_t n, const void* const* obs, int64_t* act)
{
    return bdr_agent_group_sample_members((bdr_agent_group*)g, members, n, obs, act, nullptr);
}
int32_t dg_save_member(void* g, uint32_t member, const char* dir)
{
    bdr_agent* m = nullptr;
    BDR_TRY(bdr_agent_group_member((bdr_agent_group*)g, member, &m));
    return d_save(m, dir);
}

// every refusal of bdr_evaluate_group, naming the member: the group acts on host f32 rows and writes one i64 action
int32_t check_group_eval(const bdr_evaluator* evs, const bdr_group_eval_ops* ops)
{
    BDR_REQUIRE(evs && ops, "null argument");
    BDR_REQUIRE(ops->sample_members, "the group evaluation function table is incomplete");
    BDR_REQUIRE(ops->n_members >= 1, "the group evaluation function table names no members");
    for (uint32_t p = 0; p < ops->n_members; ++p) {
        const bdr_evaluator& ev = evs[p];
        BDR_REQUIRE(ev.env.reset_with_index && ev.env.step, "member %u: the evaluator's environment function table is incomplete", p);
        BDR_REQUIRE(ev.n_episodes >= 1, "member %u: n_episodes must be >= 1", p);
        BDR_REQUIRE(ev.obs_row_bytes > 0, "member %u: obs_row_bytes must be set", p);
        BDR_REQUIRE(ev.act_row_bytes == 8, "member %u: a group acts with one i64 action per member: act_row_bytes must be 8", p);
        BDR_REQUIRE(ev.obs_dtype == BDR_DTYPE_F32, "member %u: a group acts on float32 rows (obs_dtype must be BDR_DTYPE_F32)", p);
        BDR_REQUIRE(!ev.norm, "member %u: a group acts on the rows as they are (norm must be NULL)", p);
        BDR_REQUIRE(!ev.env.obs_on_device, "member %u: a group acts on host rows (obs_on_device environments are not supported)", p);
    }
    return BDR_OK;
}

// a BC, an IQL or an AWAC group's entries behind the function tables (bdr_*_group_trainer_ops_default, bdr_*_group_eval_ops_default), over the kind's
// C functions
template <class G, auto Size, auto Member, auto Opt, auto OptRec, auto Sample>
struct GroupEntries {
    static int32_t set_train(void* g, int32_t on)
    {
        uint32_t n = 0;
        BDR_TRY(Size((G*)g, &n));
        for (uint32_t i = 0; i < n; ++i) {
            bdr_agent* m = nullptr;
            BDR_TRY(Member((G*)g, i, &m));
            BDR_TRY(bdr_agent_set_train(m, on));
        }
        return BDR_OK;
    }
    static int32_t opt(void* g, void* const* b) { return Opt((G*)g, (bdr_replay* const*)b); }
    static int32_t opt_rec(void* g, void* const* b, float* out, int32_t cap, int32_t* n) { return OptRec((G*)g, (bdr_replay* const*)b, out, cap, n); }
    static int32_t sample_members(void* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, const void* const* rows, const int32_t* dtypes,
                                  float* const* act_out)
    {
        return Sample((G*)g, members, n_sel, norms, 1, rows, dtypes, act_out);
    }
    static int32_t save_member(void* g, uint32_t member, const char* dir)
    {
        bdr_agent* m = nullptr;
        BDR_TRY(Member((G*)g, member, &m));
        return d_save(m, dir);
    }
    // the default tables of the kind
    static void eval_ops(bdr_bc_group_eval_ops* ops, G* group)
    {
        if (!ops) return;
        memset(ops, 0, sizeof *ops);
        ops->group = group;
        if (group) (void)Size(group, &ops->n_members);
        ops->sample_members = sample_members;
    }
    static void trainer_ops(bdr_group_trainer_ops* ops, G* group, bdr_replay* const* buffers)
    {
        if (!ops) return;
        memset(ops, 0, sizeof *ops);
        ops->group = group; ops->buffers = (void* const*)buffers;
        if (group) (void)Size(group, &ops->n_members);
        ops->set_train = set_train; ops->opt = opt; ops->opt_with_record = opt_rec;
    }
    static void trainer_post(bdr_bc_group_trainer_post* post, G* group)
    {
        if (!post) return;
        memset(post, 0, sizeof *post);
        eval_ops(&post->eval_ops, group);
        post->save_member = save_member;
    }
};
using BcGroupEntries = GroupEntries<bdr_bc_group, bdr_bc_group_size, bdr_bc_group_member, bdr_bc_group_opt, bdr_bc_group_opt_with_scalars, bdr_bc_group_sample_members>;
using IqlGroupEntries =
    GroupEntries<bdr_iql_group, bdr_iql_group_size, bdr_iql_group_member, bdr_iql_group_opt, bdr_iql_group_opt_with_scalars, bdr_iql_group_sample_members>;
using AwacGroupEntries =
    GroupEntries<bdr_awac_group, bdr_awac_group_size, bdr_awac_group_member, bdr_awac_group_opt, bdr_awac_group_opt_with_scalars, bdr_awac_group_sample_members>;
using CandleSacGroupEntries = GroupEntries<bdr_candle_sac_group, bdr_candle_sac_group_size, bdr_candle_sac_group_member, bdr_candle_sac_group_opt,
                                           bdr_candle_sac_group_opt_with_scalars, bdr_candle_sac_group_sample_members>;
// the kinds a default evaluation table can name: its acting entry, the action width of a member, the kind in messages, its save
struct GroupKindRow {
    decltype(bdr_bc_group_eval_ops::sample_members) sample_members;
    int (*act_dim)(const void*, uint32_t);
    const char* a;
    int32_t (*save_member)(void*, uint32_t, const char*);
};
const GroupKindRow* group_kind_of(const bdr_bc_group_eval_ops* ops)
{
    static const GroupKindRow kinds[] = {{BcGroupEntries::sample_members, bc_group_act_dim, "a BC", BcGroupEntries::save_member},
                                         {IqlGroupEntries::sample_members, iql_group_act_dim, "an IQL", IqlGroupEntries::save_member},
                                         {AwacGroupEntries::sample_members, awac_group_act_dim, "an AWAC", AwacGroupEntries::save_member},
                                         {CandleSacGroupEntries::sample_members, candle_sac_group_act_dim, "a candle SAC", CandleSacGroupEntries::save_member}};
    for (const GroupKindRow& k : kinds) if (ops && ops->sample_members == k.sample_members) return &k;
    return nullptr;
}

// every refusal of bdr_evaluate_bc_group (a BC or an IQL group behind the table), naming the member: the group acts on host rows, f32 or float64, and writes one f32 action row
int32_t check_bc_group_eval(const bdr_evaluator* evs, const bdr_bc_group_eval_ops* ops)
{
    BDR_REQUIRE(evs && ops, "null argument");
    BDR_REQUIRE(ops->sample_members, "the group evaluation function table is incomplete");
    BDR_REQUIRE(ops->n_members >= 1, "the group evaluation function table names no members");
    for (uint32_t p = 0; p < ops->n_members; ++p) {
        const bdr_evaluator& ev = evs[p];
        BDR_REQUIRE(ev.env.reset_with_index && ev.env.step, "member %u: the evaluator's environment function table is incomplete", p);
        BDR_REQUIRE(ev.n_episodes >= 1, "member %u: n_episodes must be >= 1", p);
        BDR_REQUIRE(ev.obs_row_bytes > 0, "member %u: obs_row_bytes must be set", p);
        if (const GroupKindRow* k = group_kind_of(ops)) {
            const int A = k->act_dim(ops->group, p);
            BDR_REQUIRE(A > 0, "member %u: the group has no such member", p);
            BDR_REQUIRE(ev.act_row_bytes == (uint64_t)A * 4, "member %u: %s group acts with one f32 action row per member: act_row_bytes must be 4 * act_dim = %d", p, k->a, A * 4);
        } else {
            BDR_REQUIRE(ev.act_row_bytes > 0 && ev.act_row_bytes % 4 == 0, "member %u: a BC group acts with f32 action rows: act_row_bytes must be a positive multiple of 4", p);
        }
        BDR_REQUIRE(ev.obs_dtype == BDR_DTYPE_F32 || ev.obs_dtype == BDR_DTYPE_F64, "member %u: obs_dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64", p);
        BDR_REQUIRE(!ev.env.obs_on_device, "member %u: a group acts on host rows (obs_on_device environments are not supported)", p);
    }
    return BDR_OK;
}

// default_evaluator.rs:64-88 for every member in lockstep, the one loop of bdr_evaluate_group and bdr_evaluate_bc_group: member p sees
// exactly the calls bdr_evaluate(&evs[p], member p) makes.  act(sel, n_sel, rows, act_rows): ONE acting call over the members with an
// open episode; rows[p] is member p's observation row and act_rows[p] its action row of evs[p].act_row_bytes (16-byte aligned, the
// rows of all members contiguous in member order when they have one size).
template <class Act>
int32_t evaluate_lockstep(const bdr_evaluator* evs, uint32_t P, Act&& act, bdr_eval_result* out)
{
    std::vector<std::vector<uint8_t>> prev(P), next(P);
    for (uint32_t p = 0; p < P; ++p) { prev[p].resize(evs[p].obs_row_bytes); next[p].resize(evs[p].obs_row_bytes); }
    std::vector<const void*> rows(P);
    size_t act_bytes = 0;
    for (uint32_t p = 0; p < P; ++p) act_bytes += evs[p].act_row_bytes;
    std::vector<uint64_t> act_store((act_bytes + 7) / 8 + 1);   // (u64 words: aligned for i64 and f32 rows alike)
    std::vector<uint8_t*> act_rows(P);
    for (uint32_t p = 0, off = 0; p < P; off += (uint32_t)evs[p].act_row_bytes, ++p) act_rows[p] = reinterpret_cast<uint8_t*>(act_store.data()) + off;
    std::vector<float> r_total(P, 0.f), reward(P);
    std::vector<int8_t> term(P), trunc(P), open(P, 0);
    std::vector<uint64_t> ix(P, 0), n_steps(P, 0);
    std::vector<uint32_t> sel;
    sel.reserve(P);
    for (;;) {
        sel.clear();
        for (uint32_t p = 0; p < P; ++p) {   // a member with episodes left and none open starts its next one
            if (!open[p] && ix[p] < evs[p].n_episodes) {
                BDR_TRY(evs[p].env.reset_with_index(evs[p].env.ctx, ix[p], prev[p].data()));
                open[p] = 1;
            }
            if (open[p]) sel.push_back(p);
            rows[p] = prev[p].data();
        }
        if (sel.empty()) break;   // ix == n_episodes for everybody
        BDR_TRY(act(sel.data(), (uint32_t)sel.size(), rows.data(), act_rows.data()));
        for (const uint32_t p : sel) {
            reward[p] = 0; term[p] = 0; trunc[p] = 0;
            BDR_TRY(evs[p].env.step(evs[p].env.ctx, act_rows[p], next[p].data(), &reward[p], &term[p], &trunc[p]));
        }
        for (const uint32_t p : sel) {
            r_total[p] += reward[p];
            n_steps[p] += 1;
            if (term[p] == 1 || trunc[p] == 1) { open[p] = 0; ix[p] += 1; }   // step.rs:136-138
            else prev[p].swap(next[p]);                                      // prev_obs = step.obs
        }
    }
    for (uint32_t p = 0; p < P; ++p) {
        const bdr_evaluator& ev = evs[p];
        out[p].score = r_total[p] / (float)ev.n_episodes;
        out[p].has_normalized = ev.has_ref_scores ? 1 : 0;
        out[p].normalized = ev.has_ref_scores ? (out[p].score - ev.ref_min_score) / (ev.ref_max_score - ev.ref_min_score) : 0.f;   // border-minari/src/env.rs:162-168
        out[p].n_steps = n_steps[p]; out[p].n_episodes = ev.n_episodes;
    }
    return BDR_OK;
}

// (Post: bdr_group_trainer_post or bdr_bc_group_trainer_post; check_eval: check_group_eval or check_bc_group_eval)
template <class Post, class CheckEval>
int32_t check_group_post(const Post* post, uint32_t P, CheckEval&& check_eval)
{
    if (!post) return BDR_OK;
    BDR_REQUIRE(!post->eval_interval || post->evaluators, "eval_interval is set: post-processing needs one evaluator per member");
    BDR_REQUIRE(!(post->eval_interval || post->save_interval) || post->model_dirs, "post-processing saves models: model_dirs must be set");
    if (post->eval_interval || post->save_interval)
        for (uint32_t p = 0; p < P; ++p) BDR_REQUIRE(post->model_dirs[p], "member %u: null model directory", p);
    if (post->eval_interval) {
        BDR_REQUIRE(post->eval_ops.n_members == P, "the evaluation function table names %u members, the loop %u", post->eval_ops.n_members, P);
        BDR_TRY(check_eval(post->evaluators, &post->eval_ops));
    }
    return BDR_OK;
}

typedef void (*GroupObserver)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps, int32_t event, const float* scalars, int32_t n_scalars);

// trainer.rs:231-264 for every member, after an iteration that took an opt step; max_eval_reward[p] is member p's own.
// evaluate: bdr_evaluate_group or bdr_evaluate_bc_group; save_default: the group kind's own save of a member
template <class Ops, class Post, class Evaluate>
int32_t group_post_process(State& s, const Ops* ops, const Post* post, Evaluate&& evaluate, int32_t (*save_default)(void*, uint32_t, const char*),
                           std::vector<float>& max_eval_reward, GroupObserver obs, void* ctx)
{
    if (!post) return BDR_OK;
    const uint32_t P = ops->n_members;
    const auto save = post->save_member ? post->save_member : save_default;
    if (post->eval_interval && s.opt_steps % post->eval_interval == 0) {
        BDR_TRY(ops->set_train(ops->group, 0));
        std::vector<bdr_eval_result> r(P);
        BDR_TRY(evaluate(post->evaluators, &post->eval_ops, r.data()));
        BDR_TRY(ops->set_train(ops->group, 1));
        if (obs)
            for (uint32_t p = 0; p < P; ++p) {
                const float sc[2] = {r[p].score, r[p].normalized};
                obs(ctx, p, s.env_steps, s.opt_steps, BDR_TRAINER_EVENT_EVAL, sc, r[p].has_normalized ? 2 : 1);
            }
        for (uint32_t p = 0; p < P; ++p) {
            if (!(r[p].score > max_eval_reward[p])) continue;
            max_eval_reward[p] = r[p].score;
            BDR_TRY(save(ops->group, p, (std::string(post->model_dirs[p]) + "/best").c_str()));
        }
    }
    if (post->save_interval > 0 && s.opt_steps % post->save_interval == 0)
        for (uint32_t p = 0; p < P; ++p) BDR_TRY(save(ops->group, p, (std::string(post->model_dirs[p]) + "/" + std::to_string(s.opt_steps)).c_str()));
    return BDR_OK;
}

// cost_record once for the group: every member's observer receives the one COST event, in member order
void group_cost_record(State& s, GroupObserver obs, void* obs_ctx, uint32_t P)
{
    struct Fan { GroupObserver obs; void* ctx; uint32_t P; } fan{obs, obs_ctx, P};
    cost_record(s, obs ? +[](void* f, uint64_t es, uint64_t os, int32_t ev, const float* sc, int32_t n) {
        const Fan* fn = (const Fan*)f;
        for (uint32_t p = 0; p < fn->P; ++p) fn->obs(fn->ctx, p, es, os, ev, sc, n);
    } : nullptr, &fan);
}

// ---- the online group loop, once: bdr_trainer_train_group_post (one i64 action per member) and bdr_trainer_train_cgroup_post (f32
// action rows, an observation dtype per member) share train_group_loop; an Actions type holds the members' action rows of an iteration
// and makes the table's acting and push calls on them
template <class Ops>
int32_t check_group_loop(const bdr_trainer_config* c, const uint64_t* obs_row_bytes, const Ops* ops, const bdr_env_vtable* envs)
{
    BDR_REQUIRE(c->max_opts >= 1, "max_opts must be >= 1");
    BDR_REQUIRE(c->opt_interval >= 1, "opt_interval must be >= 1");
    BDR_REQUIRE(ops->set_train && ops->sample && ops->push && ops->opt && ops->opt_with_record, "group function table is incomplete");
    const uint32_t P = ops->n_members;
    BDR_REQUIRE(P >= 1 && ops->buffers, "the group function table names no members or no buffers");
    for (uint32_t p = 0; p < P; ++p) {
        BDR_REQUIRE(envs[p].reset && envs[p].step_with_reset, "member %u: environment function table is incomplete", p);
        BDR_REQUIRE(!envs[p].obs_on_device, "member %u: the group loop takes host observations (obs_on_device environments are not supported)", p);
        BDR_REQUIRE(obs_row_bytes[p] > 0, "member %u: obs_row_bytes must be set", p);
    }
    return BDR_OK;
}

struct I64Actions {   // bdr_group_trainer_ops: one i64 action per member, one array
    const bdr_group_trainer_ops* ops;
    std::vector<int64_t> act;
    explicit I64Actions(const bdr_group_trainer_ops* o) : ops(o), act(o->n_members) {}
    const void* row(uint32_t p) const { return &act[p]; }
    int32_t sample(const void* const* rows) { return ops->sample(ops->group, rows, act.data()); }
    int32_t push(const void* const* rows, const void* const* next_rows, const float* reward, const int8_t* term, const int8_t* trunc)
    {
        return ops->push(ops->group, ops->buffers, rows, act.data(), next_rows, reward, term, trunc);
    }
};

struct F32Actions {   // bdr_cgroup_trainer_ops: one f32 action row per member; every array of a call is indexed by member
    const bdr_cgroup_trainer_ops* ops;
    std::vector<int32_t> dtypes;
    std::vector<float> act;
    std::vector<float*> act_p;
    std::vector<const float*> reward_p; std::vector<const int8_t*> term_p, trunc_p;
    F32Actions(const bdr_cgroup_trainer_ops* o, uint64_t act_row_bytes, const int32_t* obs_dtypes)
        : ops(o), dtypes(o->n_members, BDR_DTYPE_F32), act((size_t)o->n_members * (act_row_bytes / 4)), act_p(o->n_members), reward_p(o->n_members),
          term_p(o->n_members), trunc_p(o->n_members)
    {
        for (uint32_t p = 0; p < o->n_members; ++p) {
            act_p[p] = act.data() + (size_t)p * (act_row_bytes / 4);
            if (obs_dtypes) dtypes[p] = obs_dtypes[p];
        }
    }
    const void* row(uint32_t p) const { return act_p[p]; }
    int32_t sample(const void* const* rows) { return ops->sample(ops->group, rows, dtypes.data(), act_p.data()); }
    int32_t push(const void* const* rows, const void* const* next_rows, const float* reward, const int8_t* term, const int8_t* trunc)
    {
        for (uint32_t p = 0; p < ops->n_members; ++p) { reward_p[p] = reward + p; term_p[p] = term + p; trunc_p[p] = trunc + p; }
        return ops->push(ops->group, ops->buffers, rows, next_rows, dtypes.data(), act_p.data(), reward_p.data(), term_p.data(), trunc_p.data());
    }
};

// Trainer::train (trainer.rs:267-327) with post_process for every member in lockstep; everything has been checked
template <class Ops, class Post, class Actions, class Evaluate>
int32_t train_group_loop(const bdr_trainer_config* c, const uint64_t* obs_row_bytes, const Ops* ops, const bdr_env_vtable* envs, const Post* post, Actions& actions,
                         Evaluate&& evaluate, int32_t (*save_default)(void*, uint32_t, const char*), GroupObserver obs, void* obs_ctx, bdr_trainer_stats* out)
{
    const uint32_t P = ops->n_members;
    std::vector<float> max_eval_reward(P, -FLT_MAX);   // f32::MIN (trainer.rs: max_eval_reward), one per member
    GroupAdapter ga(ops, P);
    bdr_trainer_ops t{};
    t.agent = &ga; t.agent_set_train = ga_set_train; t.agent_opt = ga_opt; t.agent_opt_with_record = ga_opt_rec;
    State s; s.c = c; s.ops = &t;
    // per member: the Sampler's / SimpleStepProcessor's prev_obs, the step's obs and init_obs (bdr_trainer_train's three rows)
    std::vector<std::vector<uint8_t>> prev(P), obs_new(P), init_obs(P);
    std::vector<const void*> prev_p(P), new_p(P);
    for (uint32_t p = 0; p < P; ++p) { prev[p].resize(obs_row_bytes[p]); obs_new[p].resize(obs_row_bytes[p]); init_obs[p].resize(obs_row_bytes[p]); }
    std::vector<float> reward(P);
    std::vector<int8_t> term(P), trunc(P);
    std::vector<uint64_t> n_episodes(P, 0);
    bool have_prev = false;
    BDR_TRY(t.agent_set_train(t.agent, 1));   // trainer.rs:283
    for (;;) {
        const auto t0 = Clock::now();
        // ---- Sampler::sample_and_push (sampler.rs:99-144) of every member
        if (!have_prev) {
            for (uint32_t p = 0; p < P; ++p) BDR_TRY(envs[p].reset(envs[p].ctx, prev[p].data()));
            have_prev = true;
        }
        for (uint32_t p = 0; p < P; ++p) { prev_p[p] = prev[p].data(); new_p[p] = obs_new[p].data(); }
        BDR_TRY(actions.sample(prev_p.data()));
        for (uint32_t p = 0; p < P; ++p) {
            reward[p] = 0; term[p] = 0; trunc[p] = 0;
            BDR_TRY(envs[p].step_with_reset(envs[p].ctx, actions.row(p), obs_new[p].data(), &reward[p], &term[p], &trunc[p], init_obs[p].data()));
        }
        BDR_TRY(actions.push(prev_p.data(), new_p.data(), reward.data(), term.data(), trunc.data()));
        for (uint32_t p = 0; p < P; ++p) {
            const bool is_done = term[p] == 1 || trunc[p] == 1;   // step.rs:136-138
            prev[p].swap(is_done ? init_obs[p] : obs_new[p]);     // prev_obs = init_obs / obs (sampler.rs:137-141, step_proc.rs:131-135)
            if (is_done) n_episodes[p] += 1;
        }
        const double dt = std::chrono::duration<double>(Clock::now() - t0).count();
        s.timer_for_samples += dt; s.total_sample += dt;
        s.samples_counter += 1;
        s.env_steps += 1;
        // ---- train_step, once for all members; every member's event; the cost record
        bool is_opt = false, with_record = false;
        BDR_TRY(train_step(s, &is_opt, &with_record));
        const int32_t event = is_opt ? (with_record ? BDR_TRAINER_EVENT_OPT_RECORD : BDR_TRAINER_EVENT_OPT) : BDR_TRAINER_EVENT_SKIP;
        if (obs)
            for (uint32_t p = 0; p < P; ++p) obs(obs_ctx, p, s.env_steps, s.opt_steps, event, ga.scalars.data() + (size_t)p * 128, with_record ? ga.n_scalars[p] : 0);
        if (is_opt) BDR_TRY(group_post_process(s, ops, post, evaluate, save_default, max_eval_reward, obs, obs_ctx));
        group_cost_record(s, obs, obs_ctx, P);
        if (s.opt_steps == c->max_opts) break;   // trainer.rs:323-325
    }
    if (out)
        for (uint32_t p = 0; p < P; ++p) { fill_stats(s, out + p); out[p].n_episodes = n_episodes[p]; }
    return BDR_OK;
}


// an AWAC or a candle SAC group's online entries behind bdr_cgroup_trainer_ops (bdr_*_group_ctrainer_ops_default): the offline
// table's set_train / opt / opt_with_record (Base), acting on one row per member and the grouped push of one transition per member
template <class G, class Base, auto SampleAll, auto Push>
struct CGroupEntries {
    static int32_t sample(void* g, const void* const* rows, const int32_t* dtypes, float* const* act_out) { return SampleAll((G*)g, nullptr, 1, rows, dtypes, act_out); }
    static int32_t push(void* g, void* const* b, const void* const* rows, const void* const* next_rows, const int32_t* dtypes, const float* const* act,
                        const float* const* reward, const int8_t* const* term, const int8_t* const* trunc)
    {
        return Push((G*)g, (bdr_replay* const*)b, 1, rows, next_rows, dtypes, act, reward, term, trunc);
    }
    static void trainer_ops(bdr_cgroup_trainer_ops* ops, G* group, bdr_replay* const* buffers)
    {
        if (!ops) return;
        bdr_group_trainer_ops t;
        Base::trainer_ops(&t, group, buffers);
        memset(ops, 0, sizeof *ops);
        ops->group = t.group; ops->buffers = t.buffers; ops->n_members = t.n_members;
        ops->set_train = t.set_train; ops->opt = t.opt; ops->opt_with_record = t.opt_with_record;
        ops->sample = sample; ops->push = push;
    }
};
using AwacGroupOnline = CGroupEntries<bdr_awac_group, AwacGroupEntries, bdr_awac_group_sample, bdr_awac_group_push>;
using CandleSacGroupOnline = CGroupEntries<bdr_candle_sac_group, CandleSacGroupEntries, bdr_candle_sac_group_sample, bdr_candle_sac_group_push>;
// the kinds a default online table can name: the widths of a member, the kind in messages, its save
struct CGroupKindRow {
    decltype(bdr_cgroup_trainer_ops::sample) sample;
    int (*act_dim)(const void*, uint32_t);
    int (*obs_dim)(const void*, uint32_t);
    const char* a;
    int32_t (*save_member)(void*, uint32_t, const char*);
};
const CGroupKindRow* cgroup_kind_of(const bdr_cgroup_trainer_ops* ops)
{
    static const CGroupKindRow kinds[] = {{AwacGroupOnline::sample, awac_group_act_dim, awac_group_obs_dim, "an AWAC", AwacGroupEntries::save_member},
                                          {CandleSacGroupOnline::sample, candle_sac_group_act_dim, candle_sac_group_obs_dim, "a candle SAC", CandleSacGroupEntries::save_member}};
    for (const CGroupKindRow& k : kinds) if (ops->sample == k.sample) return &k;
    return nullptr;
}
}  // namespace

namespace bdr {
// the GPU of the library's own ring behind a function table (bdr_trainer_ops_default); false: the caller's own buffer object
bool default_buffer_device(const bdr_trainer_ops* t, int* device)
{
    if (!t || !t->buffer || t->buffer_push_device != d_push_dev) return false;
    *device = ((const bdr_replay*)t->buffer)->device;
    return true;
}
}  // namespace bdr

extern "C" {

void bdr_trainer_config_default(bdr_trainer_config* c)   // trainer/config.rs:68-87 (intervals the loops use; 0 = never)
{
    if (!c) return;
    memset(c, 0, sizeof *c);
    c->max_opts = 0; c->opt_interval = 1; c->warmup_period = 0;
    c->record_agent_info_interval = 0; c->record_compute_cost_interval = 0;
}

void bdr_trainer_ops_default(bdr_trainer_ops* ops, bdr_agent* agent, bdr_replay* buffer)
{
    if (!ops) return;
    ops->agent = agent; ops->buffer = buffer;
    ops->agent_set_train = d_set_train; ops->agent_sample = default_sample; ops->agent_opt = d_opt;
    ops->agent_opt_with_record = d_opt_rec; ops->buffer_push = d_push;
    ops->agent_sample_device = default_sample_device; ops->buffer_push_device = d_push_dev;
}

void bdr_evaluator_default(bdr_evaluator* ev, bdr_agent*)
{
    if (!ev) return;
    memset(ev, 0, sizeof *ev);
    ev->obs_dtype = BDR_DTYPE_F32;
    ev->agent_sample = default_sample; ev->agent_sample_raw = d_sample_raw;
}

void bdr_trainer_post_default(bdr_trainer_post* post)
{
    if (!post) return;
    memset(post, 0, sizeof *post);
    post->save_params = d_save;
}

// default_evaluator.rs:64-88
int32_t bdr_evaluate(const bdr_evaluator* ev, void* agent, bdr_eval_result* out)
{
    BDR_REQUIRE(ev && out, "null argument");
    BDR_REQUIRE(ev->env.reset_with_index && ev->env.step, "the evaluator's environment function table is incomplete");
    BDR_REQUIRE(ev->n_episodes >= 1, "n_episodes must be >= 1");
    BDR_REQUIRE(ev->obs_row_bytes > 0 && ev->act_row_bytes > 0, "obs_row_bytes / act_row_bytes must be set");
    BDR_REQUIRE(ev->obs_dtype == BDR_DTYPE_F32 || ev->obs_dtype == BDR_DTYPE_F64, "obs_dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64");
    const bool dev = ev->env.obs_on_device != 0;
    const bool raw = ev->norm != nullptr || ev->obs_dtype != BDR_DTYPE_F32 || dev;
    BDR_REQUIRE(raw ? ev->agent_sample_raw != nullptr : ev->agent_sample != nullptr,
                raw ? "normalised, float64 or device-resident rows need agent_sample_raw" : "agent_sample is not set");
    ObsRow prev, next;
    BDR_TRY(prev.init(dev, ev->env.device, ev->obs_row_bytes)); BDR_TRY(next.init(dev, ev->env.device, ev->obs_row_bytes));
    std::vector<uint8_t> act(std::max<uint64_t>(ev->act_row_bytes, 8));
    float r_total = 0.f;
    uint64_t n_steps = 0;
    for (uint64_t ix = 0; ix < ev->n_episodes; ++ix) {
        BDR_TRY(ev->env.reset_with_index(ev->env.ctx, ix, prev.p()));
        for (;;) {
            if (raw) BDR_TRY(ev->agent_sample_raw(agent, ev->norm, 1, prev.p(), ev->obs_dtype, dev ? 1 : 0, ev->obs_row_bytes, act.data()));
            else BDR_TRY(ev->agent_sample(agent, 1, prev.p(), act.data()));
            float reward = 0; int8_t term = 0, trunc = 0;
            BDR_TRY(ev->env.step(ev->env.ctx, act.data(), next.p(), &reward, &term, &trunc));
            r_total += reward;
            n_steps += 1;
            if (term == 1 || trunc == 1) break;   // step.rs:136-138
            prev.swap(next);                      // prev_obs = step.obs
        }
    }
    out->score = r_total / (float)ev->n_episodes;
    out->has_normalized = ev->has_ref_scores ? 1 : 0;
    out->normalized = ev->has_ref_scores ? (out->score - ev->ref_min_score) / (ev->ref_max_score - ev->ref_min_score) : 0.f;   // border-minari/src/env.rs:162-168
    out->n_steps = n_steps; out->n_episodes = ev->n_episodes;
    return BDR_OK;
}

int32_t bdr_trainer_train(const bdr_trainer_config* c, const bdr_trainer_ops* ops, const bdr_env_vtable* env,
                          bdr_trainer_observer obs, void* obs_ctx, bdr_trainer_stats* out)
{
    return bdr_trainer_train_post(c, ops, env, nullptr, obs, obs_ctx, out);
}

int32_t bdr_trainer_train_post(const bdr_trainer_config* c, const bdr_trainer_ops* ops, const bdr_env_vtable* env, const bdr_trainer_post* post,
                               bdr_trainer_observer obs, void* obs_ctx, bdr_trainer_stats* out)
{
    BDR_TRY(check(c, ops));
    BDR_TRY(check_post(post));
    BDR_REQUIRE(env && env->reset && env->step_with_reset, "environment function table is incomplete");
    BDR_REQUIRE(ops->agent_sample && ops->buffer_push, "the online loop needs agent_sample and buffer_push");
    BDR_REQUIRE(c->obs_row_bytes > 0 && c->act_row_bytes > 0, "obs_row_bytes / act_row_bytes must be set");
    const bool dev = env->obs_on_device != 0;   // the environment's observations live in HBM: act and push through the *_device entries
    BDR_REQUIRE(!dev || (ops->agent_sample_device && ops->buffer_push_device), "a device-resident environment needs agent_sample_device and buffer_push_device");
    State s; s.c = c; s.ops = ops;
    // Sampler state (sampler.rs:61-75) + SimpleStepProcessor::prev_obs (step_proc.rs:86-101).  The sampler's prev_obs and the step
    // processor's are the same observation at the top of every iteration (both become init_obs after a terminal step, obs otherwise):
    // one buffer, host or device
    ObsRow prev, obs_new, init_obs;
    BDR_TRY(prev.init(dev, env->device, c->obs_row_bytes)); BDR_TRY(obs_new.init(dev, env->device, c->obs_row_bytes)); BDR_TRY(init_obs.init(dev, env->device, c->obs_row_bytes));
    std::vector<uint8_t> act(c->act_row_bytes);
    bool have_prev = false;
    BDR_TRY(ops->agent_set_train(ops->agent, 1));   // trainer.rs:283
    for (;;) {
        const auto t0 = Clock::now();
        // ---- Sampler::sample_and_push (sampler.rs:99-144)
        if (!have_prev) {
            BDR_TRY(env->reset(env->ctx, prev.p()));    // (+ step_processor.reset(prev_obs.clone()))
            have_prev = true;
        }
        if (dev) BDR_TRY(ops->agent_sample_device(ops->agent, 1, prev.p(), c->obs_row_bytes, act.data()));
        else BDR_TRY(ops->agent_sample(ops->agent, 1, prev.p(), act.data()));
        float reward = 0; int8_t term = 0, trunc = 0;
        BDR_TRY(env->step_with_reset(env->ctx, act.data(), obs_new.p(), &reward, &term, &trunc, init_obs.p()));
        const bool is_done = term == 1 || trunc == 1;   // step.rs:136-138
        // SimpleStepProcessor::process (step_proc.rs:103-137): (prev_obs, act, obs, reward, flags); next transition starts
        // from obs, or from init_obs after a terminal step
        if (dev) BDR_TRY(ops->buffer_push_device(ops->buffer, 1, prev.p(), c->obs_row_bytes, act.data(), obs_new.p(), c->obs_row_bytes, &reward, &term, &trunc));
        else BDR_TRY(ops->buffer_push(ops->buffer, 1, prev.p(), act.data(), obs_new.p(), &reward, &term, &trunc));
        prev.swap(is_done ? init_obs : obs_new);        // prev_obs = init_obs / obs (sampler.rs:137-141, step_proc.rs:131-135)
        if (is_done) s.n_episodes += 1;
        const double dt = std::chrono::duration<double>(Clock::now() - t0).count();
        s.timer_for_samples += dt; s.total_sample += dt;
        s.samples_counter += 1;
        s.env_steps += 1;
        // ---- train_step + post_process + records
        bool stop = false;
        BDR_TRY(step_and_records(s, post, obs, obs_ctx, &stop));
        if (stop) break;
    }
    fill_stats(s, out);
    return BDR_OK;
}

void bdr_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_agent_group* group, bdr_replay* const* buffers)
{
    if (!ops) return;
    memset(ops, 0, sizeof *ops);
    ops->group = group; ops->buffers = (void* const*)buffers;
    if (group) (void)bdr_agent_group_size(group, &ops->n_members);
    ops->set_train = dg_set_train; ops->sample = dg_sample; ops->push = dg_push; ops->opt = dg_opt; ops->opt_with_record = dg_opt_rec;
}

void bdr_group_eval_ops_default(bdr_group_eval_ops* ops, bdr_agent_group* group)
{
    if (!ops) return;
    memset(ops, 0, sizeof *ops);
    ops->group = group;
    if (group) (void)bdr_agent_group_size(group, &ops->n_members);
    ops->sample_members = dg_sample_members;
}

void bdr_group_trainer_post_default(bdr_group_trainer_post* post, bdr_agent_group* group)
{
    if (!post) return;
    memset(post, 0, sizeof *post);
    bdr_group_eval_ops_default(&post->eval_ops, group);
    post->save_member = dg_save_member;
}

// default_evaluator.rs:64-88 for every member in lockstep: member p sees exactly the calls bdr_evaluate(&evs[p], member p) makes
int32_t bdr_evaluate_group(const bdr_evaluator* evs, const bdr_group_eval_ops* ops, bdr_eval_result* out)
{
    BDR_REQUIRE(evs && ops && out, "null argument");
    BDR_TRY(check_group_eval(evs, ops));
    // (act_row_bytes == 8 for every member: the action rows are one i64 array indexed by member)
    return evaluate_lockstep(evs, ops->n_members, [&](const uint32_t* sel, uint32_t n_sel, const void* const* rows, uint8_t* const* act_rows) {
        return ops->sample_members(ops->group, sel, n_sel, rows, reinterpret_cast<int64_t*>(act_rows[0]));
    }, out);
}

void bdr_bc_group_eval_ops_default(bdr_bc_group_eval_ops* ops, bdr_bc_group* group) { BcGroupEntries::eval_ops(ops, group); }
void bdr_iql_group_eval_ops_default(bdr_bc_group_eval_ops* ops, bdr_iql_group* group) { IqlGroupEntries::eval_ops(ops, group); }
void bdr_awac_group_eval_ops_default(bdr_bc_group_eval_ops* ops, bdr_awac_group* group) { AwacGroupEntries::eval_ops(ops, group); }
void bdr_candle_sac_group_eval_ops_default(bdr_bc_group_eval_ops* ops, bdr_candle_sac_group* group) { CandleSacGroupEntries::eval_ops(ops, group); }

// the same loop for a BC or an IQL group: f32 action rows, f32 or float64 observation rows, a normaliser per member
int32_t bdr_evaluate_bc_group(const bdr_evaluator* evs, const bdr_bc_group_eval_ops* ops, bdr_eval_result* out)
{
    BDR_REQUIRE(evs && ops && out, "null argument");
    BDR_TRY(check_bc_group_eval(evs, ops));
    const uint32_t P = ops->n_members;
    std::vector<const bdr_obs_norm*> norms(P);
    std::vector<int32_t> dtypes(P);
    std::vector<float*> act_out(P);
    for (uint32_t p = 0; p < P; ++p) { norms[p] = evs[p].norm; dtypes[p] = evs[p].obs_dtype; }
    return evaluate_lockstep(evs, P, [&](const uint32_t* sel, uint32_t n_sel, const void* const* rows, uint8_t* const* act_rows) {
        for (uint32_t p = 0; p < P; ++p) act_out[p] = reinterpret_cast<float*>(act_rows[p]);
        return ops->sample_members(ops->group, sel, n_sel, norms.data(), rows, dtypes.data(), act_out.data());
    }, out);
}

void bdr_bc_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_bc_group* group, bdr_replay* const* buffers)
{
    BcGroupEntries::trainer_ops(ops, group, buffers);
}
void bdr_bc_group_trainer_post_default(bdr_bc_group_trainer_post* post, bdr_bc_group* group) { BcGroupEntries::trainer_post(post, group); }
void bdr_iql_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_iql_group* group, bdr_replay* const* buffers)
{
    IqlGroupEntries::trainer_ops(ops, group, buffers);
}
void bdr_iql_group_trainer_post_default(bdr_bc_group_trainer_post* post, bdr_iql_group* group) { IqlGroupEntries::trainer_post(post, group); }
void bdr_awac_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_awac_group* group, bdr_replay* const* buffers)
{
    AwacGroupEntries::trainer_ops(ops, group, buffers);
}
void bdr_awac_group_trainer_post_default(bdr_bc_group_trainer_post* post, bdr_awac_group* group) { AwacGroupEntries::trainer_post(post, group); }
void bdr_candle_sac_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_candle_sac_group* group, bdr_replay* const* buffers)
{
    CandleSacGroupEntries::trainer_ops(ops, group, buffers);
}
void bdr_candle_sac_group_trainer_post_default(bdr_bc_group_trainer_post* post, bdr_candle_sac_group* group) { CandleSacGroupEntries::trainer_post(post, group); }

// Trainer::train_offline (trainer.rs:330-384) with post_process for every member of a group (BC or IQL) in lockstep
int32_t bdr_trainer_train_offline_group_post(const bdr_trainer_config* c_in, const bdr_group_trainer_ops* ops, const bdr_bc_group_trainer_post* post,
                                             void (*obs)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps, int32_t event, const float* scalars,
                                                         int32_t n_scalars),
                                             void* obs_ctx, bdr_trainer_stats* out)
{
    BDR_REQUIRE(c_in && ops, "null argument");
    BDR_REQUIRE(c_in->max_opts >= 1, "max_opts must be >= 1");
    BDR_REQUIRE(ops->set_train && ops->opt && ops->opt_with_record, "group function table is incomplete");
    const uint32_t P = ops->n_members;
    BDR_REQUIRE(P >= 1 && ops->buffers, "the group function table names no members or no buffers");
    BDR_TRY(check_group_post(post, P, check_bc_group_eval));
    // a NULL save_member: the save of the group kind the evaluation table names - IQL's default table: an IQL member, anything else: a BC member
    const GroupKindRow* kind = post ? group_kind_of(&post->eval_ops) : nullptr;
    const auto save_default = kind ? kind->save_member : BcGroupEntries::save_member;
    bdr_trainer_config c = *c_in;
    c.warmup_period = 0; c.opt_interval = 1;            // trainer.rs:345-346
    std::vector<float> max_eval_reward(P, -FLT_MAX);   // f32::MIN (trainer.rs: max_eval_reward), one per member
    GroupAdapter ga(ops, P);
    bdr_trainer_ops t{};
    t.agent = &ga; t.agent_set_train = ga_set_train; t.agent_opt = ga_opt; t.agent_opt_with_record = ga_opt_rec;
    State s; s.c = &c; s.ops = &t;
    BDR_TRY(t.agent_set_train(t.agent, 1));
    for (;;) {
        s.env_steps += 1;
        // ---- train_step, once for all members; every member's event; post_process; the cost record
        bool is_opt = false, with_record = false;
        BDR_TRY(train_step(s, &is_opt, &with_record));
        const int32_t event = with_record ? BDR_TRAINER_EVENT_OPT_RECORD : BDR_TRAINER_EVENT_OPT;
        if (obs)
            for (uint32_t p = 0; p < P; ++p) obs(obs_ctx, p, s.env_steps, s.opt_steps, event, ga.scalars.data() + (size_t)p * 128, with_record ? ga.n_scalars[p] : 0);
        BDR_TRY(group_post_process(s, ops, post, bdr_evaluate_bc_group, save_default, max_eval_reward, obs, obs_ctx));
        group_cost_record(s, obs, obs_ctx, P);
        if (s.opt_steps == c.max_opts) break;   // trainer.rs:323-325
    }
    if (out)
        for (uint32_t p = 0; p < P; ++p) fill_stats(s, out + p);
    return BDR_OK;
}

int32_t bdr_trainer_train_group(const bdr_trainer_config* c, const uint64_t* obs_row_bytes, const bdr_group_trainer_ops* ops, const bdr_env_vtable* envs,
                                void (*obs)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps, int32_t event, const float* scalars,
                                            int32_t n_scalars),
                                void* obs_ctx, bdr_trainer_stats* out)
{
    return bdr_trainer_train_group_post(c, obs_row_bytes, ops, envs, nullptr, obs, obs_ctx, out);
}

int32_t bdr_trainer_train_group_post(const bdr_trainer_config* c, const uint64_t* obs_row_bytes, const bdr_group_trainer_ops* ops, const bdr_env_vtable* envs,
                                     const bdr_group_trainer_post* post,
                                     void (*obs)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps, int32_t event, const float* scalars,
                                                 int32_t n_scalars),
                                     void* obs_ctx, bdr_trainer_stats* out)
{
    BDR_REQUIRE(c && ops && envs && obs_row_bytes, "null argument");
    BDR_TRY(check_group_loop(c, obs_row_bytes, ops, envs));
    BDR_REQUIRE(c->act_row_bytes == 8, "a group acts with one i64 action per member: act_row_bytes must be 8");
    BDR_TRY(check_group_post(post, ops->n_members, check_group_eval));
    I64Actions actions(ops);
    return train_group_loop(c, obs_row_bytes, ops, envs, post, actions, bdr_evaluate_group, dg_save_member, obs, obs_ctx, out);
}

// ---- a candle DQN group behind the i64-action tables (bdr_group_trainer_ops, bdr_group_eval_ops): one float32 row and one i64 action
// per member, over the group's own C functions
namespace {
using CandleDqnGroupEntries = GroupEntries<bdr_candle_dqn_group, bdr_candle_dqn_group_size, bdr_candle_dqn_group_member, bdr_candle_dqn_group_opt,
                                           bdr_candle_dqn_group_opt_with_scalars, bdr_candle_dqn_group_sample_members>;
// the per-member pointer arrays of a table call: their sizes are fixed per group, so they are kept from call to call (one set per
// thread: a compiled loop runs on the thread that called it) instead of being allocated on every environment step
struct CdqGroupScratch {
    std::vector<int32_t> dtypes; std::vector<int64_t*> out; std::vector<const int64_t*> act; std::vector<const float*> rew; std::vector<const int8_t*> term, trunc;
    void size(uint32_t P)
    {
        if (dtypes.size() == P) return;
        dtypes.assign(P, BDR_DTYPE_F32); out.resize(P); act.resize(P); rew.resize(P); term.resize(P); trunc.resize(P);
    }
};
CdqGroupScratch* cdq_scratch(void* g, uint32_t* P)
{
    static thread_local CdqGroupScratch s;
    *P = 0;
    if (bdr_candle_dqn_group_size((bdr_candle_dqn_group*)g, P) == BDR_OK) s.size(*P);
    return &s;
}
int32_t cdq_group_sample_members(void* g, const uint32_t* members, uint32_t n_sel, const void* const* obs, int64_t* act)
{
    uint32_t P = 0;
    CdqGroupScratch& s = *cdq_scratch(g, &P);
    BDR_REQUIRE(P >= 1, "null group");
    for (uint32_t p = 0; p < P; ++p) s.out[p] = act + p;
    return members ? bdr_candle_dqn_group_sample_members((bdr_candle_dqn_group*)g, members, n_sel, nullptr, 1, obs, s.dtypes.data(), s.out.data())
                   : bdr_candle_dqn_group_sample((bdr_candle_dqn_group*)g, nullptr, 1, obs, s.dtypes.data(), s.out.data());
}
int32_t cdq_group_sample(void* g, const void* const* obs, int64_t* act) { return cdq_group_sample_members(g, nullptr, 0, obs, act); }
int32_t cdq_group_push(void* g, void* const* b, const void* const* obs, const int64_t* act, const void* const* next_obs, const float* rew, const int8_t* term,
                       const int8_t* trunc)
{
    uint32_t P = 0;
    CdqGroupScratch& s = *cdq_scratch(g, &P);
    BDR_REQUIRE(P >= 1, "null group");
    for (uint32_t p = 0; p < P; ++p) { s.act[p] = act + p; s.rew[p] = rew + p; s.term[p] = term + p; s.trunc[p] = trunc + p; }
    return bdr_candle_dqn_group_push((bdr_candle_dqn_group*)g, (bdr_replay* const*)b, 1, obs, next_obs, nullptr, s.act.data(), s.rew.data(), s.term.data(), s.trunc.data());
}
}  // namespace
void bdr_candle_dqn_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_candle_dqn_group* group, bdr_replay* const* buffers)
{
    CandleDqnGroupEntries::trainer_ops(ops, group, buffers);
    if (ops) { ops->sample = cdq_group_sample; ops->push = cdq_group_push; }
}
void bdr_candle_dqn_group_eval_ops_default(bdr_group_eval_ops* ops, bdr_candle_dqn_group* group)
{
    if (!ops) return;
    memset(ops, 0, sizeof *ops);
    ops->group = group;
    if (group) (void)bdr_candle_dqn_group_size(group, &ops->n_members);
    ops->sample_members = cdq_group_sample_members;
}
void bdr_candle_dqn_group_trainer_post_default(bdr_group_trainer_post* post, bdr_candle_dqn_group* group)
{
    if (!post) return;
    memset(post, 0, sizeof *post);
    bdr_candle_dqn_group_eval_ops_default(&post->eval_ops, group);
    post->save_member = CandleDqnGroupEntries::save_member;
}

void bdr_awac_group_ctrainer_ops_default(bdr_cgroup_trainer_ops* ops, bdr_awac_group* group, bdr_replay* const* buffers)
{
    AwacGroupOnline::trainer_ops(ops, group, buffers);
}
void bdr_candle_sac_group_ctrainer_ops_default(bdr_cgroup_trainer_ops* ops, bdr_candle_sac_group* group, bdr_replay* const* buffers)
{
    CandleSacGroupOnline::trainer_ops(ops, group, buffers);
}

// the same loop for an AWAC or a candle SAC group: f32 action rows, f32 or float64 observation rows, the grouped push of the group core
int32_t bdr_trainer_train_cgroup_post(const bdr_trainer_config* c, const uint64_t* obs_row_bytes, const int32_t* obs_dtypes, const bdr_cgroup_trainer_ops* ops,
                                      const bdr_env_vtable* envs, const bdr_bc_group_trainer_post* post,
                                      void (*obs)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps, int32_t event, const float* scalars,
                                                  int32_t n_scalars),
                                      void* obs_ctx, bdr_trainer_stats* out)
{
    BDR_REQUIRE(c && ops && envs && obs_row_bytes, "null argument");
    BDR_TRY(check_group_loop(c, obs_row_bytes, ops, envs));
    const uint32_t P = ops->n_members;
    BDR_REQUIRE(c->act_row_bytes > 0 && c->act_row_bytes % 4 == 0, "a continuous-action group acts with f32 action rows: act_row_bytes must be a positive multiple of 4");
    const CGroupKindRow* online = cgroup_kind_of(ops);
    for (uint32_t p = 0; p < P; ++p) {
        const int32_t dt = obs_dtypes ? obs_dtypes[p] : BDR_DTYPE_F32;
        BDR_REQUIRE(dt == BDR_DTYPE_F32 || dt == BDR_DTYPE_F64, "member %u: obs_dtype must be BDR_DTYPE_F32 or BDR_DTYPE_F64", p);
        if (!online) continue;
        const int A = online->act_dim(ops->group, p), O = online->obs_dim(ops->group, p);
        BDR_REQUIRE(A > 0 && O > 0, "member %u: the group has no such member", p);
        BDR_REQUIRE(c->act_row_bytes == (uint64_t)A * 4, "member %u: %s group acts with one f32 action row per member: act_row_bytes must be 4 * act_dim = %d", p, online->a, A * 4);
        BDR_REQUIRE(obs_row_bytes[p] == (uint64_t)O * (dt == BDR_DTYPE_F64 ? 8 : 4), "member %u: obs_row_bytes must be obs_dim = %d elements of its obs_dtype", p, O);
    }
    BDR_TRY(check_group_post(post, P, check_bc_group_eval));
    const GroupKindRow* kind = post ? group_kind_of(&post->eval_ops) : nullptr;
    const auto save_default = kind ? kind->save_member : (online ? online->save_member : BcGroupEntries::save_member);
    F32Actions actions(ops, c->act_row_bytes, obs_dtypes);
    return train_group_loop(c, obs_row_bytes, ops, envs, post, actions, bdr_evaluate_bc_group, save_default, obs, obs_ctx, out);
}

int32_t bdr_trainer_train_offline(const bdr_trainer_config* c_in, const bdr_trainer_ops* ops, bdr_trainer_observer obs, void* obs_ctx,
                                  bdr_trainer_stats* out)
{
    return bdr_trainer_train_offline_post(c_in, ops, nullptr, obs, obs_ctx, out);
}

int32_t bdr_trainer_train_offline_post(const bdr_trainer_config* c_in, const bdr_trainer_ops* ops, const bdr_trainer_post* post, bdr_trainer_observer obs,
                                       void* obs_ctx, bdr_trainer_stats* out)
{
    BDR_TRY(check(c_in, ops));
    BDR_TRY(check_post(post));
    bdr_trainer_config c = *c_in;
    c.warmup_period = 0; c.opt_interval = 1;            // trainer.rs:345-346
    State s; s.c = &c; s.ops = ops;
    BDR_TRY(ops->agent_set_train(ops->agent, 1));
    for (;;) {
        s.env_steps += 1;
        bool stop = false;
        BDR_TRY(step_and_records(s, post, obs, obs_ctx, &stop));
        if (stop) break;
    }
    fill_stats(s, out);
    return BDR_OK;
}

}  // extern "C"
