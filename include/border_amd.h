/*
 * border_amd.h -- C ABI of the MI355X-native opt-step engine that sits behind border-core's
 * Agent / ReplayBufferBase / ExperienceBufferBase / SyncModel traits.
 *
 * The reference has no FFI of its own on this path (its only native boundary is
 * tch -> torch-sys -> libtorch, which this library replaces), so every entry point below is
 * shaped 1:1 after the Rust trait method it implements; the file:line of that method
 * (relative to the reference tree) is cited next to each declaration.  INTEGRATION.md shows
 * the Rust shim (`impl Agent for AmdDqn`, `impl ReplayBufferBase for AmdReplayBuffer`) a
 * maintainer would add on top of these symbols.
 *
 * Conventions
 *   - plain C types only; every function returns int32 status (BDR_OK == 0);
 *     bdr_last_error() returns a thread-local message for the last failure.
 *   - handles are opaque, heap allocated, NOT thread-safe but movable between threads
 *     (Rust `Send`, not `Sync`), one HIP stream per handle, hipSetDevice on every entry.
 *   - host pointers passed in are copied before the call returns unless stated otherwise.
 *   - there is no CPU fallback: without a HIP device every constructor fails with
 *     BDR_ERR_NO_DEVICE.
 */
#ifndef BORDER_AMD_H
#define BORDER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDR_API __attribute__((visibility("default")))

enum {
    BDR_OK = 0,
    BDR_ERR_INVALID = 1,    /* bad argument / config (anyhow::Error in the shim)     */
    BDR_ERR_NO_DEVICE = 2,  /* no HIP device / extension cannot run                  */
    BDR_ERR_HIP = 3,        /* a HIP runtime call failed                             */
    BDR_ERR_EMPTY = 4,      /* batch() on an empty buffer (the reference panics)     */
    BDR_ERR_IO = 5,         /* save/load failure                                     */
    BDR_ERR_COMM = 6        /* RCCL failure                                          */
};

typedef struct bdr_replay bdr_replay;
typedef struct bdr_agent bdr_agent;
typedef struct bdr_comm bdr_comm;

BDR_API const char* bdr_last_error(void);
/* 1 when the last failure on this thread reports a device-side condition of an EARLIER asynchronous step (an action index outside
 * [0, n_actions) that reached a TD step, a cross-queue wait that timed out, a non-finite priority): the call that returned it did NOT
 * fail on its own arguments, the condition has been cleared and the agent's state is that of the last good update.  Agent::opt returns
 * () in the reference (border-core/src/base/agent.rs:24-136): a caller of bdr_agent_opt may log such a report and go on, and must
 * treat every other failure (BDR_ERR_EMPTY, a buffer that does not match the agent, a HIP error of the call itself) as the reference's
 * panic.  0 otherwise.
 * 2 is the same kind of report raised by the step THE FAILING CALL ITSELF ran: bdr_agent_opt_with_record / _with_scalars enqueue the
 * step, synchronise and read the error words once more - when those flag this very step (its own TD kernel met an out-of-range action,
 * its own tree update a NaN priority) the step HAS run (n_opts and the optimizer step advanced once) and the record it produced is
 * complete in the caller's buffers (rec / out, *n_out).  A caller logs the report and keeps the record; it must NOT run the call
 * again to "retry" - that would be a second optimisation step.  After 1 the step of the failing call was never enqueued. */
BDR_API int32_t bdr_last_error_is_deferred(void);
BDR_API int32_t bdr_device_count(int32_t* count);
BDR_API const char* bdr_version(void);

/* ------------------------------------------------------------------------------------------
 * SimpleReplayBuffer  (border-core/src/generic_replay_buffer/base.rs:86-123)
 * ---------------------------------------------------------------------------------------- */

/* SimpleReplayBufferConfig (generic_replay_buffer/config.rs:185-210): capacity, seed; per_config = Some(..) is
 * bdr_replay_enable_per on the empty buffer (below). */
typedef struct {
    uint64_t capacity;
    uint64_t seed;
    uint64_t obs_row_bytes; /* bytes of one observation row (Atari: 4*1*84*84 u8 = 28224)  */
    uint64_t act_row_bytes; /* bytes of one action row (discrete: 8, one i64)              */
    int32_t device;         /* HIP device ordinal                                          */
    int32_t frame_stack;    /* 0: rows stored as given.  k > 0 (Atari: 4): SINGLE-FRAME store - an observation is k frames of
                             * obs_row_bytes / k bytes, newest first (border-atari-env/src/env.rs:197-209 stack_frame), and every
                             * distinct frame is stored once: obs_t / next_obs_t share k-1 frames and next_obs_t == obs_t+1 inside
                             * an episode, so a transition costs ONE new frame instead of 2k (8x less HBM for k = 4).  push()
                             * still takes the stacked rows and finds the sharing by comparing bytes (any input is stored
                             * exactly; what cannot be shared is stored in full), batch() rebuilds the stacks - indices, pushes
                             * and batches are identical to the plain ring's. */
    uint64_t frame_capacity;/* frames in the store (0: capacity + capacity / 4 + 64).  A push that would overwrite a frame a
                             * live transition still references fails with BDR_ERR_INVALID (raise frame_capacity). */
    int32_t index_rng;      /* BDR_RNG_STDRNG (0, default): the index stream of the reference's StdRng::seed_from_u64(seed)
                             * (base.rs:353, 386) bit for bit.  BDR_RNG_XOSHIRO256PP (1): north_star's "on-device xoshiro index
                             * generator" - one xoshiro256++ generator per batch lane in HBM (lane j seeded with outputs 4j .. 4j+3
                             * of SplitMix64(seed)), lane j draws sample j of every batch: ix = (next_u64() >> 32) % size.  NOT the
                             * reference's stream (no parity claim: a device-native alternative for hosts that do not need one);
                             * deterministic in (seed, the sequence of batch sizes).  Uniform sampling only. */
    int32_t reserved;
} bdr_replay_config;
#define BDR_RNG_STDRNG 0
#define BDR_RNG_XOSHIRO256PP 1

/* ReplayBufferBase::build (base.rs:336-356).  The ring lives in HBM as one fused record per
 * transition: [obs | next_obs | act | reward f32 | is_terminated i8 | is_truncated i8 | pad]. */
BDR_API int32_t bdr_replay_create(const bdr_replay_config* cfg, bdr_replay** out);
BDR_API int32_t bdr_replay_destroy(bdr_replay* r);
/* A VIEW of a ring: a read-only bdr_replay that borrows `owner`'s rows and carries its own ChaCha key - seed_from_u64(seed), as
 * bdr_replay_create derives it - stream position and batch buffers, so that P consumers of one dataset (a BC group's members, seeds of a
 * sweep) hold P index streams over ONE copy of the rows in HBM.  Creation synchronises the owner's stream once and takes capacity, size
 * and the layout as they are then; the view owns no ring memory and bdr_replay_destroy of a view frees none.
 * Owners: uniform StdRng rings without a frame store that are not empty; anything else is BDR_ERR_INVALID (BDR_ERR_EMPTY: an empty ring).
 * On a view every push, bdr_replay_fill_synthetic and bdr_replay_enable_per are BDR_ERR_INVALID; on the owner, while it has live views,
 * so are every push, fill, enable_per and bdr_replay_destroy, each naming the number of live views.  Without a view nothing about a
 * ring changes.  bdr_replay_batch, bdr_replay_sample_indices and an agent's opt on a view give bit for bit what they give on a separate
 * ring created with that seed and holding the same rows. */
BDR_API int32_t bdr_replay_view_create(bdr_replay* owner, uint64_t seed, bdr_replay** out);

/* ExperienceBufferBase::push (base.rs:295-316): n transitions, rows written at
 * (i+k) % capacity, i = (i+n) % capacity, size = min(size+n, capacity). Host pointers.  The call returns when the
 * caller's buffers are free (the rows sit in the buffer's pinned staging area); the copy into the ring completes on
 * the buffer's stream, in order before every later batch / read of this buffer. */
BDR_API int32_t bdr_replay_push(bdr_replay* r, uint64_t n, const void* obs, const void* act,
                                const void* next_obs, const float* reward,
                                const int8_t* is_terminated, const int8_t* is_truncated);

/* The same push for transitions whose observation rows already live in HBM - the frame stacks of a bdr_atari_prep (obs = its
 * stacks before the step, bdr_atari_prep_device_prev_stacks; next_obs = after it, bdr_atari_prep_device_stacks), or any device
 * rows `*_stride` bytes apart: trainer/sampler.rs:99-144 + border-atari-env/src/env.rs:197-209,312-324 without the HBM -> host ->
 * HBM round trip of the stacks.  act / reward / flags are host arrays (they come from the host side: exploration, the emulator).
 * Ring rows, cursor, size and PER priorities are exactly those of bdr_replay_push on the same bytes.  Not for frame_stack > 0
 * buffers (bdr_replay_push_device_frames is their device push): BDR_ERR_INVALID.  Returns when the rows have been copied. */
BDR_API int32_t bdr_replay_push_device(bdr_replay* r, uint64_t n, const void* obs_dev, uint64_t obs_stride, const void* act,
                                       const void* next_obs_dev, uint64_t next_obs_stride, const float* reward,
                                       const int8_t* is_terminated, const int8_t* is_truncated);

/* bdr_replay_push_device for a buffer with frame_stack > 0 (same arguments): the frames an incoming stack shares with the previous
 * next_obs, with its own transition and inside itself are found by comparing the rows in HBM (the previous next_obs is read from the
 * frame store), only the answers cross to the host, and the frames that are new are copied from the caller's rows into the store.
 * Ring records, cursor, size, PER priorities, bdr_replay_frames_used, the sharing state and every later batch / read are exactly
 * what bdr_replay_push leaves after the same bytes as host rows; host and device pushes may alternate on one buffer in any order.
 * BDR_ERR_INVALID before anything is written: frame_stack == 0; rows that are not device memory of the buffer's GPU; a stride
 * below the row size; a base address or stride that is not a multiple of 16 bytes.  A store that runs out of frames behaves as in
 * bdr_replay_push: the accepted prefix stays (cursor, size and priorities advance by it), BDR_ERR_INVALID, the buffer stays usable.
 * Returns when the caller's device rows may be overwritten. */
BDR_API int32_t bdr_replay_push_device_frames(bdr_replay* r, uint64_t n, const void* obs_dev, uint64_t obs_stride, const void* act,
                                              const void* next_obs_dev, uint64_t next_obs_stride, const float* reward,
                                              const int8_t* is_terminated, const int8_t* is_truncated);

/* ExperienceBufferBase::len (base.rs:318-320) and the write cursor `i`. */
BDR_API int32_t bdr_replay_len(const bdr_replay* r, uint64_t* len);
BDR_API int32_t bdr_replay_head(const bdr_replay* r, uint64_t* head);

/* Single-frame store only: frames allocated since creation (a continuing episode costs one per transition) and the store's
 * capacity in frames. */
BDR_API int32_t bdr_replay_frames_used(const bdr_replay* r, uint64_t* allocated, uint64_t* capacity);

/* The index draw of ReplayBufferBase::batch (base.rs:384-390):
 * ixs[k] = (StdRng::next_u32() as usize) % size, generated ON DEVICE by the ChaCha12 kernel
 * and copied back; advances the RNG exactly as one batch(n) call does. */
BDR_API int32_t bdr_replay_sample_indices(bdr_replay* r, uint64_t n, uint64_t* ixs_out);

/* ReplayBufferBase::batch (base.rs:376-402): draws indices and gathers the batch into
 * device-resident batch buffers owned by the replay handle (valid until the next batch()).
 * Any *_out host pointer may be NULL; non-NULL ones receive a copy (synchronises).
 * GenericTransitionBatch fields (generic_replay_buffer/batch.rs:89-162): obs, act, next_obs,
 * reward, is_terminated, is_truncated, ix_sample; weight is None (uniform sampling). */
BDR_API int32_t bdr_replay_batch(bdr_replay* r, uint64_t n, uint64_t* ixs_out, void* obs_out,
                                 void* act_out, void* next_obs_out, float* reward_out,
                                 int8_t* is_terminated_out, int8_t* is_truncated_out);

/* Device pointers of the last gathered batch (for callers that keep the batch on device). */
typedef struct {
    uint64_t n;
    const void* obs;      /* [n][obs_row_bytes] */
    const void* next_obs; /* [n][obs_row_bytes] */
    const void* act;      /* [n][act_row_bytes] */
    const float* reward;  /* [n] */
    const int8_t* is_terminated;
    const int8_t* is_truncated;
    const uint64_t* ixs;
    const float* weight;  /* [n] importance weights when PER is enabled, else NULL */
} bdr_device_batch;
BDR_API int32_t bdr_replay_last_batch(const bdr_replay* r, bdr_device_batch* out);

/* Benchmark helper (SURVEY.md section 8(d) synthetic inputs): fills transitions [0,n) on the
 * device from a counter-based generator (seed, transition index) and sets size=min(n,capacity),
 * i = n % capacity.  kind 0: Atari-like (u8 frames uniform 0..255, act uniform i64 in
 * [0,n_actions), reward in {-1,0,1} with P=(.05,.9,.05), P(term)=.005, trunc 0);
 * kind 1: f32 rows ~ N(0,1) approx (obs), act f32 ~ U(-1,1) (n_actions==0) or i64 uniform. */
BDR_API int32_t bdr_replay_fill_synthetic(bdr_replay* r, uint64_t n, uint64_t seed, int32_t kind,
                                          int32_t n_actions);
/* Test helper: copy ring rows [first, first+n) back to the host (any pointer may be NULL). */
BDR_API int32_t bdr_replay_read_rows(bdr_replay* r, uint64_t first, uint64_t n, void* obs, void* act,
                                     void* next_obs, float* reward, int8_t* term, int8_t* trunc);

/* ------------------------------------------------------------------------------------------
 * Episode datasets and observation normalisation  (border-minari/src/dataset.rs:64-109 MinariDataset::create_replay_buffer,
 * border-minari/src/d4rl/pen/candle.rs:42-161 PenConverter)
 * ---------------------------------------------------------------------------------------- */
#define BDR_DTYPE_F32 0
#define BDR_DTYPE_F64 1          /* Minari stores observations as float64 (pyobj_to_arrayd::<f64, f32>, border-minari/src/util.rs) */

/* PenConverter's per-column mean / std (pen/candle.rs:42-69) and the normalisation it applies to every observation, in the
 * replay buffer (:104-124) and at acting time (:83-87).  Element contract, for every input dtype: a float64 element is first
 * rounded to f32 (round to nearest even, Rust's `as f32`), then z = (x - mean) / std in f32 - two separately rounded operations,
 * the division correctly rounded (ndarray's `(&obs.0 - &self.mean) / &self.std`, :71-74).  The host path and the device kernels
 * give the same bits: those of numpy's (x.astype(float32) - mean32) / std32. */
typedef struct bdr_obs_norm bdr_obs_norm;
BDR_API int32_t bdr_obs_norm_create(int32_t device, uint64_t dim, bdr_obs_norm** out);
BDR_API int32_t bdr_obs_norm_destroy(bdr_obs_norm* h);
/* Statistics (pen/candle.rs:48-66): the caller passes the rows that count - the reference drops the last row of every episode
 * before it concatenates (:56, :146-152).  rows: host [n_rows][dim] of `dtype`.  Accumulation runs on the device in float64 over
 * the f32-rounded elements, in a fixed order (count / mean / M2 per block of 64 rows, blocks merged in row order: Chan et al.),
 * so the same sequence of calls gives the same bits.  finish: mean = sum / n, std = sqrt(sum (x - mean)^2 / (n - 1))
 * (`std_axis(Axis(0), 1.0)`), each rounded to f32 once.  The statement of record is "the float64 result, rounded": the reference
 * accumulates in f32 in ndarray's own order.  finish fails with BDR_ERR_INVALID when n < 2 or when a column's std is zero or not
 * finite (the message names the first such column; the reference would fill the buffer with NaN).  accumulate after finish or
 * after set: BDR_ERR_INVALID. */
BDR_API int32_t bdr_obs_norm_accumulate(bdr_obs_norm* h, uint64_t n_rows, const void* rows, int32_t dtype);
BDR_API int32_t bdr_obs_norm_finish(bdr_obs_norm* h);
/* Statistics computed elsewhere (a saved converter): dim floats each; a zero or non-finite std is BDR_ERR_INVALID.  get: the
 * statistics in use and the number of rows they were computed from (0 after set); any pointer may be NULL. */
BDR_API int32_t bdr_obs_norm_set(bdr_obs_norm* h, const float* mean, const float* std);
BDR_API int32_t bdr_obs_norm_get(const bdr_obs_norm* h, float* mean_out, float* std_out, uint64_t* count_out);
/* convert_observation (pen/candle.rs:83-87): n rows of `dtype` -> normalised f32 rows.  apply: host [n][dim] -> host [n][dim],
 * computed on the host.  apply_device: rows in HBM of the normaliser's GPU, row k at rows_dev + k * row_stride bytes, written to
 * out_dev + k * out_stride bytes - what bdr_*_sample_device takes, so an observation that lives on the device is normalised there. */
BDR_API int32_t bdr_obs_norm_apply(const bdr_obs_norm* h, uint64_t n, const void* rows, int32_t dtype, float* out);
BDR_API int32_t bdr_obs_norm_apply_device(const bdr_obs_norm* h, uint64_t n, const void* rows_dev, uint64_t row_stride,
                                          int32_t dtype, float* out_dev, uint64_t out_stride);

/* One episode into the ring (dataset.rs:80-100 + pen/candle.rs:104-161): `observations` is host [T+1][dim] of `obs_dtype`, the
 * other arrays have T rows.  By definition the result is that of
 *   bdr_replay_push(r, T, N(observations[0:T]), act, N(observations[1:T+1]), reward, is_terminated, is_truncated)
 * with N = the normaliser's element contract (norm == NULL: the conversion to f32 alone) - ring bytes, cursor, size and PER
 * priorities are identical; T may need several staging passes and may wrap the ring.  It differs in cost only: the T+1 raw rows
 * cross PCIe once, in their own dtype, and a kernel converts, normalises and writes both halves of every record; no normalised
 * copy exists on the host.  The ring's rows must be f32 (dim * 4 == obs_row_bytes), `norm` of the same dim and device; a
 * frame_stack > 0 ring is refused (BDR_ERR_INVALID); T == 0 is a no-op.  Returns when the caller's arrays are free. */
BDR_API int32_t bdr_replay_push_episode(bdr_replay* r, uint64_t T, const void* observations, int32_t obs_dtype,
                                        const void* act, const float* reward, const int8_t* is_terminated,
                                        const int8_t* is_truncated, const bdr_obs_norm* norm);

/* num_terminated_flags / num_truncated_flags / sum_rewards (generic_replay_buffer/base.rs:243-267) over rows [0, len): the counts
 * are exact, sum_rewards is the LEFT-TO-RIGHT f32 sum (`Iterator::sum` is a sequential fold, :265) - the order is the contract. */
typedef struct { uint64_t n_terminated, n_truncated; float sum_rewards; int32_t reserved; } bdr_replay_summary;
BDR_API int32_t bdr_replay_summarize(bdr_replay* r, bdr_replay_summary* out);

/* ------------------------------------------------------------------------------------------
 * Prioritized experience replay  (SimpleReplayBufferConfig::per_config, config.rs:45-83;
 * generic_replay_buffer/base/sum_tree.rs; base/iw_scheduler.rs)
 * ---------------------------------------------------------------------------------------- */
enum { BDR_PER_NORMALIZE_ALL = 0, BDR_PER_NORMALIZE_BATCH = 1 };   /* WeightNormalizer, sum_tree.rs:13-18 */
typedef struct {
    float alpha;            /* 0.6   (config.rs:76) */
    float beta_0;           /* 0.4 */
    float beta_final;       /* 1.0 */
    uint64_t n_opts_final;  /* 500_000 */
    int32_t normalize;      /* BDR_PER_NORMALIZE_ALL */
    int32_t reserved;
} bdr_per_config;
BDR_API void bdr_per_config_default(bdr_per_config* c);

/* SimpleReplayBuffer::build with per_config: Some(..) (base.rs:336-356).  Must be called on an empty
 * buffer.  From then on push() gives new rows the current maximum priority (set_priority, :227-235),
 * batch() samples through the sum tree and carries importance weights (:377-383), and agents that
 * consume weights (DQN, dqn/base.rs:123-145) call update_priority with their TD errors. */
BDR_API int32_t bdr_replay_enable_per(bdr_replay* r, const bdr_per_config* c);

/* ReplayBufferBase::update_priority (base.rs:413-426): sum_tree.update(ix, td_err) in order, then the
 * importance-weight schedule advances by one optimisation step.  Host arrays. */
BDR_API int32_t bdr_replay_update_priority(bdr_replay* r, uint64_t n, const uint64_t* ixs, const float* td_errs);

/* `weight` of the last batch() (Some(ws), base.rs:382): n floats.  Error when PER is not enabled. */
BDR_API int32_t bdr_replay_batch_weights(bdr_replay* r, uint64_t n, float* w_out);

/* Introspection for parity tests: scheduler state, SumTree::{total,max}, the raw arrays
 * (what: 0 sum tree [2*capacity-1] in the reference's layout, 1 {min over [0,n_samples), max} as two floats), SumTree::get. */
typedef struct { uint64_t n_samples, n_opts; float beta, total, max_p, min_p; } bdr_per_info;
BDR_API int32_t bdr_replay_per_info(bdr_replay* r, bdr_per_info* out);
BDR_API int32_t bdr_replay_per_read(bdr_replay* r, int32_t what, float* out, uint64_t n);
BDR_API int32_t bdr_replay_per_get(bdr_replay* r, float s, uint64_t* ix);

/* ------------------------------------------------------------------------------------------
 * DQN agent  (border-tch-agent/src/dqn/base.rs, dqn/config.rs:26-48, dqn/model/base.rs)
 * ---------------------------------------------------------------------------------------- */

enum { BDR_NET_ATARI_CNN = 0, BDR_NET_MLP = 1 };
enum { BDR_LOSS_MSE = 0, BDR_LOSS_SMOOTH_L1 = 1 };        /* util.rs:17-23 CriticLoss      */
enum { BDR_OPT_ADAM = 0, BDR_OPT_ADAMW = 1 };             /* opt.rs:13-28 OptimizerConfig  */
#define BDR_MAX_UNITS 8

/* Which products the large matrix layers of an agent compute.  NOT a reference field: the reference has one arithmetic (f32
 * products, f32 accumulation in ATen's summation order).  Both settings accumulate in f32 and sit inside the 1e-4 parity bar:
 *   BDR_ARITH_BF16X3_6   (default) every f32 operand of conv2 / conv3 forward (DQN) and of the merge / cosine-embedding layers
 *                        (IQN at C4-sized shapes) is split, round-to-nearest, into three bf16 terms (a = a0 + a1 + a2 exactly up to
 *                        the last bit) and six of the nine partial products run on the bf16 MFMA; the three dropped products are
 *                        <= 2^-24 relative per product, zero-mean.  Every other layer, every gradient and the n <= 8 acting
 *                        kernels compute exact f32 products.
 *   BDR_ARITH_F32_EXACT  every product is an f32 x f32 product on the FP32 MFMA (v_mfma_f32_32x32x2_f32).
 * The environment variables BDR_DQN_F32_EXACT / BDR_IQN_F32_EXACT (=1 exact, =0 split) override the field for A/B runs only. */
enum { BDR_ARITH_BF16X3_6 = 0, BDR_ARITH_F32_EXACT = 1 };

/* OptimizerConfig's AdamW variant (opt.rs:20-27, 38-55) beside a model's `lr`: opt_kind BDR_OPT_ADAM ignores every other field
 * (tch nn::Adam::default(): .9, .999, 1e-8, wd 0); amsgrad keeps a max_exp_avg_sq arena (parameter model +400 / arena 5). */
typedef struct {
    int32_t opt_kind; /* BDR_OPT_* */
    int32_t amsgrad;
    double beta1, beta2, weight_decay, eps;
} bdr_adamw_config;

/* AtariCnnConfig (cnn/config.rs:13-18) / MlpConfig (mlp/config.rs:7-12) */
typedef struct {
    int32_t kind;    /* BDR_NET_* */
    int32_t n_stack; /* cnn */
    int32_t in_dim;  /* mlp */
    int32_t n_units; /* mlp */
    int32_t units[BDR_MAX_UNITS];
    int32_t out_dim; /* number of actions */
    int32_t activation_out;
} bdr_net_config;

/* DqnConfig (dqn/config.rs:26-48; defaults :82-102) + DqnModelConfig.opt_config. */
typedef struct {
    bdr_net_config net;
    int32_t opt_kind; /* BDR_OPT_ADAM: lr only (tch nn::Adam::default(): .9,.999,1e-8,wd 0) */
    double lr;
    double beta1, beta2, weight_decay, eps; /* AdamW variant only */
    int32_t amsgrad;  /* AdamW{amsgrad} (opt.rs:20-27): denominator from the running max of exp_avg_sq (arena 5) */
    uint64_t soft_update_interval;
    uint64_t n_updates_per_opt;
    uint64_t batch_size;
    double discount_factor;
    double tau;
    int32_t train;
    int32_t double_dqn;
    int32_t critic_loss; /* BDR_LOSS_* */
    int32_t has_clip_td_err;
    double clip_td_err_min, clip_td_err_max;
    int32_t record_verbose_level;
    int32_t device; /* HIP device ordinal ("No device is given for DQN agent": dqn/base.rs:256) */
    uint64_t param_seed; /* seed of the library's own uniform(+-1/sqrt(fan_in)) initialiser */
    int32_t arithmetic;  /* BDR_ARITH_* (AtariCnn only; an Mlp Q-network always computes exact f32 products) */
    int32_t reserved;
} bdr_dqn_config;

BDR_API void bdr_dqn_config_default(bdr_dqn_config* cfg); /* dqn/config.rs:82-102 */

/* Configurable::build (dqn/base.rs:252-286). */
BDR_API int32_t bdr_dqn_create(const bdr_dqn_config* cfg, bdr_agent** out);
BDR_API int32_t bdr_agent_destroy(bdr_agent* a);

/* Agent::train / eval / is_train (dqn/base.rs:289-299). */
BDR_API int32_t bdr_agent_set_train(bdr_agent* a, int32_t train);
BDR_API int32_t bdr_agent_is_train(const bdr_agent* a, int32_t* out);

/* Agent::opt (border-core/src/base/agent.rs:62-64 -> dqn/base.rs:301-309 -> opt_ :182-200):
 * n_updates_per_opt x update_critic, soft-update bookkeeping, n_opts += 1.
 * Enqueues on the agent's stream and returns WITHOUT synchronising. */
BDR_API int32_t bdr_agent_opt(bdr_agent* a, bdr_replay* buffer);

/* Agent::opt_with_record (dqn/base.rs:311-343): same step, then synchronises and returns
 * the Record scalars.  keys: "loss" (always); verbose>=2 adds pred_mean, reward_mean,
 * tgt_mean, tgt_minus_pred_mean. */
typedef struct {
    float loss;
    float pred_mean, reward_mean, tgt_mean, tgt_minus_pred_mean;
    int32_t has_verbose;
} bdr_dqn_record;
BDR_API int32_t bdr_agent_opt_with_record(bdr_agent* a, bdr_replay* buffer, bdr_dqn_record* rec);

/* Agent::opt_with_record for any agent kind: the Record scalars in the agent's documented order
 * (DQN: loss[, pred_mean, reward_mean, tgt_mean, tgt_minus_pred_mean]; IQN: loss_critic;
 * SAC: loss_critic, loss_actor, ent_coef).  Synchronises. */
BDR_API int32_t bdr_agent_opt_with_scalars(bdr_agent* a, bdr_replay* buffer, float* out, int32_t cap, int32_t* n_out);

/* Names of the scalars bdr_agent_opt_with_scalars returns, '\n'-separated, in order (the keys of the reference's Record):
 *   DQN  "loss"; record_verbose_level >= 2 adds pred_mean, reward_mean, tgt_mean, tgt_minus_pred_mean (dqn/base.rs:107-121),
 *        then qnet.param_stats() - "<var>_mean", "<var>_std" (population) for c1.weight ... l2.bias / mlp.ln{i}.* in the
 *        variables' order (util.rs:64-80) - and "ratio_best_act" = n_samples_best_act / n_samples_act, which resets both
 *        counters (dqn/base.rs:316-342);
 *   IQN  "loss_critic" (iqn/base.rs:190);   SAC  "loss_critic", "loss_actor", "ent_coef" (sac/base.rs:187-196);
 *   IQL  "loss_value", "loss_critic", "loss_actor", each averaged over n_updates_per_opt (iql/base.rs:177-185);
 *   AWAC "loss_critic", "loss_actor", "q_tgt_abs_mean", "adv_mean", "adv_abs_mean" averaged over n_updates_per_opt, then
 *        "logp_mean", "reward_mean", "next_q_mean" summed over them (awac/base.rs:197-212). */
BDR_API int32_t bdr_agent_record_keys(bdr_agent* a, char* names_out, uint64_t names_cap, int32_t* n_keys);

/* Test helper: n draws of the agent's own device noise stream copied to the host - SAC: the N(0,1) draws of action_logp
 * (sac/base.rs:76 uses torch's global generator), IQN: the U[0,1) percent points of IqnSample::Uniform* (iqn/model/base.rs:365-368).
 * Counter-based (seed, running counter): advances the stream exactly as an update consuming n draws does. */
BDR_API int32_t bdr_agent_draw_noise(bdr_agent* a, uint64_t n, float* out);

/* One update_critic on a caller-supplied host minibatch (parity tests: "fixed minibatch").
 * act: int64 [n]; obs/next_obs rows as in the replay buffer. */
BDR_API int32_t bdr_dqn_update_on_batch(bdr_agent* a, uint64_t n, const void* obs, const int64_t* act,
                                        const void* next_obs, const float* reward,
                                        const int8_t* is_terminated, bdr_dqn_record* rec);

/* The `if let Some(ws) = weight` branch of update_critic (dqn/base.rs:123-145) on a caller-supplied minibatch:
 * weight[n] importance weights (NULL = the unweighted branch); td_errs_out[n] (optional) receives
 * |pred - tgt| (clipped by clip_td_err), the values the reference hands to update_priority. */
BDR_API int32_t bdr_dqn_update_on_batch_weighted(bdr_agent* a, uint64_t n, const void* obs, const int64_t* act,
                                                 const void* next_obs, const float* reward, const int8_t* is_terminated,
                                                 const float* weight, float* td_errs_out, bdr_dqn_record* rec);

/* Split step (synchronous data-parallel training): bdr_dqn_grads_on_batch = update_critic up to
 * `loss.backward()` (dqn/base.rs:60-150, opt.rs:74-83 without `step`) on a host minibatch - gradients land in arena 4
 * (bdr_agent_get_params / set_params), parameters, Adam moments and counters are untouched; bdr_agent_apply_grads = the
 * optimizer step on whatever arena 4 holds, then opt_'s bookkeeping (soft-update counter, n_opts).  N ranks that each take the
 * gradient of B/N rows, average the arenas and apply take exactly the step one rank takes on the B rows. */
BDR_API int32_t bdr_dqn_grads_on_batch(bdr_agent* a, uint64_t n, const void* obs, const int64_t* act, const void* next_obs,
                                       const float* reward, const int8_t* is_terminated, bdr_dqn_record* rec);
BDR_API int32_t bdr_agent_apply_grads(bdr_agent* a);

/* Q(obs) for n observations -> q_out[n][A] and argmax actions (either pointer may be NULL).
 * DQN: qnet.forward (dqn/base.rs:213); IQN: quantile average (iqn/base.rs:209-215). */
BDR_API int32_t bdr_agent_qvalues(bdr_agent* a, uint64_t n, const void* obs, float* q_out,
                                  int64_t* argmax_out);

/* DqnExplorer / IqnExplorer (dqn/explorer.rs:8-15, iqn/explorer.rs:9-16) with its mutable state.
 * The reference draws from fastrand's global unseeded generator; this library draws from a seeded
 * ChaCha12 stream (StdRng::seed_from_u64(seed)), so action sequences are reproducible:
 *   eps-greedy call:  eps = max(eps_start - (eps_start-eps_final)/final_step * n_calls, eps_final);
 *                     coin = f64 (one u64 of the stream, top 52 bits); n_calls += 1;
 *                     coin < eps ? n_procs x below(A) (one draw each, row order) : argmax per row
 *   softmax call:     per row one f64 u, action = first k with cumsum(softmax(q))[k] > u
 *   eval (DQN only):  f32 (one u32, top 23 bits) < 0.01 ? one below(A) for every row : argmax   */
enum { BDR_EXPLORER_SOFTMAX = 0, BDR_EXPLORER_EPS_GREEDY = 1 };
typedef struct {
    int32_t kind;          /* BDR_EXPLORER_* */
    double eps_start;      /* 1.0  (explorer.rs:47) */
    double eps_final;      /* 0.02 */
    uint64_t final_step;   /* 100_000; dqn_atari: 1_000_000 */
    uint64_t n_calls;      /* the reference's `n_opts` field of EpsilonGreedy: action() calls so far */
    uint64_t seed;         /* seed of the exploration stream (set_explorer rewinds the stream) */
} bdr_explorer_config;
BDR_API void bdr_explorer_config_default(bdr_explorer_config* e, int32_t kind);
BDR_API int32_t bdr_agent_set_explorer(bdr_agent* a, const bdr_explorer_config* e);
BDR_API int32_t bdr_agent_get_explorer(const bdr_agent* a, bdr_explorer_config* e);

/* Policy::sample (dqn/base.rs:211-242, iqn/base.rs:204-228) for n_procs observations (host rows as in the
 * replay buffer): device forward, exploration as configured, act_out[n_procs] (int64).
 * train: n_samples_act += 1 (and n_samples_best_act += 1 when every row took its greedy action, the
 * reference's `record_verbose_level >= 2` bookkeeping).  info may be NULL.
 * ONE network, two kernel families (AtariCnn DQN / IQN): calls with n_procs <= 8 run the acting kernels (csrc/act_small.hpp: exact f32
 * products from the f32 weights, k-sliced 32 x 32 tiles), larger calls the training forward (conv2 / conv3 with the agent's
 * `arithmetic`).  The two evaluate the same function to f32 round-off - Q-values within 5e-6 of the largest |Q| with BDR_ARITH_BF16X3_6,
 * 1e-6 with BDR_ARITH_F32_EXACT (tests/test_gpu_sample.py) - but not bit for bit: the greedy action of a row is the same on both
 * whenever its two leading Q-values differ by more than 2e-5 of the largest |Q|; below that distance it may depend on how many
 * environments share the call (8 vs 9).  Exact ties (equal rows of the output layer) resolve to the first maximum on both.  The
 * reference has the same property across batch sizes (ATen picks its GEMM blocking by shape); a caller that needs one family for
 * every n sets BDR_NO_ACT_SMALL=1 (training forward always, ~2x the one-observation latency). */
typedef struct {
    double eps;            /* eps used by this call (eps-greedy), else 0 */
    int32_t is_random;     /* the call took the random branch */
    uint64_t n_samples_act, n_samples_best_act;
} bdr_sample_info;
BDR_API int32_t bdr_agent_sample(bdr_agent* a, uint64_t n_procs, const void* obs, int64_t* act_out,
                                 bdr_sample_info* info);
/* Policy::sample for observations that are already on the device (trainer/sampler.rs:99-144 with the
 * observation of border-atari-env/src/env.rs:197-209 kept in HBM): row i at obs_dev + i * row_stride bytes, e.g.
 * bdr_atari_prep_device_stacks with row_stride = 4*84*84.  Forward, exploration stream, counters and results are those of
 * bdr_agent_sample on the same bytes; contiguous rows are read in place.  The rows must be complete when the call is made and
 * stay untouched until it returns.  bdr_agent_qvalues_device: the action values themselves (bdr_agent_qvalues). */
BDR_API int32_t bdr_agent_sample_device(bdr_agent* a, uint64_t n_procs, const void* obs_dev, uint64_t row_stride, int64_t* act_out,
                                        bdr_sample_info* info);
BDR_API int32_t bdr_agent_qvalues_device(bdr_agent* a, uint64_t n, const void* obs_dev, uint64_t row_stride, float* q_out,
                                         int64_t* argmax_out);

/* Block until everything enqueued on the agent's stream has finished.  Device-side error flags raised since the last check
 * (an action index outside [0, n_actions) in a TD step, a NaN priority in update_priority, a timed-out cross-queue gate) are
 * reported here - and by every other entry point that synchronises (opt_with_record / _with_scalars, get_params, save_params,
 * sample, update_on_batch); bdr_agent_opt polls them without synchronising every 256 calls. */
BDR_API int32_t bdr_agent_sync(bdr_agent* a);
BDR_API int32_t bdr_agent_n_opts(const bdr_agent* a, uint64_t* n);

/* ---- A group of small DQN agents stepped in one launch -----------------------------------------------------------------
 * A launch grouping, not an agent kind: n Mlp DQN agents (bdr_dqn_create with BDR_NET_MLP) whose Agent::opt
 * (border-core/src/base/agent.rs:62-64 -> dqn/base.rs:301-309) runs as ONE kernel launch per update round, one workgroup per member,
 * and whose Policy::sample (dqn/base.rs:211-242) runs as one launch for all of them.  Every result - parameters, target
 * parameters, Adam moments, gradients, the rings' index streams and batch arrays, records, counters, action sequences - is bit for
 * bit what stepping the same agents one after the other gives.
 * bdr_agent_group_create ADOPTS the agents: each member's own stream is synchronised and destroyed and the member enqueues on the
 * group's stream from then on, so every bdr_agent_* call keeps working on a member (bdr_agent_group_member), means what it
 * meant, and stays ordered with the group's calls.  The group owns its members: bdr_agent_group_destroy destroys them, and
 * bdr_agent_destroy on a member of a live group is BDR_ERR_INVALID.
 * Eligible (otherwise BDR_ERR_INVALID naming the member and the reason): every member is an Mlp DQN agent that takes the
 * one-workgroup step for its batch size (no layer wider than 256, at most 4 layers, batch <= 128, every phase at most 8
 * 32x32 blocks - Mlp[64, 64] up to batch 64), all on one device, no amsgrad, no gradient communicator, profiling off, and one
 * n_updates_per_opt for all.  Widths, depth, in_dim, actions, batch size, loss, double DQN, gamma, tau, soft_update_interval,
 * optimizer and its scalars and the seeds may differ per member. */
typedef struct bdr_agent_group bdr_agent_group;
BDR_API int32_t bdr_agent_group_create(bdr_agent* const* agents, uint32_t n, bdr_agent_group** out);
BDR_API int32_t bdr_agent_group_destroy(bdr_agent_group* g);
BDR_API int32_t bdr_agent_group_size(const bdr_agent_group* g, uint32_t* n);
BDR_API int32_t bdr_agent_group_member(const bdr_agent_group* g, uint32_t i, bdr_agent** out);
/* The two forms of a group.  bdr_agent_group_create takes the form of member 0:
 *   BDR_GROUP_FORM_ONE_WORKGROUP  every member takes the one-workgroup step (the rules above): one launch per update round;
 *   BDR_GROUP_FORM_LAYERS         NO member takes it and every member steps on the latency-shaped layer path (Mlp[256, 256] at batch
 *                                 64 - the reference's dqn_cartpole - and every net between it and Mlp[64, 64]): one update round is
 *                                 the launch sequence Dqn::update_critic (dqn/base.rs:60-160) takes for ONE such member - gather, pack,
 *                                 the forward layers, TD + loss, the input gradients, the grouped weight gradient, reduce + Adam with
 *                                 the soft update - each launch serving all members (11 launches for dqn_cartpole, whatever n is).
 * Layer form, further conditions (otherwise BDR_ERR_INVALID naming the member and the reason, before anybody is adopted): no layer
 * wider than 256 (padded), at most 4 layers, the layer path switched on (no BDR_NO_SMALL_GEMM), no amsgrad, no gradient
 * communicator, profiling off, one n_updates_per_opt, and ONE shape for all members: in_dim, units, out_dim, activation_out,
 * batch_size, double_dqn.  Optimizer and its scalars, loss, clip_td_err, gamma, tau, soft_update_interval and the seeds may differ.
 * A group mixing the two forms is refused, naming the first member whose form differs from member 0's.  Prioritized rings under a
 * layer-form group are refused: bdr_agent_group_set_prioritized(g, 1) on it, and a prioritized buffer handed to _opt / _push.
 * Every result is bit for bit what bdr_agent_opt on the same agents standalone gives, in both forms.
 * bdr_agent_group_info (no trait method: the launch grouping is this library's, Agent::opt - border-core/src/base/agent.rs:62-64 - is
 * what it groups): the form, the kernel launches one update round enqueues on uniform rings, and a running count of the kernel
 * launches the group's own calls (opt, push, sample, qvalues, evaluate, the compiled loop) have enqueued since it was created. */
#define BDR_GROUP_FORM_ONE_WORKGROUP 0
#define BDR_GROUP_FORM_LAYERS 1
#define BDR_GROUP_FORM_BC_LAYERS 2   /* a bdr_bc_group (below): BC's launch sequence of one member, every launch serving all members */
#define BDR_GROUP_FORM_IQL_LAYERS 3  /* a bdr_iql_group (below): IQL's launch sequence of one member, every launch serving all members */
#define BDR_GROUP_FORM_AWAC_LAYERS 4 /* a bdr_awac_group (below): AWAC's launch sequence of one member, every launch serving all members */
#define BDR_GROUP_FORM_CANDLE_SAC_LAYERS 5 /* a bdr_candle_sac_group (below): the candle SAC's launch sequence of one member, every launch serving all members */
#define BDR_GROUP_FORM_CANDLE_DQN_LAYERS 6 /* a bdr_candle_dqn_group (below): the candle DQN's launch sequence of one member, every launch serving all members */
typedef struct { int32_t form; uint32_t n_members; uint32_t launches_per_round; uint32_t reserved; uint64_t kernel_launches; } bdr_group_info;
BDR_API int32_t bdr_agent_group_info(const bdr_agent_group* g, bdr_group_info* out);
/* Prioritized replay under the group (on = 1; 0, the default, refuses every prioritized ring in _opt and _push as before).  A group
 * switched on steps and feeds rings with bdr_replay_enable_per: every prioritized member's SumTree::sample, importance weights and
 * row gather are one launch for all of them ahead of the step, update_priority one launch behind it, and set_priority of a grouped
 * push one launch behind the push - a fixed number of launches per round and per push whatever n is, no copy command, no
 * synchronisation.  Members may be mixed; a uniform member keeps the in-step sample.  Every ring ends up bit for bit as the
 * standalone calls leave it: rows, head, size, index stream, weights, the whole f32 sum tree, n_samples, n_opts, beta.  A NaN TD
 * error does what it does standalone (the update is dropped) and is reported, naming the member, as a deferred BDR_ERR_INVALID by
 * bdr_agent_group_sync / _sample.  A group switched on that is given uniform rings only enqueues exactly what the default one does. */
BDR_API int32_t bdr_agent_group_set_prioritized(bdr_agent_group* g, int32_t on);
/* Agent::opt of every member, member i on buffers[i] (n distinct buffers): n_updates_per_opt launches in all, asynchronous.
 * Every buffer must be what the one-launch step samples itself - a uniform (non-prioritized) ring with the StdRng index stream,
 * no single-frame store, f32 rows of the member's input width, on the group's device, not empty - or, once
 * bdr_agent_group_set_prioritized(g, 1) was called, a prioritized ring of that shape (at most four more launches per update round,
 * see there).  All buffers are checked BEFORE anything advances or is enqueued: a refused call leaves every member and every ring
 * exactly where it was. */
BDR_API int32_t bdr_agent_group_opt(bdr_agent_group* g, bdr_replay* const* buffers);
/* Agent::opt_with_record (dqn/base.rs:311-343) of every member: the same step, ONE synchronisation, then member i's Record scalars
 * (bdr_agent_opt_with_scalars' order) in out[i * cap_per_member ...] and their count in n_out[i]. */
BDR_API int32_t bdr_agent_group_opt_with_scalars(bdr_agent_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member,
                                                 int32_t* n_out);
/* qnet.forward (dqn/base.rs:213) of ONE host observation row per member, one launch: obs[i] -> q_out[i][A_i], the bits of
 * bdr_agent_qvalues(member i, 1, obs[i]). */
BDR_API int32_t bdr_agent_group_qvalues(bdr_agent_group* g, const void* const* obs, float* const* q_out);
/* Policy::sample (dqn/base.rs:211-242) of every member on one observation row each: one launch, then each member's own
 * exploration stream and counters exactly as bdr_agent_sample(member i, 1, obs[i]) advances them.  act_out[n]; info[n] or NULL. */
BDR_API int32_t bdr_agent_group_sample(bdr_agent_group* g, const void* const* obs, int64_t* act_out, bdr_sample_info* info);
/* Policy::sample of the members members[0..n) (strictly ascending indices) on one observation row each: one launch of n
 * workgroups.  obs / act_out / info are indexed by MEMBER ([group size]); only the selected entries are read / written.
 * A member that is not selected is not touched at all: its explorer stream, n_samples_act / n_samples_best_act, pinned error
 * mirror and last_replay_uid stay where they were.  For a selected member the call is bdr_agent_group_sample's, bit for bit.
 * Refused with BDR_ERR_INVALID before anything moves when n == 0, an index is >= the group's size, the list is not strictly
 * ascending, or a selected member's row is NULL.  With every member selected it enqueues what bdr_agent_group_sample enqueues. */
BDR_API int32_t bdr_agent_group_sample_members(bdr_agent_group* g, const uint32_t* members, uint32_t n, const void* const* obs,
                                               int64_t* act_out, bdr_sample_info* info);
/* ExperienceBufferBase::push (generic_replay_buffer/base.rs:287-313) of ONE transition per member, member i's into buffers[i] at its
 * head: one launch on the group's stream and no copy command, whatever n is.  obs[i] / next_obs[i] are host rows of the member's
 * input width; act[n] (i64), reward[n] and the flags [n] are host arrays, free again when the call returns.  Each ring ends up
 * exactly as bdr_replay_push(buffers[i], 1, ...) leaves it: the same bytes in the same row, the head advanced by one, the size
 * saturating at capacity.  The group's own later calls (opt, a member's bdr_agent_opt) are ordered behind the push by their queue;
 * calls on a ring's own stream (bdr_replay_push, _batch, _read_rows, _summarize) order themselves behind it through the ring's event.
 * Refused with BDR_ERR_INVALID before anything moves - every ring's head, size and index stream stay where they were - when a buffer
 * or a row pointer is NULL, a ring lives on another device, is prioritized (its sum tree is updated by bdr_replay_push) and the
 * group was not switched on by bdr_agent_group_set_prioritized (switched on: set_priority(1) of every prioritized ring - the
 * current maximum priority at the head row - rides behind the push, one or two launches for all of them), is a
 * single-frame store, its row width differs from the member's in_dim, act_row_bytes != 8, or two members share one ring. */
BDR_API int32_t bdr_agent_group_push(bdr_agent_group* g, bdr_replay* const* buffers, const void* const* obs, const int64_t* act,
                                     const void* const* next_obs, const float* reward, const int8_t* is_terminated,
                                     const int8_t* is_truncated);
/* bdr_agent_sync for the group's stream; reports every member's device-side error flags. */
BDR_API int32_t bdr_agent_group_sync(bdr_agent_group* g);

/* SyncModel::model_info / sync_model (border-async-trainer/src/sync_model.rs:2-13,
 * dqn/base.rs:377-402) and checkpoint access.  Parameters cross the boundary in the
 * reference's variable order and layouts (c1.weight OIHW, c1.bias, ... l2.bias / mlp.ln{i}.*).
 * which: 0 = qnet, 1 = qnet_tgt, 2 = Adam exp_avg, 3 = Adam exp_avg_sq, 4 = last gradient, 5 = AdamW amsgrad max_exp_avg_sq. */
BDR_API int32_t bdr_agent_param_count(const bdr_agent* a, uint64_t* n);
BDR_API int32_t bdr_agent_param_count_of(bdr_agent* a, int32_t which, uint64_t* n); /* per-model counts (SAC) */
BDR_API int32_t bdr_agent_get_params(bdr_agent* a, int32_t which, float* out, uint64_t n);
BDR_API int32_t bdr_agent_set_params(bdr_agent* a, int32_t which, const float* in, uint64_t n);

/* Device address of a flat parameter arena (internal kernel layout, identical on every rank) so a
 * host that already owns a communicator (e.g. torch.distributed) can reduce it in place.
 * Cost: from this call on the library cannot know when arena `which` is written, so every copy it derives from those parameters
 * (AtariCnn DQN: the bf16 planes of W2 / W3 the split-operand forward reads) is rebuilt before EVERY forward of that parameter set
 * (one ~4 us launch per forward) - until bdr_agent_arena_release(a, which) hands the arena back. */
BDR_API int32_t bdr_agent_arena_device_ptr(bdr_agent* a, int32_t which, void** ptr, uint64_t* n_floats);
/* "I no longer write through the pointer bdr_agent_arena_device_ptr gave me": derived copies are rebuilt once more and trusted again. */
BDR_API int32_t bdr_agent_arena_release(bdr_agent* a, int32_t which);

/* Agent::save_params / load_params (dqn/base.rs:345-371; iqn/base.rs:303-317; sac/base.rs:313-345): writes / reads
 * `qnet.pt.tch`, `qnet_tgt.pt.tch` (IQN: iqn, iqn_tgt; SAC: pi, qnet_{i}, qnet_tgt_{i}, ent_coef) under dir - the
 * reference's file names.  IQL (iql/base.rs:292-309): `actor.pt`, `critic.pt`, `critic.tgt.pt`, `value.pt` - candle VarMaps, which
 * are safetensors whatever the extension, so BDR_CKPT_TCH writes safetensors there and BDR_CKPT_SAFETENSORS `<stem>.safetensors`;
 * critic.tgt.pt holds the ONLINE critics and loading reads both critic files into the online critics, leaving the targets
 * untouched (util/critic.rs:272-298).  AWAC (awac/base.rs:311-333): `actor.pt`, `critic.pt`, `critic.tgt.pt`, with the same
 * containers and both critic.tgt quirks.  The container follows the file name exactly as tch's VarStore::{save,load} do:
 *   BDR_CKPT_TCH          "<stem>.pt.tch": the libtorch named-tensor archive (TorchScript module zip) that tch writes
 *                         through torch-sys at_save_multi and reads with torch::jit::load (default, = the reference);
 *   BDR_CKPT_SAFETENSORS  "<stem>.safetensors".
 * Both hold the reference's variable names in the reference's layouts (OIHW conv weights, [out,in] linear weights).
 * Loading prefers the configured container and falls back to the other one when only that file exists; it requires
 * every variable of the model with its shape and dtype float32; extra entries are ignored. */
#define BDR_CKPT_TCH 0
#define BDR_CKPT_SAFETENSORS 1
BDR_API int32_t bdr_agent_set_checkpoint_format(bdr_agent* a, int32_t format);
BDR_API int32_t bdr_agent_save_params(bdr_agent* a, const char* dir);
BDR_API int32_t bdr_agent_load_params(bdr_agent* a, const char* dir);

/* ---- host-side Trainer loops (border-core/src/trainer.rs) -------------------------------------------------------------
 * The reference's Trainer is compiled Rust; this is its compiled counterpart above the C ABI (csrc/trainer.hip, host code).
 * Agent, buffer and environment are reached through function tables, so a border maintainer can drive the library's
 * handles (bdr_trainer_ops_default) or their own objects, and the loop rules are testable without a GPU.
 *   bdr_trainer_train          Trainer::train (trainer.rs:267-327): Sampler::sample_and_push (trainer/sampler.rs:99-144, with
 *                              SimpleStepProcessor, generic_replay_buffer/step_proc.rs:62-137), then train_step (:197-228):
 *                              no opt while env_steps < warmup_period or env_steps % opt_interval != 0; opt_with_record when
 *                              (opt_steps + 1) % record_agent_info_interval == 0; the timer wraps opt*() only; stop at
 *                              opt_steps == max_opts
 *   bdr_trainer_train_offline  Trainer::train_offline (:330-384): warmup_period = 0, opt_interval = 1, no sampling
 * Recorders (TensorBoard, MLflow) are out of scope: `observer` receives what the reference would store.  The Evaluator and the
 * post-processing of every opt step (Trainer::post_process, trainer.rs:231-264: evaluate every eval_interval opt steps, keep the
 * best model, save every save_interval opt steps) are bdr_evaluate and the *_post entries below. */
typedef struct bdr_env_vtable {             /* single-process Env (border-core/src/base/env.rs:45-181) */
    void* ctx;
    int32_t (*reset)(void* ctx, void* obs_out);                                  /* Env::reset(None) */
    /* Env::step_with_reset(&act) (env.rs:137-161): writes obs, reward, flags; when the step is done also init_obs */
    int32_t (*step_with_reset)(void* ctx, const void* act, void* obs_out, float* reward, int8_t* is_terminated,
                               int8_t* is_truncated, void* init_obs_out);
    /* Device-resident observations (zero-initialised tables keep the host convention): with obs_on_device != 0
     * obs_out / init_obs_out are DEVICE buffers of obs_row_bytes on GPU `device` - the environment keeps its observation in HBM
     * (a bdr_atari_prep: bdr_atari_prep_copy_stack writes an environment's stack there) - and the loops act and push through the
     * *_device entries of their function tables: the observation never visits the host. */
    int32_t obs_on_device;
    int32_t device;
} bdr_env_vtable;

typedef struct bdr_trainer_ops {
    void* agent;
    void* buffer;
    int32_t (*agent_set_train)(void* agent, int32_t train);                                       /* Agent::train */
    int32_t (*agent_sample)(void* agent, uint64_t n_procs, const void* obs, void* act_out);       /* Policy::sample */
    int32_t (*agent_opt)(void* agent, void* buffer);                                              /* Agent::opt */
    int32_t (*agent_opt_with_record)(void* agent, void* buffer, float* scalars, int32_t cap, int32_t* n_scalars);
    int32_t (*buffer_push)(void* buffer, uint64_t n, const void* obs, const void* act, const void* next_obs,
                           const float* reward, const int8_t* is_terminated, const int8_t* is_truncated);
    /* used instead of agent_sample / buffer_push when the environment's observations are device-resident (bdr_env_vtable::obs_on_device):
     * bdr_agent_sample_device / bdr_replay_push_device by default; act_out, act, reward and the flags stay host memory */
    int32_t (*agent_sample_device)(void* agent, uint64_t n_procs, const void* obs_dev, uint64_t row_stride, void* act_out);
    int32_t (*buffer_push_device)(void* buffer, uint64_t n, const void* obs_dev, uint64_t obs_stride, const void* act,
                                  const void* next_obs_dev, uint64_t next_obs_stride, const float* reward,
                                  const int8_t* is_terminated, const int8_t* is_truncated);
} bdr_trainer_ops;

typedef struct bdr_trainer_config {         /* trainer/config.rs:30-87; an interval of 0 means "never" */
    uint64_t max_opts;
    uint64_t opt_interval;
    uint64_t warmup_period;
    uint64_t record_agent_info_interval;
    uint64_t record_compute_cost_interval;
    uint64_t obs_row_bytes;                 /* row sizes of the environment's observation / action (online loop) */
    uint64_t act_row_bytes;
} bdr_trainer_config;

typedef struct bdr_trainer_stats {
    uint64_t env_steps, opt_steps, n_records, n_episodes;
    double opt_seconds, sample_seconds;     /* timer_for_opt_steps / timer_for_samples summed over the run */
} bdr_trainer_stats;

#define BDR_TRAINER_EVENT_SKIP 0            /* iteration without an opt step */
#define BDR_TRAINER_EVENT_OPT 1             /* Agent::opt */
#define BDR_TRAINER_EVENT_OPT_RECORD 2      /* Agent::opt_with_record: scalars = the agent's Record */
#define BDR_TRAINER_EVENT_COST 3            /* scalars = {average_opt_time, average_sample_time} in ms (trainer.rs:164-181) */
typedef void (*bdr_trainer_observer)(void* ctx, uint64_t env_steps, uint64_t opt_steps, int32_t event, const float* scalars,
                                     int32_t n_scalars);

BDR_API void bdr_trainer_config_default(bdr_trainer_config* c);
BDR_API void bdr_trainer_ops_default(bdr_trainer_ops* ops, bdr_agent* agent, bdr_replay* buffer);
BDR_API int32_t bdr_trainer_train(const bdr_trainer_config* c, const bdr_trainer_ops* ops, const bdr_env_vtable* env,
                                  bdr_trainer_observer observer, void* observer_ctx, bdr_trainer_stats* out);
BDR_API int32_t bdr_trainer_train_offline(const bdr_trainer_config* c, const bdr_trainer_ops* ops, bdr_trainer_observer observer,
                                          void* observer_ctx, bdr_trainer_stats* out);

/* Trainer::train (trainer.rs:267-327) for the n members of a group in lockstep, member i on its own environment envs[i] and its own
 * buffer.  Per iteration: ONE group sample on the members' prev_obs rows, step_with_reset of every environment in member order, ONE
 * group push of (prev_obs, act, obs, reward, flags), prev_obs = init_obs / obs per member, then train_step's rule once - the members
 * share env_steps, so warm-up, opt_interval, opt vs opt_with_record and the stop at max_opts are one decision - ending in one opt /
 * opt_with_record of the group.  Member i sees exactly the calls bdr_trainer_train makes for a lone agent on envs[i].
 * c->obs_row_bytes is ignored: obs_row_bytes[i] is member i's row size; c->act_row_bytes must be 8 (one i64 action).  Environments
 * with obs_on_device are refused (BDR_ERR_INVALID); Trainer::post_process is bdr_trainer_train_group_post below.  The observer
 * (bdr_trainer_observer with the member index after ctx; may be NULL) receives every member's event of an iteration in member order (scalars: that member's Record on OPT_RECORD); out[n] receives
 * per-member statistics (env_steps, opt_steps and n_records are shared, n_episodes is the member's own). */
typedef struct bdr_group_trainer_ops {
    void* group;
    void* const* buffers;                   /* [n_members] */
    uint32_t n_members;
    uint32_t reserved;
    int32_t (*set_train)(void* group, int32_t train);                                             /* Agent::train of every member */
    int32_t (*sample)(void* group, const void* const* obs, int64_t* act_out);                     /* Policy::sample, one row per member */
    int32_t (*push)(void* group, void* const* buffers, const void* const* obs, const int64_t* act, const void* const* next_obs,
                    const float* reward, const int8_t* is_terminated, const int8_t* is_truncated);
    int32_t (*opt)(void* group, void* const* buffers);                                            /* Agent::opt of every member */
    /* member i's Record scalars in scalars[i * cap_per_member ...], their count in n_scalars[i] */
    int32_t (*opt_with_record)(void* group, void* const* buffers, float* scalars, int32_t cap_per_member, int32_t* n_scalars);
} bdr_group_trainer_ops;
/* the bdr_agent_group_* entries on a group and its members' rings (`buffers` must stay alive while `ops` is used) */
BDR_API void bdr_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_agent_group* group, bdr_replay* const* buffers);
BDR_API int32_t bdr_trainer_train_group(const bdr_trainer_config* c, const uint64_t* obs_row_bytes, const bdr_group_trainer_ops* ops,
                                        const bdr_env_vtable* envs,
                                        void (*observer)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps,
                                                         int32_t event, const float* scalars, int32_t n_scalars),
                                        void* observer_ctx, bdr_trainer_stats* out);

/* ---- Evaluator (border-core/src/evaluator/default_evaluator.rs:64-88, border-minari/src/evaluator.rs:25-62) and
 * Trainer::post_process (trainer.rs:231-264) ---------------------------------------------------------------------------------
 * bdr_evaluate is the reference's loop, literally: for ix in 0..n_episodes: reset_with_index(ix), then sample -> step ->
 * r_total += reward until is_terminated | is_truncated; r_total is one f32 accumulator and the additions happen in call order;
 * score = r_total / (float)n_episodes; normalized = (score - ref_min_score) / (ref_max_score - ref_min_score) when the
 * reference scores are present (border-minari/src/env.rs:162-168).  It does not change the agent's train / eval mode: the
 * Trainer does that. */
typedef struct bdr_eval_env_vtable {        /* the evaluator's view of an Env */
    void* ctx;
    int32_t (*reset_with_index)(void* ctx, uint64_t ix, void* obs_out);          /* Env::reset_with_index (env.rs:180) */
    /* Env::step (no reset): writes obs, reward and the flags */
    int32_t (*step)(void* ctx, const void* act, void* obs_out, float* reward, int8_t* is_terminated, int8_t* is_truncated);
    int32_t obs_on_device;                  /* as bdr_env_vtable: obs_out is a DEVICE buffer of obs_row_bytes on GPU `device` */
    int32_t device;
} bdr_eval_env_vtable;

typedef struct bdr_evaluator {
    uint64_t n_episodes;
    uint64_t obs_row_bytes;                 /* one observation row as the environment writes it (obs_dtype elements) */
    uint64_t act_row_bytes;
    int32_t obs_dtype;                      /* BDR_DTYPE_F32 / BDR_DTYPE_F64 (Minari environments produce float64 rows) */
    const bdr_obs_norm* norm;               /* NULL: the rows are the agent's input as they are */
    int32_t has_ref_scores;
    float ref_min_score;
    float ref_max_score;
    bdr_eval_env_vtable env;
    /* Policy::sample on one row.  agent_sample (every agent kind; the signature of bdr_trainer_ops) is used when norm is NULL and
     * the rows are f32 in host memory; agent_sample_raw (bdr_agent_sample_raw: IQL, AWAC, BC) otherwise. */
    int32_t (*agent_sample)(void* agent, uint64_t n_procs, const void* obs, void* act_out);
    int32_t (*agent_sample_raw)(void* agent, const bdr_obs_norm* norm, uint64_t n, const void* rows, int32_t dtype, int32_t on_device,
                                uint64_t row_stride, void* act_out);
} bdr_evaluator;

typedef struct bdr_eval_result {
    float score;                            /* r_total / n_episodes */
    int32_t has_normalized;
    float normalized;
    uint64_t n_steps;                       /* environment steps of the evaluation */
    uint64_t n_episodes;
} bdr_eval_result;

/* Trainer::post_process after every iteration that took an opt step.  An interval of 0 means never (this header's convention; the
 * reference would divide by zero).  When opt_steps % eval_interval == 0: agent_set_train(0), evaluate, agent_set_train(1) -
 * unconditionally, as trainer.rs:246-248 - the observer gets BDR_TRAINER_EVENT_EVAL, and when score > max_eval_reward (which
 * starts at -FLT_MAX = f32::MIN; a strict >) the model is saved to model_dir/best.  When save_interval > 0 and
 * opt_steps % save_interval == 0 the model is saved to model_dir/<opt_steps>.  The evaluator's time is in neither Trainer timer. */
typedef struct bdr_trainer_post {
    uint64_t eval_interval;
    uint64_t save_interval;
    const bdr_evaluator* evaluator;         /* needed when eval_interval > 0 */
    const char* model_dir;                  /* needed when something is saved */
    int32_t (*save_params)(void* agent, const char* dir);   /* NULL: bdr_agent_save_params after creating the directory */
} bdr_trainer_post;

#define BDR_TRAINER_EVENT_EVAL 4            /* scalars = {score} or {score, normalized} (with reference scores) */

/* zeroes *ev and fills both acting hooks from the library's handles (agent may be NULL: it is not read) */
BDR_API void bdr_evaluator_default(bdr_evaluator* ev, bdr_agent* agent);
BDR_API int32_t bdr_evaluate(const bdr_evaluator* ev, void* agent, bdr_eval_result* out);
BDR_API void bdr_trainer_post_default(bdr_trainer_post* post);
/* bdr_trainer_train / bdr_trainer_train_offline plus post_process; with post == NULL they are those functions (one loop body). */
BDR_API int32_t bdr_trainer_train_post(const bdr_trainer_config* c, const bdr_trainer_ops* ops, const bdr_env_vtable* env,
                                       const bdr_trainer_post* post, bdr_trainer_observer observer, void* observer_ctx,
                                       bdr_trainer_stats* out);
BDR_API int32_t bdr_trainer_train_offline_post(const bdr_trainer_config* c, const bdr_trainer_ops* ops, const bdr_trainer_post* post,
                                               bdr_trainer_observer observer, void* observer_ctx, bdr_trainer_stats* out);

/* ---- The Evaluator and Trainer::post_process for a group ---------------------------------------------------------------------
 * bdr_evaluate_group is default_evaluator.rs:64-88 for every member of a group in lockstep, member i on evs[i] (its own
 * environment, n_episodes, obs_row_bytes and reference scores).  Per round: every member that has episodes left and no open episode
 * gets reset_with_index(ix_i), in member order; ONE sample_members over the members with an open episode; step of each of those
 * environments in member order; then per member r_total_i += reward, n_steps_i += 1, and on is_terminated | is_truncated the episode
 * closes and ix_i += 1.  A member whose ix_i == n_episodes leaves the selection - it does not act any more, so its explorer stream
 * and counters end where a lone bdr_evaluate leaves them - and the loop ends when nobody is left.  Member i sees exactly the calls
 * bdr_evaluate(&evs[i], member i) makes: the same indices, the same actions, one f32 accumulator in call order, the same score
 * and normalised score.  It does not touch the train / eval mode.  evs[i].agent_sample* are not used.  Refused with
 * BDR_ERR_INVALID naming the member: an incomplete environment table, n_episodes == 0, obs_row_bytes == 0, act_row_bytes != 8,
 * obs_dtype != BDR_DTYPE_F32, norm != NULL, env.obs_on_device != 0 (the group acts on host f32 rows).  A failing environment call or
 * a failing sample_members returns its status at once. */
typedef struct bdr_group_eval_ops {
    void* group;
    uint32_t n_members;
    uint32_t reserved;
    /* Policy::sample of members[0..n) (strictly ascending); obs and act_out are indexed by member (bdr_agent_group_sample_members) */
    int32_t (*sample_members)(void* group, const uint32_t* members, uint32_t n, const void* const* obs, int64_t* act_out);
} bdr_group_eval_ops;
BDR_API void bdr_group_eval_ops_default(bdr_group_eval_ops* ops, bdr_agent_group* group);
BDR_API int32_t bdr_evaluate_group(const bdr_evaluator* evs, const bdr_group_eval_ops* ops, bdr_eval_result* out);

/* Trainer::post_process (trainer.rs:231-264) in the group loop.  After an iteration that took an opt step, behind the members'
 * OPT / OPT_RECORD events and ahead of the cost record: when opt_steps % eval_interval == 0, set_train(0), bdr_evaluate_group,
 * set_train(1) - unconditionally, as trainer.rs:246-248 - then every member's BDR_TRAINER_EVENT_EVAL in member order, and member i
 * is saved to model_dirs[i]/best when its score > its own max_eval_reward (each starts at -FLT_MAX = f32::MIN; a strict >).  When
 * save_interval > 0 and opt_steps % save_interval == 0 every member is saved to model_dirs[i]/<opt_steps>.  An interval of 0 means
 * never.  The evaluator's time is in neither Trainer timer.  Member i's observer sees the event sequence bdr_trainer_train_post gives
 * a lone agent.  Refused before anything runs: eval_interval without evaluators (or evaluators bdr_evaluate_group refuses),
 * something to save without model_dirs, a NULL model_dirs[i] (naming the member). */
typedef struct bdr_group_trainer_post {
    uint64_t eval_interval;                 /* 0 = never */
    uint64_t save_interval;                 /* 0 = never */
    const bdr_evaluator* evaluators;        /* [n_members]; needed when eval_interval > 0 */
    const char* const* model_dirs;          /* [n_members]; needed when something is saved */
    bdr_group_eval_ops eval_ops;
    int32_t (*save_member)(void* group, uint32_t member, const char* dir);   /* NULL: mkdir -p + bdr_agent_save_params of the member */
} bdr_group_trainer_post;
BDR_API void bdr_group_trainer_post_default(bdr_group_trainer_post* post, bdr_agent_group* group);
/* bdr_trainer_train_group plus post_process; with post == NULL it is that function (one loop body). */
BDR_API int32_t bdr_trainer_train_group_post(const bdr_trainer_config* c, const uint64_t* obs_row_bytes, const bdr_group_trainer_ops* ops,
                                             const bdr_env_vtable* envs, const bdr_group_trainer_post* post,
                                             void (*observer)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps,
                                                              int32_t event, const float* scalars, int32_t n_scalars),
                                             void* observer_ctx, bdr_trainer_stats* out);

/* ---- border-async-trainer (border-async-trainer/src) -----------------------------------------------------------------------
 * The reference runs one learner thread (AsyncTrainer::train, async_trainer/base.rs:299-388) and n actor threads (Actor::run,
 * actor/base.rs:120-178) in one process: actors sample with their own agent + env, buffer n_buffer transitions in a
 * ReplayBufferProxy (replay_buffer_proxy.rs:52-72) and try_send them as one PushedItemMessage; the learner drains the channel
 * into its replay buffer (update_replay_buffer, :275-284), does not optimise until buffer.len() >= warmup_period (:210,
 * 328-335), and every sync_interval opt steps sends (n_opts, model_info) back (sync, :268-272); an actor adopts a model that is
 * newer than the one it has (actor/base.rs:104-118).
 * Here: csrc/async_trainer.hip, compiled, behind function tables like the Trainer above.  One rank per GPU = one learner + its
 * actors + its local replay shard; `exchange` (optional) runs at every sync point before the local publish and is where the
 * ranks average their learners over RCCL (bdr_agent_allreduce_params).  The model channel is a device-resident mailbox:
 * publish = one device-to-device copy on the learner's stream, sync = one copy on the actor's stream, ordered by events. */
typedef struct bdr_model_mailbox bdr_model_mailbox;
BDR_API int32_t bdr_model_mailbox_create(int32_t device, uint64_t n_floats, uint32_t n_readers, bdr_model_mailbox** out);
BDR_API int32_t bdr_model_mailbox_destroy(bdr_model_mailbox* m);
/* SyncModel::model_info + send (dqn/base.rs:377-389, async_trainer/base.rs:268-272): arena `which` (bdr_agent_arena_device_ptr)
 * of the learner -> mailbox, tagged n_opts.  Asynchronous on the agent's stream. */
BDR_API int32_t bdr_agent_publish_model(bdr_agent* a, int32_t which, bdr_model_mailbox* m, uint64_t n_opts);
/* Actor::sync_model (actor/base.rs:104-118): copies the mailbox into the agent iff mailbox.n_opts > *n_opts_inout (or `first`:
 * sync_model_first, :98-102), then *n_opts_inout = mailbox.n_opts, *updated = 1.  reader: the actor's index (< n_readers). */
BDR_API int32_t bdr_agent_sync_model_from(bdr_agent* a, int32_t which, bdr_model_mailbox* m, uint32_t reader, int32_t first,
                                          uint64_t* n_opts_inout, int32_t* updated);

typedef struct bdr_async_trainer_config {   /* async_trainer/config.rs:13-36 (defaults :101-112) + ActorManagerConfig::n_buffer */
    uint64_t max_opts;
    uint64_t warmup_period;                 /* transitions in the learner's buffer before the first opt */
    uint64_t sync_interval;                 /* opt steps between model syncs (default 100; dqn_atari_async_tch: 1) */
    uint64_t record_agent_info_interval;    /* 0 = never */
    uint64_t record_compute_cost_interval;  /* 0 = never */
    uint64_t n_buffer;                      /* ReplayBufferProxyConfig::n_buffer: transitions per message (100) */
    uint64_t channel_capacity;              /* bounded(1000), actor_manager/base.rs:140 */
    uint64_t warmup_sleep_ms;               /* the 100 ms pause between warm-up and training (async_trainer/base.rs:331) */
    uint64_t obs_row_bytes, act_row_bytes;
} bdr_async_trainer_config;

typedef struct bdr_learner_ops {
    bdr_trainer_ops t;                      /* agent, buffer, set_train, opt, opt_with_record, buffer_push */
    int32_t (*buffer_len)(void* buffer, uint64_t* len);                                  /* ExperienceBufferBase::len */
    int32_t (*publish_model)(void* agent, void* mailbox, uint64_t n_opts);               /* AsyncTrainer::sync */
    void* mailbox;
    int32_t (*exchange)(void* ctx, void* agent, uint64_t opt_steps);                     /* optional: cross-GPU averaging at a sync point */
    void* exchange_ctx;
    /* optional, with `exchange`: agreement across ranks BEFORE every collective.  Called with local_ok = 1 at every sync point
     * (a rank that gets *all_ok = 0 stops there with BDR_ERR_COMM instead of entering a collective a failed peer will never
     * join) and once with local_ok = 0 by a rank whose learner or actor failed, so that its peers stop at their next sync point
     * (bdr_comm_agree: an RCCL MIN all-reduce of the flag).  ctx = exchange_ctx. */
    int32_t (*agree)(void* ctx, int32_t local_ok, int32_t* all_ok);
} bdr_learner_ops;

typedef struct bdr_actor_ops {              /* one Actor: its own agent (built from its own config) and environment */
    void* agent;
    void* mailbox;
    int32_t (*agent_set_train)(void* agent, int32_t train);
    int32_t (*agent_sample)(void* agent, uint64_t n_procs, const void* obs, void* act_out);
    int32_t (*sync_model)(void* agent, void* mailbox, uint32_t actor_id, int32_t first, uint64_t* n_opts_inout, int32_t* updated);
    int32_t (*agent_sample_device)(void* agent, uint64_t n_procs, const void* obs_dev, uint64_t row_stride, void* act_out);   /* env.obs_on_device */
    bdr_env_vtable env;
} bdr_actor_ops;

typedef struct bdr_async_stats {            /* AsyncTrainStat (async_trainer/stat.rs) + counters */
    uint64_t samples_total, opt_steps, n_records, n_syncs, n_messages;
    double duration_s;
    float samples_per_sec, opt_per_sec;
} bdr_async_stats;
typedef struct bdr_actor_stat { uint64_t env_steps, n_syncs; double duration_s; } bdr_actor_stat;   /* ActorStat (actor/stat.rs) */

/* observer(ctx, actor, a, b, event, scalars, n): never called concurrently.  actor = UINT32_MAX for learner events.
 *   SKIP / OPT / OPT_RECORD   a = samples_total, b = opt_steps after the step, scalars = the Record of opt_with_record
 *   SYNC                      the learner published the model of b = opt_steps
 *   PUSH                      a message of n transitions of `actor` entered the buffer (a = samples_total after it)
 *   COST                      scalars = {average_opt_time, average_sample_time} in ms
 *   ACTOR_SYNC                `actor` adopted the model of b opt steps before its env step a */
#define BDR_ASYNC_EVENT_SKIP 0
#define BDR_ASYNC_EVENT_OPT 1
#define BDR_ASYNC_EVENT_OPT_RECORD 2
#define BDR_ASYNC_EVENT_COST 3
#define BDR_ASYNC_EVENT_SYNC 4
#define BDR_ASYNC_EVENT_PUSH 5
#define BDR_ASYNC_EVENT_ACTOR_SYNC 6
typedef void (*bdr_async_observer)(void* ctx, uint32_t actor, uint64_t a, uint64_t b, int32_t event, const float* scalars, int32_t n);

BDR_API void bdr_async_trainer_config_default(bdr_async_trainer_config* c);
BDR_API void bdr_learner_ops_default(bdr_learner_ops* ops, bdr_agent* agent, bdr_replay* buffer, bdr_model_mailbox* mailbox);
BDR_API void bdr_actor_ops_default(bdr_actor_ops* ops, bdr_agent* agent, bdr_model_mailbox* mailbox, const bdr_env_vtable* env);
/* train_async (util.rs:31-92): runs until the learner has done max_opts opt steps; returns the first error of any thread. */
BDR_API int32_t bdr_async_train(const bdr_async_trainer_config* c, const bdr_learner_ops* learner, const bdr_actor_ops* actors,
                                uint32_t n_actors, bdr_async_observer observer, void* observer_ctx, bdr_async_stats* out,
                                bdr_actor_stat* actor_stats);

/* border-atari-env frame preprocessing on the device (border-atari-env/src/env.rs):
 * one handle keeps the `frames: [4][84][84]` u8 stack of n_envs environments in HBM (newest frame first).
 *   reset  env.rs:263-296   all four slots <- warp_and_grayscale(frame)
 *   step   env.rs:312-324   skip_and_max (:126-157: element-wise max of the two last RGB frames of the skip-4 step),
 *                           warp_and_grayscale (:171-195: image 0.23 resize(.., 84, 84, Triangle), then the reference's luma
 *                           with its (b, g, r) channel naming), stack_frame (:197-209)
 * frames are host buffers [n][height][width][3] u8 (render_rgb24 layout); env_ixs[k] names the environment of frame k and
 * may not repeat within one call.  The resize restates image 0.23.14's sample.rs (see oracle/atari_prep.py: parity
 * unpinned against the real crate).  bdr_atari_clip_reward: env.rs:159-169. */
typedef struct bdr_atari_prep bdr_atari_prep;
BDR_API int32_t bdr_atari_prep_create(int32_t device, uint32_t n_envs, uint32_t width, uint32_t height, bdr_atari_prep** out);
BDR_API int32_t bdr_atari_prep_destroy(bdr_atari_prep* h);
BDR_API int32_t bdr_atari_prep_reset(bdr_atari_prep* h, uint32_t n, const uint32_t* env_ixs, const uint8_t* frames);
BDR_API int32_t bdr_atari_prep_step(bdr_atari_prep* h, uint32_t n, const uint32_t* env_ixs, const uint8_t* frames_a,
                                    const uint8_t* frames_b);
/* stacked observations of the named environments, [n][4][84][84] u8, to the host (what BorderAtariObs carries) */
BDR_API int32_t bdr_atari_prep_obs(bdr_atari_prep* h, uint32_t n, const uint32_t* env_ixs, uint8_t* obs_out);
/* device address of all stacks, [n_envs][4][84][84] u8 */
BDR_API int32_t bdr_atari_prep_device_stacks(bdr_atari_prep* h, const uint8_t** stacks);
/* one environment's current stack -> dst_dev (device memory, 4*84*84 bytes), complete when the call returns: what an environment
 * with bdr_env_vtable::obs_on_device writes into obs_out / init_obs_out */
BDR_API int32_t bdr_atari_prep_copy_stack(bdr_atari_prep* h, uint32_t env_ix, void* dst_dev);
/* device address of every environment's stack as it was BEFORE its last step, [n_envs][4][84][84] u8: obs_t of the transition
 * whose next_obs is device_stacks (what bdr_replay_push_device takes; unchanged by reset) */
BDR_API int32_t bdr_atari_prep_device_prev_stacks(bdr_atari_prep* h, const uint8_t** prev);
BDR_API float bdr_atari_clip_reward(float r, int32_t train);

/* Host-side named-tensor files (no GPU involved): the container layer under save_params / load_params, for callers
 * that move parameters themselves (bdr_agent_get_params / set_params take the same reference-layout vectors).
 * `data` is the concatenation of the tensors in `meta` order (row-major f32); the container is chosen by the file
 * name as above.  Reading matches by name, checks shapes, ignores extra entries; nested module archives exported
 * from Python (torch.jit.save of a module with submodules c1, c2, ...) are flattened to dotted names. */
typedef struct bdr_named_tensor {
    const char* name;
    const uint64_t* dims;
    uint32_t ndim;
} bdr_named_tensor;
BDR_API int32_t bdr_checkpoint_write(const char* path, const bdr_named_tensor* meta, uint32_t n_tensors, const float* data, uint64_t n);
BDR_API int32_t bdr_checkpoint_read(const char* path, const bdr_named_tensor* meta, uint32_t n_tensors, float* data, uint64_t n);

/* Parity probes: copy intermediates of the LAST update to the host.
 * what: 0 q_pred_all [B][A], 1 q_next_all [B][A], 2 pred [B], 3 tgt [B], 4 loss [1];
 * AtariCnn only, the online network's activations on `obs`, position-major (NHWC): 5 conv1 [B][400][32], 6 conv2 [B][81][64], 7 conv3 [B][49][64];
 * AtariCnn only, the backward pass: 8 h1 [B][512] (online instance on `obs`), 9 dq [B] (dL/dQ(s,a)), 10 dh1 [B][512], and the gradients
 * w.r.t. the conv layers' pre-activations, position-major: 11 dy3 [B*49][64], 12 dy2 [B*81][64], 13 dy1 [B*400][32];
 * AtariCnn only, the other network instances of the update, layouts as 5-8 and 0: qnet_tgt(next_obs) 14 conv1, 15 conv2, 16 conv3, 17 h1
 * (its Q rows are 1); qnet(next_obs), which runs with double DQN only (BDR_ERR_INVALID without it): 18 conv1, 19 conv2, 20 conv3, 21 h1,
 * 22 Q rows [B][A]. */
BDR_API int32_t bdr_dqn_probe(bdr_agent* a, int32_t what, float* out, uint64_t n);
/* Layer probes of the Mlp DQN agent: ONE raw device buffer of the last update (bdr_dqn_update_on_batch*, opt, a group's round) to the
 * host after synchronising the agent's stream, rows x padded leading dimension, padding included.  B = rows of that update, Kp / Np =
 * sizes padded to 64, z = network instance (0 online on obs, 1 target on next_obs, 2 online on next_obs under double DQN), l = layer:
 *   X_IN(z) [B][Kp_0]; ACT(z, l) [B][Np_l]; DY(l) [B][Np_l]; PRED, TGT, LOSS_ROW, TD_ABS [B]; LOSS [1];
 *   DW_PART(l) [chunks][Kp_l * Np_l + Np_l] the row-chunk partials of the grouped weight gradient;
 *   Q, Q_TGT, GRAD, M, V: the whole padded arena (weights [Kp_l][Np_l], bias [Np_l] per layer);
 *   CHUNKS [1]: the row chunks the last grouped weight-gradient launch used; FORM [1]: the step the last update took (BDR_DQN_MLP_FORM_*).
 * z and l are 0 where the buffer has none.  BDR_ERR_INVALID, without reading anything, before any update, for a float count that is not
 * exactly the buffer's, an index out of range (z >= instances of the update) or given where the buffer has none, DW_PART / CHUNKS after
 * a step that formed no partials (the one-workgroup forms, 64x64 tiles), an unknown buffer, and a handle that is not an Mlp DQN agent. */
enum { BDR_DQN_MLP_BUF_X_IN = 0, BDR_DQN_MLP_BUF_ACT = 1, BDR_DQN_MLP_BUF_DY = 2, BDR_DQN_MLP_BUF_PRED = 3, BDR_DQN_MLP_BUF_TGT = 4,
       BDR_DQN_MLP_BUF_LOSS_ROW = 5, BDR_DQN_MLP_BUF_TD_ABS = 6, BDR_DQN_MLP_BUF_LOSS = 7, BDR_DQN_MLP_BUF_DW_PART = 8, BDR_DQN_MLP_BUF_Q = 9,
       BDR_DQN_MLP_BUF_Q_TGT = 10, BDR_DQN_MLP_BUF_GRAD = 11, BDR_DQN_MLP_BUF_M = 12, BDR_DQN_MLP_BUF_V = 13, BDR_DQN_MLP_BUF_CHUNKS = 14,
       BDR_DQN_MLP_BUF_FORM = 15 };
enum { BDR_DQN_MLP_FORM_LDS = 0,          /* one workgroup, matrices resident in LDS (k_dqn_mlp_step_lds) */
       BDR_DQN_MLP_FORM_GLOBAL = 1,       /* one workgroup through global memory (k_dqn_mlp_step) */
       BDR_DQN_MLP_FORM_LAYERS_HEAD = 2,  /* layer by layer, row-block head (k_mlp_head_td) */
       BDR_DQN_MLP_FORM_LAYERS_TD = 3,    /* layer by layer, k_td_dense + k_mean_rows */
       BDR_DQN_MLP_FORM_TILES = 4 };      /* 64x64 tiles, one launch per tensor (BDR_NO_SMALL_GEMM=1) */
BDR_API int32_t bdr_dqn_mlp_layer_probe(bdr_agent* a, int32_t buf, int32_t z, int32_t layer, float* out, uint64_t n);

/* Per-kernel device timing of the opt step (bench.py roofline leg): when enabled the step is
 * bracketed kernel by kernel with HIP events on the agent's stream. */
BDR_API int32_t bdr_agent_profile_enable(bdr_agent* a, int32_t on);
/* names_out: '\n'-separated kernel labels; ms_out[i] = mean ms per launch since enable. */
BDR_API int32_t bdr_agent_profile_read(bdr_agent* a, char* names_out, uint64_t names_cap,
                                       float* ms_out, uint64_t* count_inout);

/* ------------------------------------------------------------------------------------------
 * IQN agent  (border-tch-agent/src/iqn/base.rs, iqn/config.rs:50-67, iqn/model/base.rs)
 * ---------------------------------------------------------------------------------------- */
/* IqnSample (iqn/model/base.rs:327-387); Const32 yields 33 points like the reference. */
enum { BDR_IQN_CONST10 = 0, BDR_IQN_CONST32 = 1, BDR_IQN_UNIFORM10 = 2, BDR_IQN_UNIFORM8 = 3,
       BDR_IQN_UNIFORM32 = 4, BDR_IQN_UNIFORM64 = 5, BDR_IQN_MEDIAN = 6 };
typedef struct {
    bdr_net_config psi;          /* feature extractor F: AtariCnn{skip_linear:true} or Mlp (out_dim = feature_dim) */
    int32_t feature_dim, embed_dim;                   /* IqnModelConfig */
    int32_t n_f_units; int32_t f_units[BDR_MAX_UNITS];   /* merge net M = Mlp(feature_dim -> units -> n_actions) */
    int32_t n_actions;
    double lr;                                        /* OptimizerConfig::{Adam,AdamW}.lr; AdamW fields: `opt` below */
    uint64_t soft_update_interval, n_updates_per_opt, batch_size;
    double discount_factor, tau;
    int32_t sample_percents_pred, sample_percents_tgt, sample_percents_act;
    int32_t train;
    int32_t device;
    uint64_t seed;
    bdr_adamw_config opt;        /* IqnModelConfig.opt_config (iqn/model/config.rs:50) when it is AdamW; `lr` above either way */
    int32_t arithmetic;          /* BDR_ARITH_* */
    int32_t reserved;
} bdr_iqn_config;
BDR_API void bdr_iqn_config_default(bdr_iqn_config* cfg);                    /* iqn/config.rs:50-67 */
BDR_API int32_t bdr_iqn_create(const bdr_iqn_config* cfg, bdr_agent** out);  /* iqn/base.rs:230-268 */
/* One Iqn::opt_ update on a host minibatch with injected percent points (the reference draws them with
 * Tensor::rand, iqn/model/base.rs:365-368). */
BDR_API int32_t bdr_iqn_update_on_batch(bdr_agent* a, uint64_t n, const void* obs, const int64_t* act,
                                        const void* next_obs, const float* reward, const int8_t* is_terminated,
                                        const float* tau_pred, int32_t n_pred, const float* tau_tgt, int32_t n_tgt,
                                        float* loss_out);
/* IqnModel::forward (iqn/model/base.rs:198-234): z_out [n][n_tau][n_actions]; which 0 = iqn, 1 = iqn_tgt. */
BDR_API int32_t bdr_iqn_forward(bdr_agent* a, int32_t which, uint64_t n, const void* obs, const float* tau,
                                int32_t n_tau, float* z_out);
/* Policy::sample greedy part (iqn/base.rs:204-228): values averaged over sample_percents_act. */
BDR_API int32_t bdr_iqn_qvalues(bdr_agent* a, uint64_t n, const void* obs, float* q_out, int64_t* argmax_out);
/* Parity probes: the raw buffers, padded leading dimensions included, that the LAST model forward / update left behind, to the
 * host.  M = B * N rows; Ep, Fp, Np_i = embed_dim, feature_dim, the i-th merge-net layer's width rounded up to 64 (padding columns
 * are exactly 0); ldf = 3136 (AtariCnn) or Fp (Mlp).  Forward buffers (M = rows of the last forward; after an update that is the
 * ONLINE network's pass on `obs` with n_pred points - the target pass went through the same buffers before it):
 *   COS [M][Ep], PHI [M][Fp], PSI [B][ldf] (conv3's activation / the Mlp's output), F_ACT + i [M][Np_i] (hidden activations; the
 *   last one is z), A1 [B][400][32], A2 [B][81][64] (AtariCnn), PSI_ACT + i [B][pad64(units_i)] (Mlp).
 * Gradient buffers of the last update (M = B * n_pred):
 *   F_DY + i [M][Np_i] (gradients at the merge net's pre-activations; the last one is dL/dz), DLIN [M][Fp] (the gradient at the
 *   cosine layer's pre-activation), DPSI [B][ldf], TGT [B][n_tgt], LOSS_ROW [B], DY2 [B][81][64], DY1 [B][400][32] (AtariCnn),
 *   PSI_DY + i (Mlp).
 * n must be the buffer's float count (BDR_ERR_INVALID otherwise, as for an unknown `what` or when nothing has run yet).
 * bdr_iqn_forward and bdr_iqn_qvalues overwrite the forward buffers, and with more rows or percent points than the agent has held
 * so far they reallocate every buffer (the gradient buffers are then gone): probe before calling either. */
enum { BDR_IQN_PROBE_COS = 0, BDR_IQN_PROBE_PHI = 1, BDR_IQN_PROBE_PSI = 2, BDR_IQN_PROBE_DLIN = 3, BDR_IQN_PROBE_DPSI = 4,
       BDR_IQN_PROBE_TGT = 5, BDR_IQN_PROBE_LOSS_ROW = 6, BDR_IQN_PROBE_A1 = 7, BDR_IQN_PROBE_A2 = 8, BDR_IQN_PROBE_DY2 = 9,
       BDR_IQN_PROBE_DY1 = 10, BDR_IQN_PROBE_F_ACT = 16, BDR_IQN_PROBE_F_DY = 32, BDR_IQN_PROBE_PSI_ACT = 48, BDR_IQN_PROBE_PSI_DY = 64 };
BDR_API int32_t bdr_iqn_probe(bdr_agent* a, int32_t what, float* out, uint64_t n);

/* ------------------------------------------------------------------------------------------
 * SAC agent  (border-tch-agent/src/sac/base.rs, sac/config.rs:85-105, sac/ent_coef.rs,
 * Actor = Mlp2 (mlp/mlp2.rs), Critic = Mlp on cat(obs, act) (mlp/base.rs:83-107))
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t obs_dim, act_dim;
    int32_t n_pi_units; int32_t pi_units[BDR_MAX_UNITS];   /* ActorConfig.pi_config (MlpConfig.units) */
    int32_t n_q_units;  int32_t q_units[BDR_MAX_UNITS];    /* CriticConfig.q_config                  */
    double lr_actor, lr_critic;                             /* lr of each model; AdamW fields: opt_actor / opt_critic below */
    double gamma, tau;
    int32_t ent_coef_auto;       /* EntCoefMode::Auto(target_entropy, lr) vs Fix(alpha) */
    double ent_coef_alpha, target_entropy, ent_coef_lr;
    double epsilon, min_lstd, max_lstd;
    uint64_t n_updates_per_opt, batch_size;
    int32_t train;
    int32_t critic_loss;         /* BDR_LOSS_* */
    double reward_scale;
    int32_t n_critics;
    int32_t device;
    uint64_t seed;
    bdr_adamw_config opt_actor;  /* ActorConfig.opt_config (sac/actor/config.rs:15) when it is AdamW; lr_actor above either way  */
    bdr_adamw_config opt_critic; /* CriticConfig.opt_config (sac/critic/config.rs) likewise; EntCoef keeps nn::Adam::default() (ent_coef.rs:41) */
} bdr_sac_config;
BDR_API void bdr_sac_config_default(bdr_sac_config* cfg);                    /* sac/config.rs:85-105  */
BDR_API int32_t bdr_sac_create(const bdr_sac_config* cfg, bdr_agent** out);  /* sac/base.rs:237-285   */
/* One Sac::opt_ loop iteration on a host minibatch with injected N(0,1) draws (the reference takes
 * them from torch's global CPU generator, sac/base.rs:76).  rec3: loss_critic, loss_actor, ent_coef.
 * Parameter models for bdr_agent_{get,set}_params / param_count_of: 0 pi, 1+i qnet_i,
 * 1+n_critics+i qnet_tgt_i, 1+2*n_critics log_alpha; +100 gradient, +200 exp_avg, +300 exp_avg_sq, +400 max_exp_avg_sq (amsgrad). */
BDR_API int32_t bdr_sac_update_on_batch(bdr_agent* a, uint64_t n, const float* obs, const float* act,
                                        const float* next_obs, const float* reward, const int8_t* is_terminated,
                                        const float* z_actor, const float* z_next, float* rec3);
/* Parity probes: intermediates of the LAST SAC update, to the host.  what:
 *   0 q_pred [n_critics][B]   Q_i(obs, act), the predictions of update_critic (sac/base.rs:128-131; qvals :89-98)
 *   1 q_next [n_critics][B]   target critics on (next_obs, a'), a' ~ pi(next_obs) of the UPDATED actor (:112-118)
 *   2 qvals_min [B]           min over 1 (:100-105)          3 next_log_p [B]  log p(a' | next_obs) (:113)
 *   4 tgt [B]                 the TD target (:119-122)       7 next_act [B][act_dim]
 *   5 q_pi [n_critics][B]     Q_i(obs, a_pi) of update_actor (:157-158)      6 log_p [B]  log p(a_pi | obs) (:156)
 * 5 and 6 are overwritten by the critic phase and therefore kept aside by bdr_sac_update_on_batch only. */
BDR_API int32_t bdr_sac_probe(bdr_agent* a, int32_t what, float* out, uint64_t n);
/* Layer probes: ONE raw device buffer of the last bdr_sac_update_on_batch (or, phase CRITIC, of the last bdr_sac_sample) to the host,
 * rows x padded leading dimension, padding columns included (they must be exactly 0).  The step reuses its buffers, hence two phases:
 *   BDR_SAC_PHASE_ACTOR   a snapshot taken behind the actor's Adam launch, before the updated actor's pass on next_obs.  Opt-in
 *                         (bdr_sac_keep_layers), taken by bdr_sac_update_on_batch only: ordered device-to-device copies on the
 *                         agent's stream, never inside opt(), a captured step or the two-queue sequence.
 *   BDR_SAC_PHASE_CRITIC  the buffers as the step (or the acting call) left them.
 * buf (critic i / layer l where the buffer has them, 0 otherwise), floats; B = rows, Kp / Np = sizes padded to 64:
 *   X_O, X_NO [B][Kp_pi]; XQ_A, XQ_N, XQ_C, DXQ(i) [B][Kp_q]; Z [2][B][act_dim]; T_ACT(l), T_DY(l) [B][Np_l] (trunk layer l);
 *   MEAN, E, A_S, S_S, SD_S, GMEAN, GE [B][Np_head]; LOGP, TGT [B]; C_ACT(i, l), C2_ACT(i, l), C_DY(i, l) [B][Np_l];
 *   LROW [3 + n_critics][ceil(B / 32)] block partials (log_p + target, log_p, qmin, loss of critic 0..); SCAL [4]: loss_critic, loss_actor;
 *   LOG_ALPHA [1]; PI_CHUNKS(l), Q_CHUNKS(l) [1]: the row chunks the weight-gradient launch used for layer l (actor: heads are layers
 *   n_trunk, n_trunk + 1); PI_PART(l), Q_PART(i, l) [chunks][Kp * Np + Np] the partials; PI_GRAD, Q_GRAD(i): the whole padded gradient arena.
 * Phase ACTOR holds what the actor phase produced: X_NO, XQ_N, XQ_C, TGT (and DXQ where the row-block kernels run, which never form
 * it) are refused there.  After bdr_sac_sample / bdr_sac_sample_device phase CRITIC serves only what the acting pass wrote (X_O, T_ACT,
 * MEAN, E, A_S, S_S, SD_S, LOGP, XQ_A) until the next update.
 * BDR_ERR_INVALID for an unknown phase or buffer, an index out of range, a wrong float count, and when there is nothing to read yet. */
enum { BDR_SAC_PHASE_ACTOR = 0, BDR_SAC_PHASE_CRITIC = 1 };
enum { BDR_SAC_BUF_X_O = 0, BDR_SAC_BUF_X_NO = 1, BDR_SAC_BUF_XQ_A = 2, BDR_SAC_BUF_XQ_N = 3, BDR_SAC_BUF_XQ_C = 4, BDR_SAC_BUF_Z = 5,
       BDR_SAC_BUF_T_ACT = 6, BDR_SAC_BUF_T_DY = 7, BDR_SAC_BUF_MEAN = 8, BDR_SAC_BUF_E = 9, BDR_SAC_BUF_A_S = 10, BDR_SAC_BUF_S_S = 11,
       BDR_SAC_BUF_SD_S = 12, BDR_SAC_BUF_LOGP = 13, BDR_SAC_BUF_GMEAN = 14, BDR_SAC_BUF_GE = 15, BDR_SAC_BUF_C_ACT = 16,
       BDR_SAC_BUF_C2_ACT = 17, BDR_SAC_BUF_C_DY = 18, BDR_SAC_BUF_DXQ = 19, BDR_SAC_BUF_TGT = 20, BDR_SAC_BUF_LROW = 21,
       BDR_SAC_BUF_SCAL = 22, BDR_SAC_BUF_LOG_ALPHA = 23, BDR_SAC_BUF_PI_PART = 24, BDR_SAC_BUF_Q_PART = 25, BDR_SAC_BUF_PI_GRAD = 26,
       BDR_SAC_BUF_Q_GRAD = 27, BDR_SAC_BUF_PI_CHUNKS = 28, BDR_SAC_BUF_Q_CHUNKS = 29 };
BDR_API int32_t bdr_sac_keep_layers(bdr_agent* a, int32_t on);
BDR_API int32_t bdr_sac_layer_probe(bdr_agent* a, int32_t phase, int32_t buf, int32_t critic, int32_t layer, float* out, uint64_t n);
/* Policy::sample (sac/base.rs:215-225). */
BDR_API int32_t bdr_sac_sample(bdr_agent* a, uint64_t n, const float* obs, float* act_out);
/* the same for observation rows in HBM (row i at obs_dev + i * row_stride bytes), see bdr_agent_sample_device */
BDR_API int32_t bdr_sac_sample_device(bdr_agent* a, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out);

/* ------------------------------------------------------------------------------------------
 * IQL agent  (border-candle-agent/src/iql/{base.rs,config.rs,value.rs}; offline RL)
 * Value = Mlp (mlp.rs:14-24, iql/value.rs), critics = MultiCritic of Mlp on cat(obs, act) (util/critic.rs),
 * actor = GaussianActor (util/actor.rs) over Mlp3 (mlp/mlp3.rs): mean = Mlp(obs) without output activation and a
 * state-independent log-std `head2` [1, act_dim] initialised to 0.
 * ---------------------------------------------------------------------------------------- */
enum { BDR_ACTIVATION_NONE = 0, BDR_ACTIVATION_RELU = 1, BDR_ACTIVATION_TANH = 2, BDR_ACTIVATION_SIGMOID = 3 };   /* lib.rs:58-63 Activation */
enum { BDR_ACTION_LIMIT_CLAMP = 0, BDR_ACTION_LIMIT_TANH = 1 };                                                /* util/actor.rs:29-32 ActionLimit */

/* MlpConfig of border-candle-agent (mlp/config.rs:6-11).  activation_out: BDR_ACTIVATION_NONE / _RELU (Tanh / Sigmoid: BDR_ERR_INVALID); BC: all four.
 * The actor's Mlp3 ignores activation_out, as the reference does (mlp3.rs: mlp_forward(.., &Activation::None)). */
typedef struct {
    int32_t n_units;
    int32_t units[BDR_MAX_UNITS];
    int32_t activation_out; /* BDR_ACTIVATION_* */
} bdr_mlp_config;

/* IqlConfig (iql/config.rs:109-125) with its ValueConfig, MultiCriticConfig (util/critic.rs:35-43) and GaussianActorConfig
 * (util/actor.rs:44-55).  Each model's OptimizerConfig is `lr` plus a bdr_adamw_config: Adam{lr} is candle-optimisers' Adam with
 * PyTorch's defaults, AdamW is candle-nn's (weight_decay 0.01 by default); amsgrad does not exist there and is rejected. */
typedef struct {
    int32_t obs_dim, act_dim;
    bdr_mlp_config value;         /* ValueConfig.value_config                 */
    bdr_mlp_config actor;         /* GaussianActorConfig.policy_config (Mlp3) */
    bdr_mlp_config critic;        /* MultiCriticConfig.q_config               */
    int32_t n_critics;            /* MultiCriticConfig.n_nets (default 2)     */
    double critic_tau;            /* MultiCriticConfig.tau (default 0.005)    */
    double lr_value, lr_actor, lr_critic;
    bdr_adamw_config opt_value, opt_actor, opt_critic;
    double min_log_std, max_log_std;  /* GaussianActorConfig (-20, 2)     */
    int32_t action_limit;             /* BDR_ACTION_LIMIT_* (default Clamp{-1, 1}) */
    double action_min, action_max, action_scale;
    double gamma;                 /* 0.99 (f32 in the reference) */
    double tau_iql;               /* 0.7                          */
    double inv_lambda;            /* 10 (= 1 / lambda)            */
    double exp_adv_max;           /* 100                          */
    int32_t adv_softmax;          /* false                        */
    int32_t critic_loss;          /* BDR_LOSS_* (Mse)             */
    uint64_t n_updates_per_opt, batch_size;   /* 1, 1 */
    int32_t train;
    int32_t device;               /* -1: none given */
    uint64_t seed;                /* the library's parameter initialiser and the device noise stream of Policy::sample */
} bdr_iql_config;
BDR_API void bdr_iql_config_default(bdr_iql_config* cfg);                    /* iql/config.rs:109-125 */
BDR_API int32_t bdr_iql_create(const bdr_iql_config* cfg, bdr_agent** out);  /* iql/base.rs:226-270 (Configurable::build) */
/* One Iql::opt_ loop iteration (iql/base.rs:157-188) on a host minibatch: update_value (:75-86), update_critic (:88-121) with the
 * soft update of every target critic, update_actor (:123-155).  gamma_not_done counts is_truncated (util.rs:235-255).
 * rec3: loss_value, loss_critic, loss_actor.
 * Parameter models for bdr_agent_{get,set}_params / param_count_of: 0 actor (mlp.ln{k}.weight/bias ..., then head2), 1+i critic_i,
 * 1+n_critics+i critic_tgt_i, 1+2*n_critics value; +100 gradient, +200 exp_avg, +300 exp_avg_sq.  SyncModel ships model 0. */
BDR_API int32_t bdr_iql_update_on_batch(bdr_agent* a, uint64_t n, const float* obs, const float* act, const float* next_obs,
                                        const float* reward, const int8_t* is_terminated, const int8_t* is_truncated, float* rec3);
/* Parity probes: intermediates of the LAST IQL update, to the host.  what:
 *   0 q_tgt_min [B]     min_i Qtgt_i(obs, act) of update_value (:77; util/critic.rs:205-218)
 *   1 v [B]             V(obs) before the value step (:78)          2 u [B]     q - v (:79)
 *   3 tgt [B]           r + gamma_not_done * V'(next_obs) (:99-101)
 *   4 q_pred [n_critics][B]  Q_i(obs, act) of update_critic (:97)
 *   5 q_tgt_min [B]     min_i Qtgt_i(obs, act) of update_actor, after the soft update (:127)
 *   6 w [B]             the advantage weights (:129-136)            7 logp [B]  log pi(act | obs) (:141)
 *   8 v_next [B]        V'(next_obs) (:100)                          9 v_obs [B]  V'(obs) of update_actor (:128) */
BDR_API int32_t bdr_iql_probe(bdr_agent* a, int32_t what, float* out, uint64_t n);
/* Policy::sample (util/actor.rs:226-241): train: mean + std * N(0,1) (the agent's device noise stream, bdr_agent_draw_noise),
 * eval: mean; then clamp(action_min, action_max) or action_scale * tanh. */
BDR_API int32_t bdr_iql_sample(bdr_agent* a, uint64_t n, const float* obs, float* act_out);
/* the same for observation rows in HBM (row i at obs_dev + i * row_stride bytes), see bdr_agent_sample_device */
BDR_API int32_t bdr_iql_sample_device(bdr_agent* a, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out);

/* A GROUP of IQL agents over uniform rings (or views of one ring, bdr_replay_view_create): Iql::opt_ (iql/base.rs:157-188) of every
 * member in the launch sequence of ONE member - gather, pack, the critics', actor's and value's forwards, update_value, V'(obs) |
 * V'(next_obs), update_critic with the soft update, the target critics again, update_actor: 3 (Lq + Lv) + 2 Lp + 8 launches for Lv, Lq,
 * Lp layers (n_units + 1) of value, critic and actor, whatever the number of members; the member index is one more grid dimension -
 * bit for bit what bdr_agent_opt of the members one after the other gives.  The calls carry the semantics of their bdr_bc_group_*
 * namesakes: create adopts the members onto one stream and owns them from then on (bdr_agent_destroy of a member is refused;
 * bdr_iql_group_destroy destroys them), every bdr_agent_* / bdr_iql_* call on a member (update_on_batch, sample, probe, parameter views,
 * checkpoints) keeps its meaning and is ordered with the group's calls.
 * One value for all members: obs_dim, act_dim, the three networks' units and activation_out, n_critics, batch_size, the device.  Free
 * per member: seed, tau_iql, inv_lambda, exp_adv_max, gamma, critic_tau, adv_softmax, critic_loss, the action limit and its scale, the
 * log-std clamps, the three learning rates, optimizer kinds and scalars.  Refused (BDR_ERR_INVALID, naming the first member concerned):
 * a non-IQL agent, another shape, n_critics > 2, n_critics x critic layers > 16, more than 12 reduce segments, n_updates_per_opt != 1,
 * profiling or a gradient communicator switched on, another device, the same agent twice, an agent that is in a group already; more
 * than 65535 members or a launch beyond the grid limits (naming the kernel).
 * buffers[p] is member p's: a uniform StdRng ring of f32 rows on the group's device, or a view of one.  A prioritized ring, a frame store,
 * the xoshiro stream, an empty ring (BDR_ERR_EMPTY), a NULL and one bdr_replay for two members are refused, naming the member, and a
 * refused call leaves every member's three step counters, n_opts and stream position where they were.  _opt does not synchronise;
 * _opt_with_scalars synchronises once and returns every member's record (three keys: loss_value, loss_critic, loss_actor; cap_per_member
 * >= 3) at out + p * cap_per_member.  _info fills bdr_group_info with form = BDR_GROUP_FORM_IQL_LAYERS. */
typedef struct bdr_iql_group bdr_iql_group;
BDR_API int32_t bdr_iql_group_create(bdr_agent* const* agents, uint32_t n, bdr_iql_group** out);   /* iql/base.rs:157-188 (opt_ of every member) */
BDR_API int32_t bdr_iql_group_destroy(bdr_iql_group* g);                                           /* iql/base.rs:157-188 */
BDR_API int32_t bdr_iql_group_size(const bdr_iql_group* g, uint32_t* n);                           /* iql/base.rs:157-188 */
BDR_API int32_t bdr_iql_group_member(const bdr_iql_group* g, uint32_t i, bdr_agent** out);         /* iql/base.rs:157-188 */
BDR_API int32_t bdr_iql_group_info(const bdr_iql_group* g, bdr_group_info* out);                   /* iql/base.rs:157-188 */
BDR_API int32_t bdr_iql_group_opt(bdr_iql_group* g, bdr_replay* const* buffers);                   /* iql/base.rs:157-188 */
BDR_API int32_t bdr_iql_group_opt_with_scalars(bdr_iql_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out);   /* iql/base.rs:157-188, record :177-185 */
BDR_API int32_t bdr_iql_group_sync(bdr_iql_group* g);                                              /* iql/base.rs:157-188 */

/* ------------------------------------------------------------------------------------------
 * AWAC agent  (border-candle-agent/src/awac/{base.rs,config.rs}; offline and online RL)
 * Critics = MultiCritic of Mlp on cat(obs, act) (util/critic.rs), actor = GaussianActor (util/actor.rs) over Mlp3, as for IQL;
 * there is no value network.
 * ---------------------------------------------------------------------------------------- */
/* AwacConfig (awac/config.rs:120-141) with its MultiCriticConfig (util/critic.rs:35-43) and GaussianActorConfig (util/actor.rs:44-55).
 * AwacConfig's tau, min_lstd, max_lstd, reward_scale, n_critics and seed are not read by the reference agent (awac/base.rs:249-280)
 * and have no field here: the soft-update rate is MultiCriticConfig.tau (critic_tau), the critic count MultiCriticConfig.n_nets
 * (n_critics) and the log-std bounds GaussianActorConfig's (min_log_std, max_log_std).  amsgrad is rejected, as for IQL.
 * batch_size must be >= 2: at one row the reference's squeeze(D::Minus1) (awac/base.rs:88; util/critic.rs:197-218) turns the
 * critic minima and the TD target into scalars while each prediction keeps shape [1], and candle's same-shape tensor ops reject
 * that pair, so the reference cannot run a one-row batch (BDR_ERR_INVALID). */
typedef struct {
    int32_t obs_dim, act_dim;
    bdr_mlp_config actor;         /* GaussianActorConfig.policy_config (Mlp3) */
    bdr_mlp_config critic;        /* MultiCriticConfig.q_config               */
    int32_t n_critics;            /* MultiCriticConfig.n_nets (default 2)     */
    double critic_tau;            /* MultiCriticConfig.tau (default 0.005)    */
    double lr_actor, lr_critic;
    bdr_adamw_config opt_actor, opt_critic;
    double min_log_std, max_log_std;  /* GaussianActorConfig (-20, 2)     */
    int32_t action_limit;             /* BDR_ACTION_LIMIT_* (default Clamp{-1, 1}) */
    double action_min, action_max, action_scale;
    double gamma;                 /* 0.99 (f32 in the reference) */
    double inv_lambda;            /* 10 (= 1 / lambda)            */
    double exp_adv_max;           /* 100                          */
    int32_t adv_softmax;          /* false                        */
    int32_t critic_loss;          /* BDR_LOSS_* (Mse)             */
    uint64_t n_updates_per_opt, batch_size;   /* 1, 1 (batch_size 1 is rejected, see above) */
    int32_t train;                /* false: the agent is built in eval mode (awac/base.rs:272) */
    int32_t device;               /* -1: none given */
    uint64_t seed;                /* the library's parameter initialiser and the device noise stream of Policy::sample */
} bdr_awac_config;
BDR_API void bdr_awac_config_default(bdr_awac_config* cfg);                    /* awac/config.rs:120-141 */
BDR_API int32_t bdr_awac_create(const bdr_awac_config* cfg, bdr_agent** out);  /* awac/base.rs:249-280 (Configurable::build) */
/* One Awac::opt_ loop iteration (awac/base.rs:170-215) on a host minibatch: update_actor (:127-168), then update_critic (:66-125) on
 * the same batch with next_act drawn from the UPDATED actor, then the soft update of every target critic.  The advantage uses the
 * ONLINE critics (qvals_min, util/critic.rs:197-202); the critic loss is the SUM over critics of mse / smooth_l1; gamma_not_done
 * counts is_truncated (util.rs:235-255).
 * Noise: in train mode act_ = mean + std z_pi and next_act = mean' + std' z_next.  z_pi / z_next: n * act_dim host N(0,1) draws,
 * or NULL for the agent's device stream (the one bdr_agent_draw_noise reads); each NULL set takes n * act_dim draws, z_pi's first,
 * row-major [n][act_dim].  Host draws take nothing from the stream.  Eval mode uses the means and no draws.
 * rec8: loss_critic, loss_actor, q_tgt_abs_mean, adv_mean, adv_abs_mean, logp_mean, reward_mean, next_q_mean of this update.
 * Parameter models for bdr_agent_{get,set}_params / param_count_of: 0 actor (mlp.ln{k}.weight/bias ..., then head2), 1+i critic_i,
 * 1+n_critics+i critic_tgt_i; +100 gradient, +200 exp_avg, +300 exp_avg_sq.  SyncModel ships model 0.
 * Record of bdr_agent_opt_with_scalars: the 8 keys above; the first five averaged over n_updates_per_opt, logp_mean, reward_mean
 * and next_q_mean summed over the updates, as the reference does (awac/base.rs:197-212). */
BDR_API int32_t bdr_awac_update_on_batch(bdr_agent* a, uint64_t n, const float* obs, const float* act, const float* next_obs,
                                         const float* reward, const int8_t* is_terminated, const int8_t* is_truncated,
                                         const float* z_pi, const float* z_next, float* rec8);
/* Parity probes: intermediates of the LAST AWAC update, to the host.  what:
 *   0 q_data_min [B]    min_i Q_i(obs, act) (:134-136)           1 q_pi_min [B]   min_i Q_i(obs, act_) (:137)
 *   2 adv [B]           q - v (:138)                             3 w [B]          the advantage weights (:141-148)
 *   4 logp [B]          log pi(act | obs) (:153)                 5 act_ [B][act_dim]    actor.sample(obs) (:133)
 *   6 next_act [B][act_dim]  actor.sample(next_obs) of the updated actor (:85)
 *   7 next_q [B]        min_i Qtgt_i(next_obs, next_act) (:86-88)  8 tgt [B]      r + gamma_not_done * next_q (:88)
 *   9 q_pred [n_critics][B]  Q_i(obs, act) (:76) */
BDR_API int32_t bdr_awac_probe(bdr_agent* a, int32_t what, float* out, uint64_t n);
/* Policy::sample (util/actor.rs:226-241): train: mean + std * N(0,1) (the agent's device noise stream, bdr_agent_draw_noise),
 * eval: mean; then clamp(action_min, action_max) or action_scale * tanh. */
BDR_API int32_t bdr_awac_sample(bdr_agent* a, uint64_t n, const float* obs, float* act_out);
/* the same for observation rows in HBM (row i at obs_dev + i * row_stride bytes), see bdr_agent_sample_device */
BDR_API int32_t bdr_awac_sample_device(bdr_agent* a, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out);

/* ------------------------------------------------------------------------------------------
 * SAC agent of border-candle-agent  (border-candle-agent/src/sac/{base.rs,config.rs,ent_coef.rs}; online RL)
 * Not the bdr_sac_* agent above, which restates border-tch-agent/src/sac.  Critics = MultiCritic of Mlp on cat(obs, act)
 * (util/critic.rs), actor = GaussianActor (util/actor.rs) over Mlp3, as for IQL and AWAC, or over Mlp2 (mlp/mlp2.rs), the form the
 * reference's examples build (examples/gym/sac_pendulum, sac_fetch_reach, convert_policy: SacConfig<Mlp, Mlp2>).
 * ---------------------------------------------------------------------------------------- */
/* The actor's policy model.  BDR_ACTOR_MLP3 (mlp/mlp3.rs): mean = Mlp(obs) and a state-independent `head2` [1, act_dim] as the
 * log-std.  BDR_ACTOR_MLP2 (mlp/mlp2.rs:33-44): a trunk of `units` with ReLU after EVERY layer (mlp.rs:14-24 with Activation::ReLU),
 * then mean = W_m h + b_m and the second output exp(W_s h + b_s), which GaussianActor clamps and exponentiates once more
 * (util/actor.rs:199-201, 228-229): std = exp(clamp(exp(s), min_log_std, max_log_std)).  Mlp2 needs n_units >= 2: the reference's
 * loop bound 0..=n_layers-2 underflows with one trunk layer (BDR_ERR_INVALID). */
enum { BDR_ACTOR_MLP3 = 0, BDR_ACTOR_MLP2 = 1 };
enum { BDR_ENT_COEF_FIX = 0, BDR_ENT_COEF_AUTO = 1 };   /* sac/ent_coef.rs:13-19 EntCoefMode::Fix(alpha) | Auto(target_entropy, lr) */

/* SacConfig (sac/config.rs:82-93) with its MultiCriticConfig (util/critic.rs:35-43) and GaussianActorConfig (util/actor.rs:44-55).
 * There is no reward_scale and there are no log-std bounds of the agent's own: the bounds are GaussianActorConfig's.  amsgrad is
 * rejected, as for IQL.  batch_size must be >= 2: at one row the squeeze(D::Minus1) of sac/base.rs:83 turns the TD target into a
 * scalar while each prediction keeps shape [1], and candle's same-shape tensor ops reject that pair (BDR_ERR_INVALID). */
typedef struct {
    int32_t obs_dim, act_dim;
    bdr_mlp_config actor;         /* GaussianActorConfig.policy_config (Mlp3 or Mlp2: actor_kind) */
    bdr_mlp_config critic;        /* MultiCriticConfig.q_config               */
    int32_t n_critics;            /* MultiCriticConfig.n_nets (default 2)     */
    double critic_tau;            /* MultiCriticConfig.tau (default 0.005)    */
    double lr_actor, lr_critic;
    bdr_adamw_config opt_actor, opt_critic;
    double min_log_std, max_log_std;  /* GaussianActorConfig (-20, 2)     */
    int32_t action_limit;             /* BDR_ACTION_LIMIT_* (default Clamp{-1, 1}) */
    double action_min, action_max, action_scale;
    double gamma;                 /* 0.99 (f32 in the reference) */
    int32_t ent_coef_mode;        /* BDR_ENT_COEF_* (default Fix(1.0), sac/config.rs:90) */
    double ent_coef_alpha;        /* Fix(alpha): log_alpha = (float)ln(alpha), never stepped */
    double target_entropy;        /* Auto(target_entropy, _), used as f32 (ent_coef.rs:73-74) */
    double ent_coef_lr;           /* Auto(_, lr): candle-nn AdamW defaults (weight decay 0.01) with this learning rate */
    int32_t actor_kind;           /* BDR_ACTOR_* (default Mlp3) */
    int32_t critic_loss;          /* BDR_LOSS_* (Mse)             */
    uint64_t n_updates_per_opt, batch_size;   /* 1, 1 (batch_size 1 is rejected, see above) */
    int32_t train;                /* false: the agent is built in eval mode (sac/base.rs:204) */
    int32_t device;               /* -1: none given */
    uint64_t seed;                /* the library's parameter initialiser and the device noise stream of Policy::sample */
} bdr_candle_sac_config;
BDR_API void bdr_candle_sac_config_default(bdr_candle_sac_config* cfg);                    /* sac/config.rs:82-93 */
BDR_API int32_t bdr_candle_sac_create(const bdr_candle_sac_config* cfg, bdr_agent** out);  /* sac/base.rs:183-210 (Configurable::build) */
/* One Sac::opt_ loop iteration (sac/base.rs:124-134) on a host minibatch: update_actor (:104-122), then update_critic (:63-102) on
 * the same batch with the already updated actor and alpha, then the soft update of every target critic (:132).
 *   update_actor: a = actor.sample(obs), logp = actor.logp(obs, a) (evaluated on the limited action: atanh(clamp(a / scale)) plus the
 *     log-Jacobian of `a` itself, util/actor.rs:196-223); EntCoef::update(logp.detach()) (ent_coef.rs:71-84; Auto only) BEFORE alpha
 *     is read; loss = mean(alpha logp - min_i Q_i(obs, a)) over the ONLINE critics.  The gradient reaches the actor through `a` (z
 *     fixed) and through the mean and std logp reads; the minimum passes it to every critic whose value equals it.
 *   update_critic: tgt = r + gamma_not_done (min_i Qtgt_i(next_obs, next_a) - alpha next_logp), gamma_not_done = (1 - is_terminated)
 *     gamma; is_truncated is NOT counted (gamma_not_done(.., None, ..), :75-76); loss = mean over critics of mse / smooth_l1.
 * Noise: in train mode z_pi / z_next are n * act_dim host N(0,1) draws for a and next_a, or NULL for the agent's device stream (the
 * one bdr_agent_draw_noise reads); each NULL set takes n * act_dim draws, z_pi's first, row-major [n][act_dim].  Host draws take
 * nothing from the stream.  Eval mode uses the means and no draws; the EntCoef steps in both modes.
 * rec3: loss_critic, loss_actor, ent_coef (alpha after this update) - the record keys of :136-146, the two losses averaged over
 * n_updates_per_opt by bdr_agent_opt_with_scalars.
 * Parameter models for bdr_agent_{get,set}_params / param_count_of: 0 actor (Mlp3: mlp.ln{k}.weight/bias ..., then head2; Mlp2: the
 * trunk's mlp.ln{k}.weight/bias, then mean.weight, mean.bias, std.weight, std.bias), 1+i critic_i, 1+n_critics+i critic_tgt_i,
 * 1+2*n_critics log_alpha [1]; +100 gradient, +200 exp_avg, +300 exp_avg_sq.  SyncModel ships model 0 (the reference has no
 * SyncModel for this agent).  Checkpoints (:244-270): actor.pt, critic.pt, critic.tgt.pt as for IQL, and ent_coef.pt (log_alpha [1]). */
BDR_API int32_t bdr_candle_sac_update_on_batch(bdr_agent* a, uint64_t n, const float* obs, const float* act, const float* next_obs,
                                               const float* reward, const int8_t* is_terminated, const int8_t* is_truncated,
                                               const float* z_pi, const float* z_next, float* rec3);
/* Parity probes: intermediates of the LAST update, to the host.  what:
 *   0 a [B][act_dim]       actor.sample(obs) (:107)                  1 logp [B]       actor.logp(obs, a) (:108)
 *   2 q_min [B]            min_i Q_i(obs, a) (:114)                  3 next_a [B][act_dim]  of the updated actor (:77)
 *   4 next_logp [B]        (:78)                                     5 tgt [B]        the TD target (:79-83)
 *   6 q_pred [n_critics][B]  Q_i(obs, act) (:71)                     7 dq_da [B][act_dim]   d q_min / d a */
BDR_API int32_t bdr_candle_sac_probe(bdr_agent* a, int32_t what, float* out, uint64_t n);
/* Policy::sample (sac/base.rs:152-167 -> util/actor.rs:226-241): train: mean + std * N(0,1) (the agent's device noise stream,
 * bdr_agent_draw_noise), eval: mean; then clamp(action_min, action_max) or action_scale * tanh. */
BDR_API int32_t bdr_candle_sac_sample(bdr_agent* a, uint64_t n, const float* obs, float* act_out);
/* the same for observation rows in HBM (row i at obs_dev + i * row_stride bytes), see bdr_agent_sample_device */
BDR_API int32_t bdr_candle_sac_sample_device(bdr_agent* a, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out);

/* ------------------------------------------------------------------------------------------
 * BC agent  (border-candle-agent/src/bc/{base.rs,config.rs,model.rs}; behaviour cloning, offline)
 * Policy = Mlp (mlp/base.rs, mlp.rs:14-24): ReLU after every layer but the last, activation_out (all four BDR_ACTIVATION_*)
 * after the last.  No critic, no target, no noise.
 * ---------------------------------------------------------------------------------------- */
enum { BDR_BC_ACTION_DISCRETE = 0, BDR_BC_ACTION_CONTINUOUS = 1 };   /* bc/config.rs BcActionType */
/* How one update is launched.  GENERAL: the last layer's forward, k_bc_loss and the last layer's input gradient as three launches
 * (any out_dim).  FUSED: k_bc_head does the three in one row-block launch; it needs act_dim <= 64, at least one hidden layer and a
 * last hidden layer of at most 384 units (its weights are staged in LDS), else bdr_bc_create returns BDR_ERR_INVALID.  FUSED_MFMA:
 * the same launch with both products on the FP32 MFMA and the weights read from L2 (k_bc_head_mfma; act_dim <= 64, a hidden layer).  DEFAULT:
 * FUSED_MFMA where it applies and batch_size <= 1024 (measured at the bc_pen shape: profiles/bench_bc_pen.json), GENERAL elsewhere. */
enum { BDR_BC_KERNEL_DEFAULT = 0, BDR_BC_KERNEL_GENERAL = 1, BDR_BC_KERNEL_FUSED = 2, BDR_BC_KERNEL_FUSED_MFMA = 3 };
/* BcConfig (bc/config.rs:66-75) with BcModelConfig (bc/model.rs): policy_model_config.{policy_model_config, opt_config}.
 * amsgrad is rejected, as for IQL. */
typedef struct {
    int32_t obs_dim, act_dim;
    bdr_mlp_config policy;        /* BcModelConfig.policy_model_config; activation_out: None / ReLU / Tanh / Sigmoid */
    bdr_adamw_config opt;         /* BcModelConfig.opt_config */
    double lr;
    uint64_t batch_size;          /* 1 */
    int32_t action_type;          /* BDR_BC_ACTION_* (Discrete) */
    int32_t device;               /* -1: none given */
    int32_t record_verbose_level; /* 0 */
    int32_t kernel_form;          /* BDR_BC_KERNEL_* (Default) */
    int32_t head_rows;            /* rows per workgroup of k_bc_head: 0 (the measured default), 8, 16 or 32 */
    int32_t reserved;
    uint64_t seed;                /* the library's parameter initialiser */
} bdr_bc_config;
BDR_API void bdr_bc_config_default(bdr_bc_config* cfg);                    /* bc/config.rs:66-75 */
BDR_API int32_t bdr_bc_create(const bdr_bc_config* cfg, bdr_agent** out);  /* bc/base.rs:126-136 (Configurable::build) */
/* One Bc::opt_ (bc/base.rs:167-198) on a host minibatch: loss = mean over all n x act_dim elements of (policy(obs) - act)^2,
 * backward, one optimizer step.  rec_out (may be NULL): 1 float, "loss".  A Discrete agent returns BDR_ERR_INVALID (the reference
 * panics, bc/base.rs:174).
 * Parameter models for bdr_agent_{get,set}_params / param_count_of: 0 the policy (mlp.ln{k}.weight, mlp.ln{k}.bias ...); +100
 * gradient, +200 exp_avg, +300 exp_avg_sq.  SyncModel ships model 0.  Checkpoint: policy_model.pt (safetensors, as candle writes it).
 * bdr_agent_set_train is accepted and bdr_agent_is_train answers false (bc/base.rs:104-112). */
BDR_API int32_t bdr_bc_update_on_batch(bdr_agent* a, uint64_t n, const float* obs, const float* act, float* rec_out);
/* Parity probes: intermediates of the LAST BC update, to the host.  what:
 *   0 pred [B][act_dim]   the network output, output activation applied     1 dz [B][act_dim]   dLoss / d(last pre-activation) */
BDR_API int32_t bdr_bc_probe(bdr_agent* a, int32_t what, float* out, uint64_t n);
/* Policy::sample (bc/base.rs:49-59).  Continuous: act_out [n][act_dim] = the network output, idx_out NULL.  Discrete: idx_out [n] =
 * argmax over the last dimension (the lowest index among equal values; candle's tie order is not pinned by anything that can be
 * run against), act_out NULL. */
BDR_API int32_t bdr_bc_sample(bdr_agent* a, uint64_t n, const float* obs, float* act_out, int64_t* idx_out);
/* the same for observation rows in HBM (row i at obs_dev + i * row_stride bytes), see bdr_agent_sample_device */
BDR_API int32_t bdr_bc_sample_device(bdr_agent* a, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out, int64_t* idx_out);

/* A GROUP of BC agents over uniform rings (or views of one ring, bdr_replay_view_create): Agent::opt of every member in 2L + 4
 * launches (general form; gather, pack, L forwards, loss, L - 1 input gradients, the grouped weight gradient, reduce + Adam) or 2L + 2
 * (the MFMA head) for L layers, whatever the number of members - the launch sequence of one member, the member index one more grid
 * dimension - bit for bit what bdr_agent_opt of the members one after the other gives.  The calls carry the semantics of their
 * bdr_agent_group_* namesakes: create adopts the members onto one stream and owns them from then on (bdr_agent_destroy of a member is
 * refused; bdr_bc_group_destroy destroys them), every bdr_agent_* / bdr_bc_* call on a member keeps its meaning and is ordered with the
 * group's calls.
 * One value for all members: obs_dim, units, act_dim, activation_out, batch_size, the resolved kernel form, action_type Continuous.
 * Free per member: optimizer kind and scalars, learning rate, seed.  Refused (BDR_ERR_INVALID, naming the first member concerned): another
 * shape, the LDS head (BDR_BC_KERNEL_FUSED), a Discrete agent, profiling or a gradient communicator switched on, another device, the
 * same agent twice, an agent that is in a group already; more than 65535 members or a launch beyond the grid limits.
 * buffers[p] is member p's: a uniform StdRng ring of f32 rows on the group's device, or a view of one.  A prioritized ring, a frame store,
 * the xoshiro stream, an empty ring (BDR_ERR_EMPTY) and one bdr_replay for two members are refused, naming the member, and a refused
 * call leaves every member's step, n_opts and stream position where they were.  _opt does not synchronise; _opt_with_scalars
 * synchronises once and returns every member's record (one key, loss) at out + p * cap_per_member.  _info fills bdr_group_info with
 * form = BDR_GROUP_FORM_BC_LAYERS. */
typedef struct bdr_bc_group bdr_bc_group;
BDR_API int32_t bdr_bc_group_create(bdr_agent* const* agents, uint32_t n, bdr_bc_group** out);
BDR_API int32_t bdr_bc_group_destroy(bdr_bc_group* g);
BDR_API int32_t bdr_bc_group_size(const bdr_bc_group* g, uint32_t* n);
BDR_API int32_t bdr_bc_group_member(const bdr_bc_group* g, uint32_t i, bdr_agent** out);
BDR_API int32_t bdr_bc_group_info(const bdr_bc_group* g, bdr_group_info* out);
BDR_API int32_t bdr_bc_group_opt(bdr_bc_group* g, bdr_replay* const* buffers);
BDR_API int32_t bdr_bc_group_opt_with_scalars(bdr_bc_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out);
BDR_API int32_t bdr_bc_group_sync(bdr_bc_group* g);

/* Policy::sample of the members of a BC group in ONE launch: the one-launch acting kernel (bdr_agent_set_act_path, BDR_ACT_PATH_FUSED)
 * with the member as one more grid dimension, one workgroup per member and block of 32 rows.  Every array is indexed by MEMBER:
 * rows[i] = n host rows of obs_dim elements of dtypes[i] (BDR_DTYPE_F32 / BDR_DTYPE_F64), norms[i] = the
 * normaliser applied to member i's rows (norms or any entry may be NULL), act_out[i] receives [n][act_dim] f32: the bits of
 * bdr_agent_sample_raw(member i, norms[i], n, rows[i], dtypes[i], 0, 0, act_out[i], NULL) on either act path.  The same n, 1 <= n <=
 * 65536, holds for every member; two members may name the same rows.  The call is synchronous and counts as one launch of the group
 * (bdr_group_info::kernel_launches); n_opts does not move.  _sample_members: only members[0..n_sel) act (strictly ascending); a member
 * that is not selected sees nothing of the call - its entries of the arrays are not read and nothing of it is written.  With every
 * member selected it enqueues what _sample enqueues.
 * Refused with BDR_ERR_INVALID before anything is enqueued, naming the member: a NULL rows[i] / act_out[i] of a selected member; an
 * empty, not strictly ascending or out-of-range member list; a normaliser that is not ready, has another dim or lives on another
 * device; an unknown dtype; a network whose widest padded layer exceeds 512 (such members keep acting standalone); rows or actions of
 * one call beyond 64 MiB (split the call). */
BDR_API int32_t bdr_bc_group_sample(bdr_bc_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows,
                                    const int32_t* dtypes, float* const* act_out);
BDR_API int32_t bdr_bc_group_sample_members(bdr_bc_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms,
                                            uint64_t n, const void* const* rows, const int32_t* dtypes, float* const* act_out);

/* (bdr_bc_group_eval_ops, bdr_evaluate_bc_group, bdr_bc_group_trainer_post and bdr_trainer_train_offline_group_post below serve BC
 * groups AND IQL groups: the structs hold a void* group and hooks, and the bdr_iql_group_*_default fillers further down fill them for
 * an IQL group.  Where the text says "a BC group", an IQL group behind its default table is served the same way.)
 * bdr_evaluate_group's rule, word for word, for a BC group: resets in member order, ONE acting call per round over the members with
 * an open episode, steps in member order, one f32 accumulator per member in call order; a member that has finished its episodes
 * leaves the selection; score and normalised score as bdr_evaluate.  Member i sees exactly the calls bdr_evaluate(&evs[i], member i)
 * makes.  The differences: actions are f32 rows - act_row_bytes must be 4 * act_dim (checked against the member by the default
 * table; a positive multiple of 4 with another table) -, obs_dtype may be BDR_DTYPE_F32 or BDR_DTYPE_F64 and norm may be set, per
 * member.  env.obs_on_device is still refused.  The hook receives the rows as the environments wrote them and the evaluators' norm
 * and obs_dtype, all indexed by member, and writes member i's action row to act_out[i]. */
typedef struct bdr_bc_group_eval_ops {
    void* group;
    uint32_t n_members;
    uint32_t reserved;
    /* bdr_bc_group_sample_members with n = 1 */
    int32_t (*sample_members)(void* group, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, const void* const* rows,
                              const int32_t* dtypes, float* const* act_out);
} bdr_bc_group_eval_ops;
BDR_API void bdr_bc_group_eval_ops_default(bdr_bc_group_eval_ops* ops, bdr_bc_group* group);
BDR_API int32_t bdr_evaluate_bc_group(const bdr_evaluator* evs, const bdr_bc_group_eval_ops* ops, bdr_eval_result* out);

/* Trainer::train_offline (trainer.rs:330-384) with Trainer::post_process (:231-264) for the members of a group in lockstep.
 * set_train(1) once; per iteration env_steps += 1, ONE group opt - opt_with_record when (opt_steps + 1) %
 * record_agent_info_interval == 0 -, the members' OPT / OPT_RECORD events in member order, post_process as bdr_group_trainer_post
 * describes it (bdr_evaluate_bc_group in place of bdr_evaluate_group), the COST event (average_opt_time only: the offline loop
 * samples nothing), stop at max_opts.  An interval of 0 means never; the timer wraps opt* only.  Member i's observer sees the event
 * sequence bdr_trainer_train_offline_post gives a lone agent.  ops->sample and ops->push are not read and may be NULL; post may be
 * NULL.  Refused before anything runs: what bdr_trainer_train_group_post refuses of c, ops and post. */
typedef struct bdr_bc_group_trainer_post {
    uint64_t eval_interval;                 /* 0 = never */
    uint64_t save_interval;                 /* 0 = never */
    const bdr_evaluator* evaluators;        /* [n_members]; needed when eval_interval > 0 */
    const char* const* model_dirs;          /* [n_members]; needed when something is saved */
    bdr_bc_group_eval_ops eval_ops;
    int32_t (*save_member)(void* group, uint32_t member, const char* dir);   /* NULL: mkdir -p + bdr_agent_save_params of the member (of an
                                                                              * IQL group when eval_ops is IQL's default table, else of a BC group) */
} bdr_bc_group_trainer_post;
/* set_train over the members, opt = bdr_bc_group_opt, opt_with_record = bdr_bc_group_opt_with_scalars; sample and push stay NULL */
BDR_API void bdr_bc_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_bc_group* group, bdr_replay* const* buffers);
BDR_API void bdr_bc_group_trainer_post_default(bdr_bc_group_trainer_post* post, bdr_bc_group* group);
BDR_API int32_t bdr_trainer_train_offline_group_post(const bdr_trainer_config* c, const bdr_group_trainer_ops* ops,
                                                     const bdr_bc_group_trainer_post* post,
                                                     void (*observer)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps,
                                                                      int32_t event, const float* scalars, int32_t n_scalars),
                                                     void* observer_ctx, bdr_trainer_stats* out);

/* Policy::sample of the members of an IQL group (bdr_iql_group, above) in ONE launch: the one-launch acting kernel (bdr_agent_set_act_path,
 * BDR_ACT_PATH_FUSED) with the member as one more grid dimension, one workgroup per member and block of 32 rows.  Every array is indexed by
 * MEMBER: rows[i] = n host rows of obs_dim elements of dtypes[i] (BDR_DTYPE_F32 / BDR_DTYPE_F64), norms[i] = the
 * normaliser applied to member i's rows (norms or any entry may be NULL), act_out[i] receives [n][act_dim] f32: the bits of
 * bdr_agent_sample_raw(member i, norms[i], n, rows[i], dtypes[i], 0, 0, act_out[i], NULL) on either act path - the bits of the member's
 * own bdr_agent_sample_raw in its current mode at its current noise counter.  The same n, 1 <= n <=
 * 65536, holds for every member; two members may name the same rows.  The call is synchronous and counts as one launch of the group
 * (bdr_group_info::kernel_launches); n_opts and the three step counters do not move.  _sample_members: only members[0..n_sel) act
 * (strictly ascending); a member that is not selected sees nothing of the call - its entries of the arrays are not read and nothing of it
 * is written or advanced.  With every member selected it enqueues what _sample enqueues.
 * Train and eval mode: each selected member's mode (bdr_agent_set_train) is read at call time, and members of one call may be in
 * different modes.  A selected member in train mode takes n * act_dim draws at its own noise counter, which then advances by n *
 * act_dim; in eval mode the counter does not move.  Group calls, the member's own sample / sample_raw on either act path and
 * bdr_agent_draw_noise therefore continue ONE stream, in any interleaving.  The call touches no member's batch buffers.
 * Refused with BDR_ERR_INVALID before anything is enqueued and before any counter moves, naming the member: a NULL rows[i] / act_out[i]
 * of a selected member; an empty, not strictly ascending or out-of-range member list; a normaliser that is not ready, has another dim
 * or lives on another device; an unknown dtype; an actor whose widest padded layer exceeds 512 (refused at the first acting call, not
 * at creation: such groups keep stepping and their members keep acting standalone); rows or actions of one call beyond 64 MiB (split
 * the call). */
BDR_API int32_t bdr_iql_group_sample(bdr_iql_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows,
                                     const int32_t* dtypes, float* const* act_out);   /* util/actor.rs:226-241 */
BDR_API int32_t bdr_iql_group_sample_members(bdr_iql_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms,
                                             uint64_t n, const void* const* rows, const int32_t* dtypes, float* const* act_out);   /* util/actor.rs:226-241 */
/* The tables of bdr_evaluate_bc_group and bdr_trainer_train_offline_group_post for an IQL group: sample_members =
 * bdr_iql_group_sample_members with n = 1 (act_row_bytes is checked against the member: 4 * act_dim); set_train over the members, opt
 * = bdr_iql_group_opt, opt_with_record = bdr_iql_group_opt_with_scalars (three keys), sample and push stay NULL; save_member = mkdir -p
 * + bdr_agent_save_params of the IQL member (actor, critic, critic.tgt, value).  Evaluation runs in eval mode inside the offline loop
 * (post_process sets it); bdr_evaluate_bc_group called directly acts in whatever mode each member is in, and a member that has
 * finished its episodes takes no draws. */
BDR_API void bdr_iql_group_eval_ops_default(bdr_bc_group_eval_ops* ops, bdr_iql_group* group);                                   /* evaluator/default_evaluator.rs:64-88 */
BDR_API void bdr_iql_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_iql_group* group, bdr_replay* const* buffers);    /* trainer.rs:330-384 */
BDR_API void bdr_iql_group_trainer_post_default(bdr_bc_group_trainer_post* post, bdr_iql_group* group);                          /* trainer.rs:231-264 */

/* A GROUP of AWAC agents (bdr_awac_create, above) over uniform rings (or views of one ring, bdr_replay_view_create): Awac::opt_
 * (awac/base.rs:170-215) of every member in the launch sequence of ONE member - gather, pack, the actor on obs, the sample of act_, the
 * online critics on (obs | act) and (obs | act_), update_actor, the updated actor on next_obs, the sample of next_act, the target
 * critics, update_critic with the soft update: 3 (Lp + Lq) + 8 launches for Lp, Lq layers (n_units + 1) of actor and critic, whatever
 * the number of members; the member index is one more grid dimension - bit for bit what bdr_agent_opt of the members one after the
 * other gives.  The calls carry the semantics of their bdr_iql_group_* namesakes (ownership, ordering with the members' own calls,
 * acting, the tables of the evaluator and the offline loop).
 * Noise: a round draws INSIDE the round.  Each member's mode (bdr_agent_set_train) is read when the round is enqueued; in train mode
 * the member takes batch_size * act_dim draws at its own noise counter for act_, then as many for next_act, in eval mode none - the
 * rule of bdr_agent_opt.  Rounds, the group's acting calls, the member's own sample / sample_raw / update_on_batch and
 * bdr_agent_draw_noise continue ONE stream, in any interleaving; members of one group may be in different modes.
 * One value for all members: obs_dim, act_dim, both networks' units and activation_out, n_critics, batch_size, the device.  Free per
 * member: seed, inv_lambda, exp_adv_max, gamma, critic_tau, adv_softmax, critic_loss, the action limit with its bounds and scale, the
 * log-std clamps, both learning rates, optimizer kinds and scalars, train / eval mode.  Refused (BDR_ERR_INVALID, naming the first
 * member concerned): a non-AWAC agent, another shape, n_critics > 2, n_critics x critic layers > 16, more than 12 reduce segments
 * (the actor's head2 is one), n_updates_per_opt != 1, profiling or a gradient communicator switched on, another device, the same agent
 * twice, an agent that is in a group already; more than 65535 members or a launch beyond the grid limits (naming the kernel).
 * buffers[p] is member p's, as for bdr_iql_group_opt, with the same refusals; a refused call leaves every member's two step counters,
 * n_opts, noise counter and stream position where they were.  _opt_with_scalars returns every member's record (the eight keys of
 * bdr_agent_record_keys; cap_per_member >= 8) at out + p * cap_per_member.  _info fills bdr_group_info with form =
 * BDR_GROUP_FORM_AWAC_LAYERS.  Not built: n_updates_per_opt > 1, n_critics > 2, Mlp2 actors, host-supplied noise rows, prioritized
 * rings under the group. */
typedef struct bdr_awac_group bdr_awac_group;
BDR_API int32_t bdr_awac_group_create(bdr_agent* const* agents, uint32_t n, bdr_awac_group** out);   /* awac/base.rs:170-215 (opt_ of every member) */
BDR_API int32_t bdr_awac_group_destroy(bdr_awac_group* g);                                           /* awac/base.rs:170-215 */
BDR_API int32_t bdr_awac_group_size(const bdr_awac_group* g, uint32_t* n);                           /* awac/base.rs:170-215 */
BDR_API int32_t bdr_awac_group_member(const bdr_awac_group* g, uint32_t i, bdr_agent** out);         /* awac/base.rs:170-215 */
BDR_API int32_t bdr_awac_group_info(const bdr_awac_group* g, bdr_group_info* out);                   /* awac/base.rs:170-215 */
BDR_API int32_t bdr_awac_group_opt(bdr_awac_group* g, bdr_replay* const* buffers);                   /* awac/base.rs:170-215 */
BDR_API int32_t bdr_awac_group_opt_with_scalars(bdr_awac_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out);   /* awac/base.rs:170-215, record :190-212 */
BDR_API int32_t bdr_awac_group_sync(bdr_awac_group* g);                                              /* awac/base.rs:170-215 */
BDR_API int32_t bdr_awac_group_sample(bdr_awac_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows,
                                      const int32_t* dtypes, float* const* act_out);   /* awac/base.rs:228-233, util/actor.rs:226-241 */
BDR_API int32_t bdr_awac_group_sample_members(bdr_awac_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms,
                                              uint64_t n, const void* const* rows, const int32_t* dtypes, float* const* act_out);   /* awac/base.rs:228-233, util/actor.rs:226-241 */
/* the tables of bdr_evaluate_bc_group and bdr_trainer_train_offline_group_post for an AWAC group, as bdr_iql_group_*_default (eight
 * record keys; save_member writes actor, critic, critic.tgt) */
BDR_API void bdr_awac_group_eval_ops_default(bdr_bc_group_eval_ops* ops, bdr_awac_group* group);                                   /* awac/base.rs:228-233, evaluator/default_evaluator.rs:64-88 */
BDR_API void bdr_awac_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_awac_group* group, bdr_replay* const* buffers);    /* awac/base.rs:170-215, trainer.rs:330-384 */
BDR_API void bdr_awac_group_trainer_post_default(bdr_bc_group_trainer_post* post, bdr_awac_group* group);                          /* awac/base.rs:311-319, trainer.rs:231-264 */

/* ExperienceBufferBase::push (generic_replay_buffer/base.rs:279-313) of n transitions per member of an AWAC group, member i's into
 * buffers[i] at its head, in ONE launch and without a copy command whatever the number of members and n are.  Every array is indexed
 * by member and holds n rows: obs[i] / next_obs[i] = n rows of obs_dim elements of obs_dtypes[i] (BDR_DTYPE_F32 / BDR_DTYPE_F64;
 * obs_dtypes == NULL: all BDR_DTYPE_F32), act[i] = [n][act_dim] f32, reward[i] = [n] f32, the flags [n] i8.  Each ring ends up exactly
 * as bdr_replay_push(buffers[i], n, ...) of the same rows as float32 leaves it: the same bytes in the same rows (row j at (head + j) %
 * capacity: a push may cross the wrap), head advanced by n modulo capacity, size saturating at capacity, summary counters and index
 * stream untouched in the same way.  float64 rows are converted on the device by one round-to-nearest-even cast per element - the
 * bits of a C (float) cast / numpy astype(float32), and the cast bdr_awac_group_sample applies to the same rows with norms == NULL, so
 * acting and storing agree; no normaliser is applied (the ring stores what the reference's step processor stores,
 * generic_replay_buffer/step_proc.rs:103-137).
 * The rows are staged in a slot of a pinned push ring of the group (8 slots of 64 KiB) that the kernel reads in place: the call
 * returns once the caller's rows are staged - its arrays are free - and does not synchronise.  It runs on the group's stream: the
 * group's later rounds and acting calls are ordered behind it by their queue, calls on a ring's own stream (bdr_replay_push,
 * bdr_replay_batch, ...) order themselves through the ring's event.  It counts as one launch in bdr_group_info::kernel_launches.
 * Bounds: 1 <= n, and 80 bytes per member plus the n records of every member fit one slot (a record is the ring's own record rounded
 * up to 16 bytes; with float64 rows its two observation rows take twice their bytes); _push_max_rows returns the largest such n for
 * these rings and dtypes.  A larger call is refused with a message that says to split it.
 * Refused with BDR_ERR_INVALID before anything moves - every ring's head, size and rows, every slot and the launch counter stay where
 * they were -, naming the member: a NULL buffer or row pointer; n outside its bounds; an unknown dtype; a ring on another device; a
 * view, or a ring with live views; a prioritized ring, a single-frame store or an xoshiro256++ ring; observation rows that are not
 * 4 * obs_dim bytes or action rows that are not 4 * act_dim bytes; two members naming one ring.
 * Not built: acting on next_obs inside the push launch, a normaliser inside the push, prioritized rings. */
BDR_API int32_t bdr_awac_group_push(bdr_awac_group* g, bdr_replay* const* buffers, uint64_t n, const void* const* obs, const void* const* next_obs,
                                    const int32_t* obs_dtypes, const float* const* act, const float* const* reward,
                                    const int8_t* const* is_terminated, const int8_t* const* is_truncated);   /* generic_replay_buffer/base.rs:279-313 */
BDR_API int32_t bdr_awac_group_push_max_rows(bdr_awac_group* g, bdr_replay* const* buffers, const int32_t* obs_dtypes, uint64_t* n_max);   /* generic_replay_buffer/base.rs:279-313 */

/* A GROUP of candle SAC agents (bdr_candle_sac_create, above) over uniform rings (or views of one ring, bdr_replay_view_create):
 * Sac::opt_ (sac/base.rs:124-134) of every member in the launch sequence of ONE member - gather, pack, the actor on obs, sample + logp
 * of a, the entropy coefficient's step, the online critics on (obs | act) and (obs | a), qmin, the critics' input gradients down to
 * dq/da, update_actor, the updated actor on next_obs, sample + logp of next_a, the target critics, update_critic with the soft update:
 * 3 Lp + 4 Lq + 10 launches for Lp, Lq layers (n_units + 1) of actor and critic, whatever the number of members; the member index is
 * one more grid dimension - bit for bit what bdr_agent_opt of the members one after the other gives.  The calls carry the semantics
 * of their bdr_iql_group_* namesakes (ownership, ordering with the members' own calls, acting, the tables of the evaluator and the
 * offline loop).  The members are online agents: bdr_candle_sac_group_push (below) stores n transitions per member in one launch, and a
 * member's own bdr_replay_push between rounds keeps working.
 * Noise: as for a bdr_awac_group - each member's mode is read when the round is enqueued; in train mode the member takes batch_size *
 * act_dim draws at its own noise counter for a, then as many for next_a, in eval mode none.  Rounds, the group's acting calls, the
 * member's own sample / sample_raw / update_on_batch and bdr_agent_draw_noise continue ONE stream, in any interleaving.
 * One value for all members: obs_dim, act_dim, both networks' units and activation_out, actor_kind (Mlp2 or Mlp3), n_critics,
 * batch_size, the device.  Free per member: seed, gamma, critic_tau, critic_loss, the entropy mode (Fix(alpha) or Auto(target_entropy,
 * lr)), the action limit with its bounds and scale, the log-std clamps, both learning rates, optimizer kinds and scalars, train /
 * eval mode.  Refused (BDR_ERR_INVALID, naming the first member concerned): a non-candle_sac agent, another shape or actor kind,
 * n_critics > 2, n_critics x critic layers > 16, more than 12 reduce segments (an Mlp3 actor's head2 is one), n_updates_per_opt != 1,
 * profiling or a gradient communicator switched on, another device, the same agent twice, an agent that is in a group already; more
 * than 65535 members or a launch beyond the grid limits (naming the kernel).
 * buffers[p] is member p's, as for bdr_iql_group_opt, with the same refusals; a refused call leaves every member's three step
 * counters, n_opts, noise counter and stream position where they were.  _opt_with_scalars returns every member's record (the three
 * keys of bdr_agent_record_keys; cap_per_member >= 3) at out + p * cap_per_member.  _info fills bdr_group_info with form =
 * BDR_GROUP_FORM_CANDLE_SAC_LAYERS.  Not built: n_updates_per_opt > 1, n_critics > 2, host-supplied noise rows, a captured graph of
 * the round, prioritized rings under the group. */
typedef struct bdr_candle_sac_group bdr_candle_sac_group;
BDR_API int32_t bdr_candle_sac_group_create(bdr_agent* const* agents, uint32_t n, bdr_candle_sac_group** out);   /* sac/base.rs:124-134 (opt_ of every member) */
BDR_API int32_t bdr_candle_sac_group_destroy(bdr_candle_sac_group* g);                                           /* sac/base.rs:124-134 */
BDR_API int32_t bdr_candle_sac_group_size(const bdr_candle_sac_group* g, uint32_t* n);                           /* sac/base.rs:124-134 */
BDR_API int32_t bdr_candle_sac_group_member(const bdr_candle_sac_group* g, uint32_t i, bdr_agent** out);         /* sac/base.rs:124-134 */
BDR_API int32_t bdr_candle_sac_group_info(const bdr_candle_sac_group* g, bdr_group_info* out);                   /* sac/base.rs:124-134 */
BDR_API int32_t bdr_candle_sac_group_opt(bdr_candle_sac_group* g, bdr_replay* const* buffers);                   /* sac/base.rs:124-134 */
BDR_API int32_t bdr_candle_sac_group_opt_with_scalars(bdr_candle_sac_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out);   /* sac/base.rs:124-134, record :136-146 */
BDR_API int32_t bdr_candle_sac_group_sync(bdr_candle_sac_group* g);                                              /* sac/base.rs:124-134 */
BDR_API int32_t bdr_candle_sac_group_sample(bdr_candle_sac_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows,
                                            const int32_t* dtypes, float* const* act_out);   /* sac/base.rs:162-167, util/actor.rs:226-241 */
BDR_API int32_t bdr_candle_sac_group_sample_members(bdr_candle_sac_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms,
                                                    uint64_t n, const void* const* rows, const int32_t* dtypes, float* const* act_out);   /* sac/base.rs:162-167, util/actor.rs:226-241 */
/* the tables of bdr_evaluate_bc_group and bdr_trainer_train_offline_group_post for a candle SAC group, as bdr_iql_group_*_default
 * (three record keys; save_member writes actor, critic, critic.tgt, ent_coef) */
BDR_API void bdr_candle_sac_group_eval_ops_default(bdr_bc_group_eval_ops* ops, bdr_candle_sac_group* group);                                   /* sac/base.rs:162-167, evaluator/default_evaluator.rs:64-88 */
BDR_API void bdr_candle_sac_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_candle_sac_group* group, bdr_replay* const* buffers);    /* sac/base.rs:124-134, trainer.rs:330-384 */
BDR_API void bdr_candle_sac_group_trainer_post_default(bdr_bc_group_trainer_post* post, bdr_candle_sac_group* group);                          /* sac/base.rs:244-270, trainer.rs:231-264 */
/* bdr_awac_group_push / _push_max_rows for a candle SAC group: the same call, word for word */
BDR_API int32_t bdr_candle_sac_group_push(bdr_candle_sac_group* g, bdr_replay* const* buffers, uint64_t n, const void* const* obs,
                                          const void* const* next_obs, const int32_t* obs_dtypes, const float* const* act, const float* const* reward,
                                          const int8_t* const* is_terminated, const int8_t* const* is_truncated);   /* generic_replay_buffer/base.rs:279-313 */
BDR_API int32_t bdr_candle_sac_group_push_max_rows(bdr_candle_sac_group* g, bdr_replay* const* buffers, const int32_t* obs_dtypes, uint64_t* n_max);   /* generic_replay_buffer/base.rs:279-313 */

/* Trainer::train (trainer.rs:267-327) with Trainer::post_process (:231-264) for the members of an AWAC or a candle SAC group in
 * lockstep: bdr_trainer_train_group_post's rule, word for word - ONE group sample on the members' prev_obs rows, step_with_reset of
 * every environment in member order, ONE group push of (prev_obs, act, obs, reward, flags), prev_obs = init_obs / obs per member,
 * train_step's rule once (env_steps, warm-up, opt_interval, opt vs opt_with_record and the stop at max_opts are shared decisions), the
 * members' events in member order, post_process, the cost record - and the same loop body in the library.  Member i sees exactly the
 * calls bdr_trainer_train_post makes for a lone agent on envs[i]: acting in train mode advances its noise counter by act_dim per
 * iteration, the evaluation inside post_process runs in eval mode and returns to train mode.  The differences:
 *   actions   are f32 rows: c->act_row_bytes must be a positive multiple of 4, and 4 * act_dim of the members with a default table;
 *   dtypes    obs_dtypes[i] (BDR_DTYPE_F32 / BDR_DTYPE_F64; NULL: all F32) comes with obs_row_bytes[i]: the environments write rows
 *             of that dtype (with a default table obs_row_bytes[i] must be obs_dim elements of it), and the same host rows go to the
 *             group's acting call (n = 1, norms NULL) and to the grouped push (n = 1);
 *   post      is a bdr_bc_group_trainer_post (bdr_evaluate_bc_group, save_member), filled by bdr_*_group_trainer_post_default; with
 *             post == NULL it is the plain loop.
 * Environments with obs_on_device are refused.  Not built: obs_on_device environments, n_updates_per_opt > 1. */
typedef struct bdr_cgroup_trainer_ops {
    void* group;
    void* const* buffers;                   /* [n_members] */
    uint32_t n_members;
    uint32_t reserved;
    int32_t (*set_train)(void* group, int32_t train);                                             /* Agent::train of every member */
    /* Policy::sample, one row of dtypes[i] per member; act_out[i] receives member i's f32 action row */
    int32_t (*sample)(void* group, const void* const* rows, const int32_t* dtypes, float* const* act_out);
    /* one transition per member; every array is indexed by member */
    int32_t (*push)(void* group, void* const* buffers, const void* const* rows, const void* const* next_rows, const int32_t* dtypes,
                    const float* const* act, const float* const* reward, const int8_t* const* is_terminated, const int8_t* const* is_truncated);
    int32_t (*opt)(void* group, void* const* buffers);                                            /* Agent::opt of every member */
    /* member i's Record scalars in scalars[i * cap_per_member ...], their count in n_scalars[i] */
    int32_t (*opt_with_record)(void* group, void* const* buffers, float* scalars, int32_t cap_per_member, int32_t* n_scalars);
} bdr_cgroup_trainer_ops;
/* the bdr_<kind>_group_* entries on a group and its members' rings (`buffers` must stay alive while `ops` is used): sample =
 * _sample with n = 1 and norms NULL, push = _push with n = 1 */
BDR_API void bdr_awac_group_ctrainer_ops_default(bdr_cgroup_trainer_ops* ops, bdr_awac_group* group, bdr_replay* const* buffers);               /* trainer.rs:267-327, trainer/sampler.rs:99-144 */
BDR_API void bdr_candle_sac_group_ctrainer_ops_default(bdr_cgroup_trainer_ops* ops, bdr_candle_sac_group* group, bdr_replay* const* buffers);   /* trainer.rs:267-327, trainer/sampler.rs:99-144 */
BDR_API int32_t bdr_trainer_train_cgroup_post(const bdr_trainer_config* c, const uint64_t* obs_row_bytes, const int32_t* obs_dtypes,
                                              const bdr_cgroup_trainer_ops* ops, const bdr_env_vtable* envs, const bdr_bc_group_trainer_post* post,
                                              void (*observer)(void* ctx, uint32_t member, uint64_t env_steps, uint64_t opt_steps,
                                                               int32_t event, const float* scalars, int32_t n_scalars),
                                              void* observer_ctx, bdr_trainer_stats* out);   /* trainer.rs:267-327, :231-264 */

/* ------------------------------------------------------------------------------------------
 * DQN agent of border-candle-agent  (border-candle-agent/src/dqn/{base.rs,config.rs,explorer.rs,model.rs}; online RL)
 * Not the bdr_dqn_* agent above, which restates border-tch-agent/src/dqn.  Q-network = Mlp (mlp/base.rs, mlp.rs:14-24): ReLU after
 * every layer but the last, activation_out after the last; variables mlp.ln{i}.weight [out][in] / .bias.  The AtariCnn Q-network of
 * the candle crate (atari_cnn/base.rs) is the second form of this agent: bdr_candle_dqn_cnn_config below.
 * ---------------------------------------------------------------------------------------- */
/* DqnConfig (dqn/config.rs:25-47; defaults :75-102) with DqnModelConfig (dqn/model.rs:20-39: q_config, opt_config) plus obs_dim,
 * n_actions and record_verbose_level's integer.  clip_reward and clip_td_err are carried and unused: nothing in dqn/base.rs reads
 * them (`_clip_reward`, :40; clip_td_err only inside the commented-out prioritized loss, :138-152), and is_truncated is dropped when
 * the batch is unpacked (:62).  amsgrad is rejected, as for IQL.  explorer: DqnExplorer (dqn/explorer.rs), default Softmax; its seed
 * is the seed of the agent's SmallRng, 42 in the reference (dqn/base.rs:274) and by default here. */
typedef struct {
    int32_t obs_dim, n_actions;
    bdr_mlp_config qnet;            /* DqnModelConfig.q_config (MlpConfig); activation_out None / ReLU */
    bdr_adamw_config opt;           /* DqnModelConfig.opt_config */
    double lr;
    uint64_t soft_update_interval;  /* 1 */
    uint64_t n_updates_per_opt;     /* 1 */
    uint64_t batch_size;            /* 1 */
    double discount_factor;         /* 0.99, used as f32 (dqn/base.rs:113) */
    double tau;                     /* 0.005 */
    int32_t train;                  /* false */
    int32_t double_dqn;             /* false */
    bdr_explorer_config explorer;   /* Softmax; seed 42 */
    int32_t has_clip_reward;        /* clip_reward: None - carried, unused */
    int32_t has_clip_td_err;        /* clip_td_err: None - carried, unused */
    double clip_reward;
    double clip_td_err_min, clip_td_err_max;
    int32_t critic_loss;            /* BDR_LOSS_* (Mse) */
    int32_t record_verbose_level;   /* 0 */
    int32_t device;                 /* -1: none given ("No device is given for DQN agent", dqn/base.rs:245-248) */
    int32_t ckpt_format;            /* BDR_CKPT_TCH: qnet.pt / qnet_tgt.pt (safetensors, as candle writes them); BDR_CKPT_SAFETENSORS: *.safetensors */
    uint64_t seed;                  /* the library's parameter initialiser */
} bdr_candle_dqn_config;
BDR_API void bdr_candle_dqn_config_default(bdr_candle_dqn_config* cfg);                    /* dqn/config.rs:75-102 */
BDR_API int32_t bdr_candle_dqn_create(const bdr_candle_dqn_config* cfg, bdr_agent** out);  /* dqn/base.rs:244-276 (Configurable::build): track(tau = 1) once */
/* One Dqn::update_critic (dqn/base.rs:59-170) on a host minibatch, then the bookkeeping of opt_ (:180-186: the soft update when the
 * counter of OPTS reaches soft_update_interval, n_opts += 1).  pred = Q(obs)[act]; q = Q_tgt(next_obs)[argmax Q(next_obs)] (double_dqn,
 * the ONLINE net's first maximum) or max_j Q_tgt(next_obs)[j]; tgt = reward + (((1 - is_terminated) * (f32)gamma) * q); loss = mse or
 * smooth_l1 (util.rs:144-152).  act: int64 [n], one action index per row; an index outside [0, n_actions) touches nothing out of
 * bounds and is reported by this call, by bdr_agent_sync and by the poll of bdr_agent_opt; the flagged update and every update enqueued
 * until the report take no optimizer step and no soft update, and n_opts, the Adam step number and the soft-update counter go back
 * to what was applied (an opt counts when all its updates were applied).  is_truncated may be NULL: it is read by nothing (:62).
 * rec (may be NULL): loss and, with record_verbose_level >= 2, pred_mean, reward_mean, tgt_mean, tgt_minus_pred_mean (:88-133).
 * Parameter models for bdr_agent_{get,set}_params / param_count_of: 0 qnet, 1 qnet_tgt, 2 exp_avg, 3 exp_avg_sq, 4 the last gradient
 * (also +100 gradient, +200 exp_avg, +300 exp_avg_sq of model 0, as for the other dense agents).  SyncModel is unimplemented!() in the
 * reference (:380-392); the generic arena path ships model 0.  Checkpoints (:337-351): qnet.pt, qnet_tgt.pt.
 * bdr_agent_opt on a prioritized ring returns BDR_ERR_INVALID: the reference panics on a weighted batch (dqn/base.rs:135-137).
 * Record of bdr_agent_opt_with_scalars (:307-331): the keys above of the LAST update of the opt (Record::merge), with
 * record_verbose_level >= 2 `<var>_mean` / `<var>_std` of every qnet variable, then ratio_best_act, which resets both counters. */
BDR_API int32_t bdr_candle_dqn_update_on_batch(bdr_agent* a, uint64_t n, const float* obs, const int64_t* act, const float* next_obs,
                                               const float* reward, const int8_t* is_terminated, const int8_t* is_truncated,
                                               bdr_dqn_record* rec);
/* Parity probes: intermediates of the LAST update, to the host, each [B] floats.  what:
 *   0 pred   Q(obs)[act] (:80-86)                    1 q_next  the gathered target value (:101-111)
 *   2 y      the argmax index as a float (:103, :108)  3 tgt   the TD target (:113)
 *   4 dpred  dLoss / dpred, 1/B included (the gradient of the output itself: an output ReLU's mask is applied behind it) */
BDR_API int32_t bdr_candle_dqn_probe(bdr_agent* a, int32_t what, float* out, uint64_t n);
/* ---- the same agent with the candle crate's AtariCnn Q-network (border-candle-agent/src/atari_cnn/base.rs:31-45) ----
 * conv1 8x8/4 (n_stack -> 32), conv2 4x4/2 (-> 64), conv3 3x3/1 (-> 64), ReLU after each, flatten (c, h, w), l1 3136 -> 512, ReLU,
 * l2 512 -> out_dim.  Observation rows are u8, 84 * 84 * n_stack bytes ([n_stack][84][84]; the reference's [B, n_stack, 1, 84, 84]
 * squeezed), scaled by 1/255 inside conv1.  Variables at the root of qnet.pt / qnet_tgt.pt: c1.weight [32][n_stack][8][8], c1.bias,
 * c2.weight [64][32][4][4], c2.bias, c3.weight [64][64][3][3], c3.bias, l1.weight [512][3136], l1.bias, l2.weight [out_dim][512],
 * l2.bias - also the order of the parameter models (0 qnet, 1 qnet_tgt, 2 exp_avg, 3 exp_avg_sq, 4 gradient; +100 / +200 / +300).
 * The fields are those of bdr_candle_dqn_config with AtariCnnConfig's n_stack / out_dim / skip_linear in place of obs_dim / qnet.
 * skip_linear != 0 is refused (Dqn needs out_dim action values).  arithmetic: BDR_ARITH_F32_EXACT only (conv1 on the bf16 MFMA with
 * exact u8 operands, every other product f32 x f32); BDR_ARITH_BF16X3_6 is refused - the split-operand forward belongs to the tch
 * agent.  Everything said about bdr_candle_dqn_config's agent holds: update order, records, explorers on the SmallRng, the
 * out-of-range action rule (no parameter of the update steps, conv layers included), checkpoints.  bdr_agent_opt reads a u8 ring
 * (obs_bytes = 84 * 84 * n_stack, act_bytes = 8; a frame-stack store is accepted); an f32 ring, another row size, another device or
 * a prioritized ring returns BDR_ERR_INVALID.  bdr_agent_sample / _qvalues take u8 host rows, the _device forms rows such as
 * bdr_atari_prep_device_stacks'; BDR_ACT_PATH_FUSED and bdr_agent_sample_raw return BDR_ERR_INVALID for this network. */
typedef struct {
    int32_t n_stack;                /* AtariCnnConfig.n_stack: 1 ... 8 */
    int32_t out_dim;                /* AtariCnnConfig.out_dim = the number of actions */
    int32_t skip_linear;            /* AtariCnnConfig.skip_linear: must be 0 */
    int32_t arithmetic;             /* BDR_ARITH_F32_EXACT */
    bdr_adamw_config opt;           /* DqnModelConfig.opt_config */
    double lr;
    uint64_t soft_update_interval;  /* 1 */
    uint64_t n_updates_per_opt;     /* 1 */
    uint64_t batch_size;            /* 1 */
    double discount_factor;         /* 0.99, used as f32 */
    double tau;                     /* 0.005 */
    int32_t train;                  /* false */
    int32_t double_dqn;             /* false */
    bdr_explorer_config explorer;   /* Softmax; seed 42 */
    int32_t has_clip_reward;        /* carried, unused */
    int32_t has_clip_td_err;        /* carried, unused */
    double clip_reward;
    double clip_td_err_min, clip_td_err_max;
    int32_t critic_loss;            /* BDR_LOSS_* (Mse) */
    int32_t record_verbose_level;   /* 0 */
    int32_t device;                 /* -1: none given */
    int32_t ckpt_format;            /* BDR_CKPT_TCH: qnet.pt / qnet_tgt.pt (safetensors); BDR_CKPT_SAFETENSORS: *.safetensors */
    uint64_t seed;                  /* the library's parameter initialiser */
} bdr_candle_dqn_cnn_config;
BDR_API void bdr_candle_dqn_cnn_config_default(bdr_candle_dqn_cnn_config* cfg);   /* n_stack 4, out_dim 0, F32_EXACT; the rest as bdr_candle_dqn_config_default */
BDR_API int32_t bdr_candle_dqn_cnn_create(const bdr_candle_dqn_cnn_config* cfg, bdr_agent** out);
/* bdr_candle_dqn_update_on_batch for this form: obs / next_obs are u8 rows [n][84 * 84 * n_stack].  bdr_candle_dqn_probe serves both
 * forms; bdr_candle_dqn_update_on_batch (f32 rows) returns BDR_ERR_INVALID on this one and this call on the Mlp form. */
BDR_API int32_t bdr_candle_dqn_cnn_update_on_batch(bdr_agent* a, uint64_t n, const uint8_t* obs, const int64_t* act, const uint8_t* next_obs,
                                                   const float* reward, const int8_t* is_terminated, const int8_t* is_truncated,
                                                   bdr_dqn_record* rec);
/* Policy::sample (dqn/base.rs:202-230) goes through bdr_agent_sample / _sample_device / _sample_raw (idx_out) and the action values
 * through bdr_agent_qvalues / _qvalues_device.  The exploration stream of this kind is the reference's SmallRng (xoshiro256++ seeded
 * by rand_core's seed_from_u64; DESIGN.md 17 states the rules, which nothing here can pin against rand itself):
 *   train, Softmax (explorer.rs:31-40):        per row WeightedIndex<f32> over softmax(q_row); a NaN row returns BDR_ERR_INVALID
 *   train, EpsilonGreedy (explorer.rs:79-133): eps in f64, r = gen::<f32>(), random iff r < (f32)eps, n_calls += 1; random: per row
 *                                              gen::<u64>() % A; n_samples_best_act counts only with record_verbose_level >= 2
 *   eval (dqn/base.rs:221-227):                gen::<f32>() < 0.01 ? ONE gen_range(0..A), written to every row : argmax per row
 * bdr_agent_set_explorer rewinds the stream to its seed. */

/* A GROUP of candle DQN agents in the Mlp form (bdr_candle_dqn_create, above) over uniform rings with 8-byte action rows (or views of
 * one ring, bdr_replay_view_create): Dqn::opt_ (dqn/base.rs:172-189) of every member in the launch sequence of ONE member - gather,
 * pack, the L forward layers (the passes (qnet, obs), (qnet_tgt, next_obs) and - double_dqn - (qnet, next_obs) are the 2 or 3
 * instances of one launch per layer), update_critic's TD launch (dqn/base.rs:59-170), the L - 1 input gradients, the grouped weight
 * gradient, reduce + Adam with the soft update on the rounds a member tracks (:180-184): 2 L + 4 launches for L = n_units + 1 layers,
 * whatever the number of members; the member index is one more grid dimension - bit for bit what bdr_agent_opt of the members one
 * after the other gives: parameters, target, moments, records, probes, actions, explorer stream, counters, ring bytes, saved files.
 * The calls carry the semantics of their bdr_candle_sac_group_* namesakes (ownership, ordering with the members' own calls, the slot
 * rule, the grouped push).
 * One value for all members: obs_dim, n_actions, the Q-network's units and activation_out, batch_size, double_dqn, the device.  Free
 * per member: seed, explorer and its parameters, train / eval mode, optimizer kind and scalars, learning rate, discount_factor, tau,
 * soft_update_interval, critic_loss, record_verbose_level, act path.  Refused (BDR_ERR_INVALID, naming the first member concerned):
 * an agent that is not a candle_dqn, the AtariCnn form, n_updates_per_opt != 1, another shape, more layers than one grouped
 * weight-gradient launch (16) or one reduce + Adam launch (12 segments) holds, profiling or a gradient communicator switched on,
 * another device, the same agent twice, an agent that is in a group already; more than 65535 members or a launch beyond the grid
 * limits (naming the kernel).
 * buffers[p] is member p's: a uniform f32 ring or view with 4 * obs_dim byte observation rows and 8-byte action rows on the group's
 * device; a prioritized ring, a frame-stack store, a ring on another device or one listed twice is refused before anything moves,
 * naming the member, and leaves every member's step, n_opts, soft_update_counter and stream position where they were.
 * An out-of-range action in a member's batch (dqn/base.rs:80-86: the reference's gather raises) is clamped on the device and skips
 * THAT member's optimizer step and soft update; the other members step.  _sync, _opt_with_scalars and a member's own synchronising
 * calls put the member's step, n_opts and soft_update_counter back, as the lone agent's do, and report it as "member <p>: ..." with
 * the lone agent's status.  _opt_with_scalars returns every member's opt_with_record record (dqn/base.rs:307-331: loss, at
 * record_verbose_level >= 2 the four means and the parameter statistics, then ratio_best_act and the reset of both counters) at
 * out + p * cap_per_member.  _info fills bdr_group_info with form = BDR_GROUP_FORM_CANDLE_DQN_LAYERS.
 * Not built: the AtariCnn form, n_updates_per_opt > 1, bdr_*_group_copy_members and bdr_agent_hyper_* for this kind, a captured graph
 * of the round, an explorer on the device, prioritized rings under the group. */
typedef struct bdr_candle_dqn_group bdr_candle_dqn_group;
BDR_API int32_t bdr_candle_dqn_group_create(bdr_agent* const* agents, uint32_t n, bdr_candle_dqn_group** out);   /* dqn/base.rs:172-189 (opt_ of every member) */
BDR_API int32_t bdr_candle_dqn_group_destroy(bdr_candle_dqn_group* g);                                           /* dqn/base.rs:172-189 */
BDR_API int32_t bdr_candle_dqn_group_size(const bdr_candle_dqn_group* g, uint32_t* n);                           /* dqn/base.rs:172-189 */
BDR_API int32_t bdr_candle_dqn_group_member(const bdr_candle_dqn_group* g, uint32_t i, bdr_agent** out);         /* dqn/base.rs:172-189 */
BDR_API int32_t bdr_candle_dqn_group_info(const bdr_candle_dqn_group* g, bdr_group_info* out);                   /* dqn/base.rs:172-189 */
BDR_API int32_t bdr_candle_dqn_group_opt(bdr_candle_dqn_group* g, bdr_replay* const* buffers);                   /* dqn/base.rs:172-189, :59-170 */
BDR_API int32_t bdr_candle_dqn_group_opt_with_scalars(bdr_candle_dqn_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out);   /* dqn/base.rs:307-331 */
BDR_API int32_t bdr_candle_dqn_group_sync(bdr_candle_dqn_group* g);                                              /* dqn/base.rs:172-189 */
/* Policy::sample (dqn/base.rs:202-230) of every member (_sample) or of the members of a strictly ascending list (_sample_members)
 * on n host rows each (float32 or float64 per member, an optional normaliser per member) in ONE launch: the Q rows and each row's
 * first maximum come back, then every selected member's own explorer (dqn/explorer.rs:31-40, :79-133; eval: dqn/base.rs:221-227)
 * runs on the host in member order, exactly as after the member's own bdr_agent_sample_raw: the Softmax explorer reads the Q rows,
 * epsilon-greedy and eval mode the indices; n_samples_act, n_samples_best_act and the epsilon counter move as they do alone.  A member
 * that is not selected draws nothing.  act_out[p]: member p's n explored i64 actions.  Group calls, rounds and a member's own
 * bdr_agent_sample* calls continue ONE explorer stream.  One difference from a lone member's call: bdr_agent_sample_raw reads the
 * member's device error words between the forward pass and the explorer, so a pending error (an action clamped in an earlier round)
 * stops the lone call before it draws; a group acting call does not read them - P synchronising reads would undo the one launch -
 * and draws; the error surfaces at the next _sync, _opt_with_scalars or call of the member's own, as it does for rounds.
 * _last_q is a test and diagnostic helper, not part of the reference's surface: it copies the n * n_actions action values the last
 * group call that selected `member` brought back for it (the rows its explorer read). */
BDR_API int32_t bdr_candle_dqn_group_sample(bdr_candle_dqn_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows,
                                            const int32_t* dtypes, int64_t* const* act_out);   /* dqn/base.rs:202-230, dqn/explorer.rs:31-40, :79-133 */
BDR_API int32_t bdr_candle_dqn_group_sample_members(bdr_candle_dqn_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms,
                                                    uint64_t n, const void* const* rows, const int32_t* dtypes, int64_t* const* act_out);   /* dqn/base.rs:202-230, dqn/explorer.rs:31-40, :79-133 */
BDR_API int32_t bdr_candle_dqn_group_last_q(const bdr_candle_dqn_group* g, uint32_t member, float* q_out, uint64_t n_floats);   /* dqn/base.rs:203 */
/* bdr_awac_group_push / _push_max_rows for a candle DQN group: the same call, with ONE i64 action per row (act[p]: n indices) */
BDR_API int32_t bdr_candle_dqn_group_push(bdr_candle_dqn_group* g, bdr_replay* const* buffers, uint64_t n, const void* const* obs,
                                          const void* const* next_obs, const int32_t* obs_dtypes, const int64_t* const* act, const float* const* reward,
                                          const int8_t* const* is_terminated, const int8_t* const* is_truncated);   /* generic_replay_buffer/base.rs:279-313 */
BDR_API int32_t bdr_candle_dqn_group_push_max_rows(bdr_candle_dqn_group* g, bdr_replay* const* buffers, const int32_t* obs_dtypes, uint64_t* n_max);   /* generic_replay_buffer/base.rs:279-313 */
/* the i64-action tables of bdr_evaluate_group, bdr_trainer_train_group and bdr_trainer_train_group_post over a candle DQN group:
 * sample = _sample with n = 1 float32 row per member and norms NULL, push = _push with n = 1; _trainer_post_default fills eval_ops
 * and save_member (mkdir -p + bdr_agent_save_params of the member: qnet.pt, qnet_tgt.pt, dqn/base.rs:337-351) */
BDR_API void bdr_candle_dqn_group_trainer_ops_default(bdr_group_trainer_ops* ops, bdr_candle_dqn_group* group, bdr_replay* const* buffers);   /* trainer.rs:267-327, trainer/sampler.rs:99-144 */
BDR_API void bdr_candle_dqn_group_eval_ops_default(bdr_group_eval_ops* ops, bdr_candle_dqn_group* group);                                     /* evaluator/default_evaluator.rs:64-88 */
BDR_API void bdr_candle_dqn_group_trainer_post_default(bdr_group_trainer_post* post, bdr_candle_dqn_group* group);                            /* dqn/base.rs:337-351, trainer.rs:231-264 */

/* ---- acting of the dense-agent agents (IQL, AWAC, the candle SAC, BC, the candle DQN) ----------------------------------------------------------------------
 * Their Policy::sample has two forms that produce the same bits: the layer-by-layer path (pack, one launch per layer, the sample
 * kernel) and k_dense_act (csrc/dense_act.hpp), one launch from the raw rows to the action.  bdr_{iql,awac,bc}_sample[_device] and
 * bdr_agent_sample_raw obey the setting.  FUSED on an agent kind or a network it does not cover (a padded layer wider than 512)
 * returns BDR_ERR_INVALID with the reason.  DEFAULT is the layer path. */
#define BDR_ACT_PATH_DEFAULT 0
#define BDR_ACT_PATH_LAYERS 1
#define BDR_ACT_PATH_FUSED 2
BDR_API int32_t bdr_agent_set_act_path(bdr_agent* a, int32_t path);
/* Policy::sample on n raw environment rows of `dtype` (BDR_DTYPE_F32 / _F64): host rows, contiguous, or (on_device != 0) device rows
 * row_stride bytes apart.  float64 is rounded to f32; with a normaliser (finished or set, dim = the agent's obs dim, on the agent's
 * device) the value that enters the first layer has the bits of bdr_obs_norm_apply.  act_out [n][act_dim]; idx_out [n] for a
 * Discrete BC agent and for the candle DQN (the explored i64 actions; then act_out may be NULL), else NULL.  IQL, AWAC, the candle
 * SAC, BC and the candle DQN; other agent kinds return BDR_ERR_INVALID. */
BDR_API int32_t bdr_agent_sample_raw(bdr_agent* a, const bdr_obs_norm* norm, uint64_t n, const void* rows, int32_t dtype,
                                     int32_t on_device, uint64_t row_stride, float* act_out, int64_t* idx_out);

/* ---- hyperparameters by id, and copies of training state between the members of a group (BC, IQL, AWAC, the candle SAC) ----------------
 * The two steps of population-based training (explore, exploit), of successive halving and of a learning-rate schedule.
 * bdr_agent_hyper_get / _set read and write ONE scalar field of the agent's config - the fields the group comments above list as
 * "free per member" - on a standalone agent or a group member.  Nothing about shape, loss form or optimizer kind is settable.
 *   BC          LR, BETA1, BETA2, EPS, WEIGHT_DECAY (bdr_bc_config::lr, ::opt)
 *   IQL         LR_VALUE, LR_CRITIC, LR_ACTOR and the VALUE_ / CRITIC_ / ACTOR_ scalars of their optimizers, GAMMA, CRITIC_TAU, TAU_IQL,
 *               INV_LAMBDA, EXP_ADV_MAX
 *   AWAC        LR_ACTOR, LR_CRITIC and their optimizers' scalars, GAMMA, CRITIC_TAU, INV_LAMBDA, EXP_ADV_MAX
 *   candle SAC  LR_ACTOR, LR_CRITIC and their optimizers' scalars, GAMMA, CRITIC_TAU; with EntCoefMode::Auto also ENT_COEF_LR and
 *               TARGET_ENTROPY
 * (BETA1, BETA2, EPS and WEIGHT_DECAY are read by BDR_OPT_ADAMW only, as at creation: BDR_OPT_ADAM keeps PyTorch's defaults.)
 * BDR_ERR_INVALID: an id the kind does not have (every agent kind but these four has none), and a value outside the id's range - a
 * learning rate, eps or weight decay that is negative or not finite; a beta outside [0, 1); GAMMA or CRITIC_TAU outside [0, 1];
 * TAU_IQL outside (0, 1); INV_LAMBDA or EXP_ADV_MAX negative or not finite; a TARGET_ENTROPY that is not finite.  (The constructors
 * check none of these scalars; the setter refuses what no update defines.)
 * A set takes effect in the member's next update, a group round or its own bdr_agent_opt / update_on_batch: the learning rates and
 * optimizer scalars are recomputed from the config every update; the values a group keeps in staged static arguments (GAMMA,
 * CRITIC_TAU, TAU_IQL, INV_LAMBDA, EXP_ADV_MAX, TARGET_ENTROPY) are part of the member's static key, so the next round restages them.
 * These agent kinds replay no captured step graph, so there is no graph to patch or drop.  Setting a value to what it is changes nothing. */
enum {
    BDR_HYPER_LR = 0, BDR_HYPER_BETA1 = 1, BDR_HYPER_BETA2 = 2, BDR_HYPER_EPS = 3, BDR_HYPER_WEIGHT_DECAY = 4,
    BDR_HYPER_LR_ACTOR = 10, BDR_HYPER_ACTOR_BETA1 = 11, BDR_HYPER_ACTOR_BETA2 = 12, BDR_HYPER_ACTOR_EPS = 13, BDR_HYPER_ACTOR_WEIGHT_DECAY = 14,
    BDR_HYPER_LR_CRITIC = 20, BDR_HYPER_CRITIC_BETA1 = 21, BDR_HYPER_CRITIC_BETA2 = 22, BDR_HYPER_CRITIC_EPS = 23, BDR_HYPER_CRITIC_WEIGHT_DECAY = 24,
    BDR_HYPER_LR_VALUE = 30, BDR_HYPER_VALUE_BETA1 = 31, BDR_HYPER_VALUE_BETA2 = 32, BDR_HYPER_VALUE_EPS = 33, BDR_HYPER_VALUE_WEIGHT_DECAY = 34,
    BDR_HYPER_GAMMA = 40, BDR_HYPER_CRITIC_TAU = 41, BDR_HYPER_TAU_IQL = 42, BDR_HYPER_INV_LAMBDA = 43, BDR_HYPER_EXP_ADV_MAX = 44,
    BDR_HYPER_ENT_COEF_LR = 45, BDR_HYPER_TARGET_ENTROPY = 46
};
BDR_API int32_t bdr_agent_hyper_get(bdr_agent* a, int32_t id, double* out);
BDR_API int32_t bdr_agent_hyper_set(bdr_agent* a, int32_t id, double v);

/* bdr_<kind>_group_copy_members: member dst[i] becomes a copy of member src[i], i < n, in ONE launch whatever n and the number of
 * models are - no copy command, no event, no synchronise; the call counts as one launch in bdr_group_info::kernel_launches and
 * launches_per_round stays what it is.
 * What moves, on the device: every arena the member's model table serves (bdr_agent_get_params: online and target networks, +100 the
 * last gradient, +200 exp_avg, +300 exp_avg_sq; the candle SAC's log_alpha with its gradient and moments, and alpha).  On the host: the
 * optimizer step counters that become Adam's bias corrections, so the destination continues exactly as its source would; with
 * flags & BDR_COPY_HYPER every hyperparameter above that both members have.
 * What stays the destination's: its seed and noise counter, train / eval mode, act path, its buffer or view with its index stream,
 * n_opts, the record of its last update, and the evaluator's best-model bookkeeping - exploration stays independent.  Every derived
 * copy of the destination's parameters follows as after bdr_agent_set_params (the candle SAC's alpha is carried by the copy itself:
 * it keeps the bits its source's update wrote).
 * Refused with BDR_ERR_INVALID before anything moves, naming the pair: n == 0; an index >= the group's size; src[i] == dst[i]; a
 * destination listed twice; a member that is a destination in one pair and a source in another (so no member is read and written by
 * one call); unknown flags; more than 65535 segments - n x the member's arenas (BC 4, AWAC 4 + 5 n_critics, IQL 8 + 5 n_critics, the
 * candle SAC 5 + 5 n_critics), the extent of a grid dimension: split the call. */
#define BDR_COPY_HYPER 1
BDR_API int32_t bdr_bc_group_copy_members(bdr_bc_group* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags);
BDR_API int32_t bdr_iql_group_copy_members(bdr_iql_group* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags);
BDR_API int32_t bdr_awac_group_copy_members(bdr_awac_group* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags);
BDR_API int32_t bdr_candle_sac_group_copy_members(bdr_candle_sac_group* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU parameter exchange (replaces the learner->actors NamedTensors channel of
 * border-async-trainer/src/async_trainer/base.rs:268-272 with RCCL over xGMI).
 * ---------------------------------------------------------------------------------------- */
#define BDR_UNIQUE_ID_BYTES 128
BDR_API int32_t bdr_comm_get_unique_id(uint8_t id[BDR_UNIQUE_ID_BYTES]);
BDR_API int32_t bdr_comm_init_rank(const uint8_t id[BDR_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank,
                                   int32_t device, bdr_comm** out);
BDR_API int32_t bdr_comm_destroy(bdr_comm* c);
/* *all_ok <- MIN over ranks of (local_ok != 0): the agreement every rank reaches before it enters a collective, so that a rank
 * whose learner failed does not leave its peers blocked in the next all-reduce (bdr_learner_ops::agree).  Synchronous. */
BDR_API int32_t bdr_comm_agree(bdr_comm* c, int32_t local_ok, int32_t* all_ok);
/* params <- mean over ranks (ncclAllReduce sum on the flat arena, then 1/nranks), on the
 * agent's stream; which as in bdr_agent_get_params (0 qnet, 1 qnet_tgt, 2/3 Adam moments). */
BDR_API int32_t bdr_agent_allreduce_params(bdr_agent* a, bdr_comm* c, int32_t which);
/* Synchronous data-parallel mode for DQN agents (an IQL, AWAC or BC agent returns BDR_ERR_INVALID): from now on every Agent::opt of `a` runs backward, all-reduces the gradient
 * arena over `c` (ncclAllReduce sum, then 1/nranks, on the agent's stream) and then takes the optimizer step, so the ranks
 * stay bit-for-bit in lock step and N x batch B/N equals one step on batch B.  c == NULL: back to independent steps. */
BDR_API int32_t bdr_agent_set_grad_comm(bdr_agent* a, bdr_comm* c);
/* params <- root's (ncclBroadcast): the faithful learner->actor sync. */
BDR_API int32_t bdr_agent_broadcast_params(bdr_agent* a, bdr_comm* c, int32_t which, int32_t root);

#ifdef __cplusplus
}
#endif
#endif /* BORDER_AMD_H */
