// Shared host-side plumbing of libborder_amd.so: error reporting, HIP call checking,
// the opaque handle layouts.  gfx950 only; no CPU fallback anywhere in this library.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/border_amd.h"
#include "chacha.hpp"
#include "frame_share.hpp"

namespace bdr {

extern thread_local char g_err[512];
extern thread_local int g_err_deferred;   // the last failure on this thread reports a device-side condition of an EARLIER, asynchronous step (bdr_last_error_is_deferred)

inline int32_t fail(int32_t code, const char* fmt, ...)
{
    g_err_deferred = 0;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define BDR_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return ::bdr::fail(BDR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                               __FILE__, __LINE__);                                                \
    } while (0)

#define BDR_TRY(expr)                                                                              \
    do {                                                                                           \
        int32_t s__ = (expr);                                                                      \
        if (s__ != BDR_OK) return s__;                                                             \
    } while (0)

#define BDR_REQUIRE(cond, ...)                                                                     \
    do {                                                                                           \
        if (!(cond)) return ::bdr::fail(BDR_ERR_INVALID, __VA_ARGS__);                             \
    } while (0)

inline uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

int32_t ensure_device(int32_t device);

// bdr_{dqn,iqn}_config::arithmetic -> "the large layers take the split-operand bf16 kernels".  `override_var` (=1 exact, =0 split;
// set but empty counts as 1, as in round 5) is read for A/B runs only: the boundary's field is what a caller states.
inline bool arith_is_split(int32_t arithmetic, const char* override_var)
{
    bool split = arithmetic != BDR_ARITH_F32_EXACT;
    if (const char* e = getenv(override_var)) split = e[0] == '0';
    return split;
}

}  // namespace bdr

// ---------------------------------------------------------------------------------------------
// Replay ring: one fused record per transition, record_stride bytes apart (multiple of 128):
//   [0, obs_bytes)                       obs
//   [obs_off2, obs_off2 + obs_bytes)     next_obs      (obs_off2 = round_up(obs_bytes, 16))
//   [act_off, act_off + act_bytes)       act
//   [tail_off + 0]  f32 reward, [+4] i8 is_terminated, [+5] i8 is_truncated
// ---------------------------------------------------------------------------------------------
struct bdr_per;   // per.hip

struct bdr_replay {
    int32_t device = 0;
    bdr_per* per = nullptr;    // prioritized replay state (nullptr: uniform sampling)
    uint64_t capacity = 0, i = 0, size = 0;
    uint64_t obs_bytes = 0, act_bytes = 0;
    uint64_t next_off = 0, act_off = 0, tail_off = 0, stride = 0;
    int32_t index_rng = 0;     // BDR_RNG_STDRNG / BDR_RNG_XOSHIRO256PP
    uint64_t* xo_state = nullptr;   // xoshiro256++: [XO_LANES][4] generator states in HBM (lane j draws sample j of every batch)
    uint32_t key[8] = {0};     // ChaCha12 key = seed_from_u64(seed)
    uint64_t word_pos = 0;     // next u32 word of the key stream (host-tracked, passed by value)
    uint8_t* ring = nullptr;   // capacity * stride bytes in HBM
    // views (bdr_replay_view_create, replay.hip): a view borrows its owner's rows - `ring` is the owner's - and is read-only
    bdr_replay* view_of = nullptr;   // the owner of the rows (nullptr: this handle owns its ring)
    uint32_t n_views = 0;            // live views of this ring: pushes, fill, enable_per and destroy are refused meanwhile
    hipStream_t stream = nullptr;
    hipEvent_t written = nullptr;  // recorded after the last push/fill on `stream`
    hipEvent_t read = nullptr;     // recorded by the consumer after the last gather
    // Cross-stream ordering is lazy: a barrier packet (event record or wait) costs its queue a 5-7 us bubble
    // (tools/rocprof_timeline.py), so the opt loop's gather records / waits nothing unless a push, fill or tree update
    // actually happened in between.
    bool read_pending = false;          // a gather on read_stream may still be reading ring rows / owns the batch buffers
    hipStream_t read_stream = nullptr;
    uint64_t written_gen = 1;           // bumped with every record of `written`
    bool written_lazy = false;          // the newest write has not recorded `written` yet (wait_for_writer does it on the writer's stream)
    hipStream_t writer_stream = nullptr; // the stream of that newest write: `stream`, or a group's stream after a grouped push (bdr_agent_group_push)
    std::vector<std::pair<hipStream_t, uint64_t>> waited;   // consumer stream -> generation of `written` it has waited for
    // pinned staging for push
    uint8_t* stage = nullptr;
    uint64_t stage_records = 0;
    unsigned* done_host = nullptr; unsigned* done_dev = nullptr; unsigned done_seq = 0;   // pinned "small push finished" word (host view / device view) and its sequence number
    unsigned* done_ticket = nullptr;                        // device: records of the current small push that are finished
    unsigned dev_rows_checks = 0;                            // counts cache hits of dev_rows_ok (every 1024th one re-validates)
    const void* dev_rows_ok[2] = {nullptr, nullptr};       // bdr_replay_push_device: the obs / next_obs base addresses that passed the device-pointer check last
    // bdr_replay_push_episode: pinned staging (two halves of ep_half bytes: raw rows | act / reward / flags) and its device twin
    uint8_t* ep_stage = nullptr; uint8_t* d_ep = nullptr; uint64_t ep_half = 0; hipEvent_t ep_free[2] = {nullptr, nullptr};
    uint8_t* d_tails = nullptr; uint64_t tails_cap = 0;   // bdr_replay_push_device: device copy of a run's act / reward / flags
    // device batch buffers (lazily sized)
    uint64_t batch_cap = 0, batch_n = 0;
    uint64_t uid = 0, batch_gen = 0;   // process-unique handle id; bumped whenever the batch buffers are re-allocated or flipped
    uint8_t *b_obs = nullptr, *b_next = nullptr, *b_act = nullptr;
    float* b_reward = nullptr;
    int8_t *b_term = nullptr, *b_trunc = nullptr;
    uint64_t* b_ixs = nullptr;
    // second set of batch buffers (replay_flip_batch): a consumer that gathers the next batch on another queue while kernels
    // of the previous update still read the current one alternates between the two sets
    struct BatchSet { uint8_t *obs = nullptr, *next = nullptr, *act = nullptr; float* reward = nullptr; int8_t *term = nullptr, *trunc = nullptr; uint64_t* ixs = nullptr; } alt;
    bool alt_valid = false;
    // ---- single-frame store (bdr_replay_config::frame_stack > 0): `ring` then holds only the small records
    //   [u32 frame slot x 2k (obs newest..oldest, next_obs newest..oldest) | act | reward f32 | is_terminated i8 | is_truncated i8]
    // and `frames` the frame store (frame_cap slots of frame_bytes, allocated in push order, slot = seq % frame_cap).
    int32_t frame_stack = 0;
    uint64_t frame_bytes = 0, frame_cap = 0;
    uint8_t* frames = nullptr;
    uint64_t rec_act_off = 0, rec_tail_off = 0;               // record layout (offsets of act / tail inside a record)
    bdr::FrameShare fs;                    // frames allocated so far, first_ref, the last next_obs' sequence numbers (frame_share.hpp)
    std::vector<uint8_t> last_next;        // host copy of the last pushed next_obs (episode continuation test of the host push)
    bool last_next_stale = false;          // a device push came last: `last_next` is fetched from the frame store when a host push needs it
    uint8_t* fstage = nullptr;             // pinned staging: new frames (host push) / equality flags and scatter jobs (device push)
    uint64_t fstage_frames = 0;
    uint8_t* d_fshare = nullptr; uint64_t fshare_bytes = 0;   // bdr_replay_push_device_frames: device twin of the flags and jobs of a run
};

// Observation normaliser (dataset.hip): per-column mean / std of a dataset and the element contract
//   z = ((float)x - mean) / std     (two separately rounded f32 operations, the division correctly rounded)
// that bdr_obs_norm_apply[_device] and bdr_replay_push_episode (replay.hip, k_push_episode) share.
struct bdr_obs_norm {
    int32_t device = 0;
    uint64_t dim = 0;
    bool ready = false;                    // finish() or set() happened: mean / std are valid, accumulate is refused
    uint64_t count = 0;                    // rows accumulated so far
    uint64_t merged = 0, fill_rows = 0;    // of them: folded into d_mean / d_m2; waiting in the current staging half
    int32_t fill_dtype = 0; int half = 0;  // dtype of the waiting rows; the half being filled
    hipStream_t stream = nullptr;
    double *d_mean = nullptr, *d_m2 = nullptr;   // [dim] running mean and sum of squared deviations (float64, device)
    double* d_part = nullptr;              // [chunk_rows / 64][2][dim] per-block (mean, M2) of the chunk in flight
    float *d_meanf = nullptr, *d_stdf = nullptr; // [dim] the f32 statistics the kernels read
    std::vector<float> mean, std;          // host copies (the host path of apply, get)
    uint8_t* stage = nullptr;              // pinned: two halves of stage_half bytes
    uint8_t* d_raw = nullptr;              // device twin of the staging halves
    uint64_t stage_half = 0, chunk_rows = 0;
    hipEvent_t half_free[2] = {nullptr, nullptr};
};

namespace bdr {
// z of one element, shared by every kernel that normalises (the statement of the contract in code)
__host__ __device__ __forceinline__ float obs_norm_z(float x, float mean, float std)
{
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(x - mean, std);
#else
    return (x - mean) / std;
#endif
}
}  // namespace bdr

namespace bdr {
// Enqueue "draw n indices + gather" on `stream` (the consumer's stream).  Handles the
// cross-stream ordering against pushes.  Advances the RNG like one batch(n).
int32_t replay_sample_on_stream(bdr_replay* r, uint64_t n, hipStream_t stream);
int32_t replay_prepare_sample(bdr_replay* r, uint64_t n, hipStream_t stream);

// arguments of the gather kernels (replay.hip k_gather) - also handed to agents whose own kernel does the gather (replay_sample_plan)
struct GatherArgs {
    const uint8_t* ring;
    uint64_t stride, obs_bytes, act_bytes, next_off, act_off, tail_off;
    uint64_t* ixs;           // [n] sampled indices (written by chunk 0 of every sample)
    ChaChaKey key;           // K1 fused: every workgroup draws its own index (wave-uniform -> scalar unit)
    uint64_t word_pos, size;
    uint8_t *b_obs, *b_next, *b_act;
    float* b_reward;
    int8_t *b_term, *b_trunc;
    uint32_t chunks;      // workgroups per sample
    uint32_t vec_per_chunk;  // 16-byte vectors per chunk
    uint32_t given;       // 1: ixs[] was produced by the PER sampler, gather those rows
};
int32_t replay_sample_plan(bdr_replay* r, uint64_t n, hipStream_t stream, GatherArgs* out);
// The plans of P members gathered by ONE launch of k_gather's body (a layer-form agent group, group_layers.hpp): the descriptors sit
// in a device array, each member's stream position and ring size of this step at the start of its entry of a pinned staging slot.
// Arguments a kernel reads in place from memory go through the constant address space: uniform indices make them scalar loads.
#define BDR_CONST_AS __attribute__((address_space(4)))
struct GatherStepWords { unsigned long long word_pos, size; };
void replay_gather_shape(uint64_t obs_bytes, uint32_t* chunks, uint32_t* vec_per_chunk);
int32_t replay_gather_group(hipStream_t stream, const GatherArgs* d_args, const void* words, uint32_t word_stride, uint32_t P, uint64_t n, uint64_t obs_bytes);
int32_t replay_ensure_batch_capacity(bdr_replay* r, uint64_t n);
// A kernel on `stream` - not necessarily the ring's own - is about to write `n` rows at the head (a grouped push): begin orders
// `stream` behind the last gather (WAR) and behind every earlier write (WAW) and costs nothing when both were on `stream`; end, once
// the kernel is enqueued, makes `stream` the ring's last writer and advances head and size as one push of n rows does.  A later
// sample on `stream` is ordered by the queue; every other stream orders itself through `written`, recorded on `stream` on demand.
int32_t replay_begin_write_on_stream(bdr_replay* r, hipStream_t stream);
void replay_end_write_on_stream(bdr_replay* r, hipStream_t stream, uint64_t n);
// Consumer streams a replay buffer may have to record an event on later (lazy ordering): registered when they first sample,
// retired by their owner after synchronising and before hipStreamDestroy, so that a buffer never touches a dead handle.
void stream_register(hipStream_t s);
void stream_retire(hipStream_t s);
bool stream_alive(hipStream_t s);
bdr_replay* replay_lookup(uint64_t uid);   // live handle with this uid, or nullptr once it was destroyed
int32_t replay_per_check(uint64_t uid, bool* alive);   // per_check of that handle while the registry lock is held
// the host state a sample advances (uniform ring): snapshot / restore around a step-graph pass that may have to be re-enqueued
struct ReplaySnap {
    uint64_t word_pos, batch_n; bool read_pending; hipStream_t read_stream;
    explicit ReplaySnap(const bdr_replay* r) : word_pos(r->word_pos), batch_n(r->batch_n), read_pending(r->read_pending), read_stream(r->read_stream) {}
    void restore(bdr_replay* r) const { r->word_pos = word_pos; r->batch_n = batch_n; r->read_pending = read_pending; r->read_stream = read_stream; }
};
int32_t replay_flip_batch(bdr_replay* r, uint64_t n);   // makes the other buffer set current (allocated on first use)

// per.hip
int32_t per_create(const bdr_per_config* c, uint64_t capacity, hipStream_t stream, bdr_per** out);
void per_destroy(bdr_per* p);
int32_t per_push(bdr_per* p, uint64_t i0, uint64_t len, hipStream_t st);
int32_t per_sample(bdr_per* p, const uint32_t key[8], uint64_t word_pos, uint64_t n, uint64_t* ixs_dev, hipStream_t st);
int32_t per_update(bdr_per* p, uint64_t n, const uint64_t* ixs_dev, const float* td_dev, hipStream_t st);
const float* per_weights(const bdr_per* p);
int32_t per_read(const bdr_per* p, int32_t what, float* out, uint64_t n, hipStream_t st);
int32_t per_get(const bdr_per* p, float s, uint64_t* ix, hipStream_t st);
void per_info(const bdr_per* p, bdr_per_info* o);
int32_t per_check(bdr_per* p);   // non-finite priorities flagged by the update kernels (the reference panics); call after a sync
// weights of the batch last drawn on the consumer's stream (nullptr without PER), and the priority update
// an agent enqueues after its backward pass (device arrays, the agent's stream)
inline const float* replay_batch_weights(const bdr_replay* r) { return r->per ? per_weights(r->per) : nullptr; }
int32_t replay_update_priority_on_stream(bdr_replay* r, uint64_t n, const float* td_dev, hipStream_t stream);

// ---- per.hip: the prioritized members of an agent group (bdr_agent_group, agent_group.hpp) ----------------------------------------
// Every kernel below serves ALL prioritized members of a group in one launch on the group's stream.  The static descriptor of a member
// sits in a device array (rewritten behind a synchronise when a buffer changes), the words of one step or push in a pinned slot the
// kernels read in place.  The per_group_*_advance calls move the host state exactly as per_sample / per_update / per_push do.
struct PerGroupMember {
    float* tree; unsigned* mm; float* w;                    // sum tree, {min, max, NaN flag} words, weights of the batch [>= n]
    const float* td; uint64_t* ixs;                         // |TD error| of the step [n], sampled indices [n] (the ring's b_ixs)
    uint32_t capacity; int32_t maxdepth; float alpha, eps; int32_t normalize, n;
    const uint8_t* ring; uint32_t stride, obs_bytes, act_bytes, next_off, act_off, tail_off;   // ring layout (obs_bytes % 4 == 0)
    uint8_t *b_obs, *b_next, *b_act; float* b_reward; int8_t *b_term, *b_trunc;               // the ring's batch arrays [>= n rows]
    ChaChaKey key;
};
struct PerGroupWords { uint32_t n_samples, need_mm, head, pad0; float beta; uint32_t pad1; uint64_t word_pos; };
static_assert(sizeof(PerGroupWords) == 32, "PerGroupWords is laid out in pinned slots");
// seq != 0: the launch publishes `seq` to the group's pinned sequence word once its last workgroup is through (mf_group_done's protocol)
struct PerGroupPublish { unsigned* ticket; unsigned* seq_host; unsigned seq; };
int32_t per_group_describe(bdr_per* p, uint64_t n, PerGroupMember* out);   // tree, mm, w (allocated for n), capacity, maxdepth, alpha, eps, normalize
uint64_t per_capacity(const bdr_per* p);
bool per_normalizes_all(const bdr_per* p);
PerGroupWords per_group_sample_advance(bdr_per* p);       // n_samples, need_mm, beta; mm_valid as after per_sample
void per_group_update_advance(bdr_per* p);                // mm_valid, n_opts as after per_update
PerGroupWords per_group_push_advance(bdr_per* p);         // n_samples (before the push), need_mm; mm_valid, n_samples as after per_push of one row
// post == 0: members whose words say need_mm; post == 1: members normalised over `All` (the minimum the next batch needs)
int32_t per_group_minmax(hipStream_t st, const PerGroupMember* d, const PerGroupWords* words, uint32_t n, uint64_t max_capacity, int post, PerGroupPublish pub);
int32_t per_group_sample(hipStream_t st, const PerGroupMember* d, const PerGroupWords* words, uint32_t n);
int32_t per_group_update(hipStream_t st, const PerGroupMember* d, uint32_t n, PerGroupPublish pub);
int32_t per_group_push(hipStream_t st, const PerGroupMember* d, const PerGroupWords* words, uint32_t n, PerGroupPublish pub);
}  // namespace bdr
