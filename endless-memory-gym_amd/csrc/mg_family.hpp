// mg_family.hpp -- host-side interface every environment family implements behind the C ABI (include/memgym.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/memgym.h"
#include "mg_info.hpp"
#include "mg_lab.hpp"
#include "mg_launch.hpp"
#include "mg_device.hpp"

namespace mg {

void set_error(const std::string& msg);
static_assert(MG_MAX_OPTION_SETS == 8, "set_index() (mg_device.hpp) masks an instance's set index with 7");

// One error word in pinned, coherent host memory mapped into the device's address space: kernels raise bits with a
// system-scope atomic OR (rare path), the host reads them without touching the stream (mg_peek_errors).
struct ErrorWord {
    int* host = nullptr;
    int* dev = nullptr;
    ErrorWord() {}
    ErrorWord(const ErrorWord&) = delete;
    ErrorWord& operator=(const ErrorWord&) = delete;
    ~ErrorWord() {
        if (host) (void)hipHostFree(host);
    }
    void alloc() {
        MG_HIP(hipHostMalloc((void**)&host, 64, hipHostMallocMapped | hipHostMallocCoherent));
        *host = 0;
        MG_HIP(hipHostGetDevicePointer((void**)&dev, host, 0));
    }
    int peek() const { return __atomic_load_n(host, __ATOMIC_ACQUIRE); }
    int take() { return __atomic_exchange_n(host, 0, __ATOMIC_ACQ_REL); }
};

#ifdef __HIPCC__
__device__ __forceinline__ void raise_error(int* err, int bit) {
    __hip_atomic_fetch_or(err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Deferred-reset queues (`cap` entries + a counter that the serving launch zeroes when it has drained them): a push never
// writes past the end.  The counter can only exceed `cap` if an earlier serving launch failed after its step kernel had
// queued entries; that is flagged (bit 64) instead of becoming an out-of-bounds store, and the servers clamp the count.
constexpr int ERR_QUEUE_OVERFLOW = 64;
__device__ __forceinline__ void queue_push(int* queue, int* counter, int cap, int value, int* err) {
    const int slot = atomicAdd(counter, 1);
    if (__builtin_expect(slot < cap, 1)) queue[slot] = value;
    else raise_error(err, ERR_QUEUE_OVERFLOW);
}
__device__ __forceinline__ int queue_count(const int* counter, int cap) {
    const int c = *counter;
    return c < cap ? c : cap;
}
// One thread of every workgroup that serves a queue, when its workgroup is done: the last of the `participants` out clears the counters (entries, pops beyond
// the static first round, participants that left; bg_count: a second queue's entries, or NULL), so that the launches can be replayed from a HIP graph.
__device__ __forceinline__ void queue_leave(int* left, int participants, int* count, int* head, int* bg_count = nullptr) {
    if (atomicAdd(left, 1) != participants - 1) return;
    *count = 0; *head = 0; *left = 0;  // (in this order)
    if (bg_count) *bg_count = 0;
}
// mg_step_masked, an instance whose active flag is 0, from its own lane of the MASKED form of a step kernel: the step's outputs that stay usable as
// masks and sums without another look at the flags are zeroed -- plain stores -- and nothing else of the instance is read or written.
__device__ __forceinline__ void masked_out(int i, float* reward_out, uint8_t* done_out, const mg_info_dev& info) {
    reward_out[i] = 0.0f;
    done_out[i] = 0;
    if (info.reward64_dev) info.reward64_dev[i] = 0.0;
    if (info.capacity_dev) info.capacity_dev[i] = 0;
}
#endif

// RAII device array
template <typename T>
struct DevArray {
    T* p = nullptr;
    size_t n = 0;
    DevArray() {}
    DevArray(const DevArray&) = delete;
    DevArray& operator=(const DevArray&) = delete;
    ~DevArray() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count, bool zero = true) {
        release();
        n = count;
        MG_HIP(hipMalloc((void**)&p, sizeof(T) * (count ? count : 1)));
        if (zero) MG_HIP(hipMemset(p, 0, sizeof(T) * (count ? count : 1)));
    }
    void upload(const std::vector<T>& v) {
        alloc(v.size(), false);
        MG_HIP(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    }
    size_t bytes() const { return sizeof(T) * n; }
};

// Per-instance RNG streams (mg::RngSoA, mg_device.hpp) as five device arrays; part of every family's checkpoint
struct RngStore {
    DevArray<uint64_t> s_hi, s_lo, i_hi, i_lo, buf;
    void alloc(size_t n) { s_hi.alloc(n); s_lo.alloc(n); i_hi.alloc(n); i_lo.alloc(n); buf.alloc(n); }
    RngSoA view() { return RngSoA{s_hi.p, s_lo.p, i_hi.p, i_lo.p, buf.p}; }
    // (Family::instance_rows: the five words of one instance, 8 bytes each)
    void rows(std::vector<std::pair<void*, size_t>>& v) {
        for (auto* a : {&s_hi, &s_lo, &i_hi, &i_lo, &buf}) v.push_back({a->p, sizeof(uint64_t)});
    }
    void blobs(std::vector<std::pair<void*, size_t>>& v) {
        v.push_back({s_hi.p, s_hi.bytes()}); v.push_back({s_lo.p, s_lo.bytes()}); v.push_back({i_hi.p, i_hi.bytes()});
        v.push_back({i_lo.p, i_lo.bytes()}); v.push_back({buf.p, buf.bytes()});
    }
    void debug(int i, uint64_t out[6]) {
        uint64_t b;
        MG_HIP(hipMemcpy(&out[0], s_hi.p + i, 8, hipMemcpyDeviceToHost));
        MG_HIP(hipMemcpy(&out[1], s_lo.p + i, 8, hipMemcpyDeviceToHost));
        MG_HIP(hipMemcpy(&out[2], i_hi.p + i, 8, hipMemcpyDeviceToHost));
        MG_HIP(hipMemcpy(&out[3], i_lo.p + i, 8, hipMemcpyDeviceToHost));
        MG_HIP(hipMemcpy(&b, buf.p + i, 8, hipMemcpyDeviceToHost));
        out[4] = (b >> 32) & 1;
        out[5] = b & 0xFFFFFFFFull;
    }
    void debug_set(int i, const uint64_t in[6]) {  // (the packing of Pcg::store, mg_device.hpp)
        const uint64_t b = (in[5] & 0xFFFFFFFFull) | ((uint64_t)(in[4] ? 1 : 0) << 32);
        MG_HIP(hipMemcpy(s_hi.p + i, &in[0], 8, hipMemcpyHostToDevice));
        MG_HIP(hipMemcpy(s_lo.p + i, &in[1], 8, hipMemcpyHostToDevice));
        MG_HIP(hipMemcpy(i_hi.p + i, &in[2], 8, hipMemcpyHostToDevice));
        MG_HIP(hipMemcpy(i_lo.p + i, &in[3], 8, hipMemcpyHostToDevice));
        MG_HIP(hipMemcpy(buf.p + i, &b, 8, hipMemcpyHostToDevice));
    }
};

// Host side of an OptList (mg_device.hpp): packs the entries, owns the device copy of lists that do not fit the inline form.
struct OptListStore {
    DevArray<int32_t> ext;
    std::vector<int> host;  // the entries as set (capacity checks at reset time)
    // largest entry of the list `l` this store backs.  A store that was never set() (an option set > 0 whose parameter block was copied
    // from the defaults) has no host mirror: the defaults are short byte lists held in l's inline words -- read those (the
    // capacity check at reset time saw 0 for such a set).
    int max(const OptList& l) const {
        int m = 0;
        if (!host.empty() || l.ext) {
            for (int x : host) m = x > m ? x : m;
            return m;
        }
        for (int k = 0; k < l.n && k < OPT_INLINE; ++k) {
            const int x = (int)((l.w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
            m = x > m ? x : m;
        }
        return m;
    }
    void set(OptList& l, const std::vector<int>& v) {
        host = v;
        l.n = (int)v.size();
        for (int j = 0; j < OPT_INLINE / 4; ++j) l.w[j] = 0u;
        l.ext = nullptr;
        bool bytes = true;
        for (int x : v) bytes = bytes && x >= 0 && x <= 255;
        for (int k = 0; bytes && k < l.n && k < OPT_INLINE; ++k) l.w[k >> 2] |= (uint32_t)(v[k] & 0xFF) << (8 * (k & 3));
        if (l.n > OPT_INLINE || !bytes) {
            std::vector<int32_t> b(v.begin(), v.end());
            // the previous array may still be read by kernels in flight on some stream: synchronise before it goes
            MG_HIP(hipDeviceSynchronize());
            ext.upload(b);
            l.ext = ext.p;
        }
    }
};

struct OptionError {
    int code;  // -2 unknown key, -3 unsupported value
    std::string msg;
};

// Optional per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg).
struct KernelProfile {
    int stride = 0;          // 0 = off; N = bracket every N-th step (events cost ~7 us per bracketed launch)
    uint64_t count[2] = {0, 0};
    bool live[2] = {false, false};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[2];  // 0 = logic kernel, 1 = raster kernel
    void begin(int kind, hipStream_t s) {
        live[kind] = stride > 0 && (count[kind]++ % (uint64_t)stride) == 0;
        if (!live[kind]) return;
        hipEvent_t a, b;
        MG_HIP(hipEventCreate(&a));
        MG_HIP(hipEventCreate(&b));
        MG_HIP(hipEventRecord(a, s));
        ev[kind].push_back({a, b});
    }
    void end(int kind, hipStream_t s) {
        if (!live[kind]) return;
        MG_HIP(hipEventRecord(ev[kind].back().second, s));
    }
    // sum of elapsed ms and launch count for `kind`; synchronises and clears
    void collect(int kind, double* ms, int64_t* launches) {
        double t = 0;
        for (auto& p : ev[kind]) {
            MG_HIP(hipEventSynchronize(p.second));
            float f = 0;
            MG_HIP(hipEventElapsedTime(&f, p.first, p.second));
            t += f;
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        *ms = t;
        *launches = (int64_t)ev[kind].size();
        ev[kind].clear();
    }
};

struct ExpertArgs;  // mg_expert.hpp

// The refusal of a handle whose geometry options changed since its last reset, worded once.  who: an entry point's "mg_x: ", or empty (a family's own
// guard); before: what the reset must come before -- "first", "before the next step", "before the next render"
inline std::runtime_error stale_geometry(const std::string& who, const char* before) {
    return std::runtime_error(who + "options that change geometry need a reset " + before);
}

// mg_advance (include/memgym.h) as it reaches a family that can run the whole loop inside its own launches: the policy's arguments, the handle's
// scratch rows (what the loop's mg_expert_actions / mg_step calls would be given: info holds reward64, the episode record and the named aux slots,
// nothing else) and the caller's sums.
struct AdvanceArgs {
    int steps;
    double eps;
    uint64_t seed, step0;
    int32_t* actions;
    float* reward;
    uint8_t* done;
    float* gt;  // the caller's, or NULL
    mg_info_dev info;
    mg_advance_out out;
};

// mg_play (include/memgym.h) as it reaches a family that can run the whole loop inside its own launches: the caller's tape, mask, traces and sums, and
// the handle's scratch rows (what the loop's mg_step_masked calls would be given; info as in AdvanceArgs, alive: the loop's mask from launch to launch).
struct PlayArgs {
    int steps;
    int episode;             // mode == MG_PLAY_EPISODE
    const int32_t* tape;     // [steps][num_envs * action_dim]
    const uint8_t* active;   // the caller's, or NULL
    float* reward_trace;     // [steps][num_envs], or NULL
    uint8_t* done_trace;     // [steps][num_envs], or NULL
    int32_t* played;         // [num_envs], or NULL
    float* reward;
    uint8_t* done;
    uint8_t* alive;
    float* gt;  // the caller's, or NULL
    mg_info_dev info;
    mg_advance_out out;
};

// mg_rollout_trace (include/memgym.h: mg_advance_traced / mg_play_traced) as it reaches a family: row 0 of each [steps][...] trace array, any may be NULL.
// mg_play_traced has no actions / labels; its reward / done rows travel in PlayArgs::reward_trace / done_trace, as mg_play's do.
struct TraceRows {
    void* frames;      // [steps][num_envs] frame descriptors (frame_rows().second bytes each), 16-byte aligned
    int32_t* actions;  // [steps][num_envs * action_dim]
    int32_t* labels;   // [steps][num_envs * action_dim]
    float* reward;     // [steps][num_envs]
    uint8_t* done;     // [steps][num_envs]
};

// What the C ABI (mg_api.hip and its mg_api_*.hpp) sees of an environment family, and the host-side plumbing the three families share: the error
// word, the RNG streams, the "seeded" / "geometry changed" guards and the debug view's scratch frames.
class Family {
   public:
    explicit Family(int n) : n_(n) {}
    KernelProfile prof;
    void end_logic(hipStream_t s) { prof.end(0, s); }
    int obs_format = MG_OBS_U8_XYC;  // stream-out format of the raster kernel (include/memgym.h)
    virtual ~Family() {}
    virtual int action_dim() const = 0;
    virtual int gt_dim() const = 0;
    // mg_single_step (mg_api_single.hpp) asks the NEXT step() -- that call only, however it ends -- to store `ticket` to *flag_dev (a word the
    // host polls) from its own last kernel once its results are out.  Whether that happened is decided where step() chooses its launch:
    // done_flag_stored() is true iff the step() that just returned launched such a kernel (reading it clears it); otherwise the caller
    // puts a stream memory operation behind the step's launches.  A family without such a kernel ignores the request.
    virtual void want_done_flag(uint32_t* /*flag_dev*/, uint32_t /*ticket*/) {}
    virtual bool done_flag_stored() { return false; }
    // capacities of the per-instance lists the reference grows without limit (include/memgym.h: mg_set_capacity / mg_capacity)
    virtual void set_capacity(const std::string& what, int64_t) { throw OptionError{-2, "this env id has no capacity named " + what}; }
    virtual int64_t capacity(const std::string& what) const { throw OptionError{-2, "this env id has no capacity named " + what}; }
    virtual int vec_dim() const { return 0; }          // size of obs["vector_observation"] (MortarMayhemB*), else 0
    virtual void bind_vector_obs(float* /*dev*/) {}    // caller buffer [num_envs][vec_dim], written at every reset
    virtual const char* info_name(int k) const = 0;
    virtual void set_option(const std::string& key, const double* v, int n) = 0;  // throws OptionError
    // per-instance option sets (include/memgym.h: mg_set_option_set / mg_bind_option_sets); families without them refuse sets > 0
    virtual void set_option_set(int set, const std::string& key, const double* v, int n) {
        if (set != 0) throw OptionError{-3, "this env id has no per-instance option sets in this build (use one handle per option set)"};
        set_option(key, v, n);
    }
    virtual void bind_option_sets(const int32_t* set_of_dev) {
        if (set_of_dev) throw OptionError{-3, "this env id has no per-instance option sets in this build (use one handle per option set)"};
    }
    virtual void reset(const int64_t* seeds, const uint8_t* mask, void* obs, float* gt, hipStream_t s) = 0;
    // obs == NULL: a HEADLESS step (include/memgym.h: mg_step) -- the family's plain arrangement without its raster launch; everything but the
    // frames, the descriptors included, is what a drawn step of the same handle leaves (info->final_obs_dev is NULL then: mg_step refuses the pair)
    // active != NULL: a MASKED step (include/memgym.h: mg_step_masked) -- the arrangement of a headless step with the MASKED form of its step kernel, which
    // leaves the instances with active[i] == 0 alone but for their zeroed reward / done, then, with obs, masked_frames(): the active instances' frames
    // final_frames != NULL: TERMINAL FRAME RECORDS (include/memgym.h: mg_info_buffers.final_frames_dev) -- obs is NULL (mg_api.hip draws behind the call), the
    // RECORDS form of the (masked) step kernel stores the descriptor of the frame an instance ended on, as it is before any reset, to row i of
    // final_frames (frame_rows().second bytes each), in the same number of launches; rows of instances that did not finish are not written
    virtual void step(const int32_t* actions, const uint8_t* active, void* obs, float* reward, uint8_t* done, float* gt,
                      const mg_info_dev* info, int autoreset, hipStream_t s, void* final_frames = nullptr) = 0;
    // mg_advance: true = the family has run the loop of include/memgym.h's definition inside launches of its own (the mortar family:
    // mortar_advance_kernel); false = it has no such form (or the lab build switched it off) and nothing happened: mg_api_rollout.hpp runs the loop.
    virtual bool advance(const AdvanceArgs& /*v*/, hipStream_t /*s*/) { return false; }
    // mg_play: true = the family has run the loop of include/memgym.h's definition inside launches of its own (the mortar family:
    // mortar_play_kernel); false = it has no such form (or the lab build switched it off) and nothing happened: mg_api_rollout.hpp runs the loop.
    virtual bool play(const PlayArgs& /*v*/, hipStream_t /*s*/) { return false; }
    // mg_advance_traced / mg_play_traced with a trace: the same contract, the traced in-launch forms (the mortar family: mortar_advance_traced_kernel /
    // mortar_play_traced_kernel, mg_mortar_trace.hpp).  `frames` of play_traced: TraceRows::frames, or NULL.
    virtual bool advance_traced(const AdvanceArgs& /*v*/, const TraceRows& /*tr*/, hipStream_t /*s*/) { return false; }
    virtual bool play_traced(const PlayArgs& /*v*/, void* /*frames*/, hipStream_t /*s*/) { return false; }
    // mg_step_next: true = the family has run the call in launches of its own -- the NEXT form of its step kernel (an instance with restart[i] != 0 is reset by
    // its own lane(s), the others step without auto-reset), its dense raster launch, and a last small launch that leaves the descriptor rows as the masked
    // mg_reset of the definition leaves them (the mortar family: mg_mortar_next.hpp, the spotlight family: mg_spot_next.hpp); false = it has no such form (or
    // the lab build switched it off) and nothing happened: mg_api.hip runs the pair of the definition.  restart may be the same memory as done: each
    // instance's flag is read before its done is written, and kept in restart_copy ([num_envs] bytes of the handle's scratch) for the last launch.
    virtual bool step_next(const int32_t* /*actions*/, const uint8_t* /*restart*/, uint8_t* /*restart_copy*/, void* /*obs*/, float* /*reward*/,
                           uint8_t* /*done*/, float* /*gt*/, const mg_info_dev* /*info*/, hipStream_t /*s*/) { return false; }
    // rasterise the CURRENT frame descriptors of the instances with only[i] != 0 into `obs` (others untouched)
    virtual void raster_only(void* obs, const uint8_t* only, hipStream_t s) = 0;
    // mg_save_frames / mg_draw_frames (include/memgym.h; mg_frame_records.hpp).  frame_rows(): the frame descriptor array raster_only() draws from, as
    // (device pointer, bytes per instance: sizeof the family's Desc).  draw_records(): row j of `obs` <- the frame of records[pick[j]] (pick == NULL:
    // records[j]), j < count, in format `fmt` -- the gather form of the family's raster launch with the composer raster_only() picks and the handle's
    // atlas; nothing of the handle is written.  The arguments have passed frame_draw_refusal().
    virtual std::pair<const void*, size_t> frame_rows() = 0;
    virtual void draw_records(const void* records, int n_records, const int32_t* pick, int count, int fmt, void* obs, hipStream_t s) = 0;
    // mg_draw_frames_padded: draw_records() through the PAD form of the gather launch -- a pick below 0 writes its row as zeros and raises no error.
    virtual void draw_records_padded(const void* records, int n_records, const int32_t* pick, int count, int fmt, void* obs, hipStream_t s) = 0;
    // true: step(..., autoreset = 1) with info->final_obs_dev set keeps the terminal observations ITSELF (the frame workgroup of a finishing
    // instance draws the terminal frame into final_obs_dev, then the reset frame into obs); false: mg_step takes the generic path (a step
    // without auto-reset, the terminal rows copied, a masked reset).  Asked once per call, on the stream of the call.
    virtual bool keeps_final_obs(hipStream_t /*s*/) { return false; }
    // render("debug_rgb_array") before its final x4 stretch: the debug surface of every instance (the reference's
    // _build_debug_surface, e.g. mortar_mayhem_grid.py:104-135) as uint8 [num_envs][84 x][84 y][3], the observation layout
    virtual void raster_debug(void* frames, hipStream_t s) = 0;
    // mg_save_debug_frames / mg_draw_debug_frames (include/memgym.h).  save_debug_records(): record j <- the descriptor raster_debug() would fill for
    // instance idx[j] (idx == NULL: instance j) from the current state, j < count -- the picked form of the family's *_debug_desc_kernel, one lane per
    // entry, with mg_save_frames' index conventions; what a debug render changes (the mortar family's dbg_pops) changes for the named instances alone.
    // Stream-ordered: work a family has put off is enqueued in front, nothing synchronises.  draw_debug_records(): row j of `rgb` <- the view of
    // records[pick[j]] at `size` 84 or 336, the gather form of the family's raster launch with the composer raster_debug() picks.
    virtual void save_debug_records(const int32_t* idx, int count, void* rec, hipStream_t s) = 0;
    virtual void draw_debug_records(const void* records, int n_records, const int32_t* pick, int count, int size, void* rgb, hipStream_t s) = 0;
    // checkpoint: list of (device pointer, bytes) making up the state
    virtual std::vector<std::pair<void*, size_t>> state_blobs() = 0;
    // mg_save_instances / mg_load_instances (mg_instances.hpp): the arrays that ARE [num_envs][row], as (device pointer, bytes per instance) -- everything the
    // checkpoint holds per instance and the frame descriptor row; at most INSTANCE_MAX_ROWS.  What belongs to the handle and not to an instance stays out
    virtual std::vector<std::pair<void*, size_t>> instance_rows() = 0;
    // in front of a save's launch, on its stream: work a family has put off is done before the rows are read (Endless Mystery Path: owed path segments)
    virtual void before_instance_save(hipStream_t /*s*/) {}
    bool geometry_dirty() const { return dirty_; }                   // a geometry option was set since the last reset
    uint64_t geometry_generation() const { return geom_gen_; }       // rebuilds of the geometry so far (mg_instance_layout)
    uint64_t frame_generation() const { return frame_gen_; }         // what else makes a stored frame descriptor draw differently (mg_frame_layout)
    // called by mg_set_state after the blobs were restored: the instances now carry seeded RNG streams
    virtual void on_state_loaded() { seeded_ = true; }
    // called before anything looks at the state from outside (mg_get_state, mg_debug_rng, mg_render_debug): work a family has
    // put off without changing any result (Endless Mystery Path: owed path segments) is done now.  Synchronous.
    virtual void sync_state() {}
    virtual void debug_rng(int i, uint64_t out[6]) { rng_.debug(i, out); }
    // mg_debug_set_rng, after sync_state(): the instance's stream is replaced.  A family that holds anything computed ahead of time
    // from the old stream drops it here (Endless Mystery Path: the record of the next episode's first segment).
    virtual void debug_set_rng(int i, const uint64_t in[6]) { rng_.debug_set(i, in); }
    // info["ground_truth"] as the reference returns it -- float64 (e.g. endless_mortar_mayhem.py:259,358) -- of every instance,
    // [num_envs][gt_dim], computed from the CURRENT state (the float32 gt_dev of mg_step / mg_reset is its rounding); a small
    // launch of its own, only when a caller asks (mg_info_buffers.gt64_dev, mg_ground_truth64).  No-op for gt_dim() == 0.
    // only != NULL (mg_step_masked): the rows of the instances with only[i] != 0, the others are not written
    virtual void ground_truth64(double* /*gt64_dev*/, hipStream_t /*s*/, const uint8_t* /*only*/ = nullptr) {}
    // mg_expert_actions: the oracle's expert action of every instance from the CURRENT state (or the random one its draw gives it, ExpertArgs /
    // mg_expert.hpp), into x.actions in the layout step() reads.  One small launch; changes no state, draws from no instance's stream.
    virtual void expert_actions(const ExpertArgs& x, hipStream_t s) = 0;
    // device-side error bits accumulated since the last call (0 = none); synchronises
    virtual int poll_errors() {
        MG_HIP(hipDeviceSynchronize());
        return err_.take();
    }
    int* error_word() { return err_.dev; }  // the device address of the word, for kernels outside the families (mg_instances.hpp)
    // the same bits as seen right now, without synchronising or clearing
    virtual int peek_errors() { return err_.peek(); }
    // test / telemetry counters by name (mg_debug_counter); false = this family has no such counter.  Synchronous.
    virtual bool debug_counter(const std::string& /*name*/, int64_t* /*out*/) { return false; }

   protected:
    // head of everything that reads the geometry's constants and atlases: a geometry option set since the last reset has not reached them yet
    void require_geometry(const char* before = "before the next step") const {
        if (dirty_) throw stale_geometry("", before);
    }
    // head of every reset(): without seeds the instances keep their RNG streams, so they must have some
    void require_seeded(const int64_t* seeds) const {
        if (!seeds && !seeded_) throw std::runtime_error("reset(seed=None) before any seeded reset");
    }
    // head of every step(): the caller's info buffers, all null where it passed none
    mg_info_dev begin_step(const mg_info_dev* info) const {
        require_geometry();
        mg_info_dev ib;
        memset(&ib, 0, sizeof(ib));
        if (info) ib = *info;
        return ib;
    }
    // tail of every reset(): the frames of the instances that were reset.  With a mask few of many: `sparse(mask)` draws them by the
    // mask (launch_raster_sparse), not by a walk over every descriptor; otherwise `dense()`, the family's raster launch
    template <class Sparse, class Dense>
    void reset_frames(const uint8_t* mask, Sparse sparse, Dense dense) {
        if (mask && sparse_masked_raster()) {
            sparse(mask);
            check_launch();
        } else dense();
    }
    // tail of a masked step(): the frames of the active instances, rows of the others untouched.  Always the family's dense raster launch with the mask as
    // its filter, never launch_raster_sparse: the host does not know how many instances are active or where they lie, and the sparse launch, whose
    // workgroups own 16 consecutive instances each, is made for FEW frames spread over the batch -- measured (profiles/masked_step.md) it wins up to 12 us
    // at 1/8 and 1/64 of scattered instances and loses up to 100 us with half of them active, with all of them, or with the active ones in one block
    void masked_frames(void* obs, const uint8_t* active, hipStream_t s) {
        prof.begin(1, s);
        raster_only(obs, active, s);
        prof.end(1, s);
    }
    // raster_debug(): `fill(dbg)` writes the debug view's descriptors of all instances into scratch, `raster(dbg)` draws them
    template <typename Desc, typename Fill, typename Raster>
    void debug_frames(hipStream_t s, Fill fill, Raster raster) {
        require_geometry("before the next render");
        DevArray<Desc> dbg;
        dbg.alloc(n_, false);
        fill(dbg.p);
        raster(dbg.p);
        check_launch();
        MG_HIP(hipStreamSynchronize(s));  // dbg is released on return
    }

    const int n_;  // instances of the handle
    ErrorWord err_;
    RngStore rng_;
    bool dirty_ = true;    // a geometry option changed: the next reset rebuilds atlases and constants first
    bool seeded_ = false;  // some reset carried seeds (or a state was loaded)
    uint64_t geom_gen_ = 0;  // counts what makes earlier instance records invalid: every rebuild(), mg_set_capacity, a new vector-observation binding
    uint64_t frame_gen_ = 0;  // counts what makes earlier FRAME records invalid without a rebuild: a change of the composer raster_only() picks, of the atlas or of a
                              // template (the spotlight family's ordered_holes going from 0 to 1; host-side bookkeeping, no part of the state)
};

Family* make_mortar(int variant, int num_envs);
Family* make_spot(int endless, int num_envs);
Family* make_mystery(int variant, int num_envs);

// Workgroup size of the one-lane-per-instance logic kernels (all are written for any multiple of 64 up to 256).
// MEMGYM_STEP_BLOCK overrides `shipped` per process (measurements: profiles/r03_step_blocks.md).
inline int step_block(int shipped) {
    static const int v = lab_int("MEMGYM_STEP_BLOCK", 0);
    return (v == 64 || v == 128 || v == 256) ? v : shipped;
}

inline int to_int_checked(double v, const char* key) {
    int i = (int)v;
    if ((double)i != v) throw OptionError{-3, std::string("option ") + key + " must be integral"};
    return i;
}

// One key of the reset options as a family's set_option_set() reads it: `n` values at `v` for option set `set` (0 = the handle-wide
// set of mg_set_option), and what the families do with one.  Codes and messages are mapped by the Python package (vec_env.py: _write_set).
struct OptionArg {
    int set;
    const std::string& key;
    const double* v;
    int n;
    bool& dirty;  // the family's "a geometry option changed" guard
    int integer(int k = 0) const { return to_int_checked(v[k], key.c_str()); }
    bool flag() const { return v[0] != 0.0; }
    // a value the reference accepts and this build does not
    void must_be(bool ok) const {
        if (!ok) throw OptionError{-3, "reset parameter " + key + ": this value is not supported by the MI355X build"};
    }
    // a handle-wide value (a member of the family) that fixes geometry -- atlases, tables and derived constants are shared by the
    // handle's instances: assigned in set 0, which then needs a rebuild whether or not the value changed; a set > 0 is accepted
    // when it says what the handle's geometry already is
    template <typename T>
    void geometry(T& member, T value) const {
        if (set == 0) {
            member = value;
            dirty = true;
        } else if (member != value)
            throw OptionError{-3, "reset parameter " + key + " changes the geometry shared by the handle's instances: it can only be set for all of them (option set 0)"};
    }
    // a "sample one per episode" list of any length (np_random.choice, e.g. mortar_mayhem_grid.py:181,253-254,268-269)
    std::vector<int> int_list(int lo, int hi) const {
        if (n < 1) throw OptionError{-3, "option " + key + ": an empty list cannot be sampled"};
        std::vector<int> vals(n);
        for (int i = 0; i < n; ++i) {
            vals[i] = integer(i);
            if (vals[i] < lo || vals[i] > hi)
                throw OptionError{-3, "option " + key + ": value out of the supported range " + std::to_string(lo) + ".." + std::to_string(hi)};
        }
        return vals;
    }
};

}  // namespace mg
