// mg_mystery_endless_launch.hpp -- Endless-MysteryPath-v0, the emp_* kernels with their launch constants (EMP_SVC_*, EMP_BG_*) and the compile-time measurement hooks
// of the fused launch (MG_LAB_EMP_*; tools/build_variant.sh).
#pragma once
#include "mg_mystery_compose.hpp"
#include "mg_mystery_endless.hpp"

namespace mg {
// Endless Mystery Path: nothing that generates a path is served by the wave that carries the instance.  A reset needs
// three path generations in a row (~70 us of dependent work for one wave), a new segment one, and a wave that happened
// to hold two or three such instances set the duration of the whole launch (profiles/r01e_logic_tails.md).
// emp_step_kernel (one lane per instance, no LDS) only queues those instances; emp_serve_kernel spreads the queue over
// the chip, one wave per entry at a time, lane 0 playing the instance's lane for the unchanged serve_emp /
// emp_step_b / emp_post_reset.

template <bool PS, bool FINAL = false>
__global__ __launch_bounds__(256) void emp_step_kernel(MysteryParams P0, MysteryIO io, const int32_t* actions, float* reward_out,
                                                       uint8_t* done_out, float* gt, mg_info_dev info, int autoreset) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n) return;
    // (fewer instance-carrying lanes per wave -- 32 / 16 / 8, as the finite variants' kernel has them -- measured slower: 34-40 us
    // against 25-29, profiles/r05_emp.md)
    const MysteryParams& P = PS ? io.sets[set_index(io.set_of, i)] : P0;  // (PS: per-instance option sets)
    LAB_STEP_CLOCK(0);
    int act = actions[i];  // requested together with the state record ...
    MysteryCore s = load_core(&io.core[i]);
    asm volatile("" : "+v"(act));  // ... (a use the compiler cannot move: without it the request is issued after the record has arrived)
    int nx = 0, ny = 0;
    const int ra = emp_step_a(P, i, s, act, nx, ny, io.err);
    const int due = ra & EMP_DUE;
    LAB_STEP_CLOCK(1);
    MysteryDesc d;
    bool q = false, bg = false;
    if (due) {  // the agent entered the last-but-one segment: the rest of its step needs the new one
        queue_push(io.queue, &io.qctr[QC_COUNT], P.n, i | EMP_Q_SEGMENT, io.err);
    } else {
        q = emp_step_b<!PS, true, FINAL>(P, io, i, s, nx, ny, reward_out, done_out, gt ? gt + 3 * i : nullptr, info, autoreset, d, (ra & EMP_CAP) != 0);
        LAB_STEP_CLOCK(2);
        if (q) {
            queue_push(io.queue, &io.qctr[QC_COUNT], P.n, i, io.err);
            d.valid = DESC_QUEUED;
        } else {
            // one owed segment per step -- or, when nothing is owed, the next episode's first (EMP_PRE) -- as a job nobody waits for.
            // The record ahead of time only once the episode CAN end soon: the agent is off the path or behind its frontier (a
            // fall-off there ends the episode, endless_mystery_path.py:385-393, and no new tile refills its stamina); an agent AT its
            // frontier appends segments, each of which would drop the record again (a path-following agent: one more path per
            // appended segment for nothing, tools/emp_policy_bench.py).
            bg = P.lazy && (EMP_OWED(s) > 0 || (P.pre && !EMP_PRE(s) && (s.off || nx < s.max_x)));
        }
    }
    LAB_STEP_CLOCK(3);
    io.core[i] = s;
    if (due) io.desc[i].valid = DESC_QUEUED;  // (the rest of the descriptor is last step's)
    else io.desc[i] = d;
    // Background jobs.  Small launches (bg_coop): entries of a queue the service waves pop behind the step's own entries.  The others:
    // a FLAG per instance, collected by the background workgroups of the raster launch (round 5; rounds 3-4 pushed there too -- one more
    // atomic on a counter all 512 waves share, ~1.5 us in every wave's path).
    if (P.lazy) {
        if (P.bg_coop) {
            if (bg) queue_push(io.bgq, &io.qctr[QC_BG_COUNT], P.n, i, io.err);
        } else {
            io.bgflag[i] = bg ? 1 : 0;
        }
    }
    LAB_STEP_CLOCK(4);
}

// The MASKED form (mg_step_masked): emp_step_kernel as a masked step launches it -- the plain arrangement, P.lazy == 0, no terminal observations kept.  The lane
// of an instance with active[i] == 0 zeroes the instance's reward / done and leaves: it queues nothing, so emp_serve_kernel behind this launch serves the
// active instances' entries alone.  io.bgflag / the background queue: a plain step neither reads nor writes them (nothing is owed: the host has flushed), so
// they stay as they are for every instance, and the next fused step rewrites every instance's flag from its state.  (A kernel of its own, not a shared body:
// with the body moved into a function the compiler schedules the existing forms differently, and those stay the code they were.)
template <bool PS>
__global__ __launch_bounds__(256) void emp_step_masked_kernel(MysteryParams P0, MysteryIO io, const int32_t* actions, const uint8_t* __restrict__ active,
                                                              float* reward_out, uint8_t* done_out, float* gt, mg_info_dev info, int autoreset) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n) return;
    if (!active[i]) return masked_out(i, reward_out, done_out, info);
    const MysteryParams& P = PS ? io.sets[set_index(io.set_of, i)] : P0;
    const int act = actions[i];
    MysteryCore s = load_core(&io.core[i]);
    int nx = 0, ny = 0;
    const int ra = emp_step_a(P, i, s, act, nx, ny, io.err);
    if (ra & EMP_DUE) {  // the agent entered the last-but-one segment: the rest of its step needs the new one (emp_serve_kernel)
        queue_push(io.queue, &io.qctr[QC_COUNT], P.n, i | EMP_Q_SEGMENT, io.err);
        io.core[i] = s;
        io.desc[i].valid = DESC_QUEUED;  // (the rest of the descriptor is last step's)
        return;
    }
    MysteryDesc d;
    if (emp_step_b<!PS, true, false>(P, io, i, s, nx, ny, reward_out, done_out, gt ? gt + 3 * i : nullptr, info, autoreset, d, (ra & EMP_CAP) != 0)) {
        queue_push(io.queue, &io.qctr[QC_COUNT], P.n, i, io.err);
        d.valid = DESC_QUEUED;
    }
    io.core[i] = s;
    io.desc[i] = d;
}

// The RECORDS form (mg_info_buffers.final_frames_dev) of the step kernel as a headless or masked step launches it -- the plain arrangement, P.lazy == 0.  The rows are
// io.tdesc: the host hands this form (and emp_serve_records_kernel behind it) an io whose tdesc IS the caller's buffer, so that the FINAL tail of emp_step_b -- the
// terminal descriptor first, before anybody resets the instance -- stores straight into the caller's row.  That tail keeps the row only for an instance that is reset
// in this call; with autoreset == 0 the descriptor the step leaves IS the terminal one, and the lane stores it where its own done flag says so.  An instance whose step
// needs a new segment first finishes in the queue server: its row is written there.
template <bool PS, bool MASKED>
__global__ __launch_bounds__(256) void emp_step_records_kernel(MysteryParams P0, MysteryIO io, const int32_t* actions, const uint8_t* __restrict__ active,
                                                               float* reward_out, uint8_t* done_out, float* gt, mg_info_dev info, int autoreset) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n) return;
    if (MASKED && !active[i]) return masked_out(i, reward_out, done_out, info);
    const MysteryParams& P = PS ? io.sets[set_index(io.set_of, i)] : P0;
    const int act = actions[i];
    MysteryCore s = load_core(&io.core[i]);
    int nx = 0, ny = 0;
    const int ra = emp_step_a(P, i, s, act, nx, ny, io.err);
    if (ra & EMP_DUE) {  // the agent entered the last-but-one segment: the rest of its step needs the new one (emp_serve_records_kernel)
        queue_push(io.queue, &io.qctr[QC_COUNT], P.n, i | EMP_Q_SEGMENT, io.err);
        io.core[i] = s;
        io.desc[i].valid = DESC_QUEUED;  // (the rest of the descriptor is last step's)
        return;
    }
    MysteryDesc d;
    // (OWN_RESET = false: this form only ever runs the plain arrangement, where no instance resets itself from a record made ahead of time -- without that
    // code and its batch of loads the kernel needs 188 VGPRs, with it 262)
    if (emp_step_b<false, true, true>(P, io, i, s, nx, ny, reward_out, done_out, gt ? gt + 3 * i : nullptr, info, autoreset, d, (ra & EMP_CAP) != 0)) {
        queue_push(io.queue, &io.qctr[QC_COUNT], P.n, i, io.err);
        d.valid = DESC_QUEUED;
    } else if (!autoreset && done_out[i]) {
        io.tdesc[i] = d;
    }
    io.core[i] = s;
    io.desc[i] = d;
}

__global__ __launch_bounds__(256) void emp_enqueue_kernel(int n, MysteryIO io, const uint8_t* mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask[i]) queue_push(io.queue, &io.qctr[QC_COUNT], n, i, io.err);
    else io.desc[i].valid = 0;
}

// reset(seed=None, mask) the way the auto-reset STEP resets (round 6): an instance whose next episode's first segment exists already
// (EMP_PRE, nothing owed) is reset right here from that record -- the same stores as emp_step_b<true>'s own reset: the record becomes segment
// 0, the instance's stream becomes the record's, two segments are owed -- and everybody else becomes a queue entry (served lazily: one
// segment, two owed).  A step in the gymnasium vector convention (mg_step with final_obs_dev) is a step without auto-reset plus this masked
// reset: through emp_enqueue_kernel every finishing instance was three cooperative paths of the queue server, 92 us per step at 32,768.
__global__ __launch_bounds__(256) void emp_masked_reset_kernel(MysteryParams P, MysteryIO io, const uint8_t* mask, float* gt) {
    typedef uint32_t q4 __attribute__((ext_vector_type(4)));
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    if (!mask[i]) {
        io.desc[i].valid = 0;
        return;
    }
    MysteryCore s = load_core(&io.core[i]);
    if (!(P.pre && EMP_PRE(s) && EMP_OWED(s) == 0)) {
        queue_push(io.queue, &io.qctr[QC_COUNT], P.n, i, io.err);
        return;
    }
    const q4* aq = reinterpret_cast<const q4*>(io.aux + (size_t)i * AUX_WORDS);
    const q4 a0 = aq[0], a1 = aq[1], a2 = aq[2], a3 = aq[3], a4 = aq[4];  // the record generated ahead of time (AUX_WORDS layout above)
    emp_pre_reset(s);
    SegRec R, none;
    none.seg = -1;
    R.w[0] = a0.x | 0x4000u;  // the first node of the path shall not yield any reward
    R.w[1] = a0.y; R.w[2] = a0.z; R.w[3] = a0.w;
    R.w[4] = a1.x; R.w[5] = a1.y; R.w[6] = a1.z; R.w[7] = a1.w;
    R.w[8] = a2.x; R.w[9] = a2.y; R.w[10] = a2.z; R.w[11] = a2.w;
    R.w[12] = a3.x;
    R.seg = 0;
    uint32_t* dst = reinterpret_cast<uint32_t*>(seg_ptr(io, i, 0));
#pragma unroll
    for (int j = 0; j < SEG_STRIDE / 4; ++j) dst[j] = R.w[j];
    io.rng.s_lo[i] = (uint64_t)a4.x | ((uint64_t)a4.y << 32);
    io.rng.s_hi[i] = (uint64_t)a4.z | ((uint64_t)a4.w << 32);
    io.rng.buf[i] = (uint64_t)a3.y | ((uint64_t)(a3.z & 1u) << 32);
    s.num_seg = 1;
    s.have_start = 1;
    s.end_y = (int8_t)((a3.z >> 8) & 0xFFu);
    EMP_OWED(s) = 2;
    if (LAB_BUILD && io.stats) atomicAdd(io.stats + 2, 1ull);  // mg_debug_counter "emp_own_resets" (lab build: tests)
    emp_post_reset_state(P, io, i, s, gt ? gt + 3 * i : nullptr, R);
    MysteryDesc d;
    emp_fill_desc<false>(P, io, i, s, d, EMP_AX(s) / P.tile, R, none);
    d.cross_on = 0;
    if (P.show_stamina) d.stamina_red = 0;
    io.core[i] = s;
    io.desc[i] = d;
}

// Everything still owed, for every instance (Family::sync_state: before the state is looked at)
__global__ __launch_bounds__(64) void emp_flush_owed_kernel(MysteryParams P, MysteryIO io) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    lane_ws_init(smem);
    const LaneWS W{smem, (int)threadIdx.x};
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < P.n) lane_owed_segment(io, W, i, 255);
}

// mg_reset of every Endless-MysteryPath instance: one LANE per instance (emp_serve_kernel: one wave per instance)
__global__ __launch_bounds__(64) void emp_reset_lanes_kernel(MysteryParams P, MysteryIO io, const int64_t* seeds, float* gt) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    lane_ws_init(smem);
    const LaneWS W{smem, (int)threadIdx.x};
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool active = i < P.n;
    Pcg g;
    MysteryCore s;
    g.clear();
    memset(&s, 0, sizeof(s));
    int owed_old = 0;
    if (active) {
        s = io.core[i];
        if (seeds) g.seed((uint64_t)seeds[i]);
        else {
            g.load(io.rng, i);
            owed_old = EMP_OWED(s);  // reset(seed=None): what the old episode is owed comes first in the stream
        }
    }
    for (int k = 0; k < owed_old; ++k) lane_segment(io, W, i, s, g);  // (two of a lazy reset's, and appended ones: emp_step_a)
    if (active) {
        emp_pre_reset(s);
        EMP_OWED(s) = 0;
    }
    for (int k = 0; k < 3; ++k)
        if (active) lane_segment(io, W, i, s, g);
    if (active) {
        MysteryDesc d;
        emp_post_reset(P, io, i, s, d, gt ? gt + 3 * i : nullptr);
        io.core[i] = s;
        g.store(io.rng, i);
        io.desc[i] = d;
    }
}

// all != 0: mg_reset of every instance (entry k = instance k, seeds may be given); otherwise the queue is drained
template <bool PS>
__global__ __launch_bounds__(256) void emp_serve_kernel(MysteryParams P, MysteryIO io, const int64_t* seeds, int all, float* reward_out,
                                                        uint8_t* done_out, float* gt, mg_info_dev info, int autoreset) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    path_ws_init(smem);
    const PathWS W{smem, io.jump, io.stats};
    const bool me = (threadIdx.x & 63) == 0;
    const int count = all ? P.n : queue_count(&io.qctr[QC_COUNT], P.n);
    // the first entry of wave w is entry w (no atomic: with thousands of idle waves the same-address atomics of their
    // failing pops were the launch time); later ones are popped from a shared counter that starts after the last wave
    const int waves = gridDim.x * (blockDim.x >> 6);
    int idx = bcast((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)), 0);
    while (idx < count) {
        const int entry = all ? idx : bcast(io.queue[idx], 0);
        emp_serve_entry(PS ? io.sets[set_index(io.set_of, entry & EMP_Q_INST)] : P, io, W, entry, seeds, reward_out, done_out, gt, info, autoreset);
        if (me) {
            idx = waves + atomicAdd(&io.qctr[QC_HEAD], 1);
        }
        idx = bcast(idx, 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) queue_leave(&io.qctr[QC_LEFT], (int)gridDim.x, &io.qctr[QC_COUNT], &io.qctr[QC_HEAD]);
}

// The RECORDS form of the queue server behind emp_step_records_kernel (never `all`: a step's queue): the FINAL form of emp_serve_entry keeps the terminal descriptor of
// an instance that finishes HERE -- its step needed a new segment first -- in io.tdesc, the caller's rows (see emp_step_records_kernel); with autoreset == 0 the entry's
// own descriptor is the terminal one.
template <bool PS>
__global__ __launch_bounds__(256) void emp_serve_records_kernel(MysteryParams P, MysteryIO io, float* reward_out, uint8_t* done_out, float* gt, mg_info_dev info,
                                                                int autoreset) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    path_ws_init(smem);
    const PathWS W{smem, io.jump, io.stats};
    const bool me = (threadIdx.x & 63) == 0;
    const int count = queue_count(&io.qctr[QC_COUNT], P.n);
    const int waves = gridDim.x * (blockDim.x >> 6);
    int idx = bcast((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)), 0);
    while (idx < count) {
        const int entry = bcast(io.queue[idx], 0);
        const int i = entry & EMP_Q_INST;
        MysteryDesc d;
        emp_serve_entry<true>(PS ? io.sets[set_index(io.set_of, i)] : P, io, W, entry, nullptr, reward_out, done_out, gt, info, autoreset, &d);
        if (me) {
            if (!autoreset && (entry & EMP_Q_SEGMENT) && done_out[i]) io.tdesc[i] = d;
            idx = waves + atomicAdd(&io.qctr[QC_HEAD], 1);
        }
        idx = bcast(idx, 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) queue_leave(&io.qctr[QC_LEFT], (int)gridDim.x, &io.qctr[QC_COUNT], &io.qctr[QC_HEAD]);
}

// mg_step of the endless variant, second launch: raster AND queue service in one.  The first EMP_SVC_WGS workgroups do what
// emp_serve_kernel does -- one queue entry per wave at a time -- and then draw the frames of the instances they served
// themselves (from the descriptor their wave just produced, kept in LDS); all other workgroups walk the frames of the
// instances that were NOT queued (MysteryDesc::valid == 1; emp_step_kernel marks the queued ones).  The 100 us of dependent path generation that a
// reset costs no longer stand in front of the raster: they run next to it, on a quarter of the resident workgroups.
// Measured (32,768 instances, us per step incl. the 26 us of emp_step_kernel; separate launches: 240): 384 / 512 / 768 /
// 1,024 / 1,536 service workgroups at 7 workgroups per CU (72 VGPRs, the path generator spills) 218 / 217 / 216 / 224 / 234;
// at 5 per CU (96 VGPRs) 212 / 211 / 215 / 224 / 227; at 4 per CU 210 / 212 / 213 / 219 / 223.
#ifndef MG_LAB_EMP_SVC  // measurement builds: -DMG_LAB_EMP_SVC=<workgroups> -DMG_LAB_EMP_LB=<workgroups per CU>
#define MG_LAB_EMP_SVC 256  // round 4, with non-temporal frame stores (round 3: 384, with lazy initial segments: profiles/r03_emp.md)
#endif
#ifndef MG_LAB_EMP_LB
#define MG_LAB_EMP_LB 6  // (round 5; rounds 3-4: 5)
#endif
#ifndef MG_LAB_EMP_SVC_SMALL
#define MG_LAB_EMP_SVC_SMALL 768
#endif
constexpr int EMP_SVC_WGS = MG_LAB_EMP_SVC, EMP_SVC_WGS_SMALL = MG_LAB_EMP_SVC_SMALL;
// Frame stores of the fused launch: NON-TEMPORAL (round 4).  Alone, a plain store stream is the faster one for these frames (110 us
// against 131 us for 32,768 of them, and every other launch of the mortar / mystery families keeps plain stores: -15 to -20 % with
// nt); beside the path service the plain stream takes 149-152 us and the non-temporal one still 129-136 us -- it does not push the
// service waves' working set (segment stores, queue, the generator's spills) out of the L2.  183-190 -> 203-209 M env-steps/s at
// 32,768 instances; buffer-addressed stores, 4 / 6 workgroups per CU, 256 / 512 / 768 service workgroups: all within 2 % of it
// (profiles/r04_emp.md).  Lab switch MEMGYM_EMP_NT=0 / 1 forces plain / non-temporal stores.
// Round 5: with the next episode's first segment generated ahead of time (EMP_PRE) the service queue is all but empty (a due segment
// now and then) and the PLAIN stream is the faster one again: same box, 32,768 instances, fused launch 123.5-123.9 us plain against
// 142-161 us non-temporal (without EMP_PRE: 159 plain, 128 non-temporal); 64 service workgroups instead of 256: 121.7 us.  The
// kernel therefore exists in both forms and the host picks (profiles/r05_emp.md).
#ifndef MG_LAB_EMP_SVC_PRE
#define MG_LAB_EMP_SVC_PRE 64
#endif
constexpr int EMP_SVC_WGS_PRE = MG_LAB_EMP_SVC_PRE;
#ifdef MG_LAB_EMP_CLOCK  // measurement builds only: per-workgroup start / end of service / end, constant-rate clock (10 ns)
static __device__ unsigned long long g_lab_emp_clock[3 * 16384];
#define LAB_CLOCK(slot) do { if (threadIdx.x == 0 && blockIdx.x < 16384) g_lab_emp_clock[3 * blockIdx.x + (slot)] = wall_clock64(); } while (0)
#else
#define LAB_CLOCK(slot) do { } while (0)
#endif
constexpr int EMP_BG_WGS = 512;  // at most so many workgroups behind the service workgroups take background jobs (EMP_BG_SPAN instances' flags each)
#ifndef MG_LAB_EMP_BG_SPAN
#define MG_LAB_EMP_BG_SPAN 256
#endif
constexpr int EMP_BG_SPAN = MG_LAB_EMP_BG_SPAN;
static_assert(EMP_BG_SPAN <= 256 || EMP_BG_SPAN % 256 == 0, "a background workgroup reads its span's flags 256 at a time");
static_assert(LW_BYTES <= v1::RASTER_LDS, "the lane generator's workspace must fit into the raster workgroup's LDS");
// (Round 4 tried the service and background workgroups as a launch of their own on a side stream beside a plain raster launch:
// bit-exact, 185 M env-steps/s against 189-192 M for this fused launch -- the raster alone takes 110 us, beside the service
// 136-144 us, and the fork / join costs ~10 us of stream time: profiles/r04_emp.md.  Taken out again.  So was the arguments-as-one-
// struct form that helped the spotlight family's fused kernel (service loop reading them through an opaque pointer where it uses
// them): scratch 672 -> 624 B only -- the path generator wants ~200 VGPRs whatever the scalar side does -- and the launch got
// SLOWER, 149-151 -> 156-164 us.)
template <int FMT, bool EMP_NT, bool FINAL = false>
__global__ __launch_bounds__(256, MG_LAB_EMP_LB) void emp_raster_serve_kernel(const MysteryDesc* __restrict__ descs, RasterAtlas A, void* __restrict__ obs, int n,
                                                                  MysteryParams P, MysteryIO io, float* reward_out, uint8_t* done_out,
                                                                  float* gt, mg_info_dev info, int autoreset, int svc, int bgw, int turn) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ MysteryDesc sdesc[4];
    __shared__ int served[4];
    const RasterCtx R = make_ctx(smem, A);
    const int tid = threadIdx.x;
    LAB_CLOCK(0);
    if ((int)blockIdx.x < svc) {
        // the service waves run a long dependent instruction chain next to memory-bound raster waves: let them issue first
        if (P.svc_prio) __builtin_amdgcn_s_setprio(3);
        uint8_t* ws = smem + FRAME_BYTES;  // the path workspace lives in the (unused) mask words behind the frame
        path_ws_init(ws);
        const PathWS W{ws, io.jump, io.stats};
        const int wv = tid >> 6;
        const bool me = (tid & 63) == 0;
        const int count = queue_count(&io.qctr[QC_COUNT], n);
        // bg_coop (launches of up to ~20,000 instances): the owed segments are entries count .. count + bg - 1 of the same queue --
        // with the lane-per-path generator of the frame workgroups (below) such a launch lasts as long as that generator's one
        // path, ~105 us, whatever its frames take
        const int bg = P.bg_coop ? queue_count(&io.qctr[QC_BG_COUNT], n) : 0;
        const int waves = svc * 4;
        int idx = bcast((int)(blockIdx.x * 4 + wv), 0);
        for (;;) {
            int inst = -1;
            if (idx < count + bg) {
                const int entry = idx < count ? bcast(io.queue[idx], 0) : (bcast(io.bgq[idx - count], 0) | EMP_Q_OWED);
#ifndef MG_LAB_EMP_NOSVC  // (measurement builds: what the launch costs without the cooperative generator's registers; entries are dropped)
                emp_serve_entry<FINAL>(P, io, W, entry, nullptr, reward_out, done_out, gt, info, autoreset, &sdesc[wv]);
#endif
                if (!(entry & EMP_Q_OWED)) inst = entry & EMP_Q_INST;
                if (me) idx = waves + atomicAdd(&io.qctr[QC_HEAD], 1);
                idx = bcast(idx, 0);
            }
            if (me) served[wv] = inst;
            __syncthreads();
            LAB_CLOCK(1);
            bool any = false;
            for (int w = 0; w < 4; ++w) {
                const int e = served[w];
                if (e < 0) continue;
                any = true;
                MysteryComposer::compose(&sdesc[w], R);
                __syncthreads();
                store_frame<FMT, EMP_NT>(smem, obs, e, tid);
                __syncthreads();
            }
            // (a round in which every wave served a background job draws nothing and goes on)
            const bool more = __syncthreads_or(idx < count + bg);
            if (!any && !more) break;
            __syncthreads();  // served[] / sdesc[] are rewritten by the next round: every wave has finished reading them
        }
        if (tid == 0) queue_leave(&io.qctr[QC_LEFT], svc, &io.qctr[QC_COUNT], &io.qctr[QC_HEAD], P.bg_coop ? &io.qctr[QC_BG_COUNT] : nullptr);
        LAB_CLOCK(2);
        return;
    }
    // Background jobs (owed segments, lazy initial segments; records ahead of time, EMP_PRE): the `bgw` workgroups behind the service
    // workgroups.  Workgroup b looks at the flags of instances b * EMP_BG_SPAN .. (emp_step_kernel wrote them), compacts the flagged
    // ones (~30 of 256 under random actions) into a list in LDS and its wave 0 takes up to 64 of them, one per lane, with the
    // lane-per-path generator in the workgroup's frame buffer; ~105 us that run beside the other workgroups' frames, and nothing of
    // this launch depends on them.  What does not fit a wave waits for the instance's next step (its flag is set again; the
    // list is entered at a position that moves with the launches, so no instance waits for ever): a workgroup that generates paths
    // holds a frame workgroup's slot for the whole launch and costs the store stream in proportion -- the same launch 124 us with
    // 128 such workgroups, 111 us with the jobs moved out of it (profiles/r05_emp.md) -- so they are few and full.  These workgroups
    // draw no frames (rounds 3-4: frame workgroups carried the jobs and went on to the frames of their stride afterwards).
    const int fb = svc + bgw;  // first frame workgroup
    if ((int)blockIdx.x < fb) {
        // (the list lives behind the lane generator's workspace in the frame buffer: 1 KB more of static LDS and the seventh workgroup
        // no longer fits a CU)
        int* const bg_jobs = reinterpret_cast<int*>(smem + LW_BYTES);
        int* const bg_cnt = bg_jobs + EMP_BG_SPAN;
        static_assert(LW_BYTES + EMP_BG_SPAN * 4 + 16 <= v1::RASTER_LDS && LW_BYTES % 16 == 0, "the job list must fit behind the lane generator's workspace");
        const int b = (int)blockIdx.x - svc;
#ifdef MG_LAB_EMP_NOBG  // (measurement builds: what the launch costs without the background jobs; owed segments are never generated here)
        if (b >= 0) return;
#endif
        bool ws = false;
        for (int base = b * EMP_BG_SPAN; base < n; base += bgw * EMP_BG_SPAN) {
            int total = 0;
            for (int c = 0; c < EMP_BG_SPAN; c += 256) {  // the span's flags, 256 at a time
                const int inst = base + c + tid;
                const bool want = c + tid < EMP_BG_SPAN && inst < n && io.bgflag[inst] != 0;
                const uint64_t m = __ballot(want);
                if ((tid & 63) == 0) bg_cnt[tid >> 6] = __popcll(m);
                __syncthreads();
                int off = total;
                for (int w = 0; w < (tid >> 6); ++w) off += bg_cnt[w];
                total += bg_cnt[0] + bg_cnt[1] + bg_cnt[2] + bg_cnt[3];
                if (want) bg_jobs[off + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = inst;
                __syncthreads();  // (the counts are rewritten by the next chunk; the list is complete behind the last one)
            }
            if (total && !ws) {
                lane_ws_init(smem);
                ws = true;
            }
            if (tid < 64) {
                if (P.svc_prio) __builtin_amdgcn_s_setprio(3);  // a long dependent chain next to memory-bound raster waves
                const LaneWS LW{smem, tid};
                const int rot = total > 64 ? (int)((unsigned)turn * 61u % (unsigned)total) : 0;
                if (tid < total) lane_owed_segment(io, LW, bg_jobs[(tid + rot) % total], 1, P.pre != 0);
            }
            __syncthreads();  // (the list is rewritten by the next round)
        }
        LAB_CLOCK(1);
        LAB_CLOCK(2);
        return;
    }
    const int stride = (int)gridDim.x - fb;
    for (int env = (int)blockIdx.x - fb; env < n; env += stride) {
        const MysteryDesc* d = descs + env;
        if (d->valid != 1) continue;  // masked, or drawn by the workgroup that serves its queue entry
        MysteryComposer::compose(d, R);
        __syncthreads();
        store_frame<FMT, EMP_NT>(smem, obs, env, tid);
        __syncthreads();
    }
    LAB_CLOCK(2);
}
}  // namespace mg
