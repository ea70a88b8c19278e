// mg_mortar_one_launch.hpp -- Mortar Mayhem family (included by mg_mortar.hip only): mortar_step_raster_kernel, the step as ONE launch -- step workgroups and frame
// workgroups in one grid, the claim / epoch hand-over between them, RESCUE_AFTER_TICKS, and the MG_LABV measurement forms (tools/build_variant.sh).
#pragma once
#include "mg_mortar_compose.hpp"
#include "mg_mortar_step.hpp"

namespace mg {
using namespace v1;  // raster generation 1 (see mg_raster_v1.hpp)
// ONE launch per step (every observation format, FMT: mg_stream_out.hpp).  `logic_wgs` workgroups of the grid run the step (one lane per instance), all others
// are the raster's persistent workgroups; a frame's workgroup waits for ITS descriptor -- the epoch in the instance's hand-over
// word, read at agent scope past the caches -- instead of for the slowest wave of a separate logic launch plus that launch's
// fixed cost: the first frames leave ~8 us earlier (MortarMayhem-Grid 65,536: 233 -> 224 us per step, 281 -> 292 M env-steps/s;
// 16,384: 69 -> 65 us; profiles/r03_one_launch.md).
//
// Liveness does NOT rest on the order in which the hardware dispatches workgroups (round 4).  The instances are stepped in
// slots of 64 (one wave); a slot belongs to whichever wave first exchanges this step's ticket into its claim word.  Normally
// that is the step workgroup's wave (the step workgroups come first in the grid and are resident before the frame workgroups
// fill the chip).  A frame wave whose descriptor has not shown the epoch after RESCUE_AFTER_TICKS (200 us) tries the claim of the
// slot its frame belongs to ITSELF: if it wins, the step wave has not started yet (e.g. no free slot on the chip because frame
// workgroups were dispatched first) and the frame wave steps those 64 instances with its own lanes, then draws; if it loses,
// the slot's owner is a resident wave that never waits for anything, so the descriptor is on its way.  Every wait therefore
// ends, no frame is ever drawn from a stale descriptor, and there is no time-out to report (error bit 128 of rounds <= 3 is
// gone).  tests/test_gpu_one_launch.py runs the launch with the step workgroups LAST in the grid (lab build) -- every frame
// workgroup resident before any step workgroup -- and under a concurrent stream.
//
// Hand-over of the descriptor: ONE 64-bit word per instance (a.handover[i], layout in mg_mortar_handover.hpp: the fields the frame loop draws
// from, and the epoch in the top byte).  Writer: the instance's step lane, one relaxed agent-scope (write-through) 64-bit store as soon as the
// descriptor is known.  Reader: every wave of the frame's workgroup, relaxed agent-scope 64-bit loads until the epoch is this launch's; the
// descriptor is built in scalar registers from that SAME value.  A naturally aligned 64-bit access is single-copy atomic, so the value that
// shows the epoch is whole: no wait between words, no second load (until this form the descriptor went over as 3 + 1 words with an
// s_waitcnt vmcnt(0) between them and was read in two round trips; profiles/handover_word.md).  The word orders nothing else, and in the
// plain launch nothing else is handed over; the FINAL and <DONE_FLAG> forms keep one wait in front of it (mortar_step_body says for what).
// io.desc[i] is still written, as one plain 16-byte store behind the word: LATER launches read it (two-launch raster, sparse raster, debug view).
// Release / acquire atomics would be the textbook form; at agent scope on gfx950 they write back / invalidate
// the whole L2 of the XCD around every hand-over (buffer_wbl2 / buffer_inv sc1), with the observation stream in that L2.
// The two-launch form is used while a stream is being captured into a HIP graph (epoch and ticket are launch arguments: a
// replay would find them satisfied already) and for handles with instance groups (their stagger needs the logic launch's end).

// A frame wave tries the claim after it has waited this long (real-time clock, 100 MHz).  The step workgroups normally publish
// within 15-20 us; the first version counted 32 polls (~15 us as it turned out): every early frame wave then sent its one
// exchange at the few cache lines of claim words, and those ~7,000 serialised atomics cost the 16,384-instance launch 6 of
// its 66 us (profiles/r04_one_launch.md).
constexpr unsigned long long RESCUE_AFTER_TICKS = 20000;  // 200 us
// What a frame workgroup draws from, rebuilt from the two dwords of a hand-over word (glyph_x0 is not in the word: the launch runs under ONE option set)
__device__ __forceinline__ MortarDesc desc_from_handover(uint32_t lo, uint32_t hi, int glyph_x0) {
    const Handover f = unpack_handover(lo, hi);
    MortarDesc d;
    d.sx = (int16_t)f.sx, d.sy = (int16_t)f.sy, d.tmpl = (uint16_t)f.tmpl, d.sprite = (uint8_t)f.sprite, d.glyph = (uint8_t)f.glyph;
    d.glyph_x0 = (int16_t)glyph_x0;
    d.ring_x = d.ring_y = 0, d.ring_on = (uint8_t)f.ring_on, d.reserved = 0;
    return d;
}
// DONE_FLAG (the single-instance fast path, mg_single_step: ONE frame workgroup): when the frame is out, the workgroup stores `done_ticket`
// to `done_flag` -- a word in the caller's pinned block that the host polls -- at system scope: 2.7 us less per step than a stream memory
// operation behind the launch, 4.5 us less than hipStreamSynchronize (tools/microbench/launch_wait.hip).  Everything else the host reads
// (reward, done, the episode record) was stored by the step's wave, and waited for (mortar_step_body<ORDERED>), BEFORE it published the word this workgroup waited for.
// FINAL: the call keeps terminal observations (see mortar_step_body) -- a kernel of its own, the measured one (FINAL = false) is as it was.
// FMT: the stream-out format of both frames.  Every format but MG_OBS_U8_XYC has the plain and the FINAL form (no DONE_FLAG one: mg_single_step waits for the stream).
// Workgroups per CU the kernel is compiled for: 7 (72 VGPRs) for the one-byte formats, 6 (80 VGPRs) for the float ones -- their stream-out holds a
// lane's gather offsets and eight converted values next to the frame loop's own state, and under the bound of 7 the 16-bit forms spilled 13-14
// VGPRs (24 / 68 B of scratch per lane); with 6 no float form spills one (profiles/chw_final.md).
constexpr int one_launch_wgs_per_cu(int fmt) { return fmt == MG_OBS_U8_XYC || fmt == MG_OBS_U8_CYX ? 7 : 6; }
template <bool DONE_FLAG, bool FINAL = false, int FMT = MG_OBS_U8_XYC>
__global__ __launch_bounds__(256, one_launch_wgs_per_cu(FMT)) void mortar_step_raster_kernel(MortarStepArgs a, int logic_wgs, int logic_base, uint32_t epoch,
                                                                    uint32_t ticket, uint32_t* claims, uint32_t* rescues,
                                                                    RasterAtlas A, void* __restrict__ obs, uint32_t* done_flag, uint32_t done_ticket) {
    // The float stream-outs get this kernel's own instantiation of store_frame (SITE, mg_stream_out.hpp) and the lane index with its range
    // restored: the frame loop's index is opaque (below), and the raster kernels that share the float instantiations would be compiled for a
    // lane index of any sign with it (signed divisions in the lane's gather offsets).  The one-byte forms call what they always called.
    constexpr bool ONE_BYTE = one_launch_wgs_per_cu(FMT) == 7;
    auto store = [](uint8_t* frame, void* dst, int env, int t) {
        if constexpr (ONE_BYTE) store_frame<FMT, false>(frame, dst, env, t);
        else store_frame<FMT, false, false, 1>(frame, dst, env, t & 255);
    };
    const int n = a.n;
    const int tid = threadIdx.x, lane = tid & 63;
    const int rel = (int)blockIdx.x - logic_base;
    const bool is_logic = rel >= 0 && rel < logic_wgs;
    // true: this wave owns slot `q` (instances 64 q .. 64 q + 63) for this step
    auto claim = [&](int q) -> bool {
        uint32_t old = 0;
        if (lane == 0) old = __hip_atomic_exchange(claims + q, ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)old) != ticket;
    };
    if (is_logic) {  // a step workgroup: wave w steps slot 4 rel + w unless a frame wave got there first
        const int q = rel * 4 + (tid >> 6), i = q * 64 + lane;
#if defined(MG_LABV) && MG_LABV >= 1
        if (i < n) mortar_step_body<true, false, false, FINAL, DONE_FLAG>(i, a, epoch);
#else
        if (i < n) mortar_step_body<true, true, false, FINAL, DONE_FLAG>(i, a, epoch, claims + q, ticket);
#endif
        return;
    }
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RasterCtx R = make_ctx(smem, A);
    const int stride = (int)gridDim.x - logic_wgs;
    for (int v = (int)blockIdx.x < logic_base ? (int)blockIdx.x : (int)blockIdx.x - logic_wgs; v < n; v += stride) {
        const int env = xcd_grouped_frame(v, n);
        // every lane reads the same word (one transaction per wave); no barrier: the waves of a workgroup wait separately
        const uint64_t* src = a.handover + env;
        uint32_t lo, hi;
        bool tried = false;
        unsigned long long t0 = 0;
        for (int polls = 0;; ++polls) {
            // (all lanes read the same word; readfirstlane tells the compiler so: the wait loop's control and the descriptor stay scalar)
            const uint64_t w = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w);
            hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
            if ((hi >> (HANDOVER_EPOCH_SHIFT - 32)) == epoch) break;
#if defined(MG_LABV) && MG_LABV >= 2
            if (false) {
#else
            if (polls == 0) t0 = wall_clock64();
            if (!tried && (polls & 15) == 15 && wall_clock64() - t0 >= RESCUE_AFTER_TICKS) {  // (the clock is read every 16th poll)
#endif
                tried = true;  // (a lost claim is not retried: its owner is running)
                if (claim(env >> 6)) {  // rare: step the 64 instances around this frame here; the next poll finds the epoch
                    // The step's arguments are read AGAIN, from the kernel-argument segment, through a pointer the compiler
                    // cannot see through: as loop invariants they were hoisted out of the frame loop and kept in ~80 scalar
                    // registers for its whole length (spilled to vector lanes, those to scratch: 232 B per lane).
                    const MortarStepArgs MG_KERNARG_AS* ka = kernarg_reread<MortarStepArgs>();
                    int i = (env >> 6) * 64 + lane;
                    asm volatile("" : "+v"(i));  // (nor may what the step derives from `i` be computed at the head of every frame)
                    if (i < n) mortar_step_body<true, false, false, FINAL, DONE_FLAG>(i, *(const MortarStepArgs*)ka, epoch);
                    if (lane == 0) atomicAdd(rescues, 1u);
                    continue;
                }
            }
            __builtin_amdgcn_s_sleep(4);  // (1 and 2 measured no better: profiles/handover_word.md)
        }
        // the descriptor, from the SAME 64-bit value that showed the epoch: no second load, nothing to order
        const MortarDesc d = desc_from_handover(lo, hi, a.P.glyph_x0);
        if constexpr (FINAL) {
            if (d.ring_on) {  // the instance finished in this step: its terminal frame first, into the caller's final-observation buffer
                // (a.tdesc[env] had reached the coherence point before the word that has just been observed left its lane)
                // (both pointers re-read from the kernel-argument segment, like the rescue's arguments: held across the frame loop they cost it scratch)
                const MortarStepArgs MG_KERNARG_AS* ka = kernarg_reread<MortarStepArgs>();
                const uint64_t tw = __hip_atomic_load(ka->tdesc + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const MortarDesc td = desc_from_handover((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tw), (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tw >> 32)), a.P.glyph_x0);
                int tt = tid;
                asm volatile("" : "+v"(tt));
                R.tid = tt;
                MortarComposer::compose(&td, R);
                __syncthreads();
                store(smem, ka->info.final_obs_dev, env, tt);
                __syncthreads();
            }
        }
        if (MortarComposer::skip(&d)) continue;
        // the lane's frame offsets are derived from an opaque copy of its index, i.e. inside the iteration: as loop invariants
        // they were live across the (rare) step code above, which needs every register the kernel has
        int t = tid;
        asm volatile("" : "+v"(t));
        R.tid = t;
        MortarComposer::compose(&d, R);
        __syncthreads();
        store(smem, obs, env, t);  // (plain stores: non-temporal ones 281 -> 226-241 M at 65,536, round 4)
        __syncthreads();
    }
    if constexpr (DONE_FLAG) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // this wave's stores (the frame; after a rescue also the step's results) are performed system-wide
        __syncthreads();
        if (tid == 0) __hip_atomic_store(done_flag, done_ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
}  // namespace mg
