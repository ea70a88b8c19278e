// mg_spot_serve.hpp -- Searing Spotlights family (included by mg_spot.hip only): the kernels around spot_reset and spot_step_body -- spot_reset_kernel, spot_step_kernel and
// spot_raster_serve_kernel, the raster launch that serves the step's queued resets, with its launch constants (MG_SPOT_SVC_*, MG_SPOT_SERVE_OCC; tools/build_variant.sh)
// and its hand-made memory ordering between a service workgroup's stores and its own scalar loads.
#pragma once
#include "mg_spot_compose.hpp"
#include "mg_spot_logic.hpp"

namespace mg {
// PS: per-instance option sets -- the parameters come from memory, io.sets[set_index(io.set_of, i)], instead of from the kernel arguments
template <bool EN, bool PS>
__global__ __launch_bounds__(256) void spot_reset_kernel(SpotParams P0, SpotIO io, const int64_t* seeds, const uint8_t* mask,
                                                         float* gt) {
    __shared__ int disc_lds[(256 / 16) * DISC_INTS];
    int gid = blockIdx.x * blockDim.x + threadIdx.x;
    int i = gid >> 4, ls = gid & 15;
    if (i >= P0.n) return;
    const SpotParams& P = PS ? io.sets[set_index(io.set_of, i)] : P0;
    if (mask && !mask[i]) {
        if (ls == 0) io.desc[i].valid = 0;
        return;
    }
    Pcg g;
    if (seeds) g.seed((uint64_t)seeds[i]);
    else g.load(io.rng, i);
    SpotCore s = io.core[i];
    SpotDesc d;
    const int stale_holes = frame_holes(&io.desc[i]);
    const LaneCtx L = lane_ctx((int)threadIdx.x);
    spot_reset<EN>(P, io, i, L, s, g, d, (gt && EN && ls == 0) ? gt + 4 * i : nullptr, stale_holes, disc_slot(disc_lds, L.grp));
    if (ls == 0) {
        io.core[i] = s;
        g.store(io.rng, i);
        store_desc_head(&io.desc[i], d);
    }
}

template <bool EN, bool PS>
__global__ __launch_bounds__(256) void spot_step_kernel(SpotStepArgs a) {
    __shared__ int disc_lds[(256 / 16) * DISC_INTS];  // step_block() launches 256 lanes at most
    __shared__ SpotCore core_lds[256 / 16];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = gid >> 4;
    // (a copy of the trig tables in LDS -- 5.8 KB per workgroup, one barrier -- measured: step kernel 19.9 -> 21.7 us, nothing gained)
    if (i < a.P.n) spot_step_body<EN, PS>(i, lane_ctx((int)threadIdx.x), a, disc_lds, core_lds, Trig{a.P.cos_tab, a.P.sin_tab});
}

// The MASKED form (mg_step_masked): the sixteen lanes of an instance with active[i] == 0 skip the step together -- its first lane zeroes the instance's reward / done.
// Nothing in spot_step_body reaches beyond the instance's own 16-lane group: its shuffles are 16 wide, its ballots are read through the group's own 16 bits
// (LaneCtx::gshift), the disc and core slots in LDS are the group's (LaneCtx::grp), and it has no barrier -- the lanes beyond n of the last group leave the same way.
template <bool EN, bool PS>
__global__ __launch_bounds__(256) void spot_step_masked_kernel(SpotStepArgs a, const uint8_t* __restrict__ active) {
    __shared__ int disc_lds[(256 / 16) * DISC_INTS];
    __shared__ SpotCore core_lds[256 / 16];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = gid >> 4;
    if (i >= a.P.n) return;
    if (active[i]) spot_step_body<EN, PS>(i, lane_ctx((int)threadIdx.x), a, disc_lds, core_lds, Trig{a.P.cos_tab, a.P.sin_tab});
    else if ((gid & 15) == 0) masked_out(i, a.reward_out, a.done_out, a.info);
}

// The RECORDS forms of the two kernels above (mg_info_buffers.final_frames_dev): the 16 lanes of an instance that finishes keep the terminal frame's descriptor in the
// caller's row (spot_step_body<.., RECORDS>).  The row pointer is an argument of these forms alone: SpotStepArgs is what it was for every other kernel.
template <bool EN, bool PS, bool MASKED>
__global__ __launch_bounds__(256) void spot_step_records_kernel(SpotStepArgs a, const uint8_t* __restrict__ active, SpotDesc* __restrict__ final_frames) {
    __shared__ int disc_lds[(256 / 16) * DISC_INTS];
    __shared__ SpotCore core_lds[256 / 16];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = gid >> 4;
    if (i >= a.P.n) return;
    if (!MASKED || active[i]) spot_step_body<EN, PS, true>(i, lane_ctx((int)threadIdx.x), a, disc_lds, core_lds, Trig{a.P.cos_tab, a.P.sin_tab}, final_frames);
    else if ((gid & 15) == 0) masked_out(i, a.reward_out, a.done_out, a.info);
}

// The step's raster launch with the put-off resets served inside it: the first workgroups take the queue entries, eight
// each (the 16 lanes of a quarter wave reset one instance, like spot_reset_kernel; waves 2 and 3 wait), then draw those
// eight frames; all other workgroups walk the frames of the instances that were not queued (SpotDesc::valid == 1).  The
// descriptors a service workgroup has just written are read back through the scalar cache like every descriptor: release,
// barrier, s_dcache_inv first.  Service workgroups without an entry leave at once and issue no atomic (thousands of them on
// one address: 22 ns each, in series).  What bounds the launch is a reset's latency next to the raster's waves (~45-80 us)
// plus the frames that follow it in the same workgroup; variants measured: profiles/r02_spot_resets.md.
#ifndef MG_SPOT_SVC_BATCH
#define MG_SPOT_SVC_BATCH 8
#endif
#ifndef MG_SPOT_SVC_WGS
#define MG_SPOT_SVC_WGS 512
#endif
constexpr int SPOT_SVC_WGS = MG_SPOT_SVC_WGS, SPOT_SVC_BATCH = MG_SPOT_SVC_BATCH;
static_assert(SPOT_SVC_BATCH * (DISC_INTS * 4 + (int)sizeof(SpotCore)) <= FRAME_BYTES, "a service batch's disc lists and core records fit into the frame area");
// Workgroups per CU of the fused launch (round 4, profiles/r04_spot_serve.md): SIX, non-temporal stores.  Rounds 2-3 ran it at five (96
// VGPRs and 104-124 B of scratch, 28 KiB of LDS): with the core record of a reset in LDS and the arguments of the service loop
// read where they are used, the endless variant needs 80 VGPRs and no scratch, the finite one 80 + 88-100 B.
#ifndef MG_SPOT_SERVE_OCC
#define MG_SPOT_SERVE_OCC 6
#endif

// FINAL (round 6): a call in the gymnasium vector convention.  The step kernel has stored a finishing instance's state and frame descriptor
// "as after any other step" (valid = DESC_QUEUED): that descriptor IS the terminal frame's -- the service workgroup draws it into final_obs
// before it resets the instance and draws the new episode's first frame into obs.  A kernel of its own; the measured ones are as they were.
// FMT: the observation format of both targets (obs and final_obs), handed to store_frame at the three store sites: the draw lambda, the FINAL
// loop and -- through the lambda -- the frame walk.  MG_OBS_U8_XYC is the default: those sixteen forms keep their names and their code.  The float
// formats ignore NT and BUF in store_frame and are launched with NT = false only (mg_spot.hip).
// MG_OBS_U8_CYX -- store_frame is then a collective of the 256 lanes with two barriers that transposes the LDS frame in place (frame_to_cyx's
// caller contract, mg_stream_out.hpp):
//   * uniform flow.  Every store site sits behind a __syncthreads() of this kernel, which already needs what the collective needs.  `service`,
//     `count`, `batch` and `base` come from blockIdx, the kernel arguments and one scalar load (queue_count): the same in every lane.  The two k
//     loops run to min(batch, count - base), uniform; the `tid < 16 * batch` branch between them holds no store site.  The frame walk's `valid != 1u`
//     is a scalar load through the constant address space: a scalar decision.
//   * nobody reads the transposed frame.  A store site is always compose -> barrier -> recycle (the hole mask behind the frame, not the frame) ->
//     store_frame -> barrier, and the next user of the frame area is either another compose, which writes all of the frame before anything reads
//     it (the Composer concept, mg_raster.hpp), or the service workgroup's reset: that one WRITES its disc lists and SpotCore records into the
//     frame area (disc_slot, `s = io.core[i]`) before it reads them and never looks at what a frame left there -- in this format as in the others,
//     where the area holds the last [x][y][c] frame at that point.  What the reset leaves in the area is in turn overwritten by the next compose.
//   * 256 lanes: dim3(256) is the only block size this kernel is launched with (__launch_bounds__(256, ...)).
template <bool EN, bool BORDER, bool NT, bool FINAL = false, int FMT = MG_OBS_U8_XYC>
__global__ __launch_bounds__(256, MG_SPOT_SERVE_OCC) void spot_raster_serve_kernel(SpotServeArgs a) {
    typedef SpotComposerT<BORDER> Composer;
    // the float forms call a store_frame instantiation of their own (SITE, mg_stream_out.hpp): sharing the raster kernels' moved THEIR code
    // (profiles/spot_chw.md); the one-byte forms share it as the uint8 form always has
    constexpr int SITE = (FMT == MG_OBS_U8_XYC || FMT == MG_OBS_U8_CYX) ? 0 : 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RasterCtx R = make_ctx(smem, a.A);
    const int tid = threadIdx.x;
    const int n = a.n;
    void* const obs = a.obs;
    const cptr<SpotDesc> cdescs = as_const(a.descs);
    const bool service = (int)blockIdx.x < SPOT_SVC_WGS;
    const int count = service ? queue_count(&a.io.qctr[SQ_COUNT], n) : 0;
    int batch = (count + SPOT_SVC_WGS - 1) / SPOT_SVC_WGS;
    batch = batch < a.batch_min ? a.batch_min : (batch > a.batch_max ? a.batch_max : batch);
    if (service && (int)blockIdx.x * batch >= count) return;
    Composer::recycle(R);
    __syncthreads();
    auto draw = [&](cptr<SpotDesc> from, int env) {
        typename Composer::Pre Pq;
        Composer::prefetch(from + env, R, Pq);
        Composer::compose(from + env, Pq, R);
        __syncthreads();
        Composer::recycle(R);
        store_frame<FMT, NT, true, SITE>(smem, obs, env, tid);
        __syncthreads();
    };
    if (service) {
        for (int base = blockIdx.x * batch; base < count; base += SPOT_SVC_WGS * batch) {
            const SpotServeArgs MG_KERNARG_AS* ka = kernarg_reread<SpotServeArgs>();
            const SpotParams& P = *(const SpotParams*)&ka->P;
            const SpotIO& io = *(const SpotIO*)&ka->io;
            float* const gt = ka->gt;
            if constexpr (FINAL) {  // the terminal frames of this round's instances, from the descriptors the step kernel left
                // (the draw lambda's body once more with another target: as one lambda with a target argument, or one lambda calling the
                // other, every variant of the kernel took 96-112 B of scratch and the frame loop ran three times as long)
                void* const fin = ka->final_obs;
                for (int k = 0; k < batch && base + k < count; ++k) {
                    const int env = io.queue[base + k];
                    typename Composer::Pre Pq;
                    Composer::prefetch(cdescs + env, R, Pq);
                    Composer::compose(cdescs + env, Pq, R);
                    __syncthreads();
                    Composer::recycle(R);
                    store_frame<FMT, NT, true, SITE>(smem, fin, env, tid);
                    __syncthreads();
                }
            }
            const int e = base + (tid >> 4), ls = tid & 15;
            if (tid < 16 * batch && e < count) {
                const int i = io.queue[e];
                Pcg g;
                g.load(io.rng, i);
                // disc lists and core records of the batch: in the FRAME area -- nothing of this workgroup is being composed while it
                // resets (the barriers around draw() separate the two uses) -- so the launch asks for no more LDS than the raster alone;
                // the core record in LDS instead of registers is what lets this kernel run at the raster's occupancy (round 4)
                const LaneCtx L = lane_ctx(tid);
                SpotCore& s = reinterpret_cast<SpotCore*>(smem + SPOT_SVC_BATCH * DISC_INTS * 4)[L.grp];
                s = io.core[i];
                SpotDesc d;
                const int stale_holes = frame_holes(&io.desc[i]);
                spot_reset<EN>(P, io, i, L, s, g, d, (gt && EN && ls == 0) ? gt + 4 * i : nullptr, stale_holes,
                               disc_slot(reinterpret_cast<int*>(smem), L.grp));
                d.valid = DESC_SERVED;
                if (ls == 0) {  // (spot_reset_kernel's three stores, spelled out at both sites: as one device function this kernel's code moved)
                    io.core[i] = s;
                    g.store(io.rng, i);
                    store_desc_head(&io.desc[i], d);
                }
            }
            // The descriptors just stored are read back by THIS workgroup's composers through the scalar cache: the stores have to
            // have reached the L2 (s_waitcnt vmcnt(0); the vector L1 writes through) and the scalar cache
            // must not answer from an older copy (s_dcache_inv).  NOT __threadfence(): at agent scope that is buffer_wbl2 +
            // buffer_inv -- a write-back of the whole L2, which holds the launch's observation stream (round 4: the cost of the
            // launch grew with the number of workgroups that served resets, profiles/r04_spot_serve.md).
            // Round 6 (a race the round-4 form had, found by tools/vector_soak.py: one reset frame in ~10^7 drawn from the OLD descriptor or
            // from a half-written one): the workgroup-scope release fence this stood on compiles to s_waitcnt lgkmcnt(0) only -- outside
            // tgsplit mode the vector L1 is coherent among a workgroup's waves, so LLVM's memory model leaves vmcnt out -- but the readers here
            // are SCALAR loads, which bypass the vector L1 and could reach the L2 before the stores did.  So: wait for the stores' acknowledgement
            // by hand, and for the invalidation (an SMEM operation, asynchronous like any other) before the first scalar load is issued;
            // the descriptor pointer passes through an opaque copy behind it, so that no load of the (constant-address-space, "invariant")
            // descriptor can be scheduled above the invalidation.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            __builtin_amdgcn_s_dcache_inv();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            cptr<SpotDesc> fresh = cdescs;
            asm volatile("" : "+s"(fresh));
            for (int k = 0; k < batch && base + k < count; ++k) draw(fresh, io.queue[base + k]);
        }
        const int busy = (count + batch - 1) / batch < SPOT_SVC_WGS ? (count + batch - 1) / batch : SPOT_SVC_WGS;
        // (spelled out: queue_leave (mg_family.hpp) also clears a `head` word, which this queue -- served in static rounds -- does not have)
        if (tid == 0 && atomicAdd(&a.io.qctr[SQ_LEFT], 1) == busy - 1) {  // last service workgroup out
            a.io.qctr[SQ_COUNT] = 0;
            a.io.qctr[SQ_LEFT] = 0;
        }
        return;
    }
    const int stride = (int)gridDim.x - SPOT_SVC_WGS;
    for (int env = (int)blockIdx.x - SPOT_SVC_WGS; env < n; env += stride) {
        if (cdescs[env].valid != 1u) continue;  // masked, or drawn by the workgroup that serves its reset
        draw(cdescs, env);
    }
}
}  // namespace mg
