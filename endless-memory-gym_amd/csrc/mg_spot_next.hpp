// mg_spot_next.hpp -- Searing Spotlights family (included by mg_spot.hip only): the NEXT form of the two-launch step (include/memgym.h: mg_step_next), kernels of
// their own beside spot_step_kernel / spot_reset_kernel, which stay the code they were.
//   spot_step_next_kernel   SIXTEEN LANES per instance, with spot_step_kernel's block size and LDS.  restart[i] != 0 -> the instance is reset by its 16 lanes, as
//                           spot_reset_kernel resets a masked-in instance with seeds == NULL (Env.reset, searing_spotlights.py:332-450,
//                           endless_searing_spotlights.py:294-407), and its leader reports the zeros of masked_out(); restart[i] == 0 -> spot_step_body with
//                           autoreset = 0, defer = 0 (Env.step, :452-562 / :409-506): the descriptor it leaves is the frame after the step, the terminal frame where done.
//   raster_kernel<SpotComposer>   the family's dense launch: every row of obs is written.
//   spot_next_settle_kernel   the descriptors of the instances that were NOT restarted get the valid = 0 the masked mg_reset of the definition leaves there: the
//                           descriptor rows are part of the checkpoint, which is bit for bit the composed form's.
// The flag is per instance, so the 16 lanes of a group branch together; the four groups of a wave may diverge.  Both bodies keep to their group -- 16-wide
// shuffles, ballots read through the group's own 16 bits (LaneCtx::gshift), the group's disc and core slots in LDS, no barrier -- as in
// spot_step_masked_kernel and in the step's in-kernel reset.
#pragma once
#include "mg_spot_logic.hpp"

namespace mg {
// restart and a.done_out may be the same memory (no __restrict__ on either): the 16 lanes of instance i read restart[i] with one vector load, the branch
// on it waits for the answer, and only then does the group's leader store done_out[i]; no other group touches entry i.
template <bool EN, bool PS>
__global__ __launch_bounds__(256) void spot_step_next_kernel(SpotStepArgs a, const uint8_t* restart, uint8_t* restart_copy) {
    __shared__ int disc_lds[(256 / 16) * DISC_INTS];  // step_block() launches 256 lanes at most
    __shared__ SpotCore core_lds[256 / 16];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = gid >> 4, ls = gid & 15;
    if (i >= a.P.n) return;
    const bool again = restart[i] != 0;
    if (ls == 0) restart_copy[i] = again ? 1 : 0;
    if (!again) return spot_step_body<EN, PS>(i, lane_ctx((int)threadIdx.x), a, disc_lds, core_lds, Trig{a.P.cos_tab, a.P.sin_tab});
    const SpotIO& io = a.io;
    const SpotParams& P = PS ? io.sets[set_index(io.set_of, i)] : a.P;
    Pcg g;
    g.load(io.rng, i);
    SpotCore s = io.core[i];
    SpotDesc d;
    const int stale_holes = frame_holes(&io.desc[i]);  // (read before anything of the instance is stored)
    const LaneCtx L = lane_ctx((int)threadIdx.x);
    spot_reset<EN>(P, io, i, L, s, g, d, (a.gt && EN && ls == 0) ? a.gt + 4 * i : nullptr, stale_holes, disc_slot(disc_lds, L.grp));
    if (ls == 0) {
        io.core[i] = s;
        g.store(io.rng, i);
        store_desc_head(&io.desc[i], d);
        masked_out(i, a.reward_out, a.done_out, a.info);
    }
}

__global__ __launch_bounds__(256) void spot_next_settle_kernel(int n, SpotIO io, const uint8_t* __restrict__ restart_copy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || restart_copy[i]) return;
    io.desc[i].valid = 0;  // (spot_reset_kernel, an instance its mask leaves out)
}
}  // namespace mg
