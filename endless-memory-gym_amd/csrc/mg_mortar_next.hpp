// mg_mortar_next.hpp -- Mortar Mayhem family (included by mg_mortar.hip only): the NEXT form of the two-launch step (include/memgym.h: mg_step_next), kernels
// of their own beside mortar_step_kernel / mortar_reset_kernel, which stay the code they were.
//   mortar_step_next_kernel   a LANE per instance: restart[i] != 0 -> the instance is reset by this lane, as mortar_reset_kernel resets a masked-in instance
//                             with seeds == NULL (Env.reset, mortar_mayhem_grid.py:213-278 and its siblings), and reports the zeros of masked_out();
//                             restart[i] == 0 -> mortar_step_body with autoreset = 0 (Env.step, :280-375): the descriptor it leaves is the frame after the
//                             step, the terminal frame where done.
//   raster_kernel<MortarComposer>   the family's dense launch: every row of obs is written.
//   mortar_next_settle_kernel   the descriptor rows of the instances that were NOT restarted become what the masked mg_reset of the definition leaves there
//                             ("leave the frame untouched"), so that the handle's memory is bit for bit the composed form's.
#pragma once
#include "mg_mortar_step.hpp"

namespace mg {
// restart and a.done_out may be the same memory (no __restrict__ on either): lane i reads restart[i] -- a per-lane vector load -- before anything of
// instance i is stored, and nobody else touches entry i.  restart_copy: the flags as read, for mortar_next_settle_kernel behind the raster.
template <bool PS>
__global__ __launch_bounds__(256) void mortar_step_next_kernel(MortarStepArgs a, const uint8_t* restart, uint8_t* restart_copy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const bool again = restart[i] != 0;
    restart_copy[i] = again ? 1 : 0;
    if (!again) return mortar_step_body<false, false, PS>(i, a, 0u);
    const MortarIO& io = a.io;
    const MortarParams& P = PS ? io.sets[set_index(io.set_of, i)] : a.P;
    MortarDesc d;
    memset(&d, 0, sizeof(d));
    d.glyph_x0 = (int16_t)P.glyph_x0;
    Pcg g;
    g.load(io.rng, i);
    MortarState s = io.state[i];
    mortar_reset(P, s, g, io.cmds + (size_t)i * P.cmd_cap, d, a.gt ? a.gt + 2 * i : nullptr, io.vec ? io.vec + (size_t)i * VEC_DIM : nullptr);
    io.state[i] = s;
    g.store(io.rng, i);
    io.desc[i] = d;
    masked_out(i, a.reward_out, a.done_out, a.info);
}

template <bool PS>
__global__ __launch_bounds__(256) void mortar_next_settle_kernel(MortarParams P0, int n, MortarIO io, const uint8_t* __restrict__ restart_copy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || restart_copy[i]) return;
    const MortarParams& P = PS ? io.sets[set_index(io.set_of, i)] : P0;
    MortarDesc d;  // (mortar_reset_kernel, an instance its mask leaves out)
    memset(&d, 0, sizeof(d));
    d.glyph_x0 = (int16_t)P.glyph_x0;
    d.tmpl = 0xFFFF;
    io.desc[i] = d;
}
}  // namespace mg
