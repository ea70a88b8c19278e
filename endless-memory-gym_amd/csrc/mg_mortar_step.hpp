// mg_mortar_step.hpp -- Mortar Mayhem family (included by mg_mortar.hip only): reset and step of one instance, a LANE each (mortar_reset, mortar_step_body in its
// two-launch, one-launch, claiming and terminal-frame forms), and the two kernels of the two-launch step: mortar_reset_kernel, mortar_step_kernel.
#pragma once
#include "mg_mortar_types.hpp"

namespace mg {
// (dx, dy) of command c: {1, 0, -1, 0, 0, 1, 1, -1, -1} / {0, 1, 0, -1, 0, 1, -1, 1, -1}, two bits each (value + 1) in a constant
// -- a table in memory is a dependent load per command in the reset's serial loop, with a lane-dependent index
constexpr uint32_t pack_deltas(const int (&v)[9]) {
    uint32_t m = 0;
    for (int c = 0; c < 9; ++c) m |= (uint32_t)(v[c] + 1) << (2 * c);
    return m;
}
constexpr int kDxHost[9] = {1, 0, -1, 0, 0, 1, 1, -1, -1}, kDyHost[9] = {0, 1, 0, -1, 0, 1, -1, 1, -1};
constexpr uint32_t CMD_DX_BITS = pack_deltas(kDxHost), CMD_DY_BITS = pack_deltas(kDyHost);
__device__ __forceinline__ int cmd_dx(int c) { return (int)((CMD_DX_BITS >> (2 * c)) & 3u) - 1; }
__device__ __forceinline__ int cmd_dy(int c) { return (int)((CMD_DY_BITS >> (2 * c)) & 3u) - 1; }

__device__ __forceinline__ int floordiv(int a, int b) {  // b > 0
    int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ int mod6(int a) { return ((a % 6) + 6) % 6; }
__device__ __forceinline__ int round_haz(double v) { return v >= 0 ? (int)floor(v + 0.5) : -(int)floor(-v + 0.5); }

// Env.reset body (RNG draw order: spawn tile, [offset x2], [command_count], commands, show dur/delay, explosion dur/delay)
// _encode_commands_one_hot (mortar_mayhem_b_grid.py:100-129): slot of a Command.COMMANDS id inside its block of 9
__constant__ int8_t kCmdOneHot[9] = {1, 4, 2, 3, 0, 5, 6, 7, 8};
constexpr int VEC_DIM = 180;  // max_num_commands (20) * 9

__device__ void mortar_reset(const MortarParams& P, MortarState& s, Pcg& g, uint8_t* cmds, MortarDesc& d, float* gt, float* vec) {
    // the frame keeps showing the previous agent's rect until the first execution step (Endless only can observe it)
    if (s.disp_sprite != 0xFF && s.disp_is_agent) {
        s.disp_x = s.ax;
        s.disp_y = s.ay;
        s.disp_is_agent = 0;
    }
    int half = P.tile / 2;
    int tile_id = g.integers(0, P.N * P.N);
    int cx = P.arena_x0 + P.tile * (tile_id / P.N) + half;
    int cy = P.arena_x0 + P.tile * (tile_id % P.N) + half;
    if (P.variant == V_ENDLESS || (P.taskb && P.variant == V_FREE)) {  // mortar_mayhem_b.py:167
        cx += g.integers(P.off_lo, P.off_hi);
        cy += g.integers(P.off_lo, P.off_hi);
    }
    s.ax = (int16_t)cx;
    s.ay = (int16_t)cy;
    s.rot8 = 0;
    int nx = floordiv(cx - P.arena_x0, P.tile), ny = floordiv(cy - P.arena_x0, P.tile);
    s.nx = (int8_t)nx;
    s.ny = (int8_t)ny;
    s.gx = (uint8_t)nx;
    s.gy = (uint8_t)ny;

    int n;
    if (P.variant == V_ENDLESS) {
        n = P.initial_count;
        for (int i = 0; i < n; ++i) cmds[i] = (uint8_t)g.integers(0, P.allowed);
    } else {
        n = choice(g, P.command_count);
        int px = nx, py = ny;
        for (int i = 0; i < n; ++i) {
            uint32_t valid = 0;  // bit c: command c keeps the agent inside the arena (the reference's list, in order)
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const int qx = px + cmd_dx(c), qy = py + cmd_dy(c);
                if (c < P.allowed && qx >= 0 && qx < P.N && qy >= 0 && qy < P.N) valid |= 1u << c;
            }
            const int pick = g.integers(0, __popc(valid));
            uint32_t m = valid;
            for (int k = 0; k < pick; ++k) m &= m - 1;  // pick-th entry of the list
            const int c = __ffs(m) - 1;
            cmds[i] = (uint8_t)c;
            px += cmd_dx(c);
            py += cmd_dy(c);
        }
    }
    s.num_cmds = (uint16_t)n;
    if (P.taskb) {  // mortar_mayhem_b_grid.py:172 `_command_visualization = None`: nothing is drawn (no draws either)
        s.show_dur = s.show_delay = 0;
    } else {
        s.show_dur = (uint16_t)choice(g, P.show_dur);
        s.show_delay = (uint16_t)choice(g, P.show_delay);
    }
    s.vis_len = (uint16_t)(n * (s.show_dur + s.show_delay));
    s.vis_base = 0;
    s.vis_pos = 1;  // reset pops the first entry for its own frame
    s.dbg_pops = 0;
    int first = cmds[0];
    uint8_t glyph = s.show_dur > 0 ? (uint8_t)first : (uint8_t)9;
    if (P.variant == V_ENDLESS) {
        s.tx = (int8_t)mod6(nx + cmd_dx(first));
        s.ty = (int8_t)mod6(ny + cmd_dy(first));
    } else {
        s.tx = (int8_t)(nx + cmd_dx(first));
        s.ty = (int8_t)(ny + cmd_dy(first));
    }
    s.cur_cmd = 0;
    s.cmd_steps = 0;
    s.verify_step = 0;
    s.total_completed = 0;
    s.tiles_on = 0;
    s.t = 0;
    s.ep_len = 0;
    s.ep_sum = 0.0;
    s.expl_dur = (uint16_t)choice(g, P.expl_dur);
    s.expl_delay = (uint16_t)choice(g, P.expl_delay);

    // reset frame: blue arena, sprite 0 at the NEW agent position, first glyph
    d.tmpl = 0;
    d.sprite = 0;
    d.sx = (int16_t)(cx - P.sprite_dim / 2);
    d.sy = (int16_t)(cy - P.sprite_dim / 2);
    d.glyph = glyph;
    if (gt) {
        gt[0] = (float)(s.tx / 5.0);
        gt[1] = (float)(s.ty / 5.0);
    }
    if (vec) {  // obs["vector_observation"]: constant over the episode, written once per reset
        for (int k = 0; k < VEC_DIM; ++k) vec[k] = 0.0f;
        for (int c = 0; c < n && c < VEC_DIM / 9; ++c) vec[9 * c + kCmdOneHot[cmds[c]]] = 1.0f;
    }
}

// PS: per-instance option sets -- the parameters come from memory, io.sets[set_index(io.set_of, i)], instead of from the kernel arguments
template <bool PS>
__global__ __launch_bounds__(256) void mortar_reset_kernel(MortarParams P0, int n, MortarIO io, const int64_t* seeds,
                                                           const uint8_t* mask, float* gt) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MortarParams& P = PS ? io.sets[set_index(io.set_of, i)] : P0;
    MortarDesc d;
    memset(&d, 0, sizeof(d));
    d.glyph_x0 = (int16_t)P.glyph_x0;
    if (mask && !mask[i]) {
        d.tmpl = 0xFFFF;
        io.desc[i] = d;
        return;
    }
    Pcg g;
    if (seeds) g.seed((uint64_t)seeds[i]);
    else g.load(io.rng, i);
    MortarState s = io.state[i];
    mortar_reset(P, s, g, io.cmds + (size_t)i * P.cmd_cap, d, gt ? gt + 2 * i : nullptr, io.vec ? io.vec + (size_t)i * VEC_DIM : nullptr);
    io.state[i] = s;
    g.store(io.rng, i);
    io.desc[i] = d;
}

// The step of instance i.  FUSED (the one-launch step, mortar_step_raster_kernel): the RNG stream is read where it is drawn
// (ten registers less: that kernel must fit the raster's 72 VGPRs without scratch) and the descriptor is handed to the
// frame workgroups of the SAME launch in a.handover[i]: one agent-scope (write-through) 64-bit store that carries the epoch.
// CLAIM (the step workgroups of the one-launch step): the wave steps its 64 instances only if it is the first to exchange this
// step's ticket into `claim_word` (see mortar_step_raster_kernel).  The exchange is ISSUED first and its answer awaited together
// with the state record: as a round trip of its own in front of the loads it delayed every descriptor, i.e. the whole launch,
// by 5-8 us (16,384 instances: 65 -> 73 us).
// FINAL (the one-launch step of a call that keeps terminal observations, mg_info_buffers.final_obs_dev): an instance that finishes
// publishes the descriptor of its TERMINAL frame in a.tdesc[i] (a word of the same layout) before it resets, and says so in the reset frame's
// hand-over word (ring_on, a field only the debug view uses otherwise): the frame workgroup draws the terminal frame into final_obs_dev first.
// ORDERED: every store of the lane in front of the hand-over word is complete before the word leaves (see there).
// RECORDS (mg_info_buffers.final_frames_dev, the two-launch / headless forms): an instance that finishes stores the descriptor of its TERMINAL frame -- the
// one the else branch at the end builds, before any reset -- to final_frames[i] as one 16-byte store; the rows of the others are not written.
template <bool FUSED, bool CLAIM = false, bool PS = false, bool FINAL = false, bool ORDERED = false, bool RECORDS = false>
__device__ __forceinline__ void mortar_step_body(int i, const MortarStepArgs& a, uint32_t epoch, uint32_t* claim_word = nullptr,
                                                 uint32_t ticket = 0u, const int32_t* actions_row = nullptr, MortarDesc* final_frames = nullptr) {
    uint32_t claimed_by = 0u;
    if constexpr (CLAIM) {
        claimed_by = ticket + 1u;  // lanes other than the wave's first: any value but the ticket
        if ((threadIdx.x & 63) == 0) claimed_by = __hip_atomic_exchange(claim_word, ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (the caller has dropped lanes with i >= n: the wave's first lane has its smallest i, so it is active whenever any lane is)
    }
    const MortarIO& io = a.io;
    const MortarParams& P = PS ? io.sets[set_index(io.set_of, i)] : a.P;  // (PS: per-instance option sets)
    const int32_t* const actions = actions_row ? actions_row : a.actions;  // (actions_row: mortar_play_kernel, row t of its tape)
    float* const reward_out = a.reward_out;
    uint8_t* const done_out = a.done_out;
    float* const gt = a.gt;
    const mg_info_dev& info = a.info;
    const int autoreset = a.autoreset;
    // the action is requested together with the state record (read where it is used -- behind a test of the state -- it was
    // a second memory round trip at the head of the kernel)
    // (both reads unconditional, the grid variant's second one a repeat of the first: a load inside the variant's branch was
    // waited for at the end of that branch)
    const bool one_action = P.variant == V_GRID;
    int act0 = actions[one_action ? i : 2 * i], act1 = actions[one_action ? i : 2 * i + 1];
    // ... and so is the instance's RNG stream (40 bytes): only a finishing instance or an Endless list extension draws, but
    // read where it is drawn it was a third round trip, in the reset's tail of every launch
    Pcg g;
    bool rng_loaded = !FUSED;
    if constexpr (!FUSED) g.load(io.rng, i);
    MortarState s = io.state[i];
    asm volatile("" : "+v"(act0), "+v"(act1));  // (a use the compiler cannot move below the record's first use)
    if constexpr (!FUSED) g.pin();
    if constexpr (CLAIM) {
        asm volatile("" : "+v"(claimed_by));
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)claimed_by) == ticket) return;  // a frame wave has stepped this slot already
    }
    uint8_t* cmds = io.cmds + (size_t)i * P.cmd_cap;
    double reward = 0.0;
    bool done = false, cap = false;
    int success = 0;
    uint8_t glyph = 0xFF;
    bool rng_used = false;

    if (s.vis_pos < s.vis_len) {
        // display phase: pop the next schedule entry, agent frozen
        int period = s.show_dur + s.show_delay;
        int k = s.vis_pos / period, w = s.vis_pos % period;
        glyph = (w < s.show_dur) ? cmds[s.vis_base + k] : (uint8_t)9;
        s.vis_pos++;
        if (P.variant != V_ENDLESS || s.disp_sprite == 0xFF) {
            s.disp_sprite = 0;  // get_rotated_sprite(0) with the live agent's rect
            s.disp_is_agent = 1;
        }
    } else {
        int ax = s.ax, ay = s.ay;
        if (P.variant == V_GRID) {
            int a = act0;
            int rot = s.rot8 * 45;
            if (a == 1) rot = (rot + 90) % 360;
            if (a == 2) rot = (rot + 270) % 360;
            int gx = s.gx, gy = s.gy;
            if (a == 3) {
                int face = rot / 90;  // 0 N, 1 W, 2 S, 3 E
                if (face == 0) { if (gy > 0) gy--; }
                else if (face == 3) { if (gx < P.N - 1) gx++; }
                else if (face == 2) { if (gy < P.N - 1) gy++; }
                else { if (gx > 0) gx--; }
                ax = P.arena_x0 + P.tile * gx + P.tile / 2;
                ay = P.arena_x0 + P.tile * gy + P.tile / 2;
            }
            s.gx = (uint8_t)gx;
            s.gy = (uint8_t)gy;
            s.rot8 = (uint8_t)(rot / 45);
        } else {
            int a0 = act0, a1 = act1;
            int dxs = a0 == 1 ? -1 : (a0 == 2 ? 1 : 0), dys = a1 == 1 ? -1 : (a1 == 2 ? 1 : 0);
            int rot = s.rot8 * 45;
            if (a0 == 1) rot = 90;
            if (a0 == 2) rot = 270;
            if (a1 == 1) rot = 0;
            if (a1 == 2) rot = 180;
            if (dxs < 0 && dys < 0) rot = 45;
            if (dxs < 0 && dys > 0) rot = 135;
            if (dxs > 0 && dys < 0) rot = 315;
            if (dxs > 0 && dys > 0) rot = 225;
            s.rot8 = (uint8_t)(rot / 45);
            bool diag = dxs != 0 && dys != 0;
            if (P.variant == V_FREE) {
                int v = diag ? P.v_diag_i : P.v_axis_i;
                ax += dxs * v;
                ay += dys * v;
                int lo = P.arena_x0 + P.radius, hi = P.arena_x0 + P.tile * P.N - P.radius;
                ax = ax > hi ? hi : ax;
                ax = ax < lo ? lo : ax;
                ay = ay > hi ? hi : ay;
                ay = ay < lo ? lo : ay;
            } else {
                double v = diag ? P.v_diag : P.v_axis;
                ax = round_haz((double)ax + dxs * v);
                ay = round_haz((double)ay + dys * v);
                // wrap once the centre passes the arena edge by radius * 0.5 (character_controller.py:269-281)
                double left = P.arena_x0, right = P.arena_x0 + P.tile * P.N, off = P.radius * 0.5;
                double x = ax, y = ay;
                if (x > right + off) x = left - off;
                if (x < left - off) x = right + off;
                if (y > right + off) y = left - off;
                if (y < left - off) y = right + off;
                ax = round_haz(x);
                ay = round_haz(y);
            }
        }
        s.ax = (int16_t)ax;
        s.ay = (int16_t)ay;
        s.disp_sprite = s.rot8;
        s.disp_is_agent = 1;
        int nx = floordiv(ax - P.arena_x0, P.tile), ny = floordiv(ay - P.arena_x0, P.tile);
        s.nx = (int8_t)nx;
        s.ny = (int8_t)ny;
        bool on_target = (nx == s.tx) && (ny == s.ty);

        bool verify = (s.cmd_steps % s.expl_delay == 0) && s.cmd_steps > 0;
        if (verify && !s.tiles_on) {
            if (s.cur_cmd < s.num_cmds) {
                s.cur_cmd++;
                s.tiles_on = 1;
                if (on_target) {
                    reward += P.r_succ;
                    if (P.variant == V_ENDLESS) {
                        s.total_completed++;
                        if (s.cur_cmd == s.num_cmds) reward += P.r_new;
                    }
                } else {
                    done = true;
                    reward += P.r_fail;
                }
            }
            if (s.cur_cmd >= s.num_cmds) {
                if (P.variant == V_ENDLESS) {
                    if (!rng_loaded) g.load(io.rng, i);
                    rng_loaded = true;
                    rng_used = true;
                    int nc = g.integers(0, P.allowed);
                    if (s.num_cmds < P.cmd_cap) {
                        cmds[s.num_cmds] = (uint8_t)nc;
                        s.vis_base = s.num_cmds;
                        s.num_cmds++;
                    } else {  // capacity reached (512 commands = 131,328 correct tile visits in one episode; the reference's
                        // list is unbounded, endless_mortar_mayhem.py:316-318): end the episode AND say so
                        raise_error(io.err, ERR_CMD_OVERFLOW);
                        done = true;
                        cap = true;
                        s.vis_base = (uint16_t)(s.num_cmds - 1);
                    }
                    s.cur_cmd = 0;
                    s.verify_step = 0;
                    s.vis_pos = 0;
                    s.vis_len = (uint16_t)(s.show_dur + s.show_delay);
                    s.dbg_pops = 0;
                } else {
                    done = true;
                    success = 1;
                    reward += P.r_ep_succ;
                }
            }
            s.cmd_steps = 1;
        }
        if (s.tiles_on) {
            if (s.verify_step % s.expl_dur == 0 && s.verify_step > 0) {
                s.tiles_on = 0;
                s.verify_step = 0;
                if (s.cur_cmd < s.num_cmds) {
                    int c = cmds[s.cur_cmd];
                    if (P.variant == V_ENDLESS) {
                        s.tx = (int8_t)mod6(s.tx + cmd_dx(c));
                        s.ty = (int8_t)mod6(s.ty + cmd_dy(c));
                    } else {
                        s.tx = (int8_t)(s.tx + cmd_dx(c));
                        s.ty = (int8_t)(s.ty + cmd_dy(c));
                    }
                }
            } else {
                if (!on_target) {
                    done = true;
                    reward = P.r_fail;  // overwrite (mortar_mayhem_grid.py:348)
                }
                s.verify_step++;
            }
        } else {
            s.cmd_steps++;
        }
    }

    if (P.variant == V_ENDLESS) {
        s.t++;
        if (s.t == P.max_steps) done = true;
    }
    s.ep_sum += reward;
    s.ep_len++;

    if (done) {
        if (info.ep_reward_dev) info.ep_reward_dev[i] = s.ep_sum;
        if (info.ep_length_dev) info.ep_length_dev[i] = s.ep_len;
        if (P.variant == V_ENDLESS) {
            if (info.aux_dev[0]) info.aux_dev[0][i] = (float)s.total_completed;
            if (info.aux_dev[1]) info.aux_dev[1][i] = (float)(s.num_cmds > 1 ? s.num_cmds - 1 : 0);
        } else {
            if (info.aux_dev[0]) info.aux_dev[0][i] = (float)success;
            if (info.aux_dev[1]) info.aux_dev[1][i] = (float)((double)((int)s.cur_cmd - 1 + success) / (double)s.num_cmds);
        }
    }
    reward_out[i] = (float)reward;
    if (info.reward64_dev) info.reward64_dev[i] = reward;  // the reference's Python float, unrounded
    done_out[i] = done ? 1 : 0;
    if (info.capacity_dev) info.capacity_dev[i] = cap ? 1 : 0;  // (include/memgym.h: the episode ended on a capacity of this build)

    MortarDesc d;
    memset(&d, 0, sizeof(d));
    d.glyph_x0 = (int16_t)P.glyph_x0;
    if constexpr (RECORDS) {
        if (done) {  // the terminal frame (the else branch below, which an auto-reset replaces), kept as its descriptor
            MortarDesc td = d;
            const int tcx = s.disp_is_agent ? s.ax : s.disp_x, tcy = s.disp_is_agent ? s.ay : s.disp_y;
            td.sx = (int16_t)(tcx - P.sprite_dim / 2);
            td.sy = (int16_t)(tcy - P.sprite_dim / 2);
            td.sprite = s.disp_sprite;
            td.glyph = glyph;
            td.tmpl = (uint16_t)((s.tiles_on && P.visual_feedback) ? 1 + s.tx * P.N + s.ty : 0);
            final_frames[i] = td;
        }
    }
    if (done && autoreset) {
        if constexpr (FINAL) {  // the terminal frame (the else branch below) as a hand-over word of its own, epoch 0: read only behind ring_on
            const int tcx = s.disp_is_agent ? s.ax : s.disp_x, tcy = s.disp_is_agent ? s.ay : s.disp_y;
            const uint64_t tw = pack_handover(tcx - P.sprite_dim / 2, tcy - P.sprite_dim / 2, (s.tiles_on && P.visual_feedback) ? 1 + s.tx * P.N + s.ty : 0,
                                              0, s.disp_sprite, glyph, 0);
            __hip_atomic_store(a.tdesc + i, tw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!rng_loaded) g.load(io.rng, i);
        rng_loaded = true;
        rng_used = true;
        mortar_reset(P, s, g, cmds, d, (gt && P.variant == V_ENDLESS) ? gt + 2 * i : nullptr, io.vec ? io.vec + (size_t)i * VEC_DIM : nullptr);
        if constexpr (FINAL) d.ring_on = 1;
    } else {
        int cx = s.disp_is_agent ? s.ax : s.disp_x, cy = s.disp_is_agent ? s.ay : s.disp_y;
        d.sx = (int16_t)(cx - P.sprite_dim / 2);
        d.sy = (int16_t)(cy - P.sprite_dim / 2);
        d.sprite = s.disp_sprite;
        d.glyph = glyph;
        d.tmpl = (uint16_t)((s.tiles_on && P.visual_feedback) ? 1 + s.tx * P.N + s.ty : 0);
        if (gt && P.variant == V_ENDLESS) {
            gt[2 * i] = (float)(s.tx / 5.0);
            gt[2 * i + 1] = (float)(s.ty / 5.0);
        }
    }
    if constexpr (FUSED) {
        // The hand-over: ONE relaxed agent-scope (write-through) 64-bit store, as soon as the descriptor is known -- the frame wave polls this word
        // and takes every field from the value that showed the epoch (a 64-bit access is single-copy atomic), so nothing has to precede it:
        //   plain form      no wait.  In that launch the frame wave reads nothing else this lane wrote (templates and stamps are the handle's).
        //   FINAL           a.tdesc[i] has reached the coherence point before the word whose ring_on announces it: s_waitcnt vmcnt(0) between the two.
        //   ORDERED         (the <DONE_FLAG> launch) the host reads reward, done and the episode record once the frame workgroup has stored the flag,
        //                   and that workgroup's release fence covers its OWN stores only: this lane's stores above are complete before the word leaves.
        if constexpr (FINAL || ORDERED) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(a.handover + i, pack_handover(d.sx, d.sy, d.tmpl, d.ring_on, d.sprite, d.glyph, epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (rng_used) g.store(io.rng, i);
    io.state[i] = s;
    io.desc[i] = d;  // (one plain 16-byte store: the two-launch raster, the sparse raster, mg_render and the debug view of LATER launches read it)
}

template <bool PS>
__global__ __launch_bounds__(256) void mortar_step_kernel(MortarStepArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) mortar_step_body<false, false, PS>(i, a, 0u);
}

// The MASKED form (mg_step_masked): the lane of an instance with active[i] == 0 zeroes the instance's reward / done and leaves; the others step as above.
template <bool PS>
__global__ __launch_bounds__(256) void mortar_step_masked_kernel(MortarStepArgs a, const uint8_t* __restrict__ active) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    if (active[i]) mortar_step_body<false, false, PS>(i, a, 0u);
    else masked_out(i, a.reward_out, a.done_out, a.info);
}

// The RECORDS forms of the two kernels above (mg_info_buffers.final_frames_dev): the lane of an instance that finishes keeps the terminal frame's descriptor in
// the caller's row.  The row pointer is an argument of these forms alone: MortarStepArgs is what it was for every other kernel.
template <bool PS, bool MASKED>
__global__ __launch_bounds__(256) void mortar_step_records_kernel(MortarStepArgs a, const uint8_t* __restrict__ active, MortarDesc* __restrict__ final_frames) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    if (!MASKED || active[i]) mortar_step_body<false, false, PS, false, false, true>(i, a, 0u, nullptr, 0u, nullptr, final_frames);
    else masked_out(i, a.reward_out, a.done_out, a.info);
}
}  // namespace mg
