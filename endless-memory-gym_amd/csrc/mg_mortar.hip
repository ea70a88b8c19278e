// mg_mortar.hip -- Mortar Mayhem family on gfx950: MortarMayhem-Grid-v0, MortarMayhem-v0, Endless-MortarMayhem-v0 (and the MortarMayhemB pair).  The family's one
// translation unit: the host class (MortarFamily) and three small kernels are here, the rest of the device code in headers that only this file includes.
//
// Reference behaviour reproduced (bit-exact observations, rewards, dones, RNG consumption):
//   memory_gym/mortar_mayhem_grid.py     reset :213-278  step :280-375
//   memory_gym/mortar_mayhem.py          reset :206-272  step :274-369
//   memory_gym/endless_mortar_mayhem.py  reset :194-259  step :261-373
//   memory_gym/character_controller.py   free :89-146  grid :177-210  screen-wrap :226-283
//   memory_gym/pygame_assets.py          Command :241-304  MortarTile/MortarArena :306-418
//
//   mg_mortar_handover.hpp    the 64-bit word that carries a frame descriptor from a step lane to a frame workgroup of the same launch (host-includable)
//   mg_mortar_types.hpp       the variant constants; MortarParams, MortarState, MortarDesc, MortarIO, MortarStepArgs
//   mg_mortar_compose.hpp     MortarComposer (the observation) and MortarDebugComposer, with the measurement hooks MG_LAB_NO_TEMPLATE / MG_LAB_NO_STAMPS
//   mg_mortar_step.hpp        reset and step of one instance (mortar_reset, mortar_step_body); mortar_reset_kernel, mortar_step_kernel
//   mg_mortar_one_launch.hpp  mortar_step_raster_kernel: the step as one launch, its claim / hand-over word, RESCUE_AFTER_TICKS
//   mg_mortar_expert.hpp      mortar_expert_kernel: the scripted teacher of the five ids (mg_expert_actions), a launch of its own
//   mg_mortar_advance.hpp     mortar_advance_kernel: K steps under the teacher without a frame (mg_advance), teacher + step + sums per lane in one launch
//   mg_mortar_play.hpp        mortar_play_kernel: K steps of a caller-supplied action tape without a frame (mg_play), step + traces + sums per lane in one launch
//   mg_mortar_trace.hpp       mortar_advance_traced_kernel / mortar_play_traced_kernel: the two above as kernels of their own that also keep every step's frame
//                             descriptor, action, teacher's label, reward and done (mg_advance_traced / mg_play_traced)
//   mg_mortar_next.hpp        mortar_step_next_kernel / mortar_next_settle_kernel: the NEXT form of the two-launch step (mg_step_next), a flagged instance is reset
//                             by its lane instead of stepped
//
// The launches of a step as shipped:
//   ONE launch for handles with one option set, in every observation format (mortar_step_raster_kernel: the step's workgroups lead the raster's grid and a frame waits for its own
//   descriptor; terminal observations kept, mg_info_buffers.final_obs_dev: its <FINAL> form; mg_single_step, MG_OBS_U8_XYC: its <DONE_FLAG> form), two launches otherwise
//   (per-instance option sets, HIP-graph capture):
//   mortar_step_kernel : one LANE per environment instance.  Episode state machine, RNG, reward/done/info; emits a
//                   16-byte frame descriptor per instance.  State is small fixed-size records in HBM, read and
//                   written fully coalesced (lane i <-> record i).
//   raster_kernel<MortarComposer> : (mg_raster_v1.hpp) persistent workgroups, one frame at a time in LDS: arena
//                   template (selected by tiles-on / target tile) -> agent sprite stamp -> command glyph stamp.
#include <memory>

#include "mg_atlas_v1.hpp"
#include "mg_lab.hpp"
#include "mg_option_sets.hpp"
#include "mg_stamps.hpp"
#include "mg_mortar_types.hpp"
#include "mg_mortar_compose.hpp"
#include "mg_raster_gather_v1.hpp"
#include "mg_mortar_step.hpp"
#include "mg_mortar_one_launch.hpp"
#include "mg_mortar_expert.hpp"
#include "mg_mortar_advance.hpp"
#include "mg_mortar_play.hpp"
#include "mg_mortar_trace.hpp"
#include "mg_mortar_next.hpp"

namespace mg {
using namespace v1;  // raster generation 1 (see mg_raster_v1.hpp)

__global__ __launch_bounds__(256) void mortar_init_kernel(int n, MortarState* state) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    MortarState s;
    memset(&s, 0, sizeof(s));
    s.disp_sprite = 0xFF;
    state[i] = s;
}

// info["ground_truth"] in float64: target tile / 5.0 (endless_mortar_mayhem.py:259,358,362)
__global__ __launch_bounds__(256) void mortar_gt64_kernel(int n, const MortarState* state, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MortarState s = state[i];
    out[2 * i] = s.tx / 5.0;
    out[2 * i + 1] = s.ty / 5.0;
}

__global__ __launch_bounds__(256) void mortar_gt64_masked_kernel(int n, const MortarState* state, double* out, const uint8_t* __restrict__ only) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !only[i]) return;
    const MortarState s = state[i];
    out[2 * i] = s.tx / 5.0;
    out[2 * i + 1] = s.ty / 5.0;
}

// Debug view: the frame descriptors of the current frames with (a) the glyph the reference's CLONE of the display schedule
// yields -- its next entry, popped (dbg_pops, the only state a debug render changes), only while the real schedule still
// holds entries (oracle/mgo_mortar.c mm_debug) -- and (b) the ring around the target tile.
__global__ __launch_bounds__(256) void mortar_debug_desc_kernel(MortarParams P0, int n, MortarIO io, MortarDesc* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MortarParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    const MortarState s = io.state[i];
    const uint8_t* cmds = io.cmds + (size_t)i * P.cmd_cap;
    MortarDesc d = io.desc[i];
    {   // the agent the debug view shows is the stored (rotated_agent_surface, rotated_agent_rect) pair, which no reset clears
        // (mortar_mayhem_grid.py:115-118): stale from the previous episode until the first step; sprite 0 before any step
        const bool have = s.disp_sprite != 0xFF;
        const int cx = (have && !s.disp_is_agent) ? s.disp_x : s.ax, cy = (have && !s.disp_is_agent) ? s.disp_y : s.ay;
        d.sx = (int16_t)(cx - P.sprite_dim / 2);
        d.sy = (int16_t)(cy - P.sprite_dim / 2);
        d.sprite = have ? s.disp_sprite : (uint8_t)0;
        d.tmpl = (uint16_t)((s.tiles_on && P.visual_feedback) ? 1 + s.tx * P.N + s.ty : 0);
        d.glyph_x0 = (int16_t)P.glyph_x0;
    }
    d.glyph = 0xFF;
    if (s.vis_pos < s.vis_len) {
        const int idx = (int)s.dbg_pops, period = s.show_dur + s.show_delay;
        io.state[i].dbg_pops = s.dbg_pops + 1;
        if (idx >= 0 && idx < (int)s.vis_len && period > 0) {
            const int k = idx / period, w = idx % period;
            d.glyph = (w < s.show_dur) ? cmds[s.vis_base + k] : (uint8_t)9;
        }
    }
    const int r = P.tile / 2;  // pygame.draw.circle(surface, green, tile centre, tile_dim // 2, int(8 * SCALE))
    d.ring_x = (int16_t)(P.arena_x0 + P.tile * s.tx + P.tile / 2 - r);
    d.ring_y = (int16_t)(P.arena_x0 + P.tile * s.ty + P.tile / 2 - r);
    d.ring_on = 1;
    out[i] = d;
}

// The same descriptor for ONE instance, for the picked form below (a body of its own: mortar_debug_desc_kernel stays the code it was).
__device__ __forceinline__ MortarDesc mortar_debug_desc_one(const MortarParams& P, const MortarIO& io, int i) {
    const MortarState s = io.state[i];
    const uint8_t* cmds = io.cmds + (size_t)i * P.cmd_cap;
    MortarDesc d = io.desc[i];
    {   // the agent the debug view shows is the stored (rotated_agent_surface, rotated_agent_rect) pair, which no reset clears
        // (mortar_mayhem_grid.py:115-118): stale from the previous episode until the first step; sprite 0 before any step
        const bool have = s.disp_sprite != 0xFF;
        const int cx = (have && !s.disp_is_agent) ? s.disp_x : s.ax, cy = (have && !s.disp_is_agent) ? s.disp_y : s.ay;
        d.sx = (int16_t)(cx - P.sprite_dim / 2);
        d.sy = (int16_t)(cy - P.sprite_dim / 2);
        d.sprite = have ? s.disp_sprite : (uint8_t)0;
        d.tmpl = (uint16_t)((s.tiles_on && P.visual_feedback) ? 1 + s.tx * P.N + s.ty : 0);
        d.glyph_x0 = (int16_t)P.glyph_x0;
    }
    d.glyph = 0xFF;
    if (s.vis_pos < s.vis_len) {
        const int idx = (int)s.dbg_pops, period = s.show_dur + s.show_delay;
        io.state[i].dbg_pops = s.dbg_pops + 1;
        if (idx >= 0 && idx < (int)s.vis_len && period > 0) {
            const int k = idx / period, w = idx % period;
            d.glyph = (w < s.show_dur) ? cmds[s.vis_base + k] : (uint8_t)9;
        }
    }
    const int r = P.tile / 2;  // pygame.draw.circle(surface, green, tile centre, tile_dim // 2, int(8 * SCALE))
    d.ring_x = (int16_t)(P.arena_x0 + P.tile * s.tx + P.tile / 2 - r);
    d.ring_y = (int16_t)(P.arena_x0 + P.tile * s.ty + P.tile / 2 - r);
    d.ring_on = 1;
    return d;
}
// mg_save_debug_frames: record j <- the debug descriptor of instance idx[j] (idx == NULL: instance j), one lane per entry; the named instances are the
// ones whose display-schedule clone is popped.  An entry < 0 is skipped, one >= n is skipped and flagged; a skipped entry's record is not written.
__global__ __launch_bounds__(256) void mortar_debug_desc_picked_kernel(MortarParams P0, int n, MortarIO io, const int32_t* __restrict__ idx, int count,
                                                                       MortarDesc* rec) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const int i = idx ? idx[j] : j;
    if (i < 0) return;
    if (i >= n) return raise_error(io.err, ERR_FRAME_INDEX);
    const MortarParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    rec[j] = mortar_debug_desc_one(P, io, i);
}

// ---------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------
static const double SCALE = 0.25;  // the reference's module constant (e.g. mortar_mayhem_grid.py:13)

class MortarFamily : public Family {
   public:
    // variant 3 / 4 = MortarMayhemB-Grid-v0 / MortarMayhemB-v0: the Grid / free machine with taskb set
    MortarFamily(int variant_id, int n) : Family(n), P_(sets_[0].P) {
        memset(&P_, 0, sizeof(P_));
        const int variant = variant_id >= 3 ? variant_id - 3 : variant_id;
        P_.variant = variant;
        P_.taskb = variant_id >= 3;
        agent_scale_ = 1.0 * SCALE;
        agent_speed_ = 12.0 * SCALE;
        P_.N = variant == V_ENDLESS ? 6 : 5;
        P_.allowed = variant == V_GRID ? 5 : 9;
        P_.visual_feedback = 1;
        P_.max_steps = -1;
        P_.initial_count = 1;
        P_.cmd_cap = variant == V_ENDLESS ? 512 : 32;
        if (variant == V_ENDLESS) {  // lab build only (tests/test_gpu_error_bits.py): a small capacity makes the overflow reachable
            const int cap = lab_int("MEMGYM_EMM_CMD_CAP", 0);
            if (cap >= 4 && cap <= 512) P_.cmd_cap = cap;
        }
        MortarOpt& O = sets_[0];
        O.st_command_count.set(P_.command_count, {10});
        O.st_show_dur.set(P_.show_dur, {3});
        O.st_show_delay.set(P_.show_delay, {1});
        O.st_expl_dur.set(P_.expl_dur, {variant == V_GRID ? 2 : 6});
        O.st_expl_delay.set(P_.expl_delay, {variant == V_GRID ? 6 : 18});
        P_.r_fail = 0.0;
        P_.r_succ = 0.1;
        P_.r_ep_succ = 0.0;
        P_.r_new = 0.0;
        state_.alloc(n);
        cmds_.alloc((size_t)n * P_.cmd_cap);
        desc_.alloc(n);
        tdesc_.alloc(n);  // (terminal-frame words of the FINAL one-launch step: 8 B per instance; allocated here so that no step allocates)
        rng_.alloc(n);
        err_.alloc();
        claims_.alloc((size_t)((n + 255) / 256) * 4);
        handover_.alloc(n);  // (zeroed: epoch 0 is never a one-launch epoch; transient within a launch, so no part of state_blobs())
        rescues_.alloc(1);
        sets_.alloc();
        launch(mortar_init_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, state_.p);
        MG_HIP(hipDeviceSynchronize());
        rebuild();
        sets_.defaults = P_;
    }

    // include/memgym.h: mg_set_capacity.  "commands" (Endless-MortarMayhem-v0): entries of the command list per instance -- the reference's
    // list grows by one with every completed round (endless_mortar_mayhem.py:311-333); an episode that would need one more ends (capacity_dev)
    void set_capacity(const std::string& what, int64_t v) override {
        if (!(P_.variant == V_ENDLESS && what == "commands")) return Family::set_capacity(what, v);
        if (v < 4 || v > 32768) throw OptionError{-3, "commands: 4 .. 32,768"};
        if (seeded_) throw std::runtime_error("mg_set_capacity: before the first reset");
        if (2 * P_.initial_count > v) throw OptionError{-3, "commands: below twice the initial_command_count in force"};
        MG_HIP(hipDeviceSynchronize());
        P_.cmd_cap = (int)v;
        cmds_.alloc((size_t)n_ * P_.cmd_cap);
        ++geom_gen_;
        sets_.refresh_geometry();
    }
    int64_t capacity(const std::string& what) const override {
        if (P_.variant == V_ENDLESS && what == "commands") return P_.cmd_cap;
        return Family::capacity(what);
    }
    // mg_single_step: a request to the next step() alone, which grants it where it takes the one-launch form (see there)
    void want_done_flag(uint32_t* flag_dev, uint32_t ticket) override {
        flag_dev_ = flag_dev;
        flag_ticket_ = ticket;
    }
    bool done_flag_stored() override {
        const bool stored = flag_stored_;
        flag_stored_ = false;
        return stored;
    }
    int action_dim() const override { return P_.variant == V_GRID ? 1 : 2; }
    int gt_dim() const override { return P_.variant == V_ENDLESS ? 2 : 0; }
    int vec_dim() const override { return P_.taskb ? VEC_DIM : 0; }
    void bind_vector_obs(float* dev) override {
        if (dev != vec_) ++geom_gen_;  // (the bound row travels in an instance record: instance_rows)
        vec_ = dev;
    }
    const char* info_name(int k) const override {
        if (P_.variant == V_ENDLESS) return k == 0 ? "commands_completed" : (k == 1 ? "max_command_sequence" : nullptr);
        return k == 0 ? "success" : (k == 1 ? "commands_completed" : nullptr);
    }

    // One key of the reset options, for option set `set` (0 = the handle-wide set of mg_set_option).  Sets > 0 hold everything
    // that does not change the geometry (atlases and templates are shared by the handle's instances).
    void set_option(const std::string& key, const double* v, int n) override { set_option_set(0, key, v, n); }
    void set_option_set(int set, const std::string& key, const double* v, int n) override {
        MortarOpt& O = sets_.ensure(set);
        MortarParams& P = O.P;
        const bool endless = P_.variant == V_ENDLESS;
        const OptionArg A{set, key, v, n, dirty_};
        if (key == "agent_scale") A.geometry(agent_scale_, v[0]);
        else if (key == "allowed_commands") {
            int a = A.integer();
            if (a < 4 || a > 9) throw OptionError{-4, "assert 4 <= allowed_commands <= 9"};
            P.allowed = a;
        }
        // (entries are 16 bits in MortarState; an explosion entry of 0 is the reference's ZeroDivisionError in `% explosion_delay` (:304,343),
        // a show duration of 0 with a delay of 0 its IndexError at the reset's pop(0) (:257))
        else if (!P_.taskb && key == "command_show_duration") O.st_show_dur.set(P.show_dur, A.int_list(1, 65535));
        else if (!P_.taskb && key == "command_show_delay") O.st_show_delay.set(P.show_delay, A.int_list(0, 65535));
        else if (key == "explosion_duration") O.st_expl_dur.set(P.expl_dur, A.int_list(1, 65535));
        else if (key == "explosion_delay") O.st_expl_delay.set(P.expl_delay, A.int_list(1, 65535));
        else if (key == "visual_feedback") P.visual_feedback = A.flag();
        else if (key == "reward_command_failure") P.r_fail = v[0];
        else if (key == "reward_command_success") P.r_succ = v[0];
        else if (endless && key == "max_steps") P.max_steps = A.integer();
        else if (endless && key == "initial_command_count") {
            int c = A.integer();
            if (c < 1 || c > P_.cmd_cap / 2) throw OptionError{-3, "initial_command_count out of the supported range"};
            P.initial_count = c;
        }
        else if (endless && key == "reward_new_command_success") P.r_new = v[0];
        else if (!endless && key == "arena_size") {
            int a = A.integer();
            if (a < 2 || a > MORTAR_MAX_N) throw OptionError{-4, "assert 2 <= arena_size <= 6"};  // (MORTAR_MAX_N: what the hand-over word's template field is checked against)
            if (a != P_.N) A.geometry(P_.N, a);  // (the one geometry key that asks for a rebuild only when its value changes)
        }
        else if (!endless && key == "command_count") O.st_command_count.set(P.command_count, A.int_list(1, P_.taskb ? VEC_DIM / 9 : P_.cmd_cap));
        else if (!endless && key == "reward_episode_success") P.r_ep_succ = v[0];
        else if (P_.variant != V_GRID && key == "agent_speed") A.geometry(agent_speed_, v[0]);
        else throw OptionError{-2, "unknown reset parameter " + key};
    }
    void bind_option_sets(const int32_t* set_of_dev) override { sets_.bind(set_of_dev); }

    void reset(const int64_t* seeds, const uint8_t* mask, void* obs, float* gt, hipStream_t s) override {
        if (dirty_) rebuild();
        require_seeded(seeds);
        check_schedules();
        if (seeds) seeded_ = true;  // with a mask the caller is responsible for having seeded the other instances
        sets_.upload(s);
        with_bool(sets_.per_set(), [&](auto PS) {
            launch(mortar_reset_kernel<decltype(PS)::value>, dim3((n_ + 255) / 256), dim3(256), 0, s, P_, n_, io(), seeds, mask, gt_dim() ? gt : nullptr);
        });
        reset_frames(mask, [&](const uint8_t* m) { launch_raster_sparse<MortarComposer>(desc_.p, atlas_->dev(), obs, obs_format, n_, s, m); },
                     [&] { raster(obs, s); });
    }

    void step(const int32_t* actions, const uint8_t* active, void* obs, float* reward, uint8_t* done, float* gt, const mg_info_dev* info,
              int autoreset, hipStream_t s, void* final_frames) override {
        struct Consume {  // want_done_flag() holds for this call only, whichever way it ends
            uint32_t*& flag;
            ~Consume() { flag = nullptr; }
        } consume{flag_dev_};
        flag_stored_ = false;
        const mg_info_dev ib = begin_step(info);
        sets_.upload(s);
        const MortarStepArgs sa = step_args(actions, reward, done, gt, ib, autoreset);
        // one launch: mortar_step_raster_kernel (handles with ONE option set: the per-set step code reads its parameters from memory)
        // (a headless step, obs == NULL: mortar_step_kernel alone; a masked step, active != NULL: its MASKED form, then the active instances' frames)
        if (obs && !active && one_launch(s)) {
            epoch_ = epoch_ % 255u + 1u;  // 1 .. 255: never the 0 of a fresh hand-over array (resets and two-launch steps do not write the words)
            ++ticket_;                    // claim words hold the ticket of the last one-launch step: never this one
            const int logic_wgs = (n_ + 255) / 256;
            const int frames = frames_grid(n_);
            // lab build, MEMGYM_LAB_LOGIC_LAST=1: the step workgroups at the END of the grid -- the dispatch order the design must survive
            static const bool logic_last = lab_flag("MEMGYM_LAB_LOGIC_LAST", false);
            // The done flag (want_done_flag) is granted here: this launch is the step's last kernel, and with ONE instance and no ground
            // truth (mg_single_step puts a ground_truth64 launch behind the step) nothing follows it.  (Three of the four <FLAG, FINAL>
            // forms exist: the flag is asked for by single steps, which pass autoreset = 0, so it never meets kept terminal observations.)
            // (MG_OBS_U8_XYC alone has a <DONE_FLAG> form: single steps in the other formats are the plain launch, and mg_single_step waits for the stream)
            const bool store_flag = flag_dev_ && n_ == 1 && gt_dim() == 0 && obs_format == MG_OBS_U8_XYC;
            auto launch_step = [&](auto kernel, const MortarStepArgs& a, uint32_t* flag, uint32_t flag_ticket) {
                launch(kernel, dim3(logic_wgs + frames), dim3(256), RASTER_LDS, s, a, logic_wgs, logic_last ? frames : 0, epoch_, ticket_,
                               claims_.p, rescues_.p, atlas_->dev(), obs, flag, flag_ticket);
            };
            prof.begin(1, s);
            if (store_flag) {
                launch_step(mortar_step_raster_kernel<true>, sa, flag_dev_, flag_ticket_);
            } else if (ib.final_obs_dev && autoreset) {  // terminal observations kept by the launch itself (keeps_final_obs)
                MortarStepArgs fa = sa;
                fa.tdesc = tdesc_.p;
                with_obs_format(obs_format, [&](auto F) { launch_step(mortar_step_raster_kernel<false, true, decltype(F)::value>, fa, nullptr, 0u); });
            } else {
                with_obs_format(obs_format, [&](auto F) { launch_step(mortar_step_raster_kernel<false, false, decltype(F)::value>, sa, nullptr, 0u); });
            }
            check_launch();
            ++one_launch_steps_;
            flag_stored_ = store_flag;
            prof.end(1, s);
            return;
        }
        prof.begin(0, s);
        const int sb = step_block(256);
        with_bool(sets_.per_set(), [&](auto PS) {
            if (final_frames) {  // (terminal frame records: the RECORDS forms of the same two kernels)
                with_bool(active != nullptr, [&](auto MASKED) {
                    launch(mortar_step_records_kernel<decltype(PS)::value, decltype(MASKED)::value>, dim3((n_ + sb - 1) / sb), dim3(sb), 0, s, sa, active,
                           (MortarDesc*)final_frames);
                });
            } else if (active) launch(mortar_step_masked_kernel<decltype(PS)::value>, dim3((n_ + sb - 1) / sb), dim3(sb), 0, s, sa, active);
            else launch(mortar_step_kernel<decltype(PS)::value>, dim3((n_ + sb - 1) / sb), dim3(sb), 0, s, sa);
        });
        end_logic(s);
        if (!obs) return;
        if (active) return masked_frames(obs, active, s);
        prof.begin(1, s);
        raster(obs, s);
        prof.end(1, s);
    }

    // mg_step_next in three launches (mg_mortar_next.hpp): the NEXT form of the two-launch step -- mortar_step_next_kernel, the dense raster, the settle launch.
    // The one-launch step (mortar_step_raster_kernel) is left alone.  Lab build, MEMGYM_NEXT_FUSE=0: the composed form of mg_api.hip (mg_step_next), for A/B
    // measurements (tools/next_step_bench.py flips it between calls of one process: read at every call)
    bool step_next(const int32_t* actions, const uint8_t* restart, uint8_t* restart_copy, void* obs, float* reward, uint8_t* done, float* gt,
                   const mg_info_dev* info, hipStream_t s) override {
        if (!lab_flag("MEMGYM_NEXT_FUSE", true)) return false;
        const mg_info_dev ib = begin_step(info);
        check_schedules();  // (what the masked reset of the definition refuses, before anything is stepped)
        sets_.upload(s);
        const MortarStepArgs sa = step_args(actions, reward, done, gt, ib, 0);
        const int sb = step_block(256);
        prof.begin(0, s);
        with_bool(sets_.per_set(), [&](auto PS) {
            launch(mortar_step_next_kernel<decltype(PS)::value>, dim3((n_ + sb - 1) / sb), dim3(sb), 0, s, sa, restart, restart_copy);
        });
        end_logic(s);
        prof.begin(1, s);
        raster(obs, s);
        prof.end(1, s);
        with_bool(sets_.per_set(), [&](auto PS) {
            launch_checked(mortar_next_settle_kernel<decltype(PS)::value>, dim3((n_ + 255) / 256), dim3(256), 0, s, P_, n_, io(), (const uint8_t*)restart_copy);
        });
        return true;
    }

    // mg_advance, mg_play and their traced forms inside ONE launch per ADVANCE_MAX_STEPS steps (mg_mortar_advance.hpp, mg_mortar_play.hpp, mg_mortar_trace.hpp): the
    // chunks of the call (rollout_chunks), the arguments of a chunk (advance_chunk / play_step_args / play_chunk) and its rows of the caller's [steps][...] arrays
    // (row_at: 64-bit offsets) are below, with the private members.  Lab build, MEMGYM_MORTAR_ADVANCE_FUSE=0 / MEMGYM_MORTAR_PLAY_FUSE=0: the loop forms of
    // mg_api_rollout.hpp -- per step an expert launch (advance), the headless (masked) step and an accumulate launch -- for A/B measurements; the traced forms
    // follow the switch of their untraced sibling (tools/headless_bench.py, play_bench.py and rollout_trace_bench.py flip them between calls of one process:
    // read at every call)
    bool advance(const AdvanceArgs& v, hipStream_t s) override {
        if (!lab_flag("MEMGYM_MORTAR_ADVANCE_FUSE", true)) return false;
        require_geometry();
        sets_.upload(s);
        const MortarStepArgs sa = step_args(v.actions, v.reward, v.done, v.gt, v.info, 1);
        rollout_chunks(v.steps, [&](int t0, int k) {
            with_bool(sets_.per_set(), [&](auto PS) {
                launch_checked(mortar_advance_kernel<decltype(PS)::value>, dim3((n_ + 255) / 256), dim3(256), 0, s, sa, advance_chunk(v, t0, k));
            });
        });
        return true;
    }
    bool play(const PlayArgs& v, hipStream_t s) override {
        if (!lab_flag("MEMGYM_MORTAR_PLAY_FUSE", true)) return false;
        require_geometry();
        sets_.upload(s);
        rollout_chunks(v.steps, [&](int t0, int k) {
            with_bool(sets_.per_set(), [&](auto PS) {
                launch_checked(mortar_play_kernel<decltype(PS)::value>, dim3((n_ + 255) / 256), dim3(256), 0, s, play_step_args(v, t0), play_chunk(v, t0, k));
            });
        });
        return true;
    }
    bool advance_traced(const AdvanceArgs& v, const TraceRows& tr, hipStream_t s) override {
        if (!lab_flag("MEMGYM_MORTAR_ADVANCE_FUSE", true)) return false;
        require_geometry();
        sets_.upload(s);
        const MortarStepArgs sa = step_args(v.actions, v.reward, v.done, v.gt, v.info, 1);
        const size_t row = (size_t)n_ * (size_t)action_dim();
        rollout_chunks(v.steps, [&](int t0, int k) {
            const MortarTraceRows rows{row_at((MortarDesc*)tr.frames, t0, n_), row_at(tr.actions, t0, row), row_at(tr.labels, t0, row), row_at(tr.reward, t0, n_),
                                       row_at(tr.done, t0, n_)};
            with_bool(sets_.per_set(), [&](auto PS) {
                launch_checked(mortar_advance_traced_kernel<decltype(PS)::value>, dim3((n_ + 255) / 256), dim3(256), 0, s, sa, advance_chunk(v, t0, k), rows);
            });
        });
        return true;
    }
    bool play_traced(const PlayArgs& v, void* frames, hipStream_t s) override {
        if (!lab_flag("MEMGYM_MORTAR_PLAY_FUSE", true)) return false;
        require_geometry();
        sets_.upload(s);
        rollout_chunks(v.steps, [&](int t0, int k) {
            with_bool(sets_.per_set(), [&](auto PS) {
                launch_checked(mortar_play_traced_kernel<decltype(PS)::value>, dim3((n_ + 255) / 256), dim3(256), 0, s, play_step_args(v, t0), play_chunk(v, t0, k),
                               row_at((MortarDesc*)frames, t0, n_));
            });
        });
        return true;
    }

    std::vector<std::pair<void*, size_t>> state_blobs() override {
        std::vector<std::pair<void*, size_t>> v = {{state_.p, state_.bytes()}, {cmds_.p, cmds_.bytes()}};
        rng_.blobs(v);
        return v;
    }

    // (MortarMayhemB ids: the bound vector observation's row is CARRIED in the record -- it is constant over an episode and written by resets alone, so the
    // row of the saved instance is the row the loaded one shows; handover_, claims_ and tdesc_ are words of one launch)
    std::vector<std::pair<void*, size_t>> instance_rows() override {
        std::vector<std::pair<void*, size_t>> v = {{state_.p, sizeof(MortarState)}, {cmds_.p, (size_t)P_.cmd_cap}, {desc_.p, sizeof(MortarDesc)}};
        rng_.rows(v);
        if (vec_) v.push_back({vec_, sizeof(float) * VEC_DIM});
        return v;
    }

    void expert_actions(const ExpertArgs& x, hipStream_t s) override {
        require_geometry();
        sets_.upload(s);
        launch_checked(mortar_expert_kernel, expert_grid(n_), dim3(EXPERT_BLOCK), 0, s, P_, n_, io(), x);
    }
    void ground_truth64(double* out, hipStream_t s, const uint8_t* only = nullptr) override {
        if (!gt_dim() || !out) return;
        if (only) return launch_checked(mortar_gt64_masked_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, n_, state_.p, out, only);
        launch_checked(mortar_gt64_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, n_, state_.p, out);
    }
    bool debug_counter(const std::string& name, int64_t* out) override {
        if (name == "cmd_list_max" || name == "cmd_list_ge12") {  // the instances' command lists as they stand (a scan of the state records)
            std::vector<MortarState> h(n_);
            MG_HIP(hipDeviceSynchronize());
            MG_HIP(hipMemcpy(h.data(), state_.p, sizeof(MortarState) * (size_t)n_, hipMemcpyDeviceToHost));
            int64_t mx = 0, ge = 0;
            for (const MortarState& s : h) {
                mx = s.num_cmds > mx ? s.num_cmds : mx;
                ge += s.num_cmds >= 12;
            }
            *out = name == "cmd_list_max" ? mx : ge;
            return true;
        }
        if (name == "one_launch_steps") {  // step() calls that went out as mortar_step_raster_kernel since the handle was created (host-side count)
            *out = one_launch_steps_;
            return true;
        }
        if (name != "one_launch_rescues") return false;  // 64-instance slots stepped by a frame wave since the handle was created
        uint32_t v = 0;
        MG_HIP(hipMemcpy(&v, rescues_.p, sizeof v, hipMemcpyDeviceToHost));
        *out = (int64_t)v;
        return true;
    }

    void raster_debug(void* frames, hipStream_t s) override {
        debug_frames<MortarDesc>(
            s, [&](MortarDesc* dbg) { launch(mortar_debug_desc_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, P_, n_, io(), dbg); },
            [&](MortarDesc* dbg) { launch_raster<MortarDebugComposer>(dbg, atlas_->dev(), frames, MG_OBS_U8_XYC, n_, s); });
    }

    void save_debug_records(const int32_t* idx, int count, void* rec, hipStream_t s) override {
        sets_.upload(s);
        launch_checked(mortar_debug_desc_picked_kernel, dim3((count + 255) / 256), dim3(256), 0, s, P_, n_, io(), idx, count, (MortarDesc*)rec);
    }
    void draw_debug_records(const void* records, int n_records, const int32_t* pick, int count, int size, void* rgb, hipStream_t s) override {
        launch_raster_debug_gather<MortarDebugComposer>((const MortarDesc*)records, atlas_->dev(), rgb, size, n_records, pick, count, err_.dev, s);
        check_launch();
    }

   private:
    uint32_t* flag_dev_ = nullptr;  // want_done_flag: non-null only between the request and the end of the step() that follows it
    uint32_t flag_ticket_ = 0;
    bool flag_stored_ = false;      // done_flag_stored
    int64_t one_launch_steps_ = 0;  // debug_counter("one_launch_steps")
    uint32_t ticket_ = 0;  // one-launch step: number of the step, the value a slot's claim word takes when a wave claims it
    uint32_t epoch_ = 0;  // the one-launch step's hand-over epoch, 1 .. 255 (every one-launch step rewrites every word, so the only stale
                          // values a frame workgroup can meet are the previous one-launch step's and the 0 of the fresh array)
    // step() goes out as mortar_step_raster_kernel (instantiated for every observation format: profiles/chw_final.md has each one against the two launches)
    bool one_launch(hipStream_t s) { return fuse_step() && !sets_.per_set() && !stream_capturing(s); }
    static bool fuse_step() {  // lab build: MEMGYM_MORTAR_FUSE=0 selects the two-launch form for A/B measurements
        static const bool on = lab_flag("MEMGYM_MORTAR_FUSE", true);
        return on;
    }
    // head of every reset: the display schedule (commands x (duration + delay) entries) is indexed with 16 bits
    void check_schedules() {
        for (size_t k = 0; k < sets_.size(); ++k) {
            const MortarOpt& O = sets_[k];
            const long long n_max = P_.variant == V_ENDLESS ? O.P.initial_count : O.st_command_count.max(O.P.command_count);
            if (!P_.taskb && n_max * ((long long)O.st_show_dur.max(O.P.show_dur) + O.st_show_delay.max(O.P.show_delay)) > 65535)
                throw OptionError{-3, "command_count x (command_show_duration + command_show_delay) exceeds the 65,535 entries of this build's display schedule"};
        }
    }
    // the arguments of every form of the step kernel: the caller's rows (gt: NULL for the ids without a ground truth) on the handle's arrays
    MortarStepArgs step_args(const int32_t* actions, float* reward, uint8_t* done, float* gt, const mg_info_dev& ib, int autoreset) {
        return MortarStepArgs{P_, n_, io(), actions, reward, done, gt_dim() ? gt : nullptr, ib, autoreset, handover_.p, nullptr};
    }
    // A rollout of `steps` goes out in launches of at most ADVANCE_MAX_STEPS steps: f(t0, k) for the k steps from step t0
    template <class F>
    static void rollout_chunks(int steps, F&& f) {
        for (int t0 = 0; t0 < steps; t0 += ADVANCE_MAX_STEPS) f(t0, steps - t0 < ADVANCE_MAX_STEPS ? steps - t0 : ADVANCE_MAX_STEPS);
    }
    // row t0 of a caller's [steps][width] array, the offset in 64 bits; an array the caller left out stays NULL
    template <class T>
    static T* row_at(T* base, int t0, size_t width) {
        return base ? base + (size_t)t0 * width : nullptr;
    }
    // the chunk from step t0 as the advance / play kernels take it: `first` (the sums start from zero), play's `last` (no alive bytes stored for a next launch)
    static MortarAdvanceArgs advance_chunk(const AdvanceArgs& v, int t0, int k) {
        return MortarAdvanceArgs{k, t0 == 0 ? 1 : 0, v.eps, v.seed, v.step0 + (uint64_t)t0, v.actions, v.out};
    }
    MortarStepArgs play_step_args(const PlayArgs& v, int t0) {
        return step_args(row_at(v.tape, t0, (size_t)n_ * (size_t)action_dim()), v.reward, v.done, v.gt, v.info, v.episode ? 0 : 1);
    }
    MortarPlayArgs play_chunk(const PlayArgs& v, int t0, int k) const {
        return MortarPlayArgs{k, t0 == 0 ? 1 : 0, t0 + k == v.steps ? 1 : 0, v.episode, n_ * action_dim(), v.active, v.alive, row_at(v.reward_trace, t0, n_),
                              row_at(v.done_trace, t0, n_), v.played, v.out};
    }
    MortarIO io() {
        MortarIO o;
        o.state = state_.p;
        o.cmds = cmds_.p;
        o.rng = rng_.view();
        o.desc = desc_.p;
        o.vec = vec_;
        o.err = err_.dev;
        o.sets = sets_.dev();
        o.set_of = sets_.set_of();
        return o;
    }

    // (re)build geometry-dependent constants, atlases and templates
    void rebuild() {
        int radius = 0;
        // (the grid variants accept agent_scale and never read it: GridCharacterController(SCALE, ...), mortar_mayhem_grid.py:249)
        std::vector<Stamp> sprites = build_agent_sprites(P_.variant == V_GRID ? 1.0 * SCALE : agent_scale_, &radius);
        std::vector<Stamp> glyphs = build_glyphs(SCALE);
        P_.tile = (int)(56 * SCALE);
        P_.arena_x0 = SCREEN / 2 - ((P_.tile * P_.N) >> 1);
        P_.radius = radius;
        P_.sprite_dim = sprites[0].w;
        double inv = 1.0 / std::sqrt(2.0);
        P_.v_axis = (1.0 / 1.0) * agent_speed_;
        P_.v_diag = inv * agent_speed_;
        P_.v_axis_i = (int)P_.v_axis;
        P_.v_diag_i = (int)P_.v_diag;
        P_.off_lo = (int)(-8 * SCALE);
        P_.off_hi = (int)(8 * SCALE);

        atlas_.reset(new Atlas());
        for (auto& sp : sprites) atlas_->add_stamp(sp);   // ids 0..7
        for (auto& g : glyphs) atlas_->add_stamp(g);      // ids 8..17
        {   // id 18: the debug view's ring around the target tile (box 2r x 2r, centre (r, r), like the coin)
            const int r = P_.tile / 2;
            Stamp ring_stamp(2 * r, 2 * r);
            circle(ring_stamp, r, r, r, (int)(8 * SCALE), 6);  // palette 6 = (0, 255, 0)
            atlas_->add_stamp(ring_stamp);
        }
        atlas_->set_templates(build_mortar_templates(P_.N, SCALE, SCREEN));
        atlas_->upload();
        P_.glyph_x0 = (int)((SCREEN / 2) - std::floor(88 * SCALE / 2));
        dirty_ = false;
        ++geom_gen_;
        sets_.refresh_geometry();
    }

    // one option set: the parameter block and the lists behind it
    struct MortarOpt {
        MortarParams P;
        OptListStore st_command_count, st_show_dur, st_show_delay, st_expl_dur, st_expl_delay;
        // what the shared atlases and templates fix for every set of the handle
        static void copy_geometry(MortarParams& d, const MortarParams& s) {
            d.variant = s.variant; d.N = s.N; d.taskb = s.taskb; d.cmd_cap = s.cmd_cap; d.arena_x0 = s.arena_x0; d.tile = s.tile;
            d.radius = s.radius; d.sprite_dim = s.sprite_dim; d.glyph_x0 = s.glyph_x0; d.v_axis_i = s.v_axis_i; d.v_diag_i = s.v_diag_i;
            d.off_lo = s.off_lo; d.off_hi = s.off_hi; d.v_axis = s.v_axis; d.v_diag = s.v_diag;
        }
    };

    void raster_only(void* obs, const uint8_t* only, hipStream_t s) override {
        launch_raster<MortarComposer>(desc_.p, atlas_->dev(), obs, obs_format, n_, s, only);
        check_launch();
    }
    std::pair<const void*, size_t> frame_rows() override { return {desc_.p, sizeof(MortarDesc)}; }
    void draw_records(const void* records, int n_records, const int32_t* pick, int count, int fmt, void* obs, hipStream_t s) override {
        launch_raster_gather<MortarComposer, false>((const MortarDesc*)records, atlas_->dev(), obs, fmt, n_records, pick, count, err_.dev, s);
        check_launch();
    }
    void draw_records_padded(const void* records, int n_records, const int32_t* pick, int count, int fmt, void* obs, hipStream_t s) override {
        launch_raster_gather<MortarComposer, true>((const MortarDesc*)records, atlas_->dev(), obs, fmt, n_records, pick, count, err_.dev, s);
        check_launch();
    }
    // (the one-launch step keeps terminal observations itself: the conditions under which step() takes that launch; lab
    // MEMGYM_MORTAR_FINAL_FUSED=0: the generic path of mg_step)
    bool keeps_final_obs(hipStream_t s) override {
        static const bool wanted = lab_flag("MEMGYM_MORTAR_FINAL_FUSED", true);
        return wanted && one_launch(s);
    }

    void raster(void* obs, hipStream_t s) { raster_only(obs, nullptr, s); }

    OptionSets<MortarOpt> sets_;
    MortarParams& P_;  // set 0, the handle-wide set
    std::unique_ptr<Atlas> atlas_;
    double agent_scale_, agent_speed_;
    float* vec_ = nullptr;
    DevArray<MortarState> state_;
    DevArray<uint8_t> cmds_;
    DevArray<MortarDesc> desc_;
    DevArray<uint32_t> claims_, rescues_;  // one-launch step: one claim word per 64 instances; slots stepped by frame waves
    DevArray<uint64_t> handover_, tdesc_;  // one-launch step: the hand-over word per instance (mg_mortar_handover.hpp); tdesc_: the terminal frames' (FINAL form)
};

Family* make_mortar(int variant, int num_envs) { return new MortarFamily(variant, num_envs); }

}  // namespace mg

#ifdef MG_LAB
extern "C" int mg_lab_set_window_offsets(const long long* off, int n) {
    long long v[16] = {0};
    for (int i = 0; i < n && i < 16; ++i) v[i] = off[i];
    return hipMemcpyToSymbol(HIP_SYMBOL(mg::v1::g_lab_win_off), v, sizeof v) == hipSuccess ? 0 : -1;
}
#endif
