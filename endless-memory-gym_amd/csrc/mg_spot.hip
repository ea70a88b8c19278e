// mg_spot.hip -- Searing Spotlights family on gfx950: Endless-SearingSpotlights-v0 and SearingSpotlights-v0.  The family's one translation unit: the host class
// (SpotFamily) and four small kernels are here, the rest of the device code in headers that only this file includes.
//
// Reference behaviour reproduced (bit-exact observations, rewards, dones, RNG consumption):
//   memory_gym/endless_searing_spotlights.py  reset :294-407  step :409-506  _step_spotlight_task :179-231
//                                             _spawn_coin :256-269  _step_coin_task :271-292
//   memory_gym/searing_spotlights.py          reset :332-450  step :452-562  helpers :137-330
//   memory_gym/pygame_assets.py               GridPositionSampler :7-59  Spotlight :61-131  Coin :133-167  Exit :169-220
//   memory_gym/character_controller.py        CharacterController.step :89-146
//
//   mg_spot_types.hpp    constants; SpotParams, SpotCore, SpotDesc and its word view, SpotIO; queue counters and descriptor tags; SpotStepArgs, SpotServeArgs
//   mg_spot_compose.hpp  SpotComposerT (the observation, with or without spotlight borders) and SpotDebugComposerT
//   mg_spot_sampler.hpp  the grid position sampler for the 16 lanes of an instance (sample_cell), nothing of the environments
//   mg_spot_logic.hpp    reset and step of one instance: new_spot, new_spots_at_reset, spot_reset, spot_step_body and the clock build's hooks
//   mg_spot_serve.hpp    spot_reset_kernel, spot_step_kernel and spot_raster_serve_kernel with its launch constants
//   mg_spot_expert.hpp   spot_expert_kernel: the scripted teacher of both ids (mg_expert_actions), a launch of its own
//   mg_spot_next.hpp     spot_step_next_kernel / spot_next_settle_kernel: the NEXT form of the two-launch step (mg_step_next), a flagged instance is reset by its
//                        16 lanes instead of stepped
//
// The launches of a step as shipped (auto-reset, one option set, uint8 observations; why, and the figures: DESIGN.md and fuse_resets() below):
//   two launches   spot_step_kernel: SIXTEEN LANES per instance (4 instances per wave).  Lane s owns spotlight slot s: float64 trajectory (lerp of lerp, un-fused
//                  multiply-add: the library is built with -ffp-contract=off) and hit test; wave ballots collect the 16 done / hit flags of an instance.  The
//                  instance-level logic (agent, coin / exit, RNG, list bookkeeping) is executed redundantly by the 16 lanes -- free under SIMD -- and stored by lane 0;
//                  the grid sampler splits its 84 rows over them (sample_cell); an instance that finishes is reset by its own lanes.  Kernels are templated on
//                  ENDLESS.  Slot arrays are [N][16] so the 16 lanes of an instance read one contiguous 128-byte row per field; the Python list semantics
//                  (append / remove-while-iterating) live in a 16-nibble order word.
//                  -> raster_kernel<SpotComposer> (generation 2, mg_raster.hpp; SpotBorderComposer once black_background has been on): hole mask -> chessboard
//                  template, coin(s) / exit, agent, each darkened outside the holes while written -> coin(s) shown above the dark layer -> top bar.
//   step + fused raster / reset service
//                  spot_step_kernel with defer = 1: an instance that finishes is queued and its descriptor tagged DESC_QUEUED -> spot_raster_serve_kernel: the first
//                  SPOT_SVC_WGS workgroups take the queue entries, reset those instances and draw their frames, all others draw the frames that were not queued.
//   Which one: fuse_resets().  Endless-SearingSpotlights-v0: two launches up to RASTER_PLAIN_MAX = 16,384 instances, fused beyond; SearingSpotlights-v0: fused up to
//   FUSE_MAX = 65,536 instances, two launches beyond; MG_OBS_U8_CYX like the uint8 frame, the float formats fused up to FUSE_MAX on both ids (fuse_resets()).
//   Per-instance option sets, autoreset = 0 and the image-order formats on a stream that is being captured: always two launches.
//   Terminal observations kept (mg_info_buffers.final_obs_dev, keeps_final_obs()): always the fused pair, in its <FINAL> form -- the service workgroup draws the terminal
//   frame from the descriptor the step left, then resets.  Every observation format: spot_raster_serve_kernel<EN, BORDER, NT, FINAL, FMT>.
#include <memory>

#include "mg_atlas.hpp"
#include "mg_lab.hpp"
#include "mg_option_sets.hpp"
#include "mg_spot_types.hpp"
#include "mg_spot_compose.hpp"
#include "mg_raster_gather.hpp"
#include "mg_spot_sampler.hpp"
#include "mg_spot_logic.hpp"
#include "mg_spot_serve.hpp"
#include "mg_spot_expert.hpp"
#include "mg_spot_next.hpp"

namespace mg {

// info["ground_truth"] in float64: agent and coin position / screen size (endless_searing_spotlights.py:407,496)
__global__ __launch_bounds__(256) void spot_gt64_kernel(SpotParams P0, SpotIO io, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n) return;
    const SpotParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    const SpotCore s = io.core[i];
    write_gt(out + 4 * i, P, s.ax, s.ay, s);
}

__global__ __launch_bounds__(256) void spot_gt64_masked_kernel(SpotParams P0, SpotIO io, double* out, const uint8_t* __restrict__ only) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n || !only[i]) return;
    const SpotParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    const SpotCore s = io.core[i];
    write_gt(out + 4 * i, P, s.ax, s.ay, s);
}

__global__ __launch_bounds__(256) void spot_init_kernel(int n, SpotCore* core) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SpotCore s;
    memset(&s, 0, sizeof(s));
    core[i] = s;
}

#ifdef MG_LAB
// Measurement (lab build, MEMGYM_SPOT_WARM=1; profiles/r06_spot.md): a launch behind the raster that reads exactly what the NEXT step
// kernel's lanes will read first -- core record, generator stream, slot record -- with the same block -> instance mapping, so that the
// step finds its state in its XCD's L2.  Only the step kernel's time is of interest (would a warm state be worth building into the
// raster launch's tail?); this launch's own cost is not hidden.
__global__ __launch_bounds__(256) void spot_warm_kernel(int n, SpotIO io) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = gid >> 4, ls = gid & 15;
    if (i >= n) return;
    const size_t k = (size_t)i * SLOTS + ls;
    const uint32_t* c = reinterpret_cast<const uint32_t*>(&io.core[i]);
    uint64_t acc = c[ls] ^ c[(ls + 16) % 20];
    acc ^= io.rng.s_hi[i] ^ io.rng.s_lo[i] ^ io.rng.inc_hi[i] ^ io.rng.inc_lo[i] ^ io.rng.buf[i];
    acc ^= (uint64_t)io.sp_ang[k] ^ (uint64_t)io.sp_r[k] ^ (uint64_t)__double_as_longlong(io.sp_t[k]) ^ (uint64_t)__double_as_longlong(io.sp_speed[k]);
    if (acc == 0x1234567812345678ull) io.err[0] |= 0;  // (never: keeps the loads alive)
}
#endif

// Debug view: the current descriptors with the agent the reference's debug render shows -- the stored (sprite, rect) pair of
// the last STEP (stale right after a reset; oracle/mgo_spot.c sp_debug), sprite 0 at the agent's rect before any step.
__global__ __launch_bounds__(256) void spot_debug_desc_kernel(SpotParams P0, SpotIO io, SpotDesc* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n) return;
    const SpotParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    SpotDesc d = io.desc[i];
    const SpotCore s = io.core[i];
    d.valid = 1;
    if (s.pad >> 31) {
        d.sprite = (s.pad >> 16) & 7u;
        d.sx = (int16_t)((int)(s.pad & 0xFFu) - 128 - P.sprite_half);
        d.sy = (int16_t)((int)((s.pad >> 8) & 0xFFu) - 128 - P.sprite_half);
    }
    out[i] = d;
}

// The same descriptor for ONE instance, for the picked form below (a body of its own: spot_debug_desc_kernel stays the code it was).
__device__ __forceinline__ SpotDesc spot_debug_desc_one(const SpotParams& P, const SpotIO& io, int i) {
    SpotDesc d = io.desc[i];
    const SpotCore s = io.core[i];
    d.valid = 1;
    if (s.pad >> 31) {
        d.sprite = (s.pad >> 16) & 7u;
        d.sx = (int16_t)((int)(s.pad & 0xFFu) - 128 - P.sprite_half);
        d.sy = (int16_t)((int)((s.pad >> 8) & 0xFFu) - 128 - P.sprite_half);
    }
    return d;
}
// mg_save_debug_frames: record j <- the debug descriptor of instance idx[j] (idx == NULL: instance j), one lane per entry.  An entry < 0 is skipped, one
// >= n is skipped and flagged; a skipped entry's record is not written.
__global__ __launch_bounds__(256) void spot_debug_desc_picked_kernel(SpotParams P0, SpotIO io, const int32_t* __restrict__ idx, int count, SpotDesc* rec) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const int i = idx ? idx[j] : j;
    if (i < 0) return;
    if (i >= P0.n) return raise_error(io.err, ERR_FRAME_INDEX);
    const SpotParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    rec[j] = spot_debug_desc_one(P, io, i);
}

// ---------------------------------------------------------------------------------------------------------
static const double SCALE = 0.25;

// sin / cos by two separate libm calls (a merged sincos() differs by 1 ulp for a few integer-degree angles)
static __attribute__((noinline)) double sin_only(double x) { volatile double v = x; return std::sin(v); }
static __attribute__((noinline)) double cos_only(double x) { volatile double v = x; return std::cos(v); }

class SpotFamily : public Family {
   public:
    SpotFamily(int endless, int n) : Family(n), P_(sets_[0].P) {
        memset(&P_, 0, sizeof(P_));
        P_.endless = endless;
        P_.n = n;
        P_.speed_lo = 0.0025; P_.speed_hi = 0.0075; P_.damage = 1.0;
        P_.visual_feedback = 1; P_.light_threshold = 255;
        coin_scale_ = 1.5 * SCALE; agent_speed_ = 12.0 * SCALE; agent_scale_ = 1.0 * SCALE; exit_scale_ = 2.0 * SCALE;
        P_.sample_agent_position = 1; P_.show_last_action = 1; P_.show_last_positive_reward = 1;
        P_.r_coin = 0.25;
        if (endless) {
            P_.max_steps = -1; P_.steps_per_coin = 160; P_.initial_spawns = 3; P_.spawn_interval = 50;
            P_.coin_enabled = 1; P_.coin_show_duration = 6; P_.agent_health = 10;
        } else {
            P_.max_steps = 256; P_.initial_spawns = 4; P_.num_spawns = 30;
            initial_spawn_interval_ = 30; spawn_interval_threshold_ = 10;
            sets_[0].st_num_coins.set(P_.num_coins, {1}); P_.agent_health = 5; P_.r_exit = 1.0; P_.use_exit = 1;
        }
        core_.alloc(n);
        for (auto* a : {&sp_t_, &sp_speed_}) a->alloc((size_t)SLOTS * n);
        sp_ang_.alloc((size_t)SLOTS * n);
        sp_r_.alloc((size_t)SLOTS * n);
        flags_.alloc(4);
        exit_hist_.alloc(1 + EXIT_GENS);
        queue_.alloc((size_t)n + SQ_WORDS);

        coins_.alloc((size_t)MAX_COINS * n);
        desc_.alloc(n);
        rng_.alloc(n);
        err_.alloc();
        std::vector<double> ct(360), st(360);
        for (int a = 0; a < 360; ++a) {
            if (a % 90 == 0) {
                static const double C4[4] = {1, 0, -1, 0}, S4[4] = {0, 1, 0, -1};
                ct[a] = C4[a / 90];
                st[a] = S4[a / 90];
            } else {
                double rad = (double)a * M_PI / 180.0;
                ct[a] = cos_only(rad);
                st[a] = sin_only(rad);
            }
        }
        cos_.upload(ct);
        {   // s_k = A^k s_0 + S_k inc for k = 1 .. 16 (PCG64's 128-bit LCG, multiplier as in mg_device.hpp Pcg::advance)
            const u128 A = (((u128)0x2360ED051FC65DA4ull) << 64) | (u128)0x4385DF649FCCF645ull;
            std::vector<uint4> jt(32);
            u128 m = 1, q = 0;
            for (int k = 0; k < 16; ++k) {
                q = q * A + 1;  // S_(k+1) = S_k A + 1
                m = m * A;      // A^(k+1)
                jt[2 * k] = make_uint4((uint32_t)m, (uint32_t)(m >> 32), (uint32_t)(m >> 64), (uint32_t)(m >> 96));
                jt[2 * k + 1] = make_uint4((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)(q >> 64), (uint32_t)(q >> 96));
            }
            jump_.upload(jt);
        }
        sin_.upload(st);
        sets_.alloc();
        launch(spot_init_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, core_.p);
        MG_HIP(hipDeviceSynchronize());
        rebuild();
        sets_.defaults = P_;
    }

    int action_dim() const override { return 2; }
    int gt_dim() const override { return P_.endless ? 4 : 0; }
    const char* info_name(int k) const override {
        if (k == 0) return "agent_health";
        if (k == 1) return "coins_collected";
        if (k == 2 && !P_.endless) return "success";
        return nullptr;
    }

    // One key of the reset options, for option set `set` (0 = the handle-wide set of mg_set_option).  Sets > 0 hold everything
    // that does not change the geometry (atlases, tables and derived constants are shared by the handle's instances); a geometry
    // option is accepted there when it says what the handle's geometry already is.
    void set_option(const std::string& key, const double* v, int n) override { set_option_set(0, key, v, n); }
    void set_option_set(int set, const std::string& key, const double* v, int n) override {
        SpotOpt& O = sets_.ensure(set, derive);
        SpotParams& P = O.P;
        const bool e = P_.endless;
        const OptionArg A{set, key, v, n, dirty_};
        if (key == "max_steps") P.max_steps = A.integer();
        else if (key == "initial_spawns") { P.initial_spawns = A.integer(); A.must_be(P.initial_spawns >= 0 && P.initial_spawns <= SLOTS); }
        else if (key == "spot_min_radius") { O.min_radius = v[0]; derive(O); }
        else if (key == "spot_max_radius") { O.max_radius = v[0]; derive(O); }
        else if (key == "spot_min_speed") P.speed_lo = v[0];
        else if (key == "spot_max_speed") P.speed_hi = v[0];
        else if (key == "spot_damage") P.damage = v[0];
        else if (key == "visual_feedback") P.visual_feedback = A.flag();
        else if (key == "black_background") {
            P.black_background = A.flag();
            if (P.black_background && !P_.ordered_holes) {  // from now on spotlights may carry a border (sticky, kept in the state)
                P_.ordered_holes = 1;
                ++frame_gen_;  // (the border composer draws from now on: mg_frame_layout)
                const int one = 1;
                MG_HIP(hipMemcpy(flags_.p, &one, sizeof(int), hipMemcpyHostToDevice));
            }
        }
        else if (key == "hide_chessboard") P.hide_chessboard = A.flag();
        else if (key == "light_dim_off_duration") { O.dim_duration = A.integer(); derive(O); }
        else if (key == "light_threshold") P.light_threshold = A.integer();
        else if (key == "coin_scale") A.geometry(coin_scale_, v[0]);
        else if (key == "coins_visible") P.coins_visible = A.flag();
        else if (key == "agent_speed") A.geometry(agent_speed_, v[0]);
        else if (key == "agent_health") P.agent_health = v[0];
        else if (key == "agent_scale") A.geometry(agent_scale_, v[0]);
        else if (key == "agent_visible") P.layer_flags = (P.layer_flags & ~LAYER_AGENT_TOP) | (v[0] != 0.0 ? LAYER_AGENT_TOP : 0);
        else if (key == "sample_agent_position") P.sample_agent_position = A.flag();
        else if (key == "show_last_action") {
            // (the last-reward bar's position and width depend on it, searing_spotlights.py:385-390: geometry)
            A.geometry(P_.show_last_action, A.flag() ? 1 : 0);
            // False crashes the ENDLESS reference at its first step (endless_searing_spotlights.py:422 reads action_colors,
            // which :343 only creates when the flag is set); the finite env guards the use (searing_spotlights.py:465)
            if (e) A.must_be(v[0] != 0.0);
        }
        else if (key == "show_last_positive_reward") P.show_last_positive_reward = A.flag();
        else if (key == "reward_inside_spotlight") P.r_inside = v[0];
        else if (key == "reward_outside_spotlight") P.r_outside = v[0];
        else if (key == "reward_death") P.r_death = v[0];
        else if (key == "reward_coin") P.r_coin = v[0];
        else if (e && key == "steps_per_coin") P.steps_per_coin = A.integer();
        else if (e && key == "spawn_interval") P.spawn_interval = A.integer();
        else if (e && key == "coin_enabled") P.coin_enabled = A.flag();
        else if (e && key == "coin_show_duration") P.coin_show_duration = A.integer();
        else if (!e && key == "num_spawns") { P.num_spawns = A.integer(); A.must_be(P.num_spawns >= 0 && P.num_spawns <= 255); }
        else if (!e && key == "initial_spawn_interval") A.geometry(initial_spawn_interval_, v[0]);
        else if (!e && key == "spawn_interval_threshold") A.geometry(spawn_interval_threshold_, v[0]);
        else if (!e && key == "spawn_interval_decay") { /* only intervals[0] is ever read (pop() takes the last) */ }
        else if (!e && key == "num_coins") {
            // any length (searing_spotlights.py:408); the empty list is refused by mg_set_option: the reference ends every such
            // episode with a ZeroDivisionError (searing_spotlights.py:553)
            std::vector<int> vals(n);
            for (int k = 0; k < n; ++k) {
                vals[k] = A.integer(k);
                A.must_be(vals[k] >= 1 && vals[k] <= MAX_COINS);
            }
            O.st_num_coins.set(P.num_coins, vals);
        }
        // False: legal once the instance has had an exit (its stale one is drawn, spot_reset); before that the reference raises
        // AttributeError and the reset raises error bit 256
        else if (!e && key == "use_exit") P.use_exit = A.flag();
        else if (!e && key == "exit_scale") A.geometry(exit_scale_, v[0]);
        else if (!e && key == "exit_visible") P.layer_flags = (P.layer_flags & ~LAYER_EXIT_ABOVE) | (v[0] != 0.0 ? LAYER_EXIT_ABOVE : 0);
        else if (!e && key == "reward_exit") P.r_exit = v[0];
        else if (!e && key == "reward_max_steps") {}
        else throw OptionError{-2, "unknown reset parameter " + key};
    }
    void bind_option_sets(const int32_t* set_of_dev) override { sets_.bind(set_of_dev); }

    void reset(const int64_t* seeds, const uint8_t* mask, void* obs, float* gt, hipStream_t s) override {
        if (dirty_) rebuild();
        require_seeded(seeds);
        check_slots();
        if (seeds) seeded_ = true;
        sets_.upload(s);
        const dim3 rg((n_ * SLOTS + 255) / 256);
        with_bool(P_.endless, [&](auto EN) {
            with_bool(sets_.per_set(), [&](auto PS) {
                launch(spot_reset_kernel<decltype(EN)::value, decltype(PS)::value>, rg, dim3(256), 0, s, P_, io(), seeds, mask, gt);
            });
        });
        reset_frames(mask, [&](const uint8_t* m) {
            with_bool(P_.ordered_holes, [&](auto BO) { launch_raster_sparse<SpotComposerT<decltype(BO)::value>>(desc_.p, atlas_->dev(), obs, obs_format, n_, s, m); });
        }, [&] { raster(obs, s); });
    }

    void step(const int32_t* actions, const uint8_t* active, void* obs, float* reward, uint8_t* done, float* gt, const mg_info_dev* info,
              int autoreset, hipStream_t s, void* final_frames) override {
        const mg_info_dev ib = begin_step(info);
        sets_.upload(s);
        prof.begin(0, s);
        // (resets served inside the raster launch: handles with ONE option set -- the service code takes its parameters from the launch's arguments)
        // (a call that keeps terminal observations: always deferred -- the service workgroup draws the terminal frame from the descriptor this
        // launch leaves, then resets: keeps_final_obs)
        const bool keep_final = autoreset && ib.final_obs_dev && keeps_final_obs(s);
        // (a headless step, obs == NULL: never deferred -- there is no raster launch to serve the resets; nor is a masked step, active != NULL: the
        // MASKED form of the step kernel, then the active instances' frames)
        const int defer = (obs && !active && autoreset && (fuse_resets() || keep_final) && !sets_.per_set() && fused_here(s)) ? 1 : 0;
        const int sb = step_block(256);
        const SpotStepArgs sa{P_, io(), actions, reward, done, gt, ib, autoreset, defer};
        const dim3 sg((n_ * SLOTS + sb - 1) / sb);
        with_bool(P_.endless, [&](auto EN) {
            with_bool(sets_.per_set(), [&](auto PS) {
                if (final_frames) {  // (terminal frame records, obs == NULL: the RECORDS forms of the same two kernels; never deferred)
                    with_bool(active != nullptr, [&](auto MASKED) {
                        launch(spot_step_records_kernel<decltype(EN)::value, decltype(PS)::value, decltype(MASKED)::value>, sg, dim3(sb), 0, s, sa, active,
                               (SpotDesc*)final_frames);
                    });
                } else if (active) launch(spot_step_masked_kernel<decltype(EN)::value, decltype(PS)::value>, sg, dim3(sb), 0, s, sa, active);
                else launch(spot_step_kernel<decltype(EN)::value, decltype(PS)::value>, sg, dim3(sb), 0, s, sa);
            });
        });
        end_logic(s);
        if (active) {
            if (obs) masked_frames(obs, active, s);
            return;
        }
        prof.begin(1, s);
        if (defer) {
            const int grid = frames_grid(n_) + SPOT_SVC_WGS;
            const int forced_batch = lab_int("MEMGYM_SPOT_SVC_BATCH", 0);  // (lab build: exactly this many)
            const bool fb = forced_batch >= 1 && forced_batch <= SPOT_SVC_BATCH;
            const SpotServeArgs va{desc_.p, atlas_->dev(), obs, n_, P_, io(), gt, fb ? forced_batch : (n_ <= 12288 ? 1 : SPOT_SVC_BATCH), fb ? forced_batch : SPOT_SVC_BATCH,
                                   keep_final ? ib.final_obs_dev : nullptr};
            const bool nt = fused_nt();                // non-temporal: with plain stores the fused launch loses 5-15 us at every occupancy
            const int serve_lds = RASTER_LDS_REQUEST;  // 25 KiB: six per CU
            // (endless x border x non-temporal x kept terminal observations: all sixteen forms are launched in each of the two one-byte formats;
            // the float formats' stream-out has no non-temporal flavour -- eight forms each, NT = false)
            with_bool(P_.endless, [&](auto EN) {
                with_bool(P_.ordered_holes, [&](auto BO) {
                    with_bool(keep_final, [&](auto FINAL) {
                        with_obs_format(obs_format, [&](auto F) {
                            constexpr int FMT = decltype(F)::value;
                            constexpr bool ONE_BYTE = FMT == MG_OBS_U8_XYC || FMT == MG_OBS_U8_CYX;
                            with_bool(ONE_BYTE && nt, [&](auto NT) {
                                if constexpr (ONE_BYTE || !decltype(NT)::value)
                                    launch_checked(spot_raster_serve_kernel<decltype(EN)::value, decltype(BO)::value, decltype(NT)::value, decltype(FINAL)::value, FMT>,
                                                   dim3(grid), dim3(256), serve_lds, s, va);
                            });
                        });
                    });
                });
            });
            ++spot_fused_steps_;
        } else if (obs) {
            raster(obs, s);
        }
        prof.end(1, s);
#ifdef MG_LAB
        if (lab_flag("MEMGYM_SPOT_WARM", false)) launch(spot_warm_kernel, sg, dim3(sb), 0, s, n_, io());
#endif
    }

    // mg_step_next in three launches (mg_spot_next.hpp): the NEXT form of the two-launch step -- spot_step_next_kernel, the dense raster, the settle launch.
    // The fused serve launch (spot_raster_serve_kernel) is left alone: without auto-reset nothing is deferred.  Lab build, MEMGYM_NEXT_FUSE=0: the composed
    // form of mg_api.hip, for A/B measurements (tools/next_step_bench.py flips it between calls of one process: read at every call)
    bool step_next(const int32_t* actions, const uint8_t* restart, uint8_t* restart_copy, void* obs, float* reward, uint8_t* done, float* gt,
                   const mg_info_dev* info, hipStream_t s) override {
        if (!lab_flag("MEMGYM_NEXT_FUSE", true)) return false;
        const mg_info_dev ib = begin_step(info);
        check_slots();  // (what the masked reset of the definition refuses, before anything is stepped)
        sets_.upload(s);
        prof.begin(0, s);
        const int sb = step_block(256);
        const SpotStepArgs sa{P_, io(), actions, reward, done, gt, ib, 0, 0};
        const dim3 sg((n_ * SLOTS + sb - 1) / sb);
        with_bool(P_.endless, [&](auto EN) {
            with_bool(sets_.per_set(), [&](auto PS) {
                launch(spot_step_next_kernel<decltype(EN)::value, decltype(PS)::value>, sg, dim3(sb), 0, s, sa, restart, restart_copy);
            });
        });
        end_logic(s);
        prof.begin(1, s);
        raster(obs, s);
        prof.end(1, s);
        launch_checked(spot_next_settle_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, n_, io(), (const uint8_t*)restart_copy);
        return true;
    }

    std::vector<std::pair<void*, size_t>> state_blobs() override {
        std::vector<std::pair<void*, size_t>> v = {{core_.p, core_.bytes()}, {coins_.p, coins_.bytes()}, {sp_r_.p, sp_r_.bytes()},
                                                  {sp_ang_.p, sp_ang_.bytes()}};
        for (auto* a : {&sp_t_, &sp_speed_}) v.push_back({a->p, a->bytes()});
        v.push_back({flags_.p, flags_.bytes()});
        v.push_back({exit_hist_.p, exit_hist_.bytes()});
        // (the frame descriptors: what mg_render, mg_render_debug and a reset's stale holes read BEFORE the restored handle's first step)
        v.push_back({desc_.p, desc_.bytes()});
        rng_.blobs(v);
        return v;
    }
    // (flags_ and exit_hist_ are the handle's: ordered_holes only ever goes from 0 to 1, for every instance alive; the exit generations change with a rebuild
    // alone, which changes mg_instance_layout; queue_ is a launch's)
    std::vector<std::pair<void*, size_t>> instance_rows() override {
        std::vector<std::pair<void*, size_t>> v = {{core_.p, sizeof(SpotCore)}, {coins_.p, sizeof(uint32_t) * MAX_COINS}, {sp_r_.p, sizeof(uint8_t) * SLOTS},
                                                  {sp_ang_.p, sizeof(uint32_t) * SLOTS}, {sp_t_.p, sizeof(double) * SLOTS}, {sp_speed_.p, sizeof(double) * SLOTS},
                                                  {desc_.p, sizeof(SpotDesc)}};
        rng_.rows(v);
        return v;
    }
    void expert_actions(const ExpertArgs& x, hipStream_t s) override {
        require_geometry();
        sets_.upload(s);
        launch_checked(spot_expert_kernel, expert_grid(n_), dim3(EXPERT_BLOCK), 0, s, P_, io(), x);
    }
    void ground_truth64(double* out, hipStream_t s, const uint8_t* only = nullptr) override {
        if (!gt_dim() || !out) return;
        sets_.upload(s);
        if (only) return launch_checked(spot_gt64_masked_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, P_, io(), out, only);
        launch_checked(spot_gt64_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, P_, io(), out);
    }

    void on_state_loaded() override {
        seeded_ = true;
        int f = 0;
        MG_HIP(hipMemcpy(&f, flags_.p, sizeof(int), hipMemcpyDeviceToHost));
        if (f && !P_.ordered_holes) ++frame_gen_;  // (as in set_option_set: the border composer draws from now on)
        if (f) P_.ordered_holes = 1;
        if (!P_.endless) {  // the exit generations the restored instances refer to; the atlas follows
            std::vector<double> hist(1 + EXIT_GENS, 0.0);
            MG_HIP(hipMemcpy(hist.data(), exit_hist_.p, sizeof(double) * hist.size(), hipMemcpyDeviceToHost));
            for (int g = 0; g < EXIT_GENS; ++g) {
                exit_gen_used_[g] = hist[1 + g] != 0.0;
                exit_gen_scale_[g] = hist[1 + g];
            }
            rebuild();
        }
        sets_.touch();
    }
    void raster_debug(void* frames, hipStream_t s) override;
    bool debug_counter(const std::string& name, int64_t* out) override {
        if (name != "spot_fused_steps") return false;  // step() calls that went out as spot_raster_serve_kernel since the handle was created (host-side count)
        *out = spot_fused_steps_;
        return true;
    }

   private:
    int64_t spot_fused_steps_ = 0;  // debug_counter("spot_fused_steps")
    // head of every reset: 16 spotlight slots per instance.  Refuse option sets that overflow them in ANY episode that lasts as long
    // as the fastest spotlight lives (t reaches 1 after ceil(1 / speed) steps, the slot is freed one step later);
    // rarer overflows raise error bit 1, which mg_peek_errors shows without a synchronisation.
    void check_slots() {
        for (size_t k = 0; k < sets_.size(); ++k) {
            const SpotParams& Q = sets_[k].P;
            if (Q.r_hi <= Q.r_lo) throw OptionError{-3, "spot radius range not supported"};
            const int life_min = (int)std::ceil(1.0 / Q.speed_hi) + 1;
            const int interval = P_.endless ? Q.spawn_interval : P_.interval0;
            int later = interval > 0 ? (life_min - 1) / interval : 1 << 20;
            if (!P_.endless && later > Q.num_spawns) later = Q.num_spawns;
            if (Q.initial_spawns + later > SLOTS)
                throw std::runtime_error("these options keep " + std::to_string(Q.initial_spawns + later) +
                                         " spotlights alive at once; this build holds " + std::to_string(SLOTS) +
                                         " per instance (raise spawn_interval / spot_max_speed or lower initial_spawns)");
        }
    }
    SpotIO io() {
        SpotIO o;
        o.core = core_.p;
        o.sp_t = sp_t_.p; o.sp_speed = sp_speed_.p; o.sp_ang = sp_ang_.p; o.sp_r = sp_r_.p;
        o.coins = coins_.p;
        o.rng = rng_.view();
        o.desc = desc_.p;
        o.err = err_.dev;
        o.queue = queue_.p + SQ_WORDS;
        o.qctr = queue_.p;
        o.sets = sets_.dev();
        o.set_of = sets_.set_of();
        return o;
    }

    void rebuild() {
        int radius = 0;
        std::vector<Stamp> sprites = build_agent_sprites(agent_scale_, &radius);
        P_.agent_radius = radius;
        {
            const int full = sprites[0].w;  // blit position of the un-cropped surface: centre - full / 2
            P_.sprite_half = full / 2 - crop_common_margin(sprites);
        }
        double inv = 1.0 / std::sqrt(2.0);
        P_.v_axis_i = (int)((1.0 / 1.0) * agent_speed_);
        P_.v_diag_i = (int)(inv * agent_speed_);
        for (size_t k = 0; k < sets_.size(); ++k) {
            derive(sets_[k]);
            if (sets_[k].P.r_hi <= sets_[k].P.r_lo) throw OptionError{-3, "spot radius range not supported"};
        }
        P_.coin_radius = (int)(10 * coin_scale_);
        P_.spawn_clamp = (int)(30 * SCALE);
        P_.quarter = (int)(SCREEN / 4);
        P_.bar_h = (int)(16 * SCALE);
        if (P_.show_last_action) { P_.bar_x = (int)(P_.quarter * 2.75); P_.bar_w = (int)(P_.quarter * 0.5); }
        else { P_.bar_x = P_.quarter * 2; P_.bar_w = P_.quarter * 2; }
        P_.half_diag = std::sqrt(std::pow((double)SCREEN, 2) + std::pow((double)SCREEN, 2)) / 2;
        P_.exit_radius = 20.0 / 2 * exit_scale_;
        P_.interval0 = (int)(initial_spawn_interval_ + spawn_interval_threshold_);
        P_.cos_tab = cos_.p;
        P_.sin_tab = sin_.p;
        P_.jump = jump_.p;
        P_.lab_fallback = lab_int("MEMGYM_SPOT_RESET_FALLBACK", 0);

        atlas_.reset(new Atlas());
        // (any size: SpotComposer::Pre holds the first 256 padded pixels of a layer's stamp in registers -- every default stamp in
        // full -- and stamp_apply_lit reads what a *_scale option adds beyond that from the atlas while it composes)
        for (auto& sp : sprites) atlas_->add_stamp(sp);  // 0..7
        atlas_->add_stamp(build_coin(coin_scale_));       // 8
        if (!P_.endless) {  // 9 + 2 g, 10 + 2 g: the exits of generation g (free generations: an empty stamp)
            pick_exit_generation();
            P_.exit_halves = 0;
            for (int g = 0; g < EXIT_GENS; ++g) {
                if (exit_gen_used_[g]) {
                    const int half = (int)(20 * exit_gen_scale_[g]) >> 1;
                    if (half > 255) throw OptionError{-3, "exit_scale beyond 25: the exit would be six screens wide"};
                    P_.exit_halves |= (uint64_t)half << (8 * g);
                    atlas_->add_stamp(build_exit(exit_gen_scale_[g], false));
                    atlas_->add_stamp(build_exit(exit_gen_scale_[g], true));
                } else {
                    atlas_->add_stamp(Stamp(1, 1));
                    atlas_->add_stamp(Stamp(1, 1));
                }
            }
            std::vector<double> hist(1 + EXIT_GENS, 0.0);
            for (int g = 0; g < EXIT_GENS; ++g) hist[1 + g] = exit_gen_used_[g] ? exit_gen_scale_[g] : 0.0;
            hist[0] = (double)P_.exit_gen;
            MG_HIP(hipMemcpy(exit_hist_.p, hist.data(), sizeof(double) * hist.size(), hipMemcpyHostToDevice));
        }
        atlas_->set_templates(build_chessboards(SCALE, SCREEN));
        atlas_->upload();
        dirty_ = false;
        ++geom_gen_;
        sets_.refresh_geometry();
        {   // (the defaults' own radius / dim values, whatever set 0 holds by now)
            SpotOpt D;
            D.P = sets_.defaults;
            derive(D);
            sets_.defaults = D.P;
        }
    }

    // The generation new exits belong to = the slot that holds exit_scale_; a new scale takes a free slot.  Slots are only ever
    // freed here, when all eight are taken: the instances' pads are read back and the generations no exit refers to any more
    // are released (rare: eight different exit sizes in the life of one handle).
    void pick_exit_generation() {
        for (int g = 0; g < EXIT_GENS; ++g)
            if (exit_gen_used_[g] && exit_gen_scale_[g] == exit_scale_) { P_.exit_gen = g; return; }
        auto take_free = [&]() {
            for (int g = 0; g < EXIT_GENS; ++g)
                if (!exit_gen_used_[g]) {
                    exit_gen_used_[g] = true;
                    exit_gen_scale_[g] = exit_scale_;
                    P_.exit_gen = g;
                    return true;
                }
            return false;
        };
        if (take_free()) return;
        MG_HIP(hipDeviceSynchronize());
        std::vector<uint32_t> pads(n_);
        MG_HIP(hipMemcpy2D(pads.data(), sizeof(uint32_t), reinterpret_cast<const char*>(core_.p) + offsetof(SpotCore, pad), sizeof(SpotCore),
                           sizeof(uint32_t), n_, hipMemcpyDeviceToHost));
        bool alive[EXIT_GENS] = {false, false, false, false, false, false, false, false};
        for (uint32_t pad : pads)
            if (pad & PAD_HAS_EXIT) alive[(pad & PAD_EXIT_GEN_MASK) >> PAD_EXIT_GEN_SHIFT] = true;
        for (int g = 0; g < EXIT_GENS; ++g) exit_gen_used_[g] = alive[g];
        if (!take_free())
            throw OptionError{-3, "exits of eight different exit_scale values are still on screen (use_exit = False keeps them); a ninth size needs a reset with use_exit = True first"};
    }

    // one option set: the parameter block, the list and the raw values behind it
    struct SpotOpt {
        SpotParams P;
        OptListStore st_num_coins;
        double min_radius = 30.0 * 0.25, max_radius = 55.0 * 0.25;  // spot_min_radius / spot_max_radius (defaults x SCALE)
        int dim_duration = 6;                                      // light_dim_off_duration
        // what the shared atlases, tables and derived constants fix for every set of the handle
        static void copy_geometry(SpotParams& d, const SpotParams& s) {
            d.endless = s.endless; d.n = s.n; d.ordered_holes = s.ordered_holes;
            d.show_last_action = s.show_last_action; d.agent_radius = s.agent_radius; d.sprite_half = s.sprite_half;
            d.coin_radius = s.coin_radius; d.v_axis_i = s.v_axis_i; d.v_diag_i = s.v_diag_i; d.spawn_clamp = s.spawn_clamp; d.bar_x = s.bar_x;
            d.bar_w = s.bar_w; d.quarter = s.quarter; d.bar_h = s.bar_h; d.exit_gen = s.exit_gen; d.exit_halves = s.exit_halves; d.half_diag = s.half_diag;
            d.exit_radius = s.exit_radius; d.interval0 = s.interval0; d.cos_tab = s.cos_tab; d.sin_tab = s.sin_tab; d.jump = s.jump; d.lab_fallback = s.lab_fallback;
        }
    };
    // what a set's radius and dim options mean for the kernels (pure logic: the disc span table covers every radius up to DISC_RMAX)
    static void derive(SpotOpt& O) {
        const int r_lo = (int)O.min_radius, r_hi = (int)(O.max_radius + 1);
        // (both bounds travel through set_option one at a time: only a pair that is complete nonsense is refused here, the range
        // as a whole again by rebuild() / the reset that uses it)
        if (r_hi - 1 > DISC_RMAX || r_lo < 1) throw OptionError{-3, "spot radius range not supported"};
        O.P.r_lo = r_lo;
        O.P.r_hi = r_hi;
        O.P.dim_duration = O.dim_duration;
        O.P.dim_step = O.dim_duration > 0 ? (int)(255.0 / O.dim_duration) : 0;
    }

    void raster_only(void* obs, const uint8_t* only, hipStream_t s) override {
        with_bool(P_.ordered_holes, [&](auto BO) { launch_raster<SpotComposerT<decltype(BO)::value>>(desc_.p, atlas_->dev(), obs, obs_format, n_, s, only); });
        check_launch();
    }
    std::pair<const void*, size_t> frame_rows() override { return {desc_.p, sizeof(SpotDesc)}; }
    void draw_records(const void* records, int n_records, const int32_t* pick, int count, int fmt, void* obs, hipStream_t s) override {
        with_bool(P_.ordered_holes, [&](auto BO) {
            launch_raster_gather<SpotComposerT<decltype(BO)::value>, false>((const SpotDesc*)records, atlas_->dev(), obs, fmt, n_records, pick, count, err_.dev, s);
        });
        check_launch();
    }
    void draw_records_padded(const void* records, int n_records, const int32_t* pick, int count, int fmt, void* obs, hipStream_t s) override {
        with_bool(P_.ordered_holes, [&](auto BO) {
            launch_raster_gather<SpotComposerT<decltype(BO)::value>, true>((const SpotDesc*)records, atlas_->dev(), obs, fmt, n_records, pick, count, err_.dev, s);
        });
        check_launch();
    }

    void save_debug_records(const int32_t* idx, int count, void* rec, hipStream_t s) override {
        sets_.upload(s);
        launch_checked(spot_debug_desc_picked_kernel, dim3((count + 255) / 256), dim3(256), 0, s, P_, io(), idx, count, (SpotDesc*)rec);
    }
    void draw_debug_records(const void* records, int n_records, const int32_t* pick, int count, int size, void* rgb, hipStream_t s) override {
        with_bool(P_.ordered_holes, [&](auto BO) {
            launch_raster_debug_gather<SpotDebugComposerT<decltype(BO)::value>>((const SpotDesc*)records, atlas_->dev(), rgb, size, n_records, pick, count, err_.dev, s);
        });
        check_launch();
    }

    void raster(void* obs, hipStream_t s) { raster_only(obs, nullptr, s); }
    // (the fused raster / reset launch keeps terminal observations itself; lab MEMGYM_SPOT_FINAL_FUSED=0: the generic path of mg_step)
    bool keeps_final_obs(hipStream_t s) override {
        static const bool wanted = lab_flag("MEMGYM_SPOT_FINAL_FUSED", true);
        return wanted && !sets_.per_set() && fused_here(s);
    }
    // (a stream that is being captured into a graph: the image-order formats keep the two plain launches and mg_step's generic path there -- what
    // they took everywhere before the fused launch learnt them; the uint8 frame's fused launch is captured as it always was)
    bool fused_here(hipStream_t s) const {
        if (obs_format == MG_OBS_U8_XYC) return true;
        return !stream_capturing(s);
    }

    // Resets served inside the raster launch: on for the finite variant up to FUSE_MAX instances (more instances finish per step
    // than in the endless variant and their resets place up to five objects: ~15 us for the 16 lanes of an instance, the tail of
    // the step kernel).  Round 4, with the launch's agent-scope fence gone (profiles/r04_spot_step.md, M env-steps/s fused /
    // not): 16,384: 216 / 182, 32,768: 235 / 206, 65,536: 247 / 228, 131,072: 234 / 241 -- beyond FUSE_MAX the step kernel's reset
    // tail is amortised over several rounds of waves and the plain raster's seven workgroups per CU win.  The endless variant (its
    // step kernel's reset tail is 4 us) the other way round: off up to 16,384 instances (230 / 230; the plain raster stores with
    // the cached policy there), on beyond, where the plain raster stores non-temporally as well (32,768: 242-244 / 233-234,
    // 65,536: 245-248 / 239-242, 131,072: 256-257 / 236-252).  MEMGYM_SPOT_FUSE=0 / 1 (lab build) forces it off / on for both, in every format.
    // The other formats (profiles/spot_chw.md; M env-steps/s fused / not, two runs each, the same session):
    //   MG_OBS_U8_CYX, the uint8 frame's bytes: its thresholds.  Finite 16,384: 200.3-200.9 / 179.9-180.5, 65,536: 224.5-225.0 / 199.7-200.0; endless
    //   65,536: 242.2-242.3 / 221.2-221.9 (16,384 and below stays on two launches like the uint8 frame, not measured fused).
    //   Float formats: fused up to FUSE_MAX on BOTH ids.  Finite 16,384: bf16 120.3-120.7 / 110.9-111.1, f32 64.6-65.5 / 62.5-62.8; 65,536: bf16
    //   141.2-141.4 / 141.5-142.0 (0.3 % below, within the unfused form's own two-run spread of 0.4 %), f32 76.8-77.0 / 76.1-76.4.  Endless 16,384: bf16
    //   121.0-121.9 / 119.5-120.0, f32 65.4-66.7 / 64.8-66.1; 65,536: bf16 146.4-146.5 / 143.5-143.9, f32 77.3-77.7 / 77.4-77.5.  The stream-out
    //   bounds these launches, so the reset tail saved shows at 16,384 and hardly at 65,536; no row lost.  f16 follows bf16 (the same kernel but for
    //   the conversion instruction).  Beyond FUSE_MAX nothing is measured in these formats: two launches, as before.
    static constexpr int FUSE_MAX = 65536;
    // store flavour of the fused launch: it runs five workgroups per CU (the reset code's registers), where only the
    // non-temporal stream keeps up; MEMGYM_RASTER_NT forces (tuning only)
    bool fused_nt() const {
        static const int forced = lab_forced("MEMGYM_RASTER_NT");
        return forced >= 0 ? forced != 0 : true;
    }
    bool fuse_resets() const {
        static const int forced = lab_forced("MEMGYM_SPOT_FUSE");
        if (forced >= 0) return forced != 0;
        if (obs_format == MG_OBS_U8_XYC || obs_format == MG_OBS_U8_CYX) return P_.endless ? n_ > RASTER_PLAIN_MAX : n_ <= FUSE_MAX;
        return n_ <= FUSE_MAX;
    }

    OptionSets<SpotOpt> sets_;
    SpotParams& P_;  // set 0, the handle-wide set
    double coin_scale_, agent_speed_, agent_scale_, exit_scale_;
    double initial_spawn_interval_ = 30, spawn_interval_threshold_ = 10;

    std::unique_ptr<Atlas> atlas_;
    DevArray<SpotCore> core_;
    DevArray<double> sp_t_, sp_speed_, cos_, sin_;
    DevArray<uint32_t> sp_ang_;
    DevArray<uint4> jump_;  // SpotParams::jump
    DevArray<uint8_t> sp_r_;
    DevArray<int> queue_;  // deferred resets: the counters + n entries
    DevArray<int> flags_;  // [0] = SpotParams::ordered_holes: travels with the state (spotlights with a border may be alive in it)
    // finite variant: [0] = SpotParams::exit_gen, [1 + g] = exit_scale of generation g (0 = free); travels with the state (the
    // instances' exits name their generation, SpotCore::pad)
    DevArray<double> exit_hist_;
    double exit_gen_scale_[EXIT_GENS] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool exit_gen_used_[EXIT_GENS] = {false, false, false, false, false, false, false, false};
    DevArray<uint32_t> coins_;
    DevArray<SpotDesc> desc_;
};

void SpotFamily::raster_debug(void* frames, hipStream_t s) {
    debug_frames<SpotDesc>(
        s, [&](SpotDesc* dbg) { launch(spot_debug_desc_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, P_, io(), dbg); },
        [&](SpotDesc* dbg) {
            with_bool(P_.ordered_holes, [&](auto BO) { launch_raster<SpotDebugComposerT<decltype(BO)::value>>(dbg, atlas_->dev(), frames, MG_OBS_U8_XYC, n_, s); });
        });
}

Family* make_spot(int endless, int num_envs) { return new SpotFamily(endless, num_envs); }

}  // namespace mg

#ifdef MG_LAB_SPOT_CLOCK
extern "C" int mg_lab_spot_clock(unsigned long long* host, int n_waves, int clear) {
    if (clear) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(mg::g_lab_spot_clock)) != hipSuccess) return -1;
        return hipMemset(p, 0, sizeof(unsigned long long) * 10 * 65536) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(mg::g_lab_spot_clock), sizeof(unsigned long long) * 10 * (size_t)n_waves) == hipSuccess ? 0 : -1;
}
#endif
