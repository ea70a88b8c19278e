// mg_mystery.hip -- Mystery Path family on gfx950: MysteryPath-v0, MysteryPath-Grid-v0 and Endless-MysteryPath-v0.  The family's one translation unit: its three host
// classes and three small kernels are here, the rest of the device code in headers that only this file includes.
//
// Reference behaviour reproduced (bit-exact observations, rewards, dones, RNG consumption):
//   memory_gym/mystery_path.py          reset :130-200  step :202-276
//   memory_gym/mystery_path_grid.py     reset :129-199  step :201-277 (GridCharacterController, Discrete(4))
//   memory_gym/endless_mystery_path.py  reset :195-280  step :282-444  drawing :111-160
//   memory_gym/pygame_assets.py         Node :438-493  EndlessMysteryPath :495-604  MysteryPath (noisy A*) :606-736
//   memory_gym/character_controller.py  CharacterController.step :89-146
//
//   mg_mystery_types.hpp           constants; MysteryParams, MysteryCore, MysteryDesc, MysteryIO; queue counters and entry tags
//   mg_mystery_compose.hpp         MysteryComposer (the observation) and MysteryDebugComposer, each for sprites in registers and for BIG ones
//   mg_mystery_path.hpp            the noisy A*, twice: coop_path (a wave per path) and lane_path (a lane per path)
//   mg_mystery_finite.hpp          MysteryPath-v0 / -Grid-v0: reset, step, path service and their three kernels
//   mg_mystery_endless.hpp         Endless-MysteryPath-v0: segment store, step, resets, queue entries, owed segments and records ahead of time (device functions)
//   mg_mystery_endless_launch.hpp  ... and its emp_* kernels, launch constants and measurement hooks
//   mg_mystery_expert.hpp          mystery_expert_kernel: the scripted teacher of the three ids (mg_expert_actions), a launch of its own
//
// The host side mirrors the device headers, one class per machine (make_mystery picks; nothing outside this file knows):
//   MysteryFamily         abstract: what the three ids share -- option sets and the common keys, the atlas, the arrays of MysteryIO, checkpoint, teacher, raster, debug view
//   MysteryFiniteFamily   MysteryPath-v0 / -Grid-v0: the launches of mg_mystery_finite.hpp, the defer modes
//   MysteryEndlessFamily  Endless-MysteryPath-v0: the emp_* launches, the queue server, lazy / owed segments, records ahead of time, the segment capacity
//
// The launches of a step as shipped (auto-reset, one option set, uint8 observations, agent sprites that fit registers; why, and every other arrangement: DESIGN.md 3.1):
//   MysteryPath-Grid-v0     mystery_step_kernel, defer 1: every reset is queued -> mystery_raster_paths_kernel: its first 128 workgroups (and helpers, when the queue
//                           is long) generate the queued paths, the others draw the frames
//   MysteryPath-v0          the same two launches, defer 2: a wave serves up to HYBRID_INLINE resets itself and queues them all once it has more
//   Endless-MysteryPath-v0  emp_step_kernel: a lane per instance, due segments and most resets become queue entries -> emp_raster_serve_kernel: service workgroups take
//                           the entries and draw those instances' frames, background workgroups generate owed segments and the next episode's first (up to 20,480
//                           instances: entries of the service waves instead), the others draw the frames -- in all five observation formats
//                           (emp_raster_serve_kernel<FMT, EMP_NT, FINAL>; steps_fused(): not with per-instance option sets or BIG sprites)
//   Terminal observations kept (mg_info_buffers.final_obs_dev): the <FINAL> forms of the same launches; endless: plus one raster_sparse_kernel for the terminal frames,
//   in the handle's format.
#include <memory>

#include "mg_atlas_v1.hpp"
#include "mg_option_sets.hpp"
#include "mg_stamps.hpp"
#include "mg_mystery_types.hpp"
#include "mg_mystery_compose.hpp"
#include "mg_raster_gather_v1.hpp"
#include "mg_mystery_path.hpp"
#include "mg_mystery_finite.hpp"
#include "mg_mystery_endless.hpp"
#include "mg_mystery_endless_launch.hpp"
#include "mg_mystery_expert.hpp"

namespace mg {

// info["ground_truth"] in float64: the one-hot direction of the next path tile (endless_mystery_path.py:92-97)
__global__ __launch_bounds__(256) void mystery_gt64_kernel(int n, const MysteryCore* core, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MysteryCore s = load_core(core + i);
    out[3 * i + 0] = (double)s.td[0];
    out[3 * i + 1] = (double)s.td[1];
    out[3 * i + 2] = (double)s.td[2];
}

__global__ __launch_bounds__(256) void mystery_gt64_masked_kernel(int n, const MysteryCore* core, double* out, const uint8_t* __restrict__ only) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !only[i]) return;
    const MysteryCore s = load_core(core + i);
    out[3 * i + 0] = (double)s.td[0];
    out[3 * i + 1] = (double)s.td[1];
    out[3 * i + 2] = (double)s.td[2];
}

// Debug descriptors from the state and the current frame descriptors (see MysteryDebugComposer; oracle/mgo_mystery.c
// mpf_debug / emp_debug).
template <bool PS>
__global__ __launch_bounds__(256) void mystery_debug_desc_kernel(MysteryParams P0, MysteryIO io, MysteryDesc* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n) return;
    const MysteryParams& P = PS ? io.sets[set_index(io.set_of, i)] : P0;
    const MysteryCore s = io.core[i];
    MysteryDesc d = io.desc[i];
    d.valid = 1;
    d.tile_mask[0] = d.tile_mask[1] = 0;
    if (!P.endless) {
        mp_desc(P, s, d);  // from the state alone: a handle restored by mg_set_state has no frame descriptors before its first step
        d.pad8[0] = 1;
        const uint64_t ends = (1ull << (s.sx * G + s.sy)) | (1ull << (s.ex * G + s.ey));
        d.tile_mask[0] = s.path_mask & ~ends;
        d.tile_mask[1] = io.walls[i];
        d.goal_on = d.origin_on = 1;
        d.goal_x = s.ex; d.goal_y = s.ey;
        d.origin_x = s.sx; d.origin_y = s.sy;
        d.tile_x0 = 0;
        d.cross_on = s.cross_on;  // the cross surface keeps its alpha: the observation's visibility
    } else {
        d.pad8[0] = 2;
        const int x0 = floordiv_pos(s.camera_x, P.tile);
        d.tile_x0 = x0 * P.tile - s.camera_x;
        const int seg_lo = x0 / (G + 1) - 1, seg_hi = (x0 + 16) / (G + 1) + 1;
        for (int seg = seg_lo < 0 ? 0 : seg_lo; seg <= seg_hi && seg < s.num_seg; ++seg) {
            const uint8_t* sp = seg_ptr(io, i, seg);
            const int cnt = sp[0];
            for (int k = 1; k <= cnt; ++k) {
                const int col = node_x(seg, sp[k]) - x0, y = node_y(sp[k]);
                if (col >= 0 && col < 16) {
                    const int cell = col * G + y;
                    d.tile_mask[cell >> 6] |= 1ull << (cell & 63);
                }
            }
        }
        d.stamina_on = 1;  // blitted whatever show_stamina says
        const int st = s.stamina < P.stamina_level ? s.stamina : P.stamina_level;
        d.stamina_red = (uint8_t)(int)(SCREEN * (1 - ((double)st / P.stamina_level)));
    }
    out[i] = d;
}

// The same descriptor for ONE instance, for the picked form below (a body of its own: mystery_debug_desc_kernel stays the code it was).
__device__ __forceinline__ MysteryDesc mystery_debug_desc_one(const MysteryParams& P, const MysteryIO& io, int i) {
    const MysteryCore s = io.core[i];
    MysteryDesc d = io.desc[i];
    d.valid = 1;
    d.tile_mask[0] = d.tile_mask[1] = 0;
    if (!P.endless) {
        mp_desc(P, s, d);  // from the state alone: a handle restored by mg_set_state has no frame descriptors before its first step
        d.pad8[0] = 1;
        const uint64_t ends = (1ull << (s.sx * G + s.sy)) | (1ull << (s.ex * G + s.ey));
        d.tile_mask[0] = s.path_mask & ~ends;
        d.tile_mask[1] = io.walls[i];
        d.goal_on = d.origin_on = 1;
        d.goal_x = s.ex; d.goal_y = s.ey;
        d.origin_x = s.sx; d.origin_y = s.sy;
        d.tile_x0 = 0;
        d.cross_on = s.cross_on;  // the cross surface keeps its alpha: the observation's visibility
    } else {
        d.pad8[0] = 2;
        const int x0 = floordiv_pos(s.camera_x, P.tile);
        d.tile_x0 = x0 * P.tile - s.camera_x;
        const int seg_lo = x0 / (G + 1) - 1, seg_hi = (x0 + 16) / (G + 1) + 1;
        for (int seg = seg_lo < 0 ? 0 : seg_lo; seg <= seg_hi && seg < s.num_seg; ++seg) {
            const uint8_t* sp = seg_ptr(io, i, seg);
            const int cnt = sp[0];
            for (int k = 1; k <= cnt; ++k) {
                const int col = node_x(seg, sp[k]) - x0, y = node_y(sp[k]);
                if (col >= 0 && col < 16) {
                    const int cell = col * G + y;
                    d.tile_mask[cell >> 6] |= 1ull << (cell & 63);
                }
            }
        }
        d.stamina_on = 1;  // blitted whatever show_stamina says
        const int st = s.stamina < P.stamina_level ? s.stamina : P.stamina_level;
        d.stamina_red = (uint8_t)(int)(SCREEN * (1 - ((double)st / P.stamina_level)));
    }
    return d;
}
// mg_save_debug_frames: record j <- the debug descriptor of instance idx[j] (idx == NULL: instance j), one lane per entry.  An entry < 0 is skipped, one
// >= n is skipped and flagged; a skipped entry's record is not written.
template <bool PS>
__global__ __launch_bounds__(256) void mystery_debug_desc_picked_kernel(MysteryParams P0, MysteryIO io, const int32_t* __restrict__ idx, int count,
                                                                        MysteryDesc* rec) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const int i = idx ? idx[j] : j;
    if (i < 0) return;
    if (i >= P0.n) return raise_error(io.err, ERR_FRAME_INDEX);
    const MysteryParams& P = PS ? io.sets[set_index(io.set_of, i)] : P0;
    rec[j] = mystery_debug_desc_one(P, io, i);
}

__global__ __launch_bounds__(256) void mystery_init_kernel(int n, MysteryCore* core) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    MysteryCore s;
    memset(&s, 0, sizeof(s));
    core[i] = s;
}

static const double SCALE = 0.25;

// What the three ids share on the host.  Which launches reset and step a handle is the concrete class's business; its constructor sets the id's defaults, sizes the arrays
// the two machines size differently (segs_, aux_) and ends in start().
class MysteryFamily : public Family {
   public:
    // One key of the reset options, for option set `set` (0 = the handle-wide set of mg_set_option).  Sets > 0 hold everything that
    // does not change the geometry (sprites, camera offset and speeds are shared by the handle's instances).
    // Here: the keys the three ids share and the refusal of an unknown one; a concrete class reads its own keys first.
    void set_option(const std::string& key, const double* v, int n) override { set_option_set(0, key, v, n); }
    void set_option_set(int set, const std::string& key, const double* v, int n) override {
        MysteryParams& P = sets_.ensure(set).P;
        const OptionArg A{set, key, v, n, dirty_};
        if (key == "max_steps") P.max_steps = A.integer();
        else if (key == "agent_scale") A.geometry(agent_scale_, v[0]);
        else if (!P_.grid && key == "agent_speed") A.geometry(agent_speed_, v[0]);
        else if (key == "show_origin") P.show_origin = A.flag();
        else if (key == "visual_feedback") P.visual_feedback = A.flag();
        else if (key == "reward_fall_off") P.r_fall = v[0];
        else if (key == "reward_path_progress") P.r_progress = v[0];
        else if (key == "reward_step") P.r_step = v[0];
        else throw OptionError{-2, "unknown reset parameter " + key};
    }
    void bind_option_sets(const int32_t* set_of_dev) override { sets_.bind(set_of_dev); }

    std::vector<std::pair<void*, size_t>> state_blobs() override {
        // The same four blobs for every id, whether or not the id has anything to say in them (finite: the 16 bytes of aux_; endless: walls_): the payload's
        // size is what mg_set_state checks.  (aux: fall-off lists, and the records generated ahead of time -- they belong to the state: the EMP_PRE flags travel in `core`)
        std::vector<std::pair<void*, size_t>> v = {{core_.p, core_.bytes()}, {segs_.p, segs_.bytes()}, {aux_.p, aux_.bytes()},
                                                  {walls_.p, walls_.bytes()}};
        rng_.blobs(v);
        return v;
    }
    // core, the segment store / path order and the frame descriptor of every id; the endless id's aux row (fall-off list, the record ahead of time: EMP_PRE travels
    // in `core`), the finite ids' wall cells.  Not rows: the finite ids' 16-byte aux_ (no kernel reads it) and the endless id's walls_ (no kernel is given it);
    // queue_, bgq_, bgflag_, tdesc_ and stats_ are words of a launch or counters of the handle.
    std::vector<std::pair<void*, size_t>> instance_rows() override {
        std::vector<std::pair<void*, size_t>> v = {{core_.p, sizeof(MysteryCore)}, {segs_.p, segs_.bytes() / (size_t)n_}, {desc_.p, sizeof(MysteryDesc)}};
        if (P_.endless) v.push_back({aux_.p, sizeof(uint32_t) * AUX_WORDS});
        else v.push_back({walls_.p, sizeof(uint64_t)});
        rng_.rows(v);
        return v;
    }
    // (Endless: whatever is owed stays owed -- the node the expert aims at exists when a step has returned, mg_mystery_expert.hpp emp_expert)
    void expert_actions(const ExpertArgs& x, hipStream_t s) override {
        require_geometry();
        sets_.upload(s);
        launch_checked(mystery_expert_kernel, expert_grid(n_), dim3(EXPERT_BLOCK), 0, s, P_, io(), x);
    }
    // the counters the kernels keep in MysteryIO::stats
    bool debug_counter(const std::string& name, int64_t* out) override {
        const int k = name == "path_gen_ticks" ? 0 : (name == "path_gen_paths" ? 1 : (name == "emp_own_resets" ? 2 : (name == "emp_ahead_records" ? 3 : (name == "emp_final_served" ? 4 : (name == "path_lane_paths" ? 5 : -1)))));
        if (k < 0 || !stats_.p) return false;
        unsigned long long v = 0;
        MG_HIP(hipMemcpy(&v, stats_.p + k, sizeof v, hipMemcpyDeviceToHost));
        *out = (int64_t)v;
        return true;
    }
    void raster_debug(void* frames, hipStream_t s) override;
    void raster_only(void* obs, const uint8_t* only, hipStream_t s) override {
        with_composers([&](auto C) { launch_raster<typename decltype(C)::Obs>(desc_.p, atlas_->dev(), obs, obs_format, n_, s, only); });
        check_launch();
    }
    // (Endless: the descriptor rows are complete once the step's launches have run -- a queued instance's row is rewritten by the wave that serves its entry,
    // emp_serve_entry -- so a save reads them as mg_render does, behind nothing but the stream's order; owed segments are no part of a descriptor)
    std::pair<const void*, size_t> frame_rows() override { return {desc_.p, sizeof(MysteryDesc)}; }
    void draw_records(const void* records, int n_records, const int32_t* pick, int count, int fmt, void* obs, hipStream_t s) override {
        const MysteryDesc* rec = (const MysteryDesc*)records;
        with_composers([&](auto C) { launch_raster_gather<typename decltype(C)::Obs, false>(rec, atlas_->dev(), obs, fmt, n_records, pick, count, err_.dev, s); });
        check_launch();
    }
    void draw_records_padded(const void* records, int n_records, const int32_t* pick, int count, int fmt, void* obs, hipStream_t s) override {
        const MysteryDesc* rec = (const MysteryDesc*)records;
        with_composers([&](auto C) { launch_raster_gather<typename decltype(C)::Obs, true>(rec, atlas_->dev(), obs, fmt, n_records, pick, count, err_.dev, s); });
        check_launch();
    }
    // (Endless: the debug view reads the segment store -- owed segments are generated first, on the call's stream, as before an instance save)
    void save_debug_records(const int32_t* idx, int count, void* rec, hipStream_t s) override {
        before_instance_save(s);
        sets_.upload(s);
        with_bool(sets_.per_set(), [&](auto PS) {
            launch_checked(mystery_debug_desc_picked_kernel<decltype(PS)::value>, dim3((count + 255) / 256), dim3(256), 0, s, P_, io(), idx, count, (MysteryDesc*)rec);
        });
    }
    void draw_debug_records(const void* records, int n_records, const int32_t* pick, int count, int size, void* rgb, hipStream_t s) override {
        const MysteryDesc* rec = (const MysteryDesc*)records;
        with_composers([&](auto C) { launch_raster_debug_gather<typename decltype(C)::Debug>(rec, atlas_->dev(), rgb, size, n_records, pick, count, err_.dev, s); });
        check_launch();
    }

   protected:
    MysteryFamily(int variant, int n) : Family(n), P_(sets_[0].P) {  // 0 MysteryPath-v0, 1 Endless-MysteryPath-v0, 2 MysteryPath-Grid-v0
        memset(&P_, 0, sizeof(P_));
        P_.endless = variant == 1;
        P_.grid = variant == 2;
        P_.n = n;
        agent_scale_ = 1.0 * SCALE;
        agent_speed_ = 12.0 * SCALE;
        P_.visual_feedback = 1;
        P_.r_fall = 0.0; P_.r_progress = 0.1; P_.r_step = 0.0;
        // Every kernel of the family takes the whole MysteryParams by value, so the launch constants that only one machine's kernels read are filled in for
        // every id, as they always were (path_help: the finite ids' path service; bg_coop and the two capacities: the endless id)
        P_.path_help = lab_int("MEMGYM_PATH_HELP", 1);
        P_.bg_coop = lab_int("MEMGYM_EMP_BG_COOP", n <= 20480 ? 1 : 0);
        P_.seg_cap = std::min(MAX_SEG, std::max(4, lab_int("MEMGYM_EMP_SEG_CAP", MAX_SEG)));    // (lab build: tests reach the capacities in a few
        P_.fall_cap = std::min(MAX_FALL, std::max(1, lab_int("MEMGYM_EMP_FALL_CAP", MAX_FALL)));  // hundred steps, tests/test_gpu_capacity.py)
        core_.alloc(n);
        walls_.alloc(n);
        desc_.alloc(n);
        tdesc_.alloc(n);  // (64 B per instance; allocated here so that no step allocates)
        rng_.alloc(n);
        err_.alloc();
        queue_.alloc((size_t)n + 32 + QC_WORDS);
        {   // WaveRng: s_k = A^k s_0 + S_k inc for k = 1 .. 64 (PCG64's 128-bit LCG, multiplier as in mg_device.hpp Pcg::advance)
            const u128 A = (((u128)0x2360ED051FC65DA4ull) << 64) | (u128)0x4385DF649FCCF645ull;
            std::vector<uint4> jt(128);
            u128 m = 1, q = 0;
            for (int k = 0; k < 64; ++k) {
                q = q * A + 1;  // S_(k+1) = S_k A + 1
                m = m * A;      // A^(k+1)
                jt[2 * k] = make_uint4((uint32_t)m, (uint32_t)(m >> 32), (uint32_t)(m >> 64), (uint32_t)(m >> 96));
                jt[2 * k + 1] = make_uint4((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)(q >> 64), (uint32_t)(q >> 96));
            }
            jump_.upload(jt);
            stats_.alloc(8);
        }
        sets_.alloc();
    }
    // tail of a concrete class's constructor, once its defaults are in P_ and its arrays exist
    void start() {
        launch(mystery_init_kernel, dim3((n_ + 255) / 256), dim3(256), 0, 0, n_, core_.p);
        MG_HIP(hipDeviceSynchronize());
        rebuild();
        sets_.defaults = P_;
    }

    // one option set: the parameter block and the list behind it
    struct MysteryOpt {
        MysteryParams P;
        OptListStore st_cardinal;
        // what the shared atlas, the camera and the launch arrangement fix for every set of the handle (incl. lazy = 0 whenever sets
        // are in use: the plain arrangement generates every segment when it is due)
        static void copy_geometry(MysteryParams& d, const MysteryParams& s) {
            d.endless = s.endless; d.grid = s.grid; d.n = s.n; d.depth = s.depth; d.agent_radius = s.agent_radius; d.sprite_dim = s.sprite_dim;
            d.v_axis_i = s.v_axis_i; d.v_diag_i = s.v_diag_i; d.tile = s.tile; d.cross_dim = s.cross_dim; d.camera_offset = s.camera_offset;
            d.svc_prio = s.svc_prio; d.lazy = s.lazy; d.path_help = s.path_help; d.bg_coop = s.bg_coop; d.pre = s.pre; d.lazy_append = s.lazy_append;
            d.seg_cap = s.seg_cap; d.fall_cap = s.fall_cap;
        }
    };

    // What every launch of the family is given: the shared arrays here, the rest by the concrete class.  No pointer of it is ever null but `walls` on the endless id.
    virtual MysteryIO io() = 0;
    MysteryIO shared_io() {
        MysteryIO o;
        o.core = core_.p;
        o.segs = segs_.p;
        o.rng = rng_.view();
        o.seg_rows = MAX_SEG;
        o.desc = desc_.p;
        o.err = err_.dev;
        o.queue = queue_.p;
        o.walls = nullptr;
        o.qctr = queue_.p + ((n_ + 31) & ~31);
        o.bgq = nullptr;  // (these two: set by either concrete class)
        o.bgflag = nullptr;
        o.aux = aux_.p;
        o.jump = jump_.p;
        o.stats = stats_.p;
        o.sets = sets_.dev();
        o.set_of = sets_.set_of();
        o.tdesc = tdesc_.p;
        return o;
    }

    void rebuild() {
        int radius = 0;
        // (MysteryPath-Grid-v0 accepts agent_scale and never reads it: GridCharacterController(SCALE, ...), mystery_path_grid.py:188)
        std::vector<Stamp> sprites = build_agent_sprites(P_.grid ? 1.0 * SCALE : agent_scale_, &radius);
        P_.agent_radius = radius;
        P_.sprite_dim = sprites[0].w;
        double inv = 1.0 / std::sqrt(2.0);
        P_.v_axis_i = (int)((1.0 / 1.0) * agent_speed_);
        P_.v_diag_i = (int)(inv * agent_speed_);
        P_.tile = SCREEN / G;
        double cos_ = camera_offset_scale_ < 0 ? 0 : (camera_offset_scale_ > 5.5 ? 5.5 : camera_offset_scale_);
        double cam = -P_.tile * cos_;
        if (cam != std::floor(cam)) throw OptionError{-3, "camera_offset_scale must give an integral pixel offset (multiples of 1/12)"};
        P_.camera_offset = (int)cam;
        P_.depth = (int)camera_offset_scale_;
        if (P_.depth > 7) throw OptionError{-3, "camera_offset_scale too large"};
        Stamp cross = build_cross(SCALE);
        P_.cross_dim = cross.w;
        atlas_.reset(new Atlas());
        // MysteryComposer holds a sprite of up to 1,024 pixels in StampRegs<4>; a larger one (agent_scale beyond 0.28) switches the
        // handle to MysteryBigComposer and to the plain launch arrangement (the fused launches compose with the register form)
        big_sprites_ = sprites[0].w * sprites[0].h > 1024;
        for (auto& sp : sprites) atlas_->add_stamp(sp);  // 0..7
        atlas_->add_stamp(cross, 256);                    // 8      (StampRegs<1>; build_cross(SCALE): no option scales it)
        add_templates(*atlas_);
        atlas_->upload();
        dirty_ = false;
        ++geom_gen_;
    }
    virtual void add_templates(Atlas&) {}  // rebuild(): the id's background templates, if it has any

    // The composers every raster launch of the handle draws with, chosen once: f(C) with decltype(C)::Obs the observation's and ::Debug the debug view's
    // (agent sprites beyond MysteryComposer's registers: the Big pair).  A launch names its launcher and one of the two, nothing else.
    template <class O, class D>
    struct Composers {
        using Obs = O;
        using Debug = D;
    };
    template <class F>
    void with_composers(F&& f) {
        if (big_sprites_) f(Composers<MysteryBigComposer, MysteryDebugBigComposer>{});
        else f(Composers<MysteryComposer, MysteryDebugComposer>{});
    }

    void raster(void* obs, hipStream_t s) { raster_only(obs, nullptr, s); }
    // tail of reset(): the frames of the instances that were reset
    void draw_reset_frames(const uint8_t* mask, void* obs, hipStream_t s) {
        reset_frames(mask, [&](const uint8_t* m) {
            with_composers([&](auto C) { launch_raster_sparse<typename decltype(C)::Obs>(desc_.p, atlas_->dev(), obs, obs_format, n_, s, m); });
        }, [&] { raster(obs, s); });
    }
    // tail of a step() in the plain arrangement: the logic is out, the frames are a launch of their own (a headless step has none; a masked step, active != NULL:
    // the active instances' alone)
    void plain_frames(void* obs, hipStream_t s, const uint8_t* active = nullptr) {
        end_logic(s);
        if (!obs) return;
        if (active) return masked_frames(obs, active, s);
        prof.begin(1, s);
        raster(obs, s);
        prof.end(1, s);
    }

    OptionSets<MysteryOpt> sets_;
    MysteryParams& P_;  // set 0, the handle-wide set
    // camera_offset_scale_: an option of the endless id alone; rebuild() derives camera_offset and depth from it for every id
    double agent_scale_, agent_speed_, camera_offset_scale_ = 5.0;
    bool big_sprites_ = false;  // rebuild(): the agent sprites exceed MysteryComposer's registers
    std::unique_ptr<Atlas> atlas_;
    DevArray<MysteryCore> core_;
    DevArray<uint8_t> segs_;  // endless: the segment store; finite: the order of every instance's path (path_order, mg_mystery_types.hpp)
    DevArray<MysteryDesc> desc_, tdesc_;  // tdesc_: terminal-frame descriptors of the FINAL kernels
    DevArray<int> queue_;  // n entries + the counters
    DevArray<uint32_t> aux_;  // endless: per instance, the next episode's first segment + the stream behind it (EMP_PRE) and the fall-off list; finite: four words
    DevArray<uint4> jump_;  // WaveRng jump constants
    DevArray<unsigned long long> stats_;  // MysteryIO::stats
    DevArray<uint64_t> walls_;  // finite: wall cells of every instance's path generation (debug view); endless: a blob of the checkpoint, no kernel is given it
};

void MysteryFamily::raster_debug(void* frames, hipStream_t s) {
    debug_frames<MysteryDesc>(
        s,
        [&](MysteryDesc* dbg) {
            sets_.upload(s);
            with_bool(sets_.per_set(), [&](auto PS) {
                launch(mystery_debug_desc_kernel<decltype(PS)::value>, dim3((n_ + 255) / 256), dim3(256), 0, s, P_, io(), dbg);
            });
        },
        [&](MysteryDesc* dbg) {
            with_composers([&](auto C) { launch_raster<typename decltype(C)::Debug>(dbg, atlas_->dev(), frames, MG_OBS_U8_XYC, n_, s); });
        });
}

// MysteryPath-v0 (variant 0) and MysteryPath-Grid-v0 (variant 2): mystery_reset_kernel, mystery_step_kernel<PS, FINAL> and, where the paths of a step's resets are
// deferred, mystery_raster_paths_kernel (mg_mystery_finite.hpp).
class MysteryFiniteFamily final : public MysteryFamily {
   public:
    MysteryFiniteFamily(int variant, int n) : MysteryFamily(variant, n) {
        P_.svc_prio = lab_int("MEMGYM_SVC_PRIO", 0);  // (measured on the endless id; no effect on MysteryPath-Grid's path service)
        P_.max_steps = P_.grid ? 128 : 512;
        if (P_.grid) P_.r_progress = 0.0;
        sets_[0].st_cardinal.set(P_.cardinal, {0, 1, 2, 3});
        P_.r_goal = 1.0;
        no_bgq_.alloc(1);
        no_bgflag_.alloc(1);
        segs_.alloc((size_t)n * PATH_ORDER_STRIDE);
        aux_.alloc(4);
        start();
    }
    int action_dim() const override { return P_.grid ? 1 : 2; }
    int gt_dim() const override { return 0; }
    const char* info_name(int k) const override { return k == 0 ? "success" : (k == 1 ? "num_fails" : nullptr); }

    void set_option_set(int set, const std::string& key, const double* v, int n) override {
        MysteryOpt& O = sets_.ensure(set);
        MysteryParams& P = O.P;
        const OptionArg A{set, key, v, n, dirty_};
        if (key == "cardinal_origin_choice") {
            A.must_be(n >= 1);  // any length; every value other than 0, 1, 2 takes the reference's `else` branch (mystery_path.py:155-166)
            std::vector<int> vals(n);
            for (int k = 0; k < n; ++k) {
                const int c = A.integer(k);
                vals[k] = (c >= 0 && c <= 2) ? c : 3;
            }
            O.st_cardinal.set(P.cardinal, vals);
        }
        else if (key == "show_goal") P.show_goal = A.flag();
        else if (key == "reward_goal") P.r_goal = v[0];
        else MysteryFamily::set_option_set(set, key, v, n);
    }

    void reset(const int64_t* seeds, const uint8_t* mask, void* obs, float* gt, hipStream_t s) override {
        if (dirty_) rebuild();
        require_seeded(seeds);
        if (seeds) seeded_ = true;
        sets_.upload(s);
        with_bool(sets_.per_set(), [&](auto PS) {
            launch(mystery_reset_kernel<decltype(PS)::value>, dim3(blocks()), dim3(256), WS_BYTES, s, P_, io(), seeds, mask, nullptr, lpw());
        });
        draw_reset_frames(mask, obs, s);
    }

    void step(const int32_t* actions, const uint8_t* active, void* obs, float* reward, uint8_t* done, float* gt, const mg_info_dev* info,
              int autoreset, hipStream_t s, void* final_frames) override {
        const mg_info_dev ib = begin_step(info);
        prof.begin(0, s);
        // (per-instance option sets: only this kernel has a <PS> form -- the raster launch's path service reads nothing of the options)
        // (a headless step, obs == NULL: the paths are generated in the step kernel -- there is no raster launch to serve them)
        const int defer = (obs && !active && autoreset && !big_sprites_) ? defer_mode() : 0;
        sets_.upload(s);
        if (final_frames) {  // terminal frame records (obs == NULL): the RECORDS form of the step kernel, masked or not, with the paths generated in it
            with_bool(sets_.per_set(), [&](auto PS) {
                with_bool(active != nullptr, [&](auto MASKED) {
                    launch(mystery_step_records_kernel<decltype(PS)::value, decltype(MASKED)::value>, dim3(blocks()), dim3(256), WS_BYTES, s, P_, io(), actions, active,
                           reward, done, ib, autoreset, lpw(), (MysteryDesc*)final_frames);
                });
            });
            return plain_frames(obs, s, active);
        }
        if (active) {  // a masked step: the MASKED form of the step kernel with the paths generated in it, then the active instances' frames
            with_bool(sets_.per_set(), [&](auto PS) {
                launch(mystery_step_masked_kernel<decltype(PS)::value>, dim3(blocks()), dim3(256), WS_BYTES, s, P_, io(), actions, active, reward, done, ib, autoreset, lpw());
            });
            return plain_frames(obs, s, active);
        }
        // (three of the four <PS, FINAL> forms exist: terminal observations are kept by handles with one option set only)
        auto step_launch = [&](auto kernel) { launch(kernel, dim3(blocks()), dim3(256), WS_BYTES, s, P_, io(), actions, reward, done, nullptr, ib, autoreset, lpw(), defer); };
        if (autoreset && ib.final_obs_dev && keeps_final_obs(s)) {  // terminal observations kept by these two launches (defer != 0, one option set)
            step_launch(mystery_step_kernel<false, true>);
            end_logic(s);
            prof.begin(1, s);
            raster_with_paths(obs, s, ib.final_obs_dev);
            prof.end(1, s);
            return;
        }
        if (sets_.per_set()) step_launch(mystery_step_kernel<true>);
        else step_launch(mystery_step_kernel<false>);
        if (defer) {  // the paths of this step's resets are generated by the first workgroups of the raster launch
            end_logic(s);
            prof.begin(1, s);
            raster_with_paths(obs, s);
            prof.end(1, s);
            return;
        }
        plain_frames(obs, s);
    }
    // the step + raster / path-service launches keep terminal observations themselves, in every observation format; lab MEMGYM_MYSTERY_FINAL_FUSED=0: the
    // generic path of mg_step
    bool keeps_final_obs(hipStream_t) override {
        static const bool wanted = lab_flag("MEMGYM_MYSTERY_FINAL_FUSED", true);
        return wanted && !big_sprites_ && !sets_.per_set() && defer_mode() != 0;
    }

   private:
    // instance-carrying lanes per wave (see instance_of_lane); MEMGYM_MYSTERY_LPW overrides for tuning
    int lpw() const {
        static const int forced = lab_int("MEMGYM_MYSTERY_LPW", 0);
        if (forced == 4 || forced == 8 || forced == 16 || forced == 32 || forced == 64) return forced;
        return 16;  // measured: profiles/r01e_logic_tails.md
    }
    int blocks() const { const int per_block = 4 * lpw(); return (n_ + per_block - 1) / per_block; }
    // 0: paths of auto-resets in the step kernel; 1: all of them queued for the raster launch (MysteryPath-Grid: 0.5 % of the
    // instances reset per step, logic 32.7 -> 12.1 us); 2: hybrid, a wave queues its requests only when it has more than
    // HYBRID_INLINE of them (MysteryPath-v0: its 512-step episodes reset too rarely to pay for always queueing, but the step
    // in which all survivors are truncated at once was a 450-us launch).  MEMGYM_MYSTERY_DEFER=0 / 1 / 2 forces a mode.
    int defer_mode() const {
        static const int forced = lab_int("MEMGYM_MYSTERY_DEFER", -1);
        return forced >= 0 && forced <= 2 ? forced : (P_.grid != 0 ? 1 : 2);
    }
    void raster_with_paths(void* obs, hipStream_t s, void* final_obs = nullptr) {
        const dim3 grid(frames_grid(n_) + PATH_WGS);
        auto paths_launch = [&](auto kernel) { launch_checked(kernel, grid, dim3(256), RASTER_LDS, s, desc_.p, atlas_->dev(), obs, n_, P_, io(), final_obs); };
        with_obs_format(obs_format, [&](auto F) {
            if (final_obs) paths_launch(mystery_raster_paths_kernel<decltype(F)::value, true>);
            else paths_launch(mystery_raster_paths_kernel<decltype(F)::value>);
        });
    }
    MysteryIO io() override {
        MysteryIO o = shared_io();
        o.walls = walls_.p;
        o.bgq = no_bgq_.p;
        o.bgflag = no_bgflag_.p;
        return o;
    }
    DevArray<int> no_bgq_;         // MysteryIO::bgq and ::bgflag of a finite handle: one element each, read by no kernel it launches
    DevArray<uint8_t> no_bgflag_;
};

// Endless-MysteryPath-v0: the emp_* kernels (mg_mystery_endless_launch.hpp).  A step is emp_step_kernel and then either the fused launch (emp_raster_serve_kernel: queue
// service, background jobs and frames in one) or the plain arrangement (emp_serve_kernel, raster); steps_fused() says which, and what comes with it.
class MysteryEndlessFamily final : public MysteryFamily {
   public:
    explicit MysteryEndlessFamily(int n) : MysteryFamily(1, n) {
        // 187-189 -> 175-182 us per fused launch (profiles/r03_emp.md)
        P_.svc_prio = lab_int("MEMGYM_SVC_PRIO", 1);
        lazy_wanted_ = lab_flag("MEMGYM_EMP_LAZY", true);
        // the next episode's first segment ahead of time (EMP_PRE): with the lane-per-path background jobs of the larger launches
        // (as entries of the service queue -- bg_coop -- a record ahead of time costs the path it saves)
        pre_wanted_ = !P_.bg_coop && lab_flag("MEMGYM_EMP_PRE", true);
        P_.max_steps = -1; P_.show_past_path = 1; P_.stamina_level = 20;
        bgq_.alloc((size_t)n);
        bgflag_.alloc((size_t)n);
        segs_.alloc((size_t)n * seg_rows_ * SEG_STRIDE);
        aux_.alloc((size_t)n * AUX_WORDS);
        start();
    }

    // include/memgym.h: mg_set_capacity.  "path_segments": records of the segment store per instance -- the
    // reference's path grows without limit (pygame_assets.py:559); an episode that needs one more segment than this ends (capacity_dev)
    void set_capacity(const std::string& what, int64_t v) override {
        if (what != "path_segments") return Family::set_capacity(what, v);
        if (v < 4 || v > EMP_MAX_SEG_CAP) throw OptionError{-3, "path_segments: 4 .. 32,767"};
        if (seeded_) throw std::runtime_error("mg_set_capacity: before the first reset");
        MG_HIP(hipDeviceSynchronize());
        seg_rows_ = (int)v;
        segs_.alloc((size_t)n_ * seg_rows_ * SEG_STRIDE);
        P_.seg_cap = seg_rows_;
        ++geom_gen_;
        sets_.refresh_geometry();
    }
    int64_t capacity(const std::string& what) const override {
        if (what == "path_segments") return P_.seg_cap;
        if (what == "fall_off_cells") return P_.fall_cap;
        return Family::capacity(what);
    }
    int action_dim() const override { return 1; }
    int gt_dim() const override { return 3; }
    const char* info_name(int k) const override { return k == 0 ? "num_fails" : (k == 1 ? "max_x" : (k == 2 ? "tiles_visited" : nullptr)); }

    void set_option_set(int set, const std::string& key, const double* v, int n) override {
        MysteryParams& P = sets_.ensure(set).P;
        const OptionArg A{set, key, v, n, dirty_};
        if (key == "show_origin") P.show_origin = 0;  // dead branch in the reference (:150)
        else if (key == "show_past_path") P.show_past_path = A.flag();
        else if (key == "show_background") P.show_background = A.flag();
        else if (key == "show_stamina") P.show_stamina = A.flag();
        else if (key == "camera_offset_scale") A.geometry(camera_offset_scale_, v[0]);
        else if (key == "stamina_level") { P.stamina_level = A.integer(); A.must_be(P.stamina_level > 0); }
        else if (key == "reward_path_progress_dense") P.r_dense = v[0];
        else MysteryFamily::set_option_set(set, key, v, n);
    }

    void reset(const int64_t* seeds, const uint8_t* mask, void* obs, float* gt, hipStream_t s) override {
        if (dirty_) rebuild();
        require_seeded(seeds);
        if (seeds) seeded_ = true;
        mg_info_dev none;
        memset(&none, 0, sizeof(none));
        // a masked reset(seed=None) of a handle whose steps run the fused arrangement: reset like the auto-reset step resets (lazy
        // segments, records ahead of time: emp_masked_reset_kernel); lab MEMGYM_EMP_MASKED_FAST=0: through the queue server like any other
        static const bool fast_wanted = lab_flag("MEMGYM_EMP_MASKED_FAST", true);
        const bool fast = fast_wanted && mask && !seeds && lazy_wanted_ && steps_fused();
        P_.lazy = fast ? 1 : 0;  // (otherwise an explicit reset generates all three segments; whatever an old episode is owed comes first)
        P_.pre = (fast && pre_wanted_) ? 1 : 0;
        P_.lazy_append = 0;
        if (fast) owed_possible_ = true;
        sets_.upload(s);
        if (fast) {  // (fast: one option set)
            launch(emp_masked_reset_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, P_, io(), mask, gt);
            serve(false, seeds, nullptr, nullptr, gt, none, 0, s);
        } else if (mask) {
            launch(emp_enqueue_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, n_, io(), mask);
            serve(false, seeds, nullptr, nullptr, gt, none, 0, s);
        } else if (n_ >= 1024 && reset_by_lanes() && !sets_.per_set()) {  // many paths at once: one lane per instance
            launch(emp_reset_lanes_kernel, dim3((n_ + 63) / 64), dim3(64), LW_BYTES, s, P_, io(), seeds, gt);
        } else {
            serve(true, seeds, nullptr, nullptr, gt, none, 0, s);
        }
        draw_reset_frames(mask, obs, s);
    }

    void step(const int32_t* actions, const uint8_t* active, void* obs, float* reward, uint8_t* done, float* gt, const mg_info_dev* info,
              int autoreset, hipStream_t s, void* final_frames) override {
        const mg_info_dev ib = begin_step(info);
        prof.begin(0, s);
        // lazy initial segments need the fused launch (its frame workgroups carry the background jobs); any other path
        // first generates what earlier fused steps left owed
        // (per-instance option sets: the plain arrangement -- step kernel, queue server, raster -- whose kernels have a <PS> form)
        // (a headless step, obs == NULL: the plain arrangement as well, without its raster launch; the next drawn step is fused again)
        // (a masked step, active != NULL: the plain arrangement with the MASKED form of the step kernel and the active instances' frames.  What earlier fused
        // steps left owed is flushed first for EVERY instance, the inactive ones included: an owed segment is work put off, and generating it changes no result)
        const bool fused = obs && !active && steps_fused();
        P_.lazy = (fused && lazy_wanted_) ? 1 : 0;
        P_.pre = (P_.lazy && pre_wanted_) ? 1 : 0;
        static const int lazy_append = lab_int("MEMGYM_EMP_LAZY_APPEND", 1);
        P_.lazy_append = (P_.lazy && lazy_append) ? 1 : 0;
        // (a headless step that is being captured flushes whether or not anything is owed NOW: drawn steps may run between the replays)
        if (!P_.lazy && (owed_possible_ || ((!obs || active) && stream_capturing(s)))) flush_owed(s);
        if (P_.lazy) owed_possible_ = true;
        sets_.upload(s);
        const int sb = step_block(256);
        // terminal observations (mg_step, mg_info_buffers.final_obs_dev): the FINAL forms of the two launches leave the terminal frame
        // descriptors in tdesc_, a sparse raster launch behind them draws those frames (round 6; keeps_final_obs)
        const bool keep_final = autoreset && ib.final_obs_dev && fused && keeps_final_obs(s);
        // (three of the four <PS, FINAL> forms exist: terminal observations are kept by handles with one option set only)
        auto step_launch = [&](auto kernel) { launch(kernel, dim3((n_ + sb - 1) / sb), dim3(sb), 0, s, P_, io(), actions, reward, done, gt, ib, autoreset); };
        if (final_frames) {  // terminal frame records (obs == NULL, never fused): the RECORDS forms of the step kernel and of the queue server, whose tdesc is the caller's rows
            MysteryIO rio = io();
            rio.tdesc = (MysteryDesc*)final_frames;
            with_bool(sets_.per_set(), [&](auto PS) {
                with_bool(active != nullptr, [&](auto MASKED) {
                    launch(emp_step_records_kernel<decltype(PS)::value, decltype(MASKED)::value>, dim3((n_ + sb - 1) / sb), dim3(sb), 0, s, P_, rio, actions, active,
                           reward, done, gt, ib, autoreset);
                });
                launch(emp_serve_records_kernel<decltype(PS)::value>, dim3(servers(false)), dim3(256), WS_BYTES, s, P_, rio, reward, done, gt, ib, autoreset);
            });
            plain_frames(obs, s, active);
            return;
        }
        if (active) {
            with_bool(sets_.per_set(), [&](auto PS) {
                launch(emp_step_masked_kernel<decltype(PS)::value>, dim3((n_ + sb - 1) / sb), dim3(sb), 0, s, P_, io(), actions, active, reward, done, gt, ib, autoreset);
            });
        } else if (sets_.per_set()) step_launch(emp_step_kernel<true>);
        else if (keep_final) step_launch(emp_step_kernel<false, true>);
        else step_launch(emp_step_kernel<false>);
        if (!fused) {
            serve(false, nullptr, reward, done, gt, ib, autoreset, s);
            plain_frames(obs, s, active);
            return;
        }
        // the queue is served inside the raster launch
        end_logic(s);
        prof.begin(1, s);
        // (small launches: the owed segments are entries too; with records ahead of time: next to no entries)
        const int svc = P_.bg_coop ? EMP_SVC_WGS_SMALL : (P_.pre ? EMP_SVC_WGS_PRE : EMP_SVC_WGS);
        static const int nt_forced = lab_int("MEMGYM_EMP_NT", -1);
        const bool nt = nt_forced >= 0 ? nt_forced != 0 : !P_.pre;
        int bgw = P_.bg_coop ? 0 : std::min(EMP_BG_WGS, (n_ + EMP_BG_SPAN - 1) / EMP_BG_SPAN);   // background workgroups: EMP_BG_SPAN instances' flags each
        ++turn_;
        // lab: MEMGYM_EMP_BG_SEPARATE=1 runs the background jobs as a launch of their own BEHIND the raster (what they cost it)
        static const int bg_separate = lab_int("MEMGYM_EMP_BG_SEPARATE", 0);
        const int bgw_later = bg_separate ? bgw : 0;
        if (bg_separate) bgw = 0;
        const int grid = frames_grid(n_) + svc + bgw;  // (service, background, frames)
        auto raster_serve = [&](auto kernel, int wgs, int bg) {
            launch(kernel, dim3(wgs), dim3(256), RASTER_LDS, s, desc_.p, atlas_->dev(), obs, n_, P_, io(), reward, done, gt, ib, autoreset, svc, bg, turn_);
        };
        // (format x non-temporal x kept terminal observations: four forms in each of the two one-byte formats; the float formats' stream-out
        // has no non-temporal flavour -- two forms each, EMP_NT = false, whatever `nt` says)
        auto in_format = [&](bool want_nt, bool final, int wgs, int bg) {
            with_obs_format(obs_format, [&](auto F) {
                constexpr int FMT = decltype(F)::value;
                constexpr bool ONE_BYTE = FMT == MG_OBS_U8_XYC || FMT == MG_OBS_U8_CYX;
                with_bool(ONE_BYTE && want_nt, [&](auto NT) {
                    with_bool(final, [&](auto FINAL) {
                        if constexpr (ONE_BYTE || !decltype(NT)::value)
                            raster_serve(emp_raster_serve_kernel<FMT, decltype(NT)::value, decltype(FINAL)::value>, wgs, bg);
                    });
                });
            });
        };
        in_format(nt, keep_final, grid, bgw);
        check_launch();
        ++emp_fused_steps_;
        if (keep_final)  // every finished instance's flag is in `done` by now (the service workgroups wrote the last of them)
            launch_raster_sparse<MysteryComposer>(tdesc_.p, atlas_->dev(), ib.final_obs_dev, obs_format, n_, s, done);
        prof.end(1, s);
        if (bgw_later)  // (grid = service + background workgroups only: no frames; the queue is empty by now)
            in_format(false, false, svc + bgw_later, bgw_later);
#ifdef MG_LAB_EMP_CLOCK  // diagnosis: is the next logic kernel slow because the L2 is full of dirty observation lines?
        static const int wb = lab_int("MEMGYM_LAB_WBL2", 0);
        if (wb) launch(lab_wbl2_kernel, dim3(wb), dim3(64), 0, s);
#endif
    }
    // the step kernel and the service waves of the fused launch leave the terminal frame DESCRIPTORS behind, one sparse raster launch draws them -- lab
    // MEMGYM_EMP_FINAL_FUSED=0: the generic path of mg_step
    bool keeps_final_obs(hipStream_t) override {
        static const bool wanted = lab_flag("MEMGYM_EMP_FINAL_FUSED", true);
        return wanted && steps_fused();
    }

    void ground_truth64(double* out, hipStream_t s, const uint8_t* only = nullptr) override {
        if (!out) return;
        if (only) return launch_checked(mystery_gt64_masked_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, n_, core_.p, out, only);
        launch_checked(mystery_gt64_kernel, dim3((n_ + 255) / 256), dim3(256), 0, s, n_, core_.p, out);
    }
    bool debug_counter(const std::string& name, int64_t* out) override {
        if (name == "emp_fused_steps") {  // step() calls that went out as emp_raster_serve_kernel since the handle was created (host-side count)
            *out = emp_fused_steps_;
            return true;
        }
        if (name == "emp_segments_sum" || name == "emp_segments_max" || name == "emp_falloff_max") {  // a scan of the state records as they stand
            std::vector<MysteryCore> h(n_);
            MG_HIP(hipDeviceSynchronize());
            MG_HIP(hipMemcpy(h.data(), core_.p, sizeof(MysteryCore) * (size_t)n_, hipMemcpyDeviceToHost));
            int64_t sum = 0, mx = 0, fmx = 0;
            for (const MysteryCore& c : h) {  // (segments generated so far; the ones still owed, EMP_OWED, are not counted)
                sum += c.num_seg;
                mx = c.num_seg > mx ? c.num_seg : mx;
                fmx = c.n_falloff > fmx ? c.n_falloff : fmx;
            }
            *out = name == "emp_segments_sum" ? sum : (name == "emp_segments_max" ? mx : fmx);
            return true;
        }
        return MysteryFamily::debug_counter(name, out);
    }
    void on_state_loaded() override {
        seeded_ = true;
        owed_possible_ = true;  // the blob may carry owed segments
    }
    // (as a headless step does: stream-ordered; while capturing whether or not anything is owed NOW -- drawn steps may run between the replays)
    void before_instance_save(hipStream_t s) override {
        if (owed_possible_ || stream_capturing(s)) flush_owed(s);
    }
    void sync_state() override {
        if (owed_possible_) {
            MG_HIP(hipDeviceSynchronize());  // steps in flight on the caller's streams come first
            flush_owed(0);
            MG_HIP(hipDeviceSynchronize());
        }
    }
    // (behind sync_state(): nothing is owed, nothing is in flight.)  A record generated ahead of time continued the OLD stream and carries
    // that stream's state behind the segment: dropped, as the kernels do wherever the stream has moved (EMP_PRE, mg_mystery_endless.hpp)
    void debug_set_rng(int i, const uint64_t in[6]) override {
        Family::debug_set_rng(i, in);
        MysteryCore c;
        MG_HIP(hipMemcpy(&c, core_.p + i, sizeof c, hipMemcpyDeviceToHost));
        EMP_PRE(c) = 0;
        MG_HIP(hipMemcpy(core_.p + i, &c, sizeof c, hipMemcpyHostToDevice));
    }

   private:
    // workgroups (4 waves each) of emp_serve_kernel; MEMGYM_EMP_SERVERS overrides for tuning
    int servers(bool all) const {
        static const int forced = lab_int("MEMGYM_EMP_SERVERS", 0);
        const int want = forced > 0 ? forced : (all ? 1024 : 512);  // measured: profiles/r01e_logic_tails.md section 4
        const int cap = (n_ + 3) / 4;
        return want < cap ? want : cap;
    }
    // the queue server as a launch of its own: `all` = every instance (a full reset), else the queued ones
    void serve(bool all, const int64_t* seeds, float* reward, uint8_t* done, float* gt, const mg_info_dev& ib, int autoreset, hipStream_t s) {
        with_bool(sets_.per_set(), [&](auto PS) {
            launch(emp_serve_kernel<decltype(PS)::value>, dim3(servers(all)), dim3(256), WS_BYTES, s, P_, io(), seeds, all ? 1 : 0, reward, done, gt, ib, autoreset);
        });
    }
    // MEMGYM_EMP_FUSE=0: separate queue-server launch in front of the raster (the round-1 arrangement)
    bool fuse_serve() const {
        static const bool on = lab_flag("MEMGYM_EMP_FUSE", true);
        return on;
    }
    // This handle steps in the fused arrangement: emp_step_kernel + emp_raster_serve_kernel in the handle's format.  What comes with it comes
    // together or not at all: lazy initial segments, records ahead of time (EMP_PRE), the fast masked reset (emp_masked_reset_kernel), terminal
    // observations kept by the step's own launches (keeps_final_obs).  Per-instance option sets and BIG agent sprites keep the plain
    // arrangement (step kernel, queue server, raster), whose kernels have the <PS> forms and the BIG composer.
    // No observation format is excluded, and that is a measured choice (profiles/emp_chw.md; the parent's plain arrangement against the fused
    // one, A/B/A/B on one box, us per step at 32,768 / 16,384 instances under random actions, auto-reset leg): u8_chw 232-233 -> 153-155 /
    // 158-159 -> 102-103, bf16_chw 322-323 -> 237-239 / 218-223 -> 174-175, f16_chw like bf16_chw, f32_chw 531 -> 444 / 328-329 -> 289-296; with
    // terminal observations kept and under a path-following policy the gain is larger still.  The image-order forms need 16-48 B more scratch per
    // lane than their u8_xyc siblings (736-784 B against 736-752 B) at the same 80 VGPRs and six workgroups per CU.  The lab build's
    // MEMGYM_EMP_FUSE=0 puts a handle of any format on the plain arrangement.
    bool steps_fused() const { return fuse_serve() && !sets_.per_set() && !big_sprites_; }
    // MEMGYM_EMP_RESET_LANES=0: a full reset through the queue server, one wave per instance (round 1)
    bool reset_by_lanes() const {
        static const bool on = lab_flag("MEMGYM_EMP_RESET_LANES", true);
        return on;
    }
    void flush_owed(hipStream_t s) {
        launch_checked(emp_flush_owed_kernel, dim3((n_ + 63) / 64), dim3(64), LW_BYTES, s, P_, io());
        owed_possible_ = false;
    }
    // show_background: draw_column_tile_surface / draw_icy_surface (pygame_assets.py:780-817) blitted every `tile`
    // pixels from x = bg_scroll - tile on (endless_mystery_path.py:141-143) = one template per scroll phase
    void add_templates(Atlas& atlas) override {
        const uint8_t ice[3] = {125, 177, 250}, edge[3] = {210, 210, 210};
        std::vector<uint8_t> t((size_t)P_.tile * FRAME_BYTES);
        for (int ph = 0; ph < P_.tile; ++ph)
            for (int x = 0; x < SCREEN; ++x)
                for (int y = 0; y < SCREEN; ++y) {
                    const int u = (x + ph) % P_.tile, w = y % P_.tile;
                    const bool on_edge = u == 0 || w == 0 || u == P_.tile - 1 || w == P_.tile - 1;
                    for (int c = 0; c < 3; ++c) t[(size_t)ph * FRAME_BYTES + ((size_t)x * SCREEN + y) * 3 + c] = on_edge ? edge[c] : ice[c];
                }
        atlas.set_templates(t);
    }
    MysteryIO io() override {
        MysteryIO o = shared_io();
        o.seg_rows = seg_rows_;
        o.bgq = bgq_.p;
        o.bgflag = bgflag_.p;
        return o;
    }

    int seg_rows_ = MAX_SEG;    // records of segs_ per instance (set_capacity)
    DevArray<int> bgq_;         // background jobs (owed segments), small launches
    DevArray<uint8_t> bgflag_;  // ... larger launches: one flag per instance
    bool lazy_wanted_ = false, owed_possible_ = false, pre_wanted_ = false;
    int turn_ = 0;  // fused launches so far (where a background workgroup enters an over-long job list)
    int64_t emp_fused_steps_ = 0;  // debug_counter("emp_fused_steps")
};

// variant: 0 MysteryPath-v0, 1 Endless-MysteryPath-v0, 2 MysteryPath-Grid-v0
Family* make_mystery(int variant, int num_envs) {
    if (variant == 1) return new MysteryEndlessFamily(num_envs);
    return new MysteryFiniteFamily(variant, num_envs);
}

}  // namespace mg

#ifdef MG_LAB_EMP_CLOCK
extern "C" int mg_lab_step_clock(unsigned long long* host, int n_waves) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(mg::g_lab_step_clock), sizeof(unsigned long long) * 12 * (size_t)n_waves) == hipSuccess ? 0 : -1;
}
extern "C" int mg_lab_emp_clock(unsigned long long* host, int n_wgs) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(mg::g_lab_emp_clock), sizeof(unsigned long long) * 3 * (size_t)n_wgs) == hipSuccess ? 0 : -1;
}
#endif
