// mg_spot_logic.hpp -- Searing Spotlights family (included by mg_spot.hip only): reset and step of ONE instance as its 16 lanes execute them.  Spotlight creation (new_spot;
// new_spots_at_reset with the 16-outputs-at-once PCG64 jump), the descriptor pieces both share (coin words, top bar, ground truth, stale holes, the leader's store of the descriptor head),
// spot_reset, the measurement hooks of the clock build (SPOT_CLOCK*, MG_LAB_SPOT_CLOCK) and spot_step_body.  The kernels that run them: mg_spot_serve.hpp.
#pragma once
#include "mg_spot_types.hpp"
#include "mg_spot_sampler.hpp"

namespace mg {
__device__ __forceinline__ void clamp_spawn(const SpotParams& P, int& x, int& y) {
    int off = P.spawn_clamp;
    if (x < off) x = off; else if (x > SCREEN - off) x = SCREEN - off;
    if (y < off) y = off; else if (y > SCREEN - off) y = SCREEN - off;
}

// Spotlight.__init__: 5 draws (radius, speed, start angle, target delta, offset delta)
// `ls` = this lane's slot id: every lane of the instance draws the same numbers, the owner of the chosen slot stores them
// The record of a spotlight as the lane owning its slot holds it in registers.
struct SlotRec {
    double t, speed;
    uint32_t ang;  // start | target << 9 | offset << 18 (degrees, % 360)
    int r;         // bit 7: has_border
};
__device__ __forceinline__ uint32_t pack_angles(int start, int target, int offset) {
    return (uint32_t)(start % 360) | ((uint32_t)(target % 360) << 9) | ((uint32_t)(offset % 360) << 18);
}
// cos / sin of integer degrees (host-built tables in global memory, see SpotFamily)
struct Trig {
    const double* c;
    const double* s;
};
// Spotlight.__init__: 5 draws (radius, speed, start angle, target delta, offset delta).  `ls` = this lane's slot id: every lane of
// the instance draws the same numbers; the lane owning the slot the free mask hands out stores the record AND gets it back in
// `rec` (reading it back from memory is two round trips in every wave in which any instance spawned, i.e. in every launch).
// Returns false when all SLOTS slots are taken (the reference's list is unbounded, endless_searing_spotlights.py:191): the draws are
// consumed, no spotlight is added, error bit 1 is raised -- and the step that called ends the episode (mg_info_buffers.capacity_dev).
__device__ __forceinline__ bool new_spot(const SpotParams& P, const SpotIO& io, int i, int ls, SpotCore& s, Pcg& g, SlotRec* rec = nullptr) {
    int radius = g.integers(P.r_lo, P.r_hi);
    double speed = g.uniform(P.speed_lo, P.speed_hi);
    int start = g.integers(0, 360);
    int target = start + 180 + g.integers(-45, 45);
    int offset = target + g.integers(-135, 135);
    if (s.n_spots >= SLOTS || s.free_mask == 0) {
        raise_error(io.err, 1);
        return false;
    }
    int slot = __ffs(s.free_mask) - 1;
    s.free_mask &= ~(1u << slot);
    s.order |= (uint64_t)slot << (4 * s.n_spots);
    s.n_spots++;
    if (slot != ls) return true;
    size_t k = (size_t)i * SLOTS + slot;
    SlotRec n;
    n.r = radius | (P.black_background ? 0x80 : 0);  // bit 7: Spotlight.has_border
    n.t = 0.0;
    n.speed = speed;
    n.ang = pack_angles(start, target, offset);
    io.sp_r[k] = (uint8_t)n.r;
    io.sp_t[k] = n.t;
    io.sp_speed[k] = n.speed;
    io.sp_ang[k] = n.ang;
    if (rec) *rec = n;
    return true;
}

// The spotlights a reset starts with (free_mask == 0xFFFF: the q-th takes slot q, which lane q owns): 5 draws each, one after another
// in the generator's stream -- 20 of the ~27 draws of a reset, ~3 of the ~4 us by which a resetting instance's wave outlasts the
// others (profiles/r04_spot_step.md).  The stream's NEXT 16 outputs do not have to be produced one after another: PCG64's state
// after k steps is A^k s + S_k inc (S_k = 1 + A + ... + A^(k-1)), so lane j of the instance's 16 computes output j + 1 directly
// (two 128-bit multiplications with its pair of constants, P.jump) and lane q < count picks the three outputs spotlight q
// consumes.  Which halves feed which draw depends on whether the stream arrives with a buffered half (numpy's next_uint32 hands
// out the low half of a fresh 64-bit output and keeps the high half; Generator.uniform takes a fresh output and leaves the
// buffer alone):   buffered:  radius <- the buffered half (spotlight 0: the stream's own; q > 0: the high half of output 3q),
//                             speed <- output 3q+1, start <- low(3q+2), target <- high(3q+2), offset <- low(3q+3);
//                  otherwise: radius <- low(3q+1), speed <- output 3q+2, start <- high(3q+1), target <- low(3q+3), offset <- high(3q+3).
// Either way a spotlight consumes three outputs, the stream ends with the same "buffered" flag it came with, and the buffer word holds
// the high half of output 3 count (numpy keeps a used half in place).  This holds as long as no bounded draw is rejected (Lemire:
// possible only when the low word of the product is below the range, ~1e-7 per draw): a lane that sees such a low word makes the
// whole group fall back to the one-after-another form below from the untouched stream -- that form is the definition.
// Returns false if it did nothing (the caller then runs the loop over new_spot()).
__device__ __forceinline__ bool new_spots_at_reset(const SpotParams& P, const SpotIO& io, int i, const LaneCtx& L, SpotCore& s, Pcg& g, int count,
                                                   const uint4 jm, const uint4 jq) {
    const uint32_t n_r = (uint32_t)(P.r_hi - P.r_lo);
    if (count < 1 || count > 5 || n_r < 2u) return false;  // (16 outputs = 5 spotlights; a one-value radius range draws nothing)
    const int ls = L.ls;
    const u128 M = ((u128)jm.w << 96) | ((u128)jm.z << 64) | ((u128)jm.y << 32) | jm.x;
    const u128 S = ((u128)jq.w << 96) | ((u128)jq.z << 64) | ((u128)jq.y << 32) | jq.x;
    const u128 st = M * g.state + S * g.inc;  // the state after ls + 1 steps
    uint32_t lo, hi;
    {
        const uint64_t h = (uint64_t)(st >> 64), l = (uint64_t)st, x = h ^ l;
        const unsigned rot = (unsigned)(h >> 58);
        const uint64_t o = (x >> rot) | (x << ((64 - rot) & 63));
        lo = (uint32_t)o;
        hi = (uint32_t)(o >> 32);
    }
    const int q = ls < count ? ls : 0;  // this lane's spotlight (lanes >= count follow spotlight 0 and store nothing)
    const uint32_t lo1 = __shfl(lo, 3 * q, 16), hi1 = __shfl(hi, 3 * q, 16);
    const uint32_t lo2 = __shfl(lo, 3 * q + 1, 16), hi2 = __shfl(hi, 3 * q + 1, 16);
    const uint32_t lo3 = __shfl(lo, 3 * q + 2, 16), hi3 = __shfl(hi, 3 * q + 2, 16);
    const uint32_t hi0 = __shfl(hi, q > 0 ? 3 * q - 1 : 0, 16);
    const bool buffered = g.has;
    const uint32_t x_radius = buffered ? (q > 0 ? hi0 : g.buf) : lo1;
    const uint64_t x_speed = buffered ? (((uint64_t)hi1 << 32) | lo1) : (((uint64_t)hi2 << 32) | lo2);
    const uint32_t x_start = buffered ? lo2 : hi1;
    const uint32_t x_target = buffered ? hi2 : lo3;
    const uint32_t x_offset = buffered ? lo3 : hi3;
    const uint64_t m_radius = (uint64_t)x_radius * n_r, m_start = (uint64_t)x_start * 360u, m_target = (uint64_t)x_target * 90u,
                   m_offset = (uint64_t)x_offset * 270u;
    const bool maybe_rejected = (uint32_t)m_radius < n_r || (uint32_t)m_start < 360u || (uint32_t)m_target < 90u || (uint32_t)m_offset < 270u ||
                                (P.lab_fallback > 0 && i % P.lab_fallback == 0);
    if (((uint32_t)(__ballot(maybe_rejected) >> L.gshift) & 0xFFFFu) != 0u) return false;
    // the stream after 3 count outputs (all 16 lanes hold the same copy)
    {
        const int last = 3 * count - 1;
        const uint32_t a = __shfl((uint32_t)st, last, 16), b = __shfl((uint32_t)(st >> 32), last, 16);
        const uint32_t c = __shfl((uint32_t)(st >> 64), last, 16), d = __shfl((uint32_t)(st >> 96), last, 16);
        g.state = ((u128)d << 96) | ((u128)c << 64) | ((u128)b << 32) | a;
        g.buf = __shfl(hi, last, 16);
    }
    s.n_spots = (uint8_t)count;
    s.free_mask = 0xFFFFu & ~((1u << count) - 1u);
    s.order = 0x43210ull & ((1ull << (4 * count)) - 1ull);
    if (ls < count) {  // Spotlight.__init__ of spotlight ls, as in new_spot()
        const int radius = P.r_lo + (int)(m_radius >> 32);
        const double speed = P.speed_lo + (P.speed_hi - P.speed_lo) * ((double)(x_speed >> 11) * (1.0 / 9007199254740992.0));
        const int start = (int)(m_start >> 32);
        const int target = start + 180 + (-45 + (int)(m_target >> 32));
        const int offset = target + (-135 + (int)(m_offset >> 32));
        const size_t k = (size_t)i * SLOTS + ls;
        io.sp_r[k] = (uint8_t)(radius | (P.black_background ? 0x80 : 0));
        io.sp_t[k] = 0.0;
        io.sp_speed[k] = speed;
        io.sp_ang[k] = pack_angles(start, target, offset);
    }
    return true;
}

// A coin as the descriptor holds it (SpotDesc::coins, read back by SpotView::coin_x / coin_y): the top-left of its stamp, biased by 128, from its centre
__device__ __forceinline__ uint32_t coin_word(const SpotParams& P, int cx, int cy) {
    return (uint32_t)(cx - P.coin_radius + 128) | ((uint32_t)(cy - P.coin_radius + 128) << 16);
}
// info["ground_truth"]: agent and coin position / screen size (endless_searing_spotlights.py:407,496), as float32 or float64
template <class T>
__device__ __forceinline__ void write_gt(T* out, const SpotParams& P, int ax, int ay, const SpotCore& s) {
    out[0] = (T)((double)ax / SCREEN);
    out[1] = (T)((double)ay / SCREEN);
    out[2] = (T)(P.coin_enabled ? (double)s.coin_x / SCREEN : 0.0);
    out[3] = (T)(P.coin_enabled ? (double)s.coin_y / SCREEN : 0.0);
}
// n_holes of the frame drawn last, from its descriptor in memory (spot_reset's stale_holes)
__device__ __forceinline__ int frame_holes(const SpotDesc* d) { return (int)(reinterpret_cast<const uint32_t*>(d)[2] & 0xFFu); }

template <bool EN>
__device__ __forceinline__ void fill_topbar(const SpotParams& P, const SpotCore& s, SpotDesc& d, bool reset_frame, int a0, int a1) {
    d.c_base = EN ? C_BLACK : C_GREY50;
    d.red_w = s.red_w;
    d.quarter = (uint8_t)P.quarter;
    d.c_act0 = d.c_act1 = 0xFF;
    if (P.show_last_action) {  // 0 -> grey, 1 -> purple, 2 -> orange
        d.c_act0 = a0 == 0 ? C_GREY120 : (a0 == 1 ? C_PURPLE : C_ACT_ORANGE);
        d.c_act1 = a1 == 0 ? C_GREY120 : (a1 == 1 ? C_PURPLE : C_ACT_ORANGE);
    }
    d.c_bar = 0xFF;
    d.bar_x = (uint8_t)P.bar_x;
    d.bar_w = (uint8_t)P.bar_w;
    if (!reset_frame && P.show_last_positive_reward) d.c_bar = s.last_pos ? C_YELLOW : C_GREY50;
}

// ENDLESS is a compile-time flag: the endless instantiation has no run-time indexed local arrays (coin lists), so the
// descriptor and the state stay in registers -- with both variants in one kernel they lived in 176 B of scratch per lane.
// stale_holes: the spotlight surface is NOT repainted by reset() (searing_spotlights.py:394-397 only set its alpha), so
// the first frame of an episode shows the holes of the last frame drawn before it; they only show when the alpha is not
// 0 at reset, i.e. with light_dim_off_duration == 0.  The hole words themselves are still in the descriptor.
template <bool EN>
__device__ __forceinline__ void spot_reset(const SpotParams& P, const SpotIO& io, int i, const LaneCtx& L, SpotCore& s, Pcg& g, SpotDesc& d, float* gt,
                                           int stale_holes, int* slot) {  // slot: disc_slot() of the calling kernel's LDS array
    const int ls = L.ls;
    const uint4 jm = P.jump[2 * ls], jq = P.jump[2 * ls + 1];  // (new_spots_at_reset: requested here, used after the first draws)
    s.t = 0;
    s.coin_t = 0;
    s.ep_sum = 0.0;
    s.ep_len = 0;
    s.la0 = s.la1 = 0;
    s.rot8 = (uint8_t)g.integers(0, 8);  // choice([0, 45, ..., 315])
    Discs D;
    D.p = slot;
    D.n = 0;
    int ax, ay;
    if (P.sample_agent_position) {
        int k = g.integers(0, SCREEN * SCREEN);  // sampler with an empty mask: cell k itself
        int cy = k / SCREEN, cx = k - cy * SCREEN;
        D.push(cx, cy, 28);
        ax = cx + g.integers(2, 4);
        ay = cy + g.integers(2, 4);
    } else {
        ax = SCREEN / 2;
        ay = SCREEN / 2;
        D.push(ax, ay, 21);
    }
    s.ax = (int16_t)ax;
    s.ay = (int16_t)ay;
    s.health = P.agent_health;
    s.red_w = 0;
    s.last_pos = 0;
    s.alpha = (uint8_t)(P.dim_duration > 0 ? 0 : (P.light_threshold > 255 ? 255 : (P.light_threshold < 0 ? 0 : P.light_threshold)));
    s.n_spots = 0;
    s.order = 0;
    s.free_mask = 0xFFFFu;
    s.spawn_timer = 0;
    s.n_intervals = (uint8_t)P.num_spawns;
    if (!new_spots_at_reset(P, io, i, L, s, g, P.initial_spawns, jm, jq))
        for (int k = 0; k < P.initial_spawns; ++k) new_spot(P, io, i, ls, s, g);
    s.coins_collected = 0;
    s.n_coins = 0;
    s.has_coin = 0;
    uint32_t* coins = io.coins + (size_t)i * MAX_COINS;
    int* const coin_pos = slot + 3 * MAX_DISCS;  // the coins as placed (finite variant), next to the disc list
    if constexpr (EN) {
        if (P.coin_enabled) {  // _spawn_coin: the sampler is reset first, self.coin is None -> nothing blocked
            int k = g.integers(0, SCREEN * SCREEN);
            int cy = k / SCREEN, cx = k - cy * SCREEN;
            cx += g.integers(2, 4);
            cy += g.integers(2, 4);
            clamp_spawn(P, cx, cy);
            s.coin_x = (int16_t)cx;
            s.coin_y = (int16_t)cy;
            s.has_coin = 1;
            s.n_coins = 1;
        }
    } else {
        int nc = P.num_coins.n > 0 ? choice(g, P.num_coins) : 0;
        s.num_coins = nc;
        for (int k = 0; k < nc && k < MAX_COINS; ++k) {  // deliberately not unrolled (code size)
            int cx, cy;
            sample_cell(g, D, L, &cx, &cy);
            D.push(cx, cy, 21);
            cx += g.integers(2, 4);
            cy += g.integers(2, 4);
            clamp_spawn(P, cx, cy);
            const uint32_t w = (uint32_t)(cx & 0xFFFF) | ((uint32_t)cy << 16);
            if (ls == 0) coins[k] = w;
            coin_pos[k] = (int)w;
            s.n_coins++;
        }
        if (P.use_exit) {  // _spawn_exit (searing_spotlights.py:280-286)
            int ex, ey;
            sample_cell(g, D, L, &ex, &ey);
            ex += g.integers(2, 4);
            ey += g.integers(2, 4);
            clamp_spawn(P, ex, ey);
            s.exit_x = (int16_t)ex;
            s.exit_y = (int16_t)ey;
            s.exit_open = 0;
            s.pad = (s.pad & ~PAD_EXIT_GEN_MASK) | ((uint32_t)P.exit_gen << PAD_EXIT_GEN_SHIFT) | PAD_HAS_EXIT;
        } else if (!(s.pad & PAD_HAS_EXIT)) {
            // use_exit == False: nothing is spawned, sampled or drawn (:413-416) and the frame keeps blitting self.exit -- the Exit
            // of an earlier episode, where it was and as it was last drawn (open / closed).  Without one the reference raises
            // AttributeError at this reset (:431-435); here the bit is raised and no exit is drawn.
            raise_error(io.err, ERR_NO_EXIT);
        }
    }
    s.bg_red = 0;
    if (P.hide_chessboard) s.pad = bg_set(bg_set(s.pad, 0, BG_WHITE), 1, BG_WHITE);  // (the reference does this first thing: no draw depends on it)
    if (P.black_background) s.pad = bg_set(s.pad, 0, BG_BLACK);

    // reset frame: blue board, sprite index 0 (not the sampled rotation), dark layer at the reset alpha with the hole
    // pattern the previous frame left, coin(s) shown above the dark layer while coin_t < coin_show_duration
    memset(&d, 0, sizeof(d));
    d.valid = 1;
    d.bg = bg_template(s.pad, 0);
    d.sprite = 0;
    d.sx = (int16_t)(ax - P.sprite_half);
    d.sy = (int16_t)(ay - P.sprite_half);
    d.alpha = s.alpha;
    d.n_holes = (uint8_t)stale_holes;
    d.exit_stamp = 0xFF;
    if constexpr (EN) {
        d.n_coins = s.n_coins;
        d.coin_above = (uint8_t)(((P.coins_visible || s.coin_t < P.coin_show_duration) ? LAYER_COIN_ABOVE : 0) | P.layer_flags);
        d.coins[0] = coin_word(P, s.coin_x, s.coin_y);
    } else {
        d.n_coins = s.n_coins;
        d.coin_above = (uint8_t)((P.coins_visible ? LAYER_COIN_ABOVE : 0) | P.layer_flags);
#pragma unroll
        for (int k = 0; k < MAX_COINS; ++k) {
            if (k < s.n_coins) {
                const uint32_t w = (uint32_t)coin_pos[k];
                int cx = (int)(int16_t)(w & 0xFFFF), cy = (int)(w >> 16);
                d.coins[k] = coin_word(P, cx, cy);
            }
        }
        {
            const int eg = exit_gen_of(s.pad), half = (int)((P.exit_halves >> (8 * eg)) & 0xFFu);
            d.exit_stamp = (s.pad & PAD_HAS_EXIT) ? (uint8_t)(ST_EXIT0 + 2 * eg + (s.exit_open ? 1 : 0)) : 0xFF;
            d.exit_x = (int16_t)(s.exit_x - half);
            d.exit_y = (int16_t)(s.exit_y - half);
        }
    }
    fill_topbar<EN>(P, s, d, true, 0, 0);
    if (gt) write_gt(gt, P, ax, ay, s);
}

// the leader stores the descriptor's header + coin positions (words 0..5 and 8..15); hole words are written by the slot
// lanes.  Packed field by field (the layout of the bit-fields above) so that `d` never has to exist in memory.
__device__ __forceinline__ void store_desc_head(SpotDesc* dst, const SpotDesc& d) {
    uint4* out = reinterpret_cast<uint4*>(dst);
    const uint32_t w0 = (uint32_t)d.valid | ((uint32_t)d.bg << 8) | ((uint32_t)d.sprite << 16) | ((uint32_t)d.alpha << 24);
    const uint32_t w1 = ((uint32_t)d.sx & 0xFFFFu) | ((uint32_t)d.sy << 16);
    const uint32_t w2 = (uint32_t)d.n_holes | ((uint32_t)d.n_coins << 8) | ((uint32_t)d.coin_above << 16) | ((uint32_t)d.red_w << 24);
    const uint32_t w3 = (uint32_t)d.c_base | ((uint32_t)d.c_act0 << 8) | ((uint32_t)d.c_act1 << 16) | ((uint32_t)d.c_bar << 24);
    const uint32_t w4 = (uint32_t)d.bar_x | ((uint32_t)d.bar_w << 8) | ((uint32_t)d.quarter << 16) | ((uint32_t)d.exit_stamp << 24);
    const uint32_t w5 = ((uint32_t)d.exit_x & 0xFFFFu) | ((uint32_t)d.exit_y << 16);
    out[0] = make_uint4(w0, w1, w2, w3);
    reinterpret_cast<uint2*>(dst)[2] = make_uint2(w4, w5);
    out[2] = make_uint4(d.coins[0], d.coins[1], d.coins[2], d.coins[3]);
    out[3] = make_uint4(d.coins[4], d.coins[5], d.coins[6], d.coins[7]);
}
static_assert(MAX_COINS == 8, "store_desc_head packs eight coin words");

// The step of instance i as its 16 lanes execute it (lane ls owns spotlight slot ls).  The launch lasts as long as its slowest wave
// (all waves of a 16,384-instance launch are resident at once): every load the step can need is requested up front -- core record,
// generator stream, the lane's 17-byte slot record -- and the rare paths (spawn, coin re-sampling, reset) are kept short
// (profiles/r04_spot_step.md: 20.5 -> 14 us).  The core record lives in LDS (round 4: 123 -> 69-88 VGPRs).
#ifdef MG_LAB_SPOT_CLOCK  // measurement builds only (tools/spot_step_timeline.py): eight stamps + flags per wave of the step kernel
static __device__ unsigned long long g_lab_spot_clock[10 * 65536];
#define SPOT_CLOCK(slot) do { clk[slot] = (unsigned long long)clock64(); } while (0)
#define SPOT_CLOCK_AFTER(slot, ...) do { asm volatile("" ::__VA_ARGS__); SPOT_CLOCK(slot); } while (0)  // the stamp behind the values named ("v"(x), ...)
#define SPOT_CLOCK_FLAG(f) do { f = true; } while (0)                                                    // this wave took a rare path
#else
#define SPOT_CLOCK(slot) do { } while (0)
#define SPOT_CLOCK_AFTER(slot, ...) do { } while (0)
#define SPOT_CLOCK_FLAG(f) do { } while (0)
#endif
// RECORDS (mg_info_buffers.final_frames_dev; the step kernels proper, never deferred): the 16 lanes of an instance that finishes keep the descriptor of its TERMINAL
// frame in final_frames[i], composed BEFORE the in-kernel reset touches the state.  The row is written word for word as io.desc[i] stands after the same step
// without a reset (what mg_save_frames would store): the head by the leader (store_desc_head and the two unused words), the hole words by the slot lanes -- hole
// `rank` by the lane that has just computed it, the words behind this step's n_holes (stale holes of earlier frames; the composers do not read them) by lanes
// n_holes .. 15 from a load issued with the step's other loads.  The 16 + 4 stores of a group go to disjoint words of one 128-byte line: nothing orders them.
template <bool EN, bool PS, bool RECORDS = false>
__device__ __forceinline__ void spot_step_body(int i, const LaneCtx& L, const SpotStepArgs& a, int* disc_lds, SpotCore* core_lds, const Trig& T,
                                               SpotDesc* final_frames = nullptr) {
    const int ls = L.ls;
#ifdef MG_LAB_SPOT_CLOCK
    unsigned long long clk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long wall0 = wall_clock64();
    bool f_spawn = false, f_coin = false;
#endif
    SPOT_CLOCK(0);
    const SpotIO& io = a.io;
    const SpotParams& P = PS ? io.sets[set_index(io.set_of, i)] : a.P;  // (PS: per-instance option sets)
    const int32_t* const actions = a.actions;
    float* const reward_out = a.reward_out;
    uint8_t* const done_out = a.done_out;
    float* const gt = a.gt;
    const mg_info_dev& info = a.info;
    const int autoreset = a.autoreset, defer = a.defer;
    const int group_shift = L.gshift;  // bit position of this instance's 16 lanes in a wave ballot
    const bool leader = ls == 0;
    // The instance's core record lives in LDS for the length of the step (its 16 lanes write the same values to the same words):
    // twenty registers less at every point of a kernel that has to share its register budget with the raster (round 4:
    // 89 -> 65-73 VGPRs for this body), for a handful of LDS round trips on its critical path.
    SpotCore& s = core_lds[L.grp];
    s = io.core[i];
    // Everything the step may need is requested HERE, together: the generator's stream (spawns, coin re-sampling and resets are
    // rare, but each used to start with a memory round trip of its own, and a wave with two of them is what the launch waits
    // for) and this lane's slot record (16 bytes + a byte now).  Timeline per wave: profiles/r04_spot_step.md.
    Pcg g;
    g.load(io.rng, i);
    bool rng_used = false;  // (all 16 lanes of the instance take the same branches: they hold the same state)
    uint32_t* coins = io.coins + (size_t)i * MAX_COINS;
    const size_t k = (size_t)i * SLOTS + ls;  // lane ls looks after slot ls
    SlotRec mine;
    mine.t = io.sp_t[k];
    mine.speed = io.sp_speed[k];
    mine.ang = io.sp_ang[k];
    mine.r = io.sp_r[k];
    uint32_t rec_stale = 0u, rec_hole = 0u;
    int rec_rank = -1;
    if constexpr (RECORDS) rec_stale = io.desc[i].holes[ls];
    g.pin();

    // CharacterController.step(action, walkable_rect = (0, 4, 84, 80))
    int a0 = actions[2 * i], a1 = actions[2 * i + 1];
    int ax = s.ax, ay = s.ay;
    free_move(a0, a1, P.v_axis_i, P.v_diag_i, ax, ay, s.rot8, true, P.agent_radius, SCREEN - P.agent_radius, P.bar_h + P.agent_radius,
              SCREEN - P.agent_radius);
    s.ax = (int16_t)ax;
    s.ay = (int16_t)ay;
    SPOT_CLOCK_AFTER(1, "v"(ax), "v"(ay));
    // the top bar shows the PREVIOUS action
    int shown0 = s.la0, shown1 = s.la1;
    if (EN || P.show_last_action) {
        s.la0 = (uint8_t)a0;
        s.la1 = (uint8_t)a1;
    }
    // dim the light until off
    if ((int)s.alpha <= P.light_threshold) {
        int a = P.dim_duration > 0 ? (int)s.alpha + P.dim_step : P.light_threshold;
        s.alpha = (uint8_t)(a > 255 ? 255 : (a < 0 ? 0 : a));  // Surface.set_alpha clamps
    }

    SpotDesc d;
    memset(&d, 0, sizeof(d));
    d.valid = 1;

    // ---- spotlight task ----
    double reward = 0.0, r = 0.0;
    bool spot_done = false, cap = false;  // cap: a spotlight was due and all slots are taken -- this step ends the episode (new_spot)
    s.spawn_timer++;
    if constexpr (EN) {
        if (__builtin_expect(s.spawn_timer >= P.spawn_interval, 0)) {
            SPOT_CLOCK_FLAG(f_spawn);
            rng_used = true;
            cap = !new_spot(P, io, i, ls, s, g, &mine);
            s.spawn_timer = 0;
        }
    } else if (s.n_intervals > 0) {
        if (__builtin_expect(s.spawn_timer >= P.interval0, 0)) {
            rng_used = true;
            cap = !new_spot(P, io, i, ls, s, g, &mine);
            s.n_intervals--;
            s.spawn_timer = 0;
        }
    }
    SPOT_CLOCK(2);
    const int p_r = mine.r;  // bit 7: has_border
    const bool p_done = mine.t >= 1.0;
    const bool used = !((s.free_mask >> ls) & 1u);
    const bool my_done = used && p_done;
    const uint32_t done_mask = (uint32_t)(__ballot(my_done) >> group_shift) & 0xFFFFu;
    // `for spot in self.spotlights: if spot.done: self.spotlights.remove(spot) else: draw + hit test`:
    // removing while iterating skips the element that follows a removed one (it stays in the list untouched)
    uint32_t processed = 0;
    {
        uint64_t new_order = 0;
        int n_new = 0, n_old = s.n_spots;
        for (int pos = 0; pos < n_old;) {
            int slot = (int)((s.order >> (4 * pos)) & 15u);
            if ((done_mask >> slot) & 1u) {
                s.free_mask |= 1u << slot;
                if (pos + 1 < n_old) {
                    int nxt = (int)((s.order >> (4 * (pos + 1))) & 15u);
                    new_order |= (uint64_t)nxt << (4 * n_new++);
                }
                pos += 2;
            } else {
                processed |= 1u << slot;
                new_order |= (uint64_t)slot << (4 * n_new++);
                pos += 1;
            }
        }
        s.order = new_order;
        s.n_spots = (uint8_t)n_new;
    }
    bool my_hit = false;
    if ((processed >> ls) & 1u) {
        const int radius0 = p_r & 127;
        const double R = P.half_diag + (double)radius0, c = SCREEN / 2;  // Spotlight.__init__'s end points (see SpotIO)
        const int a_s = (int)(mine.ang & 511u), a_t = (int)((mine.ang >> 9) & 511u), a_o = (int)(mine.ang >> 18);
        const double p_sx = c + T.c[a_s] * R, p_sy = c + T.s[a_s] * R, p_tx = c + T.c[a_t] * R, p_ty = c + T.s[a_t] * R;
        const double p_ox = c + T.c[a_o] * R, p_oy = c + T.s[a_o] * R;
        double t = mine.t;
        double lx = p_tx * (1 - t) + p_ox * t, ly = p_ty * (1 - t) + p_oy * t;
        double cx = p_sx * (1 - t) + lx * t, cy = p_sy * (1 - t) + ly * t;
        const int radius = p_r & 127;
        int rank = __popc(processed & ((1u << ls) - 1u));
        if (P.ordered_holes) {  // a border is drawn over the discs before it and under the discs after it: list order
            rank = 0;
            for (int pos = 0; pos < (int)s.n_spots; ++pos) {
                const int slot = (int)((s.order >> (4 * pos)) & 15u);
                if (slot == ls) break;
                rank += (int)((processed >> slot) & 1u);
            }
        }
        io.desc[i].holes[rank] = pack_hole((int)cx, (int)cy, radius) | ((uint32_t)(p_r >> 7) << 31);
        if constexpr (RECORDS) {
            rec_hole = pack_hole((int)cx, (int)cy, radius) | ((uint32_t)(p_r >> 7) << 31);
            rec_rank = rank;
        }
        t += mine.speed;
        if (t >= 1.0) t = 1.0;  // = done: removed from the list by the next step
        io.sp_t[k] = t;
        double ddx = (double)ax - cx, ddy = (double)ay - cy;
        my_hit = sqrt(ddx * ddx + ddy * ddy) <= (double)(radius + P.agent_radius);
    }
    const int hit = __popc((uint32_t)(__ballot(my_hit) >> group_shift) & 0xFFFFu);
    const int nh = __popc(processed);
    SPOT_CLOCK_AFTER(3, "v"(hit));
    if (hit > 0) {
        s.health -= P.damage;
        r += P.r_inside;
        s.red_w = (uint8_t)(int)((SCREEN / 2) * (1 - s.health / P.agent_health));
        s.bg_red = P.visual_feedback ? 1 : 0;
    } else {
        s.bg_red = 0;
        r += P.r_outside;
    }
    if (P.black_background) s.pad = bg_set(s.pad, s.bg_red, BG_BLACK);  // bg.fill(0): that surface stays black
    if (s.health <= 0) {
        spot_done = true;
        r += P.r_death;
    }
    reward += r;

    // ---- coin / exit tasks ----
    bool done = false;
    int success = 0;
    uint32_t coin_pos[MAX_COINS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (EN) {
        if (P.coin_enabled) {
            double cr = 0.0;
            if (__builtin_expect(within(ax - (int)s.coin_x, ay - (int)s.coin_y, P.coin_radius + P.agent_radius), 0)) {
                cr += P.r_coin;
                s.coins_collected++;
                s.coin_t = 0;
                // _spawn_coin: sampler reset, previous coin blocked with r = 28
                SPOT_CLOCK_FLAG(f_coin);
                rng_used = true;
                Discs D;
                D.p = disc_slot(disc_lds, L.grp);
                D.n = 0;
                D.push(s.coin_x, s.coin_y, 28);
                int cx, cy;
                sample_cell(g, D, L, &cx, &cy);
                cx += g.integers(2, 4);
                cy += g.integers(2, 4);
                clamp_spawn(P, cx, cy);
                s.coin_x = (int16_t)cx;
                s.coin_y = (int16_t)cy;
            }
            reward += cr;
        }
        if (spot_done) done = true;
        s.t++;
        s.coin_t++;
        if (s.coin_t == P.steps_per_coin && P.coin_enabled) done = true;
        if (s.t == P.max_steps) done = true;
    } else {
        bool coins_done;
        {  // the instance's coin list as two 16-byte loads (eight predicated dword loads were issued one after another)
            const uint4 c0 = reinterpret_cast<const uint4*>(coins)[0], c1 = reinterpret_cast<const uint4*>(coins)[1];
            const uint32_t cw[MAX_COINS] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
            for (int q = 0; q < MAX_COINS; ++q) coin_pos[q] = q < s.n_coins ? cw[q] : 0u;
        }
        if (s.num_coins > 0) {
            double cr = 0.0;
#pragma unroll
            for (int q = 0; q < MAX_COINS; ++q) {  // remove-while-iterating: the coin after a collected one is skipped
                if (q >= s.n_coins) break;
                int cx = (int)(int16_t)(coin_pos[q] & 0xFFFF), cy = (int)(coin_pos[q] >> 16);
                if (within(ax - cx, ay - cy, P.coin_radius + P.agent_radius)) {
#pragma unroll
                    for (int j = q; j < MAX_COINS - 1; ++j)
                        if (j < s.n_coins - 1) coin_pos[j] = coin_pos[j + 1];
                    s.n_coins--;
                    cr += P.r_coin;
                    s.coins_collected++;
                }
            }
            coins_done = s.n_coins == 0;
            reward += cr;
        } else {
            coins_done = true;
        }
        bool exit_done = false;
        double er = 0.0;
        if (coins_done && P.use_exit) {  // _step_exit_task (:313-330)
            s.exit_open = 1;
            double ddx = (double)ax - (double)s.exit_x, ddy = (double)ay - (double)s.exit_y;
            if (sqrt(ddx * ddx + ddy * ddy) <= P.exit_radius + (double)P.agent_radius) {
                exit_done = true;
                er = P.r_exit;
            }
        }
        reward += er;
        if (spot_done) done = true;
        else if (coins_done && (P.use_exit ? exit_done : s.num_coins > 0)) { done = true; success = 1; }  // (:499-511)
        s.t++;
        if (s.t == P.max_steps) done = true;
    }
    done = done || cap;
    SPOT_CLOCK_AFTER(4, "v"(done));
    bool shown_last_pos = s.last_pos;
    if (P.show_last_positive_reward) s.last_pos = reward > 0 ? 1 : 0;
    s.ep_sum += reward;
    s.ep_len++;

    if (done && leader) {
        if (info.ep_reward_dev) info.ep_reward_dev[i] = s.ep_sum;
        if (info.ep_length_dev) info.ep_length_dev[i] = s.ep_len;
        if (info.aux_dev[0]) info.aux_dev[0][i] = (float)(s.health / P.agent_health);
        if constexpr (EN) {
            if (info.aux_dev[1]) info.aux_dev[1][i] = (float)s.coins_collected;
        } else {
            if (info.aux_dev[1]) info.aux_dev[1][i] = (float)((double)s.coins_collected / (double)s.num_coins);
            if (info.aux_dev[2]) info.aux_dev[2][i] = (float)success;
        }
    }
    if (leader) {
        reward_out[i] = (float)reward;
        if (info.reward64_dev) info.reward64_dev[i] = reward;  // the reference's Python float, unrounded
        done_out[i] = done ? 1 : 0;
        if (info.capacity_dev) info.capacity_dev[i] = cap ? 1 : 0;
    }

    // debug view only: the (rotated_agent_surface, rotated_agent_rect) pair of this step -- a reset leaves it alone, and the
    // reference's debug render shows that stale pair until the first step of the next episode
    s.pad = (s.pad & PAD_STICKY) | 0x80000000u | ((uint32_t)s.rot8 << 16) | (uint32_t)((ax + 128) & 0xFF) | ((uint32_t)((ay + 128) & 0xFF) << 8);
    // defer: the reset (position sampling on 84x84 masks: ~30 us for the 16 lanes of the instance, the tail of this launch
    // whenever any instance finishes) is queued and done by a service workgroup of the raster launch, which also draws the
    // frame; state, stream and the descriptor head (its n_holes are the reset frame's stale holes) are stored as after
    // any other step, exactly what a masked mg_reset(seed = None) would find.
    const bool reset_me = done && autoreset;
    if constexpr (RECORDS) {
        if (__builtin_expect(done, 0)) {  // the terminal frame: the else branch below, which an in-kernel reset replaces -- its descriptor alone, none of its stores
            SpotDesc* const rec = final_frames + i;
            if (rec_rank >= 0) rec->holes[rec_rank] = rec_hole;
            if (ls >= nh) rec->holes[ls] = rec_stale;
            if (leader) {
                SpotDesc td;
                memset(&td, 0, sizeof(td));
                td.valid = 1;
                td.bg = bg_template(s.pad, s.bg_red);
                td.sprite = s.rot8;
                td.sx = (int16_t)(ax - P.sprite_half);
                td.sy = (int16_t)(ay - P.sprite_half);
                td.alpha = s.alpha;
                td.n_holes = (uint8_t)nh;
                td.exit_stamp = 0xFF;
                if constexpr (EN) {
                    td.n_coins = P.coin_enabled ? 1 : 0;
                    td.coin_above = (uint8_t)(((P.coins_visible || s.coin_t < P.coin_show_duration) ? LAYER_COIN_ABOVE : 0) | P.layer_flags);
                    td.coins[0] = coin_word(P, s.coin_x, s.coin_y);
                } else {
                    td.n_coins = s.n_coins;
                    td.coin_above = (uint8_t)((P.coins_visible ? LAYER_COIN_ABOVE : 0) | P.layer_flags);
#pragma unroll
                    for (int q = 0; q < MAX_COINS; ++q) {
                        if (q < s.n_coins) {
                            int cx = (int)(int16_t)(coin_pos[q] & 0xFFFF), cy = (int)(coin_pos[q] >> 16);
                            td.coins[q] = coin_word(P, cx, cy);
                        }
                    }
                    const int eg = exit_gen_of(s.pad), half = (int)((P.exit_halves >> (8 * eg)) & 0xFFu);
                    td.exit_stamp = (s.pad & PAD_HAS_EXIT) ? (uint8_t)(ST_EXIT0 + 2 * eg + (s.exit_open ? 1 : 0)) : 0xFF;
                    td.exit_x = (int16_t)(s.exit_x - half);
                    td.exit_y = (int16_t)(s.exit_y - half);
                }
                SpotCore tb = s;
                tb.last_pos = shown_last_pos;
                fill_topbar<EN>(P, tb, td, false, shown0, shown1);
                store_desc_head(rec, td);
                reinterpret_cast<uint2*>(rec)[3] = make_uint2(0u, 0u);  // (w6, w7: unused, zero in every descriptor row)
            }
        }
    }
    SPOT_CLOCK(5);
    if (defer && reset_me && leader) queue_push(io.queue, &io.qctr[SQ_COUNT], P.n, i, io.err);
    if (__builtin_expect(reset_me && !defer, 0)) {  // cold: keep the reset code out of the hot instruction stream
        rng_used = true;
        spot_reset<EN>(P, io, i, L, s, g, d, (gt && EN && leader) ? gt + 4 * i : nullptr, nh, disc_slot(disc_lds, L.grp));
    } else {
        d.bg = bg_template(s.pad, s.bg_red);
        d.sprite = s.rot8;
        d.sx = (int16_t)(ax - P.sprite_half);
        d.sy = (int16_t)(ay - P.sprite_half);
        d.alpha = s.alpha;
        d.n_holes = (uint8_t)nh;
        d.exit_stamp = 0xFF;
        if constexpr (EN) {
            d.n_coins = P.coin_enabled ? 1 : 0;
            d.coin_above = (uint8_t)(((P.coins_visible || s.coin_t < P.coin_show_duration) ? LAYER_COIN_ABOVE : 0) | P.layer_flags);
            d.coins[0] = coin_word(P, s.coin_x, s.coin_y);
        } else {
            d.n_coins = s.n_coins;
            d.coin_above = (uint8_t)((P.coins_visible ? LAYER_COIN_ABOVE : 0) | P.layer_flags);
#pragma unroll
            for (int q = 0; q < MAX_COINS; ++q) {
                if (q < s.n_coins) {
                    int cx = (int)(int16_t)(coin_pos[q] & 0xFFFF), cy = (int)(coin_pos[q] >> 16);
                    d.coins[q] = coin_word(P, cx, cy);
                }
            }
            if (leader) {  // entries beyond n_coins are dead; written as two 16-byte stores
                reinterpret_cast<uint4*>(coins)[0] = make_uint4(coin_pos[0], coin_pos[1], coin_pos[2], coin_pos[3]);
                reinterpret_cast<uint4*>(coins)[1] = make_uint4(coin_pos[4], coin_pos[5], coin_pos[6], coin_pos[7]);
            }
            // (the exit fields as in spot_reset, and the coin words unpacked as there -- written out at each site: shared device functions moved the finite step kernel's code)
            const int eg = exit_gen_of(s.pad), half = (int)((P.exit_halves >> (8 * eg)) & 0xFFu);
            d.exit_stamp = (s.pad & PAD_HAS_EXIT) ? (uint8_t)(ST_EXIT0 + 2 * eg + (s.exit_open ? 1 : 0)) : 0xFF;
            d.exit_x = (int16_t)(s.exit_x - half);
            d.exit_y = (int16_t)(s.exit_y - half);
        }
        if (reset_me) d.valid = DESC_QUEUED;
        SpotCore tb = s;
        tb.last_pos = shown_last_pos;  // the bar shows whether the PREVIOUS reward was positive
        fill_topbar<EN>(P, tb, d, false, shown0, shown1);
        if (gt && EN && leader) {  // (write_gt, spelled out: the call moved instructions of the endless step kernel)
            gt[4 * i + 0] = (float)((double)ax / SCREEN);
            gt[4 * i + 1] = (float)((double)ay / SCREEN);
            gt[4 * i + 2] = (float)(P.coin_enabled ? (double)s.coin_x / SCREEN : 0.0);
            gt[4 * i + 3] = (float)(P.coin_enabled ? (double)s.coin_y / SCREEN : 0.0);
        }
    }
    SPOT_CLOCK(6);
    if (leader) {
        if (rng_used) g.store(io.rng, i);
        io.core[i] = s;
        store_desc_head(&io.desc[i], d);
    }
#ifdef MG_LAB_SPOT_CLOCK
    __builtin_amdgcn_s_waitcnt(0);
    SPOT_CLOCK(7);
    {
        const unsigned long long any_spawn = __ballot(f_spawn) != 0, any_coin = __ballot(f_coin) != 0, any_reset = __ballot(reset_me && !defer) != 0;
        const int wave = i >> 2;
        if ((threadIdx.x & 63) == 0 && wave < 65536) {
            unsigned long long* o = g_lab_spot_clock + 10 * (size_t)wave;
            for (int q = 0; q < 8; ++q) o[q] = clk[q];
            o[8] = any_spawn | (any_coin << 1) | (any_reset << 2);
            o[9] = (wall0 & 0xFFFFFFFFull) | (wall_clock64() << 32);
        }
    }
#endif
}
}  // namespace mg
