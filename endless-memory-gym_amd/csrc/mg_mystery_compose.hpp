// mg_mystery_compose.hpp -- Mystery Path family: what a frame workgroup draws from a MysteryDesc.  MysteryComposer: black frame (endless: the icy template) ->
// goal / origin or past-path tiles -> agent sprite -> stamina bar -> fall-off cross; MysteryDebugComposer: the reference's debug surface.
#pragma once
#include "mg_raster_v1.hpp"
#include "mg_mystery_types.hpp"

namespace mg {
using namespace v1;  // raster generation 1 (see mg_raster_v1.hpp)
// BIG = false: the agent sprite (up to 1,024 pixels: every agent_scale up to 0.28) is requested with the frame's other loads and held
// in four registers per lane.  BIG = true (an agent_scale whose sprite is larger; chosen per handle by MysteryFamily::rebuild): the
// sprite is blitted from the atlas by the generation-1 stamp() loop, any size; everything else is the same code.
template <bool BIG>
struct MysteryComposerT {
    typedef MysteryDesc Desc;
    static __device__ __forceinline__ bool skip(const Desc* dp) { return dp->valid == 0; }
    static __device__ __forceinline__ void compose(const Desc* dp, const RasterCtx& R) {
        const Desc& d = *dp;
        StampRegs<4> sprite;
        if constexpr (!BIG) sprite = stamp_fetch<4>(R, d.sprite);
        StampRegs<1> cross;
        if (d.cross_on) cross = stamp_fetch<1>(R, ST_CROSS);
        if (d.bg_on) fill_template(R, d.bg_phase);
        else fill_clear(R);
        __syncthreads();
        if (d.goal_on) rect(R, d.goal_x * TILE, d.goal_y * TILE, TILE, TILE, C_GREEN, false);
        if (d.origin_on) rect(R, d.origin_x * TILE, d.origin_y * TILE, TILE, TILE, C_BLUE, false);
        for (int h = 0; h < 2; ++h) {  // distinct path cells: no overlap between them, no barrier needed
            uint64_t m = d.tile_mask[h];
            while (m) {
                int b = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                int cell = h * 64 + b, col = cell / G, row = cell - col * G;
                rect(R, d.tile_x0 + TILE * col, TILE * row, TILE, TILE, C_WHITE, true);
            }
        }
        __syncthreads();
        if constexpr (BIG) stamp(R, d.sprite, d.sx, d.sy);
        else stamp_apply<4>(R, sprite, d.sx, d.sy);
        if (d.stamina_on) {
            __syncthreads();
            rect(R, SCREEN - STAMINA_W, 0, STAMINA_W, SCREEN, C_GREEN, false);
            if (d.stamina_red) {
                __syncthreads();
                rect(R, SCREEN - STAMINA_W, 0, STAMINA_W, d.stamina_red, C_RED, false);
            }
        }
        if (d.cross_on) {
            __syncthreads();
            stamp_apply<1>(R, cross, d.cross_x, d.cross_y);
        }
    }
};
typedef MysteryComposerT<false> MysteryComposer;
typedef MysteryComposerT<true> MysteryBigComposer;

// _build_debug_surface (mystery_path.py:103-117, endless_mystery_path.py:162-182).  The descriptor is a debug one
// (mystery_debug_desc_kernel): pad8[0] = 1 finite -- tile_mask[0] = the path between its ends (white), tile_mask[1] = the walls
// (red), goal / origin always on; pad8[0] = 2 endless -- tile_mask = EVERY path cell of the 16-column window, drawn as the
// reference's path surface: white with surface alpha 200 over the background; the stamina bar always.
__device__ __forceinline__ void rect_blend_white(const RasterCtx& R, int x, int y, int w, int h, uint32_t alpha) {
    for (int p = R.tid; p < w * h; p += 256) {
        const int px = p / h, py = p - px * h, X = x + px, Y = y + py;
        if ((unsigned)X < (unsigned)SCREEN && (unsigned)Y < (unsigned)SCREEN) {
            uint8_t* q = R.frame + X * COL_BYTES + Y * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = (uint8_t)(q[c] + ((255 - (int)q[c]) * (int)alpha) / 255);  // SDL: d += (s - d) * A / 255
        }
    }
}
template <bool BIG>
struct MysteryDebugComposerT {
    typedef MysteryDesc Desc;
    static __device__ __forceinline__ bool skip(const Desc*) { return false; }
    static __device__ __forceinline__ void compose(const Desc* dp, const RasterCtx& R) {
        const Desc& d = *dp;
        const bool endless = d.pad8[0] == 2;
        StampRegs<4> sprite;
        if constexpr (!BIG) sprite = stamp_fetch<4>(R, d.sprite);
        StampRegs<1> cross;
        if (d.cross_on) cross = stamp_fetch<1>(R, ST_CROSS);
        if (d.bg_on) fill_template(R, d.bg_phase);
        else fill_clear(R);
        __syncthreads();
        for (int h = 0; h < 2; ++h) {  // distinct cells: no overlap, no barrier
            uint64_t m = d.tile_mask[h];
            while (m) {
                const int b = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const int cell = endless ? h * 64 + b : b, col = cell / G, row = cell - col * G;
                if (endless) rect_blend_white(R, d.tile_x0 + TILE * col, TILE * row, TILE, TILE, 200u);
                else rect(R, TILE * col, TILE * row, TILE, TILE, h == 0 ? C_WHITE : C_RED, false);
            }
        }
        if (!endless) {  // path[0] (the END node) green, path[-1] (the start) blue: they are not in tile_mask[0]
            rect(R, d.goal_x * TILE, d.goal_y * TILE, TILE, TILE, C_GREEN, false);
            rect(R, d.origin_x * TILE, d.origin_y * TILE, TILE, TILE, C_BLUE, false);
        }
        __syncthreads();
        if constexpr (BIG) stamp(R, d.sprite, d.sx, d.sy);
        else stamp_apply<4>(R, sprite, d.sx, d.sy);
        if (d.cross_on) {
            __syncthreads();
            stamp_apply<1>(R, cross, d.cross_x, d.cross_y);
        }
        if (d.stamina_on) {
            __syncthreads();
            rect(R, SCREEN - STAMINA_W, 0, STAMINA_W, SCREEN, C_GREEN, false);
            if (d.stamina_red) {
                __syncthreads();
                rect(R, SCREEN - STAMINA_W, 0, STAMINA_W, d.stamina_red, C_RED, false);
            }
        }
    }
};
typedef MysteryDebugComposerT<false> MysteryDebugComposer;
typedef MysteryDebugComposerT<true> MysteryDebugBigComposer;
}  // namespace mg
