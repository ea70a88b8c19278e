// mg_spot_compose.hpp -- Searing Spotlights family (included by mg_spot.hip only): what a frame workgroup draws from a SpotDesc.  SpotComposerT<BORDER>: hole mask ->
// board, coin(s) / exit, agent, each darkened outside the holes while written -> layers shown above the dark layer -> top bar; BORDER adds the spotlights' white rings
// (ring_mask / ring_apply).  SpotDebugComposerT: the reference's debug surface from the same descriptor.
#pragma once
#include "mg_stamps.hpp"
#include "mg_spot_types.hpp"

namespace mg {
// ---- spotlights with a border (Spotlight.draw: filled disc, then pygame's 1-px circle in white, pygame_assets.py:110-113) ----
// The spotlight surface ends up with three kinds of pixels: black (the dark layer), the colour key (a hole) and white (a
// border pixel, blended over what lies below with the layer's alpha).  Spotlights are drawn in list order, so a pixel shows
// a border iff the LAST disc covering it has one and the pixel lies on it.  One lane per column walks the hole words in
// order: a disc clears the ring bits of its column span, a border sets its own (draw_circle_bresenham_thin: the end points
// of the spans draw_circle_filled walks, for every x step).  Only the border composer does this.
template <class HoleAt>
__device__ __forceinline__ void ring_mask(const RasterCtx& R, HoleAt hole_at, int nholes, uint32_t* ring) {
    if (R.tid >= SCREEN) return;
    const int X = R.tid;
    uint32_t rg[MASK_WORDS] = {0u, 0u, 0u};
    for (int h = 0; h < nholes; ++h) {
        const uint32_t hv = hole_at(h);
        const int hx = (int)(hv & 511u) - 128, hy = (int)((hv >> 9) & 511u) - 128, r = hole_radius(hv);
        const int col = X - (hx - r);
        if (col < 0 || col >= 2 * r) continue;
        const int lo = R.A.disc_span[(r * 2 * DISC_RMAX + col) * 2], hi = R.A.disc_span[(r * 2 * DISC_RMAX + col) * 2 + 1];
        int y0 = hy + lo, y1 = hy + hi;
        y0 = y0 < 0 ? 0 : y0;
        y1 = y1 > SCREEN - 1 ? SCREEN - 1 : y1;
#pragma unroll
        for (int w = 0; w < MASK_WORDS; ++w) {
            int a0 = y0 - 32 * w, a1 = y1 - 32 * w;
            a0 = a0 < 0 ? 0 : a0;
            a1 = a1 > 31 ? 31 : a1;
            if (a0 <= a1) rg[w] &= ~((a1 - a0 == 31) ? 0xFFFFFFFFu : (((1u << (a1 - a0 + 1)) - 1u) << a0));
        }
        if (!(hv >> 31)) continue;
        auto put = [&](int px, int py) {
            if (px == X && (unsigned)py < (unsigned)SCREEN) {
                const uint32_t bit = 1u << (py & 31);
#pragma unroll
                for (int w = 0; w < MASK_WORDS; ++w) rg[w] |= (py >> 5) == w ? bit : 0u;
            }
        };
        int f = 1 - r, ddx = 0, ddy = -2 * r, x = 0, y = r;
        while (x < y) {
            if (f >= 0) {
                --y;
                ddy += 2;
                f += ddy;
            }
            ++x;
            ddx += 2;
            f += ddx + 1;
            put(hx + x - 1, hy + y - 1);
            put(hx - x, hy + y - 1);
            put(hx + x - 1, hy - y);
            put(hx - x, hy - y);
            put(hx + y - 1, hy + x - 1);
            put(hx + y - 1, hy - x);
            put(hx - y, hy + x - 1);
            put(hx - y, hy - x);
        }
    }
#pragma unroll
    for (int w = 0; w < MASK_WORDS; ++w) ring[X * MASK_WORDS + w] = rg[w];
}
// the border pixels over everything drawn so far: d += (255 - d) * A / 255 (SDL ALPHA_BLEND_RGB, source white)
__device__ __forceinline__ void ring_apply(const RasterCtx& R, const uint32_t* ring, uint32_t alpha) {
    if (R.tid >= SCREEN * MASK_WORDS) return;
    const int X = R.tid / MASK_WORDS, w = R.tid - X * MASK_WORDS;
    uint32_t bits = ring[R.tid];
    while (bits) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        uint8_t* p = R.frame + (X * SCREEN + 32 * w + b) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = (uint8_t)(p[c] + ((255u - p[c]) * alpha) / 255u);
    }
}

template <bool BORDER>
__device__ __forceinline__ uint32_t* ring_words() {  // LDS of the border composers only
    if constexpr (BORDER) {
        __shared__ uint32_t ring[SCREEN * MASK_WORDS];
        return ring;
    } else {
        return nullptr;
    }
}

template <bool BORDER>
struct SpotComposerT {
    typedef SpotDesc Desc;
    static __device__ __forceinline__ bool skip(cptr<Desc> dp) { return view_of(dp).valid() == 0; }
    // top bar (rows y < BAR_H of every column); priority reward bar > action rects > red > green > base.
    // Returns false where no bar element covers column x (the scene shows through).
    template <class V>
    static __device__ __forceinline__ bool bar_colour(const V& d, cptr<AtlasTables> T, int x, uint32_t* c) {
        bool has = d.c_base() != 0xFF;
        uint32_t id = d.c_base();
        if (x < 2 * d.quarter()) { id = x < d.red_w() ? (uint32_t)C_RED : (uint32_t)C_GREEN; has = true; }
        else if (d.c_act0() != 0xFF) { id = x < 3 * d.quarter() ? d.c_act0() : d.c_act1(); has = true; }
        if (d.c_bar() != 0xFF && x >= d.bar_x() && x < d.bar_x() + d.bar_w()) { id = d.c_bar(); has = true; }
        if (has) *c = T->palette[id];
        return has;
    }
    template <class V>
    static __device__ __forceinline__ bool bar_covers(const V& d, int x) {
        return d.c_base() != 0xFF || x < 2 * d.quarter() || d.c_act0() != 0xFF || (d.c_bar() != 0xFF && x >= d.bar_x() && x < d.bar_x() + d.bar_w());
    }
    template <class V>
    static __device__ __forceinline__ void bar_columns(const V& d, cptr<AtlasTables> T, const RasterCtx& R) {
        static_assert(BAR_H == 4, "one bar column = 4 pixels = 3 dwords");
        if (R.tid < SCREEN) {
            uint32_t c = 0u;
            if (bar_colour(d, T, R.tid, &c)) {
                const uint32_t r = c & 0xFFu, g = (c >> 8) & 0xFFu, b = (c >> 16) & 0xFFu;
                uint32_t* p = reinterpret_cast<uint32_t*>(R.frame) + R.tid * (COL_BYTES / 4);
                p[0] = r | (g << 8) | (b << 16) | (r << 24);
                p[1] = g | (b << 8) | (r << 16) | (g << 24);
                p[2] = b | (r << 8) | (g << 16) | (b << 24);
            }
        }
    }
    // Order of the reference's _draw_surfaces (endless_searing_spotlights.py:464-479, searing_spotlights.py:524-545):
    // board, coins (unless drawn above), exit, agent, spotlight layer, coins above, top bar.  The spotlight layer is
    // not a pass of its own: the hole mask is built first and every layer below it is darkened as it is written.
    struct Pre {
        TemplRegs bg;
        StampRegs<1> agent, coin, exitp;
        HoleRegs8 holes;
    };
    // every global read of the frame (template, sprite / coin / exit pixels, disc spans)
    template <class V>
    static __device__ __forceinline__ void prefetch_v(const V& d, const RasterCtx& R, Pre& P) {
        templ_fetch(R, d.bg(), P.bg);
        stamp_fetch<1>(R, d.sprite(), P.agent);
        if (d.n_coins()) stamp_fetch<1>(R, ST_COIN, P.coin);
        else stamp_none<1>(P.coin);
        if (d.exit_stamp() != 0xFF) stamp_fetch<1>(R, d.exit_stamp(), P.exitp);
        else stamp_none<1>(P.exitp);
        P.holes.hole[0] = P.holes.hole[1] = P.holes.span[0] = P.holes.span[1] = 0u;
        auto hole_at = [&](int h) { return d.hole(h); };
        if (d.alpha() && holes_small(hole_at, d.n_holes())) hole_fetch8(R, hole_at, d.n_holes(), P.holes);
    }
    static __device__ __forceinline__ void prefetch(cptr<Desc> dp, const RasterCtx& R, Pre& P) { prefetch_v(view_of(dp), R, P); }
    static __device__ __forceinline__ void recycle(const RasterCtx& R) { zero_mask(R); }
    static __device__ __forceinline__ void compose(cptr<Desc> dp, const Pre& P, const RasterCtx& R) { compose_v(view_of(dp), P, R); }
    template <class V>
    static __device__ __forceinline__ void compose_v(const V& d, const Pre& P, const RasterCtx& R) {
        const cptr<AtlasTables> T = R.T;
        const uint32_t alpha = d.alpha();
        const StampRegs<1>&agent = P.agent, &coin = P.coin, &exitp = P.exitp;
        uint32_t* const ring = ring_words<BORDER>();
        auto hole_at = [&](int h) { return d.hole(h); };
        const int n_holes = d.n_holes(), n_coins = d.n_coins();
        if (alpha) {  // the hole mask is zero on entry (recycle())
            if (holes_small(hole_at, n_holes)) hole_apply8(R, P.holes);
            else hole_mask(R, hole_at, n_holes);  // radii beyond the reference's range: span table read in place
            if constexpr (BORDER) ring_mask(R, hole_at, n_holes, ring);
            __syncthreads();
        }
        templ_apply_dark(R, P.bg, alpha);
        __syncthreads();
        auto under_bar = [&](int X, int Y) { return Y < BAR_H && bar_covers(d, X); };
        const uint32_t lf = d.coin_above();
        const bool exit_here = d.exit_stamp() != 0xFF;
        const int sx = d.sx(), sy = d.sy(), exit_x = d.exit_x(), exit_y = d.exit_y();
        if constexpr (BORDER) {  // the same layers, with the border pixels blended in where the spotlight layer sits
            if (!(lf & LAYER_COIN_ABOVE))
                for (int k = 0; k < n_coins; ++k) stamp_apply_lit<1>(R, coin, d.coin_x(k), d.coin_y(k), alpha, never_skip);
            if (exit_here && !(lf & LAYER_EXIT_ABOVE)) stamp_apply_lit<1>(R, exitp, exit_x, exit_y, alpha, never_skip);
            __syncthreads();
            if (!(lf & LAYER_AGENT_TOP)) stamp_apply_lit<1>(R, agent, sx, sy, alpha, never_skip);
            __syncthreads();
            if (alpha) {
                ring_apply(R, ring, alpha);
                __syncthreads();
            }
            if (lf & LAYER_COIN_ABOVE)
                for (int k = 0; k < n_coins; ++k) stamp_apply_lit<1>(R, coin, d.coin_x(k), d.coin_y(k), 0u, under_bar);
            if (exit_here && (lf & LAYER_EXIT_ABOVE)) stamp_apply_lit<1>(R, exitp, exit_x, exit_y, 0u, under_bar);
            bar_columns(d, T, R);
            if (lf & LAYER_AGENT_TOP) {
                __syncthreads();
                stamp_apply_lit<1>(R, agent, sx, sy, 0u, never_skip);
            }
            return;
        }
        // coins keep their distance from each other and from the exit (sampler block radius): no overlap among them.
        // coins_visible / exit_visible / agent_visible move a layer from below the dark layer to above it (the agent:
        // to the very top, over the bar -- the reference's list.insert index is past the end of its surface list).
        if (!(lf & LAYER_COIN_ABOVE))
            for (int k = 0; k < n_coins; ++k) stamp_apply_lit<1>(R, coin, d.coin_x(k), d.coin_y(k), alpha, never_skip);
        if (exit_here && !(lf & LAYER_EXIT_ABOVE)) stamp_apply_lit<1>(R, exitp, exit_x, exit_y, alpha, never_skip);
        __syncthreads();
        if (!(lf & (LAYER_COIN_ABOVE | LAYER_EXIT_ABOVE))) {  // the bar follows without a barrier: leave its pixels alone
            if (!(lf & LAYER_AGENT_TOP)) stamp_apply_lit<1>(R, agent, sx, sy, alpha, under_bar);
        } else {
            if (!(lf & LAYER_AGENT_TOP)) stamp_apply_lit<1>(R, agent, sx, sy, alpha, never_skip);
            __syncthreads();
            if (lf & LAYER_COIN_ABOVE)
                for (int k = 0; k < n_coins; ++k) stamp_apply_lit<1>(R, coin, d.coin_x(k), d.coin_y(k), 0u, under_bar);
            if (exit_here && (lf & LAYER_EXIT_ABOVE)) stamp_apply_lit<1>(R, exitp, exit_x, exit_y, 0u, under_bar);
        }
        bar_columns(d, T, R);
        if (lf & LAYER_AGENT_TOP) {
            __syncthreads();
            stamp_apply_lit<1>(R, agent, sx, sy, 0u, never_skip);
        }
    }
};
typedef SpotComposerT<false> SpotComposer;
typedef SpotComposerT<true> SpotBorderComposer;  // black_background has been on: spotlights may have a border

// _build_debug_surface (searing_spotlights.py:157-185, endless_searing_spotlights.py:150-177): board, spotlight layer, then
// exit, coins and agent OVER it (undarkened), top bar last.  Same descriptor, prefetch and hole mask as the observation.
template <bool BORDER>
struct SpotDebugComposerT {
    typedef SpotDesc Desc;
    typedef SpotComposerT<false> Obs;
    typedef Obs::Pre Pre;
    static __device__ __forceinline__ bool skip(cptr<Desc>) { return false; }
    static __device__ __forceinline__ void prefetch(cptr<Desc> dp, const RasterCtx& R, Pre& P) { Obs::prefetch(dp, R, P); }
    static __device__ __forceinline__ void recycle(const RasterCtx& R) { zero_mask(R); }
    static __device__ __forceinline__ void compose(cptr<Desc> dp, const Pre& P, const RasterCtx& R) {
        const SpotViewMem d = view_of(dp);
        const uint32_t alpha = d.alpha();
        uint32_t* const ring = ring_words<BORDER>();
        auto hole_at = [&](int h) { return d.hole(h); };
        if (alpha) {
            if (holes_small(hole_at, d.n_holes())) hole_apply8(R, P.holes);
            else hole_mask(R, hole_at, d.n_holes());
            if constexpr (BORDER) ring_mask(R, hole_at, d.n_holes(), ring);
            __syncthreads();
        }
        templ_apply_dark(R, P.bg, alpha);
        __syncthreads();
        if constexpr (BORDER) {
            if (alpha) {
                ring_apply(R, ring, alpha);
                __syncthreads();
            }
        }
        auto under_bar = [&](int X, int Y) { return Y < BAR_H && Obs::bar_covers(d, X); };
        if (d.exit_stamp() != 0xFF) stamp_apply_lit<1>(R, P.exitp, d.exit_x(), d.exit_y(), 0u, under_bar);
        for (int k = 0; k < d.n_coins(); ++k) stamp_apply_lit<1>(R, P.coin, d.coin_x(k), d.coin_y(k), 0u, under_bar);
        __syncthreads();
        stamp_apply_lit<1>(R, P.agent, d.sx(), d.sy(), 0u, under_bar);
        Obs::bar_columns(d, R.T, R);
    }
};
typedef SpotDebugComposerT<false> SpotDebugComposer;
typedef SpotDebugComposerT<true> SpotBorderDebugComposer;
}  // namespace mg
