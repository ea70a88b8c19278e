// mg_mortar_compose.hpp -- Mortar Mayhem family (included by mg_mortar.hip only): what a frame workgroup draws from a MortarDesc.  MortarComposer: arena template -> agent
// sprite -> command glyph, with the measurement hooks MG_LAB_NO_TEMPLATE / MG_LAB_NO_STAMPS (tools/build_variant.sh); MortarDebugComposer: plus the target ring.
#pragma once
#include "mg_mortar_types.hpp"

namespace mg {
using namespace v1;  // raster generation 1 (see mg_raster_v1.hpp)
struct MortarComposer {
    typedef MortarDesc Desc;
    static __device__ __forceinline__ bool skip(const Desc* dp) { return dp->tmpl == 0xFFFF; }
    static __device__ __forceinline__ void compose(const Desc* dp, const RasterCtx& R) {
        const Desc& d = *dp;
#if defined(MG_LAB_NO_TEMPLATE) && MG_LAB_NO_TEMPLATE == 2  // measurement builds (profiles/r06_raster_limits.md): no template at all (stale LDS)
#elif defined(MG_LAB_NO_TEMPLATE)                           // ... a cleared frame instead of the template: no global loads, the LDS writes stay
        fill_clear(R);
#else
        fill_template(R, d.tmpl);
#endif
        __syncthreads();
#ifndef MG_LAB_NO_STAMPS
        if (d.sprite != 0xFF) stamp(R, STAMP_SPRITE0 + d.sprite, d.sx, d.sy);
        if (d.glyph < 9) {
            __syncthreads();
            stamp(R, STAMP_GLYPH0 + d.glyph, d.glyph_x0, d.glyph_x0);
        }
#endif
    }
};

// _build_debug_surface (mortar_mayhem_grid.py:104-135): the observation's layers plus a green ring around the target tile
struct MortarDebugComposer {
    typedef MortarDesc Desc;
    static __device__ __forceinline__ bool skip(const Desc*) { return false; }
    static __device__ __forceinline__ void compose(const Desc* dp, const RasterCtx& R) {
        MortarComposer::compose(dp, R);
        __syncthreads();
        if (dp->ring_on) stamp(R, STAMP_RING, dp->ring_x, dp->ring_y);
    }
};
}  // namespace mg
