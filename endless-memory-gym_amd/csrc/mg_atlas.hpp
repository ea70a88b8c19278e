// mg_atlas.hpp -- host-side container that uploads stamps / templates / tables for the raster kernel.
#pragma once
#include <vector>

#include "mg_family.hpp"
#include "mg_raster.hpp"
#include "mg_stamps.hpp"

namespace mg {

class Atlas : public AtlasStore<AtlasTables, RasterAtlas> {
   public:
    // stamp pixels are stored column-major [x][y] as RGBA words with the column
    // stride padded to a power of two (pixel index p -> x = p >> sh, y = p & (stride - 1): no division in the kernel)
    // max_px: what the composer that draws this stamp can hold in registers (256 pixels per StampRegs slot); a scale
    // option that needs more is refused instead of being drawn truncated
    int add_stamp(const Stamp& s, int max_px = 1 << 30) {
        int id = n_stamps_++;
        if (id >= MAX_STAMPS) throw std::runtime_error("too many stamps");
        int sh = 0;
        while ((1 << sh) < s.h) ++sh;
        if ((s.w << sh) > max_px)
            throw OptionError{-3, "a *_scale reset parameter makes a sprite larger than the " + std::to_string(max_px) +
                                      " (padded) pixels this build's raster holds per layer"};
        tables_.stamps[id].off = (uint32_t)data_.size();
        tables_.stamps[id].w = (uint16_t)s.w;
        tables_.stamps[id].h = (uint16_t)s.h;
        tables_.stamps[id].sh = (uint16_t)sh;
        tables_.stamps[id].pad = 0;
        for (int x = 0; x < s.w; ++x)
            for (int y = 0; y < (1 << sh); ++y) data_.push_back(y < s.h ? rgba(s.get(x, y)) : 0u);
        return id;
    }
    void upload() {
        upload_shared();
        // disc column spans for r = 0..DISC_RMAX
        std::vector<int8_t> span((size_t)(DISC_RMAX + 1) * 2 * DISC_RMAX * 2, 0);
        for (int r = 0; r <= DISC_RMAX; ++r) {
            Stamp s(2 * r + 2, 2 * r + 2);
            if (r >= 1) disc(s, r, r, r, 1);
            for (int i = 0; i < 2 * DISC_RMAX; ++i) {
                int lo = 1, hi = 0;
                if (i < 2 * r) {
                    int ymin = 1 << 20, ymax = -1;
                    for (int y = 0; y < s.h; ++y)
                        if (s.get(i, y)) {
                            ymin = std::min(ymin, y);
                            ymax = std::max(ymax, y);
                        }
                    if (ymax >= 0) {
                        lo = ymin - r;
                        hi = ymax - r;
                    }
                }
                span[((size_t)r * 2 * DISC_RMAX + i) * 2] = (int8_t)lo;
                span[((size_t)r * 2 * DISC_RMAX + i) * 2 + 1] = (int8_t)hi;
            }
        }
        span_dev_.upload(span);
        dev_.disc_span = span_dev_.p;
    }

   private:
    DevArray<int8_t> span_dev_;
};

}  // namespace mg
