// mg_atlas_v1.hpp (namespace mg::v1, pairs with mg_raster_v1.hpp) -- host-side container that uploads stamps / templates / tables for the raster kernel.
#pragma once
#include <vector>

#include "mg_family.hpp"
#include "mg_raster_v1.hpp"
#include "mg_stamps.hpp"

namespace mg {
namespace v1 {

class Atlas : public AtlasStore<AtlasTables, RasterAtlas> {
   public:
    // stamp pixels are stored column-major [x][y]
    // max_px: what the composer that draws this stamp can hold in registers (256 pixels per StampRegs slot); a scale
    // option that needs more is refused instead of being drawn truncated
    int add_stamp(const Stamp& s, int max_px = 1 << 30) {
        int id = n_stamps_++;
        if (id >= MAX_STAMPS) throw std::runtime_error("too many stamps");
        if (s.w * s.h > max_px)
            throw OptionError{-3, "a *_scale reset parameter makes a sprite larger than the " + std::to_string(max_px) +
                                      " pixels this build's raster holds per layer"};
        tables_.stamps[id].off = (uint32_t)data_.size();
        tables_.stamps[id].w = (uint16_t)s.w;
        tables_.stamps[id].h = (uint16_t)s.h;
        for (int x = 0; x < s.w; ++x)
            for (int y = 0; y < s.h; ++y) data_.push_back(rgba(s.get(x, y)));
        return id;
    }
    void upload() { upload_shared(); }
};

}  // namespace v1
}  // namespace mg
