// mg_palette.hpp -- what the two raster generations (mg_raster_v1.hpp = mg::v1, mg_raster.hpp = mg) share BY VALUE: the palette
// ids and their colours (the reference's: parity-critical, so they exist once), the sizes of the atlas tables, the host store
// behind an atlas and the sparse launch's grid.  Kernels, helpers, RASTER_GRID and RASTER_LDS belong to each generation
// (profiles/r01c_raster_generations.md).
#pragma once
#include <algorithm>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <vector>

#include "mg_device.hpp"
#include "mg_family.hpp"

namespace mg {

constexpr int MAX_STAMPS = 48;
constexpr int PALETTE_SIZE = 32;
constexpr int MASK_WORDS = 3;     // 84 bits per column
constexpr int SPARSE_CHUNK = 32;  // instances a workgroup of raster_sparse_kernel owns

// Palette ids shared by all families
enum : uint8_t {
    C_KEY = 0, C_BODY = 1, C_HAND = 2, C_OUTLINE = 3, C_WHITE = 4, C_RED = 5, C_GREEN = 6, C_BLUE = 7, C_YELLOW = 8,
    C_ORANGE = 9, C_GREY50 = 10, C_GREY120 = 11, C_PURPLE = 12, C_ACT_ORANGE = 13, C_GREY210 = 14, C_BLACK = 15,
    C_EXIT_OPEN = 16, C_EXIT_CLOSED = 17, C_ICY = 18
};
constexpr uint8_t PALETTE_RGB[][3] = {
    {0, 0, 0},       {250, 204, 153}, {250, 250, 250}, {50, 50, 50},  {255, 255, 255}, {255, 0, 0},   {0, 255, 0},
    {0, 0, 255},     {255, 255, 0},   {255, 165, 0},   {50, 50, 50},  {120, 120, 120}, {116, 1, 113}, {255, 94, 14},
    {210, 210, 210}, {0, 0, 0},       {48, 141, 70},   {55, 55, 55},  {125, 177, 250}};
static_assert(sizeof(PALETTE_RGB) / 3 == C_ICY + 1 && C_ICY < PALETTE_SIZE, "one colour per palette id");

// palette[] (r | g<<8 | b<<16) and border_of[] (a colour borders itself, the two light fills are bordered grey) of either
// generation's AtlasTables; the element type of border_of is the generation's own (uint8_t / uint32_t: mg_raster.hpp says why)
template <class Tables>
inline void fill_palette(Tables& t) {
    using Border = typename std::remove_reference<decltype(t.border_of[0])>::type;
    for (int i = 0; i <= C_ICY; ++i) {
        t.palette[i] = (uint32_t)PALETTE_RGB[i][0] | ((uint32_t)PALETTE_RGB[i][1] << 8) | ((uint32_t)PALETTE_RGB[i][2] << 16);
        t.border_of[i] = (Border)i;
    }
    t.border_of[C_WHITE] = C_GREY210;
    t.border_of[C_ICY] = C_GREY210;
}

__device__ __forceinline__ void put_rgb(uint8_t* frame, int x, int y, uint32_t rgb) {
    uint8_t* p = frame + (x * SCREEN + y) * 3;
    p[0] = (uint8_t)rgb;
    p[1] = (uint8_t)(rgb >> 8);
    p[2] = (uint8_t)(rgb >> 16);
}

// What the Atlas class of either generation (mg_atlas_v1.hpp, mg_atlas.hpp) holds on the host and on the device; how a stamp is
// laid out (add_stamp) and what else a generation uploads is its own.  Stamp pixels are palette ids (0 = transparent).
template <class Tables, class Dev>
class AtlasStore {
   public:
    AtlasStore() {
        memset(&tables_, 0, sizeof(tables_));
        fill_palette(tables_);
    }
    // palette id -> r | g<<8 | b<<16 | 0xFF<<24 (opaque); id 0 is the colour key -> 0 (transparent)
    uint32_t rgba(uint8_t id) const { return id ? (tables_.palette[id] | 0xFF000000u) : 0u; }
    int n_stamps() const { return n_stamps_; }
    void set_templates(const std::vector<uint8_t>& t) { templates_ = t; }
    const Dev& dev() const { return dev_; }

   protected:
    void upload_shared() {  // stamp pixels, templates and tables, and dev_'s pointers to them
        if (data_.empty()) data_.push_back(0);
        if (templates_.empty()) templates_.resize(16, 0);
        stamp_dev_.upload(data_);
        templ_dev_.upload(templates_);
        tables_dev_.upload(std::vector<Tables>(1, tables_));
        dev_.templates = templ_dev_.p;
        dev_.stamp_data = stamp_dev_.p;
        dev_.tables = tables_dev_.p;
    }
    Tables tables_;
    int n_stamps_ = 0;
    std::vector<uint32_t> data_;
    std::vector<uint8_t> templates_;
    DevArray<uint32_t> stamp_dev_;
    DevArray<uint8_t> templ_dev_;
    DevArray<Tables> tables_dev_;
    Dev dev_;
};

// workgroups of a sparse raster launch over n instances (raster_sparse_kernel of either generation)
inline int sparse_grid(int n) { return std::min((n + SPARSE_CHUNK - 1) / SPARSE_CHUNK, 8192); }

}  // namespace mg
