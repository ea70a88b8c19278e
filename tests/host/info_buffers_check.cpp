// Stand-alone check (no GPU, no HIP) of csrc/mg_info.hpp: mg_info_buffers read by its struct_size -- today's layout, the layout of a caller built against the
// header before final_frames_dev existed, the shortest layout, sizes that are no layout -- and what mg_step refuses of the terminal-frame members.
// Built and run by tests/test_terminal_records_host.py under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../endless-memory-gym_amd/csrc/mg_info.hpp"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);     \
            return 1;                                              \
        }                                                          \
    } while (0)

static bool refused(const void* info) {
    try {
        (void)mg::read_info((const mg_info_buffers*)info);
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

int main() {
    static_assert(sizeof(mg_info_buffers) == sizeof(mg_info_dev) + sizeof(void*), "final_frames_dev is the one member behind the kernels' view");
    const size_t old_size = offsetof(mg_info_buffers, final_frames_dev);
    double ep[1];
    int32_t len[1];
    float aux0[1];
    uint8_t cap[1];
    alignas(16) unsigned char rows[64];
    alignas(16) unsigned char obs[64];

    // no struct at all: everything NULL
    mg::InfoArgs a = mg::read_info(nullptr);
    CHECK(!a.final_frames && !a.dev.ep_reward_dev && !a.dev.capacity_dev && a.dev.struct_size == sizeof(mg_info_dev));
    CHECK(!mg::final_frames_refusal(a, true) && !mg::final_frames_refusal(a, false));

    // today's layout
    mg_info_buffers now;
    std::memset(&now, 0, sizeof now);
    now.struct_size = sizeof now;
    now.ep_reward_dev = ep;
    now.ep_length_dev = len;
    now.aux_dev[0] = aux0;
    now.capacity_dev = cap;
    now.final_frames_dev = rows;
    a = mg::read_info(&now);
    CHECK(a.final_frames == rows && a.dev.ep_reward_dev == ep && a.dev.ep_length_dev == len && a.dev.aux_dev[0] == aux0 && !a.dev.aux_dev[1] &&
          a.dev.capacity_dev == cap && !a.dev.final_obs_dev && !a.dev.reward64_dev && !a.dev.gt64_dev);
    CHECK(!mg::final_frames_refusal(a, true) && !mg::final_frames_refusal(a, false));

    // a caller built against the OLDER header: exactly old_size bytes exist -- the buffer ends there, so a read beyond it is caught -- and the member reads as NULL
    {
        std::vector<unsigned char> old(old_size);
        std::memcpy(old.data(), &now, old_size);
        const size_t sz = old_size;
        std::memcpy(old.data(), &sz, sizeof sz);
        a = mg::read_info((const mg_info_buffers*)old.data());
        CHECK(!a.final_frames && a.dev.ep_reward_dev == ep && a.dev.capacity_dev == cap && a.dev.aux_dev[0] == aux0);
    }
    // the shortest layout: the episode-record pointers alone
    {
        std::vector<unsigned char> tiny(mg::INFO_SIZE_MIN);
        std::memcpy(tiny.data(), &now, mg::INFO_SIZE_MIN);
        const size_t sz = mg::INFO_SIZE_MIN;
        std::memcpy(tiny.data(), &sz, sizeof sz);
        a = mg::read_info((const mg_info_buffers*)tiny.data());
        CHECK(!a.final_frames && a.dev.ep_length_dev == len && !a.dev.final_obs_dev && !a.dev.capacity_dev);
    }
    // a caller built against a LATER header (more members behind ours): what this build knows is read, the rest ignored
    {
        std::vector<unsigned char> later(sizeof now + 2 * sizeof(void*), 0xEE);
        std::memcpy(later.data(), &now, sizeof now);
        const size_t sz = later.size();
        std::memcpy(later.data(), &sz, sizeof sz);
        a = mg::read_info((const mg_info_buffers*)later.data());
        CHECK(a.final_frames == rows && a.dev.capacity_dev == cap);
    }
    // sizes that are no layout of the header
    for (size_t sz : {(size_t)0, (size_t)8, mg::INFO_SIZE_MIN - 8, old_size + 4, mg::INFO_SIZE_MAX + 8, (size_t)0x7f0012345678ull}) {
        mg_info_buffers bad = now;
        bad.struct_size = sz;
        CHECK(refused(&bad));
    }

    // the refusals
    now.final_obs_dev = obs;
    a = mg::read_info(&now);
    CHECK(mg::final_frames_refusal(a, false) && mg::final_frames_refusal(a, true));  // both: the caller picks one
    now.final_frames_dev = nullptr;
    a = mg::read_info(&now);
    CHECK(!mg::final_frames_refusal(a, false) && mg::final_frames_refusal(a, true));  // terminal observations stay frames: refused headless, as ever
    now.final_obs_dev = nullptr;
    for (int off = 1; off < 16; ++off) {
        now.final_frames_dev = rows + off;
        a = mg::read_info(&now);
        CHECK(mg::final_frames_refusal(a, true) && mg::final_frames_refusal(a, false));  // misaligned
    }
    now.final_frames_dev = rows + 16;
    a = mg::read_info(&now);
    CHECK(!mg::final_frames_refusal(a, true));
    std::printf("OK\n");
    return 0;
}
