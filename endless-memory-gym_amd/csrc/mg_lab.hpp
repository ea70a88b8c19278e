// mg_lab.hpp -- measurement and test switches.
//
// The shipped library (lib/libmemgym_hip.so) reads NO tuning or test switch from the environment: lab_env() is a constant
// there and every branch behind it folds away.  The same sources built with -DMG_LAB (lib/lab/libmemgym_hip_lab.so,
// __graft_entry__.build_hip(lab=True)) honour the MEMGYM_* switches named at their call sites; tools/ and the few tests that
// need a hook (tests/test_gpu_switches.py, test_gpu_error_bits.py, test_gpu_one_launch.py) load that build through MEMGYM_HIP_LIB.
// What a USER can set stays outside the library altogether: MEMGYM_OBS_PLACEMENT / MEMGYM_OBS_SEARCH_GB / MEMGYM_OBS_SEARCH_MS are
// read by the Python mirror (vec_env.py) and travel as arguments (mg_obs_alloc's budget, mg_obs_set_search_ms).
//
// Every switch is read through one of the lab_* readers below.  None of them caches: a switch that is read once per process
// sits in a `static const` at its call site, one that is read at every call does not.
#pragma once
#include <stdlib.h>

namespace mg {
#ifdef MG_LAB
inline const char* lab_env(const char* name) { return getenv(name); }
constexpr bool LAB_BUILD = true;
#else
inline const char* lab_env(const char*) { return nullptr; }
constexpr bool LAB_BUILD = false;
#endif
inline bool lab_set(const char* name) { return lab_env(name) != nullptr; }
inline int lab_int(const char* name, int dflt) {
    const char* e = lab_env(name);
    return e ? atoi(e) : dflt;
}
inline double lab_double(const char* name, double dflt) {
    const char* e = lab_env(name);
    return e ? atof(e) : dflt;
}
inline bool lab_flag(const char* name, bool dflt) { return lab_int(name, dflt ? 1 : 0) != 0; }
// a choice the code makes by itself unless the switch forces it: -1 not set, 0 forced off, 1 forced on
inline int lab_forced(const char* name) {
    const char* e = lab_env(name);
    return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}
// MEMGYM_SPARSE_RASTER=0 (lab build): masked resets draw their frames with the dense persistent launch of rounds 1-5, and a
// gymnasium-convention step (mg_info_buffers.final_obs_dev) re-draws the terminal frames instead of copying them (A/B, bit-exactness tests)
inline bool sparse_masked_raster() {
    static const bool on = lab_flag("MEMGYM_SPARSE_RASTER", true);
    return on;
}
// MEMGYM_RASTER_GRID / MEMGYM_RASTER_LDS (tuning only), shared by the two raster generations (mg_raster.hpp, mg_raster_v1.hpp):
// the forced workgroup count of a raster launch, and the forced LDS request (at least `needed`, what the kernel uses); 0 = not forced
inline int lab_raster_grid() {
    static const int forced = lab_int("MEMGYM_RASTER_GRID", 0);
    return forced > 0 ? forced : 0;
}
inline int lab_raster_lds(int needed) {
    static const int forced = lab_int("MEMGYM_RASTER_LDS", 0);
    return forced >= needed ? forced : 0;
}
}  // namespace mg
