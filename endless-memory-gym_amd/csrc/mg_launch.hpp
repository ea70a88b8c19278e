// mg_launch.hpp -- how host code picks a kernel instantiation and launches it: each launch is written once.
//
// with_bool / with_obs_format turn a run-time value into a std::integral_constant handed to a generic lambda, so the lambda
// names the kernel once with `decltype(B)::value` / `decltype(F)::value` as template arguments.  They instantiate EVERY value
// they cover: where a product of flags is only partly populated (a FINAL form exists for the uint8 format alone, say), an
// explicit `if` in front of the helper keeps the missing combinations from being instantiated.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "../../include/memgym.h"

namespace mg {

#define MG_HIP(expr)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            throw std::runtime_error(std::string(#expr) + " failed: " + hipGetErrorString(e_));      \
    } while (0)

template <typename F>
inline void with_bool(bool flag, F&& f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

// the five stream-out formats of include/memgym.h (anything else: the uint8 frame, as the kernels' own default)
template <typename F>
inline void with_obs_format(int fmt, F&& f) {
    if (fmt == MG_OBS_F32_CYX) f(std::integral_constant<int, MG_OBS_F32_CYX>{});
    else if (fmt == MG_OBS_BF16_CYX) f(std::integral_constant<int, MG_OBS_BF16_CYX>{});
    else if (fmt == MG_OBS_F16_CYX) f(std::integral_constant<int, MG_OBS_F16_CYX>{});
    else if (fmt == MG_OBS_U8_CYX) f(std::integral_constant<int, MG_OBS_U8_CYX>{});
    else f(std::integral_constant<int, MG_OBS_U8_XYC>{});
}

// Is work put on this stream being recorded into a graph (hipStreamBeginCapture) instead of being run?
inline bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

// A launch, and a launch whose error is looked at right away.  Which launches are checked is history, not design (the checked
// ones are those that were followed by a hipGetLastError() when this header was written); the rule lives in check_launch().
#ifdef __HIPCC__
template <typename... P, typename... A>
inline void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, s, static_cast<P>(args)...);
}
inline void check_launch() { MG_HIP(hipGetLastError()); }
template <typename... P, typename... A>
inline void launch_checked(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... args) {
    launch(kernel, grid, block, lds, s, static_cast<A&&>(args)...);
    check_launch();
}
#endif

}  // namespace mg
