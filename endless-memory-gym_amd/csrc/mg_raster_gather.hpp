// mg_raster_gather.hpp -- the GATHER form of raster generation 2 (mg_raster.hpp; spotlight family): mg_draw_frames (include/memgym.h).
// The dense kernel draws frame i of the handle from descriptor i; this one draws OUTPUT ROW j from the caller's record pick[j] (pick == NULL: record j),
// for any number of rows.  Same persistent workgroups, composers, prefetch / compose / recycle order and stream-out; the pick is read through the
// constant address space like the descriptor behind it, so both stay scalar loads that do not queue behind the previous frame's stores (the Composer
// concept of mg_raster.hpp).  A kernel of its own: the dense launches are the measured ones and stay as they are.
#pragma once
#include "mg_debug_stream_out.hpp"
#include "mg_frame_records.hpp"
#include "mg_raster.hpp"

namespace mg {

// records: n_records descriptors as mg_save_frames left them; pick: `count` record indices or NULL -- no kernel writes either while this one runs.
// A pick outside 0 .. n_records-1 leaves its row untouched and raises ERR_FRAME_INDEX; a record the composer skips (a masked reset's "leave the frame
// untouched") leaves its row untouched as well.  Row offsets are 64-bit (store_frame multiplies as size_t); j and the pick are 32-bit.
template <class Composer, int FMT, bool NT>
__global__ __launch_bounds__(256, 7) void raster_gather_kernel(const typename Composer::Desc* __restrict__ records, RasterAtlas A, void* __restrict__ obs,
                                                            int n_records, const int32_t* __restrict__ pick, int count, int* err) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RasterCtx R = make_ctx(smem, A);
    const int tid = threadIdx.x, stride = gridDim.x;
    const cptr<typename Composer::Desc> crecords = as_const(records);
    const cptr<int32_t> cpick = as_const(pick);
    Composer::recycle(R);  // scratch state compose() expects (e.g. a zeroed hole mask); published by the barriers below
    __syncthreads();
    for (int j = blockIdx.x; j < count; j += stride) {
        const int r = pick ? cpick[j] : j;  // workgroup-uniform index: a scalar load
        if ((unsigned)r >= (unsigned)n_records) {
            if (tid == 0) __hip_atomic_fetch_or(err, ERR_FRAME_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            continue;
        }
        if (Composer::skip(crecords + r)) continue;
        typename Composer::Pre P;
        Composer::prefetch(crecords + r, R, P);
        Composer::compose(crecords + r, P, R);
        __syncthreads();
        Composer::recycle(R);  // overlaps the stream-out, saves a barrier at the start of the next compose()
        store_frame<FMT, NT, true>(smem, obs, j, tid);
        __syncthreads();  // the LDS frame is reused by the next iteration
    }
}

// The PAD form: mg_draw_frames_padded (include/memgym.h).  raster_gather_kernel with one difference -- a pick below 0 is a PADDING row: the workgroup
// writes it as zeros (store_zero_row: 16-byte stores of a zero vector straight from registers, non-temporal where the launch's frames are; no compose, no
// LDS, no barrier -- the recycled scratch stays as the last frame left it) and raises no error.  A kernel of its own: the gather forms above are the
// measured ones and keep their symbols and their code.
template <class Composer, int FMT, bool NT = false>
__global__ __launch_bounds__(256, 7) void raster_gather_pad_kernel(const typename Composer::Desc* __restrict__ records, RasterAtlas A, void* __restrict__ obs,
                                                                int n_records, const int32_t* __restrict__ pick, int count, int* err) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RasterCtx R = make_ctx(smem, A);
    const int tid = threadIdx.x, stride = gridDim.x;
    const cptr<typename Composer::Desc> crecords = as_const(records);
    const cptr<int32_t> cpick = as_const(pick);
    Composer::recycle(R);  // scratch state compose() expects (e.g. a zeroed hole mask); published by the barriers below
    __syncthreads();
    for (int j = blockIdx.x; j < count; j += stride) {
        const int r = pick ? cpick[j] : j;  // workgroup-uniform index: a scalar load
        if (r < 0) {
            store_zero_row<FMT, NT>(obs, j, tid);
            continue;
        }
        if (r >= n_records) {
            if (tid == 0) __hip_atomic_fetch_or(err, ERR_FRAME_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            continue;
        }
        if (Composer::skip(crecords + r)) continue;
        typename Composer::Pre P;
        Composer::prefetch(crecords + r, R, P);
        Composer::compose(crecords + r, P, R);
        __syncthreads();
        Composer::recycle(R);  // overlaps the stream-out, saves a barrier at the start of the next compose()
        store_frame<FMT, NT, true>(smem, obs, j, tid);
        __syncthreads();  // the LDS frame is reused by the next iteration
    }
}

// The launch of either form -- PAD: raster_gather_pad_kernel (mg_draw_frames_padded), else raster_gather_kernel (mg_draw_frames).  Grid, LDS request and
// store flavour: launch_raster's for a launch of `count` frames
template <class Composer, bool PAD>
inline void launch_raster_gather(const typename Composer::Desc* records, const RasterAtlas& atlas, void* obs, int fmt, int n_records, const int32_t* pick,
                                 int count, int* err, hipStream_t s) {
    const int forced_lds = lab_raster_lds(RASTER_LDS);
    const bool nt = fmt == MG_OBS_U8_XYC && raster_nt(count);
    const int lds = forced_lds ? forced_lds : (nt ? RASTER_LDS_REQUEST : RASTER_LDS);
    const dim3 grid(frames_grid(count));
    auto go = [&](auto F, auto NT) {
        constexpr int FMT = decltype(F)::value;
        constexpr bool STREAM = decltype(NT)::value;
        launch(PAD ? raster_gather_pad_kernel<Composer, FMT, STREAM> : raster_gather_kernel<Composer, FMT, STREAM>, grid, dim3(256), lds, s, records, atlas, obs,
               n_records, pick, count, err);
    };
    if (nt) go(std::integral_constant<int, MG_OBS_U8_XYC>{}, std::true_type{});  // (the non-temporal stream exists for the uint8 format only)
    else with_obs_format(fmt, [&](auto F) { go(F, std::false_type{}); });
}

// mg_draw_debug_frames (include/memgym.h): the same walk over records of the DEBUG view's descriptors with a debug composer.  SIZE 84: the debug
// surface in the observation layout (the uint8 frame's buffer stores, plain); SIZE 336: the reference's debug_rgb_array, stretched and turned on the
// way out of LDS (mg_debug_stream_out.hpp).  Kernels of their own: no MG_OBS_* value names these rows.
template <class Composer, int SIZE>
__global__ __launch_bounds__(256, 7) void raster_debug_gather_kernel(const typename Composer::Desc* __restrict__ records, RasterAtlas A, void* __restrict__ rgb,
                                                                  int n_records, const int32_t* __restrict__ pick, int count, int* err) {
    static_assert(SIZE == 84 || SIZE == DEBUG336, "the debug surface, or its x4 stretch");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RasterCtx R = make_ctx(smem, A);
    const int tid = threadIdx.x, stride = gridDim.x;
    const cptr<typename Composer::Desc> crecords = as_const(records);
    const cptr<int32_t> cpick = as_const(pick);
    Composer::recycle(R);  // scratch state compose() expects (e.g. a zeroed hole mask); published by the barriers below
    __syncthreads();
    for (int j = blockIdx.x; j < count; j += stride) {
        const int r = pick ? cpick[j] : j;  // workgroup-uniform index: a scalar load
        if ((unsigned)r >= (unsigned)n_records) {
            if (tid == 0) __hip_atomic_fetch_or(err, ERR_FRAME_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            continue;
        }
        if (Composer::skip(crecords + r)) continue;
        typename Composer::Pre P;
        Composer::prefetch(crecords + r, R, P);
        Composer::compose(crecords + r, P, R);
        __syncthreads();
        Composer::recycle(R);  // overlaps the stream-out, saves a barrier at the start of the next compose()
        if constexpr (SIZE == 84) store_frame<MG_OBS_U8_XYC, false, true>(smem, rgb, j, tid);
        else store_debug336(smem, rgb, j, tid);
        __syncthreads();  // the LDS frame is reused by the next iteration
    }
}

// size: 84 or 336 (the caller has checked).  Grid and LDS request of a plain-store raster launch over `count` frames.
template <class Composer>
inline void launch_raster_debug_gather(const typename Composer::Desc* records, const RasterAtlas& atlas, void* rgb, int size, int n_records,
                                       const int32_t* pick, int count, int* err, hipStream_t s) {
    const int forced_lds = lab_raster_lds(RASTER_LDS);
    const int lds = forced_lds ? forced_lds : RASTER_LDS;
    const dim3 grid(frames_grid(count));
    if (size == 84) launch(raster_debug_gather_kernel<Composer, 84>, grid, dim3(256), lds, s, records, atlas, rgb, n_records, pick, count, err);
    else launch(raster_debug_gather_kernel<Composer, DEBUG336>, grid, dim3(256), lds, s, records, atlas, rgb, n_records, pick, count, err);
}

}  // namespace mg
