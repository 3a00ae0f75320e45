// PIL-exact 8-bit image resampling (include/wiw_resample.h; Pillow's libImaging/Resample.c: ImagingResampleHorizontal_8bpc /
// ImagingResampleVertical_8bpc) for gfx950 (MI355X): the two image resizes of a request — the conditioning image in
// (LANCZOS), the decoded frames out (BICUBIC) — as integer arithmetic on the device, byte for byte what the host computed.
//
// One launch per pass, the uint8 intermediate [N][H][ow] between them in the caller's scratch:
//   * horizontal: a thread owns one output column of H_ROWS consecutive rows — its taps (n <= 64 int32 coefficients) are
//     loaded once for the rows; neighbouring lanes own neighbouring columns, so a wave's loads of one tap fall into
//     64 * W / ow consecutive source samples;
//   * vertical: a block owns 256 columns of ONE output row: window and coefficients are block-uniform, every tap is one
//     coalesced row segment.
// The source is uint8, or the decoder's fp32 frames quantised at the load (the frames are read by the first pass that runs
// and never stored as uint8).  A source sample is fetched from HBM once: what neighbouring outputs share (ksize / scale taps)
// comes from the caches.  Sums are int32 as in Pillow (|sum| < 2^31 by the 22-bit precision), shifts arithmetic.  Windows
// are clamped to the plane, so a wrong table cannot address outside it.  Plain loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

#include "../../include/wiw_resample.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int H_ROWS = 4;          // rows per thread of the horizontal pass
constexpr int TILE = 256;          // output columns per block (= threads)
constexpr int64_t MAX_GRID = 1 << 20;

WIW_DEV int load_px(const uint8_t* p) { return (int)*p; }
// the frame quantisation of vae.frames_to_uint8_device: clamp(x / 2 + 0.5, 0, 1) * 255, round half to even, fp32
WIW_DEV int load_px(const float* p) {
#pragma clang fp contract(off)
    float t = __builtin_fmaf(*p, 0.5f, 0.5f);          // x * 0.5 is exact: one rounding, that of x / 2 + 0.5
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float s = t * 255.0f;
    return (int)__builtin_rintf(s);
}
WIW_DEV uint8_t clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

struct Planes {          // element offsets: row r of plane p at p * plane + r * row
    int64_t plane, row;
};

// rows = N * H source rows; output column xx of row r -> dst row r (same plane / row split, height H)
template <typename SrcT>
__global__ __launch_bounds__(TILE) void resample_h_kernel(const SrcT* __restrict__ src, Planes sp, uint8_t* __restrict__ dst,
                                                           Planes dp, int64_t rows, int H, int W, int ow,
                                                           const int32_t* __restrict__ coef, const int32_t* __restrict__ bounds,
                                                           int ksize) {
    const int xtiles = (ow + TILE - 1) / TILE;
    const int64_t rtiles = (rows + H_ROWS - 1) / H_ROWS;
    for (int64_t t = blockIdx.x; t < rtiles * xtiles; t += gridDim.x) {
        const int xx = (int)(t % xtiles) * TILE + (int)threadIdx.x;
        const int r0 = (int)(t / xtiles) * H_ROWS;          // rows <= 2^30 (checked by the entry point)
        if (xx >= ow) continue;
        int first = bounds[2 * xx], n = bounds[2 * xx + 1];
        first = min(max(first, 0), W);
        n = min(min(max(n, 0), ksize), W - first);
        const int32_t* k = coef + (int64_t)xx * ksize;
        const SrcT* in[H_ROWS];
        int acc[H_ROWS];
#pragma unroll
        for (int j = 0; j < H_ROWS; ++j) {
            const int r = min(r0 + j, (int)rows - 1);          // a row past the end recomputes the last one and is not stored
            in[j] = src + (r / H) * sp.plane + (r % H) * sp.row + first;
            acc[j] = 1 << (PRECISION_BITS - 1);
        }
        for (int i = 0; i < n; ++i) {
            const int c = k[i];
#pragma unroll
            for (int j = 0; j < H_ROWS; ++j) acc[j] += load_px(in[j] + i) * c;
        }
#pragma unroll
        for (int j = 0; j < H_ROWS; ++j) {
            const int r = r0 + j;
            if (r < rows) dst[(r / H) * dp.plane + (r % H) * dp.row + xx] = clip8(acc[j]);
        }
    }
}

// orows = N * oh output rows; output row yy of plane p reads source rows first .. first + n - 1 of plane p (height H)
template <typename SrcT>
__global__ __launch_bounds__(TILE) void resample_v_kernel(const SrcT* __restrict__ src, Planes sp, uint8_t* __restrict__ dst,
                                                           Planes dp, int64_t orows, int H, int oh, int ow,
                                                           const int32_t* __restrict__ coef, const int32_t* __restrict__ bounds,
                                                           int ksize) {
    const int xtiles = (ow + TILE - 1) / TILE;
    for (int64_t t = blockIdx.x; t < orows * xtiles; t += gridDim.x) {
        const int x = (int)(t % xtiles) * TILE + (int)threadIdx.x;
        const int r = (int)(t / xtiles);
        const int64_t p = r / oh;
        const int yy = r % oh;
        if (x >= ow) continue;
        int first = bounds[2 * yy], n = bounds[2 * yy + 1];
        first = min(max(first, 0), H);
        n = min(min(max(n, 0), ksize), H - first);
        const int32_t* k = coef + (int64_t)yy * ksize;
        const SrcT* in = src + p * sp.plane + (int64_t)first * sp.row + x;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int i = 0; i < n; ++i) acc += load_px(in + (int64_t)i * sp.row) * k[i];
        dst[p * dp.plane + (int64_t)yy * dp.row + x] = clip8(acc);
    }
}

// neither side changes: the copy (of the quantised frames, for an fp32 source)
template <typename SrcT>
__global__ __launch_bounds__(TILE) void resample_copy_kernel(const SrcT* __restrict__ src, Planes sp, uint8_t* __restrict__ dst,
                                                              Planes dp, int64_t rows, int H, int W) {
    const int xtiles = (W + TILE - 1) / TILE;
    for (int64_t t = blockIdx.x; t < rows * xtiles; t += gridDim.x) {
        const int x = (int)(t % xtiles) * TILE + (int)threadIdx.x;
        const int r = (int)(t / xtiles);
        if (x >= W) continue;
        dst[(r / H) * dp.plane + (r % H) * dp.row + x] = (uint8_t)load_px(src + (r / H) * sp.plane + (r % H) * sp.row + x);
    }
}

__global__ __launch_bounds__(256) void u8_to_f32_lut_kernel(const uint8_t* __restrict__ src, int64_t n, const float* __restrict__ lut,
                                                             float* __restrict__ dst) {
    __shared__ float table[256];
    table[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = table[src[i]];
}

unsigned grid_for(int64_t tiles) { return (unsigned)(tiles < MAX_GRID ? tiles : MAX_GRID); }

template <typename SrcT>
int resample_planes(const char* what, void* stream_, const SrcT* src, int64_t sps, int64_t srs, int N, int H, int W, uint8_t* dst,
                    int64_t dps, int64_t drs, int oh, int ow, const int32_t* coef_h, const int32_t* bounds_h, int ksize_h,
                    const int32_t* coef_v, const int32_t* bounds_v, int ksize_v, uint8_t* scratch) {
    WIW_REQUIRE(src && dst, "resample: null pointer");
    WIW_REQUIRE(N > 0 && H > 0 && W > 0 && oh > 0 && ow > 0, "resample: sizes must be positive");
    WIW_REQUIRE((int64_t)N * (H > oh ? H : oh) <= (1 << 30), "resample: more than 2^30 rows");
    WIW_REQUIRE(srs >= W && drs >= ow, "resample: a row stride is smaller than a row");
    WIW_REQUIRE(sps >= (int64_t)H * srs && dps >= (int64_t)oh * drs, "resample: a plane stride is smaller than a plane");
    WIW_REQUIRE((coef_h == nullptr) == (bounds_h == nullptr) && (coef_v == nullptr) == (bounds_v == nullptr),
                "resample: coefficients and bounds of a pass come together");
    WIW_REQUIRE(coef_h || ow == W, "resample: the horizontal pass is skipped (null table) but ow != W");
    WIW_REQUIRE(coef_v || oh == H, "resample: the vertical pass is skipped (null table) but oh != H");
    WIW_REQUIRE(!coef_h || (ksize_h >= 1 && ksize_h <= WIW_RESAMPLE_MAX_TAPS), "resample: 1 <= ksize_h <= 64 taps");
    WIW_REQUIRE(!coef_v || (ksize_v >= 1 && ksize_v <= WIW_RESAMPLE_MAX_TAPS), "resample: 1 <= ksize_v <= 64 taps");
    WIW_REQUIRE(!(coef_h && coef_v) || scratch, "resample: both passes run and scratch is null");
    WIW_REQUIRE((((uintptr_t)coef_h | (uintptr_t)bounds_h | (uintptr_t)coef_v | (uintptr_t)bounds_v) & 3) == 0,
                "resample: the tables must be 4-byte aligned");
    WIW_REQUIRE(sizeof(SrcT) == 1 || ((uintptr_t)src & 3) == 0, "resample: fp32 frames must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const Planes sp{sps, srs}, dp{dps, drs};
    const int64_t rows = (int64_t)N * H, orows = (int64_t)N * oh;
    const int64_t xt_o = (ow + TILE - 1) / TILE;
    if (coef_h && coef_v) {
        const Planes mid{(int64_t)H * ow, ow};
        hipLaunchKernelGGL(resample_h_kernel<SrcT>, dim3(grid_for((rows + H_ROWS - 1) / H_ROWS * xt_o)), dim3(TILE), 0, stream, src,
                           sp, scratch, mid, rows, H, W, ow, coef_h, bounds_h, ksize_h);
        hipLaunchKernelGGL(resample_v_kernel<uint8_t>, dim3(grid_for(orows * xt_o)), dim3(TILE), 0, stream,
                           (const uint8_t*)scratch, mid, dst, dp, orows, H, oh, ow, coef_v, bounds_v, ksize_v);
    } else if (coef_h) {
        hipLaunchKernelGGL(resample_h_kernel<SrcT>, dim3(grid_for((rows + H_ROWS - 1) / H_ROWS * xt_o)), dim3(TILE), 0, stream, src,
                           sp, dst, dp, rows, H, W, ow, coef_h, bounds_h, ksize_h);
    } else if (coef_v) {
        hipLaunchKernelGGL(resample_v_kernel<SrcT>, dim3(grid_for(orows * xt_o)), dim3(TILE), 0, stream, src, sp, dst, dp, orows, H,
                           oh, ow, coef_v, bounds_v, ksize_v);
    } else {
        hipLaunchKernelGGL(resample_copy_kernel<SrcT>, dim3(grid_for(rows * xt_o)), dim3(TILE), 0, stream, src, sp, dst, dp, rows,
                           H, W);
    }
    return wiw_check_launch(what);
}

}  // namespace

extern "C" int64_t wiw_resample_u8_scratch_bytes(int N, int H, int ow) {
    if (N <= 0 || H <= 0 || ow <= 0) return 0;
    return (int64_t)N * H * ow;
}

extern "C" int wiw_resample_u8(void* stream, const uint8_t* src, int64_t src_plane_stride, int64_t src_row_stride, int N, int H,
                               int W, uint8_t* dst, int64_t dst_plane_stride, int64_t dst_row_stride, int oh, int ow,
                               const int32_t* coef_h, const int32_t* bounds_h, int ksize_h, const int32_t* coef_v,
                               const int32_t* bounds_v, int ksize_v, uint8_t* scratch) {
    return resample_planes<uint8_t>("wiw_resample_u8", stream, src, src_plane_stride, src_row_stride, N, H, W, dst,
                                    dst_plane_stride, dst_row_stride, oh, ow, coef_h, bounds_h, ksize_h, coef_v, bounds_v, ksize_v,
                                    scratch);
}

extern "C" int wiw_frames_resample_u8(void* stream, const float* src, int64_t src_plane_stride, int64_t src_row_stride, int N,
                                      int H, int W, uint8_t* dst, int64_t dst_plane_stride, int64_t dst_row_stride, int oh, int ow,
                                      const int32_t* coef_h, const int32_t* bounds_h, int ksize_h, const int32_t* coef_v,
                                      const int32_t* bounds_v, int ksize_v, uint8_t* scratch) {
    return resample_planes<float>("wiw_frames_resample_u8", stream, src, src_plane_stride, src_row_stride, N, H, W, dst,
                                  dst_plane_stride, dst_row_stride, oh, ow, coef_h, bounds_h, ksize_h, coef_v, bounds_v, ksize_v,
                                  scratch);
}

extern "C" int wiw_u8_to_f32_lut(void* stream, const uint8_t* src, int64_t n, const float* lut, float* dst) {
    WIW_REQUIRE(src && lut && dst, "u8_to_f32_lut: null pointer");
    WIW_REQUIRE(n > 0, "u8_to_f32_lut: n must be positive");
    WIW_REQUIRE((((uintptr_t)lut | (uintptr_t)dst) & 3) == 0, "u8_to_f32_lut: lut and dst must be 4-byte aligned");
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(u8_to_f32_lut_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, src,
                       n, lut, dst);
    return wiw_check_launch("wiw_u8_to_f32_lut");
}
