/* PIL-exact 8-bit image resampling on the device (csrc/resample.hip) — an additive companion of include/wiw_svd.h (same
 * conventions: device pointers, caller-owned memory, `stream` a hipStream_t or NULL, WIW_OK or a negative WIW_E* code,
 * wiw_last_error() for the message; nothing is launched on error; no allocation and no synchronisation, so every entry point
 * may be captured into a graph).  Exported with the same entry points by both builds of the library (bf16: libwiwsvd.so,
 * fp16: libwiwsvd_f16.so: nothing here touches the 16-bit type); WIW_ABI_VERSION is unchanged.  Every launching entry point
 * declared here has a case in tests/test_hip_resample_footprint.py (tests/test_resample.py checks it).
 *
 * The operation is `Image.resize` of Pillow on 8-bit planes (libImaging/Resample.c): one pass per axis, horizontal first,
 *
 *     out = clip((2^21 + sum_{k < n} in[first + k] * coef[k]) >> 22, 0, 255)          int32 sum, arithmetic shift
 *
 * with the uint8 result of the horizontal pass as the input of the vertical one.  The tables come from the host
 * (`resample.pil_tables`, Pillow's precompute_coeffs + normalize_coeffs_8bpc) and are per AXIS:
 *
 *   coef_x   : int32 [out][ksize_x], 22-bit fixed point, row `o` = the taps of output sample o (entries past n are unused)
 *   bounds_x : int32 [out][2] = (first, n): output sample o reads input samples first .. first + n - 1; the kernels clamp
 *              first to [0, in] and n to [0, min(ksize_x, in - first)], so a wrong table cannot read outside a plane
 *   coef_h / bounds_h / ksize_h: the horizontal pass W -> ow (out = ow); coef_v / bounds_v / ksize_v: the vertical pass
 *   H -> oh (out = oh).  coef_x == NULL (then bounds_x must be NULL too) SKIPS that pass — the side must then be unchanged
 *   (ow == W / oh == H), as Pillow skips it.  1 <= ksize_x <= 64.
 *
 *   planes   : N planes of H rows of W samples; row r of plane p starts at p * plane_stride + r * row_stride ELEMENTS;
 *              row_stride >= the row's length, plane_stride >= rows * row_stride (of source and destination alike)
 *   scratch  : the uint8 [N][H][ow] intermediate, wiw_resample_u8_scratch_bytes(N, H, ow) bytes, needed (and touched) only
 *              when BOTH passes run; its content afterwards is unspecified
 *   alignment: one byte for the uint8 operands and the scratch, four bytes for fp32 operands and the tables
 *   N, H, W, oh, ow > 0; N * max(H, oh) <= 2^30 rows.  No atomics: bit-repeatable.
 */
#ifndef WIW_RESAMPLE_H
#define WIW_RESAMPLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WIW_RESAMPLE_MAX_TAPS 64

/* bytes of `scratch` for N planes, H source rows, ow output columns; 0 if an argument is not positive */
int64_t wiw_resample_u8_scratch_bytes(int N, int H, int ow);

/* uint8 planes -> uint8 planes */
int wiw_resample_u8(void* stream, const uint8_t* src, int64_t src_plane_stride, int64_t src_row_stride, int N, int H, int W,
                    uint8_t* dst, int64_t dst_plane_stride, int64_t dst_row_stride, int oh, int ow, const int32_t* coef_h,
                    const int32_t* bounds_h, int ksize_h, const int32_t* coef_v, const int32_t* bounds_v, int ksize_v,
                    uint8_t* scratch);

/* The same operation on the decoder's fp32 frames (N = frames x channels planes, in [-1, 1]): every load applies the frame
 * quantisation  u = rint(clamp(x / 2 + 0.5, 0, 1) * 255)  in fp32, in that order, round half to even (x / 2 is exact, so the
 * fused x * 0.5 + 0.5 rounds identically; the product by 255 is rounded on its own).  No uint8 copy of the source is made. */
int wiw_frames_resample_u8(void* stream, const float* src, int64_t src_plane_stride, int64_t src_row_stride, int N, int H,
                           int W, uint8_t* dst, int64_t dst_plane_stride, int64_t dst_row_stride, int oh, int ow,
                           const int32_t* coef_h, const int32_t* bounds_h, int ksize_h, const int32_t* coef_v,
                           const int32_t* bounds_v, int ksize_v, uint8_t* scratch);

/* dst[i] = lut[src[i]], i < n: uint8 -> fp32 through a 256-entry table (the host's own `2 * (u / 255) - 1`); n > 0 */
int wiw_u8_to_f32_lut(void* stream, const uint8_t* src, int64_t n, const float* lut, float* dst);

#ifdef __cplusplus
}
#endif
#endif /* WIW_RESAMPLE_H */
