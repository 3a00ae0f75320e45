/* Per-plane SSIM and squared error on the device (csrc/metrics.hip) — an additive companion of include/wiw_svd.h (same
 * conventions: device pointers, caller-owned memory, `stream` a hipStream_t or NULL, WIW_OK or a negative WIW_E* code,
 * wiw_last_error() for the message; nothing is launched on error; no allocation and no synchronisation, so every entry point
 * may be captured into a graph).  Exported with the same entry points by both builds of the library (bf16: libwiwsvd.so,
 * fp16: libwiwsvd_f16.so: nothing here touches the 16-bit type); WIW_ABI_VERSION is unchanged.  Every launching entry point
 * declared here has a case in tests/test_hip_metrics_footprint.py (tests/test_metrics.py checks it).
 *
 * The two frame metrics the reference's validation logs (evaluation/FVD/calculate_ssim.py:6-23, calculate_psnr.py:6-15), per
 * plane pair (a, b) of H x W samples in [0, 1]:
 *
 *   out[p][0] = mean over the (H - 10) x (W - 10) valid region of
 *                   (2 mu_a mu_b + C1) (2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1) (s_aa + s_bb + C2)),
 *               mu_x = G * x, s_xy = G * (x y) - mu_x mu_y, G = outer(k, k), k[i] ~ exp(-(i - 5)^2 / (2 * 1.5^2)), 11 taps,
 *               normalised in double; C1 = 0.01^2, C2 = 0.03^2.  Only windows that lie inside the plane are evaluated (the
 *               reference crops its filtered maps by [5:-5, 5:-5]): there is no border handling.
 *   out[p][1] = sum over the whole plane of ((double)a - (double)b)^2.
 *
 * Every operation after the load is fp64 (s_xx = E[x^2] - mu^2 cancels against C2 = 9e-4; fp32 costs up to 5e-5 of SSIM).  The
 * window is applied separably, rows then columns.
 *
 *   kind     : WIW_METRICS_F32 — fp32 samples, used as they are; WIW_METRICS_U8 — a uint8 sample u is lut[u]
 *   lut      : fp32 [256] from the host, np.arange(256, dtype=float32) / float32(255): the float32 quotient the reference's
 *              to_tensor produces, bit for bit (the kernel never divides).  May be NULL when both operands are fp32.
 *   planes   : N planes of H rows of W samples; row r of plane p starts at p * plane_stride + r * row_stride ELEMENTS;
 *              row_stride >= W, plane_stride >= H * row_stride (of a and b independently; a and b may be the same memory)
 *   partials : wiw_frame_metrics_partials(N, H, W) doubles of scratch: one (SSIM sum, squared-error sum) pair per tile, written
 *              by the first launch and summed in a fixed order by the second; its content afterwards is unspecified
 *   out      : double [N][2], nothing else is written
 *   alignment: one byte for uint8 operands, four bytes for fp32 operands and the LUT, eight bytes for partials and out
 *   N > 0; H, W >= 11; N * H <= 2^30 rows.  No atomics: bit-repeatable, and a plane's two numbers depend on neither N nor
 *   the other planes of the launch.
 */
#ifndef WIW_METRICS_H
#define WIW_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WIW_METRICS_F32 0
#define WIW_METRICS_U8 1
#define WIW_METRICS_WINDOW 11

/* doubles of `partials` for N planes of H x W; 0 if N <= 0, H or W < 11, or N * H > 2^30 */
int64_t wiw_frame_metrics_partials(int N, int H, int W);

/* out[p] = (mean SSIM, sum of squared differences) of planes a[p], b[p], p < N */
int wiw_frame_metrics(void* stream, const void* a, int a_kind, int64_t a_plane_stride, int64_t a_row_stride, const void* b,
                      int b_kind, int64_t b_plane_stride, int64_t b_row_stride, const float* lut, int N, int H, int W,
                      double* partials, double* out);

#ifdef __cplusplus
}
#endif
#endif /* WIW_METRICS_H */
