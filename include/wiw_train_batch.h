/* Batched entry point of the fine-tuning step (csrc/train_batch.hip) — an additive companion of include/wiw_svd.h (same
 * conventions: device pointers, `stream` a hipStream_t or NULL, WIW_OK or a negative WIW_E* code, wiw_last_error() for the
 * message; nothing is launched on error).  Exported by both builds of the library (bf16: libwiwsvd.so, fp16:
 * libwiwsvd_f16.so); WIW_ABI_VERSION is unchanged.  Every launching entry point declared here has a case in
 * tests/test_hip_train_batch_footprint.py (tests/test_train_batch.py checks it).
 *
 * EDM loss of B independent samples and the gradient of their MEAN loss (train_svd.py:940-952 with --per_gpu_batch_size B):
 * sample b has its own noise level sigmas[b], read on the device, and with
 *
 *     c_out = -sigma / sqrt(sigma^2 + 1),  c_skip = 1 / (sigma^2 + 1),  w = (1 + sigma^2) / sigma^2     (fp32, this order)
 *     d     = pred * c_out + c_skip * noisy - target
 *
 *   partial[b][k] = the k-th block's sum of w d^2 over its grid-stride share of sample b — bit for bit what
 *                   wiw_edm_loss_grad writes for that sample alone with the same n_partial; loss_b = sum_k partial[b][k] /
 *                   n_per_sample, loss = mean_b loss_b
 *   grad          = ((2 w c_out / n_per_sample) d) * (1.0f / B): the single-sample gradient, then ONE more fp32 product
 *                   (B = 1: the bits of wiw_edm_loss_grad; B a power of two: its bits scaled exactly)
 *
 *   pred, noisy, target, grad : fp32 [B][n_per_sample] contiguous
 *   sigmas                    : fp32 [B] on the DEVICE; a sample whose sigma is not > 0 gets NaN in its partials and gradient
 *   partial                   : fp32 [B][n_partial], fully written
 *   1 <= B <= 64, n_per_sample > 0, 1 <= n_partial <= 4096; pointers 4-byte aligned.  No atomics: bit-repeatable.
 */
#ifndef WIW_TRAIN_BATCH_H
#define WIW_TRAIN_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int wiw_edm_loss_grad_batched(void* stream, const float* pred, const float* noisy, const float* target, int64_t n_per_sample,
                              int B, const float* sigmas, float* grad, float* partial, int n_partial);

#ifdef __cplusplus
}
#endif
#endif /* WIW_TRAIN_BATCH_H */
