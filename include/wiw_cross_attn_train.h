/* Training-side entry points of the few-keys cross-attention (csrc/cross_attn_bwd.hip) — an additive companion of
 * include/wiw_svd.h (same conventions: device pointers, `stream` a hipStream_t or NULL, WIW_OK or a negative WIW_E* code,
 * wiw_last_error() for the message; nothing is launched on error).  Exported by both builds of the library (bf16:
 * libwiwsvd.so, fp16: libwiwsvd_f16.so); WIW_ABI_VERSION is unchanged.  Every launching entry point declared here has a
 * case in tests/test_hip_cross_attn_bwd_footprint.py (tests/test_cross_attn_train_abi.py checks it).
 *
 * Backward of wiw_cross_attn_fewkeys_bf16 (checkpoints fine-tuned with --num_past_obs P, 2 <= P <= 8: the cross-attention
 * of BasicTransformerBlock / TemporalBasicTransformerBlock over P conditioning tokens, dp/models/attention.py:545-551,
 * 740-743).  For every row m of an item, head h (64 channels) and key p < P, with w = softmax_p(scale * q . k_p) RECOMPUTED
 * (nothing is saved by the forward):
 *
 *     dP_p = dO . v_p                (64-term dot over the head)
 *     delta = sum_p w_p dP_p
 *     dS_p = w_p (dP_p - delta)
 *     dQ   = scale sum_p dS_p k_p                                  -> 16-bit [rows][heads*64], row stride lddq
 *     dK_p = scale sum_m dS_p[m] q[m],  dV_p = sum_m w_p[m] dO[m]  -> fp32 [rows / rows_per_item][P][heads*64], contiguous
 *
 *   Q, dO   : 16-bit [rows][heads*64], row strides ldq / lddo (multiples of 8, >= heads*64), read once
 *   K, V    : 16-bit [rows / rows_per_item][P][heads*64] contiguous — the operands of the forward
 *   partial : fp32 scratch of wiw_cross_attn_fewkeys_bwd_partials(rows, rows_per_item, heads, P) floats, fully written:
 *             one [2][P][heads*64] block of (dK | dV) sums per thread block
 *   1 <= P <= 8, heads * 64 <= 2048, rows a multiple of rows_per_item, all pointers 16-byte aligned.
 *
 * Bit-repeatable, no atomics: a thread sums its rows in ascending order, a block sums its row slots in slot order through
 * LDS, and a second launch sums the blocks of an item in ascending order.  P = 1: dQ = 0 and dK = 0 exactly, dV = sum_m dO.
 */
#ifndef WIW_CROSS_ATTN_TRAIN_H
#define WIW_CROSS_ATTN_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t wiw_cross_attn_fewkeys_bwd_partials(int64_t rows, int rows_per_item, int heads, int P); /* floats; 0: bad arguments */
int wiw_cross_attn_fewkeys_bwd_bf16(void* stream, const void* Q, int ldq, const void* K, const void* V, const void* dO, int lddo,
                                    void* dQ, int lddq, float* dK, float* dV, float* partial, int64_t rows, int rows_per_item,
                                    int heads, int P, float scale);

#ifdef __cplusplus
}
#endif
#endif /* WIW_CROSS_ATTN_TRAIN_H */
