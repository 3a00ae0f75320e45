/* Value-range statistics of a tensor on the device (csrc/range.hip) — an additive companion of include/wiw_svd.h (same
 * conventions: device pointers, caller-owned memory, `stream` a hipStream_t or NULL, WIW_OK or a negative WIW_E* code,
 * wiw_last_error() for the message; nothing is launched on error; no allocation and no synchronisation, so every entry point
 * may be captured into a graph).  Exported with the same entry points by both builds of the library (bf16: libwiwsvd.so,
 * fp16: libwiwsvd_f16.so: `f32 = 0` reads the build's own 16-bit storage type); WIW_ABI_VERSION is unchanged.  Every launching
 * entry point declared here has a case in tests/test_hip_range_footprint.py (tests/test_range.py checks it).
 *
 * What a serving worker needs to notice that it produced garbage (a NaN latent becomes black or arbitrary bytes at the frame
 * quantisation) and what a new checkpoint needs to be judged for 16-bit headroom: per SEGMENT of a strided 2-D tensor the
 * counts of NaN, +-inf, zero, "hot" and "tiny" elements, the largest and the smallest non-zero finite magnitude, and
 * optionally a 64-bin histogram of floor(log2 |x|).  Both 16-bit types convert to fp32 exactly and no sum of values is formed
 * (counts, a max and a min only), so every number is exact.
 *
 *   X        : rows x cols elements, row r at X + r * ld ELEMENTS (ld >= cols; r * ld is formed in 64 bits); elements
 *              between cols and ld are never read into the statistics.  f32 = 0: the library's 16-bit storage type, X
 *              2-byte aligned; f32 = 1: fp32, X 4-byte aligned.  Nothing more is asked of X's alignment: 16-byte loads are
 *              used where a row piece allows, scalar loads on its head and tail.
 *   segments : consecutive groups of rows_per_segment rows (rows % rows_per_segment == 0): out[s], hist[s] describe rows
 *              [s * rows_per_segment, (s + 1) * rows_per_segment).  A segment's numbers depend on neither the number of
 *              segments nor the other segments.
 *   hot, tiny: thresholds of n_hot (finite, |x| >= hot) and n_tiny (finite, 0 < |x| < tiny): finite and not negative
 *   partials : wiw_range_stats_partials(rows, cols, rows_per_segment, hist != NULL) BYTES of scratch, 8-byte aligned: one
 *              record per block, written by the first launch and reduced per segment, in a fixed order, by the second; its
 *              content afterwards is unspecified
 *   out      : WiwRangeStats [segments], 8-byte aligned; nothing else is written
 *   hist     : NULL, or uint64 [segments][WIW_RANGE_BINS], 8-byte aligned
 * No global atomics and no hand-off between workgroups inside a launch: two runs give the same bytes.
 */
#ifndef WIW_RANGE_H
#define WIW_RANGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct WiwRangeStats { /* one per segment */
    uint64_t n_nan, n_inf;     /* NaN (any payload), +-inf */
    uint64_t n_zero;           /* +0 and -0 */
    uint64_t n_hot;            /* finite, |x| >= hot */
    uint64_t n_tiny;           /* finite, 0 < |x| < tiny */
    float absmax;              /* largest finite |x|; 0 if the segment has no finite element */
    float absmin;              /* smallest non-zero finite |x|; +inf if none */
} WiwRangeStats;

#define WIW_RANGE_BINS 64 /* bin = clamp(floor(log2|x|) + 32, 0, 63) over finite non-zero x */

/* bytes of `partials`; 0 if rows, cols or rows_per_segment <= 0 or rows % rows_per_segment != 0.  Launches nothing. */
int64_t wiw_range_stats_partials(int64_t rows, int cols, int64_t rows_per_segment, int hist);

/* out[s] (and hist[s]) = the statistics of segment s of X */
int wiw_range_stats(void* stream, const void* X, int f32, int64_t rows, int cols, int64_t ld, int64_t rows_per_segment, float hot,
                    float tiny, void* partials, WiwRangeStats* out, uint64_t* hist);

#ifdef __cplusplus
}
#endif
#endif /* WIW_RANGE_H */
