// Value-range statistics of a strided 2-D tensor (include/wiw_range.h) for gfx950 (MI355X): what the serving guard reads per
// candidate (did this rollout produce a NaN or an inf?) and what the range probe records per activation tensor (how close to
// the 16-bit type's largest finite value does it sit?).  One read of the tensor, nothing written back into it.
//
// Two launches:
//   * blocks: a segment (rows_per_segment consecutive rows) is cut into UNITS — a row, or a CHUNK = 4096-element piece of a
//     row that is longer — and a block owns UNITS_PER_BLOCK = 8 consecutive units of ONE segment, two per wave.  A wave reads
//     its unit with 16-byte loads from the first 16-byte boundary on, and with one scalar load per lane on the head before it
//     and the tail after it: X is only element-aligned and a row start (r * ld) may fall anywhere.  When ld == cols the rows of
//     a segment are one contiguous run and the host hands the segment over as ONE row, so that a narrow tensor (cols = 320)
//     still fills the lanes.  Every value is classified on its fp32 BIT PATTERN (bf16 and fp16 convert exactly), so no
//     floating-point mode — denormal flushing included — takes part.  Per-thread counters go into the block's LDS record
//     (integer adds, max, min: the order cannot matter) and from there to `partials`.
//   * segments: one block per segment adds that segment's records, thread-strided and then as a tree.
// No global atomics, no hand-off between workgroups: bit-repeatable, and a segment's numbers depend on nothing but its rows.
// Measured: 1.85 TB/s on a 258 048 x 320 16-bit tensor and 3.7 TB/s on 793 MB of fp32, against 4.9 TB/s
// (read + write) of a device copy: the rate follows the ELEMENT count (0.93 T elements/s either way), i.e. the classification
// (about 16 integer VALU instructions per element), not HBM, bounds it.  With a histogram every finite non-zero element
// also costs one LDS atomic (0.59 TB/s on the same 16-bit tensor): the probe's cost, the guard passes hist = NULL.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

#include "../../include/wiw_range.h"

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int CHUNK = 4096;             // elements of a unit at most
constexpr int UNITS_PER_BLOCK = 8;
constexpr int64_t MAX_GRID = 1 << 20;
constexpr int REC_WORDS = 6;            // uint64: nan, inf, zero, hot, tiny, (absmax bits << 32 | absmin bits)
constexpr int REC_BYTES = REC_WORDS * 8, REC_BYTES_HIST = REC_BYTES + WIW_RANGE_BINS * 4;
constexpr uint32_t INF_BITS = 0x7f800000u;
static_assert(sizeof(WiwRangeStats) == 48, "five counters and two floats, no padding");

struct Acc {
    uint32_t nan = 0, inf = 0, zero = 0, hot = 0, tiny = 0, mx = 0, mn = INF_BITS;
};

// one element, as the bits of its fp32 value
template <bool HIST>
WIW_DEV void classify(uint32_t bits, uint32_t hotb, uint32_t tinyb, Acc& s, uint32_t* hist) {
    const uint32_t a = bits & 0x7fffffffu;
    const bool finite = a < INF_BITS, nonzero_finite = (a - 1u) < (INF_BITS - 1u);
    s.nan += a > INF_BITS;
    s.inf += a == INF_BITS;
    s.zero += a == 0u;
    s.hot += finite && a >= hotb;
    s.tiny += nonzero_finite && a < tinyb;
    s.mx = max(s.mx, finite ? a : 0u);
    s.mn = min(s.mn, nonzero_finite ? a : INF_BITS);
    if constexpr (HIST) {
        if (nonzero_finite) {          // floor(log2 |x|) = exponent field - 127; fp32 subnormals (field 0) fall into bin 0
            const int bin = min(max((int)(a >> 23) - 127 + 32, 0), WIW_RANGE_BINS - 1);
            atomicAdd(&hist[bin], 1u);
        }
    }
}

template <bool F32>
WIW_DEV uint32_t load_bits(const void* p, int64_t i) {
    if constexpr (F32) return ((const uint32_t*)p)[i];
    else return __float_as_uint(bf2f(((const uint16_t*)p)[i]));
}

// block `blk` = (segment, j): units [j * UNITS_PER_BLOCK, (j + 1) * UNITS_PER_BLOCK) of the segment's R x C view (row stride LD)
template <bool F32, bool HIST>
__global__ __launch_bounds__(THREADS) void range_block_kernel(const void* __restrict__ X, int64_t R, int64_t C, int64_t LD,
                                                             int64_t chunks_per_row, int64_t units, int64_t blocks_per_seg,
                                                             int64_t nblocks, uint32_t hotb, uint32_t tinyb,
                                                             uint8_t* __restrict__ partials) {
    constexpr int ES = F32 ? 4 : 2, VE = 16 / ES, REC = HIST ? REC_BYTES_HIST : REC_BYTES;
    __shared__ uint32_t s_cnt[5], s_mx, s_mn;
    __shared__ uint32_t s_hist[HIST ? WAVES : 1][WIW_RANGE_BINS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* my_hist = s_hist[HIST ? wave : 0];
    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int64_t seg = blk / blocks_per_seg, j = blk % blocks_per_seg;
        if (tid < 5) s_cnt[tid] = 0u;
        if (tid == 5) s_mx = 0u;
        if (tid == 6) s_mn = INF_BITS;
        if constexpr (HIST) s_hist[wave][lane] = 0u;          // WIW_RANGE_BINS == 64 lanes
        __syncthreads();
        Acc s;
        const int64_t u_end = min(units, (j + 1) * UNITS_PER_BLOCK);
        for (int64_t u = j * UNITS_PER_BLOCK + wave; u < u_end; u += WAVES) {
            const int64_t r = u / chunks_per_row, c0 = (u % chunks_per_row) * CHUNK;
            const int n = (int)min((int64_t)CHUNK, C - c0);
            const uint8_t* p = (const uint8_t*)X + ((seg * R + r) * LD + c0) * ES;
            const int head = min(n, (int)((16u - ((uintptr_t)p & 15u)) & 15u) / ES);          // elements before the 16-byte boundary
            const int nv = (n - head) / VE, tail0 = head + nv * VE;
            if (lane < head) classify<HIST>(load_bits<F32>(p, lane), hotb, tinyb, s, my_hist);
            const uint4* pv = (const uint4*)(p + (int64_t)head * ES);
            for (int v = lane; v < nv; v += 64) {
                const uint4 q = pv[v];
                if constexpr (F32) {
                    classify<HIST>(q.x, hotb, tinyb, s, my_hist);
                    classify<HIST>(q.y, hotb, tinyb, s, my_hist);
                    classify<HIST>(q.z, hotb, tinyb, s, my_hist);
                    classify<HIST>(q.w, hotb, tinyb, s, my_hist);
                } else {
                    float f[8];
                    unpack8(q, f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) classify<HIST>(__float_as_uint(f[e]), hotb, tinyb, s, my_hist);
                }
            }
            if (lane < n - tail0) classify<HIST>(load_bits<F32>(p, tail0 + lane), hotb, tinyb, s, my_hist);
        }
        atomicAdd(&s_cnt[0], s.nan);
        atomicAdd(&s_cnt[1], s.inf);
        atomicAdd(&s_cnt[2], s.zero);
        atomicAdd(&s_cnt[3], s.hot);
        atomicAdd(&s_cnt[4], s.tiny);
        atomicMax(&s_mx, s.mx);
        atomicMin(&s_mn, s.mn);
        __syncthreads();
        uint8_t* rec = partials + blk * REC;
        if (tid < 5) ((uint64_t*)rec)[tid] = s_cnt[tid];
        if (tid == 5) ((uint64_t*)rec)[5] = ((uint64_t)s_mx << 32) | s_mn;
        if constexpr (HIST) {
            if (tid < WIW_RANGE_BINS) {
                uint32_t h = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) h += s_hist[w][tid];
                ((uint32_t*)(rec + REC_BYTES))[tid] = h;
            }
        }
        __syncthreads();          // the record is read: the next block of this workgroup clears it
    }
}

template <typename Op>
WIW_DEV uint64_t block_reduce(uint64_t v, uint64_t* red, Op op) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}

// out[seg] (and hist[seg]) from the segment's blocks_per_seg records
template <bool HIST>
__global__ __launch_bounds__(THREADS) void range_segment_kernel(const uint8_t* __restrict__ partials, int64_t segments,
                                                               int64_t blocks_per_seg, WiwRangeStats* __restrict__ out,
                                                               uint64_t* __restrict__ hist) {
    constexpr int REC = HIST ? REC_BYTES_HIST : REC_BYTES;
    __shared__ uint64_t red[THREADS];
    const int tid = (int)threadIdx.x;
    const auto add = [](uint64_t a, uint64_t b) { return a + b; };
    for (int64_t seg = blockIdx.x; seg < segments; seg += gridDim.x) {
        const uint8_t* base = partials + seg * blocks_per_seg * REC;
        uint64_t c[5] = {0, 0, 0, 0, 0};
        uint32_t mx = 0u, mn = INF_BITS;
        for (int64_t j = tid; j < blocks_per_seg; j += THREADS) {
            const uint64_t* rec = (const uint64_t*)(base + j * REC);
#pragma unroll
            for (int q = 0; q < 5; ++q) c[q] += rec[q];
            mx = max(mx, (uint32_t)(rec[5] >> 32));
            mn = min(mn, (uint32_t)rec[5]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) c[q] = block_reduce(c[q], red, add);
        const uint64_t m = block_reduce(mx, red, [](uint64_t a, uint64_t b) { return a > b ? a : b; });
        const uint64_t n = block_reduce(mn, red, [](uint64_t a, uint64_t b) { return a < b ? a : b; });
        if (tid == 0) {
            WiwRangeStats r;
            r.n_nan = c[0]; r.n_inf = c[1]; r.n_zero = c[2]; r.n_hot = c[3]; r.n_tiny = c[4];
            r.absmax = __uint_as_float((uint32_t)m);
            r.absmin = __uint_as_float((uint32_t)n);
            out[seg] = r;
        }
        if constexpr (HIST) {          // bin = tid % 64, a quarter of the records per group of 64 threads
            uint64_t h = 0;
            for (int64_t j = tid >> 6; j < blocks_per_seg; j += WAVES)
                h += ((const uint32_t*)(base + j * REC + REC_BYTES))[tid & 63];
            __syncthreads();
            red[tid] = h;
            __syncthreads();
            if (tid < WIW_RANGE_BINS) {
                uint64_t t = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) t += red[tid + w * 64];
                hist[seg * WIW_RANGE_BINS + tid] = t;
            }
        }
    }
}

// blocks per segment of an R x C view
int64_t blocks_of(int64_t R, int64_t C) {
    const int64_t units = R * ((C + CHUNK - 1) / CHUNK);
    return (units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK;
}

bool sizes_ok(int64_t rows, int cols, int64_t rps) {
    return rows > 0 && cols > 0 && rps > 0 && rows % rps == 0 && rows <= (INT64_MAX >> 4) / cols;
}

template <bool F32, bool HIST>
void launch(hipStream_t stream, const void* X, int64_t segments, int64_t R, int64_t C, int64_t LD, uint32_t hotb, uint32_t tinyb,
            uint8_t* partials, WiwRangeStats* out, uint64_t* hist) {
    const int64_t cpr = (C + CHUNK - 1) / CHUNK, units = R * cpr, bps = blocks_of(R, C), nblocks = segments * bps;
    hipLaunchKernelGGL((range_block_kernel<F32, HIST>), dim3((unsigned)(nblocks < MAX_GRID ? nblocks : MAX_GRID)), dim3(THREADS),
                       0, stream, X, R, C, LD, cpr, units, bps, nblocks, hotb, tinyb, partials);
    hipLaunchKernelGGL((range_segment_kernel<HIST>), dim3((unsigned)(segments < MAX_GRID ? segments : MAX_GRID)), dim3(THREADS), 0,
                       stream, (const uint8_t*)partials, segments, bps, out, hist);
}

}  // namespace

extern "C" int64_t wiw_range_stats_partials(int64_t rows, int cols, int64_t rows_per_segment, int hist) {
    if (!sizes_ok(rows, cols, rows_per_segment)) return 0;
    // the strided view (a unit never crosses a row) needs the most blocks; the contiguous one (ld == cols) fewer
    return (rows / rows_per_segment) * blocks_of(rows_per_segment, cols) * (hist ? REC_BYTES_HIST : REC_BYTES);
}

extern "C" int wiw_range_stats(void* stream_, const void* X, int f32, int64_t rows, int cols, int64_t ld, int64_t rows_per_segment,
                               float hot, float tiny, void* partials, WiwRangeStats* out, uint64_t* hist) {
    WIW_REQUIRE(X && partials && out, "range_stats: null pointer");
    WIW_REQUIRE(f32 == 0 || f32 == 1, "range_stats: f32 must be 0 (the library's 16-bit type) or 1");
    WIW_REQUIRE(rows > 0 && cols > 0, "range_stats: rows and cols must be positive");
    WIW_REQUIRE(ld >= cols, "range_stats: ld is smaller than a row");
    WIW_REQUIRE(rows_per_segment > 0 && rows % rows_per_segment == 0, "range_stats: rows must be a positive multiple of rows_per_segment");
    WIW_REQUIRE(sizes_ok(rows, cols, rows_per_segment) && rows <= (INT64_MAX >> 4) / ld, "range_stats: rows * ld overflows");
    // finite and not negative (-0 counts as 0); NaN fails both comparisons
    WIW_REQUIRE(hot >= 0.0f && hot < __builtin_inff() && tiny >= 0.0f && tiny < __builtin_inff(),
                "range_stats: hot and tiny must be finite and not negative");
    WIW_REQUIRE(((uintptr_t)X & (f32 ? 3 : 1)) == 0, "range_stats: X must be element-aligned");
    WIW_REQUIRE((((uintptr_t)partials | (uintptr_t)out | (uintptr_t)hist) & 7) == 0, "range_stats: partials, out and hist must be 8-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t hotb = __builtin_bit_cast(uint32_t, hot) & 0x7fffffffu, tinyb = __builtin_bit_cast(uint32_t, tiny) & 0x7fffffffu;
    const int64_t segments = rows / rows_per_segment;
    // contiguous rows: a segment is one long row
    const int64_t R = ld == cols ? 1 : rows_per_segment, C = ld == cols ? rows_per_segment * cols : cols, LD = ld == cols ? C : ld;
    uint8_t* part = (uint8_t*)partials;
    if (f32) {
        if (hist) launch<true, true>(stream, X, segments, R, C, LD, hotb, tinyb, part, out, hist);
        else launch<true, false>(stream, X, segments, R, C, LD, hotb, tinyb, part, out, hist);
    } else {
        if (hist) launch<false, true>(stream, X, segments, R, C, LD, hotb, tinyb, part, out, hist);
        else launch<false, false>(stream, X, segments, R, C, LD, hotb, tinyb, part, out, hist);
    }
    return wiw_check_launch("wiw_range_stats");
}
