// Per-plane SSIM and squared error (include/wiw_metrics.h; the reference's evaluation/FVD/calculate_ssim.py `ssim` and
// calculate_psnr.py `img_psnr`) for gfx950 (MI355X): the frame metrics of a validation pass where the decoded frames already
// are, in HBM, instead of five float64 filter2D passes per channel per frame on the host.
//
// Two launches:
//   * tiles: a block owns TH x TW = 24 x 32 pixels of a plane's SSIM map.  It stages the (TH + 10) x (TW + 10) samples under
//     them of both operands in LDS as fp32 (a uint8 sample through the caller's 256-entry table, also in LDS), filters the five
//     moments x, y, x^2, y^2, xy along the rows into fp64 maps in LDS (34 x 32 x 5 doubles = 42.5 KiB: what bounds the tile),
//     then along the columns in registers, evaluates the SSIM expression and sums it.  The squared error is summed at the
//     staging loads over the pixels the tile OWNS — its own TH x TW, extended to the plane's edge for the last tile row /
//     column — so every pixel counts once.  One (SSIM sum, squared-error sum) pair per tile goes to `partials`.
//   * planes: a block per plane adds that plane's tile pairs, thread-strided and then as a tree: a fixed order that depends
//     on H and W only.
// Every operation after the load is fp64; fused multiply-adds are used in the two filters and nowhere in the SSIM expression,
// whose cancellation (E[x^2] - mu^2 against C2 = 9e-4) is then the reference's own.  About 110 DFMA per pixel: LDS- and
// HBM-bound.  A sample is fetched by 1.86 tiles on average; the repeats are neighbouring blocks' and come from the caches.
// No atomics, plain loads and stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

#include "../../include/wiw_metrics.h"

namespace {

constexpr int WIN = WIW_METRICS_WINDOW, HALO = WIN - 1;
constexpr int TH = 24, TW = 32, THREADS = 256;
constexpr int IN_H = TH + HALO, IN_W = TW + HALO;
constexpr int64_t MAX_GRID = 1 << 20;
static_assert((TW & (TW - 1)) == 0, "items are split into row and column by shift and mask");

// k[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum: cv2.getGaussianKernel(11, 1.5), normalised in double
__constant__ double GAUSS[WIN] = {0.00102838008447911,  0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
                                  0.2130055377112537,   0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
                                  0.03600077212843083,  0.007598758135239185, 0.00102838008447911};

struct Planes {          // element offsets: row r of plane p at p * plane + r * row
    const void* base;
    int64_t plane, row;
    int kind;
};

WIW_DEV float load_sample(const Planes& s, int64_t off, const float* lut) {
    return s.kind == WIW_METRICS_U8 ? lut[((const uint8_t*)s.base)[off]] : ((const float*)s.base)[off];
}

WIW_DEV double ssim_point(double mu1, double mu2, double e11, double e22, double e12) {
#pragma clang fp contract(off)
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const double s11 = e11 - mu1_sq, s22 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2));
}

// sum of v over the block into thread 0, by a tree over `red` [THREADS]: a fixed order
WIW_DEV double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// tile t = (p * tiles_y + ty) * tiles_x + tx -> partials[2 t] = sum of the tile's SSIM map, partials[2 t + 1] = its squared error
__global__ __launch_bounds__(THREADS) void metrics_tile_kernel(Planes A, Planes B, const float* __restrict__ lut_g, int64_t tiles,
                                                               int tiles_y, int tiles_x, int H, int W,
                                                               double* __restrict__ partials) {
    __shared__ float sA[IN_H][IN_W], sB[IN_H][IN_W];
    __shared__ float lut[256];
    __shared__ double M[5][IN_H][TW];          // row-filtered moments; afterwards the reduction's scratch
    const int tid = (int)threadIdx.x;
    if (lut_g != nullptr) lut[tid] = lut_g[tid];          // THREADS == 256; null only when no operand is uint8
    double w[WIN];
#pragma unroll
    for (int k = 0; k < WIN; ++k) w[k] = GAUSS[k];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tx = (int)(t % tiles_x), ty = (int)((t / tiles_x) % tiles_y);
        const int64_t p = t / ((int64_t)tiles_x * tiles_y);
        const int y0 = ty * TH, x0 = tx * TW;
        // the pixels whose squared error this tile counts: its own TH x TW, to the plane's edge in the last tile row / column
        const int own_h = ty == tiles_y - 1 ? H - y0 : TH, own_w = tx == tiles_x - 1 ? W - x0 : TW;
        __syncthreads();          // the table is in place; the previous tile's reduction has been read
        double se = 0.0;
        for (int i = tid; i < IN_H * IN_W; i += THREADS) {
            const int r = i / IN_W, c = i % IN_W;
            float va = 0.0f, vb = 0.0f;          // outside the plane: feeds only windows that are not evaluated
            if (y0 + r < H && x0 + c < W) {
                va = load_sample(A, p * A.plane + (int64_t)(y0 + r) * A.row + (x0 + c), lut);
                vb = load_sample(B, p * B.plane + (int64_t)(y0 + r) * B.row + (x0 + c), lut);
                if (r < own_h && c < own_w) {
                    const double d = (double)va - (double)vb;
                    se += d * d;
                }
            }
            sA[r][c] = va;
            sB[r][c] = vb;
        }
        __syncthreads();
        for (int i = tid; i < IN_H * TW; i += THREADS) {          // along the rows
            const int r = i / TW, c = i & (TW - 1);
            double m1 = 0.0, m2 = 0.0, m11 = 0.0, m22 = 0.0, m12 = 0.0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const double x = (double)sA[r][c + k], y = (double)sB[r][c + k];
                m1 = __builtin_fma(w[k], x, m1);
                m2 = __builtin_fma(w[k], y, m2);
                m11 = __builtin_fma(w[k], x * x, m11);
                m22 = __builtin_fma(w[k], y * y, m22);
                m12 = __builtin_fma(w[k], x * y, m12);
            }
            M[0][r][c] = m1; M[1][r][c] = m2; M[2][r][c] = m11; M[3][r][c] = m22; M[4][r][c] = m12;
        }
        __syncthreads();
        double ss = 0.0;
        for (int i = tid; i < TH * TW; i += THREADS) {          // along the columns, and the SSIM map
            const int r = i / TW, c = i & (TW - 1);
            if (y0 + r >= H - HALO || x0 + c >= W - HALO) continue;
            double m[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < WIN; ++k) acc = __builtin_fma(w[k], M[q][r + k][c], acc);
                m[q] = acc;
            }
            ss += ssim_point(m[0], m[1], m[2], m[3], m[4]);
        }
        __syncthreads();          // M is read: it becomes the reduction's scratch
        double* red = &M[0][0][0];
        ss = block_sum(ss, red);
        __syncthreads();
        se = block_sum(se, red);
        if (tid == 0) {
            partials[2 * t] = ss;
            partials[2 * t + 1] = se;
        }
    }
}

// out[p] = (sum of the plane's tile SSIM sums / valid pixels, sum of its tile squared errors)
__global__ __launch_bounds__(THREADS) void metrics_plane_kernel(const double* __restrict__ partials, int N, int per_plane,
                                                                double valid, double* __restrict__ out) {
    __shared__ double red[THREADS];
    for (int p = blockIdx.x; p < N; p += gridDim.x) {
        const double* src = partials + (int64_t)p * per_plane * 2;
        double ss = 0.0, se = 0.0;
        for (int j = (int)threadIdx.x; j < per_plane; j += THREADS) {
            ss += src[2 * j];
            se += src[2 * j + 1];
        }
        __syncthreads();
        ss = block_sum(ss, red);
        __syncthreads();
        se = block_sum(se, red);
        if (threadIdx.x == 0) {
            out[2 * (int64_t)p] = ss / valid;
            out[2 * (int64_t)p + 1] = se;
        }
    }
}

bool sizes_ok(int N, int H, int W) { return N > 0 && H >= WIN && W >= WIN && (int64_t)N * H <= (1 << 30); }

}  // namespace

extern "C" int64_t wiw_frame_metrics_partials(int N, int H, int W) {
    if (!sizes_ok(N, H, W)) return 0;
    const int64_t tiles_y = (H - HALO + TH - 1) / TH, tiles_x = (W - HALO + TW - 1) / TW;
    return 2 * (int64_t)N * tiles_y * tiles_x;
}

extern "C" int wiw_frame_metrics(void* stream_, const void* a, int a_kind, int64_t a_plane_stride, int64_t a_row_stride,
                                 const void* b, int b_kind, int64_t b_plane_stride, int64_t b_row_stride, const float* lut, int N,
                                 int H, int W, double* partials, double* out) {
    WIW_REQUIRE(a && b && partials && out, "frame_metrics: null pointer");
    WIW_REQUIRE((a_kind == WIW_METRICS_F32 || a_kind == WIW_METRICS_U8) && (b_kind == WIW_METRICS_F32 || b_kind == WIW_METRICS_U8),
                "frame_metrics: kind must be WIW_METRICS_F32 (0) or WIW_METRICS_U8 (1)");
    WIW_REQUIRE(lut || (a_kind == WIW_METRICS_F32 && b_kind == WIW_METRICS_F32), "frame_metrics: a uint8 operand needs the lut");
    WIW_REQUIRE(N > 0, "frame_metrics: N must be positive");
    WIW_REQUIRE(H >= WIN && W >= WIN, "frame_metrics: H and W must be at least 11 (one window)");
    WIW_REQUIRE((int64_t)N * H <= (1 << 30), "frame_metrics: more than 2^30 rows");
    WIW_REQUIRE(a_row_stride >= W && b_row_stride >= W, "frame_metrics: a row stride is smaller than a row");
    WIW_REQUIRE(a_plane_stride >= (int64_t)H * a_row_stride && b_plane_stride >= (int64_t)H * b_row_stride,
                "frame_metrics: a plane stride is smaller than a plane");
    WIW_REQUIRE((a_kind == WIW_METRICS_U8 || ((uintptr_t)a & 3) == 0) && (b_kind == WIW_METRICS_U8 || ((uintptr_t)b & 3) == 0),
                "frame_metrics: fp32 planes must be 4-byte aligned");
    WIW_REQUIRE(((uintptr_t)lut & 3) == 0, "frame_metrics: the lut must be 4-byte aligned");
    WIW_REQUIRE((((uintptr_t)partials | (uintptr_t)out) & 7) == 0, "frame_metrics: partials and out must be 8-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const int tiles_y = (H - HALO + TH - 1) / TH, tiles_x = (W - HALO + TW - 1) / TW;
    WIW_REQUIRE((int64_t)tiles_y * tiles_x <= INT32_MAX, "frame_metrics: too many tiles per plane");
    const int64_t tiles = (int64_t)N * tiles_y * tiles_x;
    const Planes A{a, a_plane_stride, a_row_stride, a_kind}, B{b, b_plane_stride, b_row_stride, b_kind};
    hipLaunchKernelGGL(metrics_tile_kernel, dim3((unsigned)(tiles < MAX_GRID ? tiles : MAX_GRID)), dim3(THREADS), 0, stream, A, B,
                       lut, tiles, tiles_y, tiles_x, H, W, partials);
    hipLaunchKernelGGL(metrics_plane_kernel, dim3((unsigned)(N < MAX_GRID ? N : MAX_GRID)), dim3(THREADS), 0, stream,
                       (const double*)partials, N, tiles_y * tiles_x, (double)(H - HALO) * (double)(W - HALO), out);
    return wiw_check_launch("wiw_frame_metrics");
}
