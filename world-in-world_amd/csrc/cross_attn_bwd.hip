// Backward of the cross-attention over a FEW keys (csrc/cross_attn.hip; include/wiw_cross_attn_train.h) for gfx950 (MI355X):
// the gradient of the attn2 of both transformer blocks when a checkpoint is fine-tuned with --num_past_obs P, 2 <= P <= 8
// (train_svd.py:359, 889-894).  With w = softmax_p(scale q . k_p) recomputed per row and head:
//
//   dP_p = dO . v_p,  delta = sum_p w_p dP_p,  dS_p = w_p (dP_p - delta)
//   dQ = scale sum_p dS_p k_p           dK_p = scale sum_m dS_p[m] q[m]           dV_p = sum_m w_p[m] dO[m]
//
// The thread mapping is the forward's: a thread = one 8-channel chunk of every key, a head = 8 aligned lanes (two 64-term dots
// per key: 8 FMAs per lane and three cross-lane steps each), the item's K and V stay in registers.  Q and dO stream through
// once, dQ is written once — HBM-bound at ~3 rows C 2 bytes.  dK / dV are sums over ALL rows of an item: a thread adds its rows
// in ascending order into 2 x 8 x 8 fp32 registers, the block adds its row slots in slot order through one LDS buffer (reused
// pass by pass over p) and writes ONE fp32 partial [2][P][C]; a second launch adds the blocks of an item in ascending order.
// No atomics: two launches on the same operands give the same bits.
#include "common.h"

#include "../../include/wiw_cross_attn_train.h"

namespace {

constexpr int CAB_MAXP = 8;
constexpr int CAB_THREADS = 256;

WIW_DEV float oct_sum(float v) {   // sum over the 8 aligned lanes of a head
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// rows per block: every row slot (256 / (C / 8) of them) walks ~32 rows, so the K / V fetch, the P reduction passes and the
// partial of a block are paid once per >= 64 rows; never more than the forward's 256
int rows_per_block_of(int C, int rows_per_item) {
    const int rp = CAB_THREADS / (C >> 3);
    int rpb = 32 * rp;
    if (rpb < 64) rpb = 64;
    if (rpb > 256) rpb = 256;
    if (rpb > rows_per_item) rpb = rows_per_item;
    return rpb;
}

__global__ __launch_bounds__(CAB_THREADS) void cross_attn_fewkeys_bwd_kernel(
    const uint16_t* __restrict__ Q, int ldq, const uint16_t* __restrict__ K, const uint16_t* __restrict__ V,
    const uint16_t* __restrict__ dO, int lddo, uint16_t* __restrict__ dQ, int lddq, float* __restrict__ partial, int C, int P,
    int rows_per_item, int rows_per_block, float scale, float scale_log2e) {
    // [row slot][dK C | dV C] of ONE key: rp * 2C <= 256 * 16 floats (16 KiB)
    __shared__ __attribute__((aligned(16))) float red[CAB_THREADS * 16];
    const int tid = threadIdx.x;
    const int chunks = C >> 3;                  // <= 256 (launcher)
    const int rp = CAB_THREADS / chunks;
    const int ci = tid % chunks, rl = tid / chunks;
    const int item = blockIdx.y;
    const int r0 = blockIdx.x * rows_per_block;
    int r1 = r0 + rows_per_block;
    if (r1 > rows_per_item) r1 = rows_per_item;
    // surplus threads (256 % chunks: whole 8-lane groups, never part of a live head) stay for the barriers below and touch
    // no memory; the live ones are tid < rp * chunks
    const bool live = rl < rp;
    uint4 kq[CAB_MAXP], vq[CAB_MAXP];
    float dk[CAB_MAXP][8], dv[CAB_MAXP][8];
#pragma unroll
    for (int p = 0; p < CAB_MAXP; ++p) {
        kq[p] = make_uint4(0u, 0u, 0u, 0u);
        vq[p] = make_uint4(0u, 0u, 0u, 0u);
        if (live && p < P) {
            kq[p] = *(const uint4*)(K + ((int64_t)item * P + p) * C + ci * 8);
            vq[p] = *(const uint4*)(V + ((int64_t)item * P + p) * C + ci * 8);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) dk[p][e] = dv[p][e] = 0.f;
    }
    if (live) {
        const int64_t base = (int64_t)item * rows_per_item;
        for (int r = r0 + rl; r < r1; r += rp) {   // the 8 lanes of a head share rl: they leave the loop together
            float q[8], g[8];
            unpack8(*(const uint4*)(Q + (base + r) * ldq + ci * 8), q);
            unpack8(*(const uint4*)(dO + (base + r) * lddo + ci * 8), g);
            float s[CAB_MAXP], dp[CAB_MAXP], mx = -INFINITY;
#pragma unroll
            for (int p = 0; p < CAB_MAXP; ++p) {
                s[p] = -INFINITY;
                dp[p] = 0.f;
                if (p < P) {
                    float k[8], v[8], a = 0.f, b = 0.f;
                    unpack8(kq[p], k);
                    unpack8(vq[p], v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        a = __builtin_fmaf(q[e], k[e], a);
                        b = __builtin_fmaf(g[e], v[e], b);
                    }
                    s[p] = oct_sum(a) * scale_log2e;
                    dp[p] = oct_sum(b);
                    mx = fmaxf(mx, s[p]);
                }
            }
            float l = 0.f, w[CAB_MAXP];
#pragma unroll
            for (int p = 0; p < CAB_MAXP; ++p) {
                w[p] = p < P ? __builtin_amdgcn_exp2f(s[p] - mx) : 0.f;
                l += w[p];
            }
            const float inv = 1.0f / l;
            float delta = 0.f;
#pragma unroll
            for (int p = 0; p < CAB_MAXP; ++p) {
                w[p] *= inv;
                delta = __builtin_fmaf(w[p], dp[p], delta);
            }
            float dq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p < CAB_MAXP; ++p) {
                if (p < P) {
                    const float ds = w[p] * (dp[p] - delta);
                    float k[8];
                    unpack8(kq[p], k);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        dq[e] = __builtin_fmaf(ds, k[e], dq[e]);
                        dk[p][e] = __builtin_fmaf(ds, q[e], dk[p][e]);
                        dv[p][e] = __builtin_fmaf(w[p], g[e], dv[p][e]);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) dq[e] *= scale;
            *(uint4*)(dQ + (base + r) * lddq + ci * 8) = pack8(dq);
        }
    }
    // ---- block sums of dK / dV, one key per pass: slot rl of the buffer <- this thread's registers; then live thread j adds
    // the rp slots of the elements j, j + nlive, ... in slot order.  P is uniform: every thread meets every barrier.
    const int C2 = 2 * C, nlive = rp * chunks;
    float* out = partial + ((int64_t)item * gridDim.x + blockIdx.x) * (int64_t)(2 * P) * C;
#pragma unroll
    for (int p = 0; p < CAB_MAXP; ++p) {
        if (p < P) {
            if (live) {
                float* slot = red + rl * C2 + ci * 8;
                *(float4*)(slot) = make_float4(dk[p][0], dk[p][1], dk[p][2], dk[p][3]);
                *(float4*)(slot + 4) = make_float4(dk[p][4], dk[p][5], dk[p][6], dk[p][7]);
                *(float4*)(slot + C) = make_float4(dv[p][0], dv[p][1], dv[p][2], dv[p][3]);
                *(float4*)(slot + C + 4) = make_float4(dv[p][4], dv[p][5], dv[p][6], dv[p][7]);
            }
            __syncthreads();
            if (live) {
                for (int j = tid; j < C2; j += nlive) {
                    float acc = 0.f;
                    for (int sl = 0; sl < rp; ++sl) acc += red[sl * C2 + j];
                    const int kind = j >= C ? 1 : 0;
                    out[(kind * P + p) * C + (j - kind * C)] = acc;
                }
            }
            __syncthreads();
        }
    }
}

// dK[item][p][c] = scale * sum over the blocks of the item (ascending), dV the same without the scale
__global__ __launch_bounds__(CAB_THREADS) void cross_attn_fewkeys_bwd_finish_kernel(const float* __restrict__ partial,
                                                                                    float* __restrict__ dK, float* __restrict__ dV,
                                                                                    int items, int splits, int PC, float scale) {
    const int64_t i = (int64_t)blockIdx.x * CAB_THREADS + threadIdx.x;      // (item, kind, p * C + c)
    if (i >= (int64_t)items * 2 * PC) return;
    const int item = (int)(i / (2 * PC));
    const int rem = (int)(i - (int64_t)item * 2 * PC);
    const float* src = partial + (int64_t)item * splits * 2 * PC + rem;
    float acc = 0.f;
    for (int s = 0; s < splits; ++s) acc += src[(int64_t)s * 2 * PC];
    if (rem < PC)
        dK[(int64_t)item * PC + rem] = acc * scale;
    else
        dV[(int64_t)item * PC + rem - PC] = acc;
}

}  // namespace

extern "C" int64_t wiw_cross_attn_fewkeys_bwd_partials(int64_t rows, int rows_per_item, int heads, int P) {
    if (heads <= 0 || heads * 64 > 2048 || P < 1 || P > CAB_MAXP || rows <= 0 || rows_per_item <= 0 || rows % rows_per_item) return 0;
    const int C = heads * 64;
    const int rpb = rows_per_block_of(C, rows_per_item);
    const int64_t splits = (rows_per_item + rpb - 1) / rpb;
    return (rows / rows_per_item) * splits * 2 * P * C;
}

extern "C" int wiw_cross_attn_fewkeys_bwd_bf16(void* stream, const void* Q, int ldq, const void* K, const void* V, const void* dO,
                                               int lddo, void* dQ, int lddq, float* dK, float* dV, float* partial, int64_t rows,
                                               int rows_per_item, int heads, int P, float scale) {
    WIW_REQUIRE(Q && K && V && dO && dQ && dK && dV && partial, "cross_attn_fewkeys_bwd: null pointer");
    WIW_REQUIRE(heads > 0 && heads * 64 <= 2048, "cross_attn_fewkeys_bwd: heads * 64 channels, at most 2048");
    WIW_REQUIRE(P >= 1 && P <= CAB_MAXP, "cross_attn_fewkeys_bwd: 1 <= P <= 8 keys per item");
    WIW_REQUIRE(rows > 0 && rows_per_item > 0 && rows % rows_per_item == 0, "cross_attn_fewkeys_bwd: rows must be whole items");
    const int C = heads * 64;
    WIW_REQUIRE(ldq % 8 == 0 && ldq >= C && lddo % 8 == 0 && lddo >= C && lddq % 8 == 0 && lddq >= C,
                "cross_attn_fewkeys_bwd: ldq / lddo / lddq must be multiples of 8 and >= C");
    WIW_REQUIRE((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)dO | (uintptr_t)dQ | (uintptr_t)dK | (uintptr_t)dV |
                  (uintptr_t)partial) & 15) == 0, "cross_attn_fewkeys_bwd: pointers must be 16-byte aligned");
    WIW_REQUIRE(rows / rows_per_item <= 65535, "cross_attn_fewkeys_bwd: at most 65535 items");
    const int items = (int)(rows / rows_per_item);
    const int rpb = rows_per_block_of(C, rows_per_item);
    const int splits = (rows_per_item + rpb - 1) / rpb;
    hipLaunchKernelGGL(cross_attn_fewkeys_bwd_kernel, dim3((unsigned)splits, (unsigned)items), dim3(CAB_THREADS), 0,
                       (hipStream_t)stream, (const uint16_t*)Q, ldq, (const uint16_t*)K, (const uint16_t*)V, (const uint16_t*)dO, lddo,
                       (uint16_t*)dQ, lddq, partial, C, P, rows_per_item, rpb, scale, scale * 1.4426950408889634f);
    const int rc = wiw_check_launch("wiw_cross_attn_fewkeys_bwd_bf16");
    if (rc != WIW_OK) return rc;
    const int64_t n = (int64_t)items * 2 * P * C;
    hipLaunchKernelGGL(cross_attn_fewkeys_bwd_finish_kernel, dim3((unsigned)((n + CAB_THREADS - 1) / CAB_THREADS)), dim3(CAB_THREADS), 0,
                       (hipStream_t)stream, (const float*)partial, dK, dV, items, splits, P * C, scale);
    return wiw_check_launch("wiw_cross_attn_fewkeys_bwd_bf16 (finish)");
}
