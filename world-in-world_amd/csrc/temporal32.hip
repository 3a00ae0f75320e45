// Temporal self-attention for prediction horizons of up to 32 frames (gfx950): the 32-frame-slot siblings of
// wiw_temporal_attn_block_bf16 (temporal.hip, T <= 14) and wiw_attn_temporal_bf16 (attention.hip, T <= 16).  Those two keep
// their limits and their code; a 25-frame (SVD-XT) UNet runs on the entries of this file.
//
//   O[(b,t,s)][h*64 + d] = sum_t' softmax_t'( q(b,t,s,h) . k(b,t',s,h) * scale ) v(b,t',s,h)[d]        rows m = (b*T + t)*S + s
//
// Both kernels give one wave ONE spatial site of one head: its 32 frame slots are two 16-row MFMA fragments (frames 0..15 and
// 16..31), S^T = K . Q^T is 32 x 32 = four 16x16 blocks, the softmax runs over the <= 32 keys a query column holds across the
// two key fragments (4 lanes x 8 registers), and P . V uses the full K = 32 of v_mfma_f32_16x16x32 (in the 16-slot kernels
// keys 16..31 are zero padding).  The K index of that MFMA is enumerated key(fq, e) = 16*(e>>2) + 4*fq + (e&3), so that the two
// S^T accumulator fragments of a query column ARE its B operand and (fused form) the two V accumulator fragments ARE the A operand.
//
// Padding: frame slots >= T read frame T-1 again (real, finite rows: never memory the tensor does not own), their scores are
// masked to -inf before the maximum (probability exactly 0) and their V rows are set to 0 before the product, so nothing of a
// padding slot reaches O.  Sites >= S of a tile's tail read site S-1 and store nothing.
//
// Fused form (wiw_temporal_attn_block32_bf16) = LayerNorm -> per-head Q|K|V projection -> attention on the raw rows X, with the
// operands `unet.pack_temporal_qkv` already produces (gamma-folded tiled weights + fold vectors, see temporal.hip): work item =
// (8 consecutive sites of one batch item, head) = the same 256 x 192 x C GEMM as the 16-slot kernel, turned sideways: a wave's
// 2 x 12 accumulator fragments hold Q, K and V of its one site.  Deliberately plain: W tiles go through a
// two-stage LDS buffer filled by LDS-DMA one K tile ahead, A rows global -> VGPR one K tile ahead (a wave's rows are private),
// one block barrier per K tile, LayerNorm row moments by v_dot2c from the A fragments the MFMAs consume.
#include <stdlib.h>

#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int BK = 64;
constexpr int NF = 12;                    // 16-column fragments of a head: 4 q | 4 k | 4 v
constexpr int W_ROWS = NF * 16;           // 192
constexpr int W_BYTES = W_ROWS * BK * 2;  // 24576: one K tile of one head's weights
constexpr int SITES = 8;                  // sites per work item = waves per block

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
// LDS-DMA (16 B per lane, destination = wave-uniform LDS address + 16 * lane) in the asm form of temporal.hip, M0 saved and
// restored inside the statement: hipcc puts `s_waitcnt vmcnt(0)` between the BUILTIN and the next LDS read it cannot prove
// disjoint, which would serialise the fill of one stage with the MFMAs on the other.  No VGPR destination; completion is
// waited for by hand (vmcnt(0) + block barrier at the top of every K tile).
WIW_DEV void glds16(const char* g, uint32_t lds_addr) {
    const uint32_t lds = __builtin_amdgcn_readfirstlane(lds_addr);
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
}

union frag_u { uint32_t u[4]; bf16x8 v; };

// The 32 x 32 attention of one site from its operands, shared by both kernels.
//   ko / qo[f][kk]: K / Q rows of frames 16f + (lane & 15) as MFMA operands of the d half kk (any d enumeration both share);
//   vo(nb):         V^T operand of the 16-d block nb: lane (d = 16nb + (lane & 15), fq) holds V[key(fq, e)][d], keys >= T zero;
//   store(nb, fqr, pk): receives O[frame 16fqr + (lane & 15)][16nb + 4fq .. +3] as 4 packed 16-bit values.
template <class VO, class ST>
WIW_DEV void attention32_core(const frag_u (&ko)[2][2], const frag_u (&qo)[2][2], int T, float scale_log2e, int lane, VO&& vo, ST&& store) {
    const int fq = lane >> 4;
    f32x4 st[2][2];   // [key fragment][query fragment]; lane: query column lane & 15, keys 16fk + 4fq + r
#pragma unroll
    for (int fk = 0; fk < 2; ++fk)
#pragma unroll
        for (int fqr = 0; fqr < 2; ++fqr) {
            f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
            z = WIW_MFMA(ko[fk][0].v, qo[fqr][0].v, z);
            st[fk][fqr] = WIW_MFMA(ko[fk][1].v, qo[fqr][1].v, z);
        }
    frag_u po[2];
    float inv[2];
#pragma unroll
    for (int fqr = 0; fqr < 2; ++fqr) {
        float sv[2][4], mx = -INFINITY;
#pragma unroll
        for (int fk = 0; fk < 2; ++fk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sv[fk][r] = (16 * fk + 4 * fq + r) < T ? st[fk][fqr][r] * scale_log2e : -INFINITY;
                mx = fmaxf(mx, sv[fk][r]);
            }
        mx = xor32_max(xor16_max(mx));   // key 0 is never masked: the maximum is a real score
        float pr[2][4], l = 0.f;
#pragma unroll
        for (int fk = 0; fk < 2; ++fk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pr[fk][r] = __builtin_amdgcn_exp2f(sv[fk][r] - mx);   // masked: exp2(-inf) = 0
                l += pr[fk][r];
            }
        l = xor32_sum(xor16_sum(l));
        inv[fqr] = __builtin_amdgcn_rcpf(l);
        po[fqr].u[0] = pack2bf(pr[0][0], pr[0][1]); po[fqr].u[1] = pack2bf(pr[0][2], pr[0][3]);
        po[fqr].u[2] = pack2bf(pr[1][0], pr[1][1]); po[fqr].u[3] = pack2bf(pr[1][2], pr[1][3]);
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const frag_u va = vo(nb);
#pragma unroll
        for (int fqr = 0; fqr < 2; ++fqr) {
            f32x4 ot = f32x4{0.f, 0.f, 0.f, 0.f};
            ot = WIW_MFMA(va.v, po[fqr].v, ot);   // O^T block: lane = query column, rows d = 16nb + 4fq + r
            uint2 pk;
            pk.x = pack2bf(ot[0] * inv[fqr], ot[1] * inv[fqr]);
            pk.y = pack2bf(ot[2] * inv[fqr], ot[3] * inv[fqr]);
            store(nb, fqr, pk);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Unfused: QKV [m][3C] in, one wave per (batch item, site, head).  K and Q fragments straight from global (16 B per lane),
// V staged in a per-wave LDS tile and read back transposed, as attn_temporal_kernel does for 16 slots.
// ---------------------------------------------------------------------------------------------
constexpr int TV_LD = 72;   // 16-bit elements per staged V row (144 B: 16-B aligned, skewed banks)

__global__ __launch_bounds__(256) void attn_temporal32_kernel(const uint16_t* __restrict__ QKV, int ldqkv, uint16_t* __restrict__ O,
                                                               int ldo, int T, int S, int heads, int64_t total, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) uint16_t vst[4][32 * TV_LD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t task = (int64_t)blockIdx.x * 4 + wave;
    if (task >= total) return;     // wave-uniform; no block-level barrier below
    const int C = heads * 64;
    const int h = (int)(task % heads);
    const int64_t site = task / heads;           // b*S + s
    const int s = (int)(site % S);
    const int64_t b = site / S;
    const int fr = lane & 15, fq = lane >> 4;
    const int64_t frame_stride = (int64_t)S * ldqkv;
    const uint16_t* base = QKV + ((b * T) * S + s) * ldqkv + h * 64;

    frag_u qo[2][2], ko[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int t = 16 * f + fr < T ? 16 * f + fr : T - 1;
        const uint16_t* src = base + t * frame_stride + fq * 8;
        qo[f][0].v = *(const bf16x8*)(src); qo[f][1].v = *(const bf16x8*)(src + 32);
        ko[f][0].v = *(const bf16x8*)(src + C); ko[f][1].v = *(const bf16x8*)(src + C + 32);
    }
    // V rows -> LDS (row = key, 64 d); rows >= T are zero
    uint16_t* vs = vst[wave];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = i * 8 + (lane >> 3);
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if (key < T) v = *(const uint4*)(base + key * frame_stride + 2 * C + (lane & 7) * 8);
        *(uint4*)(vs + key * TV_LD + (lane & 7) * 8) = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint16_t* obase = O + ((b * T) * S + s) * ldo + h * 64 + fq * 4;
    const int64_t o_stride = (int64_t)S * ldo;
    attention32_core(ko, qo, T, scale_log2e, lane,
        [&](int nb) {
            frag_u va;
            const int dcol = nb * 16 + fr;
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const int k0 = 16 * (e >> 2) + 4 * fq + (e & 3);
                const uint32_t e0 = vs[k0 * TV_LD + dcol], e1 = vs[(k0 + 1) * TV_LD + dcol];
                va.u[e >> 1] = e0 | (e1 << 16);
            }
            return va;
        },
        [&](int nb, int fqr, uint2 pk) {
            const int t = 16 * fqr + fr;
            if (t < T) *(uint2*)(obase + t * o_stride + nb * 16) = pk;
        });
}

// ---------------------------------------------------------------------------------------------
// Fused: LayerNorm (folded) + Q|K|V projection + attention.
// ---------------------------------------------------------------------------------------------
struct Temporal32Args {
    const uint16_t* X;      // 16-bit [batch*T*S][C]
    const uint16_t* W;      // 16-bit [heads*192][C] TILED (1-KiB blocks [row / 8][k tile][8 rows x 128 B, chunk c at c ^ (row & 7)])
    const float* fold;      // fp32 [heads][512]     s[192] | t[192] | pad
    uint16_t* O;            // 16-bit [batch*T*S][ldo]
    int ldo, batch, T, S, C, heads;
    int tiles_per_batch;    // ceil(S / SITES)
    int items;              // batch * tiles_per_batch * heads
    float eps, scale_log2e, inv_c;
};

__global__ __launch_bounds__(SITES * 64, 2) void temporal_block32_kernel(const Temporal32Args p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * W_BYTES];
    __shared__ __attribute__((aligned(16))) float fs[2 * W_ROWS];   // the head's fold vectors s[192] | t[192]
    const uint32_t smem_lds = (uint32_t)(uintptr_t)(lptr_t)smem;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fq = lane >> 4;
    // item = site tile * heads + head: the heads of a tile run at about the same time; blocks renumbered so that they also
    // share an XCD's L2 (block b is observed on XCD b % 8).  Placement changes speed only.
    const int nb = gridDim.x;
    int item = blockIdx.x;
    if ((nb & 7) == 0) item = (blockIdx.x & 7) * (nb >> 3) + (blockIdx.x >> 3);
    const int h = item % p.heads, mt = item / p.heads;
    const int b = mt / p.tiles_per_batch, s0 = (mt - b * p.tiles_per_batch) * SITES;
    const int nk = p.C / BK;
    const int site = s0 + wave;
    const bool site_ok = site < p.S;
    const int site_c = site_ok ? site : p.S - 1;

    if (tid < 2 * W_ROWS / 4) ((float4*)fs)[tid] = ((const float4*)(p.fold + (size_t)h * 512))[tid];   // visible after the first barrier

    // A rows of this wave (32-bit byte offsets: the launcher checks X < 4 GiB): fragment f = frames 16f + frow
    const char* const Xb = (const char*)p.X;
    uint32_t a_ofs[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int fr = 16 * f + frow < p.T ? 16 * f + frow : p.T - 1;
        const int64_t m = ((int64_t)b * p.T + fr) * p.S + site_c;
        a_ofs[f] = (uint32_t)((m * p.C + fq * 8) * 2);
    }
    auto load_a = [&](bf16x8 (&dst)[2][2], int kt) {   // [k-step][fragment]
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const char* src = Xb + (a_ofs[f] + (uint32_t)(kt * (BK * 2)));
            dst[0][f] = *(const bf16x8*)(src);
            dst[1][f] = *(const bf16x8*)(src + 64);
        }
    };
    // W tile kt of head h: 24 contiguous KiB blocks, three per wave
    const char* const Wh = (const char*)p.W + (size_t)h * (W_ROWS / 8) * nk * 1024 + lane * 16;
    auto fill_w = [&](int buf, int kt) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int rb = wave * 3 + i;
            glds16(Wh + ((size_t)rb * nk + kt) * 1024, smem_lds + (uint32_t)(buf * W_BYTES + rb * 1024));
        }
    };
    const int w_off = frow * 128 + ((fq ^ (frow & 7)) << 4);

    f32x4 acc[2][NF];
    float sum1[2] = {0.f, 0.f}, sum2[2] = {0.f, 0.f};
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int ni = 0; ni < NF; ++ni) acc[f][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 fa[2][2], fn[2][2];
    // one K tile on the A fragments `cur`; the next tile's A rows go to `nxt` (ping-pong with compile-time indices)
    auto ktile = [&](const bf16x8 (&cur)[2][2], bf16x8 (&nxt)[2][2], int kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of W tile kt has landed ...
        __syncthreads();                                    // ... and everybody's; all reads of the other buffer are done
        if (kt + 1 < nk) {
            load_a(nxt, kt + 1);
            fill_w((kt + 1) & 1, kt + 1);
        }
        const char* sW = smem + (kt & 1) * W_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fb[NF];
#pragma unroll
            for (int ni = 0; ni < NF; ++ni) fb[ni] = *(const bf16x8*)(sW + ni * 2048 + (w_off ^ (kk << 6)));
#pragma unroll
            for (int ni = 0; ni < 8; ++ni)
#pragma unroll
                for (int f = 0; f < 2; ++f)   // q, k: swapped operands -> lane = frame frow, columns 16*ni + 4*fq + r
                    acc[f][ni] = WIW_MFMA(fb[ni], cur[kk][f], acc[f][ni]);
#pragma unroll
            for (int ni = 8; ni < NF; ++ni)
#pragma unroll
                for (int f = 0; f < 2; ++f)   // v: lane = column (d) frow, rows = frames 16f + 4*fq + r
                    acc[f][ni] = WIW_MFMA(cur[kk][f], fb[ni], acc[f][ni]);
            // LayerNorm row moments from the A fragments just consumed (each lane sees 8 of the 32 k-values of its row)
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                frag_u x;
                x.v = cur[kk][f];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sum1[f] = dot2_acc(x.u[j], WIW_ONE16 * 0x10001u, sum1[f]);
                    sum2[f] = dot2_acc(x.u[j], x.u[j], sum2[f]);
                }
            }
        }
    };
    fill_w(0, 0);
    load_a(fa, 0);
    for (int kt = 0; kt < nk; kt += 2) {
        ktile(fa, fn, kt);
        if (kt + 1 < nk) ktile(fn, fa, kt + 1);
    }

    // ---- epilogue (per wave, registers only).  LayerNorm fold: x . W_n = rs * (acc_n - mean * s_n) + t_n
    float rs[2], nrm[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const float s1 = xor32_sum(xor16_sum(sum1[f])), s2 = xor32_sum(xor16_sum(sum2[f]));
        const float mean = s1 * p.inv_c;
        float var = __builtin_fmaf(-mean, mean, s2 * p.inv_c);
        var = var < 0.f ? 0.f : var;
        rs[f] = rsqrtf(var + p.eps);
        nrm[f] = -rs[f] * mean;
#pragma unroll
        for (int ni = 0; ni < 8; ++ni) {
            const float4 sv = *(const float4*)(fs + ni * 16 + fq * 4);
            const float4 tv = *(const float4*)(fs + W_ROWS + ni * 16 + fq * 4);
            acc[f][ni][0] = __builtin_fmaf(acc[f][ni][0], rs[f], __builtin_fmaf(nrm[f], sv.x, tv.x));
            acc[f][ni][1] = __builtin_fmaf(acc[f][ni][1], rs[f], __builtin_fmaf(nrm[f], sv.y, tv.y));
            acc[f][ni][2] = __builtin_fmaf(acc[f][ni][2], rs[f], __builtin_fmaf(nrm[f], sv.z, tv.z));
            acc[f][ni][3] = __builtin_fmaf(acc[f][ni][3], rs[f], __builtin_fmaf(nrm[f], sv.w, tv.w));
        }
    }
    // Q / K operands: d(fq, e) = 32kk + 16*(e>>2) + 4*fq + (e&3) — two accumulator fragments are one operand
    frag_u qo[2][2], ko[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            qo[f][kk].u[0] = pack2bf(acc[f][2 * kk][0], acc[f][2 * kk][1]);
            qo[f][kk].u[1] = pack2bf(acc[f][2 * kk][2], acc[f][2 * kk][3]);
            qo[f][kk].u[2] = pack2bf(acc[f][2 * kk + 1][0], acc[f][2 * kk + 1][1]);
            qo[f][kk].u[3] = pack2bf(acc[f][2 * kk + 1][2], acc[f][2 * kk + 1][3]);
            ko[f][kk].u[0] = pack2bf(acc[f][4 + 2 * kk][0], acc[f][4 + 2 * kk][1]);
            ko[f][kk].u[1] = pack2bf(acc[f][4 + 2 * kk][2], acc[f][4 + 2 * kk][3]);
            ko[f][kk].u[2] = pack2bf(acc[f][4 + 2 * kk + 1][0], acc[f][4 + 2 * kk + 1][1]);
            ko[f][kk].u[3] = pack2bf(acc[f][4 + 2 * kk + 1][2], acc[f][4 + 2 * kk + 1][3]);
        }
    // v: lane = d, registers = frames 16f + 4*fq + r -> needs the statistics of THOSE rows (held by lanes frow' = 4*fq + r)
    float rsv[2][4], nrv[2][4];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rsv[f][r] = __shfl(rs[f], fq * 4 + r, 64);
            nrv[f][r] = __shfl(nrm[f], fq * 4 + r, 64);
        }
    char* const Ob = (char*)p.O;
    attention32_core(ko, qo, p.T, p.scale_log2e, lane,
        [&](int nbk) {
            const float svv = fs[128 + nbk * 16 + frow], tvv = fs[W_ROWS + 128 + nbk * 16 + frow];
            frag_u vo;
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                float vv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = __builtin_fmaf(acc[f][8 + nbk][r], rsv[f][r], __builtin_fmaf(nrv[f][r], svv, tvv));
                    vv[r] = (16 * f + 4 * fq + r) < p.T ? x : 0.f;   // a padding slot's V never meets a probability
                }
                vo.u[2 * f] = pack2bf(vv[0], vv[1]);
                vo.u[2 * f + 1] = pack2bf(vv[2], vv[3]);
            }
            return vo;
        },
        [&](int nbk, int fqr, uint2 pk) {
            const int t = 16 * fqr + frow;
            if (t < p.T && site_ok) {   // 32-bit byte offsets (the launcher checks O < 4 GiB)
                const uint32_t m = (uint32_t)((b * p.T + t) * p.S + site);
                const uint32_t off = (m * (uint32_t)p.ldo + (uint32_t)(h * 64 + nbk * 16 + fq * 4)) * 2u;
                *(uint2*)(Ob + off) = pk;
            }
        });
}

}  // namespace

extern "C" int wiw_attn_temporal32_bf16(void* stream, const void* QKV, int ldqkv, void* O, int ldo, int batch, int T, int S,
                                        int heads, float scale) {
    WIW_REQUIRE(QKV && O, "attn_temporal32: null pointer");
    WIW_REQUIRE(batch > 0 && S > 0 && heads > 0, "attn_temporal32: bad sizes");
    WIW_REQUIRE(T >= 1 && T <= 32, "attn_temporal32: 1 <= T <= 32");
    WIW_REQUIRE(ldqkv % 8 == 0 && ldqkv >= 3 * heads * 64 && ldo % 4 == 0 && ldo >= heads * 64, "attn_temporal32: misaligned strides");
    WIW_REQUIRE((((uintptr_t)QKV & 15) | ((uintptr_t)O & 7)) == 0, "attn_temporal32: QKV must be 16-byte and O 8-byte aligned");
    const int64_t total = (int64_t)batch * S * heads;
    const int64_t nb = (total + 3) / 4;
    WIW_REQUIRE(nb < (1ll << 31), "attn_temporal32: grid too large");
    hipLaunchKernelGGL(attn_temporal32_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)QKV, ldqkv,
                       (uint16_t*)O, ldo, T, S, heads, total, scale * LOG2E);
    return wiw_check_launch("wiw_attn_temporal32_bf16");
}

extern "C" int wiw_temporal_attn_block32_bf16(void* stream, const void* X, const void* Wqkv, const float* fold, void* O, int ldo,
                                              int batch, int T, int S, int heads, float eps, float scale) {
    WIW_REQUIRE(X && Wqkv && fold && O, "temporal_attn_block32: null pointer");
    WIW_REQUIRE(batch > 0 && S > 0 && heads > 0, "temporal_attn_block32: bad sizes");
    WIW_REQUIRE(T >= 1 && T <= 32, "temporal_attn_block32: 1 <= T <= 32");
    WIW_REQUIRE(ldo % 8 == 0 && ldo >= heads * 64, "temporal_attn_block32: ldo must be a multiple of 8 and >= C");
    WIW_REQUIRE((((uintptr_t)X | (uintptr_t)Wqkv | (uintptr_t)fold | (uintptr_t)O) & 15) == 0,
                "temporal_attn_block32: pointers must be 16-byte aligned");
    Temporal32Args a;
    a.X = (const uint16_t*)X; a.W = (const uint16_t*)Wqkv; a.fold = fold; a.O = (uint16_t*)O;
    a.ldo = ldo; a.batch = batch; a.T = T; a.S = S; a.C = heads * 64; a.heads = heads;
    a.tiles_per_batch = (S + SITES - 1) / SITES;
    const int64_t items = (int64_t)batch * a.tiles_per_batch * heads;
    WIW_REQUIRE(items < (1ll << 31), "temporal_attn_block32: too many work items");
    WIW_REQUIRE((int64_t)batch * T * S * heads * 64 * 2 < (1ll << 32), "temporal_attn_block32: X must be < 4 GiB (32-bit source offsets)");
    WIW_REQUIRE((int64_t)batch * T * S * ldo * 2 < (1ll << 32), "temporal_attn_block32: O must be < 4 GiB (32-bit destination offsets)");
    a.items = (int)items;
    a.eps = eps; a.scale_log2e = scale * LOG2E; a.inv_c = 1.0f / (float)a.C;
    hipLaunchKernelGGL(temporal_block32_kernel, dim3((unsigned)items), dim3(SITES * 64), 0, (hipStream_t)stream, a);
    return wiw_check_launch("wiw_temporal_attn_block32_bf16");
}
