// EDM loss of a BATCH of samples with the gradient of their mean (include/wiw_train_batch.h; train_svd.py:940-952 with
// --per_gpu_batch_size B) for gfx950 (MI355X).  blockIdx.y is the sample; the n_partial blocks of a sample walk it with the
// grid-stride partition, the per-element fp32 expressions and the in-block reduction of edm_loss_kernel (csrc/train.hip), so
// partial[b][.] carries the bits wiw_edm_loss_grad writes for that sample alone.  The three EDM coefficients come from the
// device-resident sigmas[b] through the expressions the single-sample entry point evaluates on the host — products and sums
// rounded one by one (no fma contraction: the host has none), IEEE division and square root.  The gradient of the mean loss
// is the single-sample value times fp32(1 / B), a separate rounded product.  HBM-bound: 16 bytes per element, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

#include "../../include/wiw_train_batch.h"

namespace {

struct EdmCoef {
    float c_out, c_skip, w;
};

WIW_DEV EdmCoef edm_coefficients(float sigma) {
#pragma clang fp contract(off)
    EdmCoef c;
    if (!(sigma > 0.0f)) {               // the single-sample entry point refuses these on the host; here the sample turns NaN
        c.c_out = c.c_skip = c.w = __builtin_nanf("");
        return c;
    }
    const float s2 = sigma * sigma;
    c.c_out = -sigma / sqrtf(s2 + 1.0f);
    c.c_skip = 1.0f / (s2 + 1.0f);
    c.w = (1.0f + s2) / s2;
    return c;
}

__global__ __launch_bounds__(256) void edm_loss_batched_kernel(const float* __restrict__ pred, const float* __restrict__ noisy,
                                                                const float* __restrict__ target, int64_t n,
                                                                const float* __restrict__ sigmas, float inv_b,
                                                                float* __restrict__ grad, float* __restrict__ partial) {
    __shared__ float red[256];
    const int64_t base = (int64_t)blockIdx.y * n;
    pred += base;
    noisy += base;
    target += base;
    grad += base;
    const EdmCoef k = edm_coefficients(sigmas[blockIdx.y]);
    const float c_out = k.c_out, c_skip = k.c_skip, w = k.w;
    float acc = w != w ? w : 0.f;        // a refused sigma: NaN in every partial of the sample, also from a block without elements
    const float scale = 2.0f * w * c_out / (float)n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float d = pred[i] * c_out + c_skip * noisy[i] - target[i];
        acc += w * d * d;
        float g = scale * d;
        asm volatile("" : "+v"(g));      // the single-sample gradient is rounded before the 1 / B product
        grad[i] = g * inv_b;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

}  // namespace

extern "C" int wiw_edm_loss_grad_batched(void* stream, const float* pred, const float* noisy, const float* target,
                                         int64_t n_per_sample, int B, const float* sigmas, float* grad, float* partial,
                                         int n_partial) {
    WIW_REQUIRE(pred && noisy && target && sigmas && grad && partial, "edm_loss_batched: null pointer");
    WIW_REQUIRE(B >= 1 && B <= 64, "edm_loss_batched: 1 <= B <= 64 samples");
    WIW_REQUIRE(n_per_sample > 0, "edm_loss_batched: n_per_sample must be positive");
    WIW_REQUIRE(n_partial >= 1 && n_partial <= 4096, "edm_loss_batched: 1 <= n_partial <= 4096");
    hipLaunchKernelGGL(edm_loss_batched_kernel, dim3((unsigned)n_partial, (unsigned)B), dim3(256), 0, (hipStream_t)stream, pred,
                       noisy, target, n_per_sample, sigmas, 1.0f / (float)B, grad, partial);
    return wiw_check_launch("wiw_edm_loss_grad_batched");
}
