// K11  per-pixel regression loss of 2-D image regression (train_image_regression.py:183-185 and
// its validation path :141-142), and its linear-output variant for 1-D signal regression
// (train_signal_regression.py:81-95: the same grid, block sum and partials, no sigmoid, no 0.5).  The logits of the fused MLP go through a sigmoid and a
// 0.5 * mean-squared error against the target colours; the training kernel writes d(loss)/d(logits)
// in the order ATen's autograd evaluates it, the evaluation kernel the squared-error sums for the
// PSNR and, optionally, the (sigmoid * 255) u8 image in the same pass.
//
// Memory-bound and small (~44 B per pixel): one thread per pixel, grid-stride over a grid whose
// size depends on n only.  Each workgroup leaves ONE sum of squares in `partials`; the fixed-order
// final sum (regression_loss_kernel) makes the scalar.  No float atomics: the same inputs give the
// same bits.
#include "common.h"

namespace ffn {

constexpr int kRegThreads = 256;
constexpr int kRegMaxBlocks = 1024;

__host__ __device__ inline int regression_blocks(int64_t n) {
    const int64_t b = (n + kRegThreads - 1) / kRegThreads;
    return (int)(b < kRegMaxBlocks ? (b < 1 ? 1 : b) : kRegMaxBlocks);
}

// Sum over the 256 threads of a workgroup: butterfly over the 64 lanes of each wave, then the four
// wave sums in a fixed order.
__device__ __forceinline__ float reg_block_sum(float v, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float total = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return total;
}

// torch.sigmoid's f32 expression
__device__ __forceinline__ float reg_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// sigma = sigmoid(logits[:, :C]);  loss = 0.5 * mean((sigma - y)^2)  ->
//   d_logits[:, j] = ((sigma - y) * inv_count) * (1 - sigma) * sigma   for j < C,  0 for j >= C:
// mean backward gives 0.5 / count, pow backward 2 (sigma - y); their product is exactly
// (sigma - y) * inv_count in f32, and sigmoid_backward multiplies by (1 - sigma), then sigma.
template <int C>
__global__ void __launch_bounds__(kRegThreads)
regression_train_kernel(const float4* __restrict__ logits, const float* __restrict__ target,
                        int64_t n, float inv_count, float4* __restrict__ d_logits,
                        float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    float acc = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * kRegThreads;
    for (int64_t i = (int64_t)blockIdx.x * kRegThreads + threadIdx.x; i < n; i += stride) {
        const float4 z = logits[i];
        const float zz[4] = {z.x, z.y, z.z, z.w};
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float s = reg_sigmoid(zz[j]);
            const float r = s - target[i * C + j];
            sq += r * r;
            d[j] = ((r * inv_count) * (1.0f - s)) * s;
        }
        acc += sq;
        d_logits[i] = make_float4(d[0], d[1], d[2], d[3]);
    }
    const float total = reg_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Validation: sum((sigmoid - y)^2) per workgroup (target != NULL, PixelDataset.psnr) and / or the
// (sigmoid * 255) u8 pixels, truncated like numpy's astype(np.uint8) (image != NULL, to_image).
template <int C>
__global__ void __launch_bounds__(kRegThreads)
regression_eval_kernel(const float4* __restrict__ logits, const float* __restrict__ target,
                       int64_t n, float* __restrict__ partials, uint8_t* __restrict__ image) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    float acc = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * kRegThreads;
    for (int64_t i = (int64_t)blockIdx.x * kRegThreads + threadIdx.x; i < n; i += stride) {
        const float4 z = logits[i];
        const float zz[4] = {z.x, z.y, z.z, z.w};
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float s = reg_sigmoid(zz[j]);
            if (target != nullptr) {
                const float r = s - target[i * C + j];
                sq += r * r;
            }
            if (image != nullptr) {
                float v = s * 255.0f;
                v = v > 0.0f ? (v < 255.0f ? v : 255.0f) : 0.0f;     // (NaN -> 0)
                image[i * C + j] = (uint8_t)(int)v;
            }
        }
        acc += sq;
    }
    if (partials == nullptr) return;             // (uniform over the grid)
    const float total = reg_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Fixed-order sum of the per-workgroup partials: sse, and loss = 0.5 * (sse / count) (K11,
// kHalf) or sse / count (the linear MSE of signal regression).
template <bool kHalf>
__global__ void __launch_bounds__(kRegThreads)
regression_loss_kernel(const float* __restrict__ partials, int blocks, float count,
                       float* __restrict__ sse_out, float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    float acc = 0.0f;
    for (int i = threadIdx.x; i < blocks; i += kRegThreads) acc += partials[i];
    const float sse = reg_block_sum(acc, red);
    if (threadIdx.x == 0) {
        if (sse_out != nullptr) sse_out[0] = sse;
        if (loss_out != nullptr) loss_out[0] = kHalf ? 0.5f * (sse / count) : sse / count;
    }
}

// Linear MSE of 1-D signal regression (train_signal_regression.py:81-85): no sigmoid, no 0.5.
// loss = mean((logits[:, :C] - y)^2)  ->  autograd runs MeanBackward (the expanded 1 / count),
// PowBackward (exponent 2: grad * (2 * r)) and SubBackward, so in f32
//   d_logits[:, j] = inv_count * (2 * r),  r = z - y,  for j < C;  0 for j >= C
// with inv_count = fl(1 / count) (tests/test_signal_regression_gpu.py pins the order bit for bit
// against torch.autograd at counts that are not powers of two).
template <int C>
__global__ void __launch_bounds__(kRegThreads)
mse_train_kernel(const float4* __restrict__ logits, const float* __restrict__ target, int64_t n,
                 float inv_count, float4* __restrict__ d_logits, float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    float acc = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * kRegThreads;
    for (int64_t i = (int64_t)blockIdx.x * kRegThreads + threadIdx.x; i < n; i += stride) {
        const float4 z = logits[i];
        const float zz[4] = {z.x, z.y, z.z, z.w};
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float r = zz[j] - target[i * C + j];
            sq += r * r;
            d[j] = inv_count * (2.0f * r);
        }
        acc += sq;
        d_logits[i] = make_float4(d[0], d[1], d[2], d[3]);
    }
    const float total = reg_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Validation (train_signal_regression.py:88-95): sum((logits - y)^2) per workgroup only.
template <int C>
__global__ void __launch_bounds__(kRegThreads)
mse_eval_kernel(const float4* __restrict__ logits, const float* __restrict__ target, int64_t n,
                float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    float acc = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * kRegThreads;
    for (int64_t i = (int64_t)blockIdx.x * kRegThreads + threadIdx.x; i < n; i += stride) {
        const float4 z = logits[i];
        const float zz[4] = {z.x, z.y, z.z, z.w};
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float r = zz[j] - target[i * C + j];
            sq += r * r;
        }
        acc += sq;
    }
    const float total = reg_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

}  // namespace ffn

using namespace ffn;

extern "C" int ffn_regression_blocks(int64_t n) { return regression_blocks(n); }

extern "C" int ffn_regression_train(const float* logits, const float* target, int64_t n, int c,
                                    float inv_count, float* d_logits, float* partials,
                                    void* stream) {
    if (n < 1 || c < 1 || c > 4) return fail_arg("ffn_regression_train: shape (n >= 1, 1 <= c <= 4)");
    if (logits == nullptr || target == nullptr || d_logits == nullptr || partials == nullptr)
        return fail_arg("ffn_regression_train: null argument");
    const dim3 grid(regression_blocks(n)), block(kRegThreads);
    const hipStream_t s = (hipStream_t)stream;
    const float4* lg = reinterpret_cast<const float4*>(logits);
    float4* dl = reinterpret_cast<float4*>(d_logits);
    switch (c) {
        case 1: hipLaunchKernelGGL(regression_train_kernel<1>, grid, block, 0, s, lg, target, n, inv_count, dl, partials); break;
        case 2: hipLaunchKernelGGL(regression_train_kernel<2>, grid, block, 0, s, lg, target, n, inv_count, dl, partials); break;
        case 3: hipLaunchKernelGGL(regression_train_kernel<3>, grid, block, 0, s, lg, target, n, inv_count, dl, partials); break;
        default: hipLaunchKernelGGL(regression_train_kernel<4>, grid, block, 0, s, lg, target, n, inv_count, dl, partials); break;
    }
    return check_launch("ffn_regression_train");
}

extern "C" int ffn_regression_eval(const float* logits, const float* target, int64_t n, int c,
                                   float* partials, uint8_t* image, void* stream) {
    if (n < 1 || c < 1 || c > 4) return fail_arg("ffn_regression_eval: shape (n >= 1, 1 <= c <= 4)");
    if (logits == nullptr || (partials == nullptr && image == nullptr))
        return fail_arg("ffn_regression_eval: null argument");
    if (partials != nullptr && target == nullptr)
        return fail_arg("ffn_regression_eval: partials need a target");
    const dim3 grid(regression_blocks(n)), block(kRegThreads);
    const hipStream_t s = (hipStream_t)stream;
    const float4* lg = reinterpret_cast<const float4*>(logits);
    switch (c) {
        case 1: hipLaunchKernelGGL(regression_eval_kernel<1>, grid, block, 0, s, lg, target, n, partials, image); break;
        case 2: hipLaunchKernelGGL(regression_eval_kernel<2>, grid, block, 0, s, lg, target, n, partials, image); break;
        case 3: hipLaunchKernelGGL(regression_eval_kernel<3>, grid, block, 0, s, lg, target, n, partials, image); break;
        default: hipLaunchKernelGGL(regression_eval_kernel<4>, grid, block, 0, s, lg, target, n, partials, image); break;
    }
    return check_launch("ffn_regression_eval");
}

extern "C" int ffn_regression_loss(const float* partials, int num_blocks, float count,
                                   float* sse_out, float* loss_out, void* stream) {
    if (partials == nullptr || num_blocks < 1 || (sse_out == nullptr && loss_out == nullptr))
        return fail_arg("ffn_regression_loss: arguments");
    hipLaunchKernelGGL(regression_loss_kernel<true>, dim3(1), dim3(kRegThreads), 0,
                       (hipStream_t)stream, partials, num_blocks, count, sse_out, loss_out);
    return check_launch("ffn_regression_loss");
}

extern "C" int ffn_regression_mse_train(const float* logits, const float* target, int64_t n, int c,
                                        float inv_count, float* d_logits, float* partials,
                                        void* stream) {
    if (n < 1 || c < 1 || c > 4)
        return fail_arg("ffn_regression_mse_train: shape (n >= 1, 1 <= c <= 4)");
    if (logits == nullptr || target == nullptr || d_logits == nullptr || partials == nullptr)
        return fail_arg("ffn_regression_mse_train: null argument");
    const dim3 grid(regression_blocks(n)), block(kRegThreads);
    const hipStream_t s = (hipStream_t)stream;
    const float4* lg = reinterpret_cast<const float4*>(logits);
    float4* dl = reinterpret_cast<float4*>(d_logits);
    switch (c) {
        case 1: hipLaunchKernelGGL(mse_train_kernel<1>, grid, block, 0, s, lg, target, n, inv_count, dl, partials); break;
        case 2: hipLaunchKernelGGL(mse_train_kernel<2>, grid, block, 0, s, lg, target, n, inv_count, dl, partials); break;
        case 3: hipLaunchKernelGGL(mse_train_kernel<3>, grid, block, 0, s, lg, target, n, inv_count, dl, partials); break;
        default: hipLaunchKernelGGL(mse_train_kernel<4>, grid, block, 0, s, lg, target, n, inv_count, dl, partials); break;
    }
    return check_launch("ffn_regression_mse_train");
}

extern "C" int ffn_regression_mse_eval(const float* logits, const float* target, int64_t n, int c,
                                       float* partials, void* stream) {
    if (n < 1 || c < 1 || c > 4)
        return fail_arg("ffn_regression_mse_eval: shape (n >= 1, 1 <= c <= 4)");
    if (logits == nullptr || target == nullptr || partials == nullptr)
        return fail_arg("ffn_regression_mse_eval: null argument");
    const dim3 grid(regression_blocks(n)), block(kRegThreads);
    const hipStream_t s = (hipStream_t)stream;
    const float4* lg = reinterpret_cast<const float4*>(logits);
    switch (c) {
        case 1: hipLaunchKernelGGL(mse_eval_kernel<1>, grid, block, 0, s, lg, target, n, partials); break;
        case 2: hipLaunchKernelGGL(mse_eval_kernel<2>, grid, block, 0, s, lg, target, n, partials); break;
        case 3: hipLaunchKernelGGL(mse_eval_kernel<3>, grid, block, 0, s, lg, target, n, partials); break;
        default: hipLaunchKernelGGL(mse_eval_kernel<4>, grid, block, 0, s, lg, target, n, partials); break;
    }
    return check_launch("ffn_regression_mse_eval");
}

extern "C" int ffn_regression_mse_loss(const float* partials, int num_blocks, float count,
                                       float* sse_out, float* loss_out, void* stream) {
    if (partials == nullptr || num_blocks < 1 || (sse_out == nullptr && loss_out == nullptr))
        return fail_arg("ffn_regression_mse_loss: arguments");
    hipLaunchKernelGGL(regression_loss_kernel<false>, dim3(1), dim3(kRegThreads), 0,
                       (hipStream_t)stream, partials, num_blocks, count, sse_out, loss_out);
    return check_launch("ffn_regression_mse_loss");
}
