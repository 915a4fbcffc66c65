// K10 + K11: parameter-arena kernels.  The student (and teacher) parameters live in ONE flat fp32 buffer
// (desed_task_amd/arena.py), so the EMA teacher update (sed_trainer.py:187-199) and Adam
// (torch.optim.Adam defaults, train_sed.py:199-201) are single streaming launches over 1,112,420 floats
// (float4 per lane) instead of 62 / 124 tiny per-tensor ops.  HBM-bound: 12 B/param (EMA), 28 B/param (Adam).
#include "sed_common.h"
#include "../../include/sed_hip.h"   // SED_SQNORM_*: the constants the consumers of the partials (and the tests) share

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ teacher, const float* __restrict__ student, size_t n4,
                                                  size_t n, float alpha, float one_minus_alpha,
                                                  const float* __restrict__ alpha_dev) {
    if (alpha_dev) { alpha = alpha_dev[0]; one_minus_alpha = alpha_dev[1]; }   // device-resident (hipGraph replays)
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) {
        float4 t = ((float4*)teacher)[i];
        const float4 s = ((const float4*)student)[i];
        t.x = t.x * alpha + one_minus_alpha * s.x; t.y = t.y * alpha + one_minus_alpha * s.y;
        t.z = t.z * alpha + one_minus_alpha * s.z; t.w = t.w * alpha + one_minus_alpha * s.w;
        ((float4*)teacher)[i] = t;
    }
    if (i == 0) for (size_t j = n4 * 4; j < n; ++j) teacher[j] = teacher[j] * alpha + one_minus_alpha * student[j];
}
// teacher <- alpha * teacher + (1 - alpha) * student over n floats.  n >= 4 takes float4 accesses: both buffers 16-byte aligned, else
// SED_ERR_ARG; n < 4 runs the scalar tail alone and is legal at any alignment (arena.ema_update_'s unaligned 1-3-element tensors).
SED_API int sed_ema_update(float* teacher, const float* student, long long n, float alpha, float one_minus_alpha,
                              const float* alpha_dev, void* stream) {
    if (n <= 0) return SED_OK;
    const size_t n4 = (size_t)n / 4;
    if (n4 > 0 && (((uintptr_t)teacher | (uintptr_t)student) & 15) != 0) return SED_ERR_ARG;
    const int grid = (int)((n4 + 255) / 256) + (n4 == 0 ? 1 : 0);
    SED_LAUNCH(ema_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, teacher, student, n4, (size_t)n, alpha, one_minus_alpha,
               alpha_dev);
    return sed_check_launch();
}

// One element of torch.optim.Adam: shared by adam_kernel and adam_clipped_kernel, so that both compile to the same arithmetic
// (FMA contraction included) and a clipped step whose coefficient is exactly 1 equals the plain step bit for bit.
__device__ __forceinline__ void adam_element(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, size_t i, float b1, float b2, float eps, float step_size,
                                             float inv_bc2_sqrt, float grad_scale) {
    const float gi = g[i] * grad_scale;
    const float mi = m[i] * b1 + (1.0f - b1) * gi;
    const float vi = v[i] * b2 + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
    p[i] = p[i] - step_size * (mi / denom);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, size_t n, float b1, float b2, float eps,
                                                   float step_size, float inv_bc2_sqrt, float grad_scale,
                                                   const float* __restrict__ hyper_dev) {
    if (hyper_dev) { step_size = hyper_dev[0]; inv_bc2_sqrt = hyper_dev[1]; }   // device-resident (hipGraph replays)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        adam_element(p, g, m, v, i, b1, b2, eps, step_size, inv_bc2_sqrt, grad_scale);
}
// torch.optim.Adam (no weight decay, no amsgrad): step_size = lr / (1 - b1^t), inv_bc2_sqrt = 1 / sqrt(1 - b2^t).
// grad_scale folds the data-parallel 1/world_size averaging into the update.
SED_API int sed_adam_step(float* p, const float* g, float* m, float* v, long long n, float b1, float b2, float eps,
                             float step_size, float inv_bc2_sqrt, float grad_scale, const float* hyper_dev, void* stream) {
    if (n <= 0) return SED_OK;
    int grid = (int)(((size_t)n + 255) / 256);
    if (grid > 2048) grid = 2048;
    SED_LAUNCH(adam_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (size_t)n, b1, b2, eps, step_size,
               inv_bc2_sqrt, grad_scale, hyper_dev);
    return sed_check_launch();
}

// ---- gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) ----------------------------------------------------
// Two launches on one stream: grad_sqnorm_kernel leaves one partial sum of squares per workgroup, adam_clipped_kernel adds them and
// clips.  The kernel boundary is the hand-over (no fence, no ticket, no float atomics, no zero-fill launch); every addition order is
// fixed, so the same gradient gives the same bits on every run, for every workgroup, whatever the device.
#define SQN_THREADS SED_SQNORM_THREADS
#define SQN_MAX SED_SQNORM_MAX_PARTIALS
static_assert(SQN_THREADS == 256 && SQN_MAX == SQN_THREADS, "one partial per lane of the consumer's 256-thread workgroup");

// Sum over the 256 lanes of a workgroup in a fixed order: 6 butterfly levels inside each wave (both partners of an exchange add the
// same two numbers: all lanes of a wave end with equal bits), then ((w0 + w1) + w2) + w3 through LDS.  Every thread gets the sum.
__device__ __forceinline__ float sqn_block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}

// Workgroups the norm runs on: a function of n alone (sed_hip.h: SED_SQNORM_*).
static inline int sqn_grid(size_t n4) {
    size_t g = (n4 + SQN_THREADS - 1) / SQN_THREADS;
    return g < 1 ? 1 : (g > SQN_MAX ? SQN_MAX : (int)g);
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, size_t n4, size_t n,
                                                          float* __restrict__ partials) {
    __shared__ float red[4];
    float acc = 0.0f;
    // lane order: float4 k of this lane is element (k gridDim.x + blockIdx.x) 256 + threadIdx.x; x, y, z, w in turn, one FMA each
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 x = ((const float4*)g)[i];
        acc = sed_sfma(x.x, x.x, acc);
        acc = sed_sfma(x.y, x.y, acc);
        acc = sed_sfma(x.z, x.z, acc);
        acc = sed_sfma(x.w, x.w, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (size_t j = n4 * 4; j < n; ++j) acc = sed_sfma(g[j], g[j], acc);        // scalar tail (n % 4 elements)
    const float s = sqn_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
    // the consumer always adds SED_SQNORM_MAX_PARTIALS slots: the ones no workgroup owns are written as 0 here
    if (blockIdx.x == 0 && threadIdx.x >= gridDim.x) partials[threadIdx.x] = 0.0f;
}
// partials[0 .. SED_SQNORM_MAX_PARTIALS) <- per-workgroup sums of g[i]^2 over n floats (slots beyond the grid: 0).  g is only read.
// Alignment contract of sed_ema_update: n >= 4 needs a 16-byte aligned g (float4 loads), else SED_ERR_ARG; n < 4 is legal anywhere.
// n <= 0 still writes the (all-zero) partials: the consumer reads them whatever n is.
SED_API int sed_grad_sqnorm(const float* g, long long n, float* partials, void* stream) {
    if (!partials) return SED_ERR_ARG;
    if (n < 0) n = 0;
    const size_t n4 = (size_t)n / 4;
    if (n4 > 0 && ((uintptr_t)g & 15) != 0) return SED_ERR_ARG;
    SED_LAUNCH(grad_sqnorm_kernel, dim3(sqn_grid(n4)), dim3(256), 0, (hipStream_t)stream, g, n4, (size_t)n, partials);
    return sed_check_launch();
}

__global__ __launch_bounds__(256) void adam_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, size_t n, float b1, float b2, float eps,
                                                           float step_size, float inv_bc2_sqrt, float grad_scale,
                                                           const float* __restrict__ hyper_dev, const float* __restrict__ partials,
                                                           float max_norm, float* __restrict__ clip_out) {
    __shared__ float red[4];
    if (hyper_dev) { step_size = hyper_dev[0]; inv_bc2_sqrt = hyper_dev[1]; }   // device-resident (hipGraph replays)
    // every workgroup adds the same 256 partials in the same order: identical bits everywhere
    const float sq = sqn_block_sum(partials[threadIdx.x], red);
    const float total = sqrtf(sq) * fabsf(grad_scale);          // || grad_scale g ||_2
    float coef = max_norm / (total + 1e-6f);
    coef = coef > 1.0f ? 1.0f : coef;                           // torch.clamp(max=1): a NaN stays a NaN
    if (blockIdx.x == 0 && threadIdx.x == 0) { clip_out[0] = total; clip_out[1] = coef; }
    const float gs = grad_scale * coef;                         // coef == 1: grad_scale itself -> adam_kernel's bits
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        adam_element(p, g, m, v, i, b1, b2, eps, step_size, inv_bc2_sqrt, gs);
}
// sed_adam_step on g * grad_scale * coef, coef = min(1, max_norm / (|| grad_scale g ||_2 + 1e-6)) from the partials sed_grad_sqnorm
// left for the SAME g (the previous launch on this stream).  clip_out[0 .. 2) = {norm, coef}.  n <= 0: nothing is launched.
SED_API int sed_adam_step_clipped(float* p, const float* g, float* m, float* v, long long n, float b1, float b2, float eps,
                                     float step_size, float inv_bc2_sqrt, float grad_scale, const float* hyper_dev,
                                     const float* partials, float max_norm, float* clip_out, void* stream) {
    if (!partials || !clip_out) return SED_ERR_ARG;
    if (n <= 0) return SED_OK;
    int grid = (int)(((size_t)n + 255) / 256);
    if (grid > 2048) grid = 2048;
    SED_LAUNCH(adam_clipped_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (size_t)n, b1, b2, eps, step_size,
               inv_bc2_sqrt, grad_scale, hyper_dev, partials, max_norm, clip_out);
    return sed_check_launch();
}

// Zero up to four (small) accumulator buffers in one launch; null / 0 entries are skipped.  The kernel indexes with int: a count
// that does not fit is SED_ERR_UNSUPPORTED (cast to int it would turn negative and the buffer would silently stay as it was).
SED_API int sed_zero_buffers(float* p0, long long n0, float* p1, long long n1, float* p2, long long n2, float* p3, long long n3,
                                void* stream) {
    const long long nmax = 0x7fffffffLL - 255;          // (n + 255) / 256 in sed_zero4 must not overflow either
    if (n0 > nmax || n1 > nmax || n2 > nmax || n3 > nmax) return SED_ERR_UNSUPPORTED;
    if (!p0) n0 = 0;
    if (!p1) n1 = 0;
    if (!p2) n2 = 0;
    if (!p3) n3 = 0;
    sed_zero4((hipStream_t)stream, p0, (int)n0, p1, (int)n1, p2, (int)n2, p3, (int)n3);
    return sed_check_launch();
}
