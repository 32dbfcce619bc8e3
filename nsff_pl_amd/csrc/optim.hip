// Row N1: the optimizer step of the reference's training loop -- torch.optim.Adam(lr, eps=1e-8, weight_decay) as
// utils/__init__.py:45-47 (get_optimizer) builds it for train.py:140-146 -- on ONE flat buffer per tensor kind.
// Bound: HBM (28 B per parameter: read p, g, m, v; write p, m, v); 2.3 M parameters -> one launch of a few microseconds
// instead of ~10 multi-tensor launches (eager) or ~200 per-parameter scalar kernels (capturable torch Adam inside a
// hipGraph).  Step count and learning rate are device scalars, so the launch pair is capturable.
// The reference's other optimizers (utils/__init__.py:42-50: --optimizer sgd / radam) follow below on the same buffers.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/nsff_render.h"
#include "nsff_common.h"

namespace {

// state[0] = step count t (as float, exact up to 2^24), state[1] = lr / (1 - beta1^t), state[2] = sqrt(1 - beta2^t)
__global__ void adam_tick_kernel(float* state, const float* lr, double beta1, double beta2) {
    const float t = state[0] + 1.0f;
    state[0] = t;
    // double on purpose: torch evaluates the bias corrections in Python floats
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    state[1] = (float)((double)*lr / bc1);
    state[2] = (float)sqrt(bc2);
}

// index of the parameter tensor that owns flat element e: seg_start[k] <= e < seg_start[k + 1] (seg_start ascending, n_seg + 1 entries)
__device__ __forceinline__ int seg_of(const long long* __restrict__ seg_start, int n_seg, long long e) {
    int lo = 0, hi = n_seg;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seg_start[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}

// used[k] = 1 when any gradient element of parameter tensor k is non-zero this step (torch.optim.Adam skips a parameter whose
// .grad is None -- train.py's unused heads; on the flat buffer such a parameter's gradient slice is exactly zero)
__global__ __launch_bounds__(256) void adam_used_kernel(const float4* __restrict__ g, long long n4, const long long* __restrict__ seg_start,
                                                         int n_seg, int* __restrict__ used) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 gg = g[i];
        const float* G = &gg.x;
        if (gg.x == 0.f && gg.y == 0.f && gg.z == 0.f && gg.w == 0.f) continue;
        const int s0 = seg_of(seg_start, n_seg, 4 * i), s3 = seg_of(seg_start, n_seg, 4 * i + 3);
        if (s0 == s3) { used[s0] = 1; continue; }
#pragma unroll
        for (int c = 0; c < 4; ++c) if (G[c] != 0.f) used[seg_of(seg_start, n_seg, 4 * i + c)] = 1;
    }
}

// seg_start / used (both or neither): elements of a parameter tensor with used[k] == 0 are left untouched (value and moments)
__global__ __launch_bounds__(256) void adam_step_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                                         float4* __restrict__ v, long long n4, const float* __restrict__ state,
                                                         float w1, float beta2, float w2, float eps, float wd,
                                                         const long long* __restrict__ seg_start, int n_seg, const int* __restrict__ used) {
    const float step_size = state[1], sqrt_bc2 = state[2];             // w1 = 1 - beta1, w2 = 1 - beta2 (rounded from double)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        unsigned live = 0xFu;                                          // bit c: element c of this float4 is updated
        if (used != nullptr) {
            const int s0 = seg_of(seg_start, n_seg, 4 * i), s3 = seg_of(seg_start, n_seg, 4 * i + 3);
            if (s0 == s3) live = used[s0] ? 0xFu : 0u;
            else {
                live = 0u;
#pragma unroll
                for (int c = 0; c < 4; ++c) if (used[seg_of(seg_start, n_seg, 4 * i + c)]) live |= 1u << c;
            }
            if (live == 0u) continue;
        }
        float4 pp = p[i], mm = m[i], vv = v[i];
        const float4 gg = g[i];
        float* P = &pp.x; float* M = &mm.x; float* V = &vv.x; const float* G = &gg.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((live >> c) & 1u)) continue;
            // The moments take the roundings of torch.optim.Adam's default device path (its _foreach_ kernels, which the compiler
            // contracts): one fma where torch has one, and (1 - beta2) (g g), not ((1 - beta2) g) g.  Measured on the MI355X against
            // torch 2.10 on 2.1 M elements: both moments bit for bit after one step and after two (EXPERIMENTS.md R18); written
            // separately, exp_avg differed from torch's in 30 % of the elements and, where its two terms cancel, by more than
            // 2e-6 of its value.  (This file is built with -ffp-contract=off: nothing else fuses.)
            const float gr = fmaf(wd, P[c], G[c]);                     // _foreach_add(grads, params, alpha=weight_decay)
            M[c] = fmaf(w1, gr - M[c], M[c]);                          // _foreach_lerp_(exp_avgs, grads, 1 - beta1)
            V[c] = fmaf(w2, gr * gr, V[c] * beta2);                    // _foreach_mul_(exp_avg_sqs, beta2); _foreach_addcmul_(.., grads, grads, 1 - beta2)
            const float denom = sqrtf(V[c]) / sqrt_bc2 + eps;
            P[c] = P[c] - step_size * (M[c] / denom);
        }
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

// bit c set: element c of float4 i belongs to a parameter tensor that received a gradient this step (used == nullptr: all four)
__device__ __forceinline__ unsigned live_mask(const long long* __restrict__ seg_start, int n_seg, const int* __restrict__ used, long long i) {
    if (used == nullptr) return 0xFu;
    const int s0 = seg_of(seg_start, n_seg, 4 * i), s3 = seg_of(seg_start, n_seg, 4 * i + 3);
    if (s0 == s3) return used[s0] ? 0xFu : 0u;
    unsigned live = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) if (used[seg_of(seg_start, n_seg, 4 * i + c)]) live |= 1u << c;
    return live;
}

// torch.optim.SGD(lr, momentum, weight_decay), dampening 0, no Nesterov:  g' = g + wd p;  buf = momentum buf + g';  p -= lr buf.
// buf starts at zero, which gives torch's first-step buf = g' exactly.  HAS_BUF = false (momentum == 0): p -= lr g', b is never read.
// Bound: HBM, 20 B per parameter (read p, g, buf; write p, buf), 12 B without momentum.  state[0] = steps taken (SGD's arithmetic
// does not use it; one thread counts so that the flat optimizers share one notion of "step").
template <bool HAS_BUF>
__global__ __launch_bounds__(256) void sgd_step_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ b,
                                                        long long n4, float* __restrict__ state, const float* __restrict__ lr_p,
                                                        float momentum, float wd, const long long* __restrict__ seg_start, int n_seg,
                                                        const int* __restrict__ used) {
    const float lr = *lr_p;
    if (blockIdx.x == 0 && threadIdx.x == 0) state[0] += 1.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const unsigned live = live_mask(seg_start, n_seg, used, i);
        if (live == 0u) continue;
        float4 pp = p[i], bb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (HAS_BUF) bb = b[i];
        const float4 gg = g[i];
        float* P = &pp.x; float* B = &bb.x; const float* G = &gg.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((live >> c) & 1u)) continue;
            float gr = G[c];
            if (wd != 0.f) gr = gr + wd * P[c];                        // grad.add(param, alpha=weight_decay)
            if (HAS_BUF) { B[c] = B[c] * momentum + gr; gr = B[c]; }   // buf.mul_(momentum).add_(grad)
            P[c] = P[c] - lr * gr;                                     // param.add_(buf, alpha=-lr)
        }
        p[i] = pp;
        if (HAS_BUF) b[i] = bb;
    }
}

// RAdam (Liu et al. 2020) as torch.optim.RAdam(betas, eps, weight_decay, decoupled_weight_decay=True) evaluates it.
// state[0] = step count t, [1] = lr / (1 - beta1^t) (x the rectification term when rho_t > 5), [2] = sqrt(1 - beta2^t),
// [3] = 1 - lr * weight_decay, [4] = 1 when rho_t > 5 (the adaptive branch), else 0
__global__ void radam_tick_kernel(float* state, const float* lr, double beta1, double beta2, double wd) {
    const float t = state[0] + 1.0f;
    state[0] = t;
    // double on purpose: torch evaluates these in Python floats
    const double b2t = pow(beta2, (double)t);
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - b2t;
    const double rho_inf = 2.0 / (1.0 - beta2) - 1.0;
    const double rho_t = rho_inf - 2.0 * (double)t * b2t / bc2;
    double step = (double)*lr / bc1;
    const bool adaptive = rho_t > 5.0;
    if (adaptive) step *= sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t));
    state[1] = (float)step;
    state[2] = (float)sqrt(bc2);
    state[3] = (float)(1.0 - (double)*lr * wd);
    state[4] = adaptive ? 1.0f : 0.0f;
}

// Bound: HBM, 28 B per parameter (read p, g, m, v; write p, m, v), as Adam.
__global__ __launch_bounds__(256) void radam_step_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                                          float4* __restrict__ v, long long n4, const float* __restrict__ state,
                                                          float w1, float beta2, float w2, float eps, bool decay,
                                                          const long long* __restrict__ seg_start, int n_seg, const int* __restrict__ used) {
    const float step_size = state[1], sqrt_bc2 = state[2], keep = state[3];
    const bool adaptive = state[4] != 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const unsigned live = live_mask(seg_start, n_seg, used, i);
        if (live == 0u) continue;
        float4 pp = p[i], mm = m[i], vv = v[i];
        const float4 gg = g[i];
        float* P = &pp.x; float* M = &mm.x; float* V = &vv.x; const float* G = &gg.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((live >> c) & 1u)) continue;
            const float gr = G[c];
            if (decay) P[c] = P[c] * keep;                             // decoupled: param.mul_(1 - lr * weight_decay)
            M[c] = M[c] + w1 * (gr - M[c]);                           // exp_avg.lerp_(grad, 1 - beta1)
            V[c] = V[c] * beta2 + w2 * gr * gr;                       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
            const float upd = adaptive ? M[c] * (sqrt_bc2 / (sqrtf(V[c]) + eps)) : M[c];
            P[c] = P[c] - step_size * upd;
        }
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

}  // namespace

extern "C" int nsff_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                              const float* lr, double beta1, double beta2, double eps, double weight_decay, void* stream) {
    return nsff_adam_step_segments(param, grad, exp_avg, exp_avg_sq, n, state, lr, beta1, beta2, eps, weight_decay, nullptr, 0,
                                   nullptr, stream);
}

extern "C" int nsff_adam_step_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                                       const float* lr, double beta1, double beta2, double eps, double weight_decay,
                                       const int64_t* seg_start, int n_seg, int32_t* seg_used, void* stream) {
    if (!state || !lr || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq))) return NSFF_ERR_NULL;
    if (n < 0 || (n & 3)) return NSFF_ERR_INVALID;
    if ((seg_start == nullptr) != (seg_used == nullptr) || (seg_start && n_seg <= 0)) return NSFF_ERR_INVALID;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return NSFF_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, st, state, lr, beta1, beta2);
    if (n > 0) {
        const long long n4 = n / 4;
        const long long blocks = std::min<long long>((n4 + 255) / 256, 2048);
        if (seg_start) {
            hipError_t e = hipMemsetAsync(seg_used, 0, sizeof(int32_t) * (size_t)n_seg, st);
            if (e != hipSuccess) return nsff_hip_fail(e);
            hipLaunchKernelGGL(adam_used_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(grad), n4,
                               reinterpret_cast<const long long*>(seg_start), n_seg, seg_used);
        }
        hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<float4*>(param),
                           reinterpret_cast<const float4*>(grad), reinterpret_cast<float4*>(exp_avg),
                           reinterpret_cast<float4*>(exp_avg_sq), n4, state, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                           (float)eps, (float)weight_decay, reinterpret_cast<const long long*>(seg_start), n_seg, seg_used);
    }
    return nsff_launch_status();
}

// the per-tensor "received a gradient" flags of the segment form, in front of the element kernel (shared by every flat optimizer)
static int flag_used_segments(const float* grad, long long n4, unsigned blocks, const int64_t* seg_start, int n_seg, int32_t* seg_used,
                              hipStream_t st) {
    hipError_t e = hipMemsetAsync(seg_used, 0, sizeof(int32_t) * (size_t)n_seg, st);
    if (e != hipSuccess) return nsff_hip_fail(e);
    hipLaunchKernelGGL(adam_used_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(grad), n4,
                       reinterpret_cast<const long long*>(seg_start), n_seg, seg_used);
    return NSFF_OK;
}

extern "C" int nsff_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float* state, const float* lr,
                             double momentum, double weight_decay, const int64_t* seg_start, int n_seg, int32_t* seg_used,
                             void* stream) {
    const bool has_buf = momentum != 0.0;
    if (!state || !lr || (n > 0 && (!param || !grad || (has_buf && !momentum_buf)))) return NSFF_ERR_NULL;
    if (n < 0 || (n & 3)) return NSFF_ERR_INVALID;
    if ((seg_start == nullptr) != (seg_used == nullptr) || (seg_start && n_seg <= 0)) return NSFF_ERR_INVALID;
    if (((uintptr_t)param | (uintptr_t)grad | (has_buf ? (uintptr_t)momentum_buf : 0)) & 15) return NSFF_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const long long n4 = n / 4;
    const unsigned blocks = (unsigned)std::max<long long>(std::min<long long>((n4 + 255) / 256, 2048), 1);   // (n == 0: the count only)
    if (seg_start && n > 0) {
        const int rc = flag_used_segments(grad, n4, blocks, seg_start, n_seg, seg_used, st);
        if (rc != NSFF_OK) return rc;
    }
    auto kernel = has_buf ? sgd_step_kernel<true> : sgd_step_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<float4*>(param), reinterpret_cast<const float4*>(grad),
                       reinterpret_cast<float4*>(has_buf ? momentum_buf : nullptr), n4, state, lr, (float)momentum, (float)weight_decay,
                       reinterpret_cast<const long long*>(seg_start), n_seg, seg_used);
    return nsff_launch_status();
}

extern "C" int nsff_radam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                               const float* lr, double beta1, double beta2, double eps, double weight_decay,
                               const int64_t* seg_start, int n_seg, int32_t* seg_used, void* stream) {
    if (!state || !lr || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq))) return NSFF_ERR_NULL;
    if (n < 0 || (n & 3)) return NSFF_ERR_INVALID;
    if ((seg_start == nullptr) != (seg_used == nullptr) || (seg_start && n_seg <= 0)) return NSFF_ERR_INVALID;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return NSFF_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(radam_tick_kernel, dim3(1), dim3(1), 0, st, state, lr, beta1, beta2, weight_decay);
    if (n > 0) {
        const long long n4 = n / 4;
        const unsigned blocks = (unsigned)std::min<long long>((n4 + 255) / 256, 2048);
        if (seg_start) {
            const int rc = flag_used_segments(grad, n4, blocks, seg_start, n_seg, seg_used, st);
            if (rc != NSFF_OK) return rc;
        }
        hipLaunchKernelGGL(radam_step_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<float4*>(param),
                           reinterpret_cast<const float4*>(grad), reinterpret_cast<float4*>(exp_avg),
                           reinterpret_cast<float4*>(exp_avg_sq), n4, state, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                           (float)eps, weight_decay != 0.0, reinterpret_cast<const long long*>(seg_start), n_seg, seg_used);
    }
    return nsff_launch_status();
}
