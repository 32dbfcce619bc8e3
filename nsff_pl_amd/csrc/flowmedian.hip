// The image-guided weighted median of a flow map (nsff_flow_median): the non-local term of "Classic+NL" (Sun, Roth and Black 2010)
// as one filter pass.  TV-L1's isotropic smoothness and its 3 x 3 median round a flow edge off; here each flow component becomes the
// weighted median of its neighbours in a (2 r + 1)^2 window, a neighbour weighing more when it is close and has the centre's grey
// level and nothing where its own flow failed the forward-backward check, which ties the flow edge to the image edge.
//
// include/nsff_render.h states the operation.  The weights are one fp32 operation per step (this file is built -ffp-contract=off;
// IEEE division), which tests/flowmedian_numpy.py restates in numpy, and then INTEGERS of 16 bits: every sum is exact whatever its
// order, so that any selection algorithm gives the same value, and the tests compare with the twin at every pixel.
//
// The selection, both routes: the order-preserving 32-bit key of a value (sign bit flipped for positives, all bits for negatives;
// -0 counts as +0) is built from its top bit down -- 32 steps, each asking whether the candidates with a key <= the prefix so far,
// followed by ones, weigh half the total.  Fixed trip counts, no atomics, no data-dependent loop; both components go in lockstep.
//
// flow_median_plain -- the definition restated: one thread per pixel reads global memory, and every one of the 33 passes over the
//   window (the total, then 32 steps) forms the weights again.
// flow_median_tiled<R> -- a 32 x 8 tile with its halo of R in LDS as (key u, key v) pairs and grey; a pixel that is no candidate
//   (outside the image, unknown, valid == 0) has grey = +inf there, which the weight's own arithmetic turns into the integer 0:
//   di = inf, 1 / inf = 0.  A pixel's (2 R + 1)^2 integer weights are computed ONCE and kept two to a register (113 registers at
//   R = 7; the window loops are unrolled, so every register index is static); the 32 steps read the key pairs with ds_read_b64 --
//   a half wave reads 32 consecutive pairs, which no pitch can make conflict -- and compare, select and add.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_flow_chain.h"

namespace {

constexpr int MAX_R = NSFF_FLOW_MEDIAN_MAX_RADIUS;
constexpr int MAX_SIDE = 2 * MAX_R + 1;
constexpr int TILE_W = 32, TILE_H = 8, THREADS = TILE_W * TILE_H;
constexpr int PLAIN_W = 64, PLAIN_H = 4;

struct MedianParams {
    int32_t H, W, r, pad_;
    float sigma_i, pad1_;
    const float2* flow;  const float* grey;  const uint8_t* valid;  float2* out;
    float s[MAX_SIDE * MAX_SIDE];                                 // 1 + (dx^2 + dy^2) / sigma_s^2, rows of 2 r + 1
};

__device__ __forceinline__ uint32_t key_of(float v) {
    uint32_t b = __float_as_uint(v);
    b = b == 0x80000000u ? 0u : b;                                // -0 and +0 are one value
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

// the integer weight of a candidate of grey level gq for a centre of grey level gp: four roundings, then the nearest integer
__device__ __forceinline__ uint32_t weight_of(float gq, float gp, float sigma_i, float s) {
    const float di = (gq - gp) / sigma_i;
    const float w = 1.f / ((1.f + di * di) * s);
    return (uint32_t)(int)rintf(w * 65535.f);
}

__global__ __launch_bounds__(PLAIN_W * PLAIN_H) void flow_median_plain(MedianParams a) {
    const int x = blockIdx.x * PLAIN_W + threadIdx.x, y = blockIdx.y * PLAIN_H + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const int64_t plane = (int64_t)blockIdx.z * a.H * a.W;
    const int64_t p = plane + (int64_t)y * a.W + x;
    const float2 own = a.flow[p];
    if (!flow_known(own)) { a.out[p] = own; return; }
    const float gp = a.grey[p];
    const int side = 2 * a.r + 1;

    uint32_t ans_u = 0u, ans_v = 0u, total = 0u;
    for (int step = -1; step < 32; ++step) {                      // step -1: the total (every key <= all ones)
        const uint32_t low = step < 0 ? 0xffffffffu : (0x80000000u >> step) - 1u;
        const uint32_t try_u = ans_u | low, try_v = ans_v | low;
        uint32_t cum_u = 0u, cum_v = 0u;
        for (int dy = -a.r; dy <= a.r; ++dy) {                    // (uniform loops: the table comes through scalar loads)
            for (int dx = -a.r; dx <= a.r; ++dx) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                const int64_t q = plane + (int64_t)qy * a.W + qx;
                const bool centre = dx == 0 && dy == 0;
                const float2 f = a.flow[q];
                if (!centre && (!flow_known(f) || (a.valid && a.valid[q] == 0))) continue;
                const uint32_t w = centre ? 65535u : weight_of(a.grey[q], gp, a.sigma_i, a.s[(dy + a.r) * side + (dx + a.r)]);
                cum_u += key_of(f.x) <= try_u ? w : 0u;
                cum_v += key_of(f.y) <= try_v ? w : 0u;
            }
        }
        if (step < 0) { total = cum_u; continue; }
        const uint32_t bit = 0x80000000u >> step;
        ans_u |= 2u * cum_u >= total ? 0u : bit;
        ans_v |= 2u * cum_v >= total ? 0u : bit;
    }
    a.out[p] = make_float2(value_of(ans_u), value_of(ans_v));
}

template <int R>
__global__ __launch_bounds__(THREADS) void flow_median_tiled(MedianParams a) {
    constexpr int SIDE = 2 * R + 1, N = SIDE * SIDE, LW = TILE_W + 2 * R, LH = TILE_H + 2 * R, CENTRE = R * SIDE + R;
    __shared__ uint2 s_key[LH * LW];
    __shared__ float s_grey[LH * LW];
    const int tid = threadIdx.x, tx = tid % TILE_W, ty = tid / TILE_W;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    const int64_t plane = (int64_t)blockIdx.z * a.H * a.W;

    for (int e = tid; e < LH * LW; e += THREADS) {
        const int ey = e / LW, ex = e - ey * LW;
        const int gx = x0 - R + ex, gy = y0 - R + ey;
        uint2 k = make_uint2(0u, 0u);
        float g = INFINITY;                                       // no candidate: the weight comes out 0
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
            const int64_t q = plane + (int64_t)gy * a.W + gx;
            const float2 f = a.flow[q];
            if (flow_known(f) && (!a.valid || a.valid[q] != 0)) {
                k = make_uint2(key_of(f.x), key_of(f.y));
                g = a.grey[q];
            }
        }
        s_key[e] = k;
        s_grey[e] = g;
    }
    __syncthreads();

    const int x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;
    const int64_t p = plane + (int64_t)y * a.W + x;
    const float2 own = a.flow[p];
    if (!flow_known(own)) { a.out[p] = own; return; }
    const float gp = a.grey[p];                                   // (the centre's LDS entry holds +inf where valid == 0)
    const uint2 own_key = make_uint2(key_of(own.x), key_of(own.y));
    const uint2* keys = s_key + ty * LW + tx;                     // the window's corner
    const float* greys = s_grey + ty * LW + tx;

    uint32_t wp[(N + 1) / 2];                                     // the weights, two to a register
    uint32_t total = 0u;
#pragma unroll
    for (int i = 0; i < (N + 1) / 2; ++i) wp[i] = 0u;
#pragma unroll
    for (int dy = 0; dy < SIDE; ++dy) {
#pragma unroll
        for (int dx = 0; dx < SIDE; ++dx) {
            const int j = dy * SIDE + dx;
            const uint32_t w = j == CENTRE ? 65535u : weight_of(greys[dy * LW + dx], gp, a.sigma_i, a.s[j]);
            total += w;
            wp[j >> 1] |= w << (16 * (j & 1));
        }
        asm volatile("" : "+v"(total));                           // a row at a time: its loads hoisted ahead, or its sum put off, would
        __builtin_amdgcn_sched_barrier(0);                        // need registers for every row at once
    }

    uint32_t ans_u = 0u, ans_v = 0u;
#pragma nounroll
    for (int step = 0; step < 32; ++step) {
        const uint32_t bit = 0x80000000u >> step, low = bit - 1u;
        const uint32_t try_u = ans_u | low, try_v = ans_v | low;
        uint32_t cum_u = 0u, cum_v = 0u;
#pragma unroll
        for (int dy = 0; dy < SIDE; ++dy) {
            // the row's packed words are opaque here: unpacked ahead of their row, or once before the loop, the halves would need two
            // registers a word
#pragma unroll
            for (int i = (dy * SIDE) >> 1; i <= (dy * SIDE + SIDE - 1) >> 1; ++i) asm volatile("" : "+v"(wp[i]));
#pragma unroll
            for (int dx = 0; dx < SIDE; ++dx) {
                const int j = dy * SIDE + dx;
                const uint2 k = j == CENTRE ? own_key : keys[dy * LW + dx];
                const uint32_t w = (j & 1) ? wp[j >> 1] >> 16 : wp[j >> 1] & 0xffffu;
                cum_u += k.x <= try_u ? w : 0u;
                cum_v += k.y <= try_v ? w : 0u;
                if (SIDE > 9 && dx == SIDE / 2) {                 // a long row in two halves: fewer key pairs in flight at once
                    asm volatile("" : "+v"(cum_u), "+v"(cum_v));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // the row's sums are due here: the adds are not to be gathered into one tree behind the last row, all loads ahead of it
            asm volatile("" : "+v"(cum_u), "+v"(cum_v));
            __builtin_amdgcn_sched_barrier(0);
        }
        ans_u |= 2u * cum_u >= total ? 0u : bit;
        ans_v |= 2u * cum_v >= total ? 0u : bit;
    }
    a.out[p] = make_float2(value_of(ans_u), value_of(ans_v));
}

template <int R>
void launch_tiled(const MedianParams& p, int32_t n_pairs, hipStream_t st) {
    const dim3 grid((p.W + TILE_W - 1) / TILE_W, (p.H + TILE_H - 1) / TILE_H, n_pairs);
    hipLaunchKernelGGL(flow_median_tiled<R>, grid, dim3(THREADS), 0, st, p);
}

}  // namespace

extern "C" int nsff_flow_median(const NsffFlowMedianArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (a->n_pairs < 1 || a->n_pairs > 65535 || a->H < 1 || a->W < 1 || a->H > 32768 || a->W > 32768) return NSFF_ERR_INVALID;
    if ((int64_t)a->n_pairs * a->H * a->W >= ((int64_t)1 << 31)) return NSFF_ERR_INVALID;
    if (a->radius < 1 || a->radius > MAX_R || (a->tiled != 0 && a->tiled != 1)) return NSFF_ERR_INVALID;
    if (!bounded_positive(a->sigma_i) || !bounded_positive(a->sigma_s)) return NSFF_ERR_INVALID;
    if (!a->flow || !a->grey || !a->out) return NSFF_ERR_NULL;
    if (((uintptr_t)a->flow | (uintptr_t)a->out) & 7) return NSFF_ERR_ALIGN;
    if ((uintptr_t)a->grey & 3) return NSFF_ERR_ALIGN;
    // out must not overlap flow: a pixel's neighbours are read after it is written
    if (overlap(a->flow, a->out, (int64_t)a->n_pairs * a->H * a->W * 8)) return NSFF_ERR_INVALID;

    MedianParams p = {};
    p.H = a->H; p.W = a->W; p.r = a->radius; p.sigma_i = a->sigma_i;
    p.flow = reinterpret_cast<const float2*>(a->flow); p.grey = a->grey; p.valid = a->valid; p.out = reinterpret_cast<float2*>(a->out);
    const int side = 2 * a->radius + 1;
    const double ss = (double)a->sigma_s * (double)a->sigma_s;
    for (int dy = -a->radius; dy <= a->radius; ++dy)
        for (int dx = -a->radius; dx <= a->radius; ++dx)
            p.s[(dy + a->radius) * side + (dx + a->radius)] = (float)(1.0 + (double)(dx * dx + dy * dy) / ss);

    hipStream_t st = (hipStream_t)stream;
    if (!a->tiled) {
        const dim3 grid((a->W + PLAIN_W - 1) / PLAIN_W, (a->H + PLAIN_H - 1) / PLAIN_H, a->n_pairs);
        hipLaunchKernelGGL(flow_median_plain, grid, dim3(PLAIN_W, PLAIN_H), 0, st, p);
    } else {
        switch (a->radius) {
            case 1: launch_tiled<1>(p, a->n_pairs, st); break;
            case 2: launch_tiled<2>(p, a->n_pairs, st); break;
            case 3: launch_tiled<3>(p, a->n_pairs, st); break;
            case 4: launch_tiled<4>(p, a->n_pairs, st); break;
            case 5: launch_tiled<5>(p, a->n_pairs, st); break;
            case 6: launch_tiled<6>(p, a->n_pairs, st); break;
            default: launch_tiled<7>(p, a->n_pairs, st); break;
        }
    }
    return nsff_launch_status();
}
