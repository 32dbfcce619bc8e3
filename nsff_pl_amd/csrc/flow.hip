// Induced optical flow of rendered frames: the pixel motion of the expected warped points xyz_fw / xyz_bw (rendering.py:280-287),
// its end-point error against the dataset's flow and the Middlebury colour image the reference's test.ipynb shows
// (datasets/flowlib.py: flow_to_image, compute_color, flow_error) -- for F frames and both directions in one call.
//
// nsff_flow_maps, up to two launches:
//
// flow_map_kernel -- per pixel and direction
//   projection   the geometric loss's own chain (losses.py:99-116), one fp32 rounding per operation (built -ffp-contract=off;
//                ndc_to_pixel of nsff_frame_ops.h, which nsff_track_step of tracks.hip calls too):
//                  world  Rz = 2 / ((z - 1) - 1e-6f), Rx = (((-Rz) * x) * cx) / fx, Ry = (((-Rz) * y) * cy) / fy   (ray_utils.py:142-145)
//                  uvd_r  = ((P[r][0] * Rx + P[r][1] * Ry) + P[r][2] * Rz) + P[r][3],  P = Ps[min(t + 1, max_t)] (fw), Ps[max(t - 1, 0)] (bw)
//                  uv     = uvd.xy / (|uvd.z| + 1e-8f),  flow = uv - (px, py)
//                a pixel is valid when uvd.z > 0 and t < max_t (fw) / t > 0 (bw) -- valid_geo_* of losses.py:115-116; a NaN point
//                fails the comparison -- and an invalid pixel gets (1e10, 1e10), "unknown" by the Middlebury convention (> 1e7);
//   EPE          sqrtf(du^2 + dv^2) in fp32 where both flows are known and the ground truth is non-zero (flow_error's smallflow = 0
//                rule), added in fp64 for [all, mask != 0, mask == 0] with int counts;
//   radius       the maximum of sqrtf(u^2 + v^2) over the known pixels of the map and of the ground truth (flow_to_image's maxrad).
// flow_colour_kernel -- compute_color on u / d, v / d with d = float(double(maxrad) + 2^-52), the 55-entry colour wheel held as
//                float(entry / 255) in LDS; unknown (and NaN) pixels are zeroed before the radius and painted black.
//
// A workgroup owns 1024 consecutive pixels OF ONE FRAME (grid.y = frame) and lane l of it the pixels l, l + 256, l + 512, l + 768
// of those, so every global access of a wave is one contiguous run (8 bytes a lane for a flow, 3 for an image) and what a lane, a
// wave and a workgroup add depends on H * W alone: a frame's sums and radii are the same bits at any position of any batch.  The
// 12-byte points would give each lane a 12-byte stride; instead the workgroup's 12 KiB of each direction are copied to LDS as one
// contiguous run (16-byte loads where the run starts 16-byte aligned, dwords otherwise) and read from there at a 3-dword lane
// stride, which is free of bank conflicts (3 is odd).  Per-workgroup partials go to scratch and the frame's last-arriving workgroup
// adds them in block order: the ticketed reduction of nsff_frame_ops.h, which frame_image_kernel (frames.hip) uses too.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_flow_chain.h"

namespace {

constexpr int FLOW_THREADS = 256, FLOW_PX = 4, FLOW_BLOCK_PX = FLOW_THREADS * FLOW_PX;
constexpr int FLOW_WORDS = 11;                                    // one workgroup's share of a frame: 6 fp64 sums, 6 uint32 counts, 4 fp32 radii
constexpr int WHEEL = 55;                                         // RY 15 + YG 6 + GC 4 + CB 11 + BM 13 + MR 6

__global__ __launch_bounds__(FLOW_THREADS) void flow_map_kernel(NsffFlowMapsArgs a, int reduce, unsigned* __restrict__ counters,
                                                                frame_word* __restrict__ partials) {
    __shared__ float s_xyz[2][FLOW_BLOCK_PX * 3];
    __shared__ double s_sum[FLOW_THREADS / 64][6];
    __shared__ uint32_t s_cnt[FLOW_THREADS / 64][6];
    __shared__ float s_rad[FLOW_THREADS / 64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W, b0 = (int64_t)blockIdx.x * FLOW_BLOCK_PX;
    const int npx = (int)min((int64_t)FLOW_BLOCK_PX, HW - b0);    // >= 1: the grid has ceil(HW / 1024) blocks a frame

    // the workgroup's points, one contiguous run per direction
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        if (!a.xyz[d]) continue;
        const float* g = a.xyz[d] + (f * HW + b0) * 3;
        const int cnt = npx * 3;
        int done = 0;
        if (((uintptr_t)g & 15) == 0) {
            const float4* g4 = reinterpret_cast<const float4*>(g);
            float4* s4 = reinterpret_cast<float4*>(s_xyz[d]);
            for (int i = tid; i < cnt / 4; i += FLOW_THREADS) s4[i] = g4[i];
            done = cnt & ~3;
        }
        for (int i = done + tid; i < cnt; i += FLOW_THREADS) s_xyz[d][i] = g[i];
    }
    if (a.xyz[0] || a.xyz[1]) __syncthreads();

    float P[2][12];
    bool t_ok[2] = {false, false};
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int i = 0; i < 12; ++i) P[d][i] = 0.f;
    if (a.xyz[0] || a.xyz[1]) {
        const int t = a.ts[f];
        t_ok[0] = t < a.max_t;
        t_ok[1] = t > 0;
        const int idx[2] = {t < a.max_t ? t + 1 : a.max_t, t > 0 ? t - 1 : 0};    // clamp(t + 1, max = max_t), clamp(t - 1, min = 0)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            if (!a.xyz[d]) continue;
            const float* p = a.Ps + (int64_t)min(max(idx[d], 0), a.n_poses - 1) * 12;   // (a time outside the sequence reads no stray row)
#pragma unroll
            for (int i = 0; i < 12; ++i) P[d][i] = p[i];
        }
    }

    double sum[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    uint32_t cnt[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
    float rad[2][2] = {{0.f, 0.f}, {0.f, 0.f}};                   // [direction][map, ground truth]
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        if (!a.flow[d]) continue;
        float2* F2 = reinterpret_cast<float2*>(a.flow[d]) + f * HW;
        const float2* G2 = a.gt[d] ? reinterpret_cast<const float2*>(a.gt[d]) + f * HW : nullptr;
#pragma unroll
        for (int j = 0; j < FLOW_PX; ++j) {
            const int q = j * FLOW_THREADS + tid;                 // pixel within the workgroup's run
            if (q >= npx) continue;
            const int64_t p = b0 + q;
            float u, v;
            if (a.xyz[d]) {
                const float x = s_xyz[d][3 * q], y = s_xyz[d][3 * q + 1], z = s_xyz[d][3 * q + 2];
                const float wd = ndc_to_pixel(x, y, z, P[d], a.fx, a.fy, a.cx, a.cy, u, v);
                const int py = (int)(p / a.W), px = (int)(p - (int64_t)py * a.W);
                u = u - (float)px;
                v = v - (float)py;
                if (!(wd > 0.f && t_ok[d])) { u = NSFF_FLOW_UNKNOWN; v = NSFF_FLOW_UNKNOWN; }
                F2[p] = make_float2(u, v);
            } else {
                const float2 w = F2[p];
                u = w.x; v = w.y;
            }
            if (!reduce) continue;
            const bool kn = flow_known(u, v);
            if (kn) rad[d][0] = fmaxf(rad[d][0], sqrtf(u * u + v * v));
            if (!G2) continue;
            const float2 g = G2[p];
            const bool gk = flow_known(g.x, g.y);
            if (gk) rad[d][1] = fmaxf(rad[d][1], sqrtf(g.x * g.x + g.y * g.y));
            if (a.epe_sums && kn && gk && (g.x != 0.f || g.y != 0.f)) {
                const float du = g.x - u, dv = g.y - v;
                const double e = (double)sqrtf(du * du + dv * dv);   // the term in fp32, the sum in fp64
                sum[d][0] += e; cnt[d][0] += 1u;
                if (a.mask) {
                    const int k = a.mask[f * HW + p] ? 1 : 2;
                    sum[d][k] += e; cnt[d][k] += 1u;
                }
            }
        }
    }
    if (!reduce) return;

#pragma unroll
    for (int d = 0; d < 2; ++d) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { sum[d][k] = wave_sum(sum[d][k]); cnt[d][k] = wave_sum(cnt[d][k]); }
#pragma unroll
        for (int k = 0; k < 2; ++k) rad[d][k] = wave_max(rad[d][k]);
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { s_sum[wave][3 * d + k] = sum[d][k]; s_cnt[wave][3 * d + k] = cnt[d][k]; }
#pragma unroll
            for (int k = 0; k < 2; ++k) s_rad[wave][2 * d + k] = rad[d][k];
        }
    }
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_blocks = gridDim.x;
    frame_word* fp = partials + f * n_blocks * FLOW_WORDS;
    frame_word mine[FLOW_WORDS];
#pragma unroll
    for (int i = 0; i < 6; ++i) mine[i] = pack_double(sum4(s_sum, i));
#pragma unroll
    for (int i = 0; i < 3; ++i) mine[6 + i] = pack2(sum4(s_cnt, 2 * i), sum4(s_cnt, 2 * i + 1));
#pragma unroll
    for (int i = 0; i < 2; ++i) mine[9 + i] = pack2(max4(s_rad, 2 * i), max4(s_rad, 2 * i + 1));
    if (!frame_publish(fp, counters + f, blockIdx.x, n_blocks, lane, mine)) return;
    double tot[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long n[6] = {0, 0, 0, 0, 0, 0};
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    frame_fold<FLOW_WORDS>(fp, n_blocks, lane, [&](const frame_word (&w)[FLOW_WORDS]) {
#pragma unroll
        for (int i = 0; i < 6; ++i) tot[i] += word_double(w[i]);
#pragma unroll
        for (int i = 0; i < 3; ++i) { n[2 * i] += (long long)word_lo(w[6 + i]); n[2 * i + 1] += (long long)word_hi(w[6 + i]); }
#pragma unroll
        for (int i = 0; i < 2; ++i) { r[2 * i] = fmaxf(r[2 * i], word_lo_f(w[9 + i])); r[2 * i + 1] = fmaxf(r[2 * i + 1], word_hi_f(w[9 + i])); }
    });
#pragma unroll
    for (int i = 0; i < 6; ++i) { tot[i] = wave_sum(tot[i]); n[i] = wave_sum(n[i]); }
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = wave_max(r[i]);
    if (lane == 0) {
        if (a.epe_sums)
            for (int i = 0; i < 6; ++i) { a.epe_sums[f * 6 + i] = tot[i]; a.epe_counts[f * 6 + i] = (int64_t)n[i]; }
        if (a.maxrad)
            for (int i = 0; i < 4; ++i) a.maxrad[f * 4 + i] = r[i];
        frame_counter_reset(counters + f);
    }
}

// entry i of flowlib's make_color_wheel, channel c: floor(255 k / n) along each segment (integer division gives the same floor:
// a quotient that is no integer is at least 1 / 15 away from one)
__device__ __forceinline__ int wheel_entry(int i, int c) {
    int r, g, b;
    if (i < 15)      { r = 255; g = 255 * i / 15; b = 0; }
    else if (i < 21) { r = 255 - 255 * (i - 15) / 6; g = 255; b = 0; }
    else if (i < 25) { r = 0; g = 255; b = 255 * (i - 21) / 4; }
    else if (i < 36) { r = 0; g = 255 - 255 * (i - 25) / 11; b = 255; }
    else if (i < 49) { r = 255 * (i - 36) / 13; g = 0; b = 255; }
    else             { r = 255; g = 0; b = 255 - 255 * (i - 49) / 6; }
    return c == 0 ? r : (c == 1 ? g : b);
}

// flow_to_image / compute_color (flowlib.py:132-239) in fp32, every step one operation; rad_src (F, 2, 2): the radius the divisor
// is formed from, per frame, direction and [map, ground truth]
__global__ __launch_bounds__(FLOW_THREADS) void flow_colour_kernel(NsffFlowMapsArgs a, const float* __restrict__ rad_src) {
    __shared__ float s_wheel[WHEEL * 3];
    const int tid = threadIdx.x;
    if (tid < WHEEL * 3) s_wheel[tid] = (float)((double)wheel_entry(tid / 3, tid % 3) / 255.0);
    __syncthreads();
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W, b0 = (int64_t)blockIdx.x * FLOW_BLOCK_PX;
    const float pi = 3.14159265358979323846f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {                                 // the map and the ground truth of each direction
        const int d = m & 1, is_gt = m >> 1;
        uint8_t* dst = is_gt ? a.gt_image[d] : a.image[d];
        if (!dst) continue;
        const float2* S2 = reinterpret_cast<const float2*>(is_gt ? a.gt[d] : a.flow[d]) + f * HW;
        const float maxrad = rad_src[f * 4 + 2 * d + ((is_gt || a.share_gt_scale) ? 1 : 0)];
        const float div = (float)((double)maxrad + 2.220446049250313e-16);
        dst += f * HW * 3;
#pragma unroll
        for (int j = 0; j < FLOW_PX; ++j) {
            const int64_t p = b0 + j * FLOW_THREADS + tid;
            if (p >= HW) continue;
            const float2 w = S2[p];
            const bool kn = flow_known(w.x, w.y);
            const float u = (kn ? w.x : 0.f) / div, v = (kn ? w.y : 0.f) / div;
            const float rad = sqrtf(u * u + v * v);
            const float ang = atan2f(-v, -u) / pi;
            const float fk = (ang + 1.f) / 2.f * (float)(WHEEL - 1) + 1.f;
            const int k0 = min(max((int)floorf(fk), 1), WHEEL);   // (1 .. 55 for any finite input; a NaN scale cannot index outside)
            const int k1 = k0 == WHEEL ? 1 : k0 + 1;
            const float fr = fk - (float)k0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float col = (1.f - fr) * s_wheel[(k0 - 1) * 3 + c] + fr * s_wheel[(k1 - 1) * 3 + c];
                col = rad <= 1.f ? 1.f - rad * (1.f - col) : col * 0.75f;
                const float q = floorf(255.f * col);
                dst[p * 3 + c] = kn && q == q ? (uint8_t)(int)fminf(fmaxf(q, 0.f), 255.f) : (uint8_t)0;
            }
        }
    }
}

inline int64_t flow_blocks(int64_t n_pixels) { return (n_pixels + FLOW_BLOCK_PX - 1) / FLOW_BLOCK_PX; }

}  // namespace

extern "C" int64_t nsff_flow_maps_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    return frame_dims_ok(n_frames, H, W) ? frame_scratch_bytes(n_frames, flow_blocks((int64_t)H * W), FLOW_WORDS) : 0;
}

extern "C" int nsff_flow_maps(const NsffFlowMapsArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    const bool project = a->xyz[0] || a->xyz[1];
    const bool epe = a->epe_sums || a->epe_counts;
    const bool colour = a->image[0] || a->image[1] || a->gt_image[0] || a->gt_image[1];
    bool scored = false;
    for (int d = 0; d < 2; ++d) {
        if (a->xyz[d] && !a->flow[d]) return NSFF_ERR_NULL;                          // points without a map to write
        if (a->image[d] && !a->flow[d]) return NSFF_ERR_INVALID;                     // an image without its map
        if (a->gt_image[d] && !a->gt[d]) return NSFF_ERR_INVALID;
        if (a->gt[d] && !a->flow[d]) return NSFF_ERR_INVALID;                        // a ground truth goes with a map of its direction
        if (a->image[d] && a->share_gt_scale && !a->scale && !a->gt[d]) return NSFF_ERR_INVALID;   // the ground truth's radius needs it
        scored = scored || (a->flow[d] && a->gt[d]);
    }
    if (project) {
        if (!a->Ps || !a->ts) return NSFF_ERR_NULL;
        if (a->n_poses < 1 || a->max_t < 0 || a->max_t >= a->n_poses) return NSFF_ERR_INVALID;
        if (!(a->fx < 0.f || a->fx > 0.f) || !(a->fy < 0.f || a->fy > 0.f)) return NSFF_ERR_INVALID;   // zero or NaN
    }
    if (epe && (!a->epe_sums || !a->epe_counts || !scored)) return NSFF_ERR_INVALID; // sums and counts go together and need a pair
    if (a->mask && !epe) return NSFF_ERR_INVALID;
    if (a->maxrad && !a->flow[0] && !a->flow[1]) return NSFF_ERR_INVALID;
    if (colour && !a->scale && !a->maxrad) return NSFF_ERR_INVALID;                   // the colour scale: given, or reduced here
    if (!project && !epe && !a->maxrad && !colour) return NSFF_ERR_INVALID;          // nothing to compute
    const bool reduce = epe || a->maxrad;
    if (reduce && !a->scratch) return NSFF_ERR_NULL;
    if (reduce && a->scratch_bytes < nsff_flow_maps_scratch_bytes(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if (((uintptr_t)a->scratch & 15) || (((uintptr_t)a->epe_sums | (uintptr_t)a->epe_counts) & 7)) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->flow[0] | (uintptr_t)a->flow[1] | (uintptr_t)a->gt[0] | (uintptr_t)a->gt[1]) & 7) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->xyz[0] | (uintptr_t)a->xyz[1] | (uintptr_t)a->Ps | (uintptr_t)a->ts | (uintptr_t)a->maxrad | (uintptr_t)a->scale) & 3)
        return NSFF_ERR_ALIGN;
    const FrameScratch s = frame_scratch_split(a->scratch, a->n_frames);
    const dim3 grid((unsigned)flow_blocks((int64_t)a->H * a->W), a->n_frames);
    if (project || reduce)
        hipLaunchKernelGGL(flow_map_kernel, grid, dim3(FLOW_THREADS), 0, (hipStream_t)stream, *a, reduce ? 1 : 0, s.counters, s.partials);
    if (colour)
        hipLaunchKernelGGL(flow_colour_kernel, grid, dim3(FLOW_THREADS), 0, (hipStream_t)stream, *a, a->scale ? a->scale : a->maxrad);
    return nsff_launch_status();
}
