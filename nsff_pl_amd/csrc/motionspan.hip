// Motion masks over several frames (nsff_motion_span, nsff_mask_propagate): the epipolar test of nsff_motion_maps (motion.hip)
// against every neighbour f +- 1 .. f +- span a pixel reaches by chaining optical flow, and "dynamic" carried along the same chain
// from the frames f +- 1 .. f +- reach.  One frame's test misses an object that drifts less than the threshold a frame off its
// epipolar line, in every frame, and an object that pauses, in the frames of the pause; followed for k frames the drift is k times
// as large while the chained flow's noise grows like sqrt(k) (hop_scale), and a paused pixel is dynamic in a frame nearby.
//
// include/nsff_render.h states every step as a chain of single fp32 operations; this file is built -ffp-contract=off and
// tests/motionspan_numpy.py is the same chain in numpy, compared bit for bit.  The chain, its hop and the line distance are
// nsff_flow_chain.h's: line_distance is what motion.hip's motion_map_kernel calls, and the hop is the one parallax.hip's
// disparity_span_kernel has written out, here without its `masks` plane, so with span = 1, hop_scale = {1} and nsff_motion_maps' own `valid` the
// raw map and the over-counts are nsff_motion_maps', which tests/test_motionspan_gpu.py pins.
//
// motion_span_kernel -- all F frames, both directions and all hops in ONE launch, on the pixel quads of nsff_frame_ops.h.  Frame f,
//   direction d (0: s = +1, flow_fw; 1: s = -1, flow_bw): the chain starts with A = flow_d[f] at the pixel; at step k it MEASURES the
//   distance of pixel + A from the line Fm[f][d][k-1] (pixel) in the neighbour n = f + s k, scaled by hop_scale[k-1], and keeps the
//   largest; then it HOPS: b = flow_d[n] sampled bilinearly at q = pixel + A, A += b, and the chain stays alive only if q is inside
//   the image and the four taps are known and valid.  The chain state of a lane's four pixels (A, alive, best, hops) stays in
//   registers across the hops.  The matrices and scales are wave-uniform loads; the loop bounds (span, the sequence ends) are
//   uniform in a workgroup.  The taps of a hop are read by hop_taps: without a branch, from q clamped into the image, the two taps of
//   a row in one load.
// mask_propagate_kernel -- the same chain; at step k it looks src[n] up at q rounded to the nearest pixel (half to even), from q
//   clamped likewise, and counts the zero (dynamic) pixels a living chain meets.
// The counts of each frame go through frame_count_finish of nsff_frame_ops.h, which leaves the scratch all zero between calls.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_flow_chain.h"

namespace {

constexpr int SPAN_WORDS = 2, PROP_WORDS = 1;                     // one workgroup's share of a frame: 3 uint32 counts; 1

// (four waves a SIMD asked for: left alone the allocator takes 129 VGPRs, one more than four waves allow; asked, 124 and no scratch,
// and 2 to 5 % less time at 512 x 288, F = 30: DESIGN.md section 11.3)
__global__ __launch_bounds__(FIN_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void motion_span_kernel(
    NsffMotionSpanArgs a, int aligned, unsigned* __restrict__ counters, frame_word* __restrict__ partials) {
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W;
    const Quad q = quad_of(blockIdx.x, tid, f, HW, aligned);
    const float wmax = (float)(a.W - 1), hmax = (float)(a.H - 1);
    float xs[FIN_PX], ys[FIN_PX];
    quad_pixels(q, HW, a.W, xs, ys);

    uint32_t cnt[3] = {0u, 0u, 0u};                               // over fw, over bw, dynamic
    bool moving[FIN_PX] = {false, false, false, false};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int s = d == 0 ? 1 : -1;
        // the steps of this direction: up to span, fewer at the sequence ends (uniform in the workgroup)
        const int steps = min(a.span, d == 0 ? a.n_frames - 1 - (int)f : (int)f);
        const float* flow = d == 0 ? a.flow_fw : a.flow_bw;
        Chain c;
        chain_start(c, flow, a.valid, q, f, d, HW);
        float best[FIN_PX] = {0.f, 0.f, 0.f, 0.f};
        uint32_t hops[FIN_PX] = {0u, 0u, 0u, 0u};
        for (int k = 1; k <= steps; ++k) {
            const int64_t n = f + s * k;                          // 0 <= n < F by `steps`
            const bool hop = k < steps;                           // n + s is a frame too, and k < span
            Taps t;                                               // the hop's taps first, so that their latency overlaps the measurement
            if (hop)                                              // (uniform)
                hop_taps(t, c, xs, ys, reinterpret_cast<const float2*>(flow) + n * HW, a.valid ? a.valid + (n * 2 + d) * HW : nullptr,
                         a.H, a.W);
            float M[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) M[i] = a.Fm[((f * 2 + d) * a.span + (k - 1)) * 9 + i];
            const float scale = a.hop_scale[k - 1];
#pragma unroll
            for (int i = 0; i < FIN_PX; ++i) {
                const float qx = xs[i] + c.A[2 * i], qy = ys[i] + c.A[2 * i + 1];
                float e;
                bool line_ok;
                line_distance(M, xs[i], ys[i], qx, qy, e, line_ok);
                const bool take = c.alive[i] && line_ok;
                best[i] = take ? fmaxf(best[i], e * scale) : best[i];
                hops[i] += take ? 1u : 0u;
                if (hop) hop_pixel(c, t, i, qx, qy, wmax, hmax);  // (uniform)
            }
        }
        float ev[FIN_PX];
#pragma unroll
        for (int i = 0; i < FIN_PX; ++i) {
            ev[i] = hops[i] ? best[i] : NSFF_FLOW_UNKNOWN;
            const bool over = hops[i] != 0u && best[i] > a.threshold;
            cnt[d] += over ? 1u : 0u;
            moving[i] = moving[i] || over;
        }
        const Quad qd = quad_of(blockIdx.x, tid, f * 2 + d, HW, aligned);     // the direction's plane of err / hops
        if (qd.n > 0) {
            if (a.err) store_px<1>(a.err, qd, ev);
            if (a.hops) store_bytes<FIN_PX>(a.hops + qd.q0, hops, qd.n, qd.vec);
        }
    }
    uint32_t rb[FIN_PX];
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        rb[i] = moving[i] ? 0u : 255u;
        cnt[2] += moving[i] ? 1u : 0u;
    }
    if (q.n > 0) store_bytes<FIN_PX>(a.raw + q.q0, rb, q.n, q.vec);
    if (a.counts) frame_count_finish<3, FIN_THREADS>(cnt, a.counts, counters, partials, f);
}

__global__ __launch_bounds__(FIN_THREADS) void mask_propagate_kernel(NsffMaskPropagateArgs a, int aligned, unsigned* __restrict__ counters,
                                                                     frame_word* __restrict__ partials) {
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W;
    const Quad q = quad_of(blockIdx.x, tid, f, HW, aligned);
    const float wmax = (float)(a.W - 1), hmax = (float)(a.H - 1);
    float xs[FIN_PX], ys[FIN_PX];
    quad_pixels(q, HW, a.W, xs, ys);

    uint32_t hits[FIN_PX] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int s = d == 0 ? 1 : -1;
        const int steps = min(a.reach, d == 0 ? a.n_frames - 1 - (int)f : (int)f);      // (uniform in the workgroup)
        const float* flow = d == 0 ? a.flow_fw : a.flow_bw;
        Chain c;
        chain_start(c, flow, a.valid, q, f, d, HW);
        for (int k = 1; k <= steps; ++k) {
            const int64_t n = f + s * k;                          // 0 <= n < F by `steps`
            const bool hop = k < steps;                           // n + s is a frame too, and k < reach
            Taps t;
            if (hop)                                              // (uniform)
                hop_taps(t, c, xs, ys, reinterpret_cast<const float2*>(flow) + n * HW, a.valid ? a.valid + (n * 2 + d) * HW : nullptr,
                         a.H, a.W);
            // the neighbour's mask at q rounded to the nearest pixel, from q clamped into the frame: no branch, no address outside
            const uint8_t* S = a.src + n * HW;
            uint32_t sv[FIN_PX];
#pragma unroll
            for (int i = 0; i < FIN_PX; ++i) {
                const float cx = fminf(fmaxf(xs[i] + c.A[2 * i], 0.f), wmax);
                const float cy = fminf(fmaxf(ys[i] + c.A[2 * i + 1], 0.f), hmax);
                const int xi = min((int)rintf(cx), a.W - 1), yi = min((int)rintf(cy), a.H - 1);      // (W - 1 as a float may round up)
                sv[i] = S[yi * a.W + xi];
            }
#pragma unroll
            for (int i = 0; i < FIN_PX; ++i) {
                const float qx = xs[i] + c.A[2 * i], qy = ys[i] + c.A[2 * i + 1];
                const bool inside = qx >= 0.f && qx <= wmax && qy >= 0.f && qy <= hmax;
                hits[i] += (c.alive[i] && inside && sv[i] == 0u) ? 1u : 0u;
                if (hop) hop_pixel(c, t, i, qx, qy, wmax, hmax);  // (uniform)
            }
        }
    }
    uint32_t out[FIN_PX];
    uint32_t zeros = 0u;
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        const uint32_t own = i < q.n ? (uint32_t)a.src[q.q0 + i] : 255u;
        out[i] = (own == 0u || hits[i] > 0u) ? 0u : own;
        zeros += (i < q.n && out[i] == 0u) ? 1u : 0u;
    }
    if (q.n > 0) {
        store_bytes<FIN_PX>(a.dst + q.q0, out, q.n, q.vec);
        if (a.hits) store_bytes<FIN_PX>(a.hits + q.q0, hits, q.n, q.vec);
    }
    if (a.zero_counts) frame_count_finish<1, FIN_THREADS>({zeros}, a.zero_counts, counters, partials, f);
}

}  // namespace

// one size for both calls: the span pass's partials are the larger
extern "C" int64_t nsff_motion_span_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (!frame_dims_ok(n_frames, H, W)) return 0;
    return frame_scratch_bytes(n_frames, fin_blocks((int64_t)H * W), SPAN_WORDS);
}

extern "C" int nsff_motion_span(const NsffMotionSpanArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if (a->span < 1 || a->span > NSFF_MOTION_MAX_SPAN) return NSFF_ERR_INVALID;
    if (!not_negative(a->threshold)) return NSFF_ERR_INVALID;
    if (!a->flow_fw || !a->flow_bw || !a->Fm || !a->hop_scale || !a->raw) return NSFF_ERR_NULL;
    if (a->counts && !a->scratch) return NSFF_ERR_NULL;
    if (a->counts && a->scratch_bytes < frame_scratch_bytes(a->n_frames, fin_blocks((int64_t)a->H * a->W), SPAN_WORDS)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->counts) & 7) return NSFF_ERR_ALIGN;
    if (off4(a->Fm) || off4(a->hop_scale) || off4(a->err)) return NSFF_ERR_ALIGN;
    const int aligned = ((((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->err) & 15) == 0
                         && (((uintptr_t)a->hops | (uintptr_t)a->raw) & 3) == 0) ? 1 : 0;
    const FrameScratch s = frame_scratch_split(a->counts ? a->scratch : nullptr, a->n_frames);
    const dim3 grid((unsigned)fin_blocks((int64_t)a->H * a->W), a->n_frames);
    hipLaunchKernelGGL(motion_span_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned, s.counters, s.partials);
    return nsff_launch_status();
}

extern "C" int nsff_mask_propagate(const NsffMaskPropagateArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if (a->reach < 1 || a->reach > NSFF_PROPAGATE_MAX_REACH) return NSFF_ERR_INVALID;
    if (!a->src || !a->dst || !a->flow_fw || !a->flow_bw) return NSFF_ERR_NULL;
    if (overlap(a->src, a->dst, (int64_t)a->n_frames * a->H * a->W)) return NSFF_ERR_INVALID;
    if (a->zero_counts && !a->scratch) return NSFF_ERR_NULL;
    if (a->zero_counts && a->scratch_bytes < frame_scratch_bytes(a->n_frames, fin_blocks((int64_t)a->H * a->W), PROP_WORDS)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->zero_counts) & 7) return NSFF_ERR_ALIGN;
    const int aligned = ((((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw) & 15) == 0
                         && (((uintptr_t)a->dst | (uintptr_t)a->hits) & 3) == 0) ? 1 : 0;
    const FrameScratch s = frame_scratch_split(a->zero_counts ? a->scratch : nullptr, a->n_frames);
    const dim3 grid((unsigned)fin_blocks((int64_t)a->H * a->W), a->n_frames);
    hipLaunchKernelGGL(mask_propagate_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned, s.counters, s.partials);
    return nsff_launch_status();
}
