// Motion masks over several frames (nsff_motion_span, nsff_mask_propagate): the epipolar test of nsff_motion_maps (motion.hip)
// against every neighbour f +- 1 .. f +- span a pixel reaches by chaining optical flow, and "dynamic" carried along the same chain
// from the frames f +- 1 .. f +- reach.  One frame's test misses an object that drifts less than the threshold a frame off its
// epipolar line, in every frame, and an object that pauses, in the frames of the pause; followed for k frames the drift is k times
// as large while the chained flow's noise grows like sqrt(k) (hop_scale), and a paused pixel is dynamic in a frame nearby.
//
// include/nsff_render.h states every step as a chain of single fp32 operations; this file is built -ffp-contract=off and
// tests/motionspan_numpy.py is the same chain in numpy, compared bit for bit.  The line distance is motion.hip's motion_map_kernel
// restated and the hop parallax.hip's disparity_span_kernel restated, without its mask test (both files stay as they are): with
// span = 1, hop_scale = {1} and nsff_motion_maps' own `valid` the raw map and the over-counts are nsff_motion_maps', which
// tests/test_motionspan_gpu.py pins.
//
// motion_span_kernel -- all F frames, both directions and all hops in ONE launch, on the pixel quads of nsff_frame_ops.h.  Frame f,
//   direction d (0: s = +1, flow_fw; 1: s = -1, flow_bw): the chain starts with A = flow_d[f] at the pixel; at step k it MEASURES the
//   distance of pixel + A from the line Fm[f][d][k-1] (pixel) in the neighbour n = f + s k, scaled by hop_scale[k-1], and keeps the
//   largest; then it HOPS: b = flow_d[n] sampled bilinearly at q = pixel + A, A += b, and the chain stays alive only if q is inside
//   the image and the four taps are known and valid.  The chain state of a lane's four pixels (A, alive, best, hops) stays in
//   registers across the hops.  The matrices and scales are wave-uniform loads; the loop bounds (span, the sequence ends) are
//   uniform in a workgroup.  The taps of a hop are read as disparity_span_kernel reads them: without a branch, from q clamped into
//   the image (the identity where q is inside, where alone they are used), so no address leaves the neighbour's frame whatever the
//   flow holds, the two taps of a row in one load from the column xl = min(x0, W - 2) on.
// mask_propagate_kernel -- the same chain; at step k it looks src[n] up at q rounded to the nearest pixel (half to even), from q
//   clamped likewise, and counts the zero (dynamic) pixels a living chain meets.
// The counts of each frame go through the ticketed reduction of nsff_frame_ops.h; the frame's last workgroup returns the partials
// it read to zero, so the scratch is all zero between calls.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <cfloat>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_frame_ops.h"

namespace {

constexpr float FLOW_THRESH = 1e7f;                               // flowlib's UNKNOWN_FLOW_THRESH
constexpr int SPAN_WORDS = 2, PROP_WORDS = 1;                     // one workgroup's share of a frame: 3 uint32 counts; 1

// both components within the threshold; a NaN fails the comparison
__device__ __forceinline__ bool flow_known(float u, float v) { return fabsf(u) <= FLOW_THRESH && fabsf(v) <= FLOW_THRESH; }
__device__ __forceinline__ bool flow_known(float2 w) { return flow_known(w.x, w.y); }

// B at (qx, qy) inside the image, one component: ((B00 (1 - ax) + B01 ax) (1 - ay)) + ((B10 (1 - ax) + B11 ax) ay)
__device__ __forceinline__ float bilerp(float b00, float b01, float b10, float b11, float ax, float omx, float ay, float omy) {
    const float top = b00 * omx + b01 * ax;
    const float bot = b10 * omx + b11 * ax;
    return (top * omy) + (bot * ay);
}

// Two horizontally adjacent taps in one load: 16 bytes of flow at an 8-byte aligned address, two bytes of valid at any address.
typedef float flow_pair __attribute__((ext_vector_type(4), aligned(8)));
typedef uint16_t byte_pair __attribute__((aligned(1)));
// the bytes at p[0] (only where `first`) and p[1] are both non-zero
__device__ __forceinline__ bool pair_set(const uint8_t* p, bool first) {
    const uint32_t v = *reinterpret_cast<const byte_pair*>(p);
    return ((v >> 8) != 0u) & (!first | ((v & 0xffu) != 0u));
}

// The chain of one direction of a lane's four pixels: A the flow summed so far, alive.
struct Chain {
    float A[2 * FIN_PX];
    bool alive[FIN_PX];
};

// The lane's four pixels, as motion_map_kernel steps them: (x, y) of the first by one division (any W >= 1).
__device__ __forceinline__ void quad_pixels(const Quad& q, int64_t HW, int W, float (&xs)[FIN_PX], float (&ys)[FIN_PX]) {
    const int p = (int)min(q.p0, HW - 1);
    int py = p / W, px = p - py * W;
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        xs[i] = (float)px; ys[i] = (float)py;
        if (++px == W) { px = 0; ++py; }
    }
}

// A = flow_d[f] at the lane's pixels; alive = a pixel of the frame, known, valid[f][d] != 0 where given
__device__ __forceinline__ void chain_start(Chain& c, const float* flow, const uint8_t* valid, const Quad& q, int64_t f, int d, int64_t HW) {
    load_px<2>(flow, q, c.A);
    const int64_t plane = (f * 2 + d) * HW + q.p0;                // the direction's plane of `valid`
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        c.alive[i] = i < q.n && flow_known(c.A[2 * i], c.A[2 * i + 1]);
        if (valid) c.alive[i] = c.alive[i] && valid[plane + i] != 0;
    }
}

// The four taps of a hop for each of the lane's pixels, read from q = pixel + A clamped into frame n (B its flow, V its plane of
// `valid` or NULL): every address is inside the frame whatever A holds (a NaN clamps to 0).
struct Taps {
    float2 b00[FIN_PX], b01[FIN_PX], b10[FIN_PX], b11[FIN_PX];
    bool ok[FIN_PX];
};
__device__ __forceinline__ void hop_taps(Taps& t, const Chain& c, const float (&xs)[FIN_PX], const float (&ys)[FIN_PX], const float2* B,
                                         const uint8_t* V, int H, int W) {
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    int r0[FIN_PX], r1[FIN_PX];                                   // the taps' rows from their left column on: pixel indices within a frame are ints
    bool first[FIN_PX];                                           // x0 is that column (not at the right edge, where x1 == x0 == W - 1)
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        const float cx = fminf(fmaxf(xs[i] + c.A[2 * i], 0.f), wmax);
        const float cy = fminf(fmaxf(ys[i] + c.A[2 * i + 1], 0.f), hmax);
        const int x0 = min((int)floorf(cx), W - 1), y0 = min((int)floorf(cy), H - 1);      // (W - 1 as a float may round up)
        const int y1 = min(y0 + 1, H - 1);
        const int xl = max(min(x0, W - 2), 0);                    // xl and xl + 1 are columns of the image where W >= 2
        first[i] = x0 == xl;
        r0[i] = y0 * W + xl; r1[i] = y1 * W + xl;
        t.ok[i] = true;
    }
    if (W >= 2) {                                                 // (uniform) x1 = min(x0 + 1, W - 1) is column xl + 1 in every case
#pragma unroll
        for (int i = 0; i < FIN_PX; ++i) {
            const flow_pair p0 = *reinterpret_cast<const flow_pair*>(B + r0[i]);
            const flow_pair p1 = *reinterpret_cast<const flow_pair*>(B + r1[i]);
            t.b01[i] = make_float2(p0.z, p0.w); t.b00[i] = first[i] ? make_float2(p0.x, p0.y) : t.b01[i];
            t.b11[i] = make_float2(p1.z, p1.w); t.b10[i] = first[i] ? make_float2(p1.x, p1.y) : t.b11[i];
        }
        if (V) {                                                  // (uniform)
#pragma unroll
            for (int i = 0; i < FIN_PX; ++i) {
                const bool top = pair_set(V + r0[i], first[i]), bot = pair_set(V + r1[i], first[i]);      // both read, no branch
                t.ok[i] = top && bot;
            }
        }
    } else {                                                      // one column: x1 == x0 == 0
#pragma unroll
        for (int i = 0; i < FIN_PX; ++i) {
            t.b00[i] = t.b01[i] = B[r0[i]]; t.b10[i] = t.b11[i] = B[r1[i]];
            if (V) t.ok[i] = (V[r0[i]] != 0) & (V[r1[i]] != 0);
        }
    }
}

// the hop of pixel i at q = (qx, qy), the two floats the step's measurement used: alive &&= hop_ok, A += b
__device__ __forceinline__ void hop_pixel(Chain& c, const Taps& t, int i, float qx, float qy, float wmax, float hmax) {
    const bool inside = qx >= 0.f && qx <= wmax && qy >= 0.f && qy <= hmax;
    const float fx = qx - floorf(qx), fy = qy - floorf(qy);
    const float omx = 1.f - fx, omy = 1.f - fy;
    const float bu = bilerp(t.b00[i].x, t.b01[i].x, t.b10[i].x, t.b11[i].x, fx, omx, fy, omy);
    const float bv = bilerp(t.b00[i].y, t.b01[i].y, t.b10[i].y, t.b11[i].y, fx, omx, fy, omy);
    c.alive[i] = c.alive[i] && inside && t.ok[i] && flow_known(t.b00[i]) && flow_known(t.b01[i]) && flow_known(t.b10[i])
                 && flow_known(t.b11[i]);
    c.A[2 * i] = c.A[2 * i] + bu;
    c.A[2 * i + 1] = c.A[2 * i + 1] + bv;
}

// (four waves a SIMD asked for: left alone the allocator takes 129 VGPRs, one more than four waves allow; asked, 124 and no scratch,
// and 2 to 5 % less time at 512 x 288, F = 30: DESIGN.md section 11.3)
__global__ __launch_bounds__(FIN_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void motion_span_kernel(
    NsffMotionSpanArgs a, int aligned, unsigned* __restrict__ counters, frame_word* __restrict__ partials) {
    __shared__ uint32_t s_cnt[FIN_THREADS / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
                // ---- the distance from the line: the arithmetic of motion_map_kernel (motion.hip), restated ----
                const float x = xs[i], y = ys[i];
                const float qx = x + c.A[2 * i], qy = y + c.A[2 * i + 1];
                const float l0 = (M[0] * x + M[1] * y) + M[2];
                const float l1 = (M[3] * x + M[4] * y) + M[5];
                const float l2 = (M[6] * x + M[7] * y) + M[8];
                const float r = (l0 * qx + l1 * qy) + l2;
                const float nn = l0 * l0 + l1 * l1;
                const float e = fabsf(r) / sqrtf(nn);
                const bool line_ok = nn > 0.f && nn <= FLT_MAX;   // finite and positive; a NaN fails both
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
    if (!a.counts) return;

#pragma unroll
    for (int k = 0; k < 3; ++k) cnt[k] = wave_sum(cnt[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s_cnt[wave][k] = cnt[k];
    }
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_blocks = gridDim.x;
    frame_word* fp = partials + f * n_blocks * SPAN_WORDS;
    const frame_word mine[SPAN_WORDS] = {pack2(sum4(s_cnt, 0), sum4(s_cnt, 1)), pack2(sum4(s_cnt, 2), 0u)};
    if (!frame_publish(fp, counters + f, blockIdx.x, n_blocks, lane, mine)) return;
    long long n[3] = {0, 0, 0};
    frame_fold<SPAN_WORDS>(fp, n_blocks, lane, [&](const frame_word (&w)[SPAN_WORDS]) {
        n[0] += (long long)word_lo(w[0]); n[1] += (long long)word_hi(w[0]); n[2] += (long long)word_lo(w[1]);
    });
    for (unsigned b = lane; b < n_blocks; b += 64)                // what this lane read goes back to zero: the scratch is all zero again
#pragma unroll
        for (int i = 0; i < SPAN_WORDS; ++i) fp[(int64_t)b * SPAN_WORDS + i] = 0ull;
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = wave_sum(n[i]);
    if (lane == 0) {
        for (int i = 0; i < 3; ++i) a.counts[f * 3 + i] = (int64_t)n[i];
        frame_counter_reset(counters + f);
    }
}

__global__ __launch_bounds__(FIN_THREADS) void mask_propagate_kernel(NsffMaskPropagateArgs a, int aligned, unsigned* __restrict__ counters,
                                                                     frame_word* __restrict__ partials) {
    __shared__ uint32_t s_cnt[FIN_THREADS / 64][1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    if (!a.zero_counts) return;

    zeros = wave_sum(zeros);
    if (lane == 0) s_cnt[wave][0] = zeros;
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_blocks = gridDim.x;
    frame_word* fp = partials + f * n_blocks * PROP_WORDS;
    const frame_word mine[PROP_WORDS] = {pack2(sum4(s_cnt, 0), 0u)};
    if (!frame_publish(fp, counters + f, blockIdx.x, n_blocks, lane, mine)) return;
    long long total = 0;
    frame_fold<PROP_WORDS>(fp, n_blocks, lane, [&](const frame_word (&w)[PROP_WORDS]) { total += (long long)word_lo(w[0]); });
    for (unsigned b = lane; b < n_blocks; b += 64) fp[b] = 0ull;  // the scratch is all zero again
    total = wave_sum(total);
    if (lane == 0) {
        a.zero_counts[f] = (int64_t)total;
        frame_counter_reset(counters + f);
    }
}

inline bool off4(const void* p) { return ((uintptr_t)p & 3) != 0; }
// a value that is neither negative nor NaN
inline bool not_negative(float v) { return v >= 0.f; }
// n bytes from a and n bytes from b share a byte
inline bool overlap(const void* a, const void* b, int64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)n && y < x + (uintptr_t)n;
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
