// Disparity of a static pixel triangulated over several frames by chaining optical flow (nsff_disparity_span): the measurement of
// nsff_disparity_sparse (depth.hip) against every baseline f +- 1 .. f +- span instead of f +- 1 alone.  A slow camera moves a
// fraction of a pixel of parallax per frame, which min_parallax rejects; followed along the flow for k frames a pixel has k times
// the parallax while the chained flow's noise grows like sqrt(k).
//
// include/nsff_render.h states every step as a chain of single fp32 operations; this file is built -ffp-contract=off and
// tests/parallax_numpy.py is the same chain in numpy, compared bit for bit.  The vote is parallax_vote of nsff_flow_chain.h, which
// depth.hip's disparity_sparse_kernel calls too: with span = 1 the two kernels give the same bits, which
// tests/test_parallax_gpu.py pins.  flow_known, bilerp, the paired tap loads, quad_pixels and the count's tail are shared as well.
//
// The hop itself is written out here and NOT taken from nsff_flow_chain.h's Chain / hop_taps / hop_pixel, which motionspan.hip
// calls: it is the same hop with a second byte plane (`masks`), but built on those helpers this kernel compiles to 121 VGPRs for 111
// and moves 144 scalar registers through vector lanes in the hop loop for 96, and measured 2.2 to 3.0 % slower at span 4 and 8
// (512 x 288, F = 30, taken in turn with the parent's build in two calls: span 4 145.4, 145.6 against 141.2, 142.0 us, span 8 252.0,
// 252.2 against 246.0, 247.2).  The margin is the larger of the two parent runs' difference in the call and 2 %, so this is just
// outside it, in both calls: a marginal result, worth taking again when the compiler changes.  With four waves a SIMD asked for
// (110 VGPRs) the compiler waits after every byte load and the kernel is 16 to 32 % slower; three other spellings of the chain
// state measured as the first.  Until then a fix to the tap addressing is made in hop_taps AND here; tests/test_parallax_gpu.py and tests/test_motionspan_gpu.py pin both to their twins,
// which share one numpy hop.
//
// disparity_span_kernel -- all F frames, both directions and all hops in ONE launch, on the pixel quads of nsff_frame_ops.h.  Frame
//   f, direction d (0: s = +1, flow_fw; 1: s = -1, flow_bw): the chain starts with A = flow_d[f] at the pixel; at step k it VOTES with
//   A against the row Pm[f][d][k-1] of the neighbour n = f + s k, then HOPS: b = flow_d[n] sampled bilinearly at q = pixel + A (the
//   rule of nsff_motion_maps), A += b, and the chain stays alive only if q is inside the image and the four taps are known, valid
//   and static.  The chain state of a lane's four pixels (A, alive, the three sums, the vote count) stays in registers across the
//   hops; no intermediate map is written.  The rows are wave-uniform loads; the loop bounds (span, the sequence ends) are uniform
//   in a workgroup.  A hop's sixteen flow taps of a lane are read without a branch from q clamped into the image (the identity
//   where q is inside, where alone they are used), so no address leaves the neighbour's frame whatever the flow holds -- NaN (it
//   clamps to 0), +-inf, 1e10, the garbage a dead chain goes on adding up -- and the loads are in flight together.  The two taps
//   of a row are neighbours in memory and come with one load (flow: 16 bytes; valid and masks: two bytes), from the column
//   xl = min(x0, W - 2) on, so that at the right edge, where x1 == x0 == W - 1, the pair still lies in the row: a hop costs a lane
//   24 gathers instead of 48, and measured 27 us instead of 47 at 512 x 288, F = 30.  A frame one pixel
//   wide has no such pair and reads its single column.
//   The known pixels of each frame are counted through frame_count_finish of nsff_frame_ops.h.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_flow_chain.h"

namespace {

__global__ __launch_bounds__(FIN_THREADS) void disparity_span_kernel(NsffDisparitySpanArgs a, float mp2, int aligned,
                                                                     unsigned* __restrict__ counters, frame_word* __restrict__ partials) {
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W;
    const Quad q = quad_of(blockIdx.x, tid, f, HW, aligned);
    const float wmax = (float)(a.W - 1), hmax = (float)(a.H - 1);

    float xs[FIN_PX], ys[FIN_PX];
    quad_pixels(q, HW, a.W, xs, ys);
    float num[FIN_PX] = {0.f, 0.f, 0.f, 0.f}, den[FIN_PX] = {0.f, 0.f, 0.f, 0.f}, par[FIN_PX] = {0.f, 0.f, 0.f, 0.f};
    uint32_t nv[FIN_PX] = {0u, 0u, 0u, 0u};
    bool is_static[FIN_PX];
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) is_static[i] = i < q.n && (!a.masks || a.masks[q.q0 + i] != 0);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int s = d == 0 ? 1 : -1;
        // the steps of this direction: up to span, fewer at the sequence ends (uniform in the workgroup)
        const int steps = min(a.span, d == 0 ? a.n_frames - 1 - (int)f : (int)f);
        const float* flow = d == 0 ? a.flow_fw : a.flow_bw;
        float A[2 * FIN_PX];
        load_px<2>(flow, q, A);
        bool alive[FIN_PX];
        const int64_t plane = (f * 2 + d) * HW + q.p0;            // the direction's plane of `valid`
#pragma unroll
        for (int i = 0; i < FIN_PX; ++i) {
            alive[i] = is_static[i] && flow_known(A[2 * i], A[2 * i + 1]);
            if (a.valid) alive[i] = alive[i] && a.valid[plane + i] != 0;
        }
        for (int k = 1; k <= steps; ++k) {
            const int64_t n = f + s * k;                          // 0 <= n < F by `steps`
            const bool hop = k < steps;                           // n + s is a frame too, and k < span
            // the hop's taps first, so that their latency overlaps the vote: addresses from q clamped into frame n
            float2 b00[FIN_PX], b01[FIN_PX], b10[FIN_PX], b11[FIN_PX];
            bool taps_ok[FIN_PX] = {true, true, true, true};
            if (hop) {                                            // (uniform)
                const float2* B = reinterpret_cast<const float2*>(flow) + n * HW;
                const uint8_t* V = a.valid ? a.valid + (n * 2 + d) * HW : nullptr;
                const uint8_t* S = a.masks ? a.masks + n * HW : nullptr;
                int r0[FIN_PX], r1[FIN_PX];                       // the taps' rows from their left column on: pixel indices within a frame are ints
                bool first[FIN_PX];                               // x0 is that column (not at the right edge, where x1 == x0 == W - 1)
#pragma unroll
                for (int i = 0; i < FIN_PX; ++i) {
                    const float cx = fminf(fmaxf(xs[i] + A[2 * i], 0.f), wmax);
                    const float cy = fminf(fmaxf(ys[i] + A[2 * i + 1], 0.f), hmax);
                    const int x0 = min((int)floorf(cx), a.W - 1), y0 = min((int)floorf(cy), a.H - 1);      // (W - 1 as a float may round up)
                    const int y1 = min(y0 + 1, a.H - 1);
                    const int xl = max(min(x0, a.W - 2), 0);      // xl and xl + 1 are columns of the image where W >= 2
                    first[i] = x0 == xl;
                    r0[i] = y0 * a.W + xl; r1[i] = y1 * a.W + xl;
                }
                if (a.W >= 2) {                                   // (uniform) x1 = min(x0 + 1, W - 1) is column xl + 1 in every case
#pragma unroll
                    for (int i = 0; i < FIN_PX; ++i) {
                        const flow_pair p0 = *reinterpret_cast<const flow_pair*>(B + r0[i]);
                        const flow_pair p1 = *reinterpret_cast<const flow_pair*>(B + r1[i]);
                        b01[i] = make_float2(p0.z, p0.w); b00[i] = first[i] ? make_float2(p0.x, p0.y) : b01[i];
                        b11[i] = make_float2(p1.z, p1.w); b10[i] = first[i] ? make_float2(p1.x, p1.y) : b11[i];
                    }
                    if (V) {                                      // (uniform)
#pragma unroll
                        for (int i = 0; i < FIN_PX; ++i) {
                            const bool top = pair_set(V + r0[i], first[i]), bot = pair_set(V + r1[i], first[i]);      // both read, no branch
                            taps_ok[i] = taps_ok[i] && top && bot;
                        }
                    }
                    if (S) {                                      // (uniform)
#pragma unroll
                        for (int i = 0; i < FIN_PX; ++i) {
                            const bool top = pair_set(S + r0[i], first[i]), bot = pair_set(S + r1[i], first[i]);      // both read, no branch
                            taps_ok[i] = taps_ok[i] && top && bot;
                        }
                    }
                } else {                                          // one column: x1 == x0 == 0
#pragma unroll
                    for (int i = 0; i < FIN_PX; ++i) {
                        b00[i] = b01[i] = B[r0[i]]; b10[i] = b11[i] = B[r1[i]];
                        if (V) taps_ok[i] = taps_ok[i] & (V[r0[i]] != 0) & (V[r1[i]] != 0);
                        if (S) taps_ok[i] = taps_ok[i] & (S[r0[i]] != 0) & (S[r1[i]] != 0);
                    }
                }
            }
            float P[12];
            bool row = false;                                     // (uniform in the workgroup)
#pragma unroll
            for (int i = 0; i < 12; ++i) { P[i] = a.Pm[((f * 2 + d) * a.span + (k - 1)) * 12 + i]; row = row || P[i] != 0.f; }
#pragma unroll
            for (int i = 0; i < FIN_PX; ++i) {
                const float u = A[2 * i], v = A[2 * i + 1];
                const float up = xs[i] + u, vp = ys[i] + v;
                float p2, ab, aa, hz;
                parallax_vote(P, xs[i], ys[i], up, vp, p2, ab, aa, hz);
                const bool vote = alive[i] && row && hz > 0.f && p2 >= mp2;
                num[i] = num[i] + (vote ? ab : 0.f);
                den[i] = den[i] + (vote ? aa : 0.f);
                par[i] = par[i] + (vote ? p2 : 0.f);
                nv[i] += vote ? 1u : 0u;
                // ---- the hop: q = (up, vp), the same two floats ----
                if (hop) {                                        // (uniform)
                    const bool inside = up >= 0.f && up <= wmax && vp >= 0.f && vp <= hmax;
                    const float fx = up - floorf(up), fy = vp - floorf(vp);
                    const float omx = 1.f - fx, omy = 1.f - fy;
                    const float bu = bilerp(b00[i].x, b01[i].x, b10[i].x, b11[i].x, fx, omx, fy, omy);
                    const float bv = bilerp(b00[i].y, b01[i].y, b10[i].y, b11[i].y, fx, omx, fy, omy);
                    alive[i] = alive[i] && inside && taps_ok[i] && flow_known(b00[i]) && flow_known(b01[i]) && flow_known(b10[i])
                               && flow_known(b11[i]);
                    A[2 * i] = u + bu;
                    A[2 * i + 1] = v + bv;
                }
            }
        }
    }
    float cv[FIN_PX], nn[FIN_PX];
    uint32_t cnt = 0u;
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        const bool kn = i < q.n && den[i] > 0.f && num[i] > 0.f;
        cv[i] = kn ? par[i] : 0.f;
        nn[i] = kn ? par[i] * (num[i] / den[i]) : 0.f;
        cnt += kn ? 1u : 0u;
    }
    if (q.n > 0) {
        store_px<1>(a.c, q, cv);
        store_px<1>(a.n, q, nn);
        if (a.votes) store_bytes<FIN_PX>(a.votes + q.q0, nv, q.n, q.vec);
    }
    if (a.counts) frame_count_finish<1, FIN_THREADS>({cnt}, a.counts, counters, partials, f);
}

}  // namespace

extern "C" int64_t nsff_disparity_span_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (!frame_dims_ok(n_frames, H, W)) return 0;
    return frame_scratch_bytes(n_frames, fin_blocks((int64_t)H * W), 1);
}

extern "C" int nsff_disparity_span(const NsffDisparitySpanArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if (a->span < 1 || a->span > NSFF_DISPARITY_MAX_SPAN) return NSFF_ERR_INVALID;
    if (!bounded_not_negative(a->min_parallax)) return NSFF_ERR_INVALID;
    if (!a->flow_fw || !a->flow_bw || !a->Pm || !a->n || !a->c) return NSFF_ERR_NULL;
    if (a->counts && !a->scratch) return NSFF_ERR_NULL;
    if (a->counts && a->scratch_bytes < nsff_disparity_span_scratch_bytes(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->counts) & 7) return NSFF_ERR_ALIGN;
    if (off4(a->Pm) || off4(a->n) || off4(a->c) || off4(a->votes)) return NSFF_ERR_ALIGN;
    const int aligned = ((((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->n | (uintptr_t)a->c) & 15) == 0) ? 1 : 0;
    const FrameScratch s = frame_scratch_split(a->counts ? a->scratch : nullptr, a->n_frames);
    const dim3 grid((unsigned)fin_blocks((int64_t)a->H * a->W), a->n_frames);
    hipLaunchKernelGGL(disparity_span_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, a->min_parallax * a->min_parallax, aligned,
                       s.counters, s.partials);
    return nsff_launch_status();
}
