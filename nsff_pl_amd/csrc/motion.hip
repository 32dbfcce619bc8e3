// Motion masks from optical flow and camera poses: a pixel is moving when its flow leaves the epipolar line that the two camera
// poses predict for it; a pixel whose flow fails the forward-backward check is occluded or unreliable and has no vote.  The
// geometric route of the original NSFF pipeline, where the reference runs Mask-RCNN (third_party/predict_mask.py) -- and the
// 15 x 15 erosion that ends that script (line 63: it widens the dynamic area "to account for inaccurate boundaries").
//
// nsff_motion_maps, one launch:
//
// motion_map_kernel -- all F frames, both directions.  Frame f, direction d: neighbour n = f + 1 (fw) / f - 1 (bw), A = flow_fw[f],
//   B = flow_bw[n] (fw) / A = flow_bw[f], B = flow_fw[n] (bw), M = Fm[f][d] (nine wave-uniform values).  At the pixel (x, y), every
//   step one fp32 operation in this order (built -ffp-contract=off; IEEE division and square root):
//     a = A[y][x], known: |.| <= 1e7 in both components, not NaN;  qx = x + a.u, qy = y + a.v;  inside: 0 <= q <= (W-1, H-1)
//     b = B at q, bilinear: x0 = floorf(qx), ax = qx - x0, x1 = min(x0 + 1, W-1), y likewise,
//         b = ((B00 * (1 - ax) + B01 * ax) * (1 - ay)) + ((B10 * (1 - ax) + B11 * ax) * ay) per component, all four taps known
//     s = a + b, lhs = s.u s.u + s.v s.v, rhs = alpha ((a.u a.u + a.v a.v) + (b.u b.u + b.v b.v)) + beta, consistent: lhs <= rhs
//     l_i = (M[i][0] x + M[i][1] y) + M[i][2], r = (l0 qx + l1 qy) + l2, n = l0 l0 + l1 l1, e = |r| / sqrtf(n), line_ok: 0 < n < inf
//   err = e where neighbour, known and line_ok, else NSFF_FLOW_UNKNOWN; valid = neighbour, known, inside, taps, consistent, line_ok;
//   raw = 0 where a direction is valid with e > threshold, else 255.  flow_known, bilerp and line_distance are nsff_flow_chain.h's,
//   which nsff_motion_span (motionspan.hip) measures with too.  The taps are read without a branch, from q clamped into the
//   image (the identity where q is inside, where alone they are used), so no address leaves the neighbour's frame whatever the
//   flow holds and the sixteen loads of a lane's four pixels are in flight together.
//
// The pixel quads of nsff_frame_ops.h: a workgroup owns 1024 consecutive pixels of one frame and a lane four consecutive ones; err
// and valid are (F, 2, H*W), so a direction's plane f * 2 + d has a quad of its own (its flat index decides whether it is
// vectorised).  Per frame: the counts of valid and over pixels and the fp64 sum of e over the valid ones, per direction, and the
// count of dynamic pixels -- the ticketed reduction of nsff_frame_ops.h; the frame's last workgroup also returns the partials it
// read to zero, so the scratch is all zero between calls.  (The tail carries fp64 sums beside its counts, so it is written out
// here; a kernel that only counts ends in frame_count_finish.)
//
// nsff_mask_erode, one launch:
//
// mask_erode_kernel -- the minimum over a k x k window, separable: a 64 x 32 tile with its halo of k / 2 pixels goes to LDS (as
//   ssim_kernel holds its tile), pixels outside the image as 255 -- they do not contribute, OpenCV's default border for morphology --
//   then a horizontal and a vertical pass of k minima each.  The count of zero pixels per frame goes through frame_count_finish.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_flow_chain.h"

namespace {

constexpr int MOTION_WORDS = 5;                                   // one workgroup's share of a frame: 2 fp64 sums, 5 uint32 counts
__global__ __launch_bounds__(FIN_THREADS) void motion_map_kernel(NsffMotionMapsArgs a, int aligned, unsigned* __restrict__ counters,
                                                                 frame_word* __restrict__ partials) {
    __shared__ double s_sum[FIN_THREADS / 64][2];
    __shared__ uint32_t s_cnt[FIN_THREADS / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W;
    const Quad q = quad_of(blockIdx.x, tid, f, HW, aligned);
    const float wmax = (float)(a.W - 1), hmax = (float)(a.H - 1);

    // The lane's four pixels (pxs, pys), held as ints and converted at each use: held as floats the kernel takes 94 VGPRs for 100 and runs five waves a SIMD for four, and
    // measured 3.8 % slower at 512 x 288, F = 30 on random flow.
    int pxs[FIN_PX], pys[FIN_PX];
    quad_pixels(q, HW, a.W, pxs, pys);

    double sum[2] = {0.0, 0.0};
    uint32_t cnt[5] = {0u, 0u, 0u, 0u, 0u};                       // valid fw, valid bw, over fw, over bw, dynamic
    bool moving[FIN_PX] = {false, false, false, false};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int64_t n = d == 0 ? f + 1 : f - 1;
        const bool neighbour = n >= 0 && n < a.n_frames;          // (uniform in the workgroup)
        float ev[FIN_PX] = {NSFF_FLOW_UNKNOWN, NSFF_FLOW_UNKNOWN, NSFF_FLOW_UNKNOWN, NSFF_FLOW_UNKNOWN};
        uint32_t vv[FIN_PX] = {0u, 0u, 0u, 0u};
        if (neighbour) {
            const float2* B = reinterpret_cast<const float2*>(d == 0 ? a.flow_bw : a.flow_fw) + n * HW;
            float M[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) M[i] = a.epipolar ? a.Fm[(f * 2 + d) * 9 + i] : 0.f;
            float av[2 * FIN_PX];
            load_px<2>(d == 0 ? a.flow_fw : a.flow_bw, q, av);
            // The taps of all four pixels first, without a branch, so that their latencies overlap.  Their addresses come from q
            // clamped into the image -- the identity where q is inside; elsewhere (a NaN clamps to 0, a pixel past the frame's end
            // to a pixel of it) the taps are read and not used, and no address leaves the neighbour's frame.
            float2 b00[FIN_PX], b01[FIN_PX], b10[FIN_PX], b11[FIN_PX];
#pragma unroll
            for (int i = 0; i < FIN_PX; ++i) {
                const float cx = fminf(fmaxf((float)pxs[i] + av[2 * i], 0.f), wmax);
                const float cy = fminf(fmaxf((float)pys[i] + av[2 * i + 1], 0.f), hmax);
                const int x0 = (int)floorf(cx), y0 = (int)floorf(cy);
                const int x1 = min(x0 + 1, a.W - 1), y1 = min(y0 + 1, a.H - 1);
                b00[i] = B[(int64_t)y0 * a.W + x0]; b01[i] = B[(int64_t)y0 * a.W + x1];
                b10[i] = B[(int64_t)y1 * a.W + x0]; b11[i] = B[(int64_t)y1 * a.W + x1];
            }
#pragma unroll
            for (int i = 0; i < FIN_PX; ++i) {
                const float u = av[2 * i], v = av[2 * i + 1];
                const bool kn = i < q.n && flow_known(u, v);
                const float x = (float)pxs[i], y = (float)pys[i];
                const float qx = x + u, qy = y + v;
                const bool inside = qx >= 0.f && qx <= wmax && qy >= 0.f && qy <= hmax;
                const float ax = qx - floorf(qx), ay = qy - floorf(qy);
                const float omx = 1.f - ax, omy = 1.f - ay;
                const float bu = bilerp(b00[i].x, b01[i].x, b10[i].x, b11[i].x, ax, omx, ay, omy);
                const float bv = bilerp(b00[i].y, b01[i].y, b10[i].y, b11[i].y, ax, omx, ay, omy);
                const float su = u + bu, sv = v + bv;
                const float lhs = su * su + sv * sv;
                const float rhs = a.alpha * ((u * u + v * v) + (bu * bu + bv * bv)) + a.beta;
                bool ok = kn && inside && flow_known(b00[i]) && flow_known(b01[i]) && flow_known(b10[i]) && flow_known(b11[i]) && lhs <= rhs;
                bool over = false;
                if (a.epipolar) {                                 // (uniform)
                    float e;
                    bool line_ok;
                    line_distance(M, x, y, qx, qy, e, line_ok);
                    if (kn && line_ok) ev[i] = e;
                    ok = ok && line_ok;
                    over = ok && e > a.threshold;
                    sum[d] += ok ? (double)e : 0.0;               // the term in fp32, the sum in fp64
                }
                vv[i] = ok ? 1u : 0u;
                cnt[d] += vv[i];
                cnt[2 + d] += over ? 1u : 0u;
                moving[i] = moving[i] || over;
            }
        }
        const Quad qd = quad_of(blockIdx.x, tid, f * 2 + d, HW, aligned);     // the direction's plane of err / valid
        if (qd.n > 0) {
            if (a.err) store_px<1>(a.err, qd, ev);
            if (a.valid) store_bytes<FIN_PX>(a.valid + qd.q0, vv, qd.n, qd.vec);
        }
    }
    uint32_t rb[FIN_PX];
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        rb[i] = moving[i] ? 0u : 255u;
        cnt[4] += moving[i] ? 1u : 0u;
    }
    if (a.raw && q.n > 0) store_bytes<FIN_PX>(a.raw + q.q0, rb, q.n, q.vec);
    if (!a.counts) return;

#pragma unroll
    for (int d = 0; d < 2; ++d) sum[d] = wave_sum(sum[d]);
#pragma unroll
    for (int k = 0; k < 5; ++k) cnt[k] = wave_sum(cnt[k]);
    if (lane == 0) {
        s_sum[wave][0] = sum[0]; s_sum[wave][1] = sum[1];
#pragma unroll
        for (int k = 0; k < 5; ++k) s_cnt[wave][k] = cnt[k];
    }
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_blocks = gridDim.x;
    frame_word* fp = partials + f * n_blocks * MOTION_WORDS;
    const frame_word mine[MOTION_WORDS] = {pack_double(sum4(s_sum, 0)), pack_double(sum4(s_sum, 1)),
                                           pack2(sum4(s_cnt, 0), sum4(s_cnt, 1)), pack2(sum4(s_cnt, 2), sum4(s_cnt, 3)),
                                           pack2(sum4(s_cnt, 4), 0u)};
    if (!frame_publish(fp, counters + f, blockIdx.x, n_blocks, lane, mine)) return;
    double tot[2] = {0.0, 0.0};
    long long n[5] = {0, 0, 0, 0, 0};
    frame_fold<MOTION_WORDS>(fp, n_blocks, lane, [&](const frame_word (&w)[MOTION_WORDS]) {
        tot[0] += word_double(w[0]); tot[1] += word_double(w[1]);
        n[0] += (long long)word_lo(w[2]); n[1] += (long long)word_hi(w[2]);
        n[2] += (long long)word_lo(w[3]); n[3] += (long long)word_hi(w[3]);
        n[4] += (long long)word_lo(w[4]);
    });
    for (unsigned b = lane; b < n_blocks; b += 64)                // what this lane read goes back to zero: the scratch is all zero again
#pragma unroll
        for (int i = 0; i < MOTION_WORDS; ++i) fp[(int64_t)b * MOTION_WORDS + i] = 0ull;
#pragma unroll
    for (int i = 0; i < 2; ++i) tot[i] = wave_sum(tot[i]);
#pragma unroll
    for (int i = 0; i < 5; ++i) n[i] = wave_sum(n[i]);
    if (lane == 0) {
        for (int i = 0; i < 5; ++i) a.counts[f * 5 + i] = (int64_t)n[i];
        a.err_sums[f * 2] = tot[0];
        a.err_sums[f * 2 + 1] = tot[1];
        frame_counter_reset(counters + f);
    }
}

constexpr int ER_THREADS = 256, ER_TW = 64, ER_TH = 32, ER_R = NSFF_ERODE_MAX_K / 2;
constexpr int ER_PH = ER_TH + 2 * ER_R, ER_PW = (ER_TW + 2 * ER_R + 3) & ~3;
// The k minima of a pass are taken ER_BATCH LDS reads at a time, the index held at k - 1 past the window's end (the last element
// again: a minimum does not mind), so that a batch's reads are in flight together; one read per turn of a loop of unknown length
// waits out the LDS latency k times.
constexpr int ER_BATCH = 8;

__global__ __launch_bounds__(ER_THREADS) void mask_erode_kernel(NsffMaskErodeArgs a, int tiles_x, unsigned* __restrict__ counters,
                                                                frame_word* __restrict__ partials) {
    __shared__ uint8_t s_in[ER_PH][ER_PW];
    __shared__ uint8_t s_h[ER_PH][ER_TW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = tile_x * ER_TW, y0 = tile_y * ER_TH;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W;
    const uint8_t* S = a.src + f * HW;
    uint8_t* D = a.dst + f * HW;
    const int r = a.k / 2, pw = ER_TW + 2 * r, ph = ER_TH + 2 * r;

    // the tile and its halo, a row per wave: outside the image 255, which no minimum keeps (read from the clamped address, so that
    // the loads carry no branch)
#pragma unroll 4
    for (int rr = wave; rr < ph; rr += ER_THREADS / 64) {
        const int gy = y0 - r + rr;
        const uint8_t* row = S + (int64_t)min(max(gy, 0), a.H - 1) * a.W;
#pragma unroll
        for (int cc = lane; cc < ER_PW; cc += 64) {               // (two turns: the second covers the halo's rest)
            const int gx = x0 - r + cc;
            const uint8_t v = row[min(max(gx, 0), a.W - 1)];
            if (cc < pw) s_in[rr][cc] = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? v : (uint8_t)255;
        }
    }
    __syncthreads();
    for (int rr = wave; rr < ph; rr += ER_THREADS / 64) {         // horizontal pass: ph rows x 64 columns
        uint32_t m = 255u;
        for (int j0 = 0; j0 < a.k; j0 += ER_BATCH)
#pragma unroll
            for (int t = 0; t < ER_BATCH; ++t) m = min(m, (uint32_t)s_in[rr][lane + min(j0 + t, a.k - 1)]);
        s_h[rr][lane] = (uint8_t)m;
    }
    __syncthreads();
    uint32_t zeros = 0u;
    const int ox = x0 + lane;
#pragma unroll
    for (int t = 0; t < ER_TH / (ER_THREADS / 64); ++t) {         // vertical pass
        const int ty = wave + (ER_THREADS / 64) * t, oy = y0 + ty;
        uint32_t m = 255u;
        for (int j0 = 0; j0 < a.k; j0 += ER_BATCH)
#pragma unroll
            for (int t = 0; t < ER_BATCH; ++t) m = min(m, (uint32_t)s_h[ty + min(j0 + t, a.k - 1)][lane]);
        if (ox < a.W && oy < a.H) {
            D[(int64_t)oy * a.W + ox] = (uint8_t)m;
            zeros += m == 0u ? 1u : 0u;
        }
    }
    if (a.zero_counts) frame_count_finish<1, ER_THREADS>({zeros}, a.zero_counts, counters, partials, f);
}

inline int64_t erode_tiles(int32_t H, int32_t W) {
    return (((int64_t)W + ER_TW - 1) / ER_TW) * (((int64_t)H + ER_TH - 1) / ER_TH);
}

}  // namespace

// one size for both calls: the larger of the map pass's and the erosion's partials
extern "C" int64_t nsff_motion_maps_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (!frame_dims_ok(n_frames, H, W)) return 0;
    const int64_t maps = frame_scratch_bytes(n_frames, fin_blocks((int64_t)H * W), MOTION_WORDS);
    const int64_t erode = frame_scratch_bytes(n_frames, erode_tiles(H, W), 1);
    return maps > erode ? maps : erode;
}

extern "C" int nsff_motion_maps(const NsffMotionMapsArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if (a->epipolar != 0 && a->epipolar != 1) return NSFF_ERR_INVALID;
    if (!not_negative(a->alpha) || !not_negative(a->beta) || !not_negative(a->threshold)) return NSFF_ERR_INVALID;
    if (!a->err && !a->valid && !a->raw && !a->counts && !a->err_sums) return NSFF_ERR_INVALID;      // nothing to compute
    if ((a->counts == nullptr) != (a->err_sums == nullptr)) return NSFF_ERR_INVALID;                 // counts and sums go together
    if (!a->flow_fw || !a->flow_bw) return NSFF_ERR_NULL;
    if (a->epipolar && !a->Fm) return NSFF_ERR_NULL;
    if (a->counts && !a->scratch) return NSFF_ERR_NULL;
    if (a->counts && a->scratch_bytes < frame_scratch_bytes(a->n_frames, fin_blocks((int64_t)a->H * a->W), MOTION_WORDS)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->counts | (uintptr_t)a->err_sums) & 7) return NSFF_ERR_ALIGN;
    if (off4(a->Fm) || off4(a->err)) return NSFF_ERR_ALIGN;
    const int aligned = ((((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->err) & 15) == 0
                         && (((uintptr_t)a->valid | (uintptr_t)a->raw) & 3) == 0) ? 1 : 0;
    const FrameScratch s = frame_scratch_split(a->counts ? a->scratch : nullptr, a->n_frames);
    const dim3 grid((unsigned)fin_blocks((int64_t)a->H * a->W), a->n_frames);
    hipLaunchKernelGGL(motion_map_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned, s.counters, s.partials);
    return nsff_launch_status();
}

extern "C" int nsff_mask_erode(const NsffMaskErodeArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if (a->k < 1 || a->k > NSFF_ERODE_MAX_K || (a->k & 1) == 0) return NSFF_ERR_INVALID;
    if (!a->src || !a->dst) return NSFF_ERR_NULL;
    if (a->src == a->dst) return NSFF_ERR_INVALID;
    if (a->zero_counts && !a->scratch) return NSFF_ERR_NULL;
    if (a->zero_counts && a->scratch_bytes < frame_scratch_bytes(a->n_frames, erode_tiles(a->H, a->W), 1)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    if ((uintptr_t)a->zero_counts & 7) return NSFF_ERR_ALIGN;
    const FrameScratch s = frame_scratch_split(a->zero_counts ? a->scratch : nullptr, a->n_frames);
    const dim3 grid((unsigned)erode_tiles(a->H, a->W), a->n_frames);
    const int tiles_x = (a->W + ER_TW - 1) / ER_TW;
    hipLaunchKernelGGL(mask_erode_kernel, grid, dim3(ER_THREADS), 0, (hipStream_t)stream, *a, tiles_x, s.counters, s.partials);
    return nsff_launch_status();
}
