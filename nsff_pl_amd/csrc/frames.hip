// Per-frame 8-bit image outputs: eval frame finishing and the trainer's validation panels.  Both use the pixel quads and the
// per-frame reduction of nsff_frame_ops.h.
//
// nsff_frame_finish: the per-frame finishing work of the reference's eval.py on F rendered frames -- clip(rgb, 0, 1), the 8-bit
// image (255 * clip) truncated (eval.py:183-184, 213-214, 222-223), the squared-error sums of metrics.psnr over the whole frame
// and over the valid pixels (metrics.py:6-16), and the normalised 8-bit depth of utils/visualization.py:10-15 with its colour
// table lookup.  Two launches: frame_image_kernel streams the image once (and reduces the sums and the depth range),
// frame_depth_kernel quantises the depth with the range the first one wrote.  Which values a lane, a wave and a workgroup add
// depends on H * W alone (the pixel quads), so a frame's sums are the same bits at any position of any batch.
//
// nsff_val_panels: the image panels of train.py:209-235, 254-257 (see the header), on the same pixel decomposition.  Two launches:
// panel_range_kernel reduces the range of each scalar field, panel_compose_kernel writes the 8-bit tiles with them.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_frame_ops.h"

namespace {

constexpr int FIN_WORDS = 4;                                      // one workgroup's share of a frame: 3 fp64 sums, depth min | max << 32

__global__ __launch_bounds__(FIN_THREADS) void frame_image_kernel(NsffFrameFinishArgs a, int aligned, unsigned* __restrict__ counters,
                                                                  frame_word* __restrict__ partials) {
    __shared__ double s_sum[FIN_THREADS / 64][3];
    __shared__ float s_mm[FIN_THREADS / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.y;
    const Quad px = quad_of(blockIdx.x, tid, f, (int64_t)a.H * a.W, aligned);
    const int n = px.n;

    float r[3 * FIN_PX], g[3 * FIN_PX], d[FIN_PX];
    uint32_t v[FIN_PX] = {0u, 0u, 0u, 0u};
    load_px<3>(a.rgb, px, r);
    load_px<3>(a.gt, px, g);
    load_px<1>(a.depth, px, d);
    if (a.valid) {
        if (px.vec) {
            const uint32_t t = *reinterpret_cast<const uint32_t*>(a.valid + px.q0);
            v[0] = t & 255u; v[1] = (t >> 8) & 255u; v[2] = (t >> 16) & 255u; v[3] = t >> 24;
        } else {
#pragma unroll
            for (int k = 0; k < FIN_PX; ++k)
                if (k < n) v[k] = a.valid[px.q0 + k];
        }
    }

    double acc[3] = {0.0, 0.0, 0.0};                              // squared error, the same over valid pixels, valid pixels
    float mn = INFINITY, mx = -INFINITY;
    uint32_t q[3 * FIN_PX];
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float cl = clip01(r[3 * k + c]);
            r[3 * k + c] = cl;
            q[3 * k + c] = trunc_u8(255.f * cl);
            if (k < n && a.gt) {
                const float e = g[3 * k + c] - cl;
                const double sq = (double)(e * e);                // the square in fp32 (torch), the sum in fp64
                acc[0] += sq;
                if (v[k]) acc[1] += sq;
            }
        }
        if (k < n) {
            if (v[k]) acc[2] += 1.0;
            const float x = nan_to_num(d[k]);
            mn = fminf(mn, x); mx = fmaxf(mx, x);
        }
    }
    if (n > 0) {
        if (a.rgb_clipped) store_px<3>(a.rgb_clipped, px, r);
        if (a.rgb_u8) store_bytes(a.rgb_u8 + px.q0 * 3, q, 3 * n, px.vec);
    }
    if (!a.sums && !a.depth_range) return;

#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = wave_sum(acc[t]);
    mn = wave_min(mn); mx = wave_max(mx);
    if (lane == 0) { s_sum[wave][0] = acc[0]; s_sum[wave][1] = acc[1]; s_sum[wave][2] = acc[2]; s_mm[wave][0] = mn; s_mm[wave][1] = mx; }
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_blocks = gridDim.x;
    frame_word* fp = partials + f * n_blocks * FIN_WORDS;
    const frame_word mine[FIN_WORDS] = {pack_double(sum4(s_sum, 0)), pack_double(sum4(s_sum, 1)), pack_double(sum4(s_sum, 2)),
                                        pack2(min4(s_mm, 0), max4(s_mm, 1))};
    if (!frame_publish(fp, counters + f, blockIdx.x, n_blocks, lane, mine)) return;
    double tot[3] = {0.0, 0.0, 0.0};
    mn = INFINITY; mx = -INFINITY;
    frame_fold<FIN_WORDS>(fp, n_blocks, lane, [&](const frame_word (&w)[FIN_WORDS]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tot[k] += word_double(w[k]);
        mn = fminf(mn, word_lo_f(w[3])); mx = fmaxf(mx, word_hi_f(w[3]));
    });
#pragma unroll
    for (int k = 0; k < 3; ++k) tot[k] = wave_sum(tot[k]);
    mn = wave_min(mn); mx = wave_max(mx);
    if (lane == 0) {
        if (a.sums) { a.sums[f * 3 + 0] = tot[0]; a.sums[f * 3 + 1] = tot[1]; a.sums[f * 3 + 2] = tot[2]; }
        if (a.depth_range) { a.depth_range[f * 2 + 0] = mn; a.depth_range[f * 2 + 1] = mx; }
        frame_counter_reset(counters + f);
    }
}

// visualize_depth (utils/visualization.py:10-15) with the frame's own range
__global__ __launch_bounds__(FIN_THREADS) void frame_depth_kernel(NsffFrameFinishArgs a, int aligned) {
    __shared__ uint8_t s_lut[768];
    const int tid = threadIdx.x;
    if (a.depth_rgb_u8) {
        for (int i = tid; i < 768; i += FIN_THREADS) s_lut[i] = a.lut[i];
        __syncthreads();
    }
    const int64_t f = blockIdx.y;
    const Quad px = quad_of(blockIdx.x, tid, f, (int64_t)a.H * a.W, aligned);
    if (px.n == 0) return;
    const float mi = a.depth_range[f * 2], ma = a.depth_range[f * 2 + 1];
    const float span = (ma - mi) + 1e-8f;
    float d[FIN_PX];
    load_px<1>(a.depth, px, d);
    uint32_t idx[FIN_PX], col[3 * FIN_PX];
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) idx[k] = depth_index(nan_to_num(d[k]), mi, span);
    if (a.depth_u8) store_bytes(a.depth_u8 + px.q0, idx, px.n, px.vec);
    if (a.depth_rgb_u8) {
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) col[3 * k + c] = s_lut[idx[k] * 3 + c];
        store_bytes(a.depth_rgb_u8 + px.q0 * 3, col, 3 * px.n, px.vec);
    }
}

// ---- nsff_val_panels ----
constexpr int PAN_FIELDS = 5;                                     // depth, static depth, -disp, -rmse, -ssim
constexpr int PAN_WORDS = PAN_FIELDS;                             // one workgroup's share of a frame: min | max << 32 per field
constexpr int PAN_PAD_THREADS = FIN_THREADS;                      // one padding pixel of the grid per thread

// The five scalar fields of a lane's four pixels after nan_to_num, each a chain of single fp32 operations; pc = clip(pred, 0, 1)
// and g = gt are handed on to the composer.
__device__ __forceinline__ void pan_fields(const NsffValPanelsArgs& a, const Quad& px, float (&x)[PAN_FIELDS][FIN_PX],
                                           float (&pc)[3 * FIN_PX], float (&g)[3 * FIN_PX]) {
    float d[FIN_PX], sd[FIN_PX], di[FIN_PX], l[3 * FIN_PX];
    load_px<3>(a.gt, px, g);
    load_px<3>(a.pred, px, pc);
    load_px<1>(a.depth, px, d);
    load_px<1>(a.static_depth, px, sd);
    load_px<1>(a.disp, px, di);
    load_px<3>(a.ssim_loss, px, l);
#pragma unroll
    for (int i = 0; i < 3 * FIN_PX; ++i) pc[i] = clip01(pc[i]);
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) {
        const float d0 = g[3 * k] - pc[3 * k], d1 = g[3 * k + 1] - pc[3 * k + 1], d2 = g[3 * k + 2] - pc[3 * k + 2];
        const float rmse = sqrtf(((d0 * d0 + d1 * d1) + d2 * d2) / 3.0f);                 // IEEE division and square root
        const float ssim = (((1.0f - l[3 * k]) + (1.0f - l[3 * k + 1])) + (1.0f - l[3 * k + 2])) / 3.0f;
        x[0][k] = nan_to_num(d[k]);
        x[1][k] = nan_to_num(sd[k]);
        x[2][k] = nan_to_num(-di[k]);
        x[3][k] = nan_to_num(-rmse);
        x[4][k] = nan_to_num(-ssim);
    }
}

__global__ __launch_bounds__(FIN_THREADS) void panel_range_kernel(NsffValPanelsArgs a, int aligned, unsigned* __restrict__ counters,
                                                                  frame_word* __restrict__ partials) {
    __shared__ float s_mn[FIN_THREADS / 64][PAN_FIELDS], s_mx[FIN_THREADS / 64][PAN_FIELDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.y;
    const Quad px = quad_of(blockIdx.x, tid, f, (int64_t)a.H * a.W, aligned);

    float x[PAN_FIELDS][FIN_PX], pc[3 * FIN_PX], g[3 * FIN_PX];
    pan_fields(a, px, x, pc, g);
    float mn[PAN_FIELDS], mx[PAN_FIELDS];
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t) {
        mn[t] = INFINITY; mx[t] = -INFINITY;
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k)
            if (k < px.n) { mn[t] = fminf(mn[t], x[t][k]); mx[t] = fmaxf(mx[t], x[t][k]); }
        mn[t] = wave_min(mn[t]); mx[t] = wave_max(mx[t]);
        if (lane == 0) { s_mn[wave][t] = mn[t]; s_mx[wave][t] = mx[t]; }
    }
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_blocks = gridDim.x;
    frame_word* fp = partials + f * n_blocks * PAN_WORDS;
    frame_word mine[PAN_WORDS];
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t) mine[t] = pack2(min4(s_mn, t), max4(s_mx, t));
    if (!frame_publish(fp, counters + f, blockIdx.x, n_blocks, lane, mine)) return;
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t) { mn[t] = INFINITY; mx[t] = -INFINITY; }
    frame_fold<PAN_WORDS>(fp, n_blocks, lane, [&](const frame_word (&w)[PAN_WORDS]) {
#pragma unroll
        for (int t = 0; t < PAN_FIELDS; ++t) { mn[t] = fminf(mn[t], word_lo_f(w[t])); mx[t] = fmaxf(mx[t], word_hi_f(w[t])); }
    });
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t) { mn[t] = wave_min(mn[t]); mx[t] = wave_max(mx[t]); }
    if (lane == 0) {
        const bool have[PAN_FIELDS] = {a.depth != nullptr, a.static_depth != nullptr, a.disp != nullptr, a.gt != nullptr,
                                       a.ssim_loss != nullptr};
        for (int t = 0; t < PAN_FIELDS; ++t)
            if (have[t]) { a.ranges[(f * PAN_FIELDS + t) * 2] = mn[t]; a.ranges[(f * PAN_FIELDS + t) * 2 + 1] = mx[t]; }
        frame_counter_reset(counters + f);
    }
}

// Four pixels (px[k] = r | g << 8 | b << 16) of the tile in cell `slot` of the grid of one frame (G = its first byte).  A lane
// whose four pixels lie in one image row owns 12 consecutive bytes at any byte offset (3-byte pixels, odd row lengths): the
// bytes up to the next dword boundary go out one by one, the rest as dwords shifted into place.
__device__ __forceinline__ void grid_store(uint8_t* __restrict__ G, int slot, int H, int W, int GW, const Quad& q,
                                           const uint32_t (&px)[FIN_PX]) {
    const int gy0 = (slot / 3) * (H + 2) + 2, gx0 = (slot % 3) * (W + 2) + 2;
    const int y = (int)(q.p0 / W), x = (int)(q.p0 - (int64_t)y * W);
    if (q.n == FIN_PX && x + FIN_PX <= W) {
        uint8_t* dst = G + ((int64_t)(gy0 + y) * GW + gx0 + x) * 3;
        const uint32_t w0 = px[0] | (px[1] << 24), w1 = (px[1] >> 8) | (px[2] << 16), w2 = (px[2] >> 16) | (px[3] << 8);
        const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 3);
        if (m == 0) {
            uint32_t* o = reinterpret_cast<uint32_t*>(dst);
            o[0] = w0; o[1] = w1; o[2] = w2;
        } else {
            const unsigned h = 4 - m, sh = 8 * h;                 // h = 1..3 head bytes, then two dwords, then m tail bytes
            for (unsigned i = 0; i < h; ++i) dst[i] = (uint8_t)(w0 >> (8 * i));
            uint32_t* o = reinterpret_cast<uint32_t*>(dst + h);
            o[0] = (w0 >> sh) | (w1 << (32 - sh));
            o[1] = (w1 >> sh) | (w2 << (32 - sh));
            for (unsigned i = 0; i < m; ++i) dst[h + 8 + i] = (uint8_t)(w2 >> (sh + 8 * i));
        }
    } else {
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) {
            if (k >= q.n) continue;
            const int64_t p = q.p0 + k;
            const int yy = (int)(p / W), xx = (int)(p - (int64_t)yy * W);
            uint8_t* dst = G + ((int64_t)(gy0 + yy) * GW + gx0 + xx) * 3;
            dst[0] = (uint8_t)px[k]; dst[1] = (uint8_t)(px[k] >> 8); dst[2] = (uint8_t)(px[k] >> 16);
        }
    }
}

// three 8-bit channels of pixel k of v as r | g << 8 | b << 16
__device__ __forceinline__ uint32_t rgb_of(const uint32_t (&v)[3 * FIN_PX], int k) { return v[3 * k] | (v[3 * k + 1] << 8) | (v[3 * k + 2] << 16); }

// Launch 2.  Workgroups blockIdx.x < n_px_blocks compose the pixels; the ones behind them zero the grid's padding, one padding
// pixel per thread: first the 2 (ymaps + 1) full padding rows, then the four 2-pixel column strips of every image row.
__global__ __launch_bounds__(FIN_THREADS) void panel_compose_kernel(NsffValPanelsArgs a, int aligned, int n_px_blocks) {
    __shared__ uint8_t s_lut[2][768];                             // depth (JET) and mask (BONE) tables; NULL = the index itself
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W;
    const bool transient = a.transient_alpha != nullptr;
    const int slot_mask = transient ? 6 : 3, slot_disp = slot_mask + (a.mask ? 1 : 0);
    const int n_tiles = slot_disp + (a.disp ? 1 : 0), ymaps = (n_tiles + 2) / 3;
    const int GW = 3 * (W + 2) + 2, GH = ymaps * (H + 2) + 2;
    const int64_t f = blockIdx.y;
    uint8_t* G = a.grid_u8 ? a.grid_u8 + f * GH * (int64_t)GW * 3 : nullptr;

    if ((int)blockIdx.x >= n_px_blocks) {                         // (only launched with a grid)
        const int64_t t = ((int64_t)blockIdx.x - n_px_blocks) * PAN_PAD_THREADS + tid;
        const int64_t n_row = 2 * (int64_t)(ymaps + 1) * GW, n_col = 8 * (int64_t)ymaps * H;
        if (t >= n_row + n_col) return;
        int64_t gy, gx;
        if (t < n_row) {
            const int64_t r = t / GW;
            gx = t - r * GW;
            gy = (r >> 1) * (H + 2) + (r & 1);
        } else {
            const int64_t u = t - n_row, row = u >> 3;
            const int s = (int)(u & 7);
            gx = (int64_t)(s >> 1) * (W + 2) + (s & 1);
            gy = (row / H) * (H + 2) + 2 + row % H;
        }
        uint8_t* dst = G + (gy * GW + gx) * 3;
        dst[0] = 0; dst[1] = 0; dst[2] = 0;
        return;
    }

    for (int i = tid; i < 768; i += FIN_THREADS) {
        s_lut[0][i] = a.lut_depth ? a.lut_depth[i] : (uint8_t)(i / 3);
        s_lut[1][i] = a.lut_mask ? a.lut_mask[i] : (uint8_t)(i / 3);
    }
    __syncthreads();
    const Quad lq = quad_of(blockIdx.x, tid, f, (int64_t)H * W, aligned);
    if (lq.n == 0) return;

    float x[PAN_FIELDS][FIN_PX], pc[3 * FIN_PX], g[3 * FIN_PX];
    pan_fields(a, lq, x, pc, g);
    const bool have[PAN_FIELDS] = {a.depth != nullptr, a.static_depth != nullptr, a.disp != nullptr, a.gt != nullptr,
                                   a.ssim_loss != nullptr};
    uint32_t idx[PAN_FIELDS][FIN_PX], col[PAN_FIELDS][FIN_PX];   // visualize_depth's index and its colour, packed
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t) {
        const float mi = have[t] ? a.ranges[(f * PAN_FIELDS + t) * 2] : 0.f, ma = have[t] ? a.ranges[(f * PAN_FIELDS + t) * 2 + 1] : 0.f;
        const float span = (ma - mi) + 1e-8f;
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) {
            idx[t][k] = depth_index(x[t][k], mi, span);
            col[t][k] = lut_rgb(s_lut[0], idx[t][k]);
        }
    }
    uint32_t pu[3 * FIN_PX];                                      // rgb_u8 of the clipped prediction
#pragma unroll
    for (int i = 0; i < 3 * FIN_PX; ++i) pu[i] = trunc_u8(255.f * pc[i]);

    if (a.rmse_u8) store_bytes(a.rmse_u8 + lq.q0, idx[3], lq.n, lq.vec);
    if (a.ssim_u8) store_bytes(a.ssim_u8 + lq.q0, idx[4], lq.n, lq.vec);
#pragma unroll
    for (int e = 0; e < 2; ++e) {                                 // blend_images(img, visualize_depth(-map), 0.5)
        uint8_t* out = e == 0 ? a.rmse_blend_u8 : a.ssim_blend_u8;
        if (!out) continue;
        uint32_t q[3 * FIN_PX];
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t s = pu[3 * k + c] + ((col[3 + e][k] >> (8 * c)) & 255u);
                q[3 * k + c] = min(255u, (s >> 1) + 2u + (s & 1u));
            }
        store_bytes(out + lq.q0 * 3, q, 3 * lq.n, lq.vec);
    }
    if (!G) return;

    uint32_t px[FIN_PX], gu[3 * FIN_PX];
#pragma unroll
    for (int i = 0; i < 3 * FIN_PX; ++i) gu[i] = trunc_u8(255.f * g[i]);
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) px[k] = rgb_of(gu, k);
    grid_store(G, 0, H, W, GW, lq, px);
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) px[k] = rgb_of(pu, k);
    grid_store(G, 1, H, W, GW, lq, px);
    grid_store(G, 2, H, W, GW, lq, col[0]);
    if (transient) {
        float ta[FIN_PX], sr[3 * FIN_PX];
        load_px<1>(a.transient_alpha, lq, ta);
        load_px<3>(a.static_rgb, lq, sr);
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) px[k] = lut_rgb(s_lut[1], trunc_u8(255.f * ta[k]));   // visualize_mask(transient_alpha)
        grid_store(G, 3, H, W, GW, lq, px);
#pragma unroll
        for (int i = 0; i < 3 * FIN_PX; ++i) gu[i] = trunc_u8(255.f * clip01(sr[i]));
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) px[k] = rgb_of(gu, k);
        grid_store(G, 4, H, W, GW, lq, px);
        grid_store(G, 5, H, W, GW, lq, col[1]);
    }
    if (a.mask) {
        float mk[FIN_PX];
        load_px<1>(a.mask, lq, mk);
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) px[k] = lut_rgb(s_lut[1], trunc_u8(255.f * (1.0f - mk[k])));   // visualize_mask(1 - mask)
        grid_store(G, slot_mask, H, W, GW, lq, px);
    }
    if (a.disp) grid_store(G, slot_disp, H, W, GW, lq, col[2]);
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) px[k] = 0u;
    for (int s = n_tiles; s < 3 * ymaps; ++s) grid_store(G, s, H, W, GW, lq, px);   // unfilled cells of the last row
}

}  // namespace

extern "C" int64_t nsff_frame_finish_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    return frame_dims_ok(n_frames, H, W) ? frame_scratch_bytes(n_frames, fin_blocks((int64_t)H * W), FIN_WORDS) : 0;
}

extern "C" int nsff_frame_finish(const NsffFrameFinishArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!a->rgb) return NSFF_ERR_INVALID;                                        // no image: nothing to finish
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    const bool depth_out = a->depth_u8 || a->depth_rgb_u8;
    if (a->depth_rgb_u8 && !a->lut) return NSFF_ERR_INVALID;                     // a colour image needs the colour table
    if ((a->sums && !a->gt) || ((a->depth_range || depth_out) && !a->depth)) return NSFF_ERR_INVALID;
    if (depth_out && !a->depth_range) return NSFF_ERR_INVALID;                   // the second launch reads the range there
    const bool reduce = a->sums || a->depth_range;
    if (!a->rgb_clipped && !a->rgb_u8 && !reduce) return NSFF_ERR_INVALID;       // nothing to compute
    if (reduce && !a->scratch) return NSFF_ERR_NULL;
    if (reduce && a->scratch_bytes < nsff_frame_finish_scratch_bytes(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if (((uintptr_t)a->scratch & 15) || ((uintptr_t)a->sums & 7)) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->rgb | (uintptr_t)a->gt | (uintptr_t)a->depth | (uintptr_t)a->rgb_clipped | (uintptr_t)a->depth_range) & 3)
        return NSFF_ERR_ALIGN;
    // the 16-byte / dword path needs every array it touches that way aligned; otherwise every lane goes element by element
    const uintptr_t wide = (uintptr_t)a->rgb | (uintptr_t)a->gt | (uintptr_t)a->depth | (uintptr_t)a->rgb_clipped;
    const uintptr_t narrow = (uintptr_t)a->valid | (uintptr_t)a->rgb_u8 | (uintptr_t)a->depth_u8 | (uintptr_t)a->depth_rgb_u8;
    const int aligned = !(wide & 15) && !(narrow & 3);
    const FrameScratch s = frame_scratch_split(a->scratch, a->n_frames);
    const dim3 grid((unsigned)fin_blocks((int64_t)a->H * a->W), a->n_frames);
    hipLaunchKernelGGL(frame_image_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned, s.counters, s.partials);
    if (depth_out) hipLaunchKernelGGL(frame_depth_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned);
    return nsff_launch_status();
}

extern "C" int64_t nsff_val_panels_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    return frame_dims_ok(n_frames, H, W) ? frame_scratch_bytes(n_frames, fin_blocks((int64_t)H * W), PAN_WORDS) : 0;
}

extern "C" int nsff_val_panels(const NsffValPanelsArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!a->pred) return NSFF_ERR_INVALID;                                       // no prediction: no panel
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    const int n_transient = (a->transient_alpha != nullptr) + (a->static_rgb != nullptr) + (a->static_depth != nullptr);
    if (n_transient != 0 && n_transient != 3) return NSFF_ERR_INVALID;           // the three transient tiles come together
    if (a->grid_u8 && (!a->gt || !a->depth)) return NSFF_ERR_INVALID;            // its first three tiles
    if ((a->rmse_u8 || a->rmse_blend_u8) && !a->gt) return NSFF_ERR_INVALID;
    if ((a->ssim_u8 || a->ssim_blend_u8) && !a->ssim_loss) return NSFF_ERR_INVALID;
    const bool compose = a->grid_u8 || a->rmse_u8 || a->ssim_u8 || a->rmse_blend_u8 || a->ssim_blend_u8;
    if (!a->ranges) return NSFF_ERR_INVALID;                                     // nothing to compute / the second launch reads them there
    if (!a->depth && !a->static_depth && !a->disp && !a->gt && !a->ssim_loss) return NSFF_ERR_INVALID;   // no field to range
    if (!a->scratch) return NSFF_ERR_NULL;
    if (a->scratch_bytes < nsff_val_panels_scratch_bytes(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    const uintptr_t wide = (uintptr_t)a->gt | (uintptr_t)a->pred | (uintptr_t)a->depth | (uintptr_t)a->transient_alpha |
                           (uintptr_t)a->static_rgb | (uintptr_t)a->static_depth | (uintptr_t)a->mask | (uintptr_t)a->disp |
                           (uintptr_t)a->ssim_loss;
    if ((wide | (uintptr_t)a->ranges) & 3) return NSFF_ERR_ALIGN;
    // the 16-byte / dword path needs every array it touches that way aligned (the grid is stored by address, whatever its base)
    const uintptr_t narrow = (uintptr_t)a->rmse_u8 | (uintptr_t)a->ssim_u8 | (uintptr_t)a->rmse_blend_u8 | (uintptr_t)a->ssim_blend_u8;
    const int aligned = !(wide & 15) && !(narrow & 3);
    const FrameScratch s = frame_scratch_split(a->scratch, a->n_frames);
    const int64_t nb = fin_blocks((int64_t)a->H * a->W);
    hipLaunchKernelGGL(panel_range_kernel, dim3((unsigned)nb, a->n_frames), dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned,
                       s.counters, s.partials);
    if (compose) {
        int64_t pad_blocks = 0;
        if (a->grid_u8) {
            const int64_t n_tiles = 3 + n_transient + (a->mask != nullptr) + (a->disp != nullptr), ymaps = (n_tiles + 2) / 3;
            const int64_t pad_px = 2 * (ymaps + 1) * (3 * ((int64_t)a->W + 2) + 2) + 8 * ymaps * a->H;
            pad_blocks = (pad_px + PAN_PAD_THREADS - 1) / PAN_PAD_THREADS;
        }
        hipLaunchKernelGGL(panel_compose_kernel, dim3((unsigned)(nb + pad_blocks), a->n_frames), dim3(FIN_THREADS), 0,
                           (hipStream_t)stream, *a, aligned, (int)nb);
    }
    return nsff_launch_status();
}
