// SSIM metric and SSIM-driven ray sampling (the reference's metrics.ssim and its --hard_sampling dataset path).
//
// nsff_ssim: the per-pixel, per-channel SSIM loss of kornia 0.5.4's ssim_loss(gt, pred, window_size=11, reduction='none'),
// which the reference's metrics.py:19-33 turns into its metric 1 - loss.  Restated from kornia 0.5.4
// (kornia/losses/ssim.py, kornia/filters/filter.py::filter2d, kornia/filters/kernels.py::get_gaussian_kernel2d):
//   window  outer product of two normalised 1-D Gaussians, sigma 1.5, x = arange(11) - 5
//   filter  f(.) = 11x11 correlation after F.pad(mode='reflect') by 5 (edge pixel not repeated; needs H, W >= 6)
//   mu1 = f(x), mu2 = f(y), s11 = f(x^2) - mu1^2, s22 = f(y^2) - mu2^2, s12 = f(xy) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2
//   ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2) + 1e-12)
//   loss = clamp((1 - ssim) / 2, 0, 1)                                         (ssim_loss_form below)
// One workgroup per (frame, 64 x 16 output tile), one channel at a time: the tile and its 5-pixel halo are staged in LDS
// (reflect indexing at the load), a horizontal 11-tap pass writes the five moment planes to LDS, a vertical pass finishes
// them.  The moments are taken about one value per (tile, channel, image) -- the image's value at the tile centre: the
// variance terms are differences of near-equal numbers on flat images, and about a nearby value they are formed from
// small numbers (fp32 then holds the 1e-4 parity bar on a constant image with 1e-3 noise).  Per-frame reductions are
// per-tile partial sums in scratch that the frame's last-arriving workgroup adds up in tile order, in fp64 (no float
// atomics; bit-reproducible): the ticketed reduction of nsff_frame_ops.h.
//
// nsff_cdf: per-frame inclusive scan of the sampling weights in fp64 (an fp32 running sum of 147 k weights in [0, 1] has an
// ulp near 0.016 at its top: the size of the weights themselves).  One 1024-thread workgroup per frame.
//
// nsff_ray_draw: one batch of the training dataset's __getitem__ (datasets/monocular.py:233-250) on the device: pixel
// indices by inverse-CDF search (first i with cdf[i] > u * total: a zero-weight pixel is never drawn) or uniformly
// (floor(u * n)), then the record columns gathered straight into the batch tensors.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_frame_ops.h"

namespace {

constexpr int TW = 64, TH = 16, HALO = 5, PW = TW + 2 * HALO, PH = TH + 2 * HALO;
constexpr int SSIM_THREADS = 256;
constexpr int SSIM_WORDS = 2;                                     // one tile's share of a frame: three fp32 sums (and a zero)
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

// normalised 1-D Gaussian, sigma 1.5, 11 taps (computed in float64, rounded once)
__constant__ float c_gauss[11] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055428e-01f,
                                  2.660117149e-01f, 2.130055428e-01f, 1.093606874e-01f, 3.600077331e-02f, 7.598758209e-03f,
                                  1.028380124e-03f};

// kornia 0.5.4's loss form.  (Releases before it wrote clamp(1 - ssim, 0, 1) / 2; the two differ only where ssim < 0.)
__device__ __forceinline__ float ssim_loss_form(float ssim) { return fminf(fmaxf((1.0f - ssim) * 0.5f, 0.0f), 1.0f); }

// F.pad(mode='reflect') index (valid for -n < i < 2n - 1), clamped for halo rows / columns no output pixel reads
__device__ __forceinline__ int reflect_index(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(SSIM_THREADS) void ssim_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                            const uint8_t* __restrict__ mask, int H, int W,
                                                            float* __restrict__ map, float* __restrict__ mean_map,
                                                            double* __restrict__ sums, unsigned* __restrict__ counters,
                                                            frame_word* __restrict__ partials) {
    __shared__ float s_x[PH][PW], s_y[PH][PW];
    __shared__ float s_h[5][PH][TW];
    __shared__ float s_red[SSIM_THREADS / 64][3];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t f = blockIdx.z;
    const int64_t frame_px = (int64_t)H * W;
    const float* G = gt + f * frame_px * 3;
    const float* P = pred + f * frame_px * 3;
    const int ox = x0 + lane;                                   // this thread's output column, rows y0 + wave + 4 j
    const int cy = min(y0 + TH / 2, H - 1), cx = min(x0 + TW / 2, W - 1);

    float loss[4][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sx = G[((int64_t)cy * W + cx) * 3 + c], sy = P[((int64_t)cy * W + cx) * 3 + c];
        for (int i = tid; i < PH * PW; i += SSIM_THREADS) {
            const int r = i / PW, q = i - r * PW;
            const int64_t p = (int64_t)reflect_index(y0 - HALO + r, H) * W + reflect_index(x0 - HALO + q, W);
            s_x[r][q] = G[p * 3 + c] - sx;
            s_y[r][q] = P[p * 3 + c] - sy;
        }
        __syncthreads();
        for (int r = wave; r < PH; r += SSIM_THREADS / 64) {      // horizontal pass: 5 moment planes, PH rows x TW columns
            float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float g = c_gauss[k], u = s_x[r][lane + k], v = s_y[r][lane + k];
                const float gu = g * u, gv = g * v;
                a += gu; b += gv; aa += gu * u; bb += gv * v; ab += gu * v;
            }
            s_h[0][r][lane] = a; s_h[1][r][lane] = b; s_h[2][r][lane] = aa; s_h[3][r][lane] = bb; s_h[4][r][lane] = ab;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {                             // vertical pass and the SSIM formula
            const int r = wave + 4 * j;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float g = c_gauss[k];
#pragma unroll
                for (int t = 0; t < 5; ++t) m[t] += g * s_h[t][r + k][lane];
            }
            const float s11 = m[2] - m[0] * m[0], s22 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
            const float mu1 = m[0] + sx, mu2 = m[1] + sy;
            const float num = (2.f * mu1 * mu2 + C1) * (2.f * s12 + C2);
            const float den = (mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2) + 1e-12f;
            loss[j][c] = ssim_loss_form(num / den);
        }
        __syncthreads();                                          // s_x / s_y / s_h are rewritten by the next channel
    }

    float part[3] = {0.f, 0.f, 0.f};                              // loss sum, masked loss sum, masked pixel count
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = y0 + wave + 4 * j;
        if (ox >= W || oy >= H) continue;
        const int64_t p = (int64_t)oy * W + ox;
        const float s = loss[j][0] + loss[j][1] + loss[j][2];
        if (map) {
            float* o = map + (f * frame_px + p) * 3;
            o[0] = loss[j][0]; o[1] = loss[j][1]; o[2] = loss[j][2];
        }
        if (mean_map) mean_map[f * frame_px + p] = s / 3.0f;
        part[0] += s;
        if (mask && mask[f * frame_px + p]) { part[1] += s; part[2] += 1.f; }
    }
    if (!sums) return;

    // the tile's sums in fp32, the frame's from them in fp64, in tile order
#pragma unroll
    for (int t = 0; t < 3; ++t) part[t] = wave_sum(part[t]);
    if (lane == 0) { s_red[wave][0] = part[0]; s_red[wave][1] = part[1]; s_red[wave][2] = part[2]; }
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_tiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
    frame_word* fp = partials + f * n_tiles * SSIM_WORDS;
    const frame_word mine[SSIM_WORDS] = {pack2(sum4(s_red, 0), sum4(s_red, 1)), pack2(sum4(s_red, 2), 0.f)};
    if (!frame_publish(fp, counters + f, tile, n_tiles, lane, mine)) return;
    double acc[3] = {0.0, 0.0, 0.0};
    frame_fold<SSIM_WORDS>(fp, n_tiles, lane, [&](const frame_word (&w)[SSIM_WORDS]) {
        acc[0] += (double)word_lo_f(w[0]); acc[1] += (double)word_hi_f(w[0]); acc[2] += (double)word_lo_f(w[1]);
    });
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
        sums[f * 3 + 0] = acc[0]; sums[f * 3 + 1] = acc[1]; sums[f * 3 + 2] = acc[2];
        frame_counter_reset(counters + f);
    }
}

constexpr int CDF_THREADS = 1024, CDF_PER_THREAD = 4, CDF_CHUNK = CDF_THREADS * CDF_PER_THREAD;

__global__ __launch_bounds__(CDF_THREADS) void cdf_kernel(const float* __restrict__ w, int64_t n, double* __restrict__ cdf) {
    __shared__ double s_wave[CDF_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* W = w + (int64_t)blockIdx.x * n;
    double* O = cdf + (int64_t)blockIdx.x * n;
    double carry = 0.0;
    for (int64_t base = 0; base < n; base += CDF_CHUNK) {
        const int64_t i0 = base + (int64_t)tid * CDF_PER_THREAD;
        double v[CDF_PER_THREAD];
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < CDF_PER_THREAD; ++k) {
            run += i0 + k < n ? (double)W[i0 + k] : 0.0;
            v[k] = run;
        }
        double incl = run;                                        // inclusive scan of the thread totals within the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        double before = carry, total = carry;
        for (int k = 0; k < CDF_THREADS / 64; ++k) {              // (every thread adds the wave totals in the same order)
            if (k < wave) before += s_wave[k];
            total += s_wave[k];
        }
        before += incl - run;
#pragma unroll
        for (int k = 0; k < CDF_PER_THREAD; ++k)
            if (i0 + k < n) O[i0 + k] = before + v[k];
        carry = total;
        __syncthreads();                                          // s_wave is rewritten by the next chunk
    }
}

constexpr int DRAW_THREADS = 256, DRAW_TABLE = 4096;

__global__ __launch_bounds__(DRAW_THREADS) void ray_draw_kernel(NsffRayDrawArgs a) {
    __shared__ double s_tab[DRAW_TABLE];                          // cdf at the end of each segment of `seg` pixels
    const int64_t n = a.n_pixels;
    const double* C = a.cdf ? a.cdf + a.frame * n : nullptr;
    const double total = C ? C[n - 1] : 0.0;
    const bool weighted = C && total > 0.0 && isfinite(total);    // (a zero / non-finite frame draws uniformly)
    const int64_t seg = (n + DRAW_TABLE - 1) / DRAW_TABLE;
    const int n_seg = (int)((n + seg - 1) / seg);
    if (weighted) {
        for (int k = threadIdx.x; k < n_seg; k += DRAW_THREADS) s_tab[k] = C[min((int64_t)(k + 1) * seg, n) - 1];
        __syncthreads();
    }
    const int64_t b = (int64_t)blockIdx.x * DRAW_THREADS + threadIdx.x;
    if (b >= a.batch) return;
    const float u = a.u[b];
    int64_t idx;
    if (weighted) {
        const double target = (double)u * total;                  // < total for u < 1
        int lo = 0, hi = n_seg - 1;                               // first segment whose end value exceeds target
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_tab[mid] > target) hi = mid; else lo = mid + 1; }
        int64_t l = (int64_t)lo * seg, h = min((int64_t)(lo + 1) * seg, n) - 1;
        while (l < h) { const int64_t mid = (l + h) >> 1; if (C[mid] > target) h = mid; else l = mid + 1; }
        idx = l;
    } else {
        idx = min((int64_t)((double)u * (double)n), n - 1);
    }
    const float4* rec = reinterpret_cast<const float4*>(a.records + (a.frame * n + idx) * NSFF_RAY_RECORD);
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    // columns: rays_o 0-2, rays_d 3-5, rgb 6-8, t 9, disp 10, mask 11, uv_fw 12-13, uv_bw 14-15 (monocular.py:180-183)
    float* ry = a.rays + b * 6;
    ry[0] = r0.x; ry[1] = r0.y; ry[2] = r0.z; ry[3] = r0.w; ry[4] = r1.x; ry[5] = r1.y;
    float* rg = a.rgbs + b * 3;
    rg[0] = r1.z; rg[1] = r1.w; rg[2] = r2.x;
    a.ts[b] = (int64_t)r2.y;                                      // rays[:, 9].long()
    if (a.cam_ids) a.cam_ids[b] = 0;
    a.disps[b] = r2.z;
    a.rays_mask[b] = r2.w;
    a.uv_fw[b * 2] = r3.x; a.uv_fw[b * 2 + 1] = r3.y;
    a.uv_bw[b * 2] = r3.z; a.uv_bw[b * 2 + 1] = r3.w;
    if (a.rand_idx) a.rand_idx[b] = idx;
}

inline int64_t host_tiles(int32_t H, int32_t W) { return (int64_t)((W + TW - 1) / TW) * ((H + TH - 1) / TH); }

}  // namespace

extern "C" int64_t nsff_ssim_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (n_frames < 1 || H < 6 || W < 6) return 0;
    return frame_scratch_bytes(n_frames, host_tiles(H, W), SSIM_WORDS);
}

extern "C" int nsff_ssim(const NsffSsimArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (a->window != 11) return NSFF_ERR_INVALID;
    if (a->n_frames < 1 || a->n_frames > 65535 || a->H < 6 || a->W < 6) return NSFF_ERR_INVALID;
    if (!a->gt || !a->pred) return NSFF_ERR_NULL;
    if (!a->map && !a->mean_map && !a->sums) return NSFF_ERR_INVALID;           // nothing to compute
    if (a->sums && !a->scratch) return NSFF_ERR_NULL;
    if (a->sums && a->scratch_bytes < nsff_ssim_scratch_bytes(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    const FrameScratch s = frame_scratch_split(a->scratch, a->n_frames);
    const dim3 grid((a->W + TW - 1) / TW, (a->H + TH - 1) / TH, a->n_frames);
    hipLaunchKernelGGL(ssim_kernel, grid, dim3(SSIM_THREADS), 0, (hipStream_t)stream, a->gt, a->pred, a->mask, a->H, a->W,
                       a->map, a->mean_map, a->sums, s.counters, s.partials);
    return nsff_launch_status();
}

extern "C" int nsff_cdf(const float* weights, int64_t n_frames, int64_t n, double* cdf, void* stream) {
    if (n_frames < 0 || n < 0 || n_frames > 0x7fffffff) return NSFF_ERR_INVALID;
    if (n_frames == 0 || n == 0) return NSFF_OK;
    if (!weights || !cdf) return NSFF_ERR_NULL;
    hipLaunchKernelGGL(cdf_kernel, dim3((unsigned)n_frames), dim3(CDF_THREADS), 0, (hipStream_t)stream, weights, n, cdf);
    return nsff_launch_status();
}

extern "C" int nsff_ray_draw(const NsffRayDrawArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (a->n_frames < 1 || a->n_pixels < 1 || a->batch < 0 || a->frame < 0 || a->frame >= a->n_frames) return NSFF_ERR_INVALID;
    if (a->batch == 0) return NSFF_OK;
    if (!a->records || !a->u || !a->rays || !a->rgbs || !a->ts || !a->disps || !a->rays_mask || !a->uv_fw || !a->uv_bw)
        return NSFF_ERR_NULL;
    if ((uintptr_t)a->records & 15) return NSFF_ERR_ALIGN;
    const int64_t blocks = (a->batch + DRAW_THREADS - 1) / DRAW_THREADS;
    if (blocks > 0x7fffffff) return NSFF_ERR_INVALID;
    hipLaunchKernelGGL(ray_draw_kernel, dim3((unsigned)blocks), dim3(DRAW_THREADS), 0, (hipStream_t)stream, *a);
    return nsff_launch_status();
}
