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
// atomics; bit-reproducible).
//
// nsff_cdf: per-frame inclusive scan of the sampling weights in fp64 (an fp32 running sum of 147 k weights in [0, 1] has an
// ulp near 0.016 at its top: the size of the weights themselves).  One 1024-thread workgroup per frame.
//
// nsff_ray_draw: one batch of the training dataset's __getitem__ (datasets/monocular.py:233-250) on the device: pixel
// indices by inverse-CDF search (first i with cdf[i] > u * total: a zero-weight pixel is never drawn) or uniformly
// (floor(u * n)), then the record columns gathered straight into the batch tensors.
//
// nsff_frame_finish: the per-frame finishing work of the reference's eval.py on F rendered frames -- clip(rgb, 0, 1), the 8-bit
// image (255 * clip) truncated (eval.py:183-184, 213-214, 222-223), the squared-error sums of metrics.psnr over the whole frame
// and over the valid pixels (metrics.py:6-16), and the normalised 8-bit depth of utils/visualization.py:10-15 with its colour
// table lookup.  Two launches: frame_image_kernel streams the image once (and reduces the sums and the depth range),
// frame_depth_kernel quantises the depth with the range the first one wrote.  A workgroup owns 1024 consecutive pixels OF ONE
// FRAME (grid.y = frame) and a lane four consecutive ones, so which values a lane, a wave and a workgroup add depends on H * W
// alone: a frame's sums are the same bits at any position of any batch.  Per-workgroup partials go to scratch and the frame's
// last-arriving workgroup adds them in a fixed order, as ssim_kernel does.  A lane moves its four pixels as 16-byte loads and
// dword stores where its first pixel's FLAT index (frame * H * W + pixel) is a multiple of four -- then every address is
// aligned (48, 16, 12 and 4 bytes per four pixels) -- and element by element otherwise (frames whose base is not a multiple of
// four pixels, i.e. odd H * W, and each frame's last partial quad).
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"

namespace {

constexpr int TW = 64, TH = 16, HALO = 5, PW = TW + 2 * HALO, PH = TH + 2 * HALO;
constexpr int SSIM_THREADS = 256;
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
                                                            float* __restrict__ partials) {
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

    // workgroup sum in a fixed order: butterfly within each wave, then the four waves in order
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part[t] += __shfl_xor(part[t], o);
    if (lane == 0) { s_red[wave][0] = part[0]; s_red[wave][1] = part[1]; s_red[wave][2] = part[2]; }
    __syncthreads();
    if (wave != 0) return;
    const int64_t n_tiles = (int64_t)gridDim.x * gridDim.y, tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    float* my = partials + (f * n_tiles + tile) * 3;
    unsigned ticket = 0;
    if (lane == 0) {
        for (int t = 0; t < 3; ++t) my[t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
        // publish the partial, then take a ticket: agent-scope release / acquire (the frame's tiles may run on any XCD)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(counters + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ticket = __shfl(ticket, 0);
    if (ticket != (unsigned)(n_tiles - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const float* fp = partials + f * n_tiles * 3;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t t = lane; t < n_tiles; t += 64)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += (double)fp[t * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    if (lane == 0) {
        sums[f * 3 + 0] = acc[0]; sums[f * 3 + 1] = acc[1]; sums[f * 3 + 2] = acc[2];
        __hip_atomic_store(counters + f, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
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

constexpr int FIN_THREADS = 256, FIN_PX = 4, FIN_BLOCK_PX = FIN_THREADS * FIN_PX;

struct FinPartial { double s[3]; float mn, mx; };                 // one workgroup's share of a frame: four 8-byte words

// np.nan_to_num of an fp32 value: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float nan_to_num(float x) { return x != x ? 0.f : fminf(fmaxf(x, -FLT_MAX), FLT_MAX); }
// torch.clip(x, 0, 1): a NaN stays a NaN
__device__ __forceinline__ float clip01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }
// astype(np.uint8) of a value in [0, 255]: truncation toward zero; a NaN (numpy: undefined) gives 0
__device__ __forceinline__ uint32_t trunc_u8(float v) { return v == v ? (uint32_t)(int)fminf(fmaxf(v, 0.f), 255.f) : 0u; }

template <int NB>
__device__ __forceinline__ void store_bytes(uint8_t* dst, const uint32_t (&q)[NB], int n_bytes, bool vec) {
    if (vec) {                                                    // all NB bytes, dst 4-byte aligned
        uint32_t* o = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int w = 0; w < NB / 4; ++w) o[w] = q[4 * w] | (q[4 * w + 1] << 8) | (q[4 * w + 2] << 16) | (q[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (i < n_bytes) dst[i] = (uint8_t)q[i];
    }
}

__global__ __launch_bounds__(FIN_THREADS) void frame_image_kernel(NsffFrameFinishArgs a, int aligned,
                                                                  unsigned* __restrict__ counters,
                                                                  FinPartial* __restrict__ partials) {
    __shared__ double s_sum[FIN_THREADS / 64][3];
    __shared__ float s_mm[FIN_THREADS / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W, base = f * HW;
    const int64_t p0 = ((int64_t)blockIdx.x * FIN_THREADS + tid) * FIN_PX;      // first pixel of this lane, in its frame
    const int n = (int)min((int64_t)FIN_PX, max(HW - p0, (int64_t)0));          // its pixels: 4, a ragged 1..3, or none
    const bool vec = aligned && n == FIN_PX && ((base + p0) & 3) == 0;
    const int64_t q0 = base + p0;                                               // flat pixel index

    float r[3 * FIN_PX], g[3 * FIN_PX], d[FIN_PX];
    uint32_t v[FIN_PX];
#pragma unroll
    for (int i = 0; i < 3 * FIN_PX; ++i) { r[i] = 0.f; g[i] = 0.f; }
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) { d[k] = 0.f; v[k] = 0u; }
    if (vec) {
        const float4* R = reinterpret_cast<const float4*>(a.rgb + q0 * 3);
#pragma unroll
        for (int w = 0; w < 3; ++w) { const float4 t = R[w]; r[4 * w] = t.x; r[4 * w + 1] = t.y; r[4 * w + 2] = t.z; r[4 * w + 3] = t.w; }
        if (a.gt) {
            const float4* G = reinterpret_cast<const float4*>(a.gt + q0 * 3);
#pragma unroll
            for (int w = 0; w < 3; ++w) { const float4 t = G[w]; g[4 * w] = t.x; g[4 * w + 1] = t.y; g[4 * w + 2] = t.z; g[4 * w + 3] = t.w; }
        }
        if (a.valid) {
            const uint32_t t = *reinterpret_cast<const uint32_t*>(a.valid + q0);
            v[0] = t & 255u; v[1] = (t >> 8) & 255u; v[2] = (t >> 16) & 255u; v[3] = t >> 24;
        }
        if (a.depth) { const float4 t = *reinterpret_cast<const float4*>(a.depth + q0); d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w; }
    } else {
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) {
            if (k >= n) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                r[3 * k + c] = a.rgb[(q0 + k) * 3 + c];
                if (a.gt) g[3 * k + c] = a.gt[(q0 + k) * 3 + c];
            }
            if (a.valid) v[k] = a.valid[q0 + k];
            if (a.depth) d[k] = a.depth[q0 + k];
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
        if (a.rgb_clipped) {
            float* o = a.rgb_clipped + q0 * 3;
            if (vec) {
                float4* O = reinterpret_cast<float4*>(o);
#pragma unroll
                for (int w = 0; w < 3; ++w) O[w] = make_float4(r[4 * w], r[4 * w + 1], r[4 * w + 2], r[4 * w + 3]);
            } else {
#pragma unroll
                for (int i = 0; i < 3 * FIN_PX; ++i)
                    if (i < 3 * n) o[i] = r[i];
            }
        }
        if (a.rgb_u8) store_bytes(a.rgb_u8 + q0 * 3, q, 3 * n, vec);
    }
    if (!a.sums && !a.depth_range) return;

    // workgroup reduction in a fixed order: butterfly within each wave, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] += __shfl_xor(acc[t], o);
        mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if (lane == 0) { s_sum[wave][0] = acc[0]; s_sum[wave][1] = acc[1]; s_sum[wave][2] = acc[2]; s_mm[wave][0] = mn; s_mm[wave][1] = mx; }
    __syncthreads();
    if (wave != 0) return;
    const int64_t n_blocks = gridDim.x;
    FinPartial* fp = partials + f * n_blocks;
    unsigned ticket = 0;
    if (lane == 0) {
        FinPartial mine;
        for (int t = 0; t < 3; ++t) mine.s[t] = ((s_sum[0][t] + s_sum[1][t]) + s_sum[2][t]) + s_sum[3][t];
        mine.mn = fminf(fminf(s_mm[0][0], s_mm[1][0]), fminf(s_mm[2][0], s_mm[3][0]));
        mine.mx = fmaxf(fmaxf(s_mm[0][1], s_mm[1][1]), fmaxf(s_mm[2][1], s_mm[3][1]));
        // publish the partial, then take a ticket (the frame's workgroups may run on any XCD).  The four 8-byte words go out as
        // agent-scope atomic stores -- write-through, so no release fence: a fence per workgroup writes back every dirty line of
        // its L2, the image being stored included, and 14 400 of them took 0.9 of the 1.0 ms a 100-frame call then cost
        unsigned long long* slot = reinterpret_cast<unsigned long long*>(fp + blockIdx.x);
        for (int t = 0; t < 3; ++t) __hip_atomic_store(slot + t, (unsigned long long)__double_as_longlong(mine.s[t]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(slot + 3, (unsigned long long)__float_as_uint(mine.mn) | ((unsigned long long)__float_as_uint(mine.mx) << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(counters + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ticket = __shfl(ticket, 0);
    if (ticket != (unsigned)(n_blocks - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    double tot[3] = {0.0, 0.0, 0.0};
    mn = INFINITY; mx = -INFINITY;
    for (int64_t t = lane; t < n_blocks; t += 64) {               // lane l adds blocks l, l + 64, ... in order
        const volatile FinPartial* p = fp + t;
#pragma unroll
        for (int k = 0; k < 3; ++k) tot[k] += p->s[k];
        mn = fminf(mn, p->mn); mx = fmaxf(mx, p->mx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tot[k] += __shfl_xor(tot[k], o);
        mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if (lane == 0) {
        if (a.sums) { a.sums[f * 3 + 0] = tot[0]; a.sums[f * 3 + 1] = tot[1]; a.sums[f * 3 + 2] = tot[2]; }
        if (a.depth_range) { a.depth_range[f * 2 + 0] = mn; a.depth_range[f * 2 + 1] = mx; }
        __hip_atomic_store(counters + f, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
}

// visualize_depth (utils/visualization.py:10-15) with the frame's own range: every step one fp32 operation, as numpy rounds it
__global__ __launch_bounds__(FIN_THREADS) void frame_depth_kernel(NsffFrameFinishArgs a, int aligned) {
    __shared__ uint8_t s_lut[768];
    const int tid = threadIdx.x;
    if (a.depth_rgb_u8) {
        for (int i = tid; i < 768; i += FIN_THREADS) s_lut[i] = a.lut[i];
        __syncthreads();
    }
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W;
    const int64_t p0 = ((int64_t)blockIdx.x * FIN_THREADS + tid) * FIN_PX;
    const int n = (int)min((int64_t)FIN_PX, max(HW - p0, (int64_t)0));
    if (n == 0) return;
    const int64_t q0 = f * HW + p0;
    const bool vec = aligned && n == FIN_PX && (q0 & 3) == 0;
    const float mi = a.depth_range[f * 2], ma = a.depth_range[f * 2 + 1];
    const float span = (ma - mi) + 1e-8f;
    float d[FIN_PX] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        const float4 t = *reinterpret_cast<const float4*>(a.depth + q0);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k)
            if (k < n) d[k] = a.depth[q0 + k];
    }
    uint32_t idx[FIN_PX], col[3 * FIN_PX];
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) {
        const float x = (nan_to_num(d[k]) - mi) / span;            // IEEE division
        idx[k] = trunc_u8(255.f * x);
    }
    if (a.depth_u8) store_bytes(a.depth_u8 + q0, idx, n, vec);
    if (a.depth_rgb_u8) {
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) col[3 * k + c] = s_lut[idx[k] * 3 + c];
        store_bytes(a.depth_rgb_u8 + q0 * 3, col, 3 * n, vec);
    }
}

// ---- nsff_val_panels: the image panels of train.py:209-235, 254-257 (see the header).  The pixel decomposition is
// frame_image_kernel's: a workgroup owns 1024 consecutive pixels of one frame, a lane four consecutive ones. ----
constexpr int PAN_FIELDS = 5;                                     // depth, static depth, -disp, -rmse, -ssim
constexpr int PAN_PAD_THREADS = FIN_THREADS;                      // one padding pixel of the grid per thread

struct PanPartial { unsigned long long mm[PAN_FIELDS]; };         // one workgroup's share of a frame: min | max << 32 per field

// four pixels of C channels each: 16-byte loads on the aligned path, element by element otherwise; a NULL array reads as 0
template <int C>
__device__ __forceinline__ void load_px(const float* __restrict__ src, int64_t q0, int n, bool vec, float (&v)[C * FIN_PX]) {
#pragma unroll
    for (int i = 0; i < C * FIN_PX; ++i) v[i] = 0.f;
    if (!src) return;
    if (vec) {
        const float4* S = reinterpret_cast<const float4*>(src + q0 * C);
#pragma unroll
        for (int w = 0; w < C; ++w) { const float4 t = S[w]; v[4 * w] = t.x; v[4 * w + 1] = t.y; v[4 * w + 2] = t.z; v[4 * w + 3] = t.w; }
    } else {
#pragma unroll
        for (int i = 0; i < C * FIN_PX; ++i)
            if (i < C * n) v[i] = src[q0 * C + i];
    }
}

// The five scalar fields of a lane's four pixels after nan_to_num, each a chain of single fp32 operations; pc = clip(pred, 0, 1)
// and g = gt are handed on to the composer.
__device__ __forceinline__ void pan_fields(const NsffValPanelsArgs& a, int64_t q0, int n, bool vec, float (&x)[PAN_FIELDS][FIN_PX],
                                           float (&pc)[3 * FIN_PX], float (&g)[3 * FIN_PX]) {
    float d[FIN_PX], sd[FIN_PX], di[FIN_PX], l[3 * FIN_PX];
    load_px<3>(a.gt, q0, n, vec, g);
    load_px<3>(a.pred, q0, n, vec, pc);
    load_px<1>(a.depth, q0, n, vec, d);
    load_px<1>(a.static_depth, q0, n, vec, sd);
    load_px<1>(a.disp, q0, n, vec, di);
    load_px<3>(a.ssim_loss, q0, n, vec, l);
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
                                                                  PanPartial* __restrict__ partials) {
    __shared__ float s_mm[FIN_THREADS / 64][PAN_FIELDS][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W, base = f * HW;
    const int64_t p0 = ((int64_t)blockIdx.x * FIN_THREADS + tid) * FIN_PX;
    const int n = (int)min((int64_t)FIN_PX, max(HW - p0, (int64_t)0));
    const int64_t q0 = base + p0;
    const bool vec = aligned && n == FIN_PX && (q0 & 3) == 0;

    float x[PAN_FIELDS][FIN_PX], pc[3 * FIN_PX], g[3 * FIN_PX];
    pan_fields(a, q0, n, vec, x, pc, g);
    float mn[PAN_FIELDS], mx[PAN_FIELDS];
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t) {
        mn[t] = INFINITY; mx[t] = -INFINITY;
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k)
            if (k < n) { mn[t] = fminf(mn[t], x[t][k]); mx[t] = fmaxf(mx[t], x[t][k]); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[t] = fminf(mn[t], __shfl_xor(mn[t], o)); mx[t] = fmaxf(mx[t], __shfl_xor(mx[t], o)); }
        if (lane == 0) { s_mm[wave][t][0] = mn[t]; s_mm[wave][t][1] = mx[t]; }
    }
    __syncthreads();
    if (wave != 0) return;
    const int64_t n_blocks = gridDim.x;
    PanPartial* fp = partials + f * n_blocks;
    unsigned ticket = 0;
    if (lane == 0) {
        // publish the partial as agent-scope atomic stores (write-through: no release fence, see frame_image_kernel), then a ticket
        unsigned long long* slot = reinterpret_cast<unsigned long long*>(fp + blockIdx.x);
        for (int t = 0; t < PAN_FIELDS; ++t) {
            const float lo = fminf(fminf(s_mm[0][t][0], s_mm[1][t][0]), fminf(s_mm[2][t][0], s_mm[3][t][0]));
            const float hi = fmaxf(fmaxf(s_mm[0][t][1], s_mm[1][t][1]), fmaxf(s_mm[2][t][1], s_mm[3][t][1]));
            __hip_atomic_store(slot + t, (unsigned long long)__float_as_uint(lo) | ((unsigned long long)__float_as_uint(hi) << 32),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(counters + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ticket = __shfl(ticket, 0);
    if (ticket != (unsigned)(n_blocks - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t) { mn[t] = INFINITY; mx[t] = -INFINITY; }
    for (int64_t b = lane; b < n_blocks; b += 64) {
        const volatile PanPartial* p = fp + b;
#pragma unroll
        for (int t = 0; t < PAN_FIELDS; ++t) {
            const unsigned long long w = p->mm[t];
            mn[t] = fminf(mn[t], __uint_as_float((unsigned)w)); mx[t] = fmaxf(mx[t], __uint_as_float((unsigned)(w >> 32)));
        }
    }
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[t] = fminf(mn[t], __shfl_xor(mn[t], o)); mx[t] = fmaxf(mx[t], __shfl_xor(mx[t], o)); }
    if (lane == 0) {
        const bool have[PAN_FIELDS] = {a.depth != nullptr, a.static_depth != nullptr, a.disp != nullptr, a.gt != nullptr,
                                       a.ssim_loss != nullptr};
        for (int t = 0; t < PAN_FIELDS; ++t)
            if (have[t]) { a.ranges[(f * PAN_FIELDS + t) * 2] = mn[t]; a.ranges[(f * PAN_FIELDS + t) * 2 + 1] = mx[t]; }
        __hip_atomic_store(counters + f, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
}

// Four pixels (px[k] = r | g << 8 | b << 16) of the tile in cell `slot` of the grid of one frame (G = its first byte).  A lane
// whose four pixels lie in one image row owns 12 consecutive bytes at any byte offset (3-byte pixels, odd row lengths): the
// bytes up to the next dword boundary go out one by one, the rest as dwords shifted into place.
__device__ __forceinline__ void grid_store(uint8_t* __restrict__ G, int slot, int H, int W, int GW, int64_t p0, int n,
                                           const uint32_t (&px)[FIN_PX]) {
    const int gy0 = (slot / 3) * (H + 2) + 2, gx0 = (slot % 3) * (W + 2) + 2;
    const int y = (int)(p0 / W), x = (int)(p0 - (int64_t)y * W);
    if (n == FIN_PX && x + FIN_PX <= W) {
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
            if (k >= n) continue;
            const int64_t p = p0 + k;
            const int yy = (int)(p / W), xx = (int)(p - (int64_t)yy * W);
            uint8_t* dst = G + ((int64_t)(gy0 + yy) * GW + gx0 + xx) * 3;
            dst[0] = (uint8_t)px[k]; dst[1] = (uint8_t)(px[k] >> 8); dst[2] = (uint8_t)(px[k] >> 16);
        }
    }
}

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
    const int64_t HW = (int64_t)H * W;
    const int64_t p0 = ((int64_t)blockIdx.x * FIN_THREADS + tid) * FIN_PX;
    const int n = (int)min((int64_t)FIN_PX, max(HW - p0, (int64_t)0));
    if (n == 0) return;
    const int64_t q0 = f * HW + p0;
    const bool vec = aligned && n == FIN_PX && (q0 & 3) == 0;

    float x[PAN_FIELDS][FIN_PX], pc[3 * FIN_PX], g[3 * FIN_PX];
    pan_fields(a, q0, n, vec, x, pc, g);
    const bool have[PAN_FIELDS] = {a.depth != nullptr, a.static_depth != nullptr, a.disp != nullptr, a.gt != nullptr,
                                   a.ssim_loss != nullptr};
    uint32_t idx[PAN_FIELDS][FIN_PX], col[PAN_FIELDS][FIN_PX];   // visualize_depth's index and its colour, packed
#pragma unroll
    for (int t = 0; t < PAN_FIELDS; ++t) {
        const float mi = have[t] ? a.ranges[(f * PAN_FIELDS + t) * 2] : 0.f, ma = have[t] ? a.ranges[(f * PAN_FIELDS + t) * 2 + 1] : 0.f;
        const float span = (ma - mi) + 1e-8f;
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) {
            const uint32_t i = trunc_u8(255.f * ((x[t][k] - mi) / span));               // IEEE division
            idx[t][k] = i;
            col[t][k] = s_lut[0][3 * i] | (s_lut[0][3 * i + 1] << 8) | (s_lut[0][3 * i + 2] << 16);
        }
    }
    uint32_t pu[3 * FIN_PX];                                      // rgb_u8 of the clipped prediction
#pragma unroll
    for (int i = 0; i < 3 * FIN_PX; ++i) pu[i] = trunc_u8(255.f * pc[i]);

    if (a.rmse_u8) store_bytes(a.rmse_u8 + q0, idx[3], n, vec);
    if (a.ssim_u8) store_bytes(a.ssim_u8 + q0, idx[4], n, vec);
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
        store_bytes(out + q0 * 3, q, 3 * n, vec);
    }
    if (!G) return;

    uint32_t px[FIN_PX];
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) px[k] = trunc_u8(255.f * g[3 * k]) | (trunc_u8(255.f * g[3 * k + 1]) << 8) | (trunc_u8(255.f * g[3 * k + 2]) << 16);
    grid_store(G, 0, H, W, GW, p0, n, px);
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) px[k] = pu[3 * k] | (pu[3 * k + 1] << 8) | (pu[3 * k + 2] << 16);
    grid_store(G, 1, H, W, GW, p0, n, px);
    grid_store(G, 2, H, W, GW, p0, n, col[0]);
    if (transient) {
        float ta[FIN_PX], sr[3 * FIN_PX];
        load_px<1>(a.transient_alpha, q0, n, vec, ta);
        load_px<3>(a.static_rgb, q0, n, vec, sr);
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) {                        // visualize_mask(transient_alpha)
            const uint32_t i = trunc_u8(255.f * ta[k]);
            px[k] = s_lut[1][3 * i] | (s_lut[1][3 * i + 1] << 8) | (s_lut[1][3 * i + 2] << 16);
        }
        grid_store(G, 3, H, W, GW, p0, n, px);
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k)
            px[k] = trunc_u8(255.f * clip01(sr[3 * k])) | (trunc_u8(255.f * clip01(sr[3 * k + 1])) << 8) | (trunc_u8(255.f * clip01(sr[3 * k + 2])) << 16);
        grid_store(G, 4, H, W, GW, p0, n, px);
        grid_store(G, 5, H, W, GW, p0, n, col[1]);
    }
    if (a.mask) {
        float mk[FIN_PX];
        load_px<1>(a.mask, q0, n, vec, mk);
#pragma unroll
        for (int k = 0; k < FIN_PX; ++k) {                        // visualize_mask(1 - mask)
            const uint32_t i = trunc_u8(255.f * (1.0f - mk[k]));
            px[k] = s_lut[1][3 * i] | (s_lut[1][3 * i + 1] << 8) | (s_lut[1][3 * i + 2] << 16);
        }
        grid_store(G, slot_mask, H, W, GW, p0, n, px);
    }
    if (a.disp) grid_store(G, slot_disp, H, W, GW, p0, n, col[2]);
#pragma unroll
    for (int k = 0; k < FIN_PX; ++k) px[k] = 0u;
    for (int s = n_tiles; s < 3 * ymaps; ++s) grid_store(G, s, H, W, GW, p0, n, px);   // unfilled cells of the last row
}

inline int64_t fin_blocks(int64_t n_pixels) { return (n_pixels + FIN_BLOCK_PX - 1) / FIN_BLOCK_PX; }

inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }
inline int64_t host_tiles(int32_t H, int32_t W) { return (int64_t)((W + TW - 1) / TW) * ((H + TH - 1) / TH); }

}  // namespace

extern "C" int64_t nsff_ssim_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (n_frames < 1 || H < 6 || W < 6) return 0;
    return align16(4 * (int64_t)n_frames) + 12 * (int64_t)n_frames * host_tiles(H, W);
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
    unsigned* counters = reinterpret_cast<unsigned*>(a->scratch);
    float* partials = a->scratch ? reinterpret_cast<float*>(reinterpret_cast<char*>(a->scratch) + align16(4 * (int64_t)a->n_frames))
                                 : nullptr;
    const dim3 grid((a->W + TW - 1) / TW, (a->H + TH - 1) / TH, a->n_frames);
    hipLaunchKernelGGL(ssim_kernel, grid, dim3(SSIM_THREADS), 0, (hipStream_t)stream, a->gt, a->pred, a->mask, a->H, a->W,
                       a->map, a->mean_map, a->sums, counters, partials);
    return nsff_launch_status();
}

extern "C" int64_t nsff_frame_finish_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (n_frames < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff) return 0;
    return align16(4 * (int64_t)n_frames) + (int64_t)sizeof(FinPartial) * n_frames * fin_blocks((int64_t)H * W);
}

extern "C" int nsff_frame_finish(const NsffFrameFinishArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!a->rgb) return NSFF_ERR_INVALID;                                        // no image: nothing to finish
    if (a->n_frames < 1 || a->n_frames > 65535 || a->H < 1 || a->W < 1 || (int64_t)a->H * a->W > 0x7fffffff) return NSFF_ERR_INVALID;
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
    unsigned* counters = reinterpret_cast<unsigned*>(a->scratch);
    FinPartial* partials = a->scratch ? reinterpret_cast<FinPartial*>(reinterpret_cast<char*>(a->scratch) + align16(4 * (int64_t)a->n_frames))
                                      : nullptr;
    const dim3 grid((unsigned)fin_blocks((int64_t)a->H * a->W), a->n_frames);
    hipLaunchKernelGGL(frame_image_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned, counters, partials);
    if (depth_out) hipLaunchKernelGGL(frame_depth_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned);
    return nsff_launch_status();
}

extern "C" int64_t nsff_val_panels_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (n_frames < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff) return 0;
    return align16(4 * (int64_t)n_frames) + (int64_t)sizeof(PanPartial) * n_frames * fin_blocks((int64_t)H * W);
}

extern "C" int nsff_val_panels(const NsffValPanelsArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!a->pred) return NSFF_ERR_INVALID;                                       // no prediction: no panel
    if (a->n_frames < 1 || a->n_frames > 65535 || a->H < 1 || a->W < 1 || (int64_t)a->H * a->W > 0x7fffffff) return NSFF_ERR_INVALID;
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
    unsigned* counters = reinterpret_cast<unsigned*>(a->scratch);
    PanPartial* partials = reinterpret_cast<PanPartial*>(reinterpret_cast<char*>(a->scratch) + align16(4 * (int64_t)a->n_frames));
    const int64_t nb = fin_blocks((int64_t)a->H * a->W);
    hipLaunchKernelGGL(panel_range_kernel, dim3((unsigned)nb, a->n_frames), dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, aligned,
                       counters, partials);
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
