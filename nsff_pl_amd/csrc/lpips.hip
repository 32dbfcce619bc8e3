// LPIPS 0.1 (net='alex', lpips=True, spatial=True, eval mode): the reference's third score (metrics.py:36-49, eval.py:176-178,
// 235-255) on F frame pairs that are already on the device.  Restated from the public LPIPS graph:
//   x = 2 x - 1 (normalize)         ->  (x - shift) / scale per channel
//   AlexNet features, five taps:  conv 3->64 k11 s4 p2 + ReLU = f1;  maxpool 3 s2, conv 64->192 k5 p2 + ReLU = f2;
//                                 maxpool 3 s2, conv 192->384 k3 p1 + ReLU = f3;  conv 384->256 k3 p1 + ReLU = f4;
//                                 conv 256->256 k3 p1 + ReLU = f5
//   per tap:  n = f / (sqrt(sum_c f^2) + 1e-10);  m_l = sum_c w_l[c] (n0 - n1)^2;  bilinear upsample (align_corners=False) to
//   (H, W);  result = sum_l.
// The weights come from the caller (nsff_lpips_pack): nothing here knows the trained values.
//
// Launches, whatever F is: the F pairs are one batch of 2F images (gt 0 .. F-1, pred F .. 2F-1), grid.z = image.
//   conv_kernel<L> x 5   implicit GEMM on v_mfma_f32_32x32x2_f32, fp32 operands and accumulation.  D[cout][pixel]: A = weights,
//                        packed once as [cout tile of 64][k][64] (what a workgroup streams, k = (ky, kx, c) with c fastest); B = the
//                        activation gather, channels-last, so the 32 k of a step are 32 consecutive channels of ONE tap.
//                        conv1's step is one kernel row instead: its 33 (kx, c) are 33 consecutive floats of the image, padded
//                        to 36 with zero weights (K = 363 -> 396), with the normalize / scaling step applied at the load.  64 x 64 tile per workgroup,
//                        2 x 2 waves of 32 x 32, four accumulators per wave over interleaved k pairs (shorter running sums),
//                        bias + ReLU at the store.  A tile never spans two images, so a frame's features do not depend on F.
//                        Every gather is predicated: padding taps and pixels beyond the image read nothing.
//   pool_kernel x 2      maxpool 3 s2 (floor), channels-last, four channels per thread.
//   dist_kernel          all five taps in one launch, one wave per feature pixel: both norms, then the weighted squared
//                        difference of the normalised channels (identical features give exactly 0).
//   final_kernel         per output pixel the five bilinear samples and their sum; the map (F, H, W) and, by the ticketed
//                        fixed-order reduction of nsff_frame_ops.h, per frame [sum, sum over valid, valid count] in fp64.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_frame_ops.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvShape { int cin, cout, ks, stride, pad; };
constexpr ConvShape CONV[5] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};
constexpr int BM = 64, BN = 64, BK = 32, CONV_THREADS = 256;
// conv1's k step is one kernel ROW: its 11 taps x 3 channels are 33 consecutive floats of the image, padded to ROW0 with zero weights
constexpr int ROW0 = 36;
constexpr int conv_k(int l) { return CONV[l].ks * CONV[l].ks * CONV[l].cin; }
constexpr int conv_bk(int l) { return l == 0 ? ROW0 : BK; }
constexpr int conv_kpad(int l) { return l == 0 ? CONV[0].ks * ROW0 : conv_k(l); }
constexpr int LPIPS_MIN = NSFF_LPIPS_MIN_SIZE, LPIPS_WORDS = 3, LPIPS_MAX_FRAMES = 32767;      // grid.z = 2 F

// ---- layouts ----
// packed weights (floats): per layer [A tiles cout/64 x kpad x 64][bias cout][lin cout]; k = (ky, kx, c) with c fastest -- conv1:
// k = ky ROW0 + (kx, c), the last ROW0 - 33 rows of each ky zero
struct PackLayout { int64_t w[5], b[5], lin[5], total; };
inline PackLayout pack_layout() {
    PackLayout p{};
    int64_t o = 0;
    for (int l = 0; l < 5; ++l) {
        p.w[l] = o; o += (int64_t)CONV[l].cout * conv_kpad(l);
        p.b[l] = o; o += CONV[l].cout;
        p.lin[l] = o; o += CONV[l].cout;
    }
    p.total = o;
    return p;
}

// feature-map sizes: h[l] x w[l] of tap l, ph[i] x pw[i] of the two pooled maps
struct Dims { int h[5], w[5], ph[2], pw[2]; };
inline int conv_out(int n, const ConvShape& c) { return (n + 2 * c.pad - c.ks) / c.stride + 1; }
inline int pool_out(int n) { return (n - 3) / 2 + 1; }
inline bool lpips_dims(int H, int W, Dims& d) {
    if (H < LPIPS_MIN || W < LPIPS_MIN) return false;
    d.h[0] = conv_out(H, CONV[0]); d.w[0] = conv_out(W, CONV[0]);
    d.ph[0] = pool_out(d.h[0]); d.pw[0] = pool_out(d.w[0]);
    d.h[1] = conv_out(d.ph[0], CONV[1]); d.w[1] = conv_out(d.pw[0], CONV[1]);
    d.ph[1] = pool_out(d.h[1]); d.pw[1] = pool_out(d.w[1]);
    d.h[2] = conv_out(d.ph[1], CONV[2]); d.w[2] = conv_out(d.pw[1], CONV[2]);
    for (int l = 3; l < 5; ++l) { d.h[l] = conv_out(d.h[l - 1], CONV[l]); d.w[l] = conv_out(d.w[l - 1], CONV[l]); }
    return true;
}

// workspace (bytes, every region 256-byte aligned): the five taps and two pooled maps of 2F images, channels-last; the five
// small distance maps of F frames, one after the other per frame; the reduction's counters and partials
inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
struct Workspace { int64_t f[5], p[2], maps, scratch, total; int64_t ptot; };
inline Workspace workspace_layout(int64_t F, int H, int W, const Dims& d) {
    Workspace ws{};
    int64_t o = 0;
    for (int l = 0; l < 5; ++l) {
        ws.f[l] = o; o = align256(o + 4 * 2 * F * d.h[l] * d.w[l] * CONV[l].cout);
        ws.ptot += (int64_t)d.h[l] * d.w[l];
    }
    for (int i = 0; i < 2; ++i) { ws.p[i] = o; o = align256(o + 4 * 2 * F * d.ph[i] * d.pw[i] * CONV[i].cout); }
    ws.maps = o; o = align256(o + 4 * F * ws.ptot);
    ws.scratch = o; o = align256(o + frame_scratch_bytes(F, fin_blocks((int64_t)H * W), LPIPS_WORDS));
    ws.total = o;
    return ws;
}

// ---- weight packing: one launch per layer ----
template <int L>
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ lin,
                                                   float* __restrict__ dw, float* __restrict__ db, float* __restrict__ dlin) {
    constexpr int CIN = CONV[L].cin, COUT = CONV[L].cout, KS = CONV[L].ks, K = conv_k(L), KP = conv_kpad(L);
    constexpr int N_W = COUT * KP;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N_W + 2 * COUT; i += gridDim.x * 256) {
        if (i >= N_W) {
            const int j = i - N_W;
            if (j < COUT) db[j] = b[j]; else dlin[j - COUT] = lin[j - COUT];
            continue;
        }
        const int tile = i / (KP * BM), rem = i - tile * (KP * BM), k = rem / BM, m = rem - k * BM;
        float v = 0.f;
        if constexpr (L == 0) {
            const int ky = k / ROW0, e = k - ky * ROW0, kx = e / CIN, c = e - kx * CIN;
            if (e < KS * CIN) v = w[(((tile * BM + m) * CIN + c) * KS + ky) * KS + kx];
        } else {
            static_assert(K == KP, "the later layers need no zero rows");
            const int tap = k / CIN, c = k - tap * CIN, ky = tap / KS, kx = tap - ky * KS;
            v = w[(((tile * BM + m) * CIN + c) * KS + ky) * KS + kx];
        }
        dw[i] = v;
    }
}

// ---- the convolutions ----
__device__ __forceinline__ float relu(float x) { return x < 0.f ? 0.f : x; }                    // (a NaN stays a NaN)

template <int L>
__global__ __launch_bounds__(CONV_THREADS) void conv_kernel(const float* __restrict__ in0, const float* __restrict__ in1, int n_first,
                                                            const float* __restrict__ wpk, const float* __restrict__ bias,
                                                            float* __restrict__ out, int IH, int IW, int OH, int OW, int normalize) {
    constexpr int CIN = CONV[L].cin, COUT = CONV[L].cout, KS = CONV[L].ks, ST = CONV[L].stride, PD = CONV[L].pad;
    constexpr int KP = conv_kpad(L), BKL = conv_bk(L), NT = KP / BKL, NB = BKL / 4;     // NB: k rows of a step per wave
    static_assert(L == 0 || CIN % BK == 0, "a k step of the later layers lies within one tap");
    static_assert(KP % BKL == 0 && BKL % 4 == 0 && (L != 0 || NB % CIN == 0), "k steps tile K; a wave's conv1 rows start at channel 0");
    __shared__ __attribute__((aligned(16))) float s_a[BKL][BM];
    __shared__ float s_b[BKL][BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.z, OHW = OH * OW;
    const float* in = img < n_first ? in0 + (int64_t)img * IH * IW * CIN : in1 + (int64_t)(img - n_first) * IH * IW * CIN;

    // the gather: this thread's pixel of the tile and eight k rows (wave * 8 ..) of every step
    const int n = tid & 63, p = blockIdx.x * BN + n;
    const bool pv = p < OHW;
    const int oy = pv ? p / OW : 0, ox = pv ? p - oy * OW : 0;
    const int iy0 = oy * ST - PD, ix0 = ox * ST - PD;
    const float4* A = reinterpret_cast<const float4*>(wpk + (int64_t)blockIdx.y * KP * BM);

    // conv1: element e of a kernel row is float e behind the row's first tap; inside the image for e_lo <= e < e_hi
    const int e_lo = max(0, -ix0 * CIN), e_hi = min(KS * CIN, (IW - ix0) * CIN);
    float4 ra0, ra1, ra2 = make_float4(0.f, 0.f, 0.f, 0.f);
    float rb[NB];
    auto load = [&](int kt) {
        ra0 = A[kt * (BKL * BM / 4) + tid];
        ra1 = A[kt * (BKL * BM / 4) + CONV_THREADS + tid];
        if constexpr (BKL * BM / 4 > 2 * CONV_THREADS)
            if (tid < BKL * BM / 4 - 2 * CONV_THREADS) ra2 = A[kt * (BKL * BM / 4) + 2 * CONV_THREADS + tid];
        if constexpr (L == 0) {
            const int iy = iy0 + kt;                              // k step kt = kernel row ky
            const bool row = pv && (unsigned)iy < (unsigned)IH;
            const int64_t at = ((int64_t)iy * IW + ix0) * CIN;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int e = wave * NB + j, c = j % CIN;         // (NB is a multiple of CIN)
                float v = 0.f;
                if (row && e >= e_lo && e < e_hi) {
                    float x = in[at + e];
                    if (normalize) x = 2.f * x - 1.f;
                    const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
                    const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
                    v = (x - shift) / scale;
                }
                rb[j] = v;
            }
        } else {
            const int k0 = kt * BK, tap = k0 / CIN, c0 = k0 - tap * CIN + wave * 8, ky = tap / KS, kx = tap - ky * KS;
            const int iy = iy0 + ky, ix = ix0 + kx;
            float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
            if (pv && (unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW) {
                const float4* s = reinterpret_cast<const float4*>(in + ((int64_t)iy * IW + ix) * CIN + c0);
                v0 = s[0]; v1 = s[1];
            }
            rb[0] = v0.x; rb[1] = v0.y; rb[2] = v0.z; rb[3] = v0.w; rb[4] = v1.x; rb[5] = v1.y; rb[6] = v1.z; rb[7] = v1.w;
        }
    };

    const int wm = wave & 1, wn = wave >> 1, half = lane >> 5, l31 = lane & 31;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    load(0);
    for (int kt = 0; kt < NT; ++kt) {
        reinterpret_cast<float4*>(&s_a[0][0])[tid] = ra0;
        reinterpret_cast<float4*>(&s_a[0][0])[CONV_THREADS + tid] = ra1;
        if constexpr (BKL * BM / 4 > 2 * CONV_THREADS)
            if (tid < BKL * BM / 4 - 2 * CONV_THREADS) reinterpret_cast<float4*>(&s_a[0][0])[2 * CONV_THREADS + tid] = ra2;
#pragma unroll
        for (int j = 0; j < NB; ++j) s_b[wave * NB + j][n] = rb[j];
        __syncthreads();
        if (kt + 1 < NT) load(kt + 1);
#pragma unroll
        for (int kk = 0; kk < BKL / 2; ++kk) {
            const float a = s_a[kk * 2 + half][wm * 32 + l31], b = s_b[kk * 2 + half][wn * 32 + l31];
            acc[kk & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[kk & 3], 0, 0, 0);
        }
        __syncthreads();
    }

    // D: column (pixel) = lane & 31, row (cout) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): four consecutive channels per four regs
    const int pix = blockIdx.x * BN + wn * 32 + l31;
    if (pix >= OHW) return;
    const int row0 = blockIdx.y * BM + wm * 32 + 4 * half;
    float* o = out + ((int64_t)img * OHW + pix) * COUT + row0;
    const float* bz = bias + row0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * g + i;
            v[i] = relu(((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + bz[8 * g + i]);
        }
        *reinterpret_cast<float4*>(o + 8 * g) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ---- maxpool 3 s2, channels-last: (n, IH, IW, C) -> (n, OH, OW, C), C4 = C / 4.  2 (OH - 1) + 2 <= IH - 1: no edge cases ----
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }   // torch's max_pool2d keeps a NaN

__global__ __launch_bounds__(256) void pool_kernel(const float4* __restrict__ in, float4* __restrict__ out, int IH, int IW, int OH,
                                                   int OW, int C4, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        int64_t t = i / C4;
        const int ox = (int)(t % OW); t /= OW;
        const int oy = (int)(t % OH);
        const int64_t img = t / OH;
        const float4* s = in + ((img * IH + 2 * oy) * IW + 2 * ox) * C4 + c4;
        float4 m = s[0];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const float4 v = s[((int64_t)dy * IW + dx) * C4];
                m.x = max_nan(m.x, v.x); m.y = max_nan(m.y, v.y); m.z = max_nan(m.z, v.z); m.w = max_nan(m.w, v.w);
            }
        out[i] = m;
    }
}

// ---- normalise, difference, lin: one wave per feature pixel of a frame, the five taps in one launch ----
struct DistArgs {
    const float* f[5];                                            // (2F, hw, C) taps
    const float* lin[5];
    int hw[5], off[5];                                            // pixels of a tap; its first pixel in a frame's row of `maps`
    int ptot, n_frames;
    float* maps;                                                  // (F, ptot)
};
constexpr int DIST_MAX_PER_LANE = 6;                              // 384 channels / 64 lanes

__global__ __launch_bounds__(256) void dist_kernel(DistArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= a.ptot) return;
    const int64_t f = blockIdx.y;
    const float* feat = a.f[0];
    const float* lin = a.lin[0];
    int C = CONV[0].cout, hw = a.hw[0], pix = q;
#pragma unroll
    for (int l = 1; l < 5; ++l)
        if (q >= a.off[l]) { feat = a.f[l]; lin = a.lin[l]; C = CONV[l].cout; hw = a.hw[l]; pix = q - a.off[l]; }
    const float* x = feat + (f * hw + pix) * C;
    const float* y = feat + ((a.n_frames + f) * hw + pix) * C;
    float xv[DIST_MAX_PER_LANE], yv[DIST_MAX_PER_LANE];
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int i = 0; i < DIST_MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        xv[i] = c < C ? x[c] : 0.f;
        yv[i] = c < C ? y[c] : 0.f;
        sx += xv[i] * xv[i];
        sy += yv[i] * yv[i];
    }
    const float nx = sqrtf(wave_sum(sx)) + 1e-10f, ny = sqrtf(wave_sum(sy)) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < DIST_MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        const float e = xv[i] / nx - yv[i] / ny;
        if (c < C) d += lin[c] * (e * e);
    }
    d = wave_sum(d);
    if (lane == 0) a.maps[f * a.ptot + q] = d;
}

// ---- bilinear upsample of the five small maps, their sum, and the per-frame sums ----
struct FinalArgs {
    int H, W, ptot;
    int h[5], w[5], off[5];
    const float* maps;
    const uint8_t* valid;
    float* map;
    double* sums;
    unsigned* counters;
    frame_word* partials;
};

// nn.Upsample(mode='bilinear', align_corners=False): source position max((dst + 0.5) in / out - 0.5, 0), its two neighbours
// (the second clamped to the last) and the weight of the second
__device__ __forceinline__ void source_of(int dst, int n_in, int n_out, int& i0, int& i1, float& w1) {
    const double s = fmax(((double)dst + 0.5) * ((double)n_in / (double)n_out) - 0.5, 0.0);
    i0 = min((int)s, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    w1 = (float)(s - (double)i0);
}

__global__ __launch_bounds__(FIN_THREADS) void final_kernel(FinalArgs a) {
    __shared__ double s_red[FIN_THREADS / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W;
    const float* M = a.maps + f * a.ptot;
    double part[3] = {0.0, 0.0, 0.0};                             // sum, sum over the valid pixels, valid pixels
#pragma unroll
    for (int j = 0; j < FIN_PX; ++j) {
        const int64_t p = ((int64_t)blockIdx.x * FIN_THREADS + tid) * FIN_PX + j;
        if (p >= HW) break;
        const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
        float v = 0.f;
#pragma unroll
        for (int l = 0; l < 5; ++l) {
            int y0, y1, x0, x1;
            float wy, wx;
            source_of(y, a.h[l], a.H, y0, y1, wy);
            source_of(x, a.w[l], a.W, x0, x1, wx);
            const float* m = M + a.off[l];
            const float v00 = m[y0 * a.w[l] + x0], v01 = m[y0 * a.w[l] + x1], v10 = m[y1 * a.w[l] + x0], v11 = m[y1 * a.w[l] + x1];
            v += (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
        }
        if (a.map) a.map[f * HW + p] = v;
        part[0] += (double)v;
        if (a.valid && a.valid[f * HW + p]) { part[1] += (double)v; part[2] += 1.0; }
    }
    if (!a.sums) return;
#pragma unroll
    for (int t = 0; t < 3; ++t) part[t] = wave_sum(part[t]);
    if (lane == 0) { s_red[wave][0] = part[0]; s_red[wave][1] = part[1]; s_red[wave][2] = part[2]; }
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_blocks = gridDim.x;
    frame_word* fp = a.partials + f * n_blocks * LPIPS_WORDS;
    const frame_word mine[LPIPS_WORDS] = {pack_double(sum4(s_red, 0)), pack_double(sum4(s_red, 1)), pack_double(sum4(s_red, 2))};
    if (!frame_publish(fp, a.counters + f, blockIdx.x, n_blocks, lane, mine)) return;
    double acc[3] = {0.0, 0.0, 0.0};
    frame_fold<LPIPS_WORDS>(fp, n_blocks, lane, [&](const frame_word (&w)[LPIPS_WORDS]) {
        acc[0] += word_double(w[0]); acc[1] += word_double(w[1]); acc[2] += word_double(w[2]);
    });
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
        a.sums[f * 3 + 0] = acc[0]; a.sums[f * 3 + 1] = acc[1]; a.sums[f * 3 + 2] = acc[2];
        frame_counter_reset(a.counters + f);
    }
}

template <int L>
void launch_pack(const NsffLpipsWeights* w, float* packed, const PackLayout& pl, hipStream_t st) {
    const int n = CONV[L].cout * (conv_kpad(L) + 2);
    hipLaunchKernelGGL(pack_kernel<L>, dim3((n + 255) / 256), dim3(256), 0, st, w->conv_w[L], w->conv_b[L], w->lin[L], packed + pl.w[L],
                       packed + pl.b[L], packed + pl.lin[L]);
}

template <int L>
void launch_conv(const float* in0, const float* in1, int n_first, int n_images, const float* packed, const PackLayout& pl, float* out,
                 int IH, int IW, int OH, int OW, int normalize, hipStream_t st) {
    const dim3 grid((OH * OW + BN - 1) / BN, CONV[L].cout / BM, n_images);
    hipLaunchKernelGGL(conv_kernel<L>, grid, dim3(CONV_THREADS), 0, st, in0, in1, n_first, packed + pl.w[L], packed + pl.b[L], out, IH, IW,
                       OH, OW, normalize);
}

void launch_pool(const float* in, float* out, int64_t n_images, int IH, int IW, int OH, int OW, int C, hipStream_t st) {
    const int64_t total = n_images * OH * OW * (C / 4);
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(pool_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(in), reinterpret_cast<float4*>(out), IH,
                       IW, OH, OW, C / 4, total);
}

}  // namespace

extern "C" int64_t nsff_lpips_packed_bytes(void) { return 4 * pack_layout().total; }

extern "C" int nsff_lpips_dims(int32_t H, int32_t W, int32_t* hw) {
    Dims d;
    if (!hw) return NSFF_ERR_NULL;
    if (!lpips_dims(H, W, d)) return NSFF_ERR_INVALID;
    for (int l = 0; l < 5; ++l) { hw[2 * l] = d.h[l]; hw[2 * l + 1] = d.w[l]; }
    return NSFF_OK;
}

extern "C" int64_t nsff_lpips_workspace_bytes(int32_t n_frames, int32_t H, int32_t W) {
    Dims d;
    if (n_frames < 1 || n_frames > LPIPS_MAX_FRAMES || !frame_dims_ok(n_frames, H, W) || !lpips_dims(H, W, d)) return 0;
    return workspace_layout(n_frames, H, W, d).total;
}

extern "C" int nsff_lpips_pack(const NsffLpipsWeights* w, float* packed, void* stream) {
    if (!w || !packed) return NSFF_ERR_NULL;
    for (int l = 0; l < 5; ++l)
        if (!w->conv_w[l] || !w->conv_b[l] || !w->lin[l]) return NSFF_ERR_NULL;
    if ((uintptr_t)packed & 15) return NSFF_ERR_ALIGN;
    const PackLayout pl = pack_layout();
    hipStream_t st = (hipStream_t)stream;
    launch_pack<0>(w, packed, pl, st); launch_pack<1>(w, packed, pl, st); launch_pack<2>(w, packed, pl, st);
    launch_pack<3>(w, packed, pl, st); launch_pack<4>(w, packed, pl, st);
    return nsff_launch_status();
}

extern "C" int nsff_lpips(const NsffLpipsArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    Dims d;
    if (a->n_frames < 1 || a->n_frames > LPIPS_MAX_FRAMES || !frame_dims_ok(a->n_frames, a->H, a->W) || !lpips_dims(a->H, a->W, d))
        return NSFF_ERR_INVALID;
    if (!a->gt || !a->pred || !a->packed || !a->workspace) return NSFF_ERR_NULL;
    if (!a->map && !a->sums) return NSFF_ERR_INVALID;             // nothing to compute
    if (a->valid && !a->sums) return NSFF_ERR_INVALID;            // the mask selects the pixels of the sums
    const int F = a->n_frames, H = a->H, W = a->W;
    const Workspace ws = workspace_layout(F, H, W, d);
    if (a->workspace_bytes < ws.total) return NSFF_ERR_INVALID;
    if (((uintptr_t)a->workspace & 15) || ((uintptr_t)a->packed & 15)) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->gt & 3) || ((uintptr_t)a->pred & 3) || ((uintptr_t)a->map & 3) || ((uintptr_t)a->sums & 7)) return NSFF_ERR_ALIGN;

    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(a->workspace);
    float* f[5];
    for (int l = 0; l < 5; ++l) f[l] = reinterpret_cast<float*>(base + ws.f[l]);
    float* p0 = reinterpret_cast<float*>(base + ws.p[0]);
    float* p1 = reinterpret_cast<float*>(base + ws.p[1]);
    float* maps = reinterpret_cast<float*>(base + ws.maps);
    const FrameScratch fs = frame_scratch_split(base + ws.scratch, F);
    const PackLayout pl = pack_layout();
    const float* pk = a->packed;
    const int n_img = 2 * F;

    if (a->sums) {                                                // the tickets start from zero whatever the workspace held
        const hipError_t e = hipMemsetAsync(fs.counters, 0, 4 * (size_t)F, st);
        if (e != hipSuccess) return nsff_hip_fail(e);
    }
    launch_conv<0>(a->gt, a->pred, F, n_img, pk, pl, f[0], H, W, d.h[0], d.w[0], a->normalize != 0, st);
    launch_pool(f[0], p0, n_img, d.h[0], d.w[0], d.ph[0], d.pw[0], CONV[0].cout, st);
    launch_conv<1>(p0, nullptr, n_img, n_img, pk, pl, f[1], d.ph[0], d.pw[0], d.h[1], d.w[1], 0, st);
    launch_pool(f[1], p1, n_img, d.h[1], d.w[1], d.ph[1], d.pw[1], CONV[1].cout, st);
    launch_conv<2>(p1, nullptr, n_img, n_img, pk, pl, f[2], d.ph[1], d.pw[1], d.h[2], d.w[2], 0, st);
    launch_conv<3>(f[2], nullptr, n_img, n_img, pk, pl, f[3], d.h[2], d.w[2], d.h[3], d.w[3], 0, st);
    launch_conv<4>(f[3], nullptr, n_img, n_img, pk, pl, f[4], d.h[3], d.w[3], d.h[4], d.w[4], 0, st);

    DistArgs da{};
    FinalArgs fa{};
    int off = 0;
    for (int l = 0; l < 5; ++l) {
        da.f[l] = f[l]; da.lin[l] = pk + pl.lin[l]; da.hw[l] = d.h[l] * d.w[l]; da.off[l] = off;
        fa.h[l] = d.h[l]; fa.w[l] = d.w[l]; fa.off[l] = off;
        off += d.h[l] * d.w[l];
    }
    da.ptot = off; da.n_frames = F; da.maps = maps;
    hipLaunchKernelGGL(dist_kernel, dim3((off + 3) / 4, F), dim3(256), 0, st, da);
    fa.H = H; fa.W = W; fa.ptot = off; fa.maps = maps; fa.valid = a->valid; fa.map = a->map; fa.sums = a->sums;
    fa.counters = fs.counters; fa.partials = fs.partials;
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)fin_blocks((int64_t)H * W), F), dim3(FIN_THREADS), 0, st, fa);
    return nsff_launch_status();
}
