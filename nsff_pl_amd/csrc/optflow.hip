// TV-L1 optical flow between P image pairs: the classical stand-in for the reference's RAFT step (preprocess.py:106-120), so that the
// preprocessing chain images -> resize -> flow -> forward-backward check -> motion masks -> ray records needs no network.  Zach, Pock
// and Bischof 2007 in the fixed-iteration form of Sanchez, Meinhardt-Llopis and Facciolo (IPOL 2013): stencils and point-wise
// arithmetic only -- no atomics, no reductions, no device-side convergence test, nothing that depends on the launch order.
//
// include/nsff_render.h states every stage as a chain of single fp32 operations; this file is built -ffp-contract=off and
// tests/optflow_numpy.py is the same chain in numpy, compared bit for bit.  The pair is a grid dimension of every kernel: the coarse
// pyramid levels are tiny and a sequence of F frames gives 2 (F - 1) independent pairs.
//
// The iteration is the hot path (levels x warps x iters launches of it against one warp and one median per `iters`), and it has two
// routes:
//   tvl1_plain_kernel -- one iteration per launch, a thread per pixel.  p' at a pixel needs u' at its right and lower neighbours,
//     which the thread computes itself (three u updates per pixel) so that one launch is one whole iteration: the definition.
//   tvl1_fused_kernel<T, K> -- up to K iterations per launch on a T x T tile with a halo of K pixels.  One iteration reaches one
//     pixel in every direction (u' reads p at -1, p' reads u' at +1), so after j iterations the values are exact in the region
//     shrunk by j and after K the tile itself still is.  u and p live in LDS for the neighbours and in registers, with the four
//     per-warp constants, for their own pixel; two barriers an iteration.  The image's own border rules apply inside the halo by
//     image coordinates, exactly as in the plain kernel; pixels of the halo outside the image are never read by a pixel inside it.
//     Both routes call the same tv_* functions, so they agree bit for bit.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"

namespace {

constexpr int OF_THREADS = 256;
constexpr int OF_BX = 64, OF_BY = 4;                              // a workgroup of the per-pixel kernels: 64 x 4 pixels

__device__ __forceinline__ float bilerp(float c00, float c01, float c10, float c11, float ax, float ay) {
    const float omx = 1.f - ax, omy = 1.f - ay;
    const float top = c00 * omx + c01 * ax;
    const float bot = c10 * omx + c11 * ax;
    return (top * omy) + (bot * ay);
}

// ---- grey, pyramid, upsampling, median, pack ----
__global__ __launch_bounds__(OF_THREADS) void grey_kernel(const void* __restrict__ src, float* __restrict__ dst, int64_t n, int channels) {
    const int64_t i = (int64_t)blockIdx.x * OF_THREADS + threadIdx.x;
    if (i >= n) return;
    if (channels == 1) { dst[i] = static_cast<const float*>(src)[i]; return; }
    const uint8_t* c = static_cast<const uint8_t*>(src) + i * 3;
    dst[i] = (0.299f * (float)c[0] + 0.587f * (float)c[1]) + 0.114f * (float)c[2];
}

__device__ __forceinline__ float binomial(float m2, float m1, float c, float p1, float p2) {
    return (((m2 + p2) + (m1 + p1) * 4.f) + c * 6.f) * 0.0625f;
}

__global__ __launch_bounds__(OF_THREADS) void down_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int h, int w) {
    const int x = blockIdx.x * OF_BX + (threadIdx.x & (OF_BX - 1)), y = blockIdx.y * OF_BY + (threadIdx.x / OF_BX);
    if (x >= w || y >= h) return;
    const float* S = src + (int64_t)blockIdx.z * H * W;
    int xs[5], ys[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        xs[t] = min(max(2 * x + t - 2, 0), W - 1);
        ys[t] = min(max(2 * y + t - 2, 0), H - 1);
    }
    float r[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {                                 // the horizontal pass of the five rows the vertical one needs
        const float* row = S + (int64_t)ys[t] * W;
        r[t] = binomial(row[xs[0]], row[xs[1]], row[xs[2]], row[xs[3]], row[xs[4]]);
    }
    dst[((int64_t)blockIdx.z * h + y) * w + x] = binomial(r[0], r[1], r[2], r[3], r[4]);
}

__global__ __launch_bounds__(OF_THREADS) void up_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int h, int w) {
    const int x = blockIdx.x * OF_BX + (threadIdx.x & (OF_BX - 1)), y = blockIdx.y * OF_BY + (threadIdx.x / OF_BX);
    if (x >= W || y >= H) return;
    const float* S = src + (int64_t)blockIdx.z * h * w;
    const float cx = fminf((float)x * 0.5f, (float)(w - 1)), cy = fminf((float)y * 0.5f, (float)(h - 1));
    const float fx = floorf(cx), fy = floorf(cy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float v = bilerp(S[(int64_t)y0 * w + x0], S[(int64_t)y0 * w + x1], S[(int64_t)y1 * w + x0], S[(int64_t)y1 * w + x1], cx - fx, cy - fy);
    dst[((int64_t)blockIdx.z * H + y) * W + x] = v * 2.f;
}

// exchange when b < a: a plain comparison, which numpy's where() makes the same way whatever the zeros' signs
__device__ __forceinline__ void order(float& a, float& b) { const bool sw = b < a; const float lo = sw ? b : a, hi = sw ? a : b; a = lo; b = hi; }

__global__ __launch_bounds__(OF_THREADS) void median_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W) {
    const int x = blockIdx.x * OF_BX + (threadIdx.x & (OF_BX - 1)), y = blockIdx.y * OF_BY + (threadIdx.x / OF_BX);
    if (x >= W || y >= H) return;
    const float* S = src + (int64_t)blockIdx.z * H * W;
    float v[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) v[j * 3 + i] = S[(int64_t)min(max(y + j - 1, 0), H - 1) * W + min(max(x + i - 1, 0), W - 1)];
    // the nineteen exchanges of the classic median-of-nine network: v[4] ends as the fifth smallest
    order(v[1], v[2]); order(v[4], v[5]); order(v[7], v[8]); order(v[0], v[1]); order(v[3], v[4]); order(v[6], v[7]);
    order(v[1], v[2]); order(v[4], v[5]); order(v[7], v[8]); order(v[0], v[3]); order(v[5], v[8]); order(v[4], v[7]);
    order(v[3], v[6]); order(v[1], v[4]); order(v[2], v[5]); order(v[4], v[7]); order(v[4], v[2]); order(v[6], v[4]);
    order(v[4], v[2]);
    dst[((int64_t)blockIdx.z * H + y) * W + x] = v[4];
}

__global__ __launch_bounds__(OF_THREADS) void pack_kernel(const float* __restrict__ u, float2* __restrict__ flow, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * OF_THREADS + threadIdx.x;
    if (i < n) flow[i] = make_float2(u[i], u[n + i]);
}

// ---- warp ----
struct Tap { float v, dx, dy; };
__device__ __forceinline__ Tap tap_of(const float* __restrict__ I, int x, int y, int H, int W) {
    const float* row = I + (int64_t)y * W;
    Tap t;
    t.v = row[x];
    t.dx = (row[min(x + 1, W - 1)] - row[max(x - 1, 0)]) * 0.5f;
    t.dy = (I[(int64_t)min(y + 1, H - 1) * W + x] - I[(int64_t)max(y - 1, 0) * W + x]) * 0.5f;
    return t;
}

__global__ __launch_bounds__(OF_THREADS) void warp_kernel(const float* __restrict__ I0, const float* __restrict__ I1, const float* __restrict__ u,
                                                          float* __restrict__ consts, int H, int W, int64_t N) {
    const int x = blockIdx.x * OF_BX + (threadIdx.x & (OF_BX - 1)), y = blockIdx.y * OF_BY + (threadIdx.x / OF_BX);
    if (x >= W || y >= H) return;
    const int64_t HW = (int64_t)H * W, i = blockIdx.z * HW + (int64_t)y * W + x;
    const float* B = I1 + blockIdx.z * HW;
    const float u1 = u[i], u2 = u[N + i];
    // clamped into the image (a NaN clamps to 0): no address leaves the pair's frame whatever the flow holds
    const float cx = fminf(fmaxf((float)x + u1, 0.f), (float)(W - 1)), cy = fminf(fmaxf((float)y + u2, 0.f), (float)(H - 1));
    const float fx = floorf(cx), fy = floorf(cy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float ax = cx - fx, ay = cy - fy;
    const Tap t00 = tap_of(B, x0, y0, H, W), t01 = tap_of(B, x1, y0, H, W), t10 = tap_of(B, x0, y1, H, W), t11 = tap_of(B, x1, y1, H, W);
    const float I1w = bilerp(t00.v, t01.v, t10.v, t11.v, ax, ay);
    const float Ix = bilerp(t00.dx, t01.dx, t10.dx, t11.dx, ax, ay);
    const float Iy = bilerp(t00.dy, t01.dy, t10.dy, t11.dy, ax, ay);
    consts[i] = Ix;
    consts[N + i] = Iy;
    consts[2 * N + i] = Ix * Ix + Iy * Iy;
    consts[3 * N + i] = ((I1w - Ix * u1) - Iy * u2) - I0[i];
    consts[4 * N + i] = I1w;
}

// ---- the iteration's arithmetic, shared by both routes ----
struct TvParams { float l_t, theta, taut; };

// the backward difference of the divergence: p in the first column / row, p - p(-1) inside, -p(-1) in the last
__device__ __forceinline__ float tv_back(float here, float before, int pos, int last) {
    return pos == 0 ? here : (pos == last ? -before : here - before);
}

__device__ __forceinline__ void tv_u(const TvParams& k, float Ix, float Iy, float g, float rho_c, float u1, float u2, float div1, float div2,
                                     float& u1n, float& u2n) {
    const float rho = (rho_c + Ix * u1) + Iy * u2;
    const float lg = k.l_t * g;
    const float f = rho < -lg ? k.l_t : (rho > lg ? -k.l_t : (g > 1e-10f ? (-rho) / g : 0.f));
    const float v1 = u1 + f * Ix, v2 = u2 + f * Iy;
    u1n = v1 + k.theta * div1;
    u2n = v2 + k.theta * div2;
}

__device__ __forceinline__ void tv_p(const TvParams& k, float pa, float pb, float ux, float uy, float& pan, float& pbn) {
    const float ng = sqrtf(ux * ux + uy * uy);
    const float den = 1.f + k.taut * ng;
    pan = (pa + k.taut * ux) / den;
    pbn = (pb + k.taut * uy) / den;
}

// u' at one pixel from global memory (the plain route)
__device__ __forceinline__ void plain_u(const TvParams& k, const float* __restrict__ c, const float* __restrict__ s, int64_t N, int64_t base,
                                        int x, int y, int H, int W, float& u1n, float& u2n) {
    const int64_t i = base + (int64_t)y * W + x;
    const int64_t il = x > 0 ? i - 1 : i, iu = y > 0 ? i - W : i;
    const float div1 = tv_back(s[2 * N + i], s[2 * N + il], x, W - 1) + tv_back(s[3 * N + i], s[3 * N + iu], y, H - 1);
    const float div2 = tv_back(s[4 * N + i], s[4 * N + il], x, W - 1) + tv_back(s[5 * N + i], s[5 * N + iu], y, H - 1);
    tv_u(k, c[i], c[N + i], c[2 * N + i], c[3 * N + i], s[i], s[N + i], div1, div2, u1n, u2n);
}

__global__ __launch_bounds__(OF_THREADS) void tvl1_plain_kernel(TvParams k, const float* __restrict__ c, const float* __restrict__ s,
                                                                float* __restrict__ d, int H, int W, int64_t N) {
    const int x = blockIdx.x * OF_BX + (threadIdx.x & (OF_BX - 1)), y = blockIdx.y * OF_BY + (threadIdx.x / OF_BX);
    if (x >= W || y >= H) return;
    const int64_t base = (int64_t)blockIdx.z * H * W, i = base + (int64_t)y * W + x;
    float u1, u2, r1 = 0.f, r2 = 0.f, d1 = 0.f, d2 = 0.f;
    plain_u(k, c, s, N, base, x, y, H, W, u1, u2);
    if (x < W - 1) plain_u(k, c, s, N, base, x + 1, y, H, W, r1, r2);
    if (y < H - 1) plain_u(k, c, s, N, base, x, y + 1, H, W, d1, d2);
    const float ux1 = x < W - 1 ? r1 - u1 : 0.f, uy1 = y < H - 1 ? d1 - u1 : 0.f;
    const float ux2 = x < W - 1 ? r2 - u2 : 0.f, uy2 = y < H - 1 ? d2 - u2 : 0.f;
    float p11, p12, p21, p22;
    tv_p(k, s[2 * N + i], s[3 * N + i], ux1, uy1, p11, p12);
    tv_p(k, s[4 * N + i], s[5 * N + i], ux2, uy2, p21, p22);
    d[i] = u1; d[N + i] = u2;
    d[2 * N + i] = p11; d[3 * N + i] = p12; d[4 * N + i] = p21; d[5 * N + i] = p22;
}

// The fused route.  The region is R x R = (T + 2 K)^2 pixels, row-major; thread t owns the pixels t, t + 256, ...  The LDS planes
// carry a guard row before and after, so that i - R, i - 1, i + 1 and i + R are addresses of the plane for every pixel of the
// region: what a pixel on the region's edge reads from there is as wrong as the edge itself already is, and stays outside the
// region that is still exact.
template <int T, int K>
__global__ __launch_bounds__(OF_THREADS) void tvl1_fused_kernel(TvParams k, const float* __restrict__ c, const float* __restrict__ s,
                                                                float* __restrict__ d, int H, int W, int64_t N, int n_it) {
    constexpr int R = T + 2 * K, RR = R * R, NP = (RR + OF_THREADS - 1) / OF_THREADS, PLANE = RR + 2 * R;
    __shared__ float s_u1[PLANE], s_u2[PLANE], s_p11[PLANE], s_p12[PLANE], s_p21[PLANE], s_p22[PLANE];
    const int tid = threadIdx.x;
    const int gx0 = blockIdx.x * T - K, gy0 = blockIdx.y * T - K;
    const int64_t base = (int64_t)blockIdx.z * H * W;

    float Ix[NP], Iy[NP], g[NP], rc[NP], u1[NP], u2[NP], p11[NP], p12[NP], p21[NP], p22[NP];
    int px[NP], py[NP];                                           // image coordinates; px < 0: not a pixel of the image
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int r = tid + j * OF_THREADS, ry = r / R, rx = r - ry * R;
        const int x = gx0 + rx, y = gy0 + ry;
        const bool in = r < RR && x >= 0 && x < W && y >= 0 && y < H;
        px[j] = in ? x : -1; py[j] = y;
        Ix[j] = Iy[j] = g[j] = rc[j] = u1[j] = u2[j] = p11[j] = p12[j] = p21[j] = p22[j] = 0.f;
        if (in) {
            const int64_t i = base + (int64_t)y * W + x;
            Ix[j] = c[i]; Iy[j] = c[N + i]; g[j] = c[2 * N + i]; rc[j] = c[3 * N + i];
            u1[j] = s[i]; u2[j] = s[N + i];
            p11[j] = s[2 * N + i]; p12[j] = s[3 * N + i]; p21[j] = s[4 * N + i]; p22[j] = s[5 * N + i];
        }
        if (r < RR) { s_p11[R + r] = p11[j]; s_p12[R + r] = p12[j]; s_p21[R + r] = p21[j]; s_p22[R + r] = p22[j]; }
    }
    for (int it = 0; it < n_it; ++it) {
        __syncthreads();                                          // p of the previous iteration (or the load) is in LDS
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (px[j] < 0) continue;
            const int r = R + tid + j * OF_THREADS;
            const float div1 = tv_back(p11[j], s_p11[r - 1], px[j], W - 1) + tv_back(p12[j], s_p12[r - R], py[j], H - 1);
            const float div2 = tv_back(p21[j], s_p21[r - 1], px[j], W - 1) + tv_back(p22[j], s_p22[r - R], py[j], H - 1);
            tv_u(k, Ix[j], Iy[j], g[j], rc[j], u1[j], u2[j], div1, div2, u1[j], u2[j]);
            s_u1[r] = u1[j]; s_u2[r] = u2[j];
        }
        __syncthreads();                                          // u' is in LDS
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (px[j] < 0) continue;
            const int r = R + tid + j * OF_THREADS;
            const bool right = px[j] < W - 1, down = py[j] < H - 1;
            const float ux1 = right ? s_u1[r + 1] - u1[j] : 0.f, uy1 = down ? s_u1[r + R] - u1[j] : 0.f;
            const float ux2 = right ? s_u2[r + 1] - u2[j] : 0.f, uy2 = down ? s_u2[r + R] - u2[j] : 0.f;
            tv_p(k, p11[j], p12[j], ux1, uy1, p11[j], p12[j]);
            tv_p(k, p21[j], p22[j], ux2, uy2, p21[j], p22[j]);
            s_p11[r] = p11[j]; s_p12[r] = p12[j]; s_p21[r] = p21[j]; s_p22[r] = p22[j];
        }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int r = tid + j * OF_THREADS, ry = r / R, rx = r - ry * R;
        if (px[j] < 0 || rx < K || rx >= K + T || ry < K || ry >= K + T) continue;
        const int64_t i = base + (int64_t)py[j] * W + px[j];
        d[i] = u1[j]; d[N + i] = u2[j];
        d[2 * N + i] = p11[j]; d[3 * N + i] = p12[j]; d[4 * N + i] = p21[j]; d[5 * N + i] = p22[j];
    }
}

// ---- host side ----
constexpr int64_t OF_MAX_PIXELS = 0x7fffffffLL;

inline bool planes_ok(int64_t n, int32_t H, int32_t W, int32_t min_side) {
    return n >= 1 && n <= 65535 && H >= min_side && W >= min_side && H <= 65535 && W <= 65535 && n * (int64_t)H * W <= OF_MAX_PIXELS;
}
inline dim3 pixel_grid(int32_t n, int32_t H, int32_t W) { return dim3((W + OF_BX - 1) / OF_BX, (H + OF_BY - 1) / OF_BY, n); }
inline bool positive(float v) { return v > 0.f && v <= 3.0e38f; }
inline bool off4(const void* p) { return ((uintptr_t)p & 3) != 0; }

inline int fused_pair_ok(int tile, int k) {
    return (tile == 32 && (k == 2 || k == 3 || k == 4 || k == 6)) || (tile == 16 && k == 2);
}

template <int T, int K>
void launch_fused(const TvParams& p, const float* c, const float* s, float* d, int n, int H, int W, int64_t N, int n_it, hipStream_t st) {
    const dim3 grid((W + T - 1) / T, (H + T - 1) / T, n);
    hipLaunchKernelGGL((tvl1_fused_kernel<T, K>), grid, dim3(OF_THREADS), 0, st, p, c, s, d, H, W, N, n_it);
}

// `iters` iterations from state[0]; returns the slot that holds the result.  The arguments were checked by the caller.
int run_iterations(const TvParams& p, const float* c, float* const state[2], int n, int H, int W, int iters, int fused, int tile, int k,
                   hipStream_t st) {
    const int64_t N = (int64_t)n * H * W;
    int slot = 0;
    if (!fused) {
        for (int it = 0; it < iters; ++it, slot ^= 1)
            hipLaunchKernelGGL(tvl1_plain_kernel, pixel_grid(n, H, W), dim3(OF_THREADS), 0, st, p, c, state[slot], state[slot ^ 1], H, W, N);
        return slot;
    }
    for (int done = 0; done < iters; done += k, slot ^= 1) {
        const int n_it = iters - done < k ? iters - done : k;
        const float* s = state[slot];
        float* d = state[slot ^ 1];
        if (tile == 32 && k == 2) launch_fused<32, 2>(p, c, s, d, n, H, W, N, n_it, st);
        else if (tile == 32 && k == 3) launch_fused<32, 3>(p, c, s, d, n, H, W, N, n_it, st);
        else if (tile == 32 && k == 4) launch_fused<32, 4>(p, c, s, d, n, H, W, N, n_it, st);
        else if (tile == 32 && k == 6) launch_fused<32, 6>(p, c, s, d, n, H, W, N, n_it, st);
        else launch_fused<16, 2>(p, c, s, d, n, H, W, N, n_it, st);
    }
    return slot;
}

inline TvParams tv_params(float lambda, float theta, float tau) {
    TvParams p;
    p.l_t = lambda * theta; p.theta = theta; p.taut = tau / theta;
    return p;
}

void launch_down(const float* src, float* dst, int n, int H, int W, hipStream_t st) {
    const int h = (H + 1) / 2, w = (W + 1) / 2;
    hipLaunchKernelGGL(down_kernel, pixel_grid(n, h, w), dim3(OF_THREADS), 0, st, src, dst, H, W, h, w);
}
void launch_up(const float* src, float* dst, int n, int H, int W, hipStream_t st) {
    hipLaunchKernelGGL(up_kernel, pixel_grid(n, H, W), dim3(OF_THREADS), 0, st, src, dst, H, W, (H + 1) / 2, (W + 1) / 2);
}
void launch_grey(const void* src, float* dst, int64_t n, int channels, hipStream_t st) {
    hipLaunchKernelGGL(grey_kernel, dim3((unsigned)((n + OF_THREADS - 1) / OF_THREADS)), dim3(OF_THREADS), 0, st, src, dst, n, channels);
}

constexpr int OF_MAX_LEVELS = 16;
struct Pyramid { int levels; int H[OF_MAX_LEVELS], W[OF_MAX_LEVELS]; int64_t offset[OF_MAX_LEVELS + 1]; };     // offsets in pixels of ONE image set

// the levels of an H x W image, clipped so that the coarsest keeps both sides >= 4
Pyramid pyramid_of(int64_t n, int H, int W, int levels) {
    Pyramid p;
    p.levels = 0; p.offset[0] = 0;
    for (int l = 0; l < levels && l < OF_MAX_LEVELS; ++l) {
        if (l > 0 && (H < 4 || W < 4)) break;
        p.H[l] = H; p.W[l] = W;
        p.offset[l + 1] = p.offset[l] + ((n * H * W + 3) & ~(int64_t)3);
        p.levels = l + 1;
        H = (H + 1) / 2; W = (W + 1) / 2;
    }
    return p;
}

inline bool flow_dims_ok(int32_t n, int32_t H, int32_t W, int32_t levels) {
    return n <= 32767 && planes_ok(n, H, W, NSFF_OPTFLOW_MIN_SIZE) && levels >= 1 && levels <= OF_MAX_LEVELS;      // (u1 | u2 are 2 n planes)
}

}  // namespace

extern "C" int nsff_optflow_grey(const void* src, float* dst, int32_t n, int32_t H, int32_t W, int32_t channels, void* stream) {
    if (!planes_ok(n, H, W, 1) || (channels != 1 && channels != 3)) return NSFF_ERR_INVALID;
    if (!src || !dst) return NSFF_ERR_NULL;
    if (off4(dst) || (channels == 1 && off4(src))) return NSFF_ERR_ALIGN;
    launch_grey(src, dst, (int64_t)n * H * W, channels, (hipStream_t)stream);
    return nsff_launch_status();
}

extern "C" int nsff_optflow_down(const float* src, float* dst, int32_t n, int32_t H, int32_t W, void* stream) {
    if (!planes_ok(n, H, W, 2)) return NSFF_ERR_INVALID;
    if (!src || !dst) return NSFF_ERR_NULL;
    if (off4(src) || off4(dst)) return NSFF_ERR_ALIGN;
    launch_down(src, dst, n, H, W, (hipStream_t)stream);
    return nsff_launch_status();
}

extern "C" int nsff_optflow_up(const float* src, float* dst, int32_t n, int32_t H, int32_t W, void* stream) {
    if (!planes_ok(n, H, W, 2)) return NSFF_ERR_INVALID;
    if (!src || !dst) return NSFF_ERR_NULL;
    if (off4(src) || off4(dst)) return NSFF_ERR_ALIGN;
    launch_up(src, dst, n, H, W, (hipStream_t)stream);
    return nsff_launch_status();
}

extern "C" int nsff_optflow_median(const float* src, float* dst, int32_t n, int32_t H, int32_t W, void* stream) {
    if (!planes_ok(n, H, W, 1) || (src && src == dst)) return NSFF_ERR_INVALID;
    if (!src || !dst) return NSFF_ERR_NULL;
    if (off4(src) || off4(dst)) return NSFF_ERR_ALIGN;
    hipLaunchKernelGGL(median_kernel, pixel_grid(n, H, W), dim3(OF_THREADS), 0, (hipStream_t)stream, src, dst, H, W);
    return nsff_launch_status();
}

extern "C" int nsff_optflow_warp(const float* I0, const float* I1, const float* u, float* consts, int32_t n_pairs, int32_t H, int32_t W,
                                 void* stream) {
    if (!planes_ok(n_pairs, H, W, 1)) return NSFF_ERR_INVALID;
    if (!I0 || !I1 || !u || !consts) return NSFF_ERR_NULL;
    if (off4(I0) || off4(I1) || off4(u) || off4(consts)) return NSFF_ERR_ALIGN;
    hipLaunchKernelGGL(warp_kernel, pixel_grid(n_pairs, H, W), dim3(OF_THREADS), 0, (hipStream_t)stream, I0, I1, u, consts, H, W,
                       (int64_t)n_pairs * H * W);
    return nsff_launch_status();
}

extern "C" int nsff_optflow_result_slot(int32_t iters, int32_t k) {
    if (iters < 1 || k < 1) return NSFF_ERR_INVALID;
    return ((iters + k - 1) / k) & 1;
}

namespace {
// the route's checks, shared by nsff_optflow_iterate and nsff_optflow; tile / k come back resolved
int check_route(int32_t iters, int32_t fused, int32_t& tile, int32_t& k, float lambda, float theta, float tau) {
    if (iters < 1 || iters > 100000 || (fused != 0 && fused != 1)) return NSFF_ERR_INVALID;
    if (!positive(lambda) || !positive(theta) || !positive(tau)) return NSFF_ERR_INVALID;
    if (tile == 0 && k == 0) { tile = NSFF_OPTFLOW_TILE; k = NSFF_OPTFLOW_K; }
    if (fused && !fused_pair_ok(tile, k)) return NSFF_ERR_INVALID;
    return NSFF_OK;
}
}  // namespace

extern "C" int nsff_optflow_iterate(const NsffOptflowIterArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!planes_ok(a->n_pairs, a->H, a->W, 4)) return NSFF_ERR_INVALID;
    int32_t tile = a->tile, k = a->k;
    if (const int rc = check_route(a->iters, a->fused, tile, k, a->lambda, a->theta, a->tau)) return rc;
    if (!a->consts || !a->state[0] || !a->state[1]) return NSFF_ERR_NULL;
    if (a->state[0] == a->state[1]) return NSFF_ERR_INVALID;
    if (off4(a->consts) || off4(a->state[0]) || off4(a->state[1])) return NSFF_ERR_ALIGN;
    run_iterations(tv_params(a->lambda, a->theta, a->tau), a->consts, a->state, a->n_pairs, a->H, a->W, a->iters, a->fused, tile, k,
                   (hipStream_t)stream);
    return nsff_launch_status();
}

extern "C" int nsff_optflow_levels(int32_t H, int32_t W, int32_t levels) {
    if (!flow_dims_ok(1, H, W, levels)) return 0;
    return pyramid_of(1, H, W, levels).levels;
}

// two pyramids, two states of six planes, five planes of per-warp constants and the median's two planes
extern "C" int64_t nsff_optflow_scratch_bytes(int32_t n_pairs, int32_t H, int32_t W, int32_t levels) {
    if (!flow_dims_ok(n_pairs, H, W, levels)) return 0;
    const Pyramid p = pyramid_of(n_pairs, H, W, levels);
    return (2 * p.offset[p.levels] + (6 + 6 + 5 + 2) * p.offset[1]) * (int64_t)sizeof(float);
}

extern "C" int nsff_optflow(const NsffOptflowArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!flow_dims_ok(a->n_pairs, a->H, a->W, a->levels)) return NSFF_ERR_INVALID;
    if ((a->channels != 1 && a->channels != 3) || a->warps < 1 || a->warps > 1000 || (a->median != 0 && a->median != 1)) return NSFF_ERR_INVALID;
    int32_t tile = a->tile, k = a->k;
    if (const int rc = check_route(a->iters, a->fused, tile, k, a->lambda, a->theta, a->tau)) return rc;
    if (!a->images0 || !a->images1 || !a->flow || !a->scratch) return NSFF_ERR_NULL;
    if (a->scratch_bytes < nsff_optflow_scratch_bytes(a->n_pairs, a->H, a->W, a->levels)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    if ((uintptr_t)a->flow & 7) return NSFF_ERR_ALIGN;
    if (a->channels == 1 && (off4(a->images0) || off4(a->images1))) return NSFF_ERR_ALIGN;

    hipStream_t st = (hipStream_t)stream;
    const int n = a->n_pairs;
    const Pyramid py = pyramid_of(n, a->H, a->W, a->levels);
    const int64_t N0 = py.offset[1];                              // one plane of the finest level, padded to four floats
    float* pyr0 = static_cast<float*>(a->scratch);
    float* pyr1 = pyr0 + py.offset[py.levels];
    float* state[2] = {pyr1 + py.offset[py.levels], pyr1 + py.offset[py.levels] + 6 * N0};
    float* consts = state[1] + 6 * N0;
    float* med = consts + 5 * N0;
    const TvParams tv = tv_params(a->lambda, a->theta, a->tau);

    launch_grey(a->images0, pyr0, (int64_t)n * a->H * a->W, a->channels, st);
    launch_grey(a->images1, pyr1, (int64_t)n * a->H * a->W, a->channels, st);
    for (int l = 1; l < py.levels; ++l) {
        launch_down(pyr0 + py.offset[l - 1], pyr0 + py.offset[l], n, py.H[l - 1], py.W[l - 1], st);
        launch_down(pyr1 + py.offset[l - 1], pyr1 + py.offset[l], n, py.H[l - 1], py.W[l - 1], st);
    }
    int cur = 0;                                                  // the state buffer that holds the flow so far
    for (int l = py.levels - 1; l >= 0; --l) {
        const int H = py.H[l], W = py.W[l];
        const int64_t N = (int64_t)n * H * W;                     // a plane of this level: the state is six of them, back to back
        if (l == py.levels - 1) {
            if (const hipError_t e = hipMemsetAsync(state[cur], 0, 6 * N * sizeof(float), st)) return nsff_hip_fail(e);
        } else {                                                  // the coarser level's u1 | u2 are 2 n planes of its size
            launch_up(state[cur], state[cur ^ 1], 2 * n, H, W, st);
            cur ^= 1;
            if (const hipError_t e = hipMemsetAsync(state[cur] + 2 * N, 0, 4 * N * sizeof(float), st)) return nsff_hip_fail(e);
        }
        for (int w = 0; w < a->warps; ++w) {
            hipLaunchKernelGGL(warp_kernel, pixel_grid(n, H, W), dim3(OF_THREADS), 0, st, pyr0 + py.offset[l], pyr1 + py.offset[l],
                               state[cur], consts, H, W, N);
            float* const bufs[2] = {state[cur], state[cur ^ 1]};
            cur ^= run_iterations(tv, consts, bufs, n, H, W, a->iters, a->fused, tile, k, st);
            if (a->median) {
                hipLaunchKernelGGL(median_kernel, pixel_grid(2 * n, H, W), dim3(OF_THREADS), 0, st, state[cur], med, H, W);
                if (const hipError_t e = hipMemcpyAsync(state[cur], med, 2 * N * sizeof(float), hipMemcpyDeviceToDevice, st)) return nsff_hip_fail(e);
            }
        }
    }
    const int64_t N = (int64_t)n * a->H * a->W;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((N + OF_THREADS - 1) / OF_THREADS)), dim3(OF_THREADS), 0, st, state[cur],
                       reinterpret_cast<float2*>(a->flow), N);
    return nsff_launch_status();
}
