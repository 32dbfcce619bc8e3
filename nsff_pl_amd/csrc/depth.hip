// Disparity from optical flow and camera poses: the classical stand-in for the reference's DPT step (preprocess.py:106-115), so that
// the preprocessing chain images -> resize -> flow -> forward-backward check -> motion masks -> disparity -> ray records needs no
// network.  For a STATIC pixel flow plus two poses is a depth measurement (motion parallax); where there is none -- dynamic pixels,
// occlusions, too little parallax -- an image-guided fill gives a dense map.
//
// include/nsff_render.h states every stage as a chain of single fp32 operations; this file is built -ffp-contract=off and
// tests/disparity_numpy.py is the same chain in numpy, compared bit for bit.  No atomics on floats, no device-side convergence test,
// no data-dependent loop; the frame is a grid dimension of every kernel and a call is a fixed list of launches.
//
// disparity_sparse_kernel -- all F frames and both directions in one launch, on the pixel quads of nsff_frame_ops.h: the
//   least-squares disparity of a pixel over its voting directions as the pair (n, c), c the parallax in px^2 and n = c * disparity
//   (the vote is parallax_vote of nsff_flow_chain.h, which nsff_disparity_span of parallax.hip takes along a chain of flows), and
//   the per-frame count of known pixels through frame_count_finish of nsff_frame_ops.h.
// push_kernel / pull_kernel -- one step up and one step down the 2 x 2 pyramid that runs to 1 x 1: sums of clipped blocks in
//   row-major order on the way up, n / c or the parent's value on the way down (without c / n: the parent's value alone, the
//   nearest-neighbour upsampling).
// The relaxation is the hot path (levels x iters launches), and it has two routes that call the same rx_* functions and agree bit for
// bit, on the pattern of tvl1_plain_kernel / tvl1_fused_kernel<T, K> of optflow.hip:
//   relax_plain_kernel -- one weighted-Jacobi iteration per launch, a thread per pixel: the definition.
//   relax_fused<T, K> -- up to K iterations per launch on a T x T tile with a halo of K pixels.  One iteration reaches one pixel in
//     every direction, so after j iterations the values are exact in the region shrunk by j.  d lives in two LDS planes that take
//     turns (one barrier an iteration); a thread keeps n, c, its four edge weights -- computed once per launch -- and its own d in
//     registers.  The border rules apply inside the halo by image coordinates.
// The edge weights are recomputed from the grey guide instead of being stored per level: an iteration then moves d, n, c and grey
// in and d out, 20 bytes a pixel, against 24 with two stored weight planes.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_flow_chain.h"

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_BX = 64, DP_BY = 4;                              // a workgroup of the per-pixel kernels: 64 x 4 pixels

// ---- sparse ----
__global__ __launch_bounds__(FIN_THREADS) void disparity_sparse_kernel(NsffDisparitySparseArgs a, float mp2, int aligned,
                                                                       unsigned* __restrict__ counters, frame_word* __restrict__ partials) {
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.y, HW = (int64_t)a.H * a.W;
    const Quad q = quad_of(blockIdx.x, tid, f, HW, aligned);

    float xs[FIN_PX], ys[FIN_PX];
    quad_pixels(q, HW, a.W, xs, ys);
    float num[FIN_PX] = {0.f, 0.f, 0.f, 0.f}, den[FIN_PX] = {0.f, 0.f, 0.f, 0.f}, par[FIN_PX] = {0.f, 0.f, 0.f, 0.f};
    bool is_static[FIN_PX];
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) is_static[i] = !a.masks || (i < q.n && a.masks[q.q0 + i] != 0);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        float P[12];
        bool row = false;                                         // (uniform in the workgroup)
#pragma unroll
        for (int i = 0; i < 12; ++i) { P[i] = a.Pm[(f * 2 + d) * 12 + i]; row = row || P[i] != 0.f; }
        float av[2 * FIN_PX];
        load_px<2>(d == 0 ? a.flow_fw : a.flow_bw, q, av);
        const int64_t plane = (f * 2 + d) * HW + q.p0;            // the direction's plane of `valid`
#pragma unroll
        for (int i = 0; i < FIN_PX; ++i) {
            const float u = av[2 * i], v = av[2 * i + 1];
            float p2, ab, aa, hz;
            parallax_vote(P, xs[i], ys[i], xs[i] + u, ys[i] + v, p2, ab, aa, hz);
            bool vote = row && i < q.n && flow_known(u, v) && is_static[i] && hz > 0.f && p2 >= mp2;
            if (a.valid) vote = vote && i < q.n && a.valid[plane + i] != 0;
            num[i] = num[i] + (vote ? ab : 0.f);
            den[i] = den[i] + (vote ? aa : 0.f);
            par[i] = par[i] + (vote ? p2 : 0.f);
        }
    }
    float cv[FIN_PX], nv[FIN_PX];
    uint32_t cnt = 0u;
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        const bool kn = i < q.n && den[i] > 0.f && num[i] > 0.f;
        cv[i] = kn ? par[i] : 0.f;
        nv[i] = kn ? par[i] * (num[i] / den[i]) : 0.f;
        cnt += kn ? 1u : 0u;
    }
    if (q.n > 0) {
        store_px<1>(a.c, q, cv);
        store_px<1>(a.n, q, nv);
    }
    if (a.counts) frame_count_finish<1, FIN_THREADS>({cnt}, a.counts, counters, partials, f);
}

// ---- the pyramid ----
// the clipped 2 x 2 block of (x, y) in row-major order
__device__ __forceinline__ float block_sum(const float* __restrict__ S, int x, int y, int H, int W) {
    const int x0 = 2 * x, y0 = 2 * y;
    const bool right = x0 + 1 < W, down = y0 + 1 < H;
    const float* r0 = S + (int64_t)y0 * W;
    const float* r1 = S + (int64_t)(down ? y0 + 1 : y0) * W;
    float s = r0[x0];
    if (right) s = s + r0[x0 + 1];
    if (down) s = s + r1[x0];
    if (right && down) s = s + r1[x0 + 1];
    return s;
}

__global__ __launch_bounds__(DP_THREADS) void push_kernel(const float* __restrict__ c, const float* __restrict__ n, const float* __restrict__ g,
                                                          float* __restrict__ c2, float* __restrict__ n2, float* __restrict__ g2,
                                                          int H, int W, int h, int w) {
    const int x = blockIdx.x * DP_BX + (threadIdx.x & (DP_BX - 1)), y = blockIdx.y * DP_BY + (threadIdx.x / DP_BX);
    if (x >= w || y >= h) return;
    const int64_t src = (int64_t)blockIdx.z * H * W, dst = ((int64_t)blockIdx.z * h + y) * w + x;
    const float count = (float)((2 * x + 1 < W ? 2 : 1) * (2 * y + 1 < H ? 2 : 1));
    c2[dst] = block_sum(c + src, x, y, H, W);
    n2[dst] = block_sum(n + src, x, y, H, W);
    g2[dst] = block_sum(g + src, x, y, H, W) / count;
}

// d = c > 0 ? n / c : parent(y >> 1, x >> 1); no parent: 0; no c: the parent's value alone
__global__ __launch_bounds__(DP_THREADS) void pull_kernel(const float* __restrict__ c, const float* __restrict__ n, const float* __restrict__ parent,
                                                          float* __restrict__ d, int H, int W, int h, int w) {
    const int x = blockIdx.x * DP_BX + (threadIdx.x & (DP_BX - 1)), y = blockIdx.y * DP_BY + (threadIdx.x / DP_BX);
    if (x >= W || y >= H) return;
    const int64_t i = ((int64_t)blockIdx.z * H + y) * W + x;
    const float below = parent ? parent[((int64_t)blockIdx.z * h + (y >> 1)) * w + (x >> 1)] : 0.f;
    if (!c) { d[i] = below; return; }
    const float cc = c[i];
    d[i] = cc > 0.f ? n[i] / cc : below;
}

// ---- the relaxation's arithmetic, shared by both routes ----
struct RxParams { float lam, sigma; };

// the weight of the edge between two pixels from their grey values: symmetric
__device__ __forceinline__ float rx_weight(const RxParams& k, float here, float there) {
    const float t = (here - there) / k.sigma;
    return 1.f / (1.f + t * t);
}

// one Jacobi update; g* are 0 and the neighbour's value is not used where the neighbour is outside the image
__device__ __forceinline__ float rx_update(const RxParams& k, float d, float n, float c, float gl, float gr, float gu, float gd,
                                           bool hl, bool hr, bool hu, bool hd, float dl, float dr, float du, float dd) {
    float S = 0.f, Wt = 0.f;
    S = S + (hl ? gl * dl : 0.f); Wt = Wt + gl;
    S = S + (hr ? gr * dr : 0.f); Wt = Wt + gr;
    S = S + (hu ? gu * du : 0.f); Wt = Wt + gu;
    S = S + (hd ? gd * dd : 0.f); Wt = Wt + gd;
    const float num = n + k.lam * S;
    const float den = c + k.lam * Wt;
    return den > 0.f ? num / den : d;
}

__global__ __launch_bounds__(DP_THREADS) void relax_plain_kernel(RxParams k, const float* __restrict__ n, const float* __restrict__ c,
                                                                 const float* __restrict__ grey, const float* __restrict__ s,
                                                                 float* __restrict__ d, int H, int W) {
    const int x = blockIdx.x * DP_BX + (threadIdx.x & (DP_BX - 1)), y = blockIdx.y * DP_BY + (threadIdx.x / DP_BX);
    if (x >= W || y >= H) return;
    const int64_t i = ((int64_t)blockIdx.z * H + y) * W + x;
    const bool hl = x > 0, hr = x < W - 1, hu = y > 0, hd = y < H - 1;
    const int64_t il = hl ? i - 1 : i, ir = hr ? i + 1 : i, iu = hu ? i - W : i, id = hd ? i + W : i;
    const float gh = grey[i];
    const float gl = hl ? rx_weight(k, gh, grey[il]) : 0.f, gr = hr ? rx_weight(k, gh, grey[ir]) : 0.f;
    const float gu = hu ? rx_weight(k, gh, grey[iu]) : 0.f, gd = hd ? rx_weight(k, gh, grey[id]) : 0.f;
    d[i] = rx_update(k, s[i], n[i], c[i], gl, gr, gu, gd, hl, hr, hu, hd, s[il], s[ir], s[iu], s[id]);
}

// The fused route.  The region is R x R = (T + 2 K)^2 pixels, row-major; thread t owns the pixels t, t + 256, ...  The LDS planes
// carry a guard row before and after, so that i - R, i - 1, i + 1 and i + R are addresses of the plane for every pixel of the
// region: what a pixel on the region's edge reads from there is as wrong as the edge itself already is, and stays outside the
// region that is still exact.  Pixels of the region outside the image own nothing and are never read by a pixel inside it.
template <int T, int K>
__global__ __launch_bounds__(DP_THREADS) void relax_fused(RxParams k, const float* __restrict__ n, const float* __restrict__ c,
                                                          const float* __restrict__ grey, const float* __restrict__ s,
                                                          float* __restrict__ d, int H, int W, int n_it) {
    constexpr int R = T + 2 * K, RR = R * R, NP = (RR + DP_THREADS - 1) / DP_THREADS, PLANE = RR + 2 * R;
    __shared__ float s_d[2][PLANE];
    const int tid = threadIdx.x;
    const int gx0 = blockIdx.x * T - K, gy0 = blockIdx.y * T - K;
    const int64_t base = (int64_t)blockIdx.z * H * W;

    float nn[NP], cc[NP], dv[NP], gl[NP], gr[NP], gu[NP], gd[NP];
    int px[NP], py[NP];                                           // image coordinates; px < 0: not a pixel of the image
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int r = tid + j * DP_THREADS, ry = r / R, rx = r - ry * R;
        const int x = gx0 + rx, y = gy0 + ry;
        const bool in = r < RR && x >= 0 && x < W && y >= 0 && y < H;
        px[j] = in ? x : -1; py[j] = y;
        nn[j] = cc[j] = dv[j] = 0.f;
        float gh = 0.f;
        if (in) {
            const int64_t i = base + (int64_t)y * W + x;
            nn[j] = n[i]; cc[j] = c[i]; dv[j] = s[i]; gh = grey[i];
        }
        if (r < RR) { s_d[0][R + r] = dv[j]; s_d[1][R + r] = gh; }   // plane 1 holds the grey guide until the weights are formed
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        gl[j] = gr[j] = gu[j] = gd[j] = 0.f;
        if (px[j] < 0) continue;
        const int r = R + tid + j * DP_THREADS;
        const float gh = s_d[1][r];
        if (px[j] > 0) gl[j] = rx_weight(k, gh, s_d[1][r - 1]);
        if (px[j] < W - 1) gr[j] = rx_weight(k, gh, s_d[1][r + 1]);
        if (py[j] > 0) gu[j] = rx_weight(k, gh, s_d[1][r - R]);
        if (py[j] < H - 1) gd[j] = rx_weight(k, gh, s_d[1][r + R]);
    }
    for (int it = 0; it < n_it; ++it) {
        __syncthreads();                                          // d of the previous iteration (or the load) is in plane it & 1
        const float* cur = s_d[it & 1];
        float* nxt = s_d[(it & 1) ^ 1];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (px[j] < 0) continue;
            const int r = R + tid + j * DP_THREADS;
            dv[j] = rx_update(k, dv[j], nn[j], cc[j], gl[j], gr[j], gu[j], gd[j], px[j] > 0, px[j] < W - 1, py[j] > 0, py[j] < H - 1,
                              cur[r - 1], cur[r + 1], cur[r - R], cur[r + R]);
            nxt[r] = dv[j];
        }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int r = tid + j * DP_THREADS, ry = r / R, rx = r - ry * R;
        if (px[j] < 0 || rx < K || rx >= K + T || ry < K || ry >= K + T) continue;
        d[base + (int64_t)py[j] * W + px[j]] = dv[j];
    }
}

// ---- host side ----
inline bool planes_ok(int32_t n, int32_t H, int32_t W) {
    return frame_dims_ok(n, H, W) && H <= 65535 * DP_BY && (int64_t)n * H * W <= 0x7fffffffLL;
}
inline dim3 pixel_grid(int32_t n, int32_t H, int32_t W) { return dim3((W + DP_BX - 1) / DP_BX, (H + DP_BY - 1) / DP_BY, n); }

inline int fused_pair_ok(int tile, int k) {
    return (tile == 32 && (k == 2 || k == 3 || k == 4 || k == 6)) || (tile == 16 && k == 2);
}

template <int T, int K>
void launch_fused(const RxParams& p, const float* n, const float* c, const float* grey, const float* s, float* d, int F, int H, int W,
                  int n_it, hipStream_t st) {
    const dim3 grid((W + T - 1) / T, (H + T - 1) / T, F);
    hipLaunchKernelGGL((relax_fused<T, K>), grid, dim3(DP_THREADS), 0, st, p, n, c, grey, s, d, H, W, n_it);
}

// `iters` iterations from state[0]; returns the slot that holds the result.  The arguments were checked by the caller.
int run_relax(const RxParams& p, const float* n, const float* c, const float* grey, float* const state[2], int F, int H, int W, int iters,
              int fused, int tile, int k, hipStream_t st) {
    int slot = 0;
    if (!fused) {
        for (int it = 0; it < iters; ++it, slot ^= 1)
            hipLaunchKernelGGL(relax_plain_kernel, pixel_grid(F, H, W), dim3(DP_THREADS), 0, st, p, n, c, grey, state[slot], state[slot ^ 1], H, W);
        return slot;
    }
    for (int done = 0; done < iters; done += k, slot ^= 1) {
        const int n_it = iters - done < k ? iters - done : k;
        const float* s = state[slot];
        float* d = state[slot ^ 1];
        if (tile == 32 && k == 2) launch_fused<32, 2>(p, n, c, grey, s, d, F, H, W, n_it, st);
        else if (tile == 32 && k == 3) launch_fused<32, 3>(p, n, c, grey, s, d, F, H, W, n_it, st);
        else if (tile == 32 && k == 4) launch_fused<32, 4>(p, n, c, grey, s, d, F, H, W, n_it, st);
        else if (tile == 32 && k == 6) launch_fused<32, 6>(p, n, c, grey, s, d, F, H, W, n_it, st);
        else launch_fused<16, 2>(p, n, c, grey, s, d, F, H, W, n_it, st);
    }
    return slot;
}
inline int relax_launches(int iters, int fused, int k) { return fused ? (iters + k - 1) / k : iters; }

// the route's checks, shared by nsff_disparity_relax and nsff_disparity_dense; tile / k come back resolved
int check_route(int32_t iters, int32_t fused, int32_t& tile, int32_t& k, float lambda, float sigma) {
    if (iters < 0 || iters > 100000 || (fused != 0 && fused != 1)) return NSFF_ERR_INVALID;
    if (!bounded_not_negative(lambda) || !bounded_positive(sigma)) return NSFF_ERR_INVALID;
    if (tile == 0 && k == 0) { tile = NSFF_DISPARITY_TILE; k = NSFF_DISPARITY_K; }
    if (fused && !fused_pair_ok(tile, k)) return NSFF_ERR_INVALID;
    return NSFF_OK;
}

constexpr int DP_MAX_LEVELS = 33;
struct Pyramid { int levels; int H[DP_MAX_LEVELS], W[DP_MAX_LEVELS]; int64_t offset[DP_MAX_LEVELS + 1]; };    // offsets in floats

// every level of F planes of H x W pixels down to 1 x 1, each padded to four floats
Pyramid pyramid_of(int64_t F, int H, int W) {
    Pyramid p;
    p.levels = 0; p.offset[0] = 0;
    for (;;) {
        const int l = p.levels;
        p.H[l] = H; p.W[l] = W;
        p.offset[l + 1] = p.offset[l] + ((F * H * W + 3) & ~(int64_t)3);
        p.levels = l + 1;
        if (H == 1 && W == 1) break;
        H = (H + 1) / 2; W = (W + 1) / 2;
    }
    return p;
}

void launch_push(const float* c, const float* n, const float* g, float* c2, float* n2, float* g2, int F, int H, int W, hipStream_t st) {
    const int h = (H + 1) / 2, w = (W + 1) / 2;
    hipLaunchKernelGGL(push_kernel, pixel_grid(F, h, w), dim3(DP_THREADS), 0, st, c, n, g, c2, n2, g2, H, W, h, w);
}
void launch_pull(const float* c, const float* n, const float* parent, float* d, int F, int H, int W, hipStream_t st) {
    hipLaunchKernelGGL(pull_kernel, pixel_grid(F, H, W), dim3(DP_THREADS), 0, st, c, n, parent, d, H, W, (H + 1) / 2, (W + 1) / 2);
}

}  // namespace

extern "C" int64_t nsff_disparity_sparse_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (!frame_dims_ok(n_frames, H, W)) return 0;
    return frame_scratch_bytes(n_frames, fin_blocks((int64_t)H * W), 1);
}

extern "C" int nsff_disparity_sparse(const NsffDisparitySparseArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if (!bounded_not_negative(a->min_parallax)) return NSFF_ERR_INVALID;
    if (!a->flow_fw || !a->flow_bw || !a->Pm || !a->n || !a->c) return NSFF_ERR_NULL;
    if (a->counts && !a->scratch) return NSFF_ERR_NULL;
    if (a->counts && a->scratch_bytes < nsff_disparity_sparse_scratch_bytes(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->counts) & 7) return NSFF_ERR_ALIGN;
    if (off4(a->Pm) || off4(a->n) || off4(a->c)) return NSFF_ERR_ALIGN;
    const int aligned = ((((uintptr_t)a->flow_fw | (uintptr_t)a->flow_bw | (uintptr_t)a->n | (uintptr_t)a->c) & 15) == 0) ? 1 : 0;
    const FrameScratch s = frame_scratch_split(a->counts ? a->scratch : nullptr, a->n_frames);
    const dim3 grid((unsigned)fin_blocks((int64_t)a->H * a->W), a->n_frames);
    hipLaunchKernelGGL(disparity_sparse_kernel, grid, dim3(FIN_THREADS), 0, (hipStream_t)stream, *a, a->min_parallax * a->min_parallax, aligned,
                       s.counters, s.partials);
    return nsff_launch_status();
}

extern "C" int nsff_disparity_push(const float* c, const float* n, const float* grey, float* c2, float* n2, float* grey2, int32_t n_frames,
                                   int32_t H, int32_t W, void* stream) {
    if (!planes_ok(n_frames, H, W) || (H == 1 && W == 1)) return NSFF_ERR_INVALID;
    if (!c || !n || !grey || !c2 || !n2 || !grey2) return NSFF_ERR_NULL;
    if (off4(c) || off4(n) || off4(grey) || off4(c2) || off4(n2) || off4(grey2)) return NSFF_ERR_ALIGN;
    launch_push(c, n, grey, c2, n2, grey2, n_frames, H, W, (hipStream_t)stream);
    return nsff_launch_status();
}

extern "C" int nsff_disparity_pull(const float* c, const float* n, const float* parent, float* d, int32_t n_frames, int32_t H, int32_t W,
                                   void* stream) {
    if (!planes_ok(n_frames, H, W)) return NSFF_ERR_INVALID;
    if ((c == nullptr) != (n == nullptr) || (!c && !parent)) return NSFF_ERR_INVALID;
    if (!d) return NSFF_ERR_NULL;
    if (off4(c) || off4(n) || off4(parent) || off4(d)) return NSFF_ERR_ALIGN;
    launch_pull(c, n, parent, d, n_frames, H, W, (hipStream_t)stream);
    return nsff_launch_status();
}

extern "C" int nsff_disparity_result_slot(int32_t iters, int32_t k) {
    if (iters < 0 || k < 1) return NSFF_ERR_INVALID;
    return ((iters + k - 1) / k) & 1;
}

extern "C" int nsff_disparity_relax(const NsffDisparityRelaxArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!planes_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    int32_t tile = a->tile, k = a->k;
    if (const int rc = check_route(a->iters, a->fused, tile, k, a->lambda, a->sigma)) return rc;
    if (!a->n || !a->c || !a->grey || !a->state[0] || !a->state[1]) return NSFF_ERR_NULL;
    if (a->state[0] == a->state[1]) return NSFF_ERR_INVALID;
    if (off4(a->n) || off4(a->c) || off4(a->grey) || off4(a->state[0]) || off4(a->state[1])) return NSFF_ERR_ALIGN;
    const RxParams p = {a->lambda, a->sigma};
    run_relax(p, a->n, a->c, a->grey, a->state, a->n_frames, a->H, a->W, a->iters, a->fused, tile, k, (hipStream_t)stream);
    return nsff_launch_status();
}

extern "C" int nsff_disparity_levels(int32_t H, int32_t W) {
    if (!planes_ok(1, H, W)) return 0;
    return pyramid_of(1, H, W).levels;
}

// the c, n and grey pyramids above the finest level and one plane of the finest level for d (the output is its other buffer)
extern "C" int64_t nsff_disparity_dense_scratch_bytes(int32_t n_frames, int32_t H, int32_t W) {
    if (!planes_ok(n_frames, H, W)) return 0;
    const Pyramid p = pyramid_of(n_frames, H, W);
    return (3 * (p.offset[p.levels] - p.offset[1]) + p.offset[1]) * (int64_t)sizeof(float);
}

extern "C" int nsff_disparity_dense(const NsffDisparityDenseArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!planes_ok(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    const Pyramid py = pyramid_of(a->n_frames, a->H, a->W);
    const int L = py.levels;
    if (a->levels < 1 || a->levels > L) return NSFF_ERR_INVALID;
    int32_t tile = a->tile, k = a->k;
    if (const int rc = check_route(a->iters, a->fused, tile, k, a->lambda, a->sigma)) return rc;
    if (!a->n || !a->c || !a->grey || !a->disps || !a->scratch) return NSFF_ERR_NULL;
    if (a->scratch_bytes < nsff_disparity_dense_scratch_bytes(a->n_frames, a->H, a->W)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->scratch & 15) return NSFF_ERR_ALIGN;
    if (off4(a->n) || off4(a->c) || off4(a->grey) || off4(a->disps)) return NSFF_ERR_ALIGN;

    hipStream_t st = (hipStream_t)stream;
    const int F = a->n_frames;
    const int64_t upper = py.offset[L] - py.offset[1];            // the floats of one pyramid above the finest level
    float* base = static_cast<float*>(a->scratch);
    // level l of the three pyramids: the caller's arrays at the finest level, the scratch above it
    auto level = [&](int which, int l) -> const float* {
        if (l == 0) return which == 0 ? a->c : (which == 1 ? a->n : a->grey);
        return base + which * upper + (py.offset[l] - py.offset[1]);
    };
    auto level_out = [&](int which, int l) -> float* { return base + which * upper + (py.offset[l] - py.offset[1]); };
    const RxParams p = {a->lambda, a->sigma};

    for (int l = 0; l + 1 < L; ++l)
        launch_push(level(0, l), level(1, l), level(2, l), level_out(0, l + 1), level_out(1, l + 1), level_out(2, l + 1), F, py.H[l], py.W[l], st);

    // d goes back and forth between the output and one scratch plane; the first buffer is chosen so that the last launch writes
    // the output: a pull or an upsampling is one flip, the relaxation of a level relax_launches() flips
    const int start = a->levels < L - 1 ? a->levels : L - 1;      // the coarsest level that is pulled down to
    int flips = (L - 1) - start + 1;
    for (int l = a->levels - 1; l >= 0; --l) flips += (l < L - 1 ? 1 : 0) + relax_launches(a->iters, a->fused, k);
    float* buf[2] = {a->disps, base + 3 * upper};
    int cur = (flips & 1) ^ 1;                                    // the buffer the next launch writes: the last one writes buf[0]
    const float* d = nullptr;
    for (int l = L - 1; l >= start; --l) {
        launch_pull(level(0, l), level(1, l), d, buf[cur], F, py.H[l], py.W[l], st);
        d = buf[cur]; cur ^= 1;
    }
    for (int l = a->levels - 1; l >= 0; --l) {
        if (l < L - 1) {
            launch_pull(nullptr, nullptr, d, buf[cur], F, py.H[l], py.W[l], st);
            d = buf[cur]; cur ^= 1;
        }
        float* const state[2] = {buf[cur ^ 1], buf[cur]};        // state[0] holds d
        const int slot = run_relax(p, level(1, l), level(0, l), level(2, l), state, F, py.H[l], py.W[l], a->iters, a->fused, tile, k, st);
        d = state[slot];
        if (slot) cur ^= 1;
    }
    return d == a->disps ? nsff_launch_status() : NSFF_ERR_INVALID;   // (by construction)
}
