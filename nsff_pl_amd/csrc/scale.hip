// The scene scale's per-point and per-pixel work: what the reference's nearest_depth loop (datasets/monocular.py:93-116) does per
// frame with numpy, for all frames at once -- see the header.  The O(F) arithmetic on the results (regression, percentile
// interpolation, the r^2 branch, the minimum) stays on the host.
//
//   scale_clear_kernel   zeroes the selection histograms and the frame tickets (a kernel, not a memset: see loss.hip)
//   scale_points_kernel  grid (ceil(N / 256), F): projects the visible points in fp64, writes the frame's row of the (F, N) depth
//                        array (+inf where a point is not visible: the depth selection needs no compaction) and `pix`, gathers
//                        the disparity and reduces (n, mean, M2) of x = 1 / depth and y = disparity: two passes inside the
//                        workgroup (sum -> mean -> centred sums), the workgroups' triples merged by the frame's last-arriving
//                        workgroup (frame_publish / frame_fold of nsff_frame_ops.h), so what is merged with what depends on N alone
//   scale_hist_kernel    one digit pass of an exact radix select in the scheme of loss.hip: order-preserving key, 8-bit digits,
//                        most significant first, wave-level LDS histograms added to the frame's global one with integer atomics.
//                        TWO ranks descend per population, each with its own prefix and histogram.  No kernel picks a digit: every
//                        wave of the next launch redoes the small prefix scan over the earlier passes' counters (sel_resolve).
//                        <float>: the frame's H * W disparities in the pixel quads of nsff_frame_ops.h, 4 passes of 32-bit keys;
//                        <double>: the frame's row of the depth array, 8 passes of 64-bit keys.
//   scale_finish_kernel  grid (F, 2): turns the final prefixes back into values; the disparities' NaN count.
//
// numpy's matmul is the BLAS's dgemm, whose dot products on FMA hardware are chains  fma(a_k, b_k, acc)  in k order starting from
// the rounded first product; the projection below is written as exactly those chains (explicit fma; the file is built
// uncontracted, so nothing else fuses) and the divisions are IEEE.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_frame_ops.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WORDS = 6;                        // a workgroup's partial: (n_vis | n_nonfinite), mean_x, mean_y, M2xx, M2xy, M2yy
constexpr int SC_RANKS = 2;
constexpr int SC_CHUNK = FIN_BLOCK_PX;             // elements a selection workgroup owns: 1024
constexpr double SC_Q = 0.05;                      // the 5th percentile of the visible depths

inline int64_t point_blocks(int64_t n_points) { return (n_points + SC_THREADS - 1) / SC_THREADS; }
inline int64_t chunk_blocks(int64_t n) { return (n + SC_CHUNK - 1) / SC_CHUNK; }

// ---- the workspace: [frame tickets + partials][disparity histograms][depth histograms][depth array] ----
struct ScaleWork {
    unsigned* counters; frame_word* partials;
    unsigned* hist_disp;                           // [F][2 ranks][4 passes][256]
    unsigned* hist_depth;                          // [F][2 ranks][8 passes][256]
    double* depth;                                 // [F][N]
    int64_t clear_words;                           // tickets .. end of the histograms, in uint32 (a multiple of 4)
};
inline int64_t hist_words(int64_t n_frames, int passes) { return n_frames * SC_RANKS * passes * 256; }
inline int64_t work_bytes(int64_t F, int64_t N) {
    return align16(frame_scratch_bytes(F, point_blocks(N), SC_WORDS)) + 4 * (hist_words(F, 4) + hist_words(F, 8)) + 8 * F * N;
}
inline ScaleWork work_split(void* work, int64_t F, int64_t N) {
    ScaleWork w;
    char* p = reinterpret_cast<char*>(work);
    const FrameScratch s = frame_scratch_split(work, (int32_t)F);
    w.counters = s.counters; w.partials = s.partials;
    p += align16(frame_scratch_bytes(F, point_blocks(N), SC_WORDS));
    w.hist_disp = reinterpret_cast<unsigned*>(p);
    w.hist_depth = w.hist_disp + hist_words(F, 4);
    w.depth = reinterpret_cast<double*>(w.hist_depth + hist_words(F, 8));
    w.clear_words = (reinterpret_cast<char*>(w.depth) - reinterpret_cast<char*>(work)) / 4;
    return w;
}

__global__ __launch_bounds__(256) void scale_clear_kernel(uint4* __restrict__ words, int64_t n_quads) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_quads) words[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- the point pass ----
struct Moments { double n, mx, my, xx, xy, yy; };
// Chan's merge of two (n, mean, M2) triples; an empty side leaves the other as it is
__device__ __forceinline__ Moments merge(const Moments& a, const Moments& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    Moments r;
    r.n = a.n + b.n;
    const double dx = b.mx - a.mx, dy = b.my - a.my, wb = b.n / r.n, wab = a.n * wb;
    r.mx = a.mx + dx * wb;
    r.my = a.my + dy * wb;
    r.xx = (a.xx + b.xx) + dx * dx * wab;
    r.xy = (a.xy + b.xy) + dx * dy * wab;
    r.yy = (a.yy + b.yy) + dy * dy * wab;
    return r;
}
// astype(int) is defined for these only: finite and inside the int64 range (false for NaN)
__device__ __forceinline__ bool castable(double v) { return fabs(v) < 9223372036854775808.0; }
__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(SC_THREADS) void scale_points_kernel(const NsffSceneScaleArgs a, const ScaleWork w) {
    __shared__ double s_sum[4][3];
    __shared__ unsigned s_cnt[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.y, N = a.n_points, i = (int64_t)blockIdx.x * SC_THREADS + tid;
    bool visible = false, ok = false;
    double x = 0.0, y = 0.0;
    if (i < N) {
        visible = a.vis[f * N + i] == 1;
        double depth = INFINITY;
        int32_t px = -1;
        if (visible) {
            const double* __restrict__ M = a.w2c + f * 12;
            const double p0 = a.points[3 * i], p1 = a.points[3 * i + 1], p2 = a.points[3 * i + 2];
            double c[3], uvd[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) c[r] = fma(M[4 * r + 2], p2, fma(M[4 * r + 1], p1, M[4 * r] * p0)) + M[4 * r + 3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                uvd[r] = fma((double)a.K[3 * r + 2], c[2], fma((double)a.K[3 * r + 1], c[1], (double)a.K[3 * r] * c[0]));
            const double u = uvd[0] / uvd[2], v = uvd[1] / uvd[2];
            depth = uvd[2];
            x = 1.0 / depth;
            ok = castable(u) && castable(v) && finite64(x);
            px = -2;
            if (ok) {                                             // astype(int) truncates toward zero; np.clip into the image
                const int64_t ui = (int64_t)fmin(fmax(trunc(u), 0.0), (double)(a.W - 1));
                const int64_t vi = (int64_t)fmin(fmax(trunc(v), 0.0), (double)(a.H - 1));
                px = (int32_t)(vi * a.W + ui);
                y = (double)a.disps[f * a.H * (int64_t)a.W + px];
            }
        }
        w.depth[f * N + i] = depth;
        if (a.pix) a.pix[f * N + i] = px;
    }
    // pass 1: the workgroup's counts and sums -> its means; pass 2: its centred sums
    const unsigned n_vis = wave_sum(visible ? 1u : 0u), n_bad = wave_sum(visible && !ok ? 1u : 0u);
    const double sx = wave_sum(ok ? x : 0.0), sy = wave_sum(ok ? y : 0.0);
    if (lane == 0) { s_cnt[wave][0] = n_vis; s_cnt[wave][1] = n_bad; s_sum[wave][0] = sx; s_sum[wave][1] = sy; }
    __syncthreads();
    const unsigned bn_vis = sum4(s_cnt, 0), bn_bad = sum4(s_cnt, 1);
    Moments m;
    m.n = (double)(bn_vis - bn_bad);
    m.mx = m.n > 0.0 ? sum4(s_sum, 0) / m.n : 0.0;
    m.my = m.n > 0.0 ? sum4(s_sum, 1) / m.n : 0.0;
    __syncthreads();
    const double dx = ok ? x - m.mx : 0.0, dy = ok ? y - m.my : 0.0;
    const double xx = wave_sum(dx * dx), xy = wave_sum(dx * dy), yy = wave_sum(dy * dy);
    if (lane == 0) { s_sum[wave][0] = xx; s_sum[wave][1] = xy; s_sum[wave][2] = yy; }
    __syncthreads();
    if (wave != 0) return;
    m.xx = sum4(s_sum, 0); m.xy = sum4(s_sum, 1); m.yy = sum4(s_sum, 2);

    const unsigned n_blocks = gridDim.x;
    frame_word* fp = w.partials + f * n_blocks * SC_WORDS;
    const frame_word mine[SC_WORDS] = {pack2(bn_vis, bn_bad), pack_double(m.mx), pack_double(m.my), pack_double(m.xx),
                                       pack_double(m.xy), pack_double(m.yy)};
    if (!frame_publish(fp, w.counters + f, blockIdx.x, n_blocks, lane, mine)) return;
    Moments t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long t_vis = 0, t_bad = 0;
    frame_fold<SC_WORDS>(fp, n_blocks, lane, [&](const frame_word (&q)[SC_WORDS]) {
        const unsigned v = word_lo(q[0]), b = word_hi(q[0]);
        t_vis += v; t_bad += b;
        const Moments o = {(double)(v - b), word_double(q[1]), word_double(q[2]), word_double(q[3]), word_double(q[4]), word_double(q[5])};
        t = merge(t, o);
    });
    t_vis = wave_sum(t_vis); t_bad = wave_sum(t_bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                            // the lower lane of a pair is always the left operand
        Moments p;
        p.n = __shfl_xor(t.n, o); p.mx = __shfl_xor(t.mx, o); p.my = __shfl_xor(t.my, o);
        p.xx = __shfl_xor(t.xx, o); p.xy = __shfl_xor(t.xy, o); p.yy = __shfl_xor(t.yy, o);
        t = (lane & o) ? merge(p, t) : merge(t, p);
    }
    if (lane == 0) {
        double* s = a.stats + f * 8;
        s[0] = (double)t_vis; s[1] = (double)t_bad; s[2] = t.mx; s[3] = t.my; s[4] = t.xx; s[5] = t.xy; s[6] = t.yy;
        frame_counter_reset(w.counters + f);
    }
}

// ---- the selections ----
template <class T> struct Key;
template <> struct Key<float> {
    typedef uint32_t type;
    static constexpr int PASSES = 4;
    __device__ static __forceinline__ uint32_t of(float x) {      // ascending; -0 == +0
        if (x == 0.f) x = 0.f;
        const uint32_t u = __float_as_uint(x);
        return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    }
    __device__ static __forceinline__ float value(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
};
template <> struct Key<double> {
    typedef uint64_t type;
    static constexpr int PASSES = 8;
    __device__ static __forceinline__ uint64_t of(double x) {
        if (x == 0.0) x = 0.0;
        const uint64_t u = (uint64_t)__double_as_longlong(x);
        return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
    }
    __device__ static __forceinline__ double value(uint64_t k) {
        return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull)));
    }
};

// the two depth ranks of a frame with n_vis visible points: numpy's method='linear' virtual index (n - 1) q, its floor and the
// next index
__device__ __forceinline__ void depth_ranks(double n_vis, long long (&rank)[SC_RANKS]) {
    const long long n = (long long)n_vis;
    const long long lo = n > 0 ? (long long)floor((double)(n - 1) * SC_Q) : 0;
    rank[0] = lo;
    rank[1] = n > 0 ? min(lo + 1, n - 1) : 0;
}

template <class K>
struct SelState {
    K prefix;              // the digits found so far
    long long rem;         // rank still to descend inside the prefix
    long long total;       // ranked population (pass 0's histogram total)
    bool live;             // the rank lies inside the population
};
// What passes 0 .. npass-1 found for one rank, from their histograms hist[pass][256].  Called by whole waves; every lane returns
// the same state.  (loss.hip's sel_resolve, for either key width.)
template <class K>
__device__ __forceinline__ SelState<K> sel_resolve(const unsigned* hist, int npass, long long rank) {
    const int lane = threadIdx.x & 63;
    SelState<K> s; s.prefix = 0; s.rem = rank; s.total = 0; s.live = true;
    for (int p = 0; p < npass; ++p) {
        const uint4 q = *reinterpret_cast<const uint4*>(hist + p * 256 + lane * 4);
        const long long c[4] = {(long long)q.x, (long long)q.y, (long long)q.z, (long long)q.w};
        const long long tot = c[0] + c[1] + c[2] + c[3];
        long long incl = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const long long t = __shfl_up(incl, off); if (lane >= off) incl += t; }
        if (p == 0) {
            s.total = __shfl(incl, 63);
            if (rank < 0 || rank >= s.total) { s.live = false; return s; }
        }
        long long run = incl - tot, nr = 0;
        int d = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (d < 0 && s.rem >= run && s.rem < run + c[j]) { d = lane * 4 + j; nr = s.rem - run; }
            run += c[j];
        }
        const unsigned long long hit = __ballot(d >= 0);
        const int from = hit != 0ull ? (int)__builtin_ctzll(hit) : 0;
        d = __shfl(d, from); nr = __shfl(nr, from);
        s.prefix = (K)((s.prefix << 8) | (K)(d & 255));
        s.rem = nr;
    }
    return s;
}

// the ranks of frame f for either population
template <class T>
__device__ __forceinline__ void sel_ranks(const NsffSceneScaleArgs& a, int64_t f, long long (&rank)[SC_RANKS]);
template <>
__device__ __forceinline__ void sel_ranks<float>(const NsffSceneScaleArgs& a, int64_t, long long (&rank)[SC_RANKS]) {
    rank[0] = a.disp_rank[0]; rank[1] = a.disp_rank[1];
}
template <>
__device__ __forceinline__ void sel_ranks<double>(const NsffSceneScaleArgs& a, int64_t f, long long (&rank)[SC_RANKS]) {
    depth_ranks(*(const volatile double*)(a.stats + f * 8), rank);            // n_vis, written by the point pass's launch
}

// digit pass p; grid (chunks, F).  hist: the population's [F][2][PASSES][256]
template <class T>
__global__ __launch_bounds__(SC_THREADS) void scale_hist_kernel(const NsffSceneScaleArgs a, const T* __restrict__ src, unsigned* hist,
                                                                const int64_t n, const int p, const int aligned) {
    typedef typename Key<T>::type K;
    constexpr int PASSES = Key<T>::PASSES;
    __shared__ unsigned sH[4][SC_RANKS][256];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int64_t f = blockIdx.y;
    hist += f * SC_RANKS * PASSES * 256;
    long long rank[SC_RANKS];
    sel_ranks<T>(a, f, rank);
    SelState<K> s[SC_RANKS];
#pragma unroll
    for (int r = 0; r < SC_RANKS; ++r) s[r] = sel_resolve<K>(hist + r * PASSES * 256, p, rank[r]);
    if (p > 0 && !s[0].live && !s[1].live) return;
    for (int j = tid; j < 4 * SC_RANKS * 256; j += SC_THREADS) (&sH[0][0][0])[j] = 0u;
    __syncthreads();
    const int shift = 8 * (PASSES - 1 - p);
    // a lane's four consecutive elements (nsff_frame_ops.h's quads: wide loads where the flat index allows)
    const Quad q = quad_of(blockIdx.x, tid, f, n, aligned);
    T v[FIN_PX];
    if (q.vec) {
        if constexpr (sizeof(T) == 4) {
            const float4 t = *reinterpret_cast<const float4*>(src + q.q0);
            v[0] = (T)t.x; v[1] = (T)t.y; v[2] = (T)t.z; v[3] = (T)t.w;
        } else {
            const double2 t0 = *reinterpret_cast<const double2*>(src + q.q0), t1 = *reinterpret_cast<const double2*>(src + q.q0 + 2);
            v[0] = (T)t0.x; v[1] = (T)t0.y; v[2] = (T)t1.x; v[3] = (T)t1.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < FIN_PX; ++i) v[i] = i < q.n ? src[q.q0 + i] : (T)0;
    }
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        if (i >= q.n) continue;
        if (sizeof(T) == 4 && v[i] != v[i]) continue;             // a disparity NaN is counted (pass 0's total), not ranked
        const K key = Key<T>::of(v[i]);
        const unsigned digit = (unsigned)(key >> shift) & 255u;
#pragma unroll
        for (int r = 0; r < SC_RANKS; ++r)
            if (p == 0 || (s[r].live && (key >> shift >> 8) == s[r].prefix)) atomicAdd(&sH[wave][r][digit], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SC_RANKS; ++r) {
        const unsigned t = sH[0][r][tid] + sH[1][r][tid] + sH[2][r][tid] + sH[3][r][tid];
        if (t != 0u) atomicAdd(hist + (r * PASSES + p) * 256 + tid, t);
    }
}

// grid (F, 2), one wave: y = 0 the disparities' two order statistics and NaN count, y = 1 the depths'
__global__ __launch_bounds__(64) void scale_finish_kernel(const NsffSceneScaleArgs a, const ScaleWork w) {
    const int64_t f = blockIdx.x;
    const int lane = threadIdx.x;
    long long rank[SC_RANKS];
    if (blockIdx.y == 0) {
        sel_ranks<float>(a, f, rank);
        const unsigned* hist = w.hist_disp + f * SC_RANKS * 4 * 256;
#pragma unroll
        for (int r = 0; r < SC_RANKS; ++r) {
            const SelState<uint32_t> s = sel_resolve<uint32_t>(hist + r * 4 * 256, 4, rank[r]);
            if (lane == 0) {
                a.disp_os[f * 2 + r] = s.live ? Key<float>::value(s.prefix) : __uint_as_float(0x7fc00000u);
                if (r == 0) a.stats[f * 8 + 7] = (double)((long long)a.H * a.W - s.total);
            }
        }
    } else {
        sel_ranks<double>(a, f, rank);
        const unsigned* hist = w.hist_depth + f * SC_RANKS * 8 * 256;
#pragma unroll
        for (int r = 0; r < SC_RANKS; ++r) {
            const SelState<uint64_t> s = sel_resolve<uint64_t>(hist + r * 8 * 256, 8, rank[r]);
            if (lane == 0) a.depth_os[f * 2 + r] = s.live ? Key<double>::value(s.prefix) : (double)INFINITY;
        }
    }
}

}  // namespace

extern "C" int64_t nsff_scene_scale_work_bytes(int32_t n_frames, int32_t n_points, int32_t H, int32_t W) {
    return frame_dims_ok(n_frames, H, W) && n_points >= 1 ? work_bytes(n_frames, n_points) : 0;
}

extern "C" int nsff_scene_scale(const NsffSceneScaleArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(a->n_frames, a->H, a->W) || a->n_points < 1) return NSFF_ERR_INVALID;
    const int64_t HW = (int64_t)a->H * a->W, F = a->n_frames, N = a->n_points;
    for (int r = 0; r < SC_RANKS; ++r)
        if (a->disp_rank[r] < 0 || a->disp_rank[r] >= HW) return NSFF_ERR_INVALID;
    if (!a->points || !a->vis || !a->w2c || !a->K || !a->disps || !a->stats || !a->disp_os || !a->depth_os || !a->work) return NSFF_ERR_NULL;
    if (a->work_bytes < work_bytes(F, N)) return NSFF_ERR_INVALID;
    if ((uintptr_t)a->work & 15) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->points | (uintptr_t)a->w2c | (uintptr_t)a->stats | (uintptr_t)a->depth_os) & 7) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->K | (uintptr_t)a->disps | (uintptr_t)a->disp_os | (uintptr_t)a->pix) & 3) return NSFF_ERR_ALIGN;
    const ScaleWork w = work_split(a->work, F, N);
    hipStream_t st = (hipStream_t)stream;
    const int64_t quads = w.clear_words / 4;
    hipLaunchKernelGGL(scale_clear_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, reinterpret_cast<uint4*>(a->work), quads);
    hipLaunchKernelGGL(scale_points_kernel, dim3((unsigned)point_blocks(N), (unsigned)F), dim3(SC_THREADS), 0, st, *a, w);
    const dim3 gp((unsigned)chunk_blocks(HW), (unsigned)F), gd((unsigned)chunk_blocks(N), (unsigned)F);
    const int disp_aligned = ((uintptr_t)a->disps & 15) == 0;     // (the depth array starts 16-byte aligned in the workspace)
    for (int p = 0; p < 4; ++p)
        hipLaunchKernelGGL(scale_hist_kernel<float>, gp, dim3(SC_THREADS), 0, st, *a, a->disps, w.hist_disp, HW, p, disp_aligned);
    for (int p = 0; p < 8; ++p)
        hipLaunchKernelGGL(scale_hist_kernel<double>, gd, dim3(SC_THREADS), 0, st, *a, (const double*)w.depth, w.hist_depth, N, p, 1);
    hipLaunchKernelGGL(scale_finish_kernel, dim3((unsigned)F, 2), dim3(64), 0, st, *a, w);
    return nsff_launch_status();
}
