// The per-frame reduction and the pixel-quad layer of the image kernels of metrics.hip (SSIM), frames.hip and flow.hip; everything
// here is per translation unit (the library is not built with -fgpu-rdc).
//
// The reduction.  A frame's workgroups each reduce their share in a fixed order (wave_* butterflies, then sum4 / min4 / max4 over
// the four waves' values in LDS), and wave 0 hands the result to frame_publish as WORDS 8-byte words.  The frame's last-arriving
// workgroup (by ticket on the frame's counter) folds all the partials -- frame_fold, then the same butterflies -- writes the
// outputs and returns the counter to zero.  What is added to what depends on the frame's block count alone, so a frame's numbers
// are the same bits alone or in a batch.  Scratch: [n_frames uint32 counters, padded to 16 B][n_frames x blocks x WORDS words].
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include <cmath>

namespace {

typedef unsigned long long frame_word;

// ---- (a) fixed-order workgroup reduction: butterfly within a wave (offsets 32 down to 1), then the four waves in order ----
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
__device__ __forceinline__ float wave_min(float v) { return wave_reduce(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_max(float v) { return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); }); }
// s[wave][i] of a 256-thread workgroup
template <class T, int N>
__device__ __forceinline__ T sum4(const T (&s)[4][N], int i) { return ((s[0][i] + s[1][i]) + s[2][i]) + s[3][i]; }
template <int N>
__device__ __forceinline__ float min4(const float (&s)[4][N], int i) { return fminf(fminf(s[0][i], s[1][i]), fminf(s[2][i], s[3][i])); }
template <int N>
__device__ __forceinline__ float max4(const float (&s)[4][N], int i) { return fmaxf(fmaxf(s[0][i], s[1][i]), fmaxf(s[2][i], s[3][i])); }

// ---- (b) the ticketed per-frame reduction ----
__device__ __forceinline__ frame_word pack2(float lo, float hi) { return (frame_word)__float_as_uint(lo) | ((frame_word)__float_as_uint(hi) << 32); }
__device__ __forceinline__ frame_word pack2(uint32_t lo, uint32_t hi) { return (frame_word)lo | ((frame_word)hi << 32); }
__device__ __forceinline__ frame_word pack_double(double x) { return (frame_word)__double_as_longlong(x); }
__device__ __forceinline__ uint32_t word_lo(frame_word w) { return (uint32_t)w; }
__device__ __forceinline__ uint32_t word_hi(frame_word w) { return (uint32_t)(w >> 32); }
__device__ __forceinline__ float word_lo_f(frame_word w) { return __uint_as_float(word_lo(w)); }
__device__ __forceinline__ float word_hi_f(frame_word w) { return __uint_as_float(word_hi(w)); }
__device__ __forceinline__ double word_double(frame_word w) { return __longlong_as_double((long long)w); }

// Wave 0 of workgroup `block` of frame f, converged: publish w (lane 0's) as the block's partial and take a ticket.  True, in
// every lane, in the frame's last-arriving workgroup, which may then read every partial of the frame.
// The frame's workgroups may run on any XCD.  The words go out as agent-scope atomic stores -- write-through, so no release
// fence: a fence per workgroup writes back every dirty line of its L2, the image being stored included, and 14 400 of them took
// 0.9 of the 1.0 ms a 100-frame nsff_frame_finish then cost -- and are drained before the ticket; the last workgroup acquires.
template <int WORDS>
__device__ __forceinline__ bool frame_publish(frame_word* __restrict__ frame_partials, unsigned* __restrict__ counter, unsigned block,
                                              unsigned n_blocks, int lane, const frame_word (&w)[WORDS]) {
    unsigned ticket = 0;
    if (lane == 0) {
        frame_word* slot = frame_partials + (int64_t)block * WORDS;
#pragma unroll
        for (int i = 0; i < WORDS; ++i) __hip_atomic_store(slot + i, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ticket = __shfl(ticket, 0);
    if (ticket != n_blocks - 1) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return true;
}

// the last workgroup's wave 0: lane l hands add(w) the words of blocks l, l + 64, ... in order
template <int WORDS, class Add>
__device__ __forceinline__ void frame_fold(const frame_word* frame_partials, unsigned n_blocks, int lane, Add add) {
    for (unsigned b = lane; b < n_blocks; b += 64) {
        const volatile frame_word* p = frame_partials + (int64_t)b * WORDS;
        frame_word w[WORDS];
#pragma unroll
        for (int i = 0; i < WORDS; ++i) w[i] = p[i];
        add(w);
    }
}

// by one lane, after the frame's outputs: ready for the next launch
__device__ __forceinline__ void frame_counter_reset(unsigned* counter) { __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The whole tail of a kernel that counts N uint32 values per frame, called by every thread of a workgroup of frame f -- of THREADS
// threads, the constant of the kernel's __launch_bounds__ and of its launch, which must be the four waves that sum4 adds --
// (grid.x the frame's workgroups, which hold (N + 1) / 2 words each in `partials`): cnt summed over the workgroup, two counts to a
// word ({c0, c1}, {c2, 0}), published; the frame's last workgroup folds them in block order into out[f * N ..] as int64, returns the
// partials it read to zero -- the scratch is all zero between calls -- and resets the frame's counter.
template <int N, int THREADS>
__device__ __forceinline__ void frame_count_finish(const uint32_t (&cnt)[N], int64_t* __restrict__ out, unsigned* __restrict__ counters,
                                                   frame_word* __restrict__ partials, int64_t f) {
    static_assert(THREADS == 4 * 64, "frame_count_finish adds the counts of four waves (sum4)");
    constexpr int WORDS = (N + 1) / 2;
    __shared__ uint32_t s_cnt[THREADS / 64][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c[N];
#pragma unroll
    for (int k = 0; k < N; ++k) c[k] = wave_sum(cnt[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_cnt[wave][k] = c[k];
    }
    __syncthreads();
    if (wave != 0) return;
    const unsigned n_blocks = gridDim.x;
    frame_word* fp = partials + f * n_blocks * WORDS;
    uint32_t tot[2 * WORDS] = {};
#pragma unroll
    for (int k = 0; k < N; ++k) tot[k] = sum4(s_cnt, k);
    frame_word mine[WORDS];
#pragma unroll
    for (int i = 0; i < WORDS; ++i) mine[i] = pack2(tot[2 * i], tot[2 * i + 1]);
    if (!frame_publish(fp, counters + f, blockIdx.x, n_blocks, lane, mine)) return;
    long long n[N];
#pragma unroll
    for (int k = 0; k < N; ++k) n[k] = 0;
    frame_fold<WORDS>(fp, n_blocks, lane, [&](const frame_word (&w)[WORDS]) {
#pragma unroll
        for (int k = 0; k < N; ++k) n[k] += (long long)((k & 1) ? word_hi(w[k / 2]) : word_lo(w[k / 2]));
    });
    for (unsigned b = lane; b < n_blocks; b += 64)                // what this lane read goes back to zero
#pragma unroll
        for (int i = 0; i < WORDS; ++i) fp[(int64_t)b * WORDS + i] = 0ull;
#pragma unroll
    for (int k = 0; k < N; ++k) n[k] = wave_sum(n[k]);
    if (lane == 0) {
        for (int k = 0; k < N; ++k) out[f * N + k] = (int64_t)n[k];
        frame_counter_reset(counters + f);
    }
}

// ---- (c) host side: argument checks, frame limits and the scratch layout ----
inline bool off4(const void* p) { return ((uintptr_t)p & 3) != 0; }
// n bytes from a and n bytes from b share a byte
inline bool overlap(const void* a, const void* b, int64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)n && y < x + (uintptr_t)n;
}
// neither negative nor NaN; +inf passes (a threshold nothing exceeds)
inline bool not_negative(float v) { return v >= 0.f; }
// a parameter that is squared or divided by: no NaN, and small enough to stay finite
inline bool bounded_not_negative(float v) { return v >= 0.f && v <= 3.0e38f; }
inline bool bounded_positive(float v) { return v > 0.f && v <= 3.0e38f; }
inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }
// grid.y = frame; pixel indices within a frame are ints
inline bool frame_dims_ok(int32_t n_frames, int32_t H, int32_t W) {
    return n_frames >= 1 && n_frames <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff;
}
inline int64_t frame_scratch_bytes(int64_t n_frames, int64_t blocks_per_frame, int words) {
    return align16(4 * n_frames) + 8 * (int64_t)words * n_frames * blocks_per_frame;
}
struct FrameScratch { unsigned* counters; frame_word* partials; };
inline FrameScratch frame_scratch_split(void* scratch, int32_t n_frames) {      // (NULL stays NULL: a call that reduces nothing)
    if (!scratch) return {nullptr, nullptr};
    return {reinterpret_cast<unsigned*>(scratch), reinterpret_cast<frame_word*>(reinterpret_cast<char*>(scratch) + align16(4 * (int64_t)n_frames))};
}

// ---- the pixel quads: a workgroup owns 1024 consecutive pixels OF ONE FRAME (grid.y = frame) and a lane four consecutive ones.
// A lane moves its four pixels as 16-byte loads and dword stores where its first pixel's FLAT index (frame * H * W + pixel) is a
// multiple of four -- then every address is aligned (48, 16, 12 and 4 bytes per four pixels), given 16-byte aligned fp32 and
// 4-byte aligned uint8 arrays (`aligned`) -- and element by element otherwise (frames whose base is not a multiple of four
// pixels, i.e. odd H * W, and each frame's last partial quad). ----
constexpr int FIN_THREADS = 256, FIN_PX = 4, FIN_BLOCK_PX = FIN_THREADS * FIN_PX;
inline int64_t fin_blocks(int64_t n_pixels) { return (n_pixels + FIN_BLOCK_PX - 1) / FIN_BLOCK_PX; }

struct Quad {
    int64_t p0, q0;                                               // the lane's first pixel: in its frame, and flat
    int n;                                                        // its pixels: 4, a ragged 1..3, or none
    bool vec;
};
__device__ __forceinline__ Quad quad_of(unsigned block, int tid, int64_t f, int64_t HW, int aligned) {
    Quad q;
    q.p0 = ((int64_t)block * FIN_THREADS + tid) * FIN_PX;
    q.n = (int)min((int64_t)FIN_PX, max(HW - q.p0, (int64_t)0));
    q.q0 = f * HW + q.p0;
    q.vec = aligned && q.n == FIN_PX && (q.q0 & 3) == 0;
    return q;
}

// four pixels of C channels each; a NULL array reads as 0
template <int C>
__device__ __forceinline__ void load_px(const float* __restrict__ src, const Quad& q, float (&v)[C * FIN_PX]) {
#pragma unroll
    for (int i = 0; i < C * FIN_PX; ++i) v[i] = 0.f;
    if (!src) return;
    if (q.vec) {
        const float4* S = reinterpret_cast<const float4*>(src + q.q0 * C);
#pragma unroll
        for (int w = 0; w < C; ++w) { const float4 t = S[w]; v[4 * w] = t.x; v[4 * w + 1] = t.y; v[4 * w + 2] = t.z; v[4 * w + 3] = t.w; }
    } else {
#pragma unroll
        for (int i = 0; i < C * FIN_PX; ++i)
            if (i / C < q.n) v[i] = src[q.q0 * C + i];
    }
}
template <int C>
__device__ __forceinline__ void store_px(float* __restrict__ dst, const Quad& q, const float (&v)[C * FIN_PX]) {
    float* o = dst + q.q0 * C;
    if (q.vec) {
        float4* O = reinterpret_cast<float4*>(o);
#pragma unroll
        for (int w = 0; w < C; ++w) O[w] = make_float4(v[4 * w], v[4 * w + 1], v[4 * w + 2], v[4 * w + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < C * FIN_PX; ++i)
            if (i / C < q.n) o[i] = v[i];
    }
}
// NB byte values, one per element of b: dwords where vec (all NB bytes, dst 4-byte aligned), else the first n_bytes singly
template <int NB>
__device__ __forceinline__ void store_bytes(uint8_t* dst, const uint32_t (&b)[NB], int n_bytes, bool vec) {
    if (vec) {
        uint32_t* o = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int w = 0; w < NB / 4; ++w) o[w] = b[4 * w] | (b[4 * w + 1] << 8) | (b[4 * w + 2] << 16) | (b[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (i < n_bytes) dst[i] = (uint8_t)b[i];
    }
}

// An NDC point seen by the camera M (3, 4 row-major, world -> pixel): the geometric loss's chain (losses.py:99-116), every step one
// fp32 operation in a translation unit built -ffp-contract=off (flow.hip, tracks.hip):
//   world  Rz = 2 / ((z - 1) - 1e-6f), Rx = (((-Rz) * x) * cx) / fx, Ry = (((-Rz) * y) * cy) / fy               (ray_utils.py:142-145)
//   uvd_r  = ((M[r][0] * Rx + M[r][1] * Ry) + M[r][2] * Rz) + M[r][3],  u = uvd.x / (|uvd.z| + 1e-8f), v likewise
// Returns uvd.z: the point is in front of the camera when it is > 0 (a NaN point fails that comparison).
__device__ __forceinline__ float ndc_to_pixel(float x, float y, float z, const float* M, float fx, float fy, float cx, float cy,
                                              float& u, float& v) {
    const float Rz = 2.f / ((z - 1.f) - 1e-6f);
    const float Rx = (((-Rz) * x) * cx) / fx;
    const float Ry = (((-Rz) * y) * cy) / fy;
    const float ud = ((M[0] * Rx + M[1] * Ry) + M[2] * Rz) + M[3];
    const float vd = ((M[4] * Rx + M[5] * Ry) + M[6] * Rz) + M[7];
    const float wd = ((M[8] * Rx + M[9] * Ry) + M[10] * Rz) + M[11];
    const float den = fabsf(wd) + 1e-8f;
    u = ud / den;
    v = vd / den;
    return wd;
}

// np.nan_to_num of an fp32 value: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float nan_to_num(float x) { return x != x ? 0.f : fminf(fmaxf(x, -FLT_MAX), FLT_MAX); }
// torch.clip(x, 0, 1): a NaN stays a NaN
__device__ __forceinline__ float clip01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }
// astype(np.uint8) of a value in [0, 255]: truncation toward zero; a NaN (numpy: undefined) gives 0
__device__ __forceinline__ uint32_t trunc_u8(float v) { return v == v ? (uint32_t)(int)fminf(fmaxf(v, 0.f), 255.f) : 0u; }
// visualize_depth's 8-bit index (utils/visualization.py:10-15), span = (ma - mi) + 1e-8f: every step one fp32 operation, as numpy
// rounds it, with an IEEE division
__device__ __forceinline__ uint32_t depth_index(float x, float mi, float span) { return trunc_u8(255.f * ((x - mi) / span)); }
// entry i of a (256, 3) colour table as r | g << 8 | b << 16
__device__ __forceinline__ uint32_t lut_rgb(const uint8_t* lut, uint32_t i) { return lut[3 * i] | (lut[3 * i + 1] << 8) | (lut[3 * i + 2] << 16); }

}  // namespace
