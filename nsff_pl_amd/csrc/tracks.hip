// Chained scene-flow tracks: a point at time t followed through the trained flow field to t + 1, t + 2, ... (forward head) or
// t - 1, t - 2, ... (backward head), and motion trails of the projected tracks drawn on an 8-bit frame (nsff_pl_amd/tracks.py).
//
// nsff_track_step -- one launch per step over the R * S points of R rows (the S points of a row share a time, as the samples of a
// ray do).  Per point p of row r, with x = xyz_in[p], t = t_in[r]:
//   can    = raw given && alive_in[r] && (t < max_t forward, t > 0 backward)
//   f      = columns 8..10 (forward) / 11..13 (backward) of the point's raw field record, read in place;
//            0 where (x.z + 1f) * 0.5f > 0.95f -- the reference's  flows[zs > z_far] = 0  (rendering.py:126,187-188) restated on the
//            point: on NDC rays o_z = -1, d_z = 2, so zs = (z + 1) / 2 -- and 0 without records
//   x'     = can ? x + f : x;  t' = can ? t +- 1 : t;  alive' = can
// x' goes to xyz_out, t' / alive' to t_out / alive_out once per row (by the lane that holds the row's first point).  With
// cameras, x' is projected by the camera of ITS time t' (Ps[t'], or the one fixed view) through ndc_to_pixel (nsff_frame_ops.h:
// the chain nsff_flow_maps runs; this file is built -ffp-contract=off like flow.hip): uv = (1e10, 1e10) where the point is not in
// front of the camera, depth = uvd.z.  Without records (raw NULL) nothing moves and no state is written: that is the projection
// of slab 0, so there is one code path.
// The kernel is memory-bound.  A lane owns four consecutive points: 48 bytes of positions in and out, 32 of uv, 16 of depth --
// 16-byte loads and stores where the lane's first element is 16-byte aligned, dwords otherwise (slab j of a path starts
// j * R * S * 12 bytes in: off 16 bytes whenever R * S is no multiple of 4, which odd S brings about; the ragged last lane
// too) -- and of each 64-byte record the one aligned 16-byte (forward) or the 4 + 8 bytes (backward) that hold the flow.
//
// nsff_track_draw -- three launches: clear the H * W uint32 canvas; one lane per (segment j, track q) walks its line and
// atomicMax-es the key ((j + 1) << 20) | q into the pixels it visits; the resolve pass writes lut[(255 * (j + 1)) / n] where a key
// is set and the source pixel elsewhere.  The largest key wins whatever order the lanes run in: the image is deterministic.
// Segment j of track q runs from uv[j][q] to uv[j + 1][q] and is drawn when both ends are ok, finite, known (|u|, |v| <= 1e7 is
// implied by) |u|, |v| < 32768, and max(|dx|, |dy|) <= H + W after rounding the ends with floor(u + 0.5f).
// The line rule, all in integers: N = max(|dx|, |dy|); pixel i = 0 .. N is
//   (x0 + floor((2 i dx + N) / (2 N)), y0 + floor((2 i dy + N) / (2 N)))       (N = 0: the one pixel (x0, y0))
// i.e. the major axis advances by one per pixel and the minor axis is the exact position rounded half up.  It visits N + 1
// pixels, both ends included (i = 0 gives floor(1 / 2) = 0, i = N gives dx + floor(1 / 2)); successive pixels differ by at most
// one in each coordinate (|dx|, |dy| <= N), so the line is 8-connected.  Off-image pixels are skipped one by one.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_frame_ops.h"

namespace {

constexpr int TRK_THREADS = 256, TRK_PTS = 4;
constexpr float TRK_Z_FAR = 0.95f;

// n (1..4) points of C floats each from / to p: one 16-byte access per four floats where p is 16-byte aligned and n == 4
template <int C>
__device__ __forceinline__ void load_pts(const float* __restrict__ p, int n, float (&v)[C * TRK_PTS]) {
    if (n == TRK_PTS && ((uintptr_t)p & 15) == 0) {
        const float4* s = reinterpret_cast<const float4*>(p);
#pragma unroll
        for (int w = 0; w < C; ++w) { const float4 t = s[w]; v[4 * w] = t.x; v[4 * w + 1] = t.y; v[4 * w + 2] = t.z; v[4 * w + 3] = t.w; }
    } else {
#pragma unroll
        for (int i = 0; i < C * TRK_PTS; ++i) v[i] = i / C < n ? p[i] : 0.f;
    }
}
template <int C>
__device__ __forceinline__ void store_pts(float* __restrict__ p, int n, const float (&v)[C * TRK_PTS]) {
    if (n == TRK_PTS && ((uintptr_t)p & 15) == 0) {
        float4* o = reinterpret_cast<float4*>(p);
#pragma unroll
        for (int w = 0; w < C; ++w) o[w] = make_float4(v[4 * w], v[4 * w + 1], v[4 * w + 2], v[4 * w + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < C * TRK_PTS; ++i)
            if (i / C < n) p[i] = v[i];
    }
}

__global__ __launch_bounds__(TRK_THREADS) void track_step_kernel(NsffTrackStepArgs a) {
    const int64_t n_points = a.n_rows * a.pts_per_row;
    const int64_t p0 = ((int64_t)blockIdx.x * TRK_THREADS + threadIdx.x) * TRK_PTS;
    if (p0 >= n_points) return;
    const int n = (int)min((int64_t)TRK_PTS, n_points - p0);
    float x[3 * TRK_PTS], uv[2 * TRK_PTS], depth[TRK_PTS];
    load_pts<3>(a.xyz_in + p0 * 3, n, x);
    int64_t row = p0 / a.pts_per_row;
    int rem = (int)(p0 - row * a.pts_per_row);
    const bool project = a.uv != nullptr;
#pragma unroll
    for (int i = 0; i < TRK_PTS; ++i) {
        uv[2 * i] = uv[2 * i + 1] = depth[i] = 0.f;
        if (i >= n) continue;
        const int t = a.t_in[row];
        const bool can = a.raw && a.alive_in[row] != 0 && (a.direction > 0 ? t < a.max_t : t > 0);
        const int t_next = can ? t + (a.direction > 0 ? 1 : -1) : t;
        if (rem == 0 && a.t_out) { a.t_out[row] = t_next; a.alive_out[row] = can ? 1 : 0; }
        float fx = 0.f, fy = 0.f, fz = 0.f;
        if (can) {
            const float* rec = a.raw + (p0 + i) * NSFF_RAW_STRIDE;
            if (a.direction > 0) {
                const float4 w = *reinterpret_cast<const float4*>(rec + 8);
                fx = w.x; fy = w.y; fz = w.z;
            } else {
                fx = rec[11];
                const float2 w = *reinterpret_cast<const float2*>(rec + 12);
                fy = w.x; fz = w.y;
            }
            if ((x[3 * i + 2] + 1.f) * 0.5f > TRK_Z_FAR) { fx = 0.f; fy = 0.f; fz = 0.f; }
            x[3 * i] = x[3 * i] + fx; x[3 * i + 1] = x[3 * i + 1] + fy; x[3 * i + 2] = x[3 * i + 2] + fz;
        }
        if (project) {
            const int cam = a.fixed_view ? 0 : min(max(t_next, 0), a.n_poses - 1);     // (a time outside the sequence reads no stray row)
            const float* M = a.Ps + (int64_t)cam * 12;
            float u, v;
            const float wd = ndc_to_pixel(x[3 * i], x[3 * i + 1], x[3 * i + 2], M, a.fx, a.fy, a.cx, a.cy, u, v);
            if (!(wd > 0.f)) { u = NSFF_FLOW_UNKNOWN; v = NSFF_FLOW_UNKNOWN; }
            uv[2 * i] = u; uv[2 * i + 1] = v; depth[i] = wd;
        }
        if (++rem == a.pts_per_row) { rem = 0; ++row; }
    }
    if (a.xyz_out) store_pts<3>(a.xyz_out + p0 * 3, n, x);
    if (project) {
        store_pts<2>(a.uv + p0 * 2, n, uv);
        store_pts<1>(a.depth + p0, n, depth);
    }
}

__global__ __launch_bounds__(256) void track_clear_kernel(uint32_t* __restrict__ canvas, int64_t n_pixels) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n_pixels) canvas[p] = 0u;
}

// an end of a segment that can be drawn: finite and |u|, |v| < 32768 (NSFF_FLOW_UNKNOWN and NaN fail)
__device__ __forceinline__ bool end_ok(float u, float v) { return fabsf(u) < 32768.f && fabsf(v) < 32768.f; }
// floor(a / b), b > 0
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

__global__ __launch_bounds__(256) void track_draw_kernel(NsffTrackDrawArgs a, uint32_t* __restrict__ canvas) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.n_steps * a.n_tracks) return;
    const int j = (int)(idx / a.n_tracks), q = (int)(idx - (int64_t)j * a.n_tracks);
    const int64_t e0 = (int64_t)j * a.n_tracks + q, e1 = e0 + a.n_tracks;
    if (!a.ok[e0] || !a.ok[e1]) return;
    const float2 A = reinterpret_cast<const float2*>(a.uv)[e0], B = reinterpret_cast<const float2*>(a.uv)[e1];
    if (!end_ok(A.x, A.y) || !end_ok(B.x, B.y)) return;
    const int x0 = (int)floorf(A.x + 0.5f), y0 = (int)floorf(A.y + 0.5f);
    const int dx = (int)floorf(B.x + 0.5f) - x0, dy = (int)floorf(B.y + 0.5f) - y0;
    const int N = max(abs(dx), abs(dy));
    if (N > (int64_t)a.H + a.W) return;
    const uint32_t key = ((uint32_t)(j + 1) << 20) | (uint32_t)q;
    for (int i = 0; i <= N; ++i) {
        int x = x0, y = y0;
        if (N > 0) {
            x += (int)floor_div(2 * (int64_t)i * dx + N, 2 * (int64_t)N);
            y += (int)floor_div(2 * (int64_t)i * dy + N, 2 * (int64_t)N);
        }
        if (x < 0 || x >= a.W || y < 0 || y >= a.H) continue;
        atomicMax(canvas + (int64_t)y * a.W + x, key);
    }
}

__global__ __launch_bounds__(256) void track_resolve_kernel(NsffTrackDrawArgs a, const uint32_t* __restrict__ canvas) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)a.H * a.W) return;
    const uint32_t key = canvas[p];
    const uint8_t* src = a.image + p * 3;
    if (key) src = a.lut + 3 * ((255 * (int)(key >> 20)) / a.n_steps);
    uint8_t* dst = a.out + p * 3;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
}

inline unsigned blocks_of(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

extern "C" int nsff_track_step(const NsffTrackStepArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (a->n_rows < 0 || a->pts_per_row < 1 || a->max_t < 0 || (a->direction != 1 && a->direction != -1)) return NSFF_ERR_INVALID;
    if (a->n_rows > NSFF_TRACK_MAX_POINTS / a->pts_per_row) return NSFF_ERR_INVALID;
    const bool cameras = a->Ps || a->uv || a->depth;
    if (cameras) {
        if (!a->Ps || !a->uv || !a->depth) return NSFF_ERR_NULL;
        if (a->n_poses < 1 || (!a->fixed_view && a->max_t >= a->n_poses)) return NSFF_ERR_INVALID;
        if (!(a->fx < 0.f || a->fx > 0.f) || !(a->fy < 0.f || a->fy > 0.f)) return NSFF_ERR_INVALID;   // zero or NaN
    }
    const bool moves = a->raw != nullptr;
    if (!moves && !cameras) return NSFF_ERR_INVALID;                                 // nothing to compute
    if (!moves && (a->xyz_out || a->t_out || a->alive_out)) return NSFF_ERR_INVALID; // a next slab without records to step by
    if (a->n_rows == 0) return NSFF_OK;
    if (!a->xyz_in || !a->t_in || !a->alive_in) return NSFF_ERR_NULL;
    if (moves && (!a->xyz_out || !a->t_out || !a->alive_out)) return NSFF_ERR_NULL;
    if (moves && (a->t_out == a->t_in || a->alive_out == a->alive_in)) return NSFF_ERR_INVALID;   // a row's state is read by S lanes and written by one
    if ((uintptr_t)a->raw & 15) return NSFF_ERR_ALIGN;
    if (((uintptr_t)a->xyz_in | (uintptr_t)a->xyz_out | (uintptr_t)a->t_in | (uintptr_t)a->t_out | (uintptr_t)a->Ps |
         (uintptr_t)a->uv | (uintptr_t)a->depth) & 3)
        return NSFF_ERR_ALIGN;
    const int64_t n_points = a->n_rows * a->pts_per_row;
    hipLaunchKernelGGL(track_step_kernel, dim3(blocks_of(n_points, TRK_THREADS * TRK_PTS)), dim3(TRK_THREADS), 0, (hipStream_t)stream, *a);
    return nsff_launch_status();
}

extern "C" int64_t nsff_track_draw_scratch_bytes(int32_t H, int32_t W) {
    return frame_dims_ok(1, H, W) ? 4 * (int64_t)H * W : 0;
}

extern "C" int nsff_track_draw(const NsffTrackDrawArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!frame_dims_ok(1, a->H, a->W)) return NSFF_ERR_INVALID;
    if (a->n_steps < 1 || a->n_steps >= NSFF_TRACK_MAX_STEPS || a->n_tracks < 0 || a->n_tracks >= NSFF_TRACK_MAX_TRACKS) return NSFF_ERR_INVALID;
    if (!a->image || !a->out || !a->lut || !a->scratch) return NSFF_ERR_NULL;
    if (a->n_tracks > 0 && (!a->uv || !a->ok)) return NSFF_ERR_NULL;
    if (a->scratch_bytes < nsff_track_draw_scratch_bytes(a->H, a->W)) return NSFF_ERR_INVALID;
    if (((uintptr_t)a->scratch & 3) || ((uintptr_t)a->uv & 7)) return NSFF_ERR_ALIGN;
    const int64_t n_pixels = (int64_t)a->H * a->W, n_segments = (int64_t)a->n_steps * a->n_tracks;
    uint32_t* canvas = reinterpret_cast<uint32_t*>(a->scratch);
    hipLaunchKernelGGL(track_clear_kernel, dim3(blocks_of(n_pixels, 256)), dim3(256), 0, (hipStream_t)stream, canvas, n_pixels);
    if (n_segments > 0)
        hipLaunchKernelGGL(track_draw_kernel, dim3(blocks_of(n_segments, 256)), dim3(256), 0, (hipStream_t)stream, *a, canvas);
    hipLaunchKernelGGL(track_resolve_kernel, dim3(blocks_of(n_pixels, 256)), dim3(256), 0, (hipStream_t)stream, *a, canvas);
    return nsff_launch_status();
}
