// What the kernels that follow optical flow from frame to frame share (flow.hip, flowmedian.hip, motion.hip, depth.hip, parallax.hip,
// motionspan.hip): the known-flow rule, the bilinear sample, the chain of a lane's four pixels and its hop, and the two measurements
// taken along it -- the distance from the epipolar line and the triangulation vote.  include/nsff_render.h states every step as a
// chain of single fp32 operations, and the functions here keep that order: a translation unit that includes this header is built
// -ffp-contract=off, and the numpy twins under tests/ are the same chains, compared bit for bit.  Per translation unit, like
// nsff_frame_ops.h, whose pixel quads this builds on.
#pragma once
#include <cfloat>

#include "nsff_frame_ops.h"

namespace {

constexpr float FLOW_THRESH = 1e7f;                               // flowlib's UNKNOWN_FLOW_THRESH

// both components within the threshold; a NaN fails the comparison
__device__ __forceinline__ bool flow_known(float u, float v) { return fabsf(u) <= FLOW_THRESH && fabsf(v) <= FLOW_THRESH; }
__device__ __forceinline__ bool flow_known(float2 w) { return flow_known(w.x, w.y); }

// B at (qx, qy) inside the image, one component: ((B00 (1 - ax) + B01 ax) (1 - ay)) + ((B10 (1 - ax) + B11 ax) ay)
__device__ __forceinline__ float bilerp(float b00, float b01, float b10, float b11, float ax, float omx, float ay, float omy) {
    const float top = b00 * omx + b01 * ax;
    const float bot = b10 * omx + b11 * ax;
    return (top * omy) + (bot * ay);
}

// Two horizontally adjacent taps in one load -- a hop is bound by the number of gathers a lane issues, not by their bytes: 16 bytes
// of flow at an 8-byte aligned address, two bytes of valid / masks at any address.
typedef float flow_pair __attribute__((ext_vector_type(4), aligned(8)));
typedef uint16_t byte_pair __attribute__((aligned(1)));
// the bytes at p[0] (only where `first`) and p[1] are both non-zero
__device__ __forceinline__ bool pair_set(const uint8_t* p, bool first) {
    const uint32_t v = *reinterpret_cast<const byte_pair*>(p);
    return ((v >> 8) != 0u) & (!first | ((v & 0xffu) != 0u));
}

// The lane's four pixels: (x, y) of the first by one division, the others by stepping (any W >= 1).  As floats for the kernels that
// carry them through a loop of hops, as ints where they are used once or twice (motion_map_kernel, which converts at each use).
template <class T>
__device__ __forceinline__ void quad_pixels(const Quad& q, int64_t HW, int W, T (&xs)[FIN_PX], T (&ys)[FIN_PX]) {
    const int p = (int)min(q.p0, HW - 1);
    int py = p / W, px = p - py * W;
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        xs[i] = (T)px; ys[i] = (T)py;
        if (++px == W) { px = 0; ++py; }
    }
}

// ---- the chain: frame f, direction d (0: s = +1, flow_fw; 1: s = -1, flow_bw) starts with A = flow_d[f] at the pixel; at step k the
// caller measures with q = pixel + A in the neighbour n = f + s k, then the chain HOPS: b = flow_d[n] sampled bilinearly at q,
// A += b, and it stays alive only if q is inside the image and the four taps are known and set in the byte planes given.  The
// state of a lane's four pixels stays in registers across the hops. ----
struct Chain {
    float A[2 * FIN_PX];                                          // the flow summed so far
    bool alive[FIN_PX];
};

// A = flow_d[f] at the lane's pixels; alive = a pixel of the frame, known, valid[f][d] != 0 where given
__device__ __forceinline__ void chain_start(Chain& c, const float* flow, const uint8_t* valid, const Quad& q, int64_t f, int d, int64_t HW) {
    load_px<2>(flow, q, c.A);
    const int64_t plane = (f * 2 + d) * HW + q.p0;                // the direction's plane of `valid`
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        c.alive[i] = i < q.n && flow_known(c.A[2 * i], c.A[2 * i + 1]);
        if (valid) c.alive[i] = c.alive[i] && valid[plane + i] != 0;
    }
}

// The four taps of a hop for each of the lane's pixels, read without a branch from q = pixel + A clamped into frame n (B its flow, V
// its plane of `valid` or NULL).  The clamp is the identity where q is inside, where alone the
// taps are used, so no address leaves the frame whatever A holds -- NaN (it clamps to 0), +-inf, 1e10, the garbage a dead chain goes
// on adding up -- and the loads of a lane are in flight together.  The two taps of a row are neighbours in memory and come with one
// load, from the column xl = min(x0, W - 2) on, so that at the right edge, where x1 == x0 == W - 1, the pair still lies in the row:
// half the gathers.  A frame one pixel wide has no such pair and reads its single column.
// (disparity_span_kernel of parallax.hip has this hop written out, with a second byte plane: its header says why.)
struct Taps {
    float2 b00[FIN_PX], b01[FIN_PX], b10[FIN_PX], b11[FIN_PX];
    bool ok[FIN_PX];                                              // set in V at all four
};
__device__ __forceinline__ void hop_taps(Taps& t, const Chain& c, const float (&xs)[FIN_PX], const float (&ys)[FIN_PX], const float2* B,
                                         const uint8_t* V, int H, int W) {
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    int r0[FIN_PX], r1[FIN_PX];                                   // the taps' rows from their left column on: pixel indices within a frame are ints
    bool first[FIN_PX];                                           // x0 is that column (not at the right edge, where x1 == x0 == W - 1)
#pragma unroll
    for (int i = 0; i < FIN_PX; ++i) {
        const float cx = fminf(fmaxf(xs[i] + c.A[2 * i], 0.f), wmax);
        const float cy = fminf(fmaxf(ys[i] + c.A[2 * i + 1], 0.f), hmax);
        const int x0 = min((int)floorf(cx), W - 1), y0 = min((int)floorf(cy), H - 1);      // (W - 1 as a float may round up)
        const int y1 = min(y0 + 1, H - 1);
        const int xl = max(min(x0, W - 2), 0);                    // xl and xl + 1 are columns of the image where W >= 2
        first[i] = x0 == xl;
        r0[i] = y0 * W + xl; r1[i] = y1 * W + xl;
        t.ok[i] = true;
    }
    if (W >= 2) {                                                 // (uniform) x1 = min(x0 + 1, W - 1) is column xl + 1 in every case
#pragma unroll
        for (int i = 0; i < FIN_PX; ++i) {
            const flow_pair p0 = *reinterpret_cast<const flow_pair*>(B + r0[i]);
            const flow_pair p1 = *reinterpret_cast<const flow_pair*>(B + r1[i]);
            t.b01[i] = make_float2(p0.z, p0.w); t.b00[i] = first[i] ? make_float2(p0.x, p0.y) : t.b01[i];
            t.b11[i] = make_float2(p1.z, p1.w); t.b10[i] = first[i] ? make_float2(p1.x, p1.y) : t.b11[i];
        }
        if (V) {                                                  // (uniform)
#pragma unroll
            for (int i = 0; i < FIN_PX; ++i) {
                const bool top = pair_set(V + r0[i], first[i]), bot = pair_set(V + r1[i], first[i]);      // both read, no branch
                t.ok[i] = top && bot;
            }
        }
    } else {                                                      // one column: x1 == x0 == 0
#pragma unroll
        for (int i = 0; i < FIN_PX; ++i) {
            t.b00[i] = t.b01[i] = B[r0[i]]; t.b10[i] = t.b11[i] = B[r1[i]];
            if (V) t.ok[i] = (V[r0[i]] != 0) & (V[r1[i]] != 0);
        }
    }
}

// the hop of pixel i at q = (qx, qy), the two floats the step's measurement used: alive &&= hop_ok, A += b
__device__ __forceinline__ void hop_pixel(Chain& c, const Taps& t, int i, float qx, float qy, float wmax, float hmax) {
    const bool inside = qx >= 0.f && qx <= wmax && qy >= 0.f && qy <= hmax;
    const float fx = qx - floorf(qx), fy = qy - floorf(qy);
    const float omx = 1.f - fx, omy = 1.f - fy;
    const float bu = bilerp(t.b00[i].x, t.b01[i].x, t.b10[i].x, t.b11[i].x, fx, omx, fy, omy);
    const float bv = bilerp(t.b00[i].y, t.b01[i].y, t.b10[i].y, t.b11[i].y, fx, omx, fy, omy);
    c.alive[i] = c.alive[i] && inside && t.ok[i] && flow_known(t.b00[i]) && flow_known(t.b01[i]) && flow_known(t.b10[i])
                 && flow_known(t.b11[i]);
    c.A[2 * i] = c.A[2 * i] + bu;
    c.A[2 * i + 1] = c.A[2 * i + 1] + bv;
}

// ---- the measurements ----
// The distance of q = (qx, qy) from the epipolar line M (3 x 3, row-major) gives the pixel (x, y):
//   l_i = (M[i][0] x + M[i][1] y) + M[i][2], r = (l0 qx + l1 qy) + l2, n = l0 l0 + l1 l1, e = |r| / sqrtf(n), line_ok: 0 < n < inf
__device__ __forceinline__ void line_distance(const float (&M)[9], float x, float y, float qx, float qy, float& e, bool& line_ok) {
    const float l0 = (M[0] * x + M[1] * y) + M[2];
    const float l1 = (M[3] * x + M[4] * y) + M[5];
    const float l2 = (M[6] * x + M[7] * y) + M[8];
    const float r = (l0 * qx + l1 * qy) + l2;
    const float nn = l0 * l0 + l1 * l1;
    e = fabsf(r) / sqrtf(nn);
    line_ok = nn > 0.f && nn <= FLT_MAX;                          // finite and positive; a NaN fails both
}

// The triangulation vote of the pixel (x, y) seen at (up, vp) = pixel + flow, against the row P of twelve values: the parallax p2
// in px^2 and the two sums ab, aa of the least-squares disparity ab / aa; the vote counts only where hz > 0.
__device__ __forceinline__ void parallax_vote(const float (&P)[12], float x, float y, float up, float vp, float& p2, float& ab, float& aa,
                                              float& hz) {
    const float hx = (P[0] * x + P[1] * y) + P[2];
    const float hy = (P[3] * x + P[4] * y) + P[5];
    hz = (P[6] * x + P[7] * y) + P[8];
    const float r = 1.f / hz;
    const float ax = (P[9] - up * P[11]) * r, ay = (P[10] - vp * P[11]) * r;
    const float bx = up - hx * r, by = vp - hy * r;
    p2 = bx * bx + by * by;
    ab = ax * bx + ay * by;
    aa = ax * ax + ay * ay;
}

}  // namespace
