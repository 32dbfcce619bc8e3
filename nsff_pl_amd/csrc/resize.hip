// Resizing decoded frames to the training resolution: the four resize statements of the reference's dataset constructor
// (datasets/monocular.py:98-99, 146-147, 158-163, 168-176; datasets/flowlib.py:320-338), see the header.
//
// The per-axis tables (nsff_resize_ksize, nsff_resize_table) are built on the host in double, per filter; the kernels only apply
// them, so one table serves every frame of a sequence.
//
// lanczos_u8_kernel: Pillow's two 8-bit passes (ImagingResampleHorizontal_8bpc, then ...Vertical_8bpc) in ONE launch.  A workgroup
// owns an output tile of LZ_TW x TH pixels.  Pass 1 filters the source rows the tile's output rows need, restricted to the tile's
// columns, into LDS as uint8 (rounded and clipped exactly where Pillow writes its temporary image); pass 2 filters that LDS
// image down the columns and stores the tile.  No intermediate goes to memory.
//
// LDS layout.  A row of the intermediate is the tile's LZ_TW x C bytes, flat (pixel-interleaved as in memory), LZ_TW = 128: 32, 64
// or 96 dwords for C = 1, 2, 3 -- always a whole number of 32-dword bank rows of ds_read_b32 / ds_write_b32 (banks (a / 4) % 32,
// conflicts within a 32-lane half).  A lane owns FOUR consecutive bytes = one dword of a row, whatever pixels and channels they
// belong to (with the 3-byte stride they straddle two pixels): pass 1 writes it with one ds_write_b32 and pass 2 reads it with one
// ds_read_b32 and unpacks, so there is no byte-wide LDS access at all.  Work item t -> row (pass 1: block of LZ_RB rows) t / DW,
// dword t % DW with DW = 32 C: the 32 lanes of a half-wave always lie in one row at 32 consecutive dwords = 32 distinct banks, in
// both passes, for any row pitch.  The vertical weights of a half-wave are one address (a broadcast).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <vector>

#include "../../include/nsff_render.h"
#include "nsff_common.h"
#include "nsff_frame_ops.h"

namespace {

constexpr int LZ_THREADS = 256;
constexpr int LZ_TW = 128;                                        // output tile width, pixels
constexpr int LZ_TH = 16;                                         // largest output tile height
constexpr int LZ_MAX_C = 3;
constexpr int LZ_RB = 8;                                         // source rows a pass-1 work item filters together
constexpr int LZ_KMAX = NSFF_RESIZE_MAX_KSIZE;                    // 49
constexpr int LZ_ROWS_SMALL = 64, LZ_ROWS_LARGE = 128;            // source rows of a tile held in LDS (two builds of the kernel)
constexpr int LZ_WX_TAPS = 24;                                    // horizontal tables up to this many taps (a 3.6x downscale) are staged in LDS
constexpr int LZ_PRECISION = 22;                                  // Pillow's PRECISION_BITS = 32 - 8 - 2

// Pillow's clip8.  The empty asm keeps the clamped value opaque to instruction selection: left visible, two of them packed as
// c0 | c1 << 8 are selected as one v_ashr_pk_u8_i32, whose result had the previous contents of the destination in bits 31:16
// on the MI355X (bytes 2 and 3 of every stored dword came out OR-ed with them; measured).
__device__ __forceinline__ uint32_t clip8(int acc) {
    int v = min(max(acc >> LZ_PRECISION, 0), 255);
    asm volatile("" : "+v"(v));
    return (uint32_t)v;
}

// static LDS: ROWS * 384 + 128 * 24 * 4 + 16 * 49 * 4 + 2 * 16 * 4 bytes = 40 128 (ROWS = 64) or 64 704 (ROWS = 128), within 64 KiB
template <int ROWS>
__global__ __launch_bounds__(LZ_THREADS) void lanczos_u8_kernel(const NsffFrameResizeArgs a, int th) {
    __shared__ uint32_t s_mid[ROWS * LZ_TW * LZ_MAX_C / 4];
    __shared__ int s_wx[LZ_TW * LZ_WX_TAPS];
    __shared__ int s_wy[LZ_TH * LZ_KMAX];
    __shared__ int s_y0[LZ_TH], s_yn[LZ_TH];
    const int tid = threadIdx.x;
    const int C = a.channels, DW = LZ_TW * C / 4;                 // dwords per LDS row
    const int x0 = blockIdx.x * LZ_TW, y0 = blockIdx.y * th;
    const int tw = min(LZ_TW, a.dst_w - x0), rows_out = min(th, a.dst_h - y0);
    const int nbytes = tw * C;                                    // valid bytes of a tile row
    const bool pass_h = a.src_w != a.dst_w, pass_v = a.src_h != a.dst_h;
    const bool stage_x = pass_h && a.ksize_x <= LZ_WX_TAPS;       // the tile's horizontal weights from LDS, else from memory
    const int64_t f = blockIdx.z;
    const uint8_t* __restrict__ src = reinterpret_cast<const uint8_t*>(a.src) + f * a.src_h * (int64_t)a.src_w * C;
    uint8_t* __restrict__ dst = reinterpret_cast<uint8_t*>(a.dst) + f * a.dst_h * (int64_t)a.dst_w * C;
    const int* __restrict__ wx = reinterpret_cast<const int*>(a.x_weights);
    const int* __restrict__ wy = reinterpret_cast<const int*>(a.y_weights);

    // the tile's output rows: first source row, tap count (clamped into the image: a bad table reads nothing outside it), weights
    if (tid < LZ_TH) {
        int s = y0 + tid, n = 1;
        if (tid < rows_out && pass_v) {
            s = min(max(a.y_start[y0 + tid], 0), a.src_h - 1);
            n = min(max(a.y_count[y0 + tid], 0), min(a.src_h - s, a.ksize_y));
        }
        s_y0[tid] = s; s_yn[tid] = n;
    }
    if (pass_v)
        for (int i = tid; i < rows_out * a.ksize_y; i += LZ_THREADS) s_wy[i] = wy[(int64_t)y0 * a.ksize_y + i];
    if (stage_x)
        for (int i = tid; i < tw * a.ksize_x; i += LZ_THREADS) s_wx[i] = wx[(int64_t)x0 * a.ksize_x + i];
    __syncthreads();
    const int row0 = s_y0[0];
    const int n_rows = min(s_y0[rows_out - 1] + s_yn[rows_out - 1] - row0, ROWS);   // (the host sized th so that they fit)

    // ---- pass 1: source rows row0 .. row0 + n_rows - 1, the tile's columns -> LDS ----
    // A work item is one dword column q of LZ_RB consecutive rows: the taps and weights of its four bytes do not depend on the
    // row, so a weight is loaded once for LZ_RB rows and the LZ_RB byte loads of a tap are independent (in flight together).
    // Rows past the last one are clamped onto it (loaded, not stored): no branch inside the tap loop.
    const int64_t pitch = (int64_t)a.src_w * C;
    const int n_blocks = (n_rows + LZ_RB - 1) / LZ_RB;
    for (int t = tid; t < n_blocks * DW; t += LZ_THREADS) {
        const int rb = t / DW, q = t - rb * DW, r_first = rb * LZ_RB;
        const uint8_t* __restrict__ line = src + (row0 + r_first) * pitch;
        int64_t off[LZ_RB];                                       // each row's offset from `line`
#pragma unroll
        for (int i = 0; i < LZ_RB; ++i) off[i] = min(i, n_rows - 1 - r_first) * pitch;
        uint32_t word[LZ_RB];
#pragma unroll
        for (int i = 0; i < LZ_RB; ++i) word[i] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int e = 4 * q + b;
            if (e >= nbytes) break;
            const int xp = e / C, c = e - xp * C, x = x0 + xp;
            if (pass_h) {
                const int s = min(max(a.x_start[x], 0), a.src_w - 1);
                const int n = min(max(a.x_count[x], 0), min(a.src_w - s, a.ksize_x));
                const uint8_t* __restrict__ p = line + (int64_t)s * C + c;
                int acc[LZ_RB];
#pragma unroll
                for (int i = 0; i < LZ_RB; ++i) acc[i] = 1 << (LZ_PRECISION - 1);
                // The weights of pixel x: ksize_x dwords apart from pixel to pixel.  In memory a wave's weight load touches a line
                // per pixel; in LDS the stride is odd (ksize = 2 ceil(..) + 1), so a half-wave's pixels fall on distinct banks
                // and the three lanes of a pixel share one address.
                auto taps = [&](const int* __restrict__ k) {
#pragma unroll 1                                                  // (by four measured neutral, and costs 100 registers)
                    for (int j = 0; j < n; ++j) {
                        const int w = k[j];
#pragma unroll
                        for (int i = 0; i < LZ_RB; ++i) acc[i] += __mul24((int)p[off[i] + j * C], w);
                    }
                };
                if (stage_x) taps(s_wx + xp * a.ksize_x);
                else taps(wx + (int64_t)x * a.ksize_x);
#pragma unroll
                for (int i = 0; i < LZ_RB; ++i) word[i] |= clip8(acc[i]) << (8 * b);
            } else {
#pragma unroll
                for (int i = 0; i < LZ_RB; ++i) word[i] |= (uint32_t)line[off[i] + (int64_t)x * C + c] << (8 * b);
            }
        }
#pragma unroll
        for (int i = 0; i < LZ_RB; ++i)
            if (r_first + i < n_rows) s_mid[(r_first + i) * DW + q] = word[i];
    }
    __syncthreads();

    // ---- pass 2: LDS columns -> the tile ----
    for (int t = tid; t < rows_out * DW; t += LZ_THREADS) {
        const int yy = t / DW, q = t - yy * DW;
        if (4 * q >= nbytes) continue;
        uint32_t word;
        if (pass_v) {
            const int r0 = max(s_y0[yy] - row0, 0), n = min(s_yn[yy], n_rows - r0);
            const int* k = s_wy + yy * a.ksize_y;
            int acc0 = 1 << (LZ_PRECISION - 1), acc1 = acc0, acc2 = acc0, acc3 = acc0;
            for (int j = 0; j < n; ++j) {
                const uint32_t m = s_mid[(r0 + j) * DW + q];
                const int w = k[j];
                acc0 += __mul24((int)(m & 255u), w);
                acc1 += __mul24((int)((m >> 8) & 255u), w);
                acc2 += __mul24((int)((m >> 16) & 255u), w);
                acc3 += __mul24((int)(m >> 24), w);
            }
            word = clip8(acc0) | (clip8(acc1) << 8) | (clip8(acc2) << 16) | (clip8(acc3) << 24);
        } else {
            word = s_mid[yy * DW + q];
        }
        uint8_t* o = dst + ((int64_t)(y0 + yy) * a.dst_w + x0) * C + 4 * q;
        const int left = nbytes - 4 * q;
        if (left >= 4 && !(reinterpret_cast<uintptr_t>(o) & 3)) {
            *reinterpret_cast<uint32_t*>(o) = word;
        } else {
            for (int b = 0; b < 4 && b < left; ++b) o[b] = (uint8_t)(word >> (8 * b));
        }
    }
}

// NEAREST_PIL (uint8) and NEAREST_CV (fp32): dst[f][y][x][c] = src[f][iy[y]][ix[x]][c], one element a lane
template <class T>
__global__ __launch_bounds__(256) void gather_kernel(const NsffFrameResizeArgs a) {
    const int64_t per = (int64_t)a.dst_h * a.dst_w * a.channels;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    const int64_t f = blockIdx.y;
    const int C = a.channels;
    const int64_t pix = i / C;
    const int c = (int)(i - pix * C), y = (int)(pix / a.dst_w), x = (int)(pix - (int64_t)y * a.dst_w);
    const int sy = min(max(a.y_start[y], 0), a.src_h - 1), sx = min(max(a.x_start[x], 0), a.src_w - 1);
    const T* __restrict__ s = reinterpret_cast<const T*>(a.src) + f * a.src_h * (int64_t)a.src_w * C;
    reinterpret_cast<T*>(a.dst)[f * per + i] = s[((int64_t)sy * a.src_w + sx) * C + c];
}

// LINEAR_CV (fp32, C channels, here the flow's 2): the two rows' horizontal lerps, the vertical lerp, the ratio; this file is
// built uncontracted, so every step is one fp32 operation
__global__ __launch_bounds__(256) void linear_kernel(const NsffFrameResizeArgs a) {
    const int64_t per = (int64_t)a.dst_h * a.dst_w * a.channels;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    const int64_t f = blockIdx.y;
    const int C = a.channels;
    const int64_t pix = i / C;
    const int c = (int)(i - pix * C), y = (int)(pix / a.dst_w), x = (int)(pix - (int64_t)y * a.dst_w);
    const int sy0 = min(max(a.y_start[y], 0), a.src_h - 1), sy1 = min(sy0 + max(a.y_count[y] - 1, 0), a.src_h - 1);
    const int sx0 = min(max(a.x_start[x], 0), a.src_w - 1), sx1 = min(sx0 + max(a.x_count[x] - 1, 0), a.src_w - 1);
    const float* __restrict__ wxp = reinterpret_cast<const float*>(a.x_weights) + 2 * x;
    const float* __restrict__ wyp = reinterpret_cast<const float*>(a.y_weights) + 2 * y;
    const float a0 = wxp[0], a1 = wxp[1], b0 = wyp[0], b1 = wyp[1];
    const float* __restrict__ s = reinterpret_cast<const float*>(a.src) + f * a.src_h * (int64_t)a.src_w * C;
    const float* __restrict__ r0 = s + (int64_t)sy0 * a.src_w * C, * __restrict__ r1 = s + (int64_t)sy1 * a.src_w * C;
    const float h0 = r0[(int64_t)sx0 * C + c] * a0 + r0[(int64_t)sx1 * C + c] * a1;
    const float h1 = r1[(int64_t)sx0 * C + c] * a0 + r1[(int64_t)sx1 * C + c] * a1;
    const float v = h0 * b0 + h1 * b1;
    reinterpret_cast<float*>(a.dst)[f * per + i] = v * a.ratio[c < 2 ? c : 1];
}

// ---- host: the tables ----
double sinc(double x) { return x == 0.0 ? 1.0 : std::sin(x * M_PI) / (x * M_PI); }
double lanczos3(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3.0) : 0.0; }

int lanczos_ksize(int32_t n_in, int32_t n_out) {
    const double scale = (double)n_in / (double)n_out, fs = scale < 1.0 ? 1.0 : scale;
    return 2 * (int)std::ceil(3.0 * fs) + 1;
}

// source rows a tile of `th` output rows can need: its last row starts at most ceil((th - 1) scale) + 1 rows below its first
// (two truncations of centres (th - 1) scale apart) and has at most ksize taps
int64_t lanczos_tile_rows(int th, int32_t n_in, int32_t n_out) {
    if (n_in == n_out) return th;
    return (int64_t)std::ceil((th - 1) * ((double)n_in / (double)n_out)) + 1 + lanczos_ksize(n_in, n_out);
}

bool filter_ok(int32_t filter) { return filter >= NSFF_RESIZE_LANCZOS_U8 && filter <= NSFF_RESIZE_LINEAR_CV; }

}  // namespace

extern "C" int nsff_resize_ksize(int32_t filter, int32_t n_in, int32_t n_out) {
    if (!filter_ok(filter) || n_in < 1 || n_out < 1) return NSFF_ERR_INVALID;
    if (filter == NSFF_RESIZE_LINEAR_CV) return 2;
    if (filter != NSFF_RESIZE_LANCZOS_U8) return 1;
    const double ks = 2.0 * std::ceil(3.0 * std::fmax((double)n_in / (double)n_out, 1.0)) + 1.0;
    return ks > NSFF_RESIZE_MAX_KSIZE ? NSFF_ERR_UNSUPPORTED : (int)ks;
}

extern "C" int nsff_resize_table(int32_t filter, int32_t n_in, int32_t n_out, int32_t* start, int32_t* count, void* weights) {
    const int ksize = nsff_resize_ksize(filter, n_in, n_out);
    if (ksize < 0) return ksize;
    if (!start || !count || (!weights && ksize > 1)) return NSFF_ERR_NULL;
    if (filter == NSFF_RESIZE_LANCZOS_U8) {                        // Pillow's precompute_coeffs and normalize_coeffs_8bpc
        int32_t* kk = reinterpret_cast<int32_t*>(weights);
        const double scale = (double)n_in / (double)n_out, fs = scale < 1.0 ? 1.0 : scale;
        const double support = 3.0 * fs, ss = 1.0 / fs;
        std::vector<double> k(ksize);
        for (int i = 0; i < n_out; ++i) {
            const double center = (i + 0.5) * scale;
            int xmin = (int)(center - support + 0.5);
            if (xmin < 0) xmin = 0;
            int xmax = (int)(center + support + 0.5);
            if (xmax > n_in) xmax = n_in;
            xmax -= xmin;
            double ww = 0.0;
            for (int j = 0; j < xmax; ++j) { k[j] = lanczos3((j + xmin - center + 0.5) * ss); ww += k[j]; }
            for (int j = 0; j < ksize; ++j) {
                double w = j < xmax ? k[j] : 0.0;
                if (j < xmax && ww != 0.0) w /= ww;
                kk[(int64_t)i * ksize + j] = w < 0 ? (int)(-0.5 + w * (1 << LZ_PRECISION)) : (int)(0.5 + w * (1 << LZ_PRECISION));
            }
            start[i] = xmin; count[i] = xmax;
        }
    } else if (filter == NSFF_RESIZE_NEAREST_PIL) {                // ImagingScaleAffine: a running sum, not (i + 0.5) a
        const double step = (double)n_in / (double)n_out;
        double x = 0.5 * step;
        for (int i = 0; i < n_out; ++i, x += step) {
            const int s = (int)x;
            start[i] = s < n_in - 1 ? s : n_in - 1; count[i] = 1;
        }
    } else if (filter == NSFF_RESIZE_NEAREST_CV) {                 // resizeNN
        const double ifx = 1.0 / ((double)n_out / (double)n_in);
        for (int i = 0; i < n_out; ++i) {
            const int s = (int)std::floor(i * ifx);
            start[i] = s < n_in - 1 ? s : n_in - 1; count[i] = 1;
        }
    } else {                                                       // the fp32 INTER_LINEAR tables
        float* w = reinterpret_cast<float*>(weights);
        const double scale = (double)n_in / (double)n_out;
        for (int i = 0; i < n_out; ++i) {
            float fx = (float)((i + 0.5) * scale - 0.5);
            int sx = (int)std::floor(fx);
            fx -= (float)sx;
            if (sx < 0) { sx = 0; fx = 0.f; }
            if (sx >= n_in - 1) { sx = n_in - 1; fx = 0.f; }
            start[i] = sx; count[i] = sx + 1 <= n_in - 1 ? 2 : 1;
            w[2 * i] = 1.f - fx; w[2 * i + 1] = fx;
        }
    }
    return NSFF_OK;
}

extern "C" int nsff_frame_resize(const NsffFrameResizeArgs* a, void* stream) {
    if (!a) return NSFF_ERR_NULL;
    if (!filter_ok(a->filter)) return NSFF_ERR_INVALID;
    if (!frame_dims_ok(a->n_frames, a->src_h, a->src_w) || !frame_dims_ok(a->n_frames, a->dst_h, a->dst_w)) return NSFF_ERR_INVALID;
    const bool lanczos = a->filter == NSFF_RESIZE_LANCZOS_U8, linear = a->filter == NSFF_RESIZE_LINEAR_CV;
    if (a->channels < 1 || a->channels > (linear ? 2 : LZ_MAX_C)) return NSFF_ERR_INVALID;
    if ((int64_t)a->dst_h * a->dst_w * a->channels > 0x7fffffff || (int64_t)a->src_h * a->src_w * a->channels > 0x7fffffff)
        return NSFF_ERR_INVALID;
    const int kx = nsff_resize_ksize(a->filter, a->src_w, a->dst_w), ky = nsff_resize_ksize(a->filter, a->src_h, a->dst_h);
    if (kx < 0) return kx;
    if (ky < 0) return ky;
    if (a->ksize_x != kx || a->ksize_y != ky) return NSFF_ERR_INVALID;            // tables of another size pair
    if (!a->src || !a->dst || !a->x_start || !a->y_start) return NSFF_ERR_NULL;
    if ((lanczos || linear) && (!a->x_count || !a->y_count || !a->x_weights || !a->y_weights)) return NSFF_ERR_NULL;
    if (((uintptr_t)a->x_start | (uintptr_t)a->y_start | (uintptr_t)a->x_count | (uintptr_t)a->y_count | (uintptr_t)a->x_weights |
         (uintptr_t)a->y_weights) & 3)
        return NSFF_ERR_ALIGN;
    const bool fp32 = linear || a->filter == NSFF_RESIZE_NEAREST_CV;
    if (fp32 && (((uintptr_t)a->src | (uintptr_t)a->dst) & 3)) return NSFF_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (lanczos) {
        // the tallest tile whose source rows fit the LDS image: 16 rows up to a 5.9x vertical downscale, 8 from there to 8x
        int th = LZ_TH;
        while (th > 1 && lanczos_tile_rows(th, a->src_h, a->dst_h) > LZ_ROWS_LARGE) th >>= 1;
        const int64_t rows = lanczos_tile_rows(th, a->src_h, a->dst_h);
        if (rows > LZ_ROWS_LARGE) return NSFF_ERR_UNSUPPORTED;
        const int64_t gx = ((int64_t)a->dst_w + LZ_TW - 1) / LZ_TW, gy = ((int64_t)a->dst_h + th - 1) / th;
        if (gy > 65535) return NSFF_ERR_INVALID;
        const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)a->n_frames);
        if (rows <= LZ_ROWS_SMALL) hipLaunchKernelGGL(lanczos_u8_kernel<LZ_ROWS_SMALL>, grid, dim3(LZ_THREADS), 0, st, *a, th);
        else hipLaunchKernelGGL(lanczos_u8_kernel<LZ_ROWS_LARGE>, grid, dim3(LZ_THREADS), 0, st, *a, th);
        return nsff_launch_status();
    }
    const int64_t per = (int64_t)a->dst_h * a->dst_w * a->channels;
    const dim3 grid((unsigned)((per + 255) / 256), (unsigned)a->n_frames);
    if (linear) hipLaunchKernelGGL(linear_kernel, grid, dim3(256), 0, st, *a);
    else if (fp32) hipLaunchKernelGGL(gather_kernel<float>, grid, dim3(256), 0, st, *a);
    else hipLaunchKernelGGL(gather_kernel<uint8_t>, grid, dim3(256), 0, st, *a);
    return nsff_launch_status();
}
