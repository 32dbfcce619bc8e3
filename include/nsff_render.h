/*
 * nsff_render.h -- C-ABI of the MI355X (gfx950) NSFF ray renderer.
 *
 * Drop-in boundary for ONE hot path of kwea123/nsff_pl: models/rendering.py
 * (render_rays, inference, render_transient_warping, sample_pdf) and
 * models/nerf.py (PosEmbedding, NeRF).  The reference has no FFI of its own
 * (pure Python on torch); these entry points are what a maintainer would bind
 * with ctypes to replace the torch ops of that path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (int32 where said);
 *     the library never allocates, frees or copies user-visible memory;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *     the call returns without synchronising;
 *   - return value: 0 = ok, <0 = NSFF_ERR_* (no exceptions cross the ABI);
 *   - not thread-safe per stream; re-entrant across streams (no global state).
 */
#ifndef NSFF_RENDER_H
#define NSFF_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSFF_OK               0
#define NSFF_ERR_INVALID     -1   /* bad shape / flag / unsupported architecture */
#define NSFF_ERR_NULL        -2   /* required pointer missing                      */
#define NSFF_ERR_ALIGN       -3   /* pointer not 16-byte aligned where required    */
#define NSFF_ERR_HIP         -4   /* a HIP runtime call failed (see nsff_last_hip_error) */

#define NSFF_ABI_VERSION      32
#define NSFF_RAW_STRIDE      16   /* floats per point in a raw field record        */
#define NSFF_MAX_FREQS       24
#define NSFF_MAX_LAYERS       8

/* Raw field record (what NeRF.forward returns per point, reference nerf.py:187-213):
 *   [0..2] static rgb (sigmoid)  [3] static sigma (raw)
 *   [4..6] transient rgb         [7] transient sigma (raw)
 *   [8..10] flow_fw = flow_scale*tanh(.)   [11..13] flow_bw   [14..15] unused
 * nsff_field_query writes whole 64-byte records: slots a launch does not evaluate are written as 0. */

/* ---- model description: mirrors NeRF.__init__ (reference nerf.py:34-40) ---- */
typedef struct NsffModelDesc {
    int32_t D;              /* trunk depth, 2..8 (reference: 8)                     */
    int32_t W;              /* width, must be 256                                  */
    int32_t skip;           /* the layer (0-based, 1..D-1) that re-reads the input (reference: 4); 0 = none or see skip_mask */
    int32_t in_xyz;         /* 63                                                  */
    int32_t in_dir;         /* 27                                                  */
    int32_t in_a;           /* appearance code width or 0                          */
    int32_t in_t;           /* transient code width or 0                           */
    int32_t use_viewdir;    /* static_dir_encoding present                         */
    int32_t has_transient;  /* encode_transient                                    */
    int32_t has_flow;       /* transient_flow_fw / _bw heads present               */
    float   flow_scale;     /* 0.2                                                 */
    int32_t skip_mask;      /* several skip layers (the reference's `skips` list, nerf.py:34-40,163-167): bit l set = layer l
                               reads [input | previous layer]; 0 = just `skip`.  Any subset of layers 1..D-1, in the
                               inference kernels and in the training kernels alike                         */
} NsffModelDesc;

/* effective set of skip layers of a description */
static inline uint32_t nsff_skip_layers(const NsffModelDesc* d) {
    return d->skip_mask ? (uint32_t)d->skip_mask : (d->skip > 0 ? 1u << d->skip : 0u);
}

/* Arithmetic of the field kernel's dense layers:
 *   NSFF_PREC_F32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
 *   NSFF_PREC_F16X3 fp32 operands split into two halfs, three f16 MFMAs per product,
 *                   fp32 accumulate (v_mfma_f32_32x32x16_f16), activations staged in LDS;
 *                   agrees with F32 to fp32 rounding level (same 1e-4 parity tests)
 * (Value 3 was the single-product fast mode of earlier ABI versions: not parity-grade, removed -- NSFF_ERR_INVALID now.)
 */
#define NSFF_PREC_F32        0
#define NSFF_PREC_F16X3      1

/* Size in bytes of the packed-weight buffer for `desc` at `precision`. */
int nsff_packed_bytes(const NsffModelDesc* desc, int precision, size_t* bytes);

/* Number of parameter tensors nsff_pack_weights expects, in this order
 * (PyTorch Linear layout, weight (out,in) row-major then bias):
 *   static_xyz_encoding_{1..D}.0, static_xyz_encoding_final,
 *   [static_dir_encoding.0], static_sigma, static_rgb.0,
 *   [transient_xyz_encoding_{1..D}.0, transient_xyz_encoding_final,
 *    transient_sigma, transient_rgb.0, [transient_flow_fw.0, transient_flow_bw.0]] */
int nsff_param_count(const NsffModelDesc* desc);

/* Repack the module parameters into MFMA B-operand tiles (DESIGN.md "weight pack").
 * `params`: HOST array of nsff_param_count() device pointers. */
int nsff_pack_weights(const NsffModelDesc* desc, int precision, const float* const* params,
                      void* packed, void* stream);

/* Finer-grained form for callers that re-pack after every optimizer step.  Inference launches (every precision; the
 * exact-fp32 kernel folds everything but the static trunk of view-direction models) read "folded" head rows -- the heads that consume the activation-free *_xyz_encoding_final layers (nerf.py:170,195),
 * pre-multiplied with them, so that those two 256x256 layers are never executed.  nsff_pack_weights builds them;
 * nsff_pack_weights_ex(..., NSFF_PACK_SKIP_FOLD, ...) does not (enough for training forwards, i.e. nsff_field_query
 * with save_* buffers, which execute the layers because the backward pass needs their output), and nsff_fold_heads
 * adds them to such a buffer later.  An inference launch on a buffer without them computes garbage heads.          */
#define NSFF_PACK_SKIP_FOLD 1
int nsff_pack_weights_ex(const NsffModelDesc* desc, int precision, const float* const* params,
                         void* packed, int32_t flags, void* stream);
int nsff_fold_heads(const NsffModelDesc* desc, int precision, const float* const* params, void* packed, void* stream);

/* ---- a1: PosEmbedding.forward (reference nerf.py:17-30) ---- */
int nsff_posenc(const float* x, int64_t n_rows, const float* freqs_host, int n_freqs,
                float* out, void* stream);

/* ---- a2: the two neighbouring-frame gathers of the warp path, embedding_t(clamp(ts + 1, max=max_t)) and
 * embedding_t(clamp(ts - 1, min=0)) (reference rendering.py:218,224), from the table of an nn.Embedding:
 * table (n_table, width) fp32, ts (n) int64 on the device; next / prev (n, width), either may be NULL. */
int nsff_time_rows(const float* table, int64_t n_table, int32_t width, const int64_t* ts, int64_t n, int64_t max_t,
                   float* next, float* prev, void* stream);

/* N1: gradient of those gathers and of embedding_t(ts) itself (rendering.py:162) w.r.t. the table: d_table (n_table, width),
 * every row written, = the rows of g_cur / g_next / g_prev (each (n, width) or NULL) summed by their (clamped) frame index.
 * Replaces three embedding backwards (torch: atomics on ~30 distinct rows) with one deterministic launch. */
int nsff_time_rows_backward(const float* g_cur, const float* g_next, const float* g_prev, const int64_t* ts, int64_t n,
                            int64_t max_t, int64_t n_table, int32_t width, float* d_table, void* stream);

/* ---- a3/a5: fused field query = encode -> trunk(s) -> heads (NeRF.forward) ---- */
typedef struct NsffFieldArgs {
    int64_t n_points;        /* P                                                   */
    int32_t precision;       /* NSFF_PREC_*: must match the packed buffer           */
    int32_t tile_points;     /* F16X3 only: 0 = library default (128-point tiles; 64 points for inference launches below
                                32768 points), 64 = 64-point tiles, 130 = 128-point tiles: the hand-scheduled body
                                (nsff_field_kernel_h3a: one wave per SIMD, resident weights, two 64-point halves) for
                                inference launches it covers, else eight waves of 32 neurons; 131 = 128-point tiles,
                                always the compiler-scheduled eight-wave kernel                                       */
    int32_t pts_per_ray;     /* ray index of point p is p / pts_per_ray             */
    int32_t static_mode;     /* 0 skip, 1 sigma only, 2 rgb+sigma                   */
    int32_t transient_mode;  /* 0 skip, 1 sigma only, 2 rgb+sigma(+flow heads)      */
    int32_t flow_heads;      /* flow heads the caller consumes (0,1,2); the kernel always
                                evaluates every head the model has, this only feeds the
                                algorithmic-FLOP accounting of nsff_prof_collect          */
    /* input A: raw positions, encoded in-kernel (render path) */
    const float* xyz;        /* (P,3) or NULL                                       */
    int32_t n_freqs;         /* of the xyz embedding                                */
    float   freqs[NSFF_MAX_FREQS];
    const float* dir_emb;    /* (n_rays, in_dir) per-ray, needed iff use_viewdir    */
    const float* a_emb;      /* (n_rays, in_a)   per-ray, needed iff in_a>0 && use_viewdir */
    const float* t_emb;      /* (n_rays, in_t)   per-ray, needed iff transient_mode */
    /* input B: rows already embedded by the caller (NeRF.forward API) */
    const float* x_emb;      /* (P, ld_emb) or NULL                                 */
    int32_t ld_emb;
    int32_t off_xyz, off_dir, off_a, off_t;  /* column offsets in x_emb, -1 = absent */
    float*  raw;             /* (P, NSFF_RAW_STRIDE) output                         */
    /* training forward (F16X3, input A): also keep what nsff_field_backward / nsff_weight_grad need.  T = ceil(P/64) point
     * tiles; any of them may be NULL.  NS = 2*D+2 activation slots.  XR / t_row0 / SR: nsff_train_dims.
     *   save_acts : fp16 (NS, T, 4, 256, 16): slot l = ReLU output of static layer l (l < D), slots D+1 .. 2*D the same for
     *               the transient trunk, slot D = static_dir_encoding output (use_viewdir; ABI 30 -- it was slot 2*D+2); slot 2*D+1
     *               (and slot D without view directions: the *_xyz_encoding_final outputs of earlier ABI versions) is never
     *               written: *_final is folded into the heads in training as in inference (slots of a trunk that is not
     *               evaluated stay unwritten too).  Inside a tile: [16-point
     *               group][neuron][point] = the fragment order of the weight-gradient GEMM (K = points);
     *   save_xin  : fp16 (T, 4, XR, 16) trunk input, rows [0,in_xyz) xyz embedding, rows [t_row0, t_row0+in_t) time code
     *               (t_row0 = ceil64(in_xyz); XR = 128 or 256); rows from ceil64 of what the launch encodes up stay unwritten;
     *   save_masks: uint64 (NS, T, 256) ReLU sign bits of every trunk activation, in accumulator order;
     *   save_side : fp16 (T, 4, SR, 16) [dir | a] input of static_dir_encoding (use_viewdir, static_mode 2), rows
     *               [0, in_dir + in_a); rows from ceil64(in_dir + in_a) up stay unwritten (SR = 128 or 256).          */
    void*   save_acts;
    void*   save_xin;
    void*   save_masks;
    void*   save_side;
    /* inference (F16X3, input A), optional: the time code's part of the dynamic trunk's input layers, computed once per ray by
     * nsff_time_bias from the same t_emb rows: (n_rays, t_bias_rows, 256) fp32.  With it -- and pts_per_ray a multiple of 64 --
     * the hand-scheduled kernel multiplies no time-code column (8 of a dynamic trunk's 128 k-steps); results agree with the
     * plain launch to fp32 rounding.  t_emb must be given either way (it is what every other kernel variant reads). */
    const float* t_bias;
    int32_t t_bias_rows;     /* nsff_time_bias_rows(desc), or 0                     */
    int32_t reserved0;
    /* inference (F16X3, input A, use_viewdir models, static_mode 2), optional: what [dir | a] contributes to
     * static_dir_encoding, computed once per ray by nsff_side_bias from the same dir_emb / a_emb rows: (n_rays, 1, 256) fp32.
     * With it -- and pts_per_ray a multiple of 64 -- the static trunk of a view-direction model runs on the hand-scheduled
     * kernel: static_dir_encoding becomes one more 256-wide layer with per-ray bias rows, sigma is accumulated in the epilogue
     * of the last trunk layer.  dir_emb / a_emb must be given either way (every other kernel variant reads them). */
    const float* s_bias;
    int32_t s_bias_rows;     /* 1, or 0                                             */
    /* 0: the library's choice -- large hand-scheduled launches are PERSISTENT (one workgroup per compute unit walking its tiles,
     * nsff_last_field_grid); 1: one workgroup per 128-point tile (bit-identical records).  A persistent launch holds every
     * compute unit until it ends: a caller whose collective kernel runs beside the render stream (the overlapped pixel
     * all-gather of a multi-GPU evaluation, nsff_pl_amd/dist.py::all_gather_pixels_async) asks for 1, so that the collective gets
     * a compute unit at the next tile boundary and a render workgroup never waits behind it for a whole launch. */
    int32_t launch_form;
    /* Training forward for the THREE-PRODUCT backward (nsff_field_backward / nsff_weight_grad* with grad_x3): every saved tile is
     * written twice -- the fp16 value `v = fp16(x)` as before and, save_lo_delta[i] ELEMENTS behind it in the same buffer
     * (i = 0 save_acts, 1 save_xin, 2 save_side; 0 = not wanted), the remainder `fp16(x - v)`: the backward's GEMMs then multiply
     * hi + lo operands as the forward does.  Eight-wave SAVE kernel only (the launch takes it when any delta is set). */
    int64_t save_lo_delta[3];
} NsffFieldArgs;

int nsff_field_query(const NsffModelDesc* desc, const void* packed,
                     const NsffFieldArgs* args, void* stream);

/* ---- a2/a3: what the time code contributes to the dynamic trunk, once per RAY instead of once per point.  Every sample of a
 * ray shares its time code (reference rendering.py:153,168,221,227 repeat it), so for layer 0 and the skip layers -- the layers
 * whose input holds [xyz | t] (nerf.py:163-167) -- the product of the time-code columns is a per-ray vector:
 *     out[ray][i][n] = b_l[n] + sum_j W_l[n][in_xyz + j] * t_rows[ray][j],   l = 0, then the skip layers in ascending order
 * (i = 0 .. nsff_time_bias_rows(desc) - 1), in fp32.  nsff_field_query takes the result as NsffFieldArgs::t_bias.
 * Up to NSFF_MAX_TIME_BIAS_JOBS (model, time rows) pairs per launch: a render_rays call needs the coarse model at t and the fine
 * model at t, t + 1, t - 1.  w[i] / b[i]: weight (256, in_xyz + in_t [+ 256 for a skip layer]) and bias (256) of
 * transient_xyz_encoding_{l_i + 1}, the parameters themselves (PyTorch Linear layout, no pack needed).
 * Time codes wider than 64 columns or with in_t % 4 != 0 are refused (NSFF_ERR_INVALID): the kernel stages 64 columns per ray
 * as float4s, and such models keep their time-code columns on the matrix pipe (nsff_field_query ignores t_bias for them). */
#define NSFF_MAX_TIME_BIAS_JOBS 4
typedef struct NsffTimeBiasJob {
    const NsffModelDesc* desc;
    const float* w[NSFF_MAX_LAYERS];
    const float* b[NSFF_MAX_LAYERS];
    const float* t_rows;     /* (n_rays, in_t), or NULL: index mode (below)         */
    float* out;              /* (n_rays, nsff_time_bias_rows(desc), 256)            */
    /* index mode (t_rows == NULL): the job gathers its rows itself, t_rows[r] = table[clamp(ts[r] + delta)] -- the reference's
     * embedding_t(ts), embedding_t(clamp(ts + 1, max=max_t)), embedding_t(clamp(ts - 1, min=0)) (rendering.py:153,218,224) for
     * delta = 0, +1, -1 (the index is also kept inside the table) -- and leaves them in rows_out (n_rays, in_t) when that is
     * given: one launch instead of a gather, the neighbour-row kernel and this one. */
    const float* table;      /* (n_table, in_t) time-code table                     */
    const int64_t* ts;       /* (n_rays) frame indices                              */
    int64_t n_table, max_t;
    int32_t delta, pad_;
    float* rows_out;         /* (n_rays, in_t) or NULL                              */
} NsffTimeBiasJob;
int nsff_time_bias_rows(const NsffModelDesc* desc);      /* 0: the model has no dynamic trunk */
int nsff_time_bias(const NsffTimeBiasJob* jobs, int32_t n_jobs, int64_t n_rays, void* stream);

/* ---- a4: the random draws of a render_rays call (reference rendering.py:321 perturb, 207 / 213 noise per pass, 128 the two
 * warps, 338-340 the inverse-CDF draws) in ONE launch, bit-identical to torch.rand / torch.randn of the same generator state:
 * job j fills out[0, numel) with what a torch kernel of `grid` blocks of 256 threads -- ATen's launch geometry for numel
 * elements: min(#CU * (max threads per CU / 256), ceil(numel / 256)) -- started at Philox offset `offset` (a multiple of 4) of
 * `seed` would write; the caller advances the generator by ((numel - 1) / (1024 grid) + 1) * 4 per job, as torch does.
 * kind 0: uniform [0, 1) (torch.rand), 1: standard normal (torch.randn).  */
#define NSFF_MAX_RNG_JOBS 12
typedef struct NsffRngJob {
    float*   out;
    int64_t  numel;
    uint64_t offset;
    int32_t  kind;
    uint32_t grid;
} NsffRngJob;
int nsff_rng_draws(const NsffRngJob* jobs, int32_t n_jobs, uint64_t seed, void* stream);
/* The same launch also makes the coarse depths (reference rendering.py:314-324, 332; nsff_coarse_samples is the stand-alone
 * form) from the stratified-sampling draw, where that draw is made: job `job` is the uniform (n_rays, n_samples) draw of
 * rendering.py:321 (its `out` may be NULL: nobody else reads it), zs / xyz as nsff_coarse_samples writes them (perturb > 0). */
typedef struct NsffRngCoarse {
    const float* rays;       /* (n_rays, 6)                       */
    const float* z_lin;      /* (n_samples)                       */
    float*       zs;         /* (n_rays, n_samples)               */
    float*       xyz;        /* (n_rays, n_samples, 3)            */
    int32_t      n_samples;
    float        perturb;
    int32_t      job;
    int32_t      pad_;
} NsffRngCoarse;
int nsff_rng_draws_coarse(const NsffRngJob* jobs, int32_t n_jobs, uint64_t seed, const NsffRngCoarse* coarse, void* stream);

/* ---- a3: the same for a view-direction model's per-ray inputs (reference nerf.py:183-185, rendering.py:153-172 repeat the
 * direction embedding and the appearance code over a ray's samples):
 *     out[ray][n] = b_fold[n] + sum_j W_dir[n][256 + j] * [dir_rows[ray] | a_rows[ray]][j]
 * with W_dir = static_dir_encoding's weight (256, 256 + in_dir + in_a), the parameter itself, and b_fold = W_dir[:, :256] b_final
 * + b_dir from the F16X3 packed buffer of an inference pack (nsff_pack_weights / nsff_fold_heads).  fp32, columns in ascending
 * order.  a_rows may be NULL iff in_a == 0.  nsff_field_query takes the result as NsffFieldArgs::s_bias. */
int nsff_side_bias(const NsffModelDesc* desc, const void* packed_f16x3, const float* w_dir, const float* dir_rows,
                   const float* a_rows, int64_t n_rays, float* out, void* stream);

/* ---- N1: backward of the field query (training).  Mixed precision: fp16 MFMA operands, fp32 accumulation;
 * every point's gradient row is normalised by its own power of two (block floating point), weight-gradient
 * operands are expressed on one global power-of-two scale G = 2^floor(log2(4096 / *gmax)).
 *
 * nsff_bwd_packed_bytes / nsff_pack_weights_bwd: the TRANSPOSED fp16 weight tiles the data-gradient chain
 * streams (same parameter order as nsff_pack_weights).
 * nsff_field_backward: d_raw (P,16) -> d(trunk input) and the pre-activation gradients of every layer:
 *   dpre : fp16 (NS, T, 4, 256, 16)  slot t*(D+1)+l = trunk t (0 static, 1 transient) layer l < D (slot l = D, *_final, is
 *          never written: the layer is folded into the heads), slot D = static_dir_encoding (use_viewdir); values = true
 *          gradient * G, fragment order as save_acts;
 *   dhead: fp16 (2, T, 4, 32, 16) head pre-activation gradients * G, rows 0..15: static rgb(3) sigma(1);
 *          transient rgb(3) sigma(1) fw(3) bw(3); rows 16..31: the fp16 rounding remainder of rows 0..15 (the head
 *          weight / bias gradients are the sum of both halves);
 *   d_xin: fp32 (P, XR) true gradient w.r.t. the transient trunk input (rows as save_xin), or NULL;
 *   d_side: fp32 (P, SR) true gradient w.r.t. the [dir | a] input of static_dir_encoding (rows as save_side), or NULL.
 * nsff_train_dims: XR (xin_rows), t_row0 and SR (side_rows) of a model -- 128 unless ceil64(in_xyz) + ceil64(in_t) > 128
 * (resp. in_dir + in_a > 128), then 256.  Any skip list the forward takes is differentiated (nerf.py:34-40,163-167). */
int nsff_train_dims(const NsffModelDesc* desc, int32_t* xin_rows, int32_t* t_row0, int32_t* side_rows);
int nsff_bwd_packed_bytes(const NsffModelDesc* desc, size_t* bytes);
int nsff_pack_weights_bwd(const NsffModelDesc* desc, const float* const* params, void* packed, void* stream);
/* ... given the F16X3 forward pack of the SAME weights (nsff_pack_weights with folded heads), whose fp32 scratch already holds the
 * folded products W_head W_final the transposed tiles need (else they are multiplied here); fwd_packed may be NULL. */
int nsff_pack_weights_bwd_ex(const NsffModelDesc* desc, const float* const* params, void* packed, const void* fwd_packed, void* stream);

typedef struct NsffFieldBwdArgs {
    int64_t n_points;
    int32_t static_mode;        /* 0 skip, 2 rgb+sigma (as in the forward call)            */
    int32_t transient_mode;     /* 0 skip, 2                                                */
    const float* d_raw;         /* (P, NSFF_RAW_STRIDE) gradient w.r.t. the raw record      */
    const float* raw;           /* (P, NSFF_RAW_STRIDE) forward outputs (activation derivatives) */
    const float* gmax;          /* device float[16]: max |d_raw| per record column (nsff_absmax_raw): each trunk's fragments are on
                                 * the power-of-two scale of its largest column, every head row of dhead on its own        */
    const void*  masks;         /* save_masks of the forward call                            */
    void*  dpre;                /* OUT */
    void*  dhead;               /* OUT */
    float* d_xin;               /* OUT or NULL                                               */
    float* d_side;              /* OUT or NULL (use_viewdir models, static_mode 2)           */
    int64_t dpre_lo_delta;      /* 0: one fp16 product per multiply-accumulate (the measured path).  Otherwise THREE, as the forward
                                 * multiplies: gradient tiles and weights as fp16 value + fp16 remainder, every pre-activation-gradient
                                 * tile written twice -- dpre as above and its remainder this many ELEMENTS behind it (multiple of 8) --
                                 * for nsff_weight_grad* jobs with a_lo_delta set.  The forward of such a step saves its activations
                                 * the same way (NsffFieldArgs::save_lo_delta).  Gradients then match the reference's fp32 ones to
                                 * ~1e-5 instead of ~1e-3; the chain runs at about a third of the speed. */
} NsffFieldBwdArgs;
int nsff_field_backward(const NsffModelDesc* desc, const void* packed_bwd, const NsffFieldBwdArgs* args, void* stream);
/* Which kernel the last nsff_field_backward launch took: 2 = both (a view-direction model's launch of both trunks: the static trunk
 * on nsff_field_bwd_kernel, the dynamic one on the hand-scheduled body, as two launches); 1 = nsff_field_bwd_kernel_h3b, the hand-scheduled body (128-point
 * workgroups, one wave per SIMD, resident transposed weights, epilogues / fragment copies / refills riding in the other half's MFMA
 * gaps: tools/h3asm/gen_bwd.py) -- launches with an even number of 64-point tiles whose trunks it executes (no view-direction static
 * trunk, at most one skip layer with a trunk-input gradient, none at the last layer); 0 = the kernel nsff_field_bwd_kernel -- compiler-scheduled,
 * 64-point workgroups; NSFF_BWD_KERNEL=c forces it.  Both leave bit-identical dpre / dhead / d_xin. */
int nsff_last_bwd_kernel(void);
/* Workgroups of the last hand-scheduled data-gradient launch (0: none since the last nsff_field_backward).  Launches that give
 * every compute unit at least two (tile, trunk) items run PERSISTENT: one workgroup per compute unit, further items from a device
 * counter, the next item's records brought into LDS behind the current item's body; NSFF_BWD_PERSIST=0: one workgroup per item. */
int nsff_last_bwd_grid(void);
/* Host-only (no GPU): the hand-scheduled body's phase program for one trunk of `desc` (dynamic: the transient trunk, with or without
 * the trunk-input gradient) at n_tiles 64-point tiles -> out[max_phases][8] uint32 descriptors; seg_offsets (or NULL): byte offsets of
 * the trunk's step segments in the transposed pack.  Returns the number of descriptors, 0 when the body does not cover the trunk. */
int nsff_field_bwd_phase_program(const NsffModelDesc* desc, int32_t dynamic, int32_t want_xin, int64_t n_tiles, uint32_t* out,
                                 int32_t max_phases, uint32_t* seg_offsets, int32_t max_segs);

/* Host-only, as nsff_field_launch_plan: what nsff_field_backward would launch on a device of n_cus compute units.
 * kernel_override: 'c' as NSFF_BWD_KERNEL=c, else 0; persist: 0 as NSFF_BWD_PERSIST=0, else 1.  Returns the nsff_last_bwd_kernel
 * code (0 c, 1 h3b, 2 c+h3b, 3 x3) or the call's negative error (n_points == 0: NSFF_OK, no record).  out: max_launches (>= 2)
 * records of NSFF_PLAN_WORDS int32: [0] NSFF_BWD_LAUNCH_* kernel, [1] workgroups (a persistent launch falls back to [4] when no
 * counter word can be had), [2] threads, [3] trunks (1 static, 2 dynamic, 3 both), [4] (tile, trunk) items, [5] 1 = persistent: the
 * launch takes an item counter, [6] steps of the launch's step program, [11] FNV-1a of the argument bytes (counter null). */
#define NSFF_BWD_LAUNCH_C    1   /* nsff_field_bwd_kernel      */
#define NSFF_BWD_LAUNCH_H3B  2   /* nsff_field_bwd_kernel_h3b  */
#define NSFF_BWD_LAUNCH_X3   3   /* nsff_field_bwd_kernel_x3   */
int nsff_field_bwd_launch_plan(const NsffModelDesc* desc, const NsffFieldBwdArgs* args, int32_t n_cus, int32_t kernel_override,
                               int32_t persist, int32_t* out, int32_t max_launches);

/* d_xin (P, xin_rows) of nsff_field_backward -> gradient w.r.t. the points (derivative of PosEmbedding, reference
 * nerf.py:17-30) and w.r.t. the per-ray time codes (sum over the ray's pts_per_ray consecutive points, the repeat of
 * rendering.py:168).  d_xyz (P,3) / d_t (n_rays, in_t): either may be NULL.  freqs_host: HOST array.                */
int nsff_field_input_backward(const float* d_xin, int32_t xin_rows, int32_t t_row0, const float* xyz, int64_t n_rays,
                              int32_t pts_per_ray, const float* freqs_host, int32_t n_freqs, int32_t in_t, float* d_xyz,
                              float* d_t, void* stream);

/* Batched weight-gradient GEMMs, K = points:  out_j = (1/G) * A_j^T . B_j over all point tiles, G as above.
 * A_j: fp16 fragment-major (T,4,a_rows,16), a_rows in {256, 32};  B_j: (T,4,b_rows,16), b_rows in {256, 128}.
 * Split-K: every job is cut into about n_splits tile ranges (rounded per job shape so that the workgroups of equally
 * shaped jobs fill whole rounds of the 256 CUs; heads: 8x as many) whose partial sums go to `scratch`
 * (nsff_weight_grad_scratch floats) and are summed, scaled and written by a second launch to
 *   out + out_off[j]  : fp32 a_rows_j x b_rows_j (row-major),     bias + 256*j : fp32 row sums of A_j (bias gradients).
 * `jobs` is a HOST array.                                                                                      */
typedef struct NsffWgradJob {
    const void* a;  const void* b;
    int32_t a_rows, b_rows;
    int64_t out_off;            /* floats */
    int32_t trunk, pad_;        /* 0 static / 1 dynamic: which of the two scales (gmax[trunk]) the job's A operand is on */
    int64_t a_lo_delta, b_lo_delta;   /* 0 / 0: one fp16 product per multiply-accumulate.  Three products (the launches behind a
                                 * nsff_field_backward with dpre_lo_delta): ELEMENTS from a / b to their remainder planes (dpre's twin,
                                 * the forward's save_lo_delta twins); every job of a call or none; a_lo_delta stays 0 for the 32-row
                                 * head jobs, whose A carries its remainder rows itself */
} NsffWgradJob;
int64_t nsff_weight_grad_scratch(const NsffWgradJob* jobs, int32_t n_jobs, int64_t n_tiles, int32_t n_splits);
int nsff_weight_grad(const NsffWgradJob* jobs, int32_t n_jobs, int64_t n_tiles, int32_t n_splits,
                     float* scratch, float* out, float* bias, const float* gmax, void* stream);

/* The same GEMMs, but the second launch ACCUMULATES straight into the parameters' gradient memory (what autograd's
 * AccumulateGrad does for torch.nn.Linear's grad_weight / grad_bias): for every map entry
 *   grad_base[dst] += (1/G) * (S(job_a, e_a) + S(job_b, e_b)),      S(j, e) = sum over the splits of job j's partials,
 * e < a_rows*b_rows: element e of out_j (row-major);  e >= a_rows*b_rows: row sum (bias gradient) e - a_rows*b_rows;
 * job_b < 0: no second term (it carries the fp16-remainder rows of the head gradients).  Every dst must appear at most
 * once (one owner per gradient element: the result is deterministic).  `map` is a DEVICE array, 16-byte aligned;
 * jobs[].out_off is ignored.                                                                                       */
typedef struct NsffGradMapEntry {
    int32_t dst;                /* floats from grad_base */
    int32_t e_a, e_b;
    int16_t job_a, job_b;
} NsffGradMapEntry;
int nsff_weight_grad_accumulate(const NsffWgradJob* jobs, int32_t n_jobs, int64_t n_tiles, int32_t n_splits, float* scratch,
                                const NsffGradMapEntry* map, int64_t n_map, float* grad_base, const float* gmax, void* stream);

/* nsff_weight_grad_accumulate with a second destination: map entries with dst < 0 STORE their value at aux[-(dst + 1)]
 * -- dense sums of the jobs the FOLDED parameters are made of: *_xyz_encoding_final is never executed as a layer (the heads that
 * read it are evaluated as (W_head W_final) h), so its gradient and the heads' are small matrix products of the folded heads'
 * gradient G = sum_p dpre_p (x) h_p:  dW_head = G W_final^T + gb (x) b_final,  dW_final = W_head^T G,  db_final = W_head^T gb. */
int nsff_weight_grad_accumulate_aux(const NsffWgradJob* jobs, int32_t n_jobs, int64_t n_tiles, int32_t n_splits, float* scratch,
                                    const NsffGradMapEntry* map, int64_t n_map, float* grad_base, float* aux, const float* gmax,
                                    void* stream);

/* One launch that turns the folded heads' gradient into the gradients of *_xyz_encoding_final and of the heads that read it
 * and ADDS them to the parameters' gradient memory:  g (32, 256) / gb (32): the dense sum / row sums of the heads' job (rows r
 * and 16 + r = fp16 value + rounding remainder of folded row r < n_rows <= 16);
 *   d_w_head[r] += G[r] W_final^T + gb[r] b_final,  *d_b_head[r] += gb[r],  d_w_final += W_head^T G,  d_b_final += W_head^T gb. */
typedef struct NsffFoldGradArgs {
    int32_t n_rows, pad_;
    const float* g; const float* gb;
    const float* w_final; const float* b_final;        /* (256, 256), (256) */
    const float* w_head[16];                           /* row r of the heads' weights: 256 floats */
    float* d_w_head[16]; float* d_b_head[16];
    float* d_w_final; float* d_b_final;
} NsffFoldGradArgs;
int nsff_fold_grads(const NsffFoldGradArgs* args, void* stream);

/* The same algebra for a folded layer of ANY height (n_rows <= 256) whose weights are one strided matrix -- the view-direction
 * layer static_dir_encoding (reference models/nerf.py:83-91,183-186: it reads [*_final | dir | a]; its first 256 columns are the
 * folded part, ld_head = 256 + in_dir + in_a) -- and for callers that want the results as tensors instead of accumulated
 * (accumulate = 0: every output element is STORED):
 *   g (n_rows, 256) [+ g2: a second summand, the fp16 rounding-remainder rows of a heads' job, or NULL], gb (n_rows) [+ gb2]
 *   d_w_head[r * ld_dhead + o] (+)= sum_i G[r][i] W_final[o][i] + gb[r] b_final[o]      d_b_head[r] (+)= gb[r]
 *   d_w_final[o][i] (+)= sum_r W_head[r * ld_head + o] G[r][i]                          d_b_final[o] (+)= sum_r W_head[r * ld_head + o] gb[r]
 * Two launches (rows of the head layer / neurons of *_final); fp32 FMAs in a fixed order: deterministic.  Every pointer needs
 * 4-byte alignment only, w_final included (the callers pass views of a flat parameter buffer without padding; off 16 bytes
 * its rows are read float by float, the same products in the same order: the same bits).  This is what ran
 * through torch.addmm / `@` (rocBLAS) for view-direction models and for gradients returned as tensors until round 5.       */
typedef struct NsffFoldDenseArgs {
    int32_t n_rows, accumulate;
    int32_t ld_head, ld_dhead;
    const float* g; const float* g2; const float* gb; const float* gb2;
    const float* w_head; const float* w_final; const float* b_final;
    float* d_w_head; float* d_b_head; float* d_w_final; float* d_b_final;
} NsffFoldDenseArgs;
int nsff_fold_grads_dense(const NsffFoldDenseArgs* args, void* stream);

/* out[0] = max |x[i]| (0 for n == 0): the device scalar `gmax` of nsff_field_backward / nsff_weight_grad without a
 * host round trip (replaces d_raw.abs().max()).  x 16-byte aligned.                                                */
int nsff_absmax(const float* x, int64_t n, float* out, void* stream);
/* out16[c] = max |d_raw[:, c]| for the 16 floats of a record: the `gmax` vector of nsff_field_backward / nsff_weight_grad*.  A trunk's
 * fragments (dpre) are on the scale of its largest column (static: 0..3, dynamic: 4..13), every head row of dhead on its own: in a
 * real NSFF step the columns' gradients are 10^6-10^7 apart (the 2D flow terms of the loss are in pixels); on a common scale the
 * smaller ones' fp16 fragments fall into and below the subnormal range -- a bit or two, then zero (round 6, golden g20:
 * static weight gradients 40-70 % too small at 512 rays, transient_sigma.weight 25 %). */
int nsff_absmax_raw(const float* d_raw, int64_t n_points, float* out16, void* stream);

/* ---- N1: the optimizer step: torch.optim.Adam(lr, betas, eps, weight_decay) as the reference builds it
 * (utils/__init__.py:45-47 get_optimizer, used by train.py:140-146), amsgrad off, on flat fp32 buffers of n elements
 * (n % 4 == 0, 16-byte aligned):  g' = g + weight_decay * p;  m = lerp(m, g', 1 - beta1);  v = beta2 * v + (1 - beta2) * g'^2;
 * p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
 * state: DEVICE float[4]; state[0] = number of steps taken so far (zero it once; the call increments it), state[1..2]
 * scratch.  lr: DEVICE scalar.  Two launches, no host round trip: capturable into a hipGraph.                      */
int nsff_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                   const float* lr, double beta1, double beta2, double eps, double weight_decay, void* stream);

/* The same step with torch.optim.Adam's treatment of parameters that receive no gradient (`if p.grad is None: continue`,
 * what train.py's optimizer does for a head the step never used): the flat buffers are n_seg consecutive parameter tensors,
 * tensor k = elements [seg_start[k], seg_start[k+1]) (DEVICE int64[n_seg + 1], ascending, seg_start[0] = 0); a tensor whose
 * gradient slice is identically zero this step keeps its values AND its moments (no weight decay, no moment decay);
 * seg_used: DEVICE int32[n_seg] scratch (receives the per-tensor flags).  One memset + three launches, capturable.
 * seg_start == NULL (with seg_used == NULL): every element is updated, exactly nsff_adam_step.                          */
int nsff_adam_step_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                            const float* lr, double beta1, double beta2, double eps, double weight_decay,
                            const int64_t* seg_start, int n_seg, int32_t* seg_used, void* stream);

/* The reference's other optimizers (utils/__init__.py:42-50 get_optimizer, --optimizer sgd / radam), on the same flat buffers
 * with the same conventions: n % 4 == 0, 16-byte aligned, lr a DEVICE scalar, capturable; seg_start / seg_used both NULL (every
 * element is updated) or both given (the segment form of nsff_adam_step_segments: a tensor whose gradient slice is identically
 * zero this step keeps its value and its state, torch's `if p.grad is None: continue`).
 *
 * torch.optim.SGD(lr, momentum, weight_decay), dampening 0, no Nesterov:  g' = g + weight_decay * p;
 * buf = momentum * buf + g';  p -= lr * buf.  momentum_buf starts at zero (that IS torch's first-step buf = g').  With
 * momentum == 0 the step is p -= lr * g' and momentum_buf is neither read nor written (NULL is fine).
 * state: DEVICE float[4]; state[0] = number of steps taken so far (the call increments it; the arithmetic does not use it).
 * One launch (segment form: one memset + two launches).                                                                  */
int nsff_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float* state, const float* lr,
                  double momentum, double weight_decay, const int64_t* seg_start, int n_seg, int32_t* seg_used, void* stream);

/* RAdam as torch.optim.RAdam(lr, betas, eps, weight_decay, decoupled_weight_decay=True) evaluates it:  p *= 1 - lr * weight_decay;
 * m, v as Adam;  rho_inf = 2 / (1 - beta2) - 1,  rho_t = rho_inf - 2 t beta2^t / (1 - beta2^t);
 * rho_t > 5:  p -= lr / (1 - beta1^t) * r_t * m * sqrt(1 - beta2^t) / (sqrt(v) + eps),
 *             r_t = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t));   otherwise  p -= lr / (1 - beta1^t) * m.
 * state: DEVICE float[8]; state[0] = number of steps taken so far (zero it once; the call increments it), state[1..4] scratch
 * (the per-step scalars, evaluated in double on the device from state[0]).  Two launches (segment form: + memset + one).  */
int nsff_radam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                    const float* lr, double beta1, double beta2, double eps, double weight_decay,
                    const int64_t* seg_start, int n_seg, int32_t* seg_used, void* stream);

/* ---- N1: the training objective NeRFWLoss (reference losses.py:8-28, 31-171) on the render dict, NSFF train-mode
 * configuration (flows + disocclusion present, topk == 1, no per-ray weights, thickness == 1), every term reduced to
 * its scalar.  mode 1: terms[11] = col_l, disp_l, entropy_l, cross_entropy_l, flow_fw_l, flow_bw_l, pho_l, cyc_l,
 * reg_temp_sm_l, reg_min_l, reg_sp_sm_l (six launches; `stats`, `per_ray` and `coef` receive what mode 2 re-uses).
 * mode 2: g_* = gradient of sum_k term_w[k] * term_k w.r.t. the tensor of the same name (two launches).
 * Reduction of a term (losses.py:162-169): its per-ray values v_n (times weights[n] when given) over its population -- every
 * ray, or for the two flow terms the M rays whose projection is valid -- are reduced to the mean of the K LARGEST,
 * K = int(topk * M) for topk < 1, else K = M (the plain mean; 0 for an empty population).  `thickness` > 1 dilates the
 * detached transient weights of cross_entropy_l with a 1 x thickness box filter, zero padded (losses.py:91-95).
 * n_rays <= 4096 (nsff_nerfw_loss) or <= NSFF_LOSS_MAX_RAYS (nsff_nerfw_loss_ex, below).
 * hyper (device): lambda_geo_d, lambda_geo_f, cross-entropy weight, lambda_reg, lambda_ent.                       */
typedef struct NsffLossArgs {
    int64_t n_rays; int32_t n_samples; int32_t n_keep;   /* n_keep = int(n_samples * z_far): samples the regularisers see */
    int32_t n_frames; int32_t max_t;
    double  topk;                                        /* --topk (opt.py:80): >= 1 = plain means                 */
    int32_t thickness; int32_t pad_;                     /* --thickness (opt.py:49), >= 1                          */
    /* render dict */
    const float* rgb_fine; const float* rgb_coarse;      /* (N,3); coarse pair may be NULL                         */
    const float* depth_fine; const float* depth_coarse;  /* (N)                                                    */
    const float* t_weights; const float* s_weights;      /* (N,S) transient_weights_fine, static_weights_fine      */
    const float* xyz_fw; const float* xyz_bw;            /* (N,3)                                                  */
    const float* rgb_fw; const float* rgb_bw;            /* (N,3)                                                  */
    const float* disocc_fw; const float* disocc_bw;      /* (N)                                                    */
    const float* disoccs_fw; const float* disoccs_bw;    /* (N,S)                                                  */
    const float* xyzs_fw_bw; const float* xyzs_bw_fw;    /* (N,S,3)                                                */
    const float* xyzs_fine; const float* xyzs_fw; const float* xyzs_bw;   /* (N,S,3)                               */
    /* targets / camera buffers (train.py:136-138) */
    const float* rgbs; const float* disps;               /* (N,3), (N)                                             */
    const int64_t* ts; const int64_t* cam_ids;           /* (N); cam_ids may be NULL (= 0)                         */
    const float* uv_fw; const float* uv_bw;              /* (N,2)                                                  */
    const float* Ks; const float* Ps;                    /* (n_cam,3,3), (n_cam,n_frames,3,4)                      */
    const float* hyper;                                  /* device, 5 floats                                       */
    float* stats;                                        /* device, 24 floats: written by mode 1, read by mode 2   */
    float* terms;                                        /* OUT mode 1: 11 floats                                  */
    const float* term_w;                                 /* mode 2: 11 upstream scalars (device)                   */
    const float* weights;                                /* (N) per-ray loss weights (hard sampling) or NULL       */
    float* per_ray;                                      /* device (11, N): weighted per-ray values, mode 1 OUT; < 0 marks a
                                                            ray outside a flow term's population                    */
    float* coef;                                         /* device (11, N): d term_k / d v_n = weights[n] * [n selected] / K,
                                                            mode 1 OUT, mode 2 IN                                   */
    float* g_rgb_fine; float* g_rgb_coarse; float* g_depth_fine; float* g_depth_coarse;
    float* g_t_weights; float* g_s_weights; float* g_xyz_fw; float* g_xyz_bw; float* g_rgb_fw; float* g_rgb_bw;
    float* g_xyzs_fw_bw; float* g_xyzs_bw_fw; float* g_xyzs_fw; float* g_xyzs_bw;
} NsffLossArgs;
int nsff_nerfw_loss(const NsffLossArgs* args, int mode, void* stream);
/* The same objective for up to NSFF_LOSS_MAX_RAYS rays: the medians and the top-k selection, which nsff_nerfw_loss ranks inside
 * one workgroup's LDS (hence its 4096 rays), run as an exact radix select over many workgroups -- same definition of the result
 * (lower median, the K largest, ties to the lower index), any n_rays from 1.  `work`: device memory of at least
 * nsff_nerfw_loss_work_bytes(n_rays) bytes, 16-byte aligned, owned by the caller, contents irrelevant before and after a call
 * (mode 2 does not touch it); a null (NSFF_ERR_NULL), misaligned (NSFF_ERR_ALIGN) or too small workspace and n_rays outside
 * 1 .. NSFF_LOSS_MAX_RAYS (NSFF_ERR_INVALID) are refused before anything is launched.  Asynchronous on `stream`, allocates nothing, capturable.  nsff_nerfw_loss_work_bytes is host
 * arithmetic: positive and non-decreasing up to the bound, 0 outside it.
 * nsff_last_loss_path(): which of the two the last loss call of this process launched -- 0 none yet, 1 rank counting
 * (nsff_nerfw_loss), 2 radix select (nsff_nerfw_loss_ex).                                                          */
#define NSFF_LOSS_MAX_RAYS 1048576
size_t nsff_nerfw_loss_work_bytes(long long n_rays);
int nsff_nerfw_loss_ex(const NsffLossArgs* args, int mode, void* work, size_t work_bytes, void* stream);
int nsff_last_loss_path(void);

/* ---- a4: coarse sample placement (reference rendering.py:314-324,332) ----
 * zs[n][i] = z_lin[i]                                   (perturb == 0)
 *          = lower + (upper-lower) * perturb * rnd[n][i] (perturb > 0)
 * xyz[n][i] = o[n] + d[n]*zs[n][i]                                             */
int nsff_coarse_samples(const float* rays, int64_t n_rays, const float* z_lin, int32_t n_samples,
                        float perturb, const float* perturb_rand,
                        float* zs, float* xyz, void* stream);

/* ---- a9: sample_pdf x{1,2} + merge + sort (reference rendering.py:10-49,335-348,359) ----
 * weights_* are the (n_rays, n_samples) coarse weights (the [1:-1] slice is taken here).
 * u_* : (n_importance) when u_per_ray==0 (deterministic linspace), else (n_rays, n_importance).
 * zs_fine: (n_rays, n_samples + k*n_importance) sorted ascending, k = 1 + (weights_transient!=NULL)
 * xyz_fine = o + d*zs_fine.  samples_static/transient (n_rays,n_importance) optional. */
int nsff_fine_samples(const float* rays, int64_t n_rays, const float* z_lin, const float* zs_coarse,
                      int32_t n_samples, int32_t n_importance,
                      const float* weights_static, const float* weights_transient,
                      const float* u_static, const float* u_transient, int32_t u_per_ray,
                      float* samples_static, float* samples_transient,
                      float* zs_fine, float* xyz_fine, void* stream);

/* standalone sample_pdf(bins, weights, N_importance) with explicit u (reference rendering.py:10-49) */
int nsff_sample_pdf(const float* bins, const float* weights, int64_t n_rays, int32_t n_bins_minus1,
                    const float* u, int32_t n_importance, int32_t u_per_ray, float eps,
                    float* samples, void* stream);

/* ---- a8 (first half): xyzs_fw = xyz + flow_fw, xyzs_bw = xyz + flow_bw with the
 * z > z_far flow zeroing (reference rendering.py:187-188,218,224) ---- */
int nsff_warp_points(const float* raw, const float* xyz, const float* zs, int64_t n_points,
                     float z_far, float* xyz_fw, float* xyz_bw, void* stream);

/* ---- N3 (step before the path): NDC camera rays of a pinhole frame, generated on the device
 * (reference datasets/ray_utils.py:7-106 via datasets/monocular.py:268-276).
 * K4_host = {fx, fy, cx, cy}, c2w_host = row-major (3,4), both HOST pointers; pixel p = row*W + col;
 * rays: (n_pixels, 6) = NDC origin | NDC direction for pixels [first_pixel, first_pixel+n_pixels). */
int nsff_frame_rays(const float* K4_host, const float* c2w_host, int32_t H, int32_t W, float near, float shift_near,
                    int64_t first_pixel, int64_t n_pixels, float* rays, void* stream);

/* ---- the training split's ray bank, built on the device (reference datasets/monocular.py:136-184): the records of frames
 * [first_frame, first_frame + frame_count) in ONE launch, written to records[frame] in the NSFF_RAY_RECORD column layout:
 * NDC ray 0-5 (the arithmetic of nsff_frame_rays, bit for bit), rgb 6-8, (float) frame 9, disparity 10, mask 11,
 * uv + flow_fw 12-13, uv + flow_bw 14-15 with uv = (pix % W, pix / W).  Every input holds all n_frames frames, already at the
 * target resolution: images (F,H,W,3) and masks (F,H,W) as uint8 (converted by a true division by 255, torchvision's ToTensor)
 * or fp32, disps (F,H,W) fp32, flow_fw / flow_bw (F,H,W,2) fp32 or NULL (= zero flow).  Frame n_frames-1 gets zero forward flow
 * and frame 0 zero backward flow whatever the flow tensors hold there (monocular.py:167-179).
 * frame_table: device (n_frames, NSFF_FRAME_TABLE) fp32 = row-major c2w (3,4) | shift_near = -min(-1, c2w[2][3]) | 3 unused.
 * n_pixels (the records' second dimension) must equal H * W and be below 2^31; frame_count <= 65535.  records 16-byte, flows 8-byte aligned (NSFF_ERR_ALIGN). */
#define NSFF_FRAME_TABLE     16
typedef struct NsffRayRecordArgs {
    int32_t n_frames, H, W;
    int32_t first_frame, frame_count;
    int32_t image_u8, mask_u8;  /* 1: uint8 input, 0: fp32                                  */
    float   fx, fy, cx, cy, near;
    int64_t n_pixels;
    const void*  images;
    const float* disps;
    const void*  masks;
    const float* flow_fw;
    const float* flow_bw;
    const float* frame_table;
    float*       records;       /* (n_frames, n_pixels, NSFF_RAY_RECORD)                    */
} NsffRayRecordArgs;
int nsff_ray_records(const NsffRayRecordArgs* args, void* stream);

/* ---- resizing decoded frames to the training resolution (csrc/resize.hip): the four resize statements of
 * the reference's dataset constructor, datasets/monocular.py:98-99, 146-147, 158-163, 168-176 and datasets/flowlib.py:320-338.
 * A resize is separable: one table per axis says, for each output index, which source indices it reads and with which weights.
 * The tables are built on the HOST, in double, by nsff_resize_table and applied on the device by nsff_frame_resize.
 *   NSFF_RESIZE_LANCZOS_U8   PIL Image.resize(.., LANCZOS) on 8-bit pixels: Pillow's precompute_coeffs + normalize_coeffs_8bpc.
 *                            scale = n_in / n_out, fs = max(scale, 1), support = 3 fs, ksize = 2 ceil(support) + 1; output i:
 *                            c = (i + 0.5) scale, start = max((int)(c - support + 0.5), 0), count = min((int)(c + support + 0.5),
 *                            n_in) - start, w_j = L((j + start - c + 0.5) (1 / fs)) with L(x) = sinc(x) sinc(x / 3) on -3 <= x < 3,
 *                            divided by their sum where that is non-zero, then int32 (int)(+-0.5 + w 2^22) (sign of w), zero-padded
 *                            to ksize.  Tables wider than NSFF_RESIZE_MAX_KSIZE = 2 ceil(3 * 8) + 1 (a downscale beyond 8x) are
 *                            NSFF_ERR_UNSUPPORTED; every upscale has ksize 7.
 *   NSFF_RESIZE_NEAREST_PIL  PIL Image.resize(.., NEAREST): a = n_in / n_out, x = 0.5 a, index = (int)x, x += a (the running sum).
 *   NSFF_RESIZE_NEAREST_CV   OpenCV resizeNN: min(floor(i * (1 / (n_out / n_in))), n_in - 1).
 *   NSFF_RESIZE_LINEAR_CV    OpenCV fp32 INTER_LINEAR: fx = (float)((i + 0.5)(n_in / n_out) - 0.5), sx = floor(fx), fx -= sx; sx < 0:
 *                            sx = 0, fx = 0; sx >= n_in - 1: sx = n_in - 1, fx = 0; taps sx and min(sx + 1, n_in - 1) (count = their
 *                            number), weights the fp32 pair (1 - fx, fx).
 * nsff_resize_ksize: weights per output index (1 for the two nearest rules -- they have none --, 2 for linear), or an error.
 * nsff_resize_table: start, count (n_out) int32 and weights (n_out, ksize) int32 (Lanczos) / fp32 (linear) / unused, NULL allowed
 * (nearest), all HOST memory; no GPU work. */
#define NSFF_ERR_UNSUPPORTED     -5   /* a valid request outside what the kernels are built for */
#define NSFF_RESIZE_LANCZOS_U8    0
#define NSFF_RESIZE_NEAREST_PIL   1
#define NSFF_RESIZE_NEAREST_CV    2
#define NSFF_RESIZE_LINEAR_CV     3
#define NSFF_RESIZE_MAX_KSIZE    49
int nsff_resize_ksize(int32_t filter, int32_t n_in, int32_t n_out);
int nsff_resize_table(int32_t filter, int32_t n_in, int32_t n_out, int32_t* start, int32_t* count, void* weights);

/* n_frames frames (F, src_h, src_w, C) -> (F, dst_h, dst_w, C), channels last, with the DEVICE tables of the two axes.  One launch,
 * asynchronous on `stream`, no allocation, no synchronisation, no scratch: capturable.
 *   LANCZOS_U8   uint8, C = 1..3.  Pillow's two 8-bit passes, horizontal first, each acc = 2^21 + sum pixel * k in int32 and
 *                clamp(acc >> 22, 0, 255); a pass whose size does not change is skipped.  The intermediate image between the
 *                passes exists only in LDS, as uint8, per output tile.
 *   NEAREST_PIL  uint8, C = 1..3;  NEAREST_CV  fp32, C = 1..3: dst[y][x] = src[y_start[y]][x_start[x]].
 *   LINEAR_CV    fp32, C = 1..2: h_r = s[r][x0] wx0 + s[r][x1] wx1 for the two rows, v = h_0 wy0 + h_1 wy1, dst = v * ratio[c];
 *                every step one fp32 operation (flowlib.resize_flow: ratio = {(float)(w / ws), (float)(h / hs)}).
 * ksize_x / ksize_y must be nsff_resize_ksize of the axis (else NSFF_ERR_INVALID; beyond the limit NSFF_ERR_UNSUPPORTED);
 * n_frames <= 65535, 1 <= h * w * C < 2^31 on both sides; a missing pointer is NSFF_ERR_NULL; tables and fp32 images 4-byte
 * aligned (NSFF_ERR_ALIGN).  Table entries are clamped into the source image on the device. */
typedef struct NsffFrameResizeArgs {
    int32_t n_frames, filter, channels, pad_;
    int32_t src_h, src_w, dst_h, dst_w;
    int32_t ksize_x, ksize_y;
    float   ratio[2];           /* LINEAR_CV only                                           */
    const void* src;  void* dst;
    const int32_t* x_start;  const int32_t* x_count;  const void* x_weights;     /* (dst_w), (dst_w), (dst_w, ksize_x) */
    const int32_t* y_start;  const int32_t* y_count;  const void* y_weights;     /* (dst_h), (dst_h), (dst_h, ksize_y) */
} NsffFrameResizeArgs;
int nsff_frame_resize(const NsffFrameResizeArgs* args, void* stream);

/* ---- a6: eval-only frustum visibility (reference rendering.py:190-200 with datasets/ray_utils.py:127-151,154-181) ---- */
typedef struct NsffFrustumArgs {
    const float*   w2c;         /* device (n_cams * n_frames, 12): row-major first three rows of inverse([c2w; 0 0 0 1]),
                                   camera i of frame f at row i * n_frames + f (dataset.poses order, rendering.py:199)  */
    const int64_t* ts;          /* device: the frame is ts[0] (read on the device: no host synchronisation); a frame outside
                                   [0, n_frames) is treated as seen by no camera (count 0), never read out of bounds      */
    float   K4[4];              /* fx, fy, cx, cy of dataset.Ks[0]                                                     */
    int32_t n_cams, n_frames, H, W;
} NsffFrustumArgs;

/* ---- a7/a8: sigma->alpha compositing and every per-ray / per-sample output ---- */
typedef struct NsffCompositeArgs {
    int64_t n_rays;
    int32_t n_samples;          /* S of this pass                                   */
    int32_t has_transient;      /* output_transient                                 */
    int32_t has_rgb;            /* 0 for the sigma-only coarse test-time pass       */
    int32_t flow_mode;          /* 0 none, 1 per-ray/per-sample flow outputs, 2 + warped renders */
    int32_t want_disocc;        /* 'disocc' in output_transient_flow (flow_mode 2)   */
    float   noise_std;
    float   z_far;              /* 0.95                                             */
    const float* raw;           /* (N*S,16) field records at xyz                    */
    const float* raw_fw;        /* (N*S,16) records at xyz+flow_fw, t+1 (flow_mode 2)*/
    const float* raw_bw;        /* (N*S,16) records at xyz+flow_bw, t-1             */
    const float* zs;            /* (N,S)                                            */
    const float* xyz;           /* (N,S,3)                                          */
    const float* xyz_fw;        /* (N,S,3) (flow_mode 2)                            */
    const float* xyz_bw;
    const float* noise_static;  /* (N,S) standard normal draws or NULL (=> 0)       */
    const float* noise_transient;
    const float* noise_fw;
    const float* noise_bw;
    const float* visibility;    /* (N*S) or NULL; ==0 => raw transient sigma := -10 (rendering.py:200) */
    /* per-sample outputs (NULL = not wanted) */
    float* static_rgbs;  float* transient_rgbs;        /* (N,S,3) */
    float* flows_fw;     float* flows_bw;              /* (N,S,3) zeroed beyond z_far */
    float* static_sigmas; float* transient_sigmas;     /* (N,S) softplus'd */
    float* static_alphas; float* transient_alphas;     /* (N,S) */
    float* static_weights; float* transient_weights; float* weights;   /* (N,S) */
    float* xyzs_fw_bw;   float* xyzs_bw_fw;            /* (N,S,3) */
    float* disoccs_fw;   float* disoccs_bw;            /* (N,S) */
    /* per-ray outputs */
    float* depth;  float* rgb;  float* transient_alpha;  float* transient_rgb;
    float* static_only_rgb;  float* static_only_depth;
    float* xyz_exp;  float* flow_fw_exp;  float* flow_bw_exp;  float* xyz_fw_exp;  float* xyz_bw_exp;
    float* rgb_fw;   float* rgb_bw;
    float* disocc_fw;  float* disocc_bw;
    NsffFrustumArgs vis;        /* a6 evaluated INSIDE this kernel: vis.w2c != NULL => the raw transient sigma of every sample
                                   no training camera of frame ts[0] sees becomes -10 (`visibility` above is the same mask
                                   handed in as an array) */
} NsffCompositeArgs;

int nsff_composite(const NsffCompositeArgs* args, void* stream);

/* The a6 mask as a stage of its own (tests, callers that want the mask): vis_count[p] = number of the frame's training
 * cameras whose image contains NDC point xyz[p] (float, like the reference's `visibilities`). */
int nsff_frustum_visibility(const NsffFrustumArgs* vis, const float* xyz, int64_t n_points, float* vis_count,
                            void* stream);

/* ---- N2: time interpolation of two test-time renders (reference models/rendering.py:365-460 with
 * models/softsplat.py:6-44,303-326 'average' splatting).  The S sample planes of a frame are splatted by ONE
 * launch (the reference: 2*S cupy launches with host round trips) into a per-pixel, per-plane accumulator
 *     accum[(pixel*S + s)*8 + c],  c = r*1, g*1, b*1, a*1 (bilinear-weighted sums), 4 = sum of weights, 5..7 unused
 * with hardware fp32 atomic adds; nsff_mpi_composite normalises (zeros -> 1) and composites front to back. ---- */
typedef struct NsffSplatArgs {
    int32_t H, W, n_planes;     /* n_planes = S = samples per ray (xyzs_fine.shape[1])                      */
    float   K4[4];              /* fx, fy, cx, cy (ndc2world, datasets/ray_utils.py:127-151)                 */
    float   P[12];              /* row-major (3,4) K @ w2c with rows 1,2 of w2c negated (rendering.py:390-394) */
    float   scale;              /* dt for the forward splat of frame t, 1-dt for the backward splat of t+1  */
    const float* xyz;           /* (H*W, S, 3) NDC sample points (xyzs_fine)                                 */
    const float* flow;          /* (H*W, S, 3) transient_flows_fw of t  /  transient_flows_bw of t+1         */
    const float* rgb;           /* (H*W, S, 3) transient_rgbs_fine                                           */
    const float* alpha;         /* (H*W, S)    transient_alphas_fine                                         */
    float*       accum;         /* (H*W, S, 8) OUT; cleared by this call                                     */
    void*        work;          /* device workspace of the binned far path (32-byte aligned) or NULL: samples that land
                                   farther than 4 pixels from their own pixel are then added with device-scope atomics */
    int64_t      work_bytes;    /* nsff_splat_work_bytes(H, W, S) holds every far sample twice (a sample makes one record
                                   per 32 x 8 output block it touches, 1.16 on average); what does not fit takes the
                                   atomic route                                                                       */
} NsffSplatArgs;
int64_t nsff_splat_work_bytes(int32_t H, int32_t W, int32_t n_planes);
int nsff_splat_planes(const NsffSplatArgs* args, void* stream);

typedef struct NsffMpiArgs {
    int32_t H, W, n_planes;
    float   dt;
    const float* accum_fw;      /* nsff_splat_planes of (t, flows_fw, dt)                                    */
    const float* accum_bw;      /* nsff_splat_planes of (t+1, flows_bw, 1-dt)                                */
    const float* static_rgb;    /* (H*W, S, 3) static_rgbs_fine of t                                         */
    const float* static_alpha;  /* (H*W, S)    static_alphas_fine of t                                       */
    const float* zs;            /* (H*W, S)    zs_fine of t                                                  */
    float* rgb;                 /* (H*W, 3) OUT                                                              */
    float* depth;               /* (H*W)    OUT (NDC)                                                        */
} NsffMpiArgs;
int nsff_mpi_composite(const NsffMpiArgs* args, void* stream);

/* ---- N1: backward of nsff_composite for the training configurations (has_rgb = 1, flow_mode 0, 1 or 2): gradients
 * w.r.t. the raw records of the main pass and of the two warped re-queries, and w.r.t. the (far-masked) per-sample
 * flows that enter the per-ray flow expectations.  flow_mode (has_transient only, else NSFF_ERR_INVALID): 0 no flow
 * outputs; 1 the per-ray expectations xyz_exp / flow_fw_exp / flow_bw_exp without the warped renders -- xyz, f_fw, f_bw
 * are required, d_f_fw / d_f_bw are written where given, raw_fw / raw_bw / noise_fw / noise_bw / g_rgb_fw / g_rgb_bw /
 * d_raw_fw / d_raw_bw are neither read nor written; 2 also rgb_fw / rgb_bw (raw_fw, raw_bw, d_raw_fw, d_raw_bw required).
 * tests/test_composite_kernels.py holds all three to float64.  g_* = gradient of the output of that name (NULL = zero):
 * per sample (n_rays, S): static_sigmas, transient_sigmas, static_weights, transient_weights, weights;
 * per ray: depth (n), rgb (n,3), transient_alpha (n), transient_rgb (n,3), so_rgb = _static_rgb (n,3), so_depth =
 * _static_depth (n), xyz_exp = xyz_fine (n,3), flow_fw_exp / flow_bw_exp = transient_flow_fw / _bw (n,3), rgb_fw, rgb_bw.
 * The per-sample passthrough outputs (rgbs, flows, warped points) are plain views of the inputs and stay with the
 * caller.  scratch: (n_rays, S, 4) floats.  d_raw* : (P, NSFF_RAW_STRIDE), slots 0-7 written, the rest zeroed. ---- */
typedef struct NsffCompositeBwdArgs {
    int64_t n_rays;
    int32_t n_samples, has_transient, flow_mode;
    float   noise_std;
    const float* raw;  const float* raw_fw;  const float* raw_bw;
    const float* zs;   const float* xyz;     const float* f_fw;  const float* f_bw;
    const float* noise_static;  const float* noise_transient;  const float* noise_fw;  const float* noise_bw;
    const float* g_static_sigmas;  const float* g_transient_sigmas;
    const float* g_static_weights; const float* g_transient_weights;  const float* g_weights;
    const float* g_depth;  const float* g_rgb;  const float* g_transient_alpha;  const float* g_transient_rgb;
    const float* g_so_rgb; const float* g_so_depth;
    const float* g_xyz_exp;  const float* g_flow_fw_exp;  const float* g_flow_bw_exp;
    const float* g_rgb_fw;   const float* g_rgb_bw;
    float* scratch;
    float* d_raw;  float* d_raw_fw;  float* d_raw_bw;  float* d_f_fw;  float* d_f_bw;
} NsffCompositeBwdArgs;
int nsff_composite_backward(const NsffCompositeBwdArgs* args, void* stream);

/* ---- N1: gradient of the scene-flow glue of `inference` (reference models/rendering.py:187-188 flows zeroed beyond
 * z = 0.95, :218/:224 warped points xyz + flow, :226-232 cycle points xyz_fw + flow_bw(xyz_fw)) w.r.t. the field record it
 * reads.  For every point p (depth zs[p]):
 *     out[p][col_a .. col_a+2] (+)= m * sum_k g_a[k][p][0..2],   out[p][col_b .. col_b+2] (+)= m * sum_k g_b[k][p][0..2],
 * m = zs[p] > z_far ? 0 : 1; accumulate = 0 also writes zeros to the other 10 columns of the (P,16) record (a whole-record
 * store), accumulate = 1 adds into the named columns only.  g_a / g_b: up to four (P,3) cotangents each (NULL = absent) -- the
 * consumers of one flow: the compositing node, the warped query, the loss.  col_a / col_b < 0 disables a group.  One launch
 * replaces autograd's where / slice / zeros / add chain (~12 small kernels per flow direction). */
typedef struct {
    int64_t n_points;
    const float* zs;            /* (P) sample depths                                          */
    float z_far;                /* 0.95 (rendering.py:187)                                    */
    int32_t accumulate;
    int32_t col_a, col_b;       /* first column of each 3-wide group in the 16-float record   */
    int32_t pad_;
    const float* g_a[4];
    const float* g_b[4];
    float* out;                 /* (P,16), 16-byte aligned                                    */
} NsffFlowGradArgs;
int nsff_flow_grad(const NsffFlowGradArgs* args, void* stream);

/* ---- SSIM metric and SSIM-driven ray sampling (reference metrics.py:19-33 over kornia 0.5.4's ssim_loss; train.py:140-143,
 * 184-185, 246-253 and datasets/monocular.py:184-187, 222-250 for --hard_sampling).  DESIGN.md section 11. ---- */
#define NSFF_RAY_RECORD      16   /* floats per training-ray record (monocular.py:180-183): rays_o 0-2, rays_d 3-5, rgb 6-8,
                                     t 9, disp 10, mask 11, uv_fw 12-13, uv_bw 14-15                                   */

/* The per-pixel, per-channel SSIM LOSS  clamp((1 - ssim) / 2, 0, 1)  of kornia 0.5.4 (11x11 Gaussian window, sigma 1.5,
 * reflect padding, C1 = 0.01^2, C2 = 0.03^2) of n_frames image pairs; the reference's metric is 1 - loss.  gt / pred: (F, H, W, 3)
 * fp32, HWC, contiguous.  Outputs (any subset, at least one):
 *   map       (F, H, W, 3) the loss;
 *   mean_map  (F, H*W)     its channel mean = the hard-sampling weight 1 - ssim_map.mean(-1) of train.py:253;
 *   sums      (F, 3) fp64  per frame: sum of the loss over pixels and channels, the same over the pixels with mask != 0,
 *                          and the number of those pixels (mask (F, H*W) uint8 or NULL = none selected).
 * sums are combined from per-tile partials in a fixed order (bit-reproducible) in `scratch`: nsff_ssim_scratch_bytes() bytes,
 * 16-byte aligned, ZERO before its first use (every call leaves it so; one call at a time per scratch buffer).
 * window must be 11; H, W >= 6 (the reflect padding's minimum) else NSFF_ERR_INVALID. */
typedef struct NsffSsimArgs {
    int32_t n_frames, H, W, window;
    const float* gt;  const float* pred;  const uint8_t* mask;
    float* map;  float* mean_map;  double* sums;
    void* scratch;  int64_t scratch_bytes;
} NsffSsimArgs;
int64_t nsff_ssim_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int nsff_ssim(const NsffSsimArgs* args, void* stream);

/* The per-frame finishing work of eval.py on n_frames rendered frames of H x W pixels (eval.py:113-118, 183-184, 213-214,
 * 222-223, 230-240; utils/visualization.py:10-15; metrics.py:6-16).  Only rgb is required; every other pointer may be NULL and
 * every output is written only when given.  Inputs: rgb (F, H*W, 3) fp32, the raw rgb_fine; gt (F, H*W, 3) fp32; valid (F, H*W)
 * uint8, non-zero = the pixel counts (the caller passes mask == 0); depth (F, H*W) fp32; lut (256, 3) uint8.  Outputs:
 *   rgb_clipped  (F, H*W, 3) fp32   clip(rgb, 0, 1) (a NaN stays a NaN);
 *   rgb_u8       (F, H*W, 3) uint8  255 * clip(rgb, 0, 1) rounded to fp32, then truncated (astype(np.uint8)); NaN gives 0;
 *   sums         (F, 3) fp64        sum of (gt - clip(rgb))^2 over all 3 H W values, the same over the valid pixels, and the
 *                                   number of valid pixels (needs gt): squares in fp32, added in fp64 in an order that depends
 *                                   on H * W only -- bit-reproducible, and the same for a frame alone or inside a batch;
 *   depth_range  (F, 2) fp32        min and max of nan_to_num(depth): NaN counts as 0, +-inf as +-FLT_MAX (needs depth);
 *   depth_u8     (F, H*W) uint8     255 * ((x - min) / (max - min + 1e-8f)) truncated, x = nan_to_num(depth), each step one
 *                                   fp32 operation, with the frame's own range (needs depth_range as well);
 *   depth_rgb_u8 (F, H*W, 3) uint8  lut[depth_u8] (needs lut and depth_range).
 * Two launches on `stream` (the second only for the 8-bit depth), no synchronisation, no allocation: capturable.  sums and
 * depth_range are combined from per-workgroup partials in `scratch`: nsff_frame_finish_scratch_bytes() bytes, 16-byte aligned,
 * ZERO before its first use (every call returns its counter words to zero and rewrites the partials before it reads them, so the
 * buffer serves call after call; one call at a time per scratch buffer).  n_frames <= 65535 and
 * 1 <= H * W < 2^31; a missing image, an output without its input or nothing to compute is NSFF_ERR_INVALID, before any launch.
 * fp32 arrays 16-byte and uint8 arrays 4-byte aligned take the wide path; less aligned ones are read element by element. */
typedef struct NsffFrameFinishArgs {
    int32_t n_frames, H, W, pad_;
    const float* rgb;  const float* gt;  const uint8_t* valid;  const float* depth;  const uint8_t* lut;
    float* rgb_clipped;  uint8_t* rgb_u8;  double* sums;  float* depth_range;  uint8_t* depth_u8;  uint8_t* depth_rgb_u8;
    void* scratch;  int64_t scratch_bytes;
} NsffFrameFinishArgs;
int64_t nsff_frame_finish_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int nsff_frame_finish(const NsffFrameFinishArgs* args, void* stream);

/* The image panels of the trainer's validation step (train.py:209-235, 254-257 over utils/visualization.py:6-44 and
 * torchvision's make_grid) for n_frames frames of H x W pixels, as 8-bit images.  Only pred is required; every other pointer may be
 * NULL and every output is written only when given.  Inputs, fp32, (F, H*W[, 3]) contiguous, channels last: gt; pred, the raw
 * rgb_fine; depth; transient_alpha, static_rgb (the raw _static_rgb_fine) and static_depth -- all three or none; mask (0 = static,
 * 1 = dynamic, as the validation batch carries it); disp; ssim_loss (F, H*W, 3), the `map` of nsff_ssim for (gt, clip(pred)).
 * lut_depth / lut_mask (256, 3) uint8 stand for cv2.applyColorMap(., COLORMAP_JET) / (., COLORMAP_BONE) and are used as they are
 * (the reference hands cv2's BGR bytes to PIL unchanged); a NULL table writes the index into all three channels.
 * Two error maps are formed per pixel, every step one fp32 operation (divide and square root correctly rounded):
 *   rmse = sqrt(((d0^2 + d1^2) + d2^2) / 3), d = gt - clip(pred, 0, 1)          (train.py:215)
 *   ssim = (((1 - l0) + (1 - l1)) + (1 - l2)) / 3, l = ssim_loss                (train.py:218)
 * Launch 1 writes
 *   ranges  (F, 5, 2) fp32   min and max of nan_to_num of [depth, static_depth, -disp, -rmse (needs gt), -ssim (needs ssim_loss)];
 *                            the rows of missing fields are left untouched.  Combined from per-workgroup partials in an order
 *                            that depends on H * W only: the same bits for a frame alone or in a batch.
 * Launch 2 (only with one of the outputs below) recomputes the maps and writes, with index(x) = the 8-bit index of
 * visualize_depth, 255 * ((x - min) / (max - min + 1e-8f)) truncated, on the frame's own range of that field:
 *   rmse_u8, ssim_u8  (F, H*W) uint8            index(-rmse), index(-ssim);
 *   rmse_blend_u8, ssim_blend_u8  (F, H*W, 3)   blend_images(clip(pred), visualize_depth(-map), 0.5): with a = the 8-bit clipped
 *                            prediction and b = lut_depth[index] per channel, min(255, ((a + b) >> 1) + 2 + ((a + b) & 1)), which
 *                            is cv2.addWeighted(a, .5, b, .5, 2.2) = saturate(round(a / 2 + b / 2 + 2.2)) for every byte pair;
 *   grid_u8  (F, GH, GW, 3) uint8               make_grid(tiles, nrow=3) with padding 2 and pad value 0: tile k at row
 *                            (k / 3)(H + 2) + 2, column (k % 3)(W + 2) + 2; GW = 3 (W + 2) + 2, GH = ymaps (H + 2) + 2, ymaps =
 *                            ceil(tiles / 3).  Tiles in order (train.py:225-231): gt, clip(pred), depth colour [, transient_alpha
 *                            through visualize_mask, clip(static_rgb), static-depth colour] [, 1 - mask through visualize_mask]
 *                            [, -disp colour]: 3 to 8 of them (needs gt and depth).  Padding and unfilled cells are written as 0.
 *                            Float tiles are 255 * x truncated, colour tiles lut_depth[index(x)], mask tiles lut_mask[255 * x
 *                            truncated].  Every truncation CLAMPS to 0..255 first (a NaN gives 0) -- numpy's astype(uint8) of a
 *                            value outside that range (a ground truth above 1, an alpha below 0) is platform-defined.
 * No synchronisation, no allocation: capturable.  `scratch`: nsff_val_panels_scratch_bytes() bytes, 16-byte aligned, ZERO before
 * its first use (every call returns its counter words to zero; one call at a time per scratch buffer).  n_frames <= 65535 and
 * 1 <= H * W < 2^31; a missing pred or ranges, an output without its input, a transient set given in part or no field at all is
 * NSFF_ERR_INVALID, before any launch.  fp32 arrays 16-byte and the (F, H*W[, 3]) uint8 outputs 4-byte aligned take the wide
 * path, less aligned ones go element by element; the grid's 3-byte pixels are packed into dword stores by address. */
typedef struct NsffValPanelsArgs {
    int32_t n_frames, H, W, pad_;
    const float* gt;  const float* pred;  const float* depth;  const float* transient_alpha;  const float* static_rgb;
    const float* static_depth;  const float* mask;  const float* disp;  const float* ssim_loss;
    const uint8_t* lut_depth;  const uint8_t* lut_mask;
    float* ranges;  uint8_t* grid_u8;  uint8_t* rmse_u8;  uint8_t* ssim_u8;  uint8_t* rmse_blend_u8;  uint8_t* ssim_blend_u8;
    void* scratch;  int64_t scratch_bytes;
} NsffValPanelsArgs;
int64_t nsff_val_panels_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int nsff_val_panels(const NsffValPanelsArgs* args, void* stream);

/* ---- induced optical flow of rendered frames: maps, end-point error, colour images (csrc/flow.hip).
 * What the reference's test.ipynb does on the host with the test-time outputs xyz_fw / xyz_bw (rendering.py:280-287), for
 * n_frames frames of H x W pixels and both directions (index 0 forward, 1 backward) in one call.  Three stages, selected by the
 * pointers given, each callable alone:
 *   projection   xyz[d] (F, H*W, 3) fp32 NDC points -> flow[d] (F, H*W, 2) fp32, pixels: the reference's ndc2world
 *                (ray_utils.py:142-145, eps = 1e-6f), Ps[clamp(t + 1, max = max_t)] (fw) / Ps[clamp(t - 1, min = 0)] (bw) applied as
 *                ((p0 X + p1 Y) + p2 Z) + p3 per row, uv = uvd.xy / (|uvd.z| + 1e-8f) (losses.py:99-111), minus the integer pixel
 *                coordinates; every step one fp32 operation.  t = ts[frame] (int32, (F)); Ps (n_poses, 3, 4) fp32; fx, fy, cx, cy
 *                the intrinsics.  A pixel is valid when uvd.z > 0 and t < max_t (fw) / t > 0 (bw) (losses.py:115-116; a NaN point
 *                is not); an invalid pixel gets both components NSFF_FLOW_UNKNOWN (the Middlebury convention: |.| > 1e7 is unknown).
 *                A row index outside 0 .. n_poses - 1 (a time outside the sequence) is clamped into it.
 *   EPE          flow[d] (written by the projection, or the caller's own map where xyz[d] is NULL) against gt[d] (F, H*W, 2):
 *                sqrtf(du^2 + dv^2) in fp32 over the pixels where both flows are known (|.| <= 1e7, not NaN) and the ground truth
 *                is non-zero in a component (flowlib.flow_error's smallflow = 0 rule), added in fp64:
 *                epe_sums (F, 2, 3) fp64 and epe_counts (F, 2, 3) int64 per frame and direction for [all, mask != 0, mask == 0]
 *                (mask (F, H*W) uint8 or NULL: the last two stay 0).  A direction without a pair has zero sums and counts.
 *                Fixed summation order that depends on H * W only: the same bits for a frame alone or in a batch.
 *   colour       flowlib.flow_to_image / compute_color in fp32: image[d] (F, H*W, 3) uint8 of flow[d], gt_image[d] of gt[d].
 *                Unknown and NaN pixels are zeroed before the radius and painted black.  The scale of frame f, direction d is
 *                float(double(r) + 2^-52) with r = scale[f][d][c] where `scale` (F, 2, 2) fp32 is given, else maxrad[f][d][c];
 *                c = 1 for a ground-truth image -- and for the map's image too when share_gt_scale != 0 -- else 0.
 *   maxrad       (F, 2, 2) fp32 out: per frame and direction the maximum of sqrtf(u^2 + v^2) over the known pixels of [flow[d],
 *                gt[d]] (0 where there is none); needed for colouring without `scale`.
 * At most two launches on `stream`, no synchronisation, no allocation: capturable.  epe_* and maxrad are combined from
 * per-workgroup partials in `scratch`: nsff_flow_maps_scratch_bytes() bytes, 16-byte aligned, ZERO before its first use (every
 * call leaves its counter words zero; one call at a time per scratch buffer).  n_frames <= 65535, 1 <= H * W < 2^31,
 * 0 <= max_t < n_poses; an output without its input, a ground truth without a map of its direction or nothing to compute is
 * NSFF_ERR_INVALID, a missing Ps / ts / flow[d] beside points or a missing scratch NSFF_ERR_NULL -- all before any launch.
 * flow / gt need 8-byte, every other fp32 / int32 array 4-byte alignment (NSFF_ERR_ALIGN). */
#define NSFF_FLOW_UNKNOWN    1e10f
typedef struct NsffFlowMapsArgs {
    int32_t n_frames, H, W, n_poses, max_t, share_gt_scale;
    float   fx, fy, cx, cy;
    const float* xyz[2];  const float* Ps;  const int32_t* ts;
    float* flow[2];  const float* gt[2];  const uint8_t* mask;
    double* epe_sums;  int64_t* epe_counts;  float* maxrad;  const float* scale;
    uint8_t* image[2];  uint8_t* gt_image[2];
    void* scratch;  int64_t scratch_bytes;
} NsffFlowMapsArgs;
int64_t nsff_flow_maps_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int nsff_flow_maps(const NsffFlowMapsArgs* args, void* stream);

/* ---- chained scene-flow tracks (csrc/tracks.hip; nsff_pl_amd/tracks.py).  Entry points added without a
 * change of NSFF_ABI_VERSION: nothing that existed changes.
 * nsff_track_step: one step of n_rows rows of pts_per_row points each, one launch.  For point p of row r, x = xyz_in[p] (fp32 NDC),
 * t = t_in[r] (int32), with the records `raw` (n_rows * pts_per_row, NSFF_RAW_STRIDE) of a field query at (x, E_t[t]):
 *   can = alive_in[r] && (direction > 0 ? t < max_t : t > 0);  f = raw columns 8..10 (direction +1) or 11..13 (-1), set to 0 where
 *   (x.z + 1f) * 0.5f > 0.95f (the reference's flows[zs > z_far] = 0 on NDC rays);  xyz_out[p] = can ? x + f : x;
 *   t_out[r] = can ? t + direction : t;  alive_out[r] = can  (uint8 0 / 1; t_out / alive_out must not be t_in / alive_in).
 * With cameras (Ps, uv and depth given together) the NEW position is projected by Ps[t_out[r]] -- Ps (n_poses, 3, 4), max_t <
 * n_poses -- or, with fixed_view != 0, by Ps[0]: the chain of nsff_flow_maps' projection (every step one fp32 operation), uv (.., 2)
 * = (NSFF_FLOW_UNKNOWN, NSFF_FLOW_UNKNOWN) where uvd.z > 0 fails, depth = uvd.z.
 * raw == NULL (then xyz_out, t_out, alive_out must be NULL and cameras given): nothing moves, xyz_in is projected at t_in -- the
 * projection of a path's first slab.  raw needs 16-byte, every other array 4-byte alignment (NSFF_ERR_ALIGN); 16-byte accesses are
 * used where a lane's four points start 16-byte aligned, dwords otherwise.  n_rows * pts_per_row <= NSFF_TRACK_MAX_POINTS. */
#define NSFF_TRACK_MAX_POINTS 0x7fffffffLL
typedef struct NsffTrackStepArgs {
    int64_t n_rows;
    int32_t pts_per_row, direction, max_t, n_poses, fixed_view, pad_;
    float   fx, fy, cx, cy;
    const float* raw;  const float* xyz_in;  const int32_t* t_in;  const uint8_t* alive_in;
    float* xyz_out;  int32_t* t_out;  uint8_t* alive_out;
    const float* Ps;  float* uv;  float* depth;
} NsffTrackStepArgs;
int nsff_track_step(const NsffTrackStepArgs* args, void* stream);

/* nsff_track_draw: motion trails of n_tracks tracks of n_steps segments on a copy of an (H, W, 3) uint8 image, deterministic.
 * uv (n_steps + 1, n_tracks, 2) fp32 pixels, ok (n_steps + 1, n_tracks) uint8.  Segment j of track q, uv[j][q] -> uv[j + 1][q], is
 * drawn when both ends are ok and have |u|, |v| < 32768 (NaN, infinities and NSFF_FLOW_UNKNOWN fail) and, with the ends rounded by
 * floor(u + 0.5f) to (x0, y0), (x0 + dx, y0 + dy), N = max(|dx|, |dy|) <= H + W.  Its pixels, in integers, i = 0 .. N:
 *   (x0 + floor((2 i dx + N) / (2 N)), y0 + floor((2 i dy + N) / (2 N)))       (N = 0: the one pixel (x0, y0))
 * -- N + 1 pixels, both ends included, 8-connected; pixels outside the image are skipped one by one.  A pixel takes the segment with
 * the largest key ((j + 1) << 20) | q (atomicMax on the uint32 canvas in `scratch`), and out = lut[(255 * (j + 1)) / n_steps]
 * (lut (256, 3) uint8) there, the image's pixel elsewhere.  n_tracks < NSFF_TRACK_MAX_TRACKS, 1 <= n_steps < NSFF_TRACK_MAX_STEPS
 * (NSFF_ERR_INVALID).  scratch: nsff_track_draw_scratch_bytes(H, W) bytes, 4-byte aligned, any content; uv 8-byte aligned.
 * Three launches on `stream`, no synchronisation. */
#define NSFF_TRACK_MAX_TRACKS (1 << 20)
#define NSFF_TRACK_MAX_STEPS  (1 << 11)
typedef struct NsffTrackDrawArgs {
    int32_t H, W, n_steps, n_tracks;
    const float* uv;  const uint8_t* ok;  const uint8_t* image;  const uint8_t* lut;  uint8_t* out;
    void* scratch;  int64_t scratch_bytes;
} NsffTrackDrawArgs;
int64_t nsff_track_draw_scratch_bytes(int32_t H, int32_t W);
int nsff_track_draw(const NsffTrackDrawArgs* args, void* stream);

/* ---- motion masks from optical flow and camera poses (csrc/motion.hip; nsff_pl_amd/motion.py).  Entry
 * points added without a change of NSFF_ABI_VERSION: nothing that existed changes.
 * nsff_motion_maps: one launch for n_frames frames of H x W pixels and both directions (index 0 forward, 1 backward).  Frame f,
 * direction d uses the neighbour n = f + 1 (fw) / f - 1 (bw), A = flow_fw[f], B = flow_bw[n] (fw) / A = flow_bw[f], B = flow_fw[n]
 * (bw) -- flow_fw / flow_bw (F, H*W, 2) fp32 pixels -- and M = Fm[f][d], Fm (F, 2, 3, 3) fp32, which maps a pixel of f to its
 * epipolar line in n.  A frame has no neighbour outside 0 .. F-1.  At the pixel (x, y), integers as floats, every step one fp32
 * operation in the order written (IEEE division and square root):
 *   a = A[y][x];  known(a): both components |.| <= 1e7 and not NaN (the Middlebury convention of nsff_flow_maps)
 *   qx = x + a.u, qy = y + a.v;  inside = 0 <= qx <= W-1 && 0 <= qy <= H-1
 *   b = B sampled bilinearly at q:  x0 = floorf(qx), ax = qx - x0, x1 = min(x0 + 1, W-1), y likewise, per component
 *       b = ((B00 * (1 - ax) + B01 * ax) * (1 - ay)) + ((B10 * (1 - ax) + B11 * ax) * ay),  Bij = B[yi][xj];  all four taps known
 *   s = a + b;  lhs = s.u * s.u + s.v * s.v;  rhs = alpha * ((a.u * a.u + a.v * a.v) + (b.u * b.u + b.v * b.v)) + beta
 *   consistent = lhs <= rhs                                               (the forward-backward check)
 *   l_i = (M[i][0] * x + M[i][1] * y) + M[i][2];  r = (l0 * qx + l1 * qy) + l2;  n = l0 * l0 + l1 * l1
 *   e = fabsf(r) / sqrtf(n);  line_ok = n is finite and > 0               (the distance of q from the epipolar line of (x, y))
 * Outputs, each optional (at least one):
 *   err   (F, 2, H*W) fp32   e where there is a neighbour, known(a) and line_ok, else NSFF_FLOW_UNKNOWN
 *   valid (F, 2, H*W) uint8  1 where neighbour && known(a) && inside && taps known && consistent && line_ok, else 0
 *   raw   (F, H*W) uint8     0 (dynamic) where valid && e > threshold in either direction, else 255 (static): the polarity of the
 *                            reference's masks/ *.png
 *   counts (F, 5) int64 [valid fw, valid bw, over fw, over bw, dynamic pixels of raw] and err_sums (F, 2) fp64, the sum of e over
 *   the valid pixels of each direction (fp32 terms added in fp64) -- given together; fixed summation order that depends on H * W
 *   only: the same bits for a frame alone or in a batch.
 * epipolar == 0 is the consistency check alone: Fm is not read, line_ok counts as true in `valid`, err is NSFF_FLOW_UNKNOWN
 * everywhere, nothing is over and raw is 255.
 * No synchronisation, no allocation: capturable.  counts / err_sums are combined from per-workgroup partials in `scratch`:
 * nsff_motion_maps_scratch_bytes() bytes, 16-byte aligned, ZERO before its first use (every call leaves it as it needs it: the
 * counter words zero; one call at a time per scratch buffer).  The same size serves nsff_mask_erode.
 * n_frames <= 65535, 1 <= H * W < 2^31; epipolar not 0 / 1, alpha, beta or threshold negative or NaN, no output, counts without
 * err_sums or a scratch that is too small: NSFF_ERR_INVALID; a missing flow, Fm (epipolar) or scratch (counts): NSFF_ERR_NULL; flows,
 * counts and err_sums 8-byte, scratch 16-byte, Fm and err 4-byte aligned (NSFF_ERR_ALIGN) -- all before the launch.  16-byte
 * accesses are used where every fp32 array is 16-byte and every uint8 array 4-byte aligned and a lane's four pixels start
 * there, single elements otherwise. */
typedef struct NsffMotionMapsArgs {
    int32_t n_frames, H, W, epipolar;
    float   alpha, beta, threshold, pad_;
    const float* flow_fw;  const float* flow_bw;  const float* Fm;
    float* err;  uint8_t* valid;  uint8_t* raw;
    int64_t* counts;  double* err_sums;
    void* scratch;  int64_t scratch_bytes;
} NsffMotionMapsArgs;
int64_t nsff_motion_maps_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int nsff_motion_maps(const NsffMotionMapsArgs* args, void* stream);

/* nsff_mask_erode: cv2.erode(src, ones((k, k))) of n_frames uint8 images of H x W pixels (any values), one launch:
 * dst[y][x] = the minimum of src over the k x k window centred on (x, y); pixels outside the image do not contribute (OpenCV's
 * default border for morphology), so an image smaller than the window is legal.  k odd, 1 .. NSFF_ERODE_MAX_K; k = 1 copies.
 * zero_counts (F) int64, optional: the number of zero pixels of each frame of dst; it needs `scratch`
 * (nsff_motion_maps_scratch_bytes() bytes, 16-byte aligned, zero before its first use, left so).  dst must not overlap src.
 * An even or out-of-range k, dst == src or a scratch that is too small: NSFF_ERR_INVALID; a missing src / dst or scratch
 * (zero_counts): NSFF_ERR_NULL; zero_counts 8-byte, scratch 16-byte aligned (NSFF_ERR_ALIGN) -- all before the launch.  No
 * synchronisation, no allocation. */
#define NSFF_ERODE_MAX_K 31
typedef struct NsffMaskErodeArgs {
    int32_t n_frames, H, W, k;
    const uint8_t* src;  uint8_t* dst;  int64_t* zero_counts;
    void* scratch;  int64_t scratch_bytes;
} NsffMaskErodeArgs;
int nsff_mask_erode(const NsffMaskErodeArgs* args, void* stream);

/* ---- TV-L1 optical flow (csrc/optflow.hip; nsff_pl_amd/optflow.py): dense flow between P image pairs, the
 * classical stand-in for the reference's RAFT step (preprocess.py:106-120).  Zach, Pock and Bischof 2007 in the fixed-iteration
 * form of Sanchez, Meinhardt-Llopis and Facciolo (IPOL 2013).  Entry points added without a change of NSFF_ABI_VERSION: nothing that
 * existed changes.  Every array is fp32 unless said otherwise, every image plane (n, H, W) contiguous, and every step below ONE
 * fp32 operation in the order written (the file is built -ffp-contract=off; IEEE division and square root), which the tests
 * compare bit for bit with numpy.  No atomics, no reductions, no synchronisation, no allocation: every call is capturable.
 * Common refusals, all before a launch: a size outside the stated range, a bad flag or a scratch that is too small NSFF_ERR_INVALID;
 * a missing pointer NSFF_ERR_NULL; an array off its element's alignment NSFF_ERR_ALIGN.
 *
 * grey     channels == 3: src (n, H*W, 3) uint8 -> dst = (0.299f * R + 0.587f * G) + 0.114f * B on the 0..255 scale;
 *          channels == 1: src fp32, copied.
 * down     one pyramid step, (n, H, W) -> (n, (H+1)/2, (W+1)/2): the separable binomial [1, 4, 6, 4, 1] / 16 with a replicated
 *          border, horizontal pass first, each pass  (((a[-2] + a[+2]) + (a[-1] + a[+1]) * 4f) + a[0] * 6f) * 0.0625f,  then every
 *          second pixel from (0, 0).  H, W >= 2.
 * up       a coarse plane (n, h, w) to the next finer level (n, H, W), (H+1)/2 == h and (W+1)/2 == w: bilinear at
 *          cx = min(x * 0.5f, w-1), cy likewise -- x0 = floorf(cx), ax = cx - x0, x1 = min(x0 + 1, w-1),
 *          ((c00 * (1 - ax) + c01 * ax) * (1 - ay)) + ((c10 * (1 - ax) + c11 * ax) * ay) -- and the value times 2f.
 * median   the 3 x 3 median of every plane with a replicated border; dst must not be src.
 * warp     per pair and pixel, with (u1, u2) the flow so far: Dx = (I1[y][min(x+1, W-1)] - I1[y][max(x-1, 0)]) * 0.5f, Dy likewise
 *          along y; I1, Dx and Dy sampled bilinearly (the formula of `up`) at cx = min(max(x + u1, 0), W-1), cy likewise ->
 *          I1w, Ix, Iy;  g = Ix * Ix + Iy * Iy;  rho_c = ((I1w - Ix * u1) - Iy * u2) - I0.
 *          consts: five planes of P * H * W values each: Ix | Iy | g | rho_c | I1w.
 * iterate  `iters` iterations on a state of six planes of P * H * W values each, u1 | u2 | p11 | p12 | p21 | p22, with
 *          l_t = lambda * theta and taut = tau / theta (fp32, formed on the host):
 *            rho = (rho_c + Ix * u1) + Iy * u2;  lg = l_t * g
 *            f = rho < -lg ? l_t : rho > lg ? -l_t : g > 1e-10f ? (-rho) / g : 0
 *            v1 = u1 + f * Ix;  v2 = u2 + f * Iy
 *            div1 = dx(p11) + dy(p12),  dx(p)(x) = p(x) in the first column, p(x) - p(x-1) inside, -p(x-1) in the last; dy by rows
 *            u1' = v1 + theta * div1   (u2' from v2, p21, p22)
 *            ux = u1'(x+1) - u1'(x), 0 in the last column; uy by rows, 0 in the last row;  ng = sqrtf(ux * ux + uy * uy)
 *            p11' = (p11 + taut * ux) / (1f + taut * ng);  p12' = (p12 + taut * uy) / (same)   (p21', p22' from u2')
 *          The iterations go back and forth between state[0] (the input) and state[1]; the result is in
 *          state[nsff_optflow_result_slot(iters, fused ? k : 1)].  fused == 0: one launch per iteration, the definition.
 *          fused == 1: k iterations per launch on a tile x tile block of pixels held in LDS with a halo of k pixels, bit-identical
 *          to the plain route for every iters (a last launch runs iters % k); (tile, k) one of the built pairs, (16, 2), (32, 2),
 *          (32, 3), (32, 4), (32, 6), or (0, 0) = NSFF_OPTFLOW_TILE, NSFF_OPTFLOW_K, the measured default.
 *          4 <= H, W; P <= 65535; P * H * W < 2^31; 1 <= iters <= 100000; lambda, theta, tau > 0 and finite.
 * nsff_optflow: the whole estimate for P pairs, images0[p] -> images1[p]: grey, `levels` pyramid levels (clipped so that the
 *          coarsest keeps both sides >= 4), and from the coarsest level down: the flow of the level above through `up` (zero at the
 *          coarsest), the dual variables p zero, then `warps` times { warp; iterate; median when `median` != 0 }.
 *          flow (P, H*W, 2): pixels, x first.  images: channels == 3 uint8 (P, H*W, 3), channels == 1 fp32 (P, H*W).
 *          16 <= H, W (NSFF_OPTFLOW_MIN_SIZE); 1 <= levels <= 16, 1 <= warps <= 1000; scratch: nsff_optflow_scratch_bytes bytes (0 = the
 *          shape is refused), 16-byte aligned, any content. */
#define NSFF_OPTFLOW_MIN_SIZE 16
#define NSFF_OPTFLOW_TILE     32   /* the fused route's default tile side ...                                    */
#define NSFF_OPTFLOW_K        3    /* ... and iterations per launch (DESIGN.md section 11.4 has the measurement) */
#define NSFF_OPTFLOW_FUSED    1    /* the route nsff_pl_amd.optflow takes when not told: 1 fused, 0 plain        */
typedef struct NsffOptflowIterArgs {
    int32_t n_pairs, H, W, iters;
    int32_t fused, tile, k, pad_;
    float   lambda, theta, tau, pad1_;
    const float* consts;  float* state[2];
} NsffOptflowIterArgs;
typedef struct NsffOptflowArgs {
    int32_t n_pairs, H, W, channels;
    int32_t levels, warps, iters, median;
    int32_t fused, tile, k, pad_;
    float   lambda, theta, tau, pad1_;
    const void* images0;  const void* images1;  float* flow;
    void* scratch;  int64_t scratch_bytes;
} NsffOptflowArgs;
int     nsff_optflow_grey(const void* src, float* dst, int32_t n, int32_t H, int32_t W, int32_t channels, void* stream);
int     nsff_optflow_down(const float* src, float* dst, int32_t n, int32_t H, int32_t W, void* stream);
int     nsff_optflow_up(const float* src, float* dst, int32_t n, int32_t H, int32_t W, void* stream);
int     nsff_optflow_median(const float* src, float* dst, int32_t n, int32_t H, int32_t W, void* stream);
int     nsff_optflow_warp(const float* I0, const float* I1, const float* u, float* consts, int32_t n_pairs, int32_t H, int32_t W,
                          void* stream);
int     nsff_optflow_iterate(const NsffOptflowIterArgs* args, void* stream);
/* host only: 0 or 1, the state buffer that holds the result of `iters` iterations run k per launch (k = 1: the plain route);
 * negative for iters < 1 or k < 1 */
int     nsff_optflow_result_slot(int32_t iters, int32_t k);
/* host only: the number of pyramid levels nsff_optflow uses for an H x W image when asked for `levels` (0: a refused shape) */
int     nsff_optflow_levels(int32_t H, int32_t W, int32_t levels);
int64_t nsff_optflow_scratch_bytes(int32_t n_pairs, int32_t H, int32_t W, int32_t levels);
int     nsff_optflow(const NsffOptflowArgs* args, void* stream);

/* ---- the image-guided weighted median of a flow map (csrc/flowmedian.hip; nsff_pl_amd/optflow.py refine_flow; DESIGN.md section
 * 11.4): the non-local term of "Classic+NL" (Sun, Roth and Black 2010) as one filter pass over the flow of P pairs.  TV-L1 rounds a
 * motion edge off; the weighted median ties it to the image edge it belongs to.  Entry point added without a change of
 * NSFF_ABI_VERSION: nothing that existed changes.  The conventions of the section above hold (fp32, one fp32 operation per step in
 * the order written, the file built -ffp-contract=off, IEEE division).
 *
 * flow (P, H*W, 2) fp32; grey (P, H*W) fp32, finite, on the 0..255 scale: the grey stage of the image the flow STARTS from; valid
 * (P, H*W) uint8, optional; out (P, H*W, 2) fp32, which must not overlap flow.  Pixel p, with known(f) = both components |.| <= 1e7
 * (a NaN is not; the rule of nsff_motion_maps):
 *   unknown centre   !known(flow[p]):  out[p] = flow[p], bits unchanged.
 *   candidates       q = p + (dx, dy), |dx|, |dy| <= radius, with q inside the image (there is no replicated border),
 *                    known(flow[q]) and (q == p || valid == NULL || valid[q] != 0).
 *   weight           di = (grey[q] - grey[p]) / sigma_i;  w = 1f / ((1f + di * di) * s[dy][dx]);  wq = (int) rintf(w * 65535f)
 *                    s[dy][dx] = 1 + (dx^2 + dy^2) / sigma_s^2, formed on the host in double from the fp32 sigma_s and rounded once;
 *                    the centre has wq = 65535, so the total is never zero.  The weights are INTEGERS of 16 bits on purpose: every
 *                    sum is exact whatever its order, and the result the same for any selection algorithm.
 *   result           per component c:  out[p][c] = the smallest candidate value v with
 *                    2 * sum{wq_j : flow[q_j][c] <= v} >= sum{wq_j}.  Values compare as numbers: -0 and +0 are one value (+0 comes back).
 * tiled == 0: one thread per pixel reads global memory and bisects the order-preserving 32-bit key of the value in 32 steps, the
 * weights formed again on every visit: the definition.  tiled == 1: a 32 x 8 tile with its halo in LDS, a pixel's integer weights
 * computed once and kept in registers two to a word; bit-identical to the plain route, built for every radius.
 * NSFF_FLOW_MEDIAN_TILED is the measured default.  ONE launch for all pairs; fixed trip counts, no atomics, no data-dependent loop,
 * no synchronisation, no allocation: capturable.
 * 1 <= radius <= NSFF_FLOW_MEDIAN_MAX_RADIUS; sigma_i, sigma_s > 0 and finite; 1 <= P <= 65535; 1 <= H, W <= 32768; P * H * W < 2^31;
 * tiled 0 or 1; out overlapping flow: NSFF_ERR_INVALID.  A missing flow / grey / out NSFF_ERR_NULL.  flow and out 8-byte, grey 4-byte
 * aligned (NSFF_ERR_ALIGN).  All before the launch. */
#define NSFF_FLOW_MEDIAN_MAX_RADIUS 7
#define NSFF_FLOW_MEDIAN_TILED      1   /* the route nsff_pl_amd.optflow.refine_flow takes when not told */
typedef struct NsffFlowMedianArgs {
    int32_t n_pairs, H, W, radius;
    float   sigma_i, sigma_s;  int32_t tiled, pad_;
    const float* flow;  const float* grey;  const uint8_t* valid;  float* out;
} NsffFlowMedianArgs;
int     nsff_flow_median(const NsffFlowMedianArgs* args, void* stream);

/* ---- disparity from optical flow and camera poses (csrc/depth.hip; nsff_pl_amd/depth.py): the classical
 * stand-in for the reference's DPT step (preprocess.py:106-115).  For a static pixel flow plus two poses is a depth measurement
 * (motion parallax); where there is none an image-guided fill gives a dense map.  Entry points added without a change of
 * NSFF_ABI_VERSION: nothing that existed changes.  Every array is fp32 unless said otherwise, every plane (F, H, W) contiguous, and
 * every step below ONE fp32 operation in the order written (the file is built -ffp-contract=off; IEEE division), which the tests
 * compare bit for bit with numpy.  No atomics on floats, no device-side convergence test, no data-dependent loop, no
 * synchronisation, no allocation: every call is a fixed list of launches and capturable; the frame is a grid dimension of every
 * kernel.  Common refusals, all before a launch: a size outside the stated range, a bad flag or value or a scratch that is too
 * small NSFF_ERR_INVALID; a missing pointer NSFF_ERR_NULL; an array off its alignment NSFF_ERR_ALIGN.
 *
 * sparse   one launch for n_frames frames and both directions (0 forward: neighbour f + 1, flow_fw[f]; 1 backward: f - 1,
 *          flow_bw[f]); flows (F, H*W, 2) pixels.  Pm (F, 2, 12): per frame and direction the nine entries of G = M_n M_f^-1,
 *          row-major, and the three of e = M_n (C_f - C_n), with M = K diag(1,-1,-1) R^-1 and C the camera centre: a pixel (x, y, 1)
 *          of f at depth 1 / delta appears in n at delta * e + h, h = G (x, y, 1).  A row of twelve zeros: no vote (no neighbour,
 *          coincident centres).  At the pixel (x, y), integers as floats, per direction with the flow (u, v):
 *            hx = (G[0] * x + G[1] * y) + G[2];  hy = (G[3] * x + G[4] * y) + G[5];  hz = (G[6] * x + G[7] * y) + G[8]
 *            up = x + u;  vp = y + v;  r = 1f / hz
 *            ax = (e[0] - up * e[2]) * r;  ay = (e[1] - vp * e[2]) * r
 *            bx = up - hx * r;  by = vp - hy * r             (the parallax in pixels against the point at infinity)
 *            p2 = bx * bx + by * by;  ab = ax * bx + ay * by;  aa = ax * ax + ay * ay
 *            vote = row non-zero && |u|, |v| <= 1e7 (a NaN is not) && (valid == NULL || valid[f][d] != 0)
 *                   && (masks == NULL || masks[f] != 0) && hz > 0 && p2 >= min_parallax * min_parallax (fp32, formed on the host)
 *          and over the directions in the order fw, bw, each sum from 0:  num += vote ? ab : 0;  den += vote ? aa : 0;
 *          par += vote ? p2 : 0.  known = den > 0 && num > 0;  c = known ? par : 0 (the confidence, px^2);
 *          n = known ? par * (num / den) : 0 (so that the disparity is n / c).  valid (F, 2, H*W) uint8 and masks (F, H*W) uint8
 *          (0 dynamic, the polarity of nsff_motion_maps) are optional.  counts (F) int64, optional: the known pixels of each
 *          frame, an exact integer through the per-frame reduction; it needs `scratch`, nsff_disparity_sparse_scratch_bytes bytes,
 *          16-byte aligned, ZERO before its first use and left zero.  n_frames <= 65535, 1 <= H * W < 2^31; min_parallax >= 0;
 *          flows and counts 8-byte aligned.
 * push     one pyramid step of the planes c, n and grey, (F, H, W) -> (F, (H+1)/2, (W+1)/2): each coarse pixel takes the 2 x 2
 *          block of the finer level, clipped at the image, in row-major order -- s = v00; s = s + v01; s = s + v10; s = s + v11,
 *          the terms that exist -- c' = the sum of c, n' of n, grey' = the sum of grey / the block's pixel count.  Not for 1 x 1.
 * pull     one step down: d = c > 0 ? n / c : parent[y >> 1][x >> 1], parent the (F, (H+1)/2, (W+1)/2) level above; parent NULL
 *          (the 1 x 1 top): 0 in its place; c and n NULL: d = the parent's value alone, the nearest-neighbour upsampling.
 * relax    `iters` weighted-Jacobi iterations of d on the planes n, c and the guide grey:
 *            g_q = 1f / (1f + t * t), t = (grey_p - grey_q) / sigma, for the neighbours q = left, right, up, down inside the image,
 *            0 for those outside;  S = 0, Wt = 0, then in that order  S = S + (inside ? g_q * d_q : 0);  Wt = Wt + g_q
 *            num = n + lambda * S;  den = c + lambda * Wt;  d' = den > 0 ? num / den : d
 *          The iterations go back and forth between state[0] (the input) and state[1]; the result is in
 *          state[nsff_disparity_result_slot(iters, fused ? k : 1)].  fused == 0: one launch per iteration, the definition.
 *          fused == 1: k iterations per launch on a tile x tile block of pixels held in LDS with a halo of k pixels, bit-identical
 *          to the plain route for every iters (a last launch runs iters % k); (tile, k) one of the built pairs, (16, 2), (32, 2),
 *          (32, 3), (32, 4), (32, 6), or (0, 0) = NSFF_DISPARITY_TILE, NSFF_DISPARITY_K.  The weights are recomputed from grey
 *          (an iteration reads d, n, c, grey and writes d: 20 bytes a pixel).  0 <= iters <= 100000; lambda >= 0, sigma > 0, finite;
 *          n_frames * H * W < 2^31.
 * nsff_disparity_dense: the whole densification of F frames from n, c and grey: push to the 1 x 1 top, level after level
 *          (nsff_disparity_levels of them, the finest being level 0); pull from the top down to level `levels` (the top itself
 *          where levels equals their number); then at each of the finest `levels` levels, coarse to fine, the nearest-neighbour
 *          upsampling of the level above (at the top: its own pulled value) as the start of `iters` relax iterations.  disps
 *          (F, H, W): the result.  A frame without a known pixel comes out all zero.  1 <= levels <= nsff_disparity_levels(H, W);
 *          scratch: nsff_disparity_dense_scratch_bytes bytes (0 = the shape is refused), 16-byte aligned, any content. */
#define NSFF_DISPARITY_TILE   32   /* the fused route's default tile side ...                                    */
#define NSFF_DISPARITY_K      3    /* ... and iterations per launch (DESIGN.md section 11.5 has the measurement) */
#define NSFF_DISPARITY_FUSED  1    /* the route nsff_pl_amd.depth takes when not told: 1 fused, 0 plain          */
typedef struct NsffDisparitySparseArgs {
    int32_t n_frames, H, W;
    float   min_parallax;
    const float* flow_fw;  const float* flow_bw;  const float* Pm;
    const uint8_t* valid;  const uint8_t* masks;
    float* n;  float* c;  int64_t* counts;
    void* scratch;  int64_t scratch_bytes;
} NsffDisparitySparseArgs;
typedef struct NsffDisparityRelaxArgs {
    int32_t n_frames, H, W, iters;
    int32_t fused, tile, k, pad_;
    float   lambda, sigma;
    const float* n;  const float* c;  const float* grey;  float* state[2];
} NsffDisparityRelaxArgs;
typedef struct NsffDisparityDenseArgs {
    int32_t n_frames, H, W, levels;
    int32_t iters, fused, tile, k;
    float   lambda, sigma;
    const float* n;  const float* c;  const float* grey;  float* disps;
    void* scratch;  int64_t scratch_bytes;
} NsffDisparityDenseArgs;
int64_t nsff_disparity_sparse_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int     nsff_disparity_sparse(const NsffDisparitySparseArgs* args, void* stream);
int     nsff_disparity_push(const float* c, const float* n, const float* grey, float* c2, float* n2, float* grey2, int32_t n_frames,
                            int32_t H, int32_t W, void* stream);
int     nsff_disparity_pull(const float* c, const float* n, const float* parent, float* d, int32_t n_frames, int32_t H, int32_t W,
                            void* stream);
int     nsff_disparity_relax(const NsffDisparityRelaxArgs* args, void* stream);
/* host only: 0 or 1, the state buffer that holds the result of `iters` iterations run k per launch (k = 1: the plain route);
 * negative for iters < 0 or k < 1 */
int     nsff_disparity_result_slot(int32_t iters, int32_t k);
/* host only: the number of levels of the pyramid of an H x W image down to 1 x 1 (0: a refused shape) */
int     nsff_disparity_levels(int32_t H, int32_t W);
int64_t nsff_disparity_dense_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int     nsff_disparity_dense(const NsffDisparityDenseArgs* args, void* stream);

/* ---- disparity triangulated over several frames by chaining optical flow (csrc/parallax.hip; nsff_pl_amd/depth.py with span > 1;
 * DESIGN.md section 11.5).  The measurement of `sparse` above sees the neighbours f +- 1 only: a slow camera's parallax per frame
 * stays below min_parallax and nothing is measured, a fast camera's is measured against one frame's baseline.  Here a pixel is
 * followed along the flow for up to `span` frames and votes against every baseline it reaches: the parallax grows with the number
 * of frames k, a chained flow's noise like sqrt(k).  Entry points added without a change of NSFF_ABI_VERSION: nothing that existed
 * changes.  The conventions and the common refusals of the section above hold (fp32, one fp32 operation per step in the order
 * written, the file built -ffp-contract=off, compared bit for bit with numpy); ONE launch for all frames, both directions and all
 * hops; no atomics on floats, no data-dependent loop, no synchronisation, no allocation: capturable.
 *
 * Frame f, direction d (0: s = +1 with flow_fw; 1: s = -1 with flow_bw), pixel p = (x, y), integers as floats.  Pm (F, 2, span, 12):
 * row k - 1 of (f, d) is the row of `sparse` for the neighbour n = f + s * k (G = M_n M_f^-1, e = M_n (C_f - C_n)); twelve zeros: no
 * vote (coincident centres; beyond the sequence ends the row is not read).
 *   A_1 = flow_d[f][y][x]
 *   alive_1 = known(A_1) && (valid == NULL || valid[f][d][p] != 0) && (masks == NULL || masks[f][p] != 0)
 *             known: both components |.| <= 1e7, a NaN is not (as `sparse`)
 *   for k = 1 .. span, n = f + s * k; the direction ends where n leaves 0 .. F-1:
 *     vote  with (u, v) = A_k and the row Pm[f][d][k-1]: hx, hy, hz, up, vp, r, ax, ay, bx, by, p2, ab, aa exactly as `sparse`
 *           states them (x, y the pixel's own coordinates in f);
 *           vote = alive_k && row non-zero && hz > 0 && p2 >= min_parallax * min_parallax (fp32, formed on the host)
 *           num += vote ? ab : 0;  den += vote ? aa : 0;  par += vote ? p2 : 0;  votes += vote
 *           (a zero row has no vote, and the chain goes on)
 *     hop   only if k < span and n + s is inside 0 .. F-1:  q = (up, vp), the same two floats as in the vote
 *           inside = 0 <= qx <= W-1 && 0 <= qy <= H-1
 *           b = flow_d[n] sampled bilinearly at q by the rule of nsff_motion_maps: x0 = floorf(qx), ax = qx - x0,
 *               x1 = min(x0 + 1, W-1), y likewise, per component
 *               b = ((B00 * (1 - ax) + B01 * ax) * (1 - ay)) + ((B10 * (1 - ax) + B11 * ax) * ay),  Bij = flow_d[n][yi][xj]
 *           hop_ok = inside && all four taps known && (valid == NULL || the four taps of valid[n][d] != 0)
 *                    && (masks == NULL || the four taps of masks[n] != 0)
 *           alive_{k+1} = alive_k && hop_ok;  A_{k+1} = A_k + b, per component
 *   The sums start from 0 and take d = 0 with k = 1 .. span, then d = 1 with k = 1 .. span: with span == 1 the order of `sparse`, and
 *   the same bits.  Then, as there:  known = den > 0 && num > 0;  c = known ? par : 0;  n = known ? par * (num / den) : 0.
 * The taps are read from q clamped into the image (the identity where q is inside, where alone a chain stays alive), so no
 * address leaves a frame whatever the flow holds; what a dead chain goes on adding up is never used.
 * valid (F, 2, H*W) uint8 and masks (F, H*W) uint8 (0 dynamic) are optional.  votes (F, H*W) uint8, optional: the votes of a pixel,
 * at most 2 * span.  counts (F) int64, optional: the known pixels of each frame, an exact integer through the per-frame reduction;
 * it needs `scratch`, nsff_disparity_span_scratch_bytes bytes, 16-byte aligned, ZERO before its first use and left zero.
 * 1 <= span <= NSFF_DISPARITY_MAX_SPAN, n_frames <= 65535, 1 <= H * W < 2^31, min_parallax >= 0 (else NSFF_ERR_INVALID); flows and
 * counts 8-byte, Pm, n, c and votes 4-byte aligned (NSFF_ERR_ALIGN) -- all before the launch.
 * Bytes: per pixel and direction 10 for the first vote (flow, valid, mask) and 10 of unique taps per hop -- the 40 a lane issues
 * per hop overlap between neighbouring pixels -- and 8 written (+1 with votes): about (20 * span + 9) bytes a pixel. */
#define NSFF_DISPARITY_MAX_SPAN 8
typedef struct NsffDisparitySpanArgs {
    int32_t n_frames, H, W, span;              /* 1 <= span <= NSFF_DISPARITY_MAX_SPAN */
    float   min_parallax;  int32_t pad_;
    const float* flow_fw;  const float* flow_bw;     /* (F, H*W, 2)                          */
    const float* Pm;                                 /* (F, 2, span, 12)                     */
    const uint8_t* valid;  const uint8_t* masks;     /* optional, as nsff_disparity_sparse   */
    float* n;  float* c;  uint8_t* votes;  int64_t* counts;   /* votes, counts optional      */
    void* scratch;  int64_t scratch_bytes;
} NsffDisparitySpanArgs;
int64_t nsff_disparity_span_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int     nsff_disparity_span(const NsffDisparitySpanArgs* args, void* stream);

/* ---- motion masks over several frames: the chained epipolar test and the propagation of "dynamic" along the flow
 * (csrc/motionspan.hip; nsff_pl_amd/motion.py with span > 1 / reach > 0).  nsff_motion_maps tests a pixel's
 * flow against the neighbours f +- 1 only: an object that drifts less than `threshold` a frame off its epipolar line is never
 * flagged, and an object that pauses is static in the frames of the pause.  nsff_motion_span follows a pixel along the flow for up
 * to `span` frames and tests it against every line it reaches; nsff_mask_propagate carries "dynamic" from the frames f +- 1 ..
 * f +- reach back along the same chain.  Entry points added without a change of NSFF_ABI_VERSION: nothing that existed changes.
 * The conventions of nsff_disparity_span hold (fp32, one fp32 operation per step in the order written, IEEE division and square
 * root, the file built -ffp-contract=off, compared bit for bit with numpy); ONE launch each for all frames, both directions and
 * all hops; no atomics on floats, no data-dependent loop beyond the fixed hop count, no synchronisation, no allocation: capturable.
 * known(w): both components |.| <= 1e7, a NaN is not (nsff_motion_maps' rule).  UNKNOWN = NSFF_FLOW_UNKNOWN = 1e10.
 *
 * nsff_motion_span.  flow_fw, flow_bw (F, H*W, 2).  Fm (F, 2, span, 3, 3): row k - 1 of (f, d) maps a pixel of f to its line in
 * f + k (d = 0) / f - k (d = 1); a zero matrix beyond the sequence ends and for coincident centres.  valid (F, 2, H*W) uint8,
 * optional.  hop_scale (span).  Frame f, direction d (0: s = +1 with A = flow_fw; 1: s = -1 with A = flow_bw), pixel p = (x, y),
 * integers as floats:
 *   alive = known(A[f][p]) && (valid == NULL || valid[f][d][p] != 0);  (u, v) = A[f][p];  best = 0;  hops = 0
 *   for k = 1 .. span, nb = f + s * k; the direction ends where nb leaves 0 .. F-1:
 *     q = (x + u, y + v)
 *     with M = Fm[f][d][k-1]:  l_i = (M[i][0] x + M[i][1] y) + M[i][2],  r = (l0 qx + l1 qy) + l2,  n = l0 l0 + l1 l1,
 *       e = |r| / sqrtf(n)                                                   (exactly as nsff_motion_maps forms them)
 *     if alive && isfinite(n) && n > 0:  best = fmaxf(best, e * hop_scale[k-1]);  hops += 1
 *     hop, only if k < span and nb + s is inside 0 .. F-1:
 *       inside = 0 <= qx <= W-1 && 0 <= qy <= H-1
 *       b = flow_d[nb] sampled bilinearly at q by the rule of nsff_motion_maps: x0 = floorf(qx), ax = qx - x0,
 *           x1 = min(x0 + 1, W-1), y likewise, per component
 *           b = ((B00 * (1 - ax) + B01 * ax) * (1 - ay)) + ((B10 * (1 - ax) + B11 * ax) * ay),  Bij = flow_d[nb][yi][xj]
 *       hop_ok = inside && all four taps known && (valid == NULL || the four taps of valid[nb][d] != 0)
 *                (the hop of nsff_disparity_span; there is no mask test here)
 *       alive = alive && hop_ok;  (u, v) = (u + b_u, v + b_v)
 *   err[f][d][p] = hops ? best : UNKNOWN;  hops[f][d][p] = hops;  over_d = hops > 0 && best > threshold
 *   raw[f][p] = over_fw || over_bw ? 0 : 255                                 (the reference's polarity: 0 dynamic)
 * err (F, 2, H*W) fp32 and hops (F, 2, H*W) uint8 are optional; raw (F, H*W) uint8 is not.  counts (F, 3) int64, optional:
 * [over fw, over bw, dynamic pixels of raw], exact integers through the per-frame reduction; it needs `scratch`,
 * nsff_motion_span_scratch_bytes bytes, 16-byte aligned, ZERO before its first use and left zero.  With span == 1, hop_scale = {1}
 * and nsff_motion_maps' own `valid`, raw and the over-counts are nsff_motion_maps'.
 * The taps are read from q clamped into the image (the identity where q is inside, where alone a chain stays alive), so no
 * address leaves a frame whatever the flow holds; what a dead chain goes on adding up is never used.
 * 1 <= span <= NSFF_MOTION_MAX_SPAN, n_frames <= 65535, 1 <= H * W < 2^31, threshold >= 0, scratch_bytes large enough (else
 * NSFF_ERR_INVALID); flow_fw, flow_bw, Fm, hop_scale, raw, and scratch with counts, not NULL (NSFF_ERR_NULL); scratch 16-byte,
 * flows and counts 8-byte, Fm, hop_scale and err 4-byte aligned (NSFF_ERR_ALIGN) -- all before the launch.
 * Bytes: per pixel and direction 9 for the first step (flow, valid) and 10 of unique taps per hop, and 11 written a pixel (err,
 * hops, raw): about (20 * span + 9) a pixel.
 *
 * nsff_mask_propagate.  src (F, H*W) uint8, 0 = dynamic; flows and valid as above.  Per pixel and direction alive and (u, v) start
 * as above, hits = 0:
 *   for k = 1 .. reach, nb = f + s * k; the direction ends where nb leaves 0 .. F-1:
 *     q = (x + u, y + v);  inside = 0 <= qx <= W-1 && 0 <= qy <= H-1
 *     xi = (int)rintf(qx), yi = (int)rintf(qy)         (round half to even, numpy's rint; used only where inside)
 *     if alive && inside && src[nb][yi][xi] == 0:  hits += 1
 *     hop exactly as above (k < reach, nb + s inside 0 .. F-1)
 *   dst[f][p] = (src[f][p] == 0 || hits_fw + hits_bw > 0) ? 0 : src[f][p]
 * hits (F, H*W) uint8, optional: hits_fw + hits_bw, at most 2 * reach.  zero_counts (F) int64, optional: the zero pixels of each
 * frame of dst, with the same scratch rule (nsff_motion_span_scratch_bytes covers both calls).
 * 1 <= reach <= NSFF_PROPAGATE_MAX_REACH, the frame limits above, dst must not overlap src, scratch_bytes large enough (else
 * NSFF_ERR_INVALID); src, dst, flow_fw, flow_bw, and scratch with zero_counts, not NULL (NSFF_ERR_NULL); scratch 16-byte, flows and
 * zero_counts 8-byte aligned (NSFF_ERR_ALIGN) -- all before the launch.
 * Bytes: per pixel and direction 9 for the first step, 1 of mask per step and 10 of unique taps per hop; 2 read and written a
 * pixel (src, dst; +1 with hits): (22 * reach + 1) a pixel with hits. */
#define NSFF_MOTION_MAX_SPAN 8
#define NSFF_PROPAGATE_MAX_REACH 8
typedef struct NsffMotionSpanArgs {
    int32_t n_frames, H, W, span;              /* 1 <= span <= NSFF_MOTION_MAX_SPAN */
    float   threshold;  int32_t pad_;
    const float* flow_fw;  const float* flow_bw;     /* (F, H*W, 2)                          */
    const float* Fm;                                 /* (F, 2, span, 3, 3)                   */
    const float* hop_scale;                          /* (span)                               */
    const uint8_t* valid;                            /* (F, 2, H*W), optional                */
    float* err;  uint8_t* hops;  uint8_t* raw;  int64_t* counts;      /* err, hops, counts optional */
    void* scratch;  int64_t scratch_bytes;
} NsffMotionSpanArgs;
typedef struct NsffMaskPropagateArgs {
    int32_t n_frames, H, W, reach;             /* 1 <= reach <= NSFF_PROPAGATE_MAX_REACH */
    const uint8_t* src;                              /* (F, H*W), 0 dynamic                  */
    const float* flow_fw;  const float* flow_bw;     /* (F, H*W, 2)                          */
    const uint8_t* valid;                            /* (F, 2, H*W), optional                */
    uint8_t* dst;  uint8_t* hits;  int64_t* zero_counts;              /* hits, zero_counts optional */
    void* scratch;  int64_t scratch_bytes;
} NsffMaskPropagateArgs;
int64_t nsff_motion_span_scratch_bytes(int32_t n_frames, int32_t H, int32_t W);
int     nsff_motion_span(const NsffMotionSpanArgs* args, void* stream);
int     nsff_mask_propagate(const NsffMaskPropagateArgs* args, void* stream);

/* cdf (n_frames, n) fp64 = per-frame inclusive prefix sum of weights (n_frames, n) fp32 (non-negative). */
int nsff_cdf(const float* weights, int64_t n_frames, int64_t n, double* cdf, void* stream);

/* One training batch of frame `frame` (datasets/monocular.py:233-250) drawn and gathered in one launch: for each b < batch,
 * idx = first i with cdf[frame][i] > u[b] * cdf[frame][n-1] (cdf non-NULL and that total > 0 and finite), else
 * floor(u[b] * n_pixels); then the columns of records[frame][idx] go to rays (B,6), rgbs (B,3), ts (B, int64, = (int64) t),
 * disps (B), rays_mask (B), uv_fw (B,2), uv_bw (B,2); cam_ids (B, int64) zeros and rand_idx (B, int64) = idx where non-NULL.
 * records (n_frames, n_pixels, NSFF_RAY_RECORD) 16-byte aligned; u (B) in [0, 1). */
typedef struct NsffRayDrawArgs {
    int64_t n_frames, n_pixels, frame, batch;
    const float* records;  const double* cdf;  const float* u;
    float* rays;  float* rgbs;  int64_t* ts;  int64_t* cam_ids;  float* disps;  float* rays_mask;  float* uv_fw;  float* uv_bw;
    int64_t* rand_idx;
} NsffRayDrawArgs;
int nsff_ray_draw(const NsffRayDrawArgs* args, void* stream);

/* ---- profiling hooks used by bench.py (HIP events around field-query launches) ---- */
int nsff_prof_enable(int on);
/* Synchronises the recorded events; returns launches, summed milliseconds and summed
 * algorithmic FLOPs (2*MACs of the reference's Linear layers, unpadded K) since the last reset, and the FLOPs the
 * kernels executed for them: inference launches evaluate the heads that read the activation-free
 * *_xyz_encoding_final layers (nerf.py:170,195) with pre-multiplied rows and skip those 256x256 layers. */
int nsff_prof_collect(int64_t* launches, double* total_ms, double* total_flops, double* executed_flops);
/* The same, plus the shader clock the f16 / f16x3 field kernels ran at: while profiling is on a sample of every launch's
 * workgroups measure their own lifetime with s_memtime (shader-clock ticks) and s_memrealtime (the constant-rate wall clock,
 * hipDeviceAttributeWallClockRate); this call returns the summed shader ticks and the summed wall time of those lifetimes in
 * milliseconds: clock [GHz] = shader_ticks / ticks_ms * 1e-6 (0 / 0 when nothing was measured, e.g. exact-fp32 launches). */
int nsff_prof_collect_clock(int64_t* launches, double* total_ms, double* total_flops, double* executed_flops,
                            double* shader_ticks, double* ticks_ms);

/* Which kernel the LAST nsff_field_query of this process launched (diagnostics; tests assert that large inference launches run
 * the hand-scheduled body and not a fallback): */
#define NSFF_KERNEL_F32       1   /* nsff_field_kernel: exact fp32 MFMA                                               */
#define NSFF_KERNEL_H3_64     2   /* f16x3, 64-point tiles (launches below 32768 points, tile_points = 64)           */
#define NSFF_KERNEL_H3_8WAVE  3   /* f16x3, 128-point tiles, eight waves of 32 neurons, compiler-scheduled           */
#define NSFF_KERNEL_H3A       4   /* f16x3, 128-point tiles, hand-scheduled body (nsff_field_kernel_h3a)             */
#define NSFF_KERNEL_H3_SAVE   5   /* f16x3 training forward (keeps activations)                                      */
/*      (6: the single-product fast mode of earlier ABI versions, removed) */
#define NSFF_KERNEL_H3A_TBIAS 7   /* NSFF_KERNEL_H3A with the time code folded into per-ray bias rows (NsffFieldArgs::t_bias) */
#define NSFF_KERNEL_H3A_SAVE  9   /* f16x3 training forward on the hand-scheduled body (nsff_field_kernel_h3a_save)          */
#define NSFF_KERNEL_H3A_SIDE  8   /* NSFF_KERNEL_H3A[_TBIAS] whose static trunk has the view-direction branch (NsffFieldArgs::s_bias) */
int         nsff_last_field_kernel(void);
/* Workgroups of that launch when it ran the hand-scheduled inference kernel (0 otherwise).  Large launches of that kernel are
 * PERSISTENT: one workgroup per compute unit, each walking tiles  first, first + stride, ...  of one trunk (both trunks: the
 * workgroups of XCDs 0..3 take the static trunk, 4..7 the dynamic one -- taken when both trunks cost the same number of matrix
 * steps); the plain bias rows are loaded once per workgroup, the next tile's first eight weight slots are requested by the last
 * trunk phase of the current one and its point by the body's first instructions.  Results are bit-identical to the one-workgroup-per-tile form (environment
 * NSFF_NO_PERSIST=1, read per launch, selects that form for A/B measurements). */
int         nsff_last_field_grid(void);
/* The MFMA shape of the hand-scheduled inference kernel's trunk phases.  nsff_field_kernel_h3a multiplies with
 * v_mfma_f32_32x32x16_f16; nsff_field_kernel_h3a16 runs the same schedule, phase programs and arguments on v_mfma_f32_16x16x32_f16
 * and reads a second packed buffer: the f16x3 pack with the trunk segments' 16-byte chunks in that operand's order
 * (nsff_repack_field_weights; same size, same offsets, everything but the trunk segments copied).  It covers the inference launches
 * of models without the view-direction branch (kernel codes NSFF_KERNEL_H3A / _TBIAS, unchanged), whatever their size or form, and
 * is what nsff_field_query_repacked runs there; nsff_field_query, which has no second buffer, runs the 32 shape.  Environment
 * NSFF_H3A_SHAPE=16 | 32, read per launch, forces either.  Records differ between the shapes in fp32 summation order only.
 *   nsff_field_mfma_shape       host-only: the shape nsff_field_query_repacked would run these arguments on (16 or 32; < 0: error)
 *   nsff_repack_field_weights   asynchronous on `stream`: repacked <- packed (nsff_packed_bytes of the f16x3 pack, 16-byte aligned)
 *   nsff_field_query_repacked   nsff_field_query given both buffers; a launch planned for shape 16 through nsff_field_query, which
 *                               has no second buffer, returns NSFF_ERR_NULL instead of running another kernel
 *   nsff_last_field_mfma_shape  the shape of the last f16x3 launch of this process (0: none yet) */
int         nsff_field_mfma_shape(const NsffModelDesc* desc, const NsffFieldArgs* args);
int         nsff_repack_field_weights(const NsffModelDesc* desc, const void* packed, void* repacked, void* stream);
int         nsff_field_query_repacked(const NsffModelDesc* desc, const void* packed, const void* repacked, const NsffFieldArgs* args,
                                      void* stream);
int         nsff_last_field_mfma_shape(void);
/* Host-only (no GPU work): the f16x3 step program of an inference launch with these modes -- steps[n][4] = {weight segment
 * offset (words), bias offset (words; 0xFFFFFFFF = accumulate), nks | pre << 8 | post << 16 | head << 24, 0} -- and the phase
 * programs (8-dword descriptors, 36 at most per trunk) the hand-scheduled kernel would execute for its static / dynamic trunk;
 * n_phases[t] = 0 when trunk t is absent or not covered by that kernel.  Used by the tests that pin the host-side program
 * builder to the one the simulator runs (tools/h3asm/check.py).  steps: room for 28 x 4, phases_*: room for 36 x 8.
 * fold_t != 0: the dynamic trunk's program of a launch that was given NsffFieldArgs::t_bias (bias fields of its descriptors
 * then index a table whose per-ray rows follow the plain ones: half A's row replaces the layer's bias row, half B's is appended).
 * fold_t bit 1: the static trunk's program of a view-direction launch given NsffFieldArgs::s_bias; bit 2: the programs of a
 * PERSISTENT launch (nsff_last_field_grid): the last segment's B phase carries descriptor 0's stream fields and requests the
 * first segments' weight slots 0..7 for the workgroup's next tile (n_phases[t] = 0 for a trunk that ends with a skip layer). */
int         nsff_field_phase_program(const NsffModelDesc* desc, int static_mode, int transient_mode, int fold_t, uint32_t* steps,
                             int* n_steps, int* n_static_steps, uint32_t* phases_static, uint32_t* phases_dynamic, int* n_phases);

/* Host-only (no GPU work; the pointers of `args` are tested against null and for alignment, never read): what nsff_field_query
 * would launch for these arguments on a device of n_cus compute units (no_persist != 0: as under NSFF_NO_PERSIST=1).  Only the
 * dispatcher's own checks run, not nsff_field_query's argument checks; `packed` and the stream are not part of the decision.
 * Returns the NSFF_KERNEL_* code nsff_last_field_kernel would report, or the dispatcher's negative error.  out: room for
 * max_launches (>= 3) records of NSFF_PLAN_WORDS int32, in issue order, unused records zeroed:
 *   [0] NSFF_LAUNCH_* kernel, [1] workgroups, [2] threads per workgroup, [3] p_mode (0 one workgroup per tile; 1..4 the persistent
 *   forms: one trunk / both by XCD / the dynamic trunk beside an eight-wave static launch / both, unequal cost), [4] p_tiles,
 *   [5] p_split, [6] p_long, [7] split_trunks, [8] grid_tiles, [9] time-bias rows in use (NsffFieldArgs::t_bias), [10] side-bias
 *   rows in use (s_bias), [11] FNV-1a (32 bit) of the kernel's argument bytes -- equal words mean equal launches.           */
#define NSFF_PLAN_WORDS 12
#define NSFF_LAUNCH_SIDE_TILE      1   /* nsff_side_tile_kernel: save_side from the per-ray codes                  */
#define NSFF_LAUNCH_H3_64          2   /* nsff_field_kernel_h3, 64-point tiles                                    */
#define NSFF_LAUNCH_H3_64_SAVE     3   /* ... its training forward                                                */
#define NSFF_LAUNCH_H3_8WAVE       4   /* nsff_field_kernel_h3, 128-point tiles, eight waves                      */
#define NSFF_LAUNCH_H3_8WAVE_SAVE  5   /* ... its training forward                                                */
#define NSFF_LAUNCH_H3A            6   /* nsff_field_kernel_h3a                                                   */
#define NSFF_LAUNCH_H3A_SAVE       7   /* nsff_field_kernel_h3a_save                                              */
int         nsff_field_launch_plan(const NsffModelDesc* desc, const NsffFieldArgs* args, int32_t n_cus, int32_t no_persist,
                                   int32_t* out, int32_t max_launches);

/* ---- f16x3 value-domain flag ----
 * The f16x3 kernels carry every fp32 operand as hi + lo halfs with hi = rtz_f16(x): exact to fp32 rounding only while
 * |x| <= 65504.  Every kernel that splits an fp32 value into fp16 MFMA operands ORs one bit per source into a sticky 32-bit
 * word of the current device when a value with !(|x| <= 65504) reached the split (inf included; NaN where the check sees it --
 * a ReLU or a max drops it).  Values are never changed: the flag only records.  The "f32" kernels never set a bit. */
#define NSFF_RANGE_ACT     0x1u   /* trunk activations / position input rows of an f16x3 inference launch          */
#define NSFF_RANGE_SAVED   0x2u   /* activations and input rows of the training forward (the fp16 tiles it saves)     */
#define NSFF_RANGE_PARAMS  0x4u   /* parameters at packing time (nsff_pack_weights f16x3, nsff_pack_weights_bwd)      */
#define NSFF_RANGE_CODES   0x8u   /* time / appearance / view-direction code columns of an f16x3 input tile           */
/* Asynchronous on `stream` (graph-capturable): one tiny kernel copies the current device's word to the DEVICE pointer `out`
 * and, clear != 0, zeroes it (atomically: a bit set concurrently is either reported or kept). */
int         nsff_range_flags(uint32_t* out, int32_t clear, void* stream);

/* ---- LPIPS 0.1, net='alex', spatial=True (reference metrics.py:36-49, eval.py:176-178, 235-255).  DESIGN.md section 11. ----
 * The graph: x = 2 x - 1 when `normalize`; (x - shift) / scale per channel; AlexNet `features` with its five ReLU outputs tapped
 * (conv 3->64 k11 s4 p2 | maxpool 3 s2, conv 64->192 k5 p2 | maxpool 3 s2, conv 192->384 k3 p1 | conv 384->256 k3 p1 |
 * conv 256->256 k3 p1); per tap  sum_c lin[c] (n0[c] - n1[c])^2  of the channel-normalised features n = f / (|f| + 1e-10);
 * bilinear upsampling (align_corners = False) of the five maps to (H, W), and their sum.  fp32 operands and accumulation on the
 * fp32 MFMA.  The library holds no trained values: the caller supplies the 15 tensors. */
#define NSFF_LPIPS_MIN_SIZE  31   /* smallest H and W: below it the second pooling has no output pixel */

/* The 15 fp32 device tensors in torch's layouts: conv_w[l] (cout, cin, k, k), conv_b[l] (cout), lin[l] (cout) for the five
 * layers above.  nsff_lpips_pack writes them into `packed` (nsff_lpips_packed_bytes bytes, 16-byte aligned) in the order the
 * convolution kernels stream: per layer the weights as [cout / 64][k][64] with k = (ky, kx, c), c fastest (the first layer's 33
 * (kx, c) of a kernel row padded to 36 with zeros), then the bias and the lin vector.  Five small launches on `stream`. */
typedef struct NsffLpipsWeights {
    const float* conv_w[5];  const float* conv_b[5];  const float* lin[5];
} NsffLpipsWeights;
int64_t nsff_lpips_packed_bytes(void);
int     nsff_lpips_pack(const NsffLpipsWeights* weights, float* packed, void* stream);

/* hw[2 l], hw[2 l + 1] = height and width of tap l's feature map for an H x W image (288 x 512: 71 x 127, 35 x 63, 17 x 31
 * three times); NSFF_ERR_INVALID below NSFF_LPIPS_MIN_SIZE.  Host only. */
int     nsff_lpips_dims(int32_t H, int32_t W, int32_t* hw);

/* n_frames image pairs gt / pred (F, H, W, 3) fp32, HWC, contiguous -- one batch of 2 F images, the launch count does not
 * depend on F.  Outputs (at least one):
 *   map   (F, H*W) fp32   the spatial LPIPS map;
 *   sums  (F, 3) fp64     per frame: sum of the map over all pixels, the same over the pixels with valid != 0, and the number
 *                         of those pixels (valid (F, H*W) uint8 or NULL = none selected; valid needs sums).  Added in a fixed
 *                         order that depends on H * W alone: a frame's numbers are the same bits alone or in a batch.
 * workspace: nsff_lpips_workspace_bytes bytes (0 = the shape is refused), 16-byte aligned, any content; one call at a time per
 * workspace.  Refused before any launch: H or W below NSFF_LPIPS_MIN_SIZE, H * W >= 2^31, n_frames outside 1 .. 32767, no output,
 * a workspace that is too small (NSFF_ERR_INVALID); a missing gt / pred / packed / workspace (NSFF_ERR_NULL); NSFF_ERR_ALIGN.
 * Asynchronous on `stream`, allocates nothing, capturable. */
typedef struct NsffLpipsArgs {
    int32_t n_frames, H, W, normalize;
    const float* gt;  const float* pred;  const uint8_t* valid;
    const float* packed;
    float* map;  double* sums;
    void* workspace;  int64_t workspace_bytes;
} NsffLpipsArgs;
int64_t nsff_lpips_workspace_bytes(int32_t n_frames, int32_t H, int32_t W);
int     nsff_lpips(const NsffLpipsArgs* args, void* stream);

/* ---- the scene scale from COLMAP points and mono-depth disparities (csrc/scale.hip): the per-pixel and
 * per-point work of the reference's nearest_depth loop, datasets/monocular.py:93-116, for all frames at once.  The O(F) rest --
 * slope, intercept, r^2, numpy's percentile interpolation, the r^2 branch, the minimum and the factor 0.75 -- is the caller's
 * (nsff_pl_amd/scene.py does it in numpy float64).
 * Inputs, all DEVICE memory:
 *   points (N, 3) fp64   COLMAP world points;                vis (F, N) uint8   1 where point i is visible in frame f;
 *   w2c (F, 3, 4) fp64   COLMAP world-to-camera [R | t];     K (3, 3) fp32      its nine values are converted to double as they are;
 *   disps (F, H, W) fp32 disparities at the training resolution.
 * The point pass (fp64, uncontracted): c = R p + t, uvd = K c, u = uvd.x / uvd.z, v = uvd.y / uvd.z, truncated toward zero and
 * clamped into the image (astype(int), then np.clip), x = 1 / uvd.z, y = (double)disps[f][v][u].  Points behind the camera are
 * not excluded (the reference does not).  A visible point with a non-finite u, v or x counts in n_nonfinite and is left out of
 * the moments.  Outputs:
 *   stats (F, 8) fp64     [n_vis, n_nonfinite, mean_x, mean_y, sxx, sxy, syy, n_nan_disp]: the means and the mean-centred sums
 *                         sum (x - mean_x)^2, sum (x - mean_x)(y - mean_y), sum (y - mean_y)^2 over the n_vis - n_nonfinite
 *                         points, from per-workgroup two-pass moments merged as (n, mean, M2) triples in a fixed order that
 *                         depends on N alone: a frame's numbers are the same bits alone or in a batch.  n_nan_disp: NaNs among
 *                         the frame's H * W disparities;
 *   disp_os (F, 2) fp32   the frame's disparities of ascending rank disp_rank[0] and disp_rank[1] (0-based; NaNs are not ranked,
 *                         -0 ranks as and comes back as +0; a rank beyond the ranked population gives NaN);
 *   depth_os (F, 2) fp64  the visible points' camera depths uvd.z of rank lo = floor((n_vis - 1) * 0.05) and min(lo + 1, n_vis - 1),
 *                         the product formed on the device in double (+inf where n_vis = 0);
 *                         unspecified for a frame with n_nonfinite > 0: a NaN depth is ranked by its bits;
 *   pix (F, N) int32      optional: the flat pixel index v * W + u a visible point gathered from, -1 not visible, -2 non-finite.
 * Both selections are exact radix selects (8-bit digits, most significant first, of an order-preserving 32- / 64-bit key;
 * integer histograms, so nothing depends on the launch order).
 * work: nsff_scene_scale_work_bytes bytes (0 = the shape is refused), 16-byte aligned, any content before a call; its counters
 * are zero again after it; one call at a time per workspace.  Refused before any launch: n_frames outside 1 .. 65535, H * W >= 2^31,
 * n_points < 1, a rank outside [0, H * W), a workspace that is too small (NSFF_ERR_INVALID); a missing pointer other than pix
 * (NSFF_ERR_NULL); fp64 arrays and work not 8- / 16-byte, fp32 / int32 arrays not 4-byte aligned (NSFF_ERR_ALIGN).
 * Asynchronous on `stream`, allocates nothing, capturable. */
typedef struct NsffSceneScaleArgs {
    int32_t n_frames, n_points, H, W;
    int32_t disp_rank[2];
    const double* points;  const uint8_t* vis;  const double* w2c;  const float* K;  const float* disps;
    double* stats;  float* disp_os;  double* depth_os;  int32_t* pix;
    void* work;  int64_t work_bytes;
} NsffSceneScaleArgs;
int64_t nsff_scene_scale_work_bytes(int32_t n_frames, int32_t n_points, int32_t H, int32_t W);
int     nsff_scene_scale(const NsffSceneScaleArgs* args, void* stream);

int         nsff_abi_version(void);
const char* nsff_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif /* NSFF_RENDER_H */
