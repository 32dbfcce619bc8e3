"""numpy restatement of the four resize rules of the reference's dataset constructor (datasets/monocular.py:98-99, 146-147,
158-163, 168-176; datasets/flowlib.py:320-338), as include/nsff_render.h states them.  Tables are (start, count, weights) per axis.

* lanczos: Pillow's precompute_coeffs + normalize_coeffs_8bpc and its two 8-bit passes, pinned by Pillow byte for byte (golden g28);
* nearest_pil: Pillow's running-sum affine nearest, pinned by Pillow;
* nearest_cv, linear_cv: OpenCV's resizeNN and fp32 INTER_LINEAR as stated in the header -- cv2 is not installed, so these two are
  pinned to the stated rule only.  The linear rule runs on fp32 arrays with one rounding per operation.

Pillow evaluates sin through the C library; so does math.sin, which numpy's vectorised sin need not match in the last place.
"""
import math

import numpy as np

LANCZOS_U8, NEAREST_PIL, NEAREST_CV, LINEAR_CV = range(4)
PRECISION_BITS = 22
MAX_KSIZE = 49


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def lanczos_ksize(n_in, n_out):
    return 2 * int(math.ceil(3.0 * max(n_in / n_out, 1.0))) + 1


def lanczos_table(n_in, n_out):
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 3.0 * fs, 1.0 / fs
    ksize = lanczos_ksize(n_in, n_out)
    start, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    weights = np.zeros((n_out, ksize), np.int32)
    for i in range(n_out):
        c = (i + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), n_in) - xmin
        k = [_lanczos((j + xmin - c + 0.5) * ss) for j in range(n)]
        ww = 0.0
        for w in k:
            ww += w
        for j, w in enumerate(k):
            if ww != 0.0:
                w = w / ww
            weights[i, j] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
        start[i], count[i] = xmin, n
    return start, count, weights


def nearest_pil_table(n_in, n_out):
    a = n_in / n_out
    x = 0.5 * a
    start = np.zeros(n_out, np.int32)
    for i in range(n_out):
        start[i] = min(int(x), n_in - 1)
        x += a
    return start, np.ones(n_out, np.int32), None


def nearest_cv_table(n_in, n_out):
    ifx = 1.0 / (n_out / n_in)
    start = np.array([min(int(math.floor(i * ifx)), n_in - 1) for i in range(n_out)], np.int32)
    return start, np.ones(n_out, np.int32), None


def linear_cv_table(n_in, n_out):
    scale = n_in / n_out
    start, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    weights = np.zeros((n_out, 2), np.float32)
    for i in range(n_out):
        fx = np.float32((i + 0.5) * scale - 0.5)
        sx = int(math.floor(fx))
        fx = fx - np.float32(sx)
        if sx < 0:
            sx, fx = 0, np.float32(0)
        if sx >= n_in - 1:
            sx, fx = n_in - 1, np.float32(0)
        start[i], count[i] = sx, min(sx + 1, n_in - 1) - sx + 1
        weights[i] = np.float32(1) - fx, fx
    return start, count, weights


def table(filter, n_in, n_out):
    return (lanczos_table, nearest_pil_table, nearest_cv_table, linear_cv_table)[filter](n_in, n_out)


def _pass_u8(img, tab, axis):
    """One of Pillow's 8-bit passes along `axis` of (..., H, W, C) uint8: int32 accumulator from 2^21, >> 22, clip."""
    start, count, weights = tab
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.zeros((len(start),) + src.shape[1:], np.uint8)
    for i in range(len(start)):
        k = weights[i, :count[i]].astype(np.int64)
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[start[i]:start[i] + count[i]], axes=(0, 0))
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)                 # Pillow's accumulator is an int32
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_lanczos(img, img_wh):
    """img (F, h, w, C) or (h, w, C) uint8 -> (.., H, W, C): PIL's img.resize(img_wh, Image.LANCZOS).  Horizontal first; a pass
    whose size does not change is skipped."""
    W, H = img_wh
    h, w = img.shape[-3], img.shape[-2]
    out = img
    if w != W:
        out = _pass_u8(out, lanczos_table(w, W), img.ndim - 2)
    if h != H:
        out = _pass_u8(out, lanczos_table(h, H), img.ndim - 3)
    return out.copy() if out is img else out


def _gather(x, iy, ix):
    """x (F, h, w[, C]) -> (F, H, W[, C])"""
    return x[:, iy][:, :, ix]


def resize_nearest_pil(mask, img_wh):
    """mask (F, h, w) uint8: PIL's mask.resize(img_wh, Image.NEAREST)"""
    W, H = img_wh
    return _gather(mask, nearest_pil_table(mask.shape[1], H)[0], nearest_pil_table(mask.shape[2], W)[0])


def resize_nearest_cv(disp, img_wh):
    """disp (F, h, w) fp32: cv2.resize(disp, img_wh, interpolation=cv2.INTER_NEAREST)"""
    W, H = img_wh
    return _gather(disp, nearest_cv_table(disp.shape[1], H)[0], nearest_cv_table(disp.shape[2], W)[0])


def flow_ratio(src_wh, img_wh):
    return np.array([np.float32(img_wh[0] / src_wh[0]), np.float32(img_wh[1] / src_wh[1])], np.float32)


def resize_flow(flow, img_wh):
    """flow (F, h, w, 2) fp32: flowlib.resize_flow(flow, W, H) -- the two rows' horizontal lerps, the vertical lerp, then the
    ratio; every step one fp32 operation."""
    assert flow.dtype == np.float32
    W, H = img_wh
    h, w = flow.shape[1:3]
    if (w, h) == (W, H):
        return flow.copy()
    sx, nx, wx = linear_cv_table(w, W)
    sy, ny, wy = linear_cv_table(h, H)
    x0, x1, y0, y1 = sx, sx + nx - 1, sy, sy + ny - 1
    a0, a1 = wx[None, None, :, 0, None], wx[None, None, :, 1, None]
    b0, b1 = wy[None, :, 0, None, None], wy[None, :, 1, None, None]
    r0, r1 = flow[:, y0], flow[:, y1]
    h0 = r0[:, :, x0] * a0 + r0[:, :, x1] * a1
    h1 = r1[:, :, x0] * a0 + r1[:, :, x1] * a1
    v = h0 * b0 + h1 * b1
    out = v * flow_ratio((w, h), img_wh)[None, None, None, :]
    assert out.dtype == np.float32
    return out


def scaled_intrinsics(f, src_wh, img_wh):
    """monocular.py:61-65"""
    W, H = src_wh
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=np.float32)
    K[0] *= img_wh[0] / W
    K[1] *= img_wh[1] / H
    return K
