"""numpy restatement of nsff_frame_finish (csrc/frames.hip), one frame at a time, in the number formats eval.py runs in:
fp32 arrays through numpy's own fp32 operations (eval.py:183-184, 213-214, 222-223; utils/visualization.py:10-15 as
eval.py's save_depth calls it), the squared errors of metrics.py:6-12 formed in fp32 and added in float64.

tests/test_eval_split_host.py checks these functions against golden g25 (the reference's own statements); the GPU tests
compare the kernels with them."""
import numpy as np


def rgb_u8(rgb):
    """(255 * clip(rgb, 0, 1)).astype(uint8) of an fp32 array."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.float32
    return (255 * np.clip(rgb, 0, 1)).astype(np.uint8)


def depth_range(depth):
    """(min, max) fp32 of nan_to_num(depth) per frame: (F, 2)."""
    x = np.nan_to_num(np.asarray(depth))
    assert x.dtype == np.float32
    x = x.reshape(len(x), -1)
    return np.stack([x.min(1), x.max(1)], -1)


def depth_u8(depth):
    """The index image of visualize_depth for every frame of (F, H, W) fp32, each with its own range."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32
    out = np.empty(depth.shape, np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, frame in enumerate(depth):
            x = np.nan_to_num(frame)
            mi = np.min(x)
            ma = np.max(x)
            x = (x - mi) / (ma - mi + 1e-8)                 # fp32 throughout: 1e-8 is rounded to fp32 before the addition
            assert x.dtype == np.float32
            out[i] = (255 * x).astype(np.uint8)
    return out


def error_sums(gt, rgb, valid=None):
    """(F, 3) float64: sum of (gt - clip(rgb))^2 over every value of a frame, the same over the valid pixels, valid pixels --
    each square an fp32 number, the additions in float64 (math.fsum: the correctly rounded sum)."""
    import math
    gt, rgb = np.asarray(gt), np.asarray(rgb)
    assert gt.dtype == rgb.dtype == np.float32
    F = len(gt)
    sq = ((gt - np.clip(rgb, 0, 1)) ** 2).reshape(F, -1, 3)
    assert sq.dtype == np.float32
    out = np.zeros((F, 3))
    for i in range(F):
        out[i, 0] = math.fsum(sq[i].astype(np.float64).ravel())
        if valid is not None:
            sel = np.asarray(valid[i]).reshape(-1) != 0
            out[i, 1] = math.fsum(sq[i][sel].astype(np.float64).ravel())
            out[i, 2] = sel.sum()
    return out


def psnr_from_sums(sums, n_pixels):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (-10 * np.log10(sums[:, 0] / (3 * n_pixels))).astype(np.float32), \
               (-10 * np.log10(sums[:, 1] / (3 * sums[:, 2]))).astype(np.float32)
