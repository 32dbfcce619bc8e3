"""numpy restatement of nsff_val_panels (csrc/frames.hip), one frame at a time, in the number formats the reference's
validation step runs in (train.py:209-235 over utils/visualization.py:6-44 and torchvision's make_grid): fp32 arrays through
numpy's own fp32 operations, the shared chains taken from tests/frame_finish_numpy.py.

tests/test_panels_host.py checks these functions against golden g27 (the reference's own statements); the GPU tests compare the
kernels with them.  Three things are restated rather than run, as the golden's generator explains: cv2.addWeighted (the integer
form below), make_grid (its documented layout) and the colour maps (a table lookup)."""
import numpy as np

import frame_finish_numpy as ffn

FIELDS = ("depth", "static_depth", "neg_disp", "neg_rmse", "neg_ssim")


def trunc_u8(v):
    """astype(uint8) of an fp32 array with the kernel's clamp to 0..255 (NaN -> 0): equal to numpy's cast wherever that is
    defined."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return np.clip(np.where(np.isnan(v), np.float32(0), v), 0, 255).astype(np.uint8)


def float_u8(x):
    """An image tile: (255 * x) truncated."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        return trunc_u8(255 * x)


def rmse_map(gt, pred):
    """train.py:215, sqrt(((d0^2 + d1^2) + d2^2) / 3) with d = gt - clip(pred, 0, 1): every step one fp32 operation."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    assert gt.dtype == pred.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        d = gt - np.clip(pred, 0, 1)
        sq = d * d
        out = np.sqrt(((sq[..., 0] + sq[..., 1]) + sq[..., 2]) / np.float32(3))
    assert out.dtype == np.float32
    return out


def ssim_map(loss):
    """train.py:218, the channel mean of 1 - loss: (((1 - l0) + (1 - l1)) + (1 - l2)) / 3 in fp32."""
    loss = np.asarray(loss)
    assert loss.dtype == np.float32
    one = np.float32(1)
    out = (((one - loss[..., 0]) + (one - loss[..., 1])) + (one - loss[..., 2])) / np.float32(3)
    assert out.dtype == np.float32
    return out


def index_image(x):
    """visualize_depth's index image of (F, H, W) fp32, each frame on its own range."""
    return ffn.depth_u8(np.asarray(x))


def colour(idx, lut):
    """applyColorMap as a table; no table = the index in all three channels."""
    return np.repeat(idx[..., None], 3, -1) if lut is None else np.asarray(lut)[idx]


def blend(a, b):
    """cv2.addWeighted(a, .5, b, .5, 2.2) of two uint8 images = saturate(round(a / 2 + b / 2 + 2.2)), in integers."""
    s = a.astype(np.int32) + b.astype(np.int32)
    return np.minimum(255, (s >> 1) + 2 + (s & 1)).astype(np.uint8)


def blend_float(a, b, dtype):
    """The same formula evaluated in floating point (the form cv2 documents), for the check of the integer form."""
    v = a.astype(dtype) * dtype(0.5) + b.astype(dtype) * dtype(0.5) + dtype(2.2)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def make_grid(tiles, nrow=3, padding=2):
    """torchvision.utils.make_grid of equally sized (H, W, 3) uint8 tiles, pad_value 0, in HWC."""
    H, W = tiles[0].shape[:2]
    xmaps = min(nrow, len(tiles))
    ymaps = -(-len(tiles) // xmaps)
    grid = np.zeros((ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, 3), np.uint8)
    for k, t in enumerate(tiles):
        y, x = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        grid[y:y + H, x:x + W] = t
    return grid


def panels(pred, gt=None, depth=None, transient_alpha=None, static_rgb=None, static_depth=None, mask=None, disp=None,
           ssim_loss=None, lut_depth=None, lut_mask=None):
    """All outputs of nsff_val_panels for (F, H, W[, 3]) fp32 inputs: a dict with 'ranges' (F, 5, 2) (NaN rows for absent
    fields), 'rmse_u8', 'ssim_u8', 'rmse_blend_u8', 'ssim_blend_u8' and 'grid_u8' -- whichever the inputs allow."""
    pred = np.asarray(pred)
    F = len(pred)
    out = {"ranges": np.full((F, 5, 2), np.nan, np.float32)}
    pred_u8 = ffn.rgb_u8(pred)
    fields = {}
    with np.errstate(over="ignore", invalid="ignore"):
        if depth is not None:
            fields[0] = np.asarray(depth)
        if static_depth is not None:
            fields[1] = np.asarray(static_depth)
        if disp is not None:
            fields[2] = -np.asarray(disp)
        if gt is not None:
            fields[3] = -rmse_map(gt, pred)
        if ssim_loss is not None:
            fields[4] = -ssim_map(ssim_loss)
    idx = {}
    for t, x in fields.items():
        out["ranges"][:, t] = ffn.depth_range(x)
        idx[t] = index_image(x)
    for t, name in ((3, "rmse"), (4, "ssim")):
        if t in idx:
            out[name + "_u8"] = idx[t]
            out[name + "_blend_u8"] = blend(pred_u8, colour(idx[t], lut_depth))
    if gt is not None and depth is not None:
        grids = []
        for f in range(F):
            tiles = [float_u8(np.asarray(gt)[f]), pred_u8[f], colour(idx[0][f], lut_depth)]
            if transient_alpha is not None:
                tiles += [colour(float_u8(np.asarray(transient_alpha)[f]), lut_mask), ffn.rgb_u8(np.asarray(static_rgb)[f]),
                          colour(idx[1][f], lut_depth)]
            if mask is not None:
                tiles += [colour(float_u8(np.float32(1) - np.asarray(mask)[f]), lut_mask)]
            if disp is not None:
                tiles += [colour(idx[2][f], lut_depth)]
            grids.append(make_grid(tiles))
        out["grid_u8"] = np.stack(grids)
    return out
