"""From a COLMAP model and mono-depth disparities to the poses a training run needs: the scene scale ``nearest_depth`` and the
centred, scaled camera-to-world matrices of the reference's dataset constructor (datasets/monocular.py:67-134).

* :func:`visibility_matrix` -- the (F, N) table of monocular.py:85-91 from flat (point, COLMAP image id) pairs, host numpy;
* :func:`nearest_depth`     -- monocular.py:93-116.  The per-point and per-pixel work of every frame -- projection, the gather of
                               the disparity, the regression's moments, two order statistics of the H*W disparities and two of the
                               visible depths -- is ONE ``nsff_scene_scale`` call (csrc/scale.hip); slope, intercept, r^2, numpy's
                               percentile interpolation, the ``r^2 > 0.9`` branch, the minimum over the frames and the factor 0.75
                               are numpy float64 on the (F, 8) table it returns;
* :func:`scene_from_colmap` -- the whole chain: K at the training resolution, the scale, the poses (axis flip, centring on the average frame,
                               division by the scale), ``Ks`` and ``Ps``.  ``RayBank.from_frames(d['K'], d['poses'], ...)`` takes
                               the result as it is.

One deviation from the reference, documented in DESIGN.md sections 5 and 11: ``scipy.stats.linregress`` forms ``ymean`` with
``np.mean(y)`` in y's dtype, float32 (the gathered disparities), so the reference's intercept carries a float32 rounding of that
mean.  Here the mean is float64.  The resulting relative difference of ``nearest_depth`` measured on the golden scenes is at
most 2.3e-8 (2.28e-8).

np.percentile is restated for numpy 2.x's ``method='linear'``: the virtual index is ``(n - 1) * q`` with ``q = 95 /
float32(100)`` -- float32 arithmetic -- for the float32 disparities and ``q = 5 / 100.0`` in float64 for the depths;
``lo = floor``, ``hi = min(lo + 1, n - 1)``, ``g = index - lo`` and ``_lerp`` in the array's dtype.
"""
import numpy as np
import torch

from . import _lib
from . import frames

__all__ = ["visibility_matrix", "nearest_depth", "scene_from_colmap", "corrected_poses"]

R2_AUTHENTIC = 0.9              # monocular.py:111


def _host(x, dtype):
    return np.ascontiguousarray(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x), dtype=dtype)


def visibility_matrix(point_index, image_id, n_points, start_end):
    """(F, N) uint8, 1 where point i was seen in frame f, from the flat pairs (point_index[k], image_id[k]) of a COLMAP
    ``points3D`` table: the reference's rule ``start <= id - 1 < end`` -> row ``id - 1 - start`` (monocular.py:87-91), with
    start_end = (start_frame, end_frame).  The rule goes by COLMAP's image id, not by the sorted file names."""
    point_index, image_id = _host(point_index, np.int64).ravel(), _host(image_id, np.int64).ravel()
    start, end = (int(v) for v in start_end)
    if point_index.shape != image_id.shape:
        raise ValueError(f"visibility_matrix: {point_index.size} point indices for {image_id.size} image ids")
    if end <= start or n_points < 1:
        raise ValueError(f"visibility_matrix: need start < end and n_points >= 1, got {start_end!r} and {n_points}")
    if point_index.size and (point_index.min() < 0 or point_index.max() >= n_points):
        raise ValueError(f"visibility_matrix: point indices must lie in [0, {n_points})")
    vis = np.zeros((end - start, int(n_points)), np.uint8)
    keep = (start <= image_id - 1) & (image_id - 1 < end)
    vis[image_id[keep] - 1 - start, point_index[keep]] = 1
    return vis


def percentile_ranks(n, q_percent, dtype):
    """numpy's method='linear' for np.percentile(a, q_percent) of n values of `dtype`: (lo, hi, g) with g of that dtype."""
    t = np.dtype(dtype).type
    index = t(n - 1) * (t(q_percent) / t(100))                  # every step in the array's dtype: float32 for float32 data
    lo = int(np.floor(index))
    return lo, min(lo + 1, n - 1), index - t(lo)


def lerp(a, b, g):
    """numpy's _lerp on scalars of one dtype: a + (b - a) g, and b - (b - a)(1 - g) where g >= 0.5."""
    d = b - a
    return b - d * (1 - g) if g >= 0.5 else a + d * g


def regression_table(stats, disp_os, depth_os, HW):
    """The O(F) arithmetic of monocular.py:110-114 on nsff_scene_scale's tables, numpy float64: per-frame arrays in a dict."""
    stats = np.asarray(stats, np.float64)
    F = stats.shape[0]
    n_vis, n_bad, n_nan = stats[:, 0].astype(np.int64), stats[:, 1].astype(np.int64), stats[:, 7].astype(np.int64)
    for f in range(F):
        if n_vis[f] < 2:
            raise ValueError(f"nearest_depth: frame {f} has {n_vis[f]} visible points, the regression needs at least 2")
        if n_bad[f]:
            raise ValueError(f"nearest_depth: frame {f} has {n_bad[f]} visible points whose projection is not finite "
                             "(a point in the camera's plane)")
        if n_nan[f]:
            raise ValueError(f"nearest_depth: frame {f} has {n_nan[f]} NaN disparities")
        if not stats[f, 4] > 0.0:
            raise ValueError(f"nearest_depth: all 1/depth values of frame {f} are identical, the regression is undefined")
    mx, my, sxx, sxy, syy = (stats[:, k] for k in (2, 3, 4, 5, 6))
    slope = sxy / sxx
    intercept = my - slope * mx
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(syy > 0.0, sxy / np.sqrt(sxx * syy), 0.0)       # scipy: r = 0 where the y are all equal
    r = np.clip(r, -1.0, 1.0)
    _, _, g = percentile_ranks(HW, 95, np.float32)
    disp_os = np.asarray(disp_os, np.float32)
    p95 = np.array([lerp(disp_os[f, 0], disp_os[f, 1], g) for f in range(F)], np.float32)
    depth_os = np.asarray(depth_os, np.float64)
    p5 = np.array([lerp(depth_os[f, 0], depth_os[f, 1], percentile_ranks(int(n_vis[f]), 5, np.float64)[2]) for f in range(F)])
    used = r ** 2 > R2_AUTHENTIC
    with np.errstate(divide="ignore", invalid="ignore"):
        candidate = np.where(used, slope / (p95 - intercept), p5)
    return dict(n_vis=n_vis, slope=slope, intercept=intercept, r2=r ** 2, r=r, p95_disp=p95, p5_depth=p5, candidate=candidate,
                used_regression=used, mean_x=mx, mean_y=my, sxx=sxx, sxy=sxy, syy=syy, disp_os=disp_os, depth_os=depth_os)


def nearest_depth(K, w2c, points, visibility, disps, img_wh=None, return_table=False):
    """The reference's ``nearest_depth`` (monocular.py:93-116): 0.75 x the minimum over the frames of
    ``slope / (percentile(disp, 95) - intercept)`` where the regression of the disparity on 1/depth has r^2 > 0.9, else of
    ``percentile(depths, 5)``.  A Python float; with return_table also the dict of per-frame arrays ``n_vis, slope, intercept,
    r2, p95_disp, p5_depth, candidate, used_regression, pix`` (and the moments and order statistics they come from).

    K (3,3) -- used as float32, the reference's ``self.K``; w2c (F,3,4) or (F,4,4) COLMAP world-to-camera matrices, uncorrected;
    points (N,3); visibility (F,N) (:func:`visibility_matrix`) -- GPU or host arrays; disps (F,h,w) fp32 GPU tensor, resized with
    :func:`frames.resize_disps` first where img_wh = (W, H) is given and differs.  The intercept's mean is float64, not scipy's
    float32 (see the module docstring).  ValueError, naming the frame: fewer than 2 visible points, all 1/depth identical,
    non-finite projections, NaN disparities -- the reference's own failures, stated up front."""
    if not isinstance(disps, torch.Tensor) or not disps.is_cuda:
        raise RuntimeError("nearest_depth: disps must be a GPU tensor: the scene scale runs only on the HIP kernels of "
                           "libnsff_hip.so (no CPU fallback)")
    if disps.dim() != 3 or disps.dtype != torch.float32:
        raise ValueError(f"nearest_depth: disps must be (F,h,w) float32, got {tuple(disps.shape)} {disps.dtype}")
    if img_wh is not None and (int(disps.shape[2]), int(disps.shape[1])) != tuple(int(v) for v in img_wh):
        disps = frames.resize_disps(disps, img_wh)
    F, H, W = (int(v) for v in disps.shape)
    K32 = _host(K, np.float32)
    w2c, points, vis = _host(w2c, np.float64), _host(points, np.float64), _host(visibility, np.float64)
    if w2c.ndim == 3 and w2c.shape[1:] == (4, 4):
        w2c = np.ascontiguousarray(w2c[:, :3])
    if K32.shape != (3, 3) or w2c.shape != (F, 3, 4):
        raise ValueError(f"nearest_depth: K must be (3,3) and w2c ({F},3,4) to go with disps {tuple(disps.shape)}, got "
                         f"{K32.shape} and {w2c.shape}")
    if points.ndim != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"nearest_depth: points must be (N,3) with N >= 1, got {points.shape}")
    N = points.shape[0]
    if vis.shape != (F, N):
        raise ValueError(f"nearest_depth: visibility must be ({F},{N}), got {vis.shape}")
    short = np.flatnonzero((vis == 1).sum(1) < 2)
    if short.size:
        raise ValueError(f"nearest_depth: frame {int(short[0])} has {int((vis[short[0]] == 1).sum())} visible points, the "
                         "regression needs at least 2")
    dev = disps.device
    lo, hi, _ = percentile_ranks(H * W, 95, np.float32)
    stats, disp_os, depth_os, pix = _lib.scene_scale(
        torch.from_numpy(points).to(dev), torch.from_numpy((vis == 1).astype(np.uint8)).to(dev), torch.from_numpy(w2c).to(dev),
        torch.from_numpy(K32).to(dev), disps.contiguous(), (lo, hi), want_pix=return_table)
    table = regression_table(stats.cpu().numpy(), disp_os.cpu().numpy(), depth_os.cpu().numpy(), H * W)
    scale = float(min(1e8, table["candidate"].min()) * 0.75)        # (min_depth starts at 1e8, monocular.py:93)
    if not return_table:
        return scale
    table["pix"] = pix.cpu().numpy()
    return scale, table


def _unit(v):
    return v / np.sqrt((v * v).sum())


def average_frame(c2w):
    """The frame the reference centres its poses on (colmap_utils.average_poses), as (A (3,3), c (3,)): c is the mean camera
    position; A's third column is the unit mean of the cameras' backward axes, its first the unit cross product of the mean up
    axis with that, its second completes the right-handed triad."""
    c2w = np.asarray(c2w, np.float64)
    c = c2w[:, :, 3].mean(axis=0)
    back = _unit(c2w[:, :, 2].mean(axis=0))
    right = _unit(np.cross(c2w[:, :, 1].mean(axis=0), back))
    return np.column_stack([right, np.cross(back, right), back]), c


def corrected_poses(w2c, scale):
    """COLMAP world-to-camera matrices (F,3,4) / (F,4,4) -> the reference's final ``poses`` (monocular.py:80, 118-125), float64.
    [R | t] inverts to the camera-to-world [R^-1 | -R^-1 t]; COLMAP's "right down front" axes become "right up back" by negating
    the second and third column; with the average frame (A, c) of those, a pose [Q | p] becomes [A^-1 Q | A^-1 (p - c) / scale]."""
    w2c = np.asarray(w2c, np.float64)
    R_inv = np.linalg.inv(w2c[:, :3, :3])
    Q = R_inv * np.array([1.0, -1.0, -1.0])
    p = -(R_inv @ w2c[:, :3, 3:])[:, :, 0]
    A, c = average_frame(np.concatenate([Q, p[:, :, None]], axis=2))
    A_inv = np.linalg.inv(A)
    return np.concatenate([A_inv @ Q, (A_inv @ (p - c).T).T[:, :, None] / scale], axis=2)


def scene_from_colmap(K_or_f, src_wh, img_wh, w2c, points, visibility, disps):
    """COLMAP arrays plus decoded disparities -> dict(K (3,3) fp32 at img_wh, poses (F,3,4) float64 centred and scaled,
    nearest_depth, Ks (1,3,3), Ps (1,F,3,4)): monocular.py:61-65 and 80-134.  K_or_f / src_wh as in
    :func:`frames.scaled_intrinsics`; the other arguments as in :func:`nearest_depth` (disps at any size, resized to img_wh)."""
    K = frames.scaled_intrinsics(K_or_f, src_wh, img_wh)
    scale = nearest_depth(K, w2c, points, visibility, disps, img_wh=img_wh)
    poses = corrected_poses(_host(w2c, np.float64), scale)
    Ks, Ps = frames.projection_matrices(K, poses)
    return dict(K=K, poses=poses, nearest_depth=scale, Ks=Ks, Ps=Ps)
