"""numpy float64 restatement of the reference's scene-scale loop (datasets/monocular.py:93-116) and pose steps (:80, :120-134,
colmap_utils.center_poses), for tests/test_scene_scale_host.py and tests/test_scene_scale_gpu.py.  No scipy: the GPU box need
not have it.  Two things are stated explicitly where the reference leaves them to its libraries:

* ``w2c @ pts`` and ``K @ pts_c`` are the BLAS's dgemm, whose dot products on FMA hardware are chains ``fma(a_k, b_k, acc)`` in k
  order starting from the rounded first product.  :func:`project` is exactly those chains (an exact fma through fractions), so
  that depths and pixel indices are defined bit for bit; g29 pins that this is what the matmul gave.
* np.percentile's ``method='linear'`` as numpy 2.x computes it: the virtual index ``(n - 1) q`` with ``q = 95 / float32(100)`` in
  float32 for a float32 array and ``q = 5 / 100.0`` in float64 for a float64 one; floor, next index, ``_lerp`` in the array's dtype.

The regression is scipy.stats.linregress's arithmetic -- mean-centred moments, slope = sxy / sxx, r = sxy / sqrt(sxx syy) --
with the mean of y in float64; ``intercept_f32mean`` is the same with scipy's ``np.mean(y)`` in y's float32.
"""
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    """round(a * b + c), one rounding (finite doubles)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def project(K32, w2c, pts):
    """pts (n, 3) world points -> uvd (3, n): K @ (w2c @ [p; 1])[:3] as the fma chains of a dgemm.  w2c (3, 4)."""
    K = np.asarray(K32, np.float32).astype(np.float64)
    w2c, pts = np.asarray(w2c, np.float64), np.asarray(pts, np.float64)
    uvd = np.empty((3, len(pts)))
    for j, p in enumerate(pts):
        c = [0.0] * 3
        for r in range(3):
            acc = w2c[r, 0] * p[0]
            acc = fma(w2c[r, 1], p[1], acc)
            acc = fma(w2c[r, 2], p[2], acc)
            c[r] = acc + w2c[r, 3]                              # (fma(t, 1.0, acc))
        for r in range(3):
            acc = K[r, 0] * c[0]
            acc = fma(K[r, 1], c[1], acc)
            uvd[r, j] = fma(K[r, 2], c[2], acc)
    return uvd


def percentile_linear(a, q_percent):
    """np.percentile(a, q_percent) of numpy 2.x, method='linear', with its parts: (value, lo, hi, a_sorted[lo], a_sorted[hi])."""
    a = np.sort(np.asarray(a).ravel())
    t = a.dtype.type
    n = a.size
    index = t(n - 1) * (t(q_percent) / t(100))
    lo = int(np.floor(index))
    hi = min(lo + 1, n - 1)
    g = index - t(lo)
    lo_v, hi_v = a[lo] + t(0), a[hi] + t(0)                      # (+ 0: a -0.0 order statistic counts as +0.0, as the kernel ranks it)
    d = hi_v - lo_v
    value = hi_v - d * (t(1) - g) if g >= 0.5 else lo_v + d * g
    assert value.dtype == a.dtype
    return value, lo, hi, lo_v, hi_v


def frame_scale(K32, w2c_f, points, vis_f, disp):
    """One iteration of monocular.py:94-114 for a frame: every intermediate in a dict."""
    H, W = disp.shape
    uvd = project(K32, w2c_f, points[vis_f == 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = (uvd[:2] / uvd[2:]).T
    col = np.minimum(np.maximum(np.trunc(uv[:, 0]), 0), W - 1).astype(np.int64)      # truncation toward zero, then into the image
    row = np.minimum(np.maximum(np.trunc(uv[:, 1]), 0), H - 1).astype(np.int64)
    d = uvd[2]
    x, y32 = 1 / d, disp[row, col]
    y = y32.astype(np.float64)
    n = len(x)
    mx, my = x.sum() / n, y.sum() / n
    sxx, sxy, syy = ((x - mx) ** 2).sum(), ((x - mx) * (y - my)).sum(), ((y - my) ** 2).sum()
    slope = sxy / sxx
    r = 0.0 if sxx == 0.0 or syy == 0.0 else float(np.clip(sxy / np.sqrt(sxx * syy), -1.0, 1.0))
    intercept = my - slope * mx
    p95, _, _, d_lo, d_hi = percentile_linear(disp, 95)
    p5, _, _, z_lo, z_hi = percentile_linear(d, 5)
    used = r ** 2 > 0.9
    with np.errstate(divide="ignore"):
        candidate = slope / (p95 - intercept) if used else p5
        ymean32 = np.mean(y32)                                  # scipy's ymean: float32
        intercept32 = ymean32 - slope * mx
        candidate32 = slope / (p95 - intercept32) if used else p5
    pix = np.full(len(points), -1, np.int32)
    pix[vis_f == 1] = row * W + col
    return dict(n_vis=n, pix=pix, uv=uv, mean_x=mx, mean_y=my, sxx=sxx, sxy=sxy, syy=syy, slope=slope, r=r, r2=r ** 2,
                intercept=intercept, intercept_f32mean=float(intercept32), p95_disp=p95, p5_depth=p5,
                disp_os=np.array([d_lo, d_hi], np.float32), depth_os=np.array([z_lo, z_hi], np.float64), used_regression=used,
                candidate=float(candidate), candidate_f32mean=float(candidate32),
                abs_terms=dict(mean_x=np.abs(x).sum() / n, mean_y=np.abs(y).sum() / n, sxx=sxx,
                               sxy=np.abs((x - mx) * (y - my)).sum(), syy=syy))


def nearest_depth(K32, w2c, points, vis, disps, f32mean=False):
    """(nearest_depth, [frame dicts]); f32mean: with scipy's float32 mean of y, i.e. the reference's own number."""
    frames = [frame_scale(K32, w2c[f][:3], points, vis[f], disps[f]) for f in range(len(disps))]
    key = "candidate_f32mean" if f32mean else "candidate"
    return min([1e8] + [fr[key] for fr in frames]) * 0.75, frames


def _unit(v):
    return v / np.sqrt(v @ v)


def poses_and_Ps(K32, w2c44, scale):
    """The reference's final poses and projection matrices (monocular.py:80, 118-132) from rotations and camera centres, with
    transposes where it inverts (every matrix involved is a rotation): (poses (F,3,4), Ps (F,3,4)), float64.
    Camera f sits at C_f = -R_f^T t_f with axes R_f^T diag(1,-1,-1) ("right up back"); the average frame has the mean centre, the
    unit mean backward axis, right = unit(mean up x backward), up = backward x right; pose_f = [A^T Q_f | A^T (C_f - c) / scale]
    and Ps_f = K diag(1,-1,-1) [Q'^T | -Q'^T p'] of that pose."""
    R, t = w2c44[:, :3, :3], w2c44[:, :3, 3]
    flip = np.diag([1.0, -1.0, -1.0])
    Q = np.stack([Rf.T @ flip for Rf in R])
    C = np.stack([-Rf.T @ tf for Rf, tf in zip(R, t)])
    back = _unit(Q[:, :, 2].sum(0) / len(Q))
    right = _unit(np.cross(Q[:, :, 1].sum(0) / len(Q), back))
    A = np.stack([right, np.cross(back, right), back], axis=1)
    c = C.sum(0) / len(C)
    poses = np.stack([np.concatenate([A.T @ Qf, (A.T @ (Cf - c) / scale)[:, None]], 1) for Qf, Cf in zip(Q, C)])
    K = np.asarray(K32, np.float32).astype(np.float64)
    Ps = np.stack([K @ flip @ np.concatenate([P[:, :3].T, -(P[:, :3].T @ P[:, 3])[:, None]], 1) for P in poses])
    return poses, Ps


def visibility(point_index, image_id, n_points, start, end):
    """monocular.py:86-91: a pair counts where its frame row, image id - 1 - start, exists"""
    out = np.zeros((end - start, n_points), np.uint8)
    for point, image in zip(point_index, image_id):
        row = image - 1 - start
        if 0 <= row < end - start:
            out[row, point] = 1
    return out
