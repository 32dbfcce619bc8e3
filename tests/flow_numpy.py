"""numpy restatement of nsff_flow_maps (csrc/flow.hip) in the number format the kernels run in: fp32 arrays through numpy's own
fp32 operations, one rounding per operation, in the order the header states -- the reference's ndc2world (ray_utils.py:142-145),
the geometric loss's projection (losses.py:99-116), flowlib's flow_to_image / compute_color (flowlib.py:132-239) and the
end-point error of flowlib.flow_error with fp32 terms added in float64.

tests/test_flow_host.py checks these functions against golden g26 (the reference's own statements); the GPU tests compare the
kernels with them."""
import math

import numpy as np

f32 = np.float32
UNKNOWN = f32(1e10)
THRESH = f32(1e7)
SEGMENTS = (15, 6, 4, 11, 13, 6)                            # RY, YG, GC, CB, BM, MR


def ndc2world(xyz, K4):
    """(..., 3) fp32 NDC -> world, eps = 1e-6: Rz = 2 / ((z - 1) - eps), Rx = (((-Rz) x) cx) / fx, Ry likewise."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32
    fx, fy, cx, cy = (f32(v) for v in K4)
    with np.errstate(all="ignore"):
        Rz = f32(2) / ((xyz[..., 2] - f32(1)) - f32(1e-6))
        Rx = (((-Rz) * xyz[..., 0]) * cx) / fx
        Ry = (((-Rz) * xyz[..., 1]) * cy) / fy
    out = np.stack([Rx, Ry, Rz], -1)
    assert out.dtype == np.float32
    return out


def project(xyz, K4, Ps, ts, max_t, direction):
    """xyz (F, N, 3) fp32, Ps (n, 3, 4) fp32, ts (F,) ints, direction 'fw' / 'bw' -> (uv (F, N, 2) fp32, valid (F, N) bool):
    uvd = ((p0 X + p1 Y) + p2 Z) + p3 with Ps[clamp(t + 1, max = max_t)] / Ps[clamp(t - 1, min = 0)], uv = uvd.xy / (|uvd.z| + 1e-8),
    valid = uvd.z > 0 and t < max_t / t > 0."""
    Ps = np.asarray(Ps).reshape(-1, 3, 4)
    assert Ps.dtype == np.float32
    world = ndc2world(xyz, K4)
    ts = np.asarray(ts).reshape(-1).astype(np.int64)
    if direction == "fw":
        idx, t_ok = np.minimum(ts + 1, max_t), ts < max_t
    else:
        idx, t_ok = np.maximum(ts - 1, 0), ts > 0
    P = Ps[np.clip(idx, 0, len(Ps) - 1)][:, None]             # (F, 1, 3, 4)
    X, Y, Z = world[..., 0:1], world[..., 1:2], world[..., 2:3]
    with np.errstate(all="ignore"):
        uvd = ((P[..., 0] * X + P[..., 1] * Y) + P[..., 2] * Z) + P[..., 3]
        uv = uvd[..., :2] / (np.abs(uvd[..., 2:]) + f32(1e-8))
        valid = (uvd[..., 2] > 0) & t_ok[:, None]
    assert uv.dtype == np.float32
    return uv, valid


def induced_flow(xyz, K4, Ps, ts, max_t, H, W, direction):
    """(F, H, W, 2) fp32: uv minus the integer pixel coordinates; (UNKNOWN, UNKNOWN) where the pixel is not valid."""
    F = len(xyz)
    uv, valid = project(np.asarray(xyz).reshape(F, H * W, 3), K4, Ps, ts, max_t, direction)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        flow = uv - np.stack([xs, ys], -1).reshape(1, H * W, 2)
    flow[~valid] = UNKNOWN
    assert flow.dtype == np.float32
    return flow.reshape(F, H, W, 2)


def known(flow):
    """(...,) bool: both components within 1e7 (a NaN is not)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(flow[..., 0]) <= THRESH) & (np.abs(flow[..., 1]) <= THRESH)


def radius(u, v):
    with np.errstate(all="ignore"):
        r = np.sqrt(u * u + v * v)
    assert r.dtype == np.float32
    return r


def maxrad(flow):
    """(F,) fp32: the largest sqrt(u^2 + v^2) over each frame's known pixels, 0 where a frame has none."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32
    out = np.zeros(len(flow), np.float32)
    for i, fr in enumerate(flow):
        k = known(fr)
        if k.any():
            out[i] = radius(fr[..., 0][k], fr[..., 1][k]).max()
    return out


def color_wheel():
    """(55, 3) fp32: flowlib.make_color_wheel's entries / 255, rounded once."""
    ry, yg, gc, cb, bm, mr = SEGMENTS
    wheel = np.zeros((sum(SEGMENTS), 3))
    ramp = lambda n: np.floor(255 * np.arange(0, n) / n)
    col = 0
    wheel[0:ry, 0], wheel[0:ry, 1] = 255, ramp(ry)
    col += ry
    wheel[col:col + yg, 0], wheel[col:col + yg, 1] = 255 - ramp(yg), 255
    col += yg
    wheel[col:col + gc, 1], wheel[col:col + gc, 2] = 255, ramp(gc)
    col += gc
    wheel[col:col + cb, 1], wheel[col:col + cb, 2] = 255 - ramp(cb), 255
    col += cb
    wheel[col:col + bm, 2], wheel[col:col + bm, 0] = 255, ramp(bm)
    col += bm
    wheel[col:col + mr, 2], wheel[col:col + mr, 0] = 255 - ramp(mr), 255
    return (wheel / 255).astype(np.float32)


def flow_to_image(flow, given_maxrad=None):
    """(image (F, H, W, 3) uint8, maxrad (F,) fp32, near_one (F, H, W) bool) of (F, H, W, 2) fp32 flows.  near_one marks the pixels
    whose scaled radius is within 1e-5 of 1, where ``rad <= 1`` may fall either way in another arithmetic."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 4
    F = len(flow)
    mr = maxrad(flow) if given_maxrad is None else np.broadcast_to(np.asarray(given_maxrad, np.float32), (F,)).copy()
    wheel = color_wheel()
    n = len(wheel)
    img = np.zeros(flow.shape[:3] + (3,), np.uint8)
    near = np.zeros(flow.shape[:3], bool)
    for i in range(F):
        k = known(flow[i])
        u, v = np.where(k, flow[i, ..., 0], f32(0)), np.where(k, flow[i, ..., 1], f32(0))
        div = f32(np.float64(mr[i]) + 2.220446049250313e-16)
        with np.errstate(all="ignore"):
            u, v = u / div, v / div
            rad = radius(u, v)
            a = np.arctan2(-v, -u) / f32(np.pi)
            fk = (a + f32(1)) / f32(2) * f32(n - 1) + f32(1)
            k0 = np.clip(np.floor(np.nan_to_num(fk)).astype(np.int64), 1, n)
            k1 = np.where(k0 == n, 1, k0 + 1)
            fr = fk - k0.astype(np.float32)
            assert fk.dtype == fr.dtype == np.float32
            for c in range(3):
                col = (f32(1) - fr) * wheel[k0 - 1, c] + fr * wheel[k1 - 1, c]
                col = np.where(rad <= 1, f32(1) - rad * (f32(1) - col), col * f32(0.75))
                assert col.dtype == np.float32
                q = np.clip(np.nan_to_num(np.floor(f32(255) * col)), 0, 255)
                img[i, ..., c] = np.where(k, q, 0).astype(np.uint8)
            near[i] = k & (np.abs(rad - f32(1)) < 1e-5)
    return img, mr, near


def epe_terms(gt, pred):
    """(terms (F, H, W) fp32, counted (F, H, W) bool): sqrt(du^2 + dv^2) where both flows are known and gt is non-zero."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    assert gt.dtype == pred.dtype == np.float32
    counted = known(gt) & known(pred) & ((gt[..., 0] != 0) | (gt[..., 1] != 0))
    with np.errstate(all="ignore"):
        du, dv = gt[..., 0] - pred[..., 0], gt[..., 1] - pred[..., 1]
        e = np.sqrt(du * du + dv * dv)
    assert e.dtype == np.float32
    return e, counted


def epe_sums(gt, pred, mask=None):
    """(sums (F, 3) float64, counts (F, 3) int64) for [all, mask != 0, mask == 0]: fp32 terms, added in float64 (math.fsum).  Without
    a mask the last two stay 0."""
    e, counted = epe_terms(gt, pred)
    F = len(e)
    sums, counts = np.zeros((F, 3)), np.zeros((F, 3), np.int64)
    for i in range(F):
        sels = [counted[i]]
        if mask is not None:
            m = np.asarray(mask[i]) != 0
            sels += [counted[i] & m, counted[i] & ~m]
        for k, sel in enumerate(sels):
            sums[i, k] = math.fsum(e[i][sel].astype(np.float64).ravel())
            counts[i, k] = int(sel.sum())
    return sums, counts


def epe_from_sums(sums, counts):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(counts > 0, sums / counts, np.nan)
