"""numpy restatement of nsff_motion_maps and nsff_mask_erode (csrc/motion.hip) in the number format the kernels run in -- fp32
arrays through numpy's own fp32 operations, one rounding per operation, in the order include/nsff_render.h states -- and a
synthetic scene with analytic optical flow to try the method on.

tests/test_motion_host.py checks the erosion against scipy and by hand and asks whether the method finds a moving object at all;
the GPU tests compare the kernels with these functions bit for bit."""
import math

import numpy as np

f32 = np.float32
UNKNOWN = f32(1e10)
THRESH = f32(1e7)


def known(flow):
    """(...,) bool: both components within 1e7 (a NaN is not)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(flow[..., 0]) <= THRESH) & (np.abs(flow[..., 1]) <= THRESH)


def _direction(A, B, M, alpha, beta, threshold, epipolar):
    """One frame, one direction: A (H, W, 2) fp32 the frame's flow, B the neighbour's opposite flow (None: no neighbour), M (3, 3)
    fp32 -> (err (H, W) fp32, valid (H, W) bool, over (H, W) bool)."""
    H, W = A.shape[:2]
    err = np.full((H, W), UNKNOWN, f32)
    if B is None:
        return err, np.zeros((H, W), bool), np.zeros((H, W), bool)
    assert A.dtype == B.dtype == M.dtype == np.float32
    alpha, beta, threshold = f32(alpha), f32(beta), f32(threshold)
    ys, xs = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    u, v = A[..., 0], A[..., 1]
    kn = known(A)
    with np.errstate(all="ignore"):
        qx, qy = xs + u, ys + v
        inside = (qx >= 0) & (qx <= f32(W - 1)) & (qy >= 0) & (qy <= f32(H - 1))
        x0f, y0f = np.floor(qx), np.floor(qy)
        ax, ay = qx - x0f, qy - y0f
        x0 = np.clip(np.nan_to_num(x0f), 0, W - 1).astype(np.int64)        # (clipped only where the pixel is not inside, and unused there)
        y0 = np.clip(np.nan_to_num(y0f), 0, H - 1).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        b00, b01, b10, b11 = B[y0, x0], B[y0, x1], B[y1, x0], B[y1, x1]
        taps = known(b00) & known(b01) & known(b10) & known(b11)
        omx, omy = f32(1) - ax, f32(1) - ay
        b = []
        for c in range(2):
            top = b00[..., c] * omx + b01[..., c] * ax
            bot = b10[..., c] * omx + b11[..., c] * ax
            b.append((top * omy) + (bot * ay))
        bu, bv = b
        su, sv = u + bu, v + bv
        lhs = su * su + sv * sv
        rhs = alpha * ((u * u + v * v) + (bu * bu + bv * bv)) + beta
        valid = kn & inside & taps & (lhs <= rhs)
        over = np.zeros((H, W), bool)
        if epipolar:
            l0 = (M[0, 0] * xs + M[0, 1] * ys) + M[0, 2]
            l1 = (M[1, 0] * xs + M[1, 1] * ys) + M[1, 2]
            l2 = (M[2, 0] * xs + M[2, 1] * ys) + M[2, 2]
            r = (l0 * qx + l1 * qy) + l2
            n = l0 * l0 + l1 * l1
            e = np.abs(r) / np.sqrt(n)
            line_ok = np.isfinite(n) & (n > 0)
            assert e.dtype == lhs.dtype == rhs.dtype == np.float32
            err = np.where(kn & line_ok, e, UNKNOWN).astype(f32)
            valid = valid & line_ok
            over = valid & (e > threshold)
    return err, valid, over


def motion_maps(flows_fw, flows_bw, Fm=None, alpha=0.01, beta=0.5, threshold=1.0):
    """flows (F, H, W, 2) fp32, Fm (F, 2, 3, 3) fp32 or None (the consistency check alone) -> dict: err (F, 2, H, W) fp32, valid
    (F, 2, H, W) uint8, raw (F, H, W) uint8 (0 dynamic, 255 static), counts (F, 5) int64 [valid fw, valid bw, over fw, over bw,
    dynamic], err_sums (F, 2) float64 (fp32 terms over the valid pixels, added with math.fsum)."""
    flows_fw, flows_bw = np.asarray(flows_fw), np.asarray(flows_bw)
    assert flows_fw.dtype == flows_bw.dtype == np.float32 and flows_fw.shape == flows_bw.shape and flows_fw.ndim == 4
    F, H, W = flows_fw.shape[:3]
    epipolar = Fm is not None
    Fm = np.zeros((F, 2, 3, 3), f32) if Fm is None else np.asarray(Fm)
    assert Fm.dtype == np.float32 and Fm.shape == (F, 2, 3, 3)
    out = dict(err=np.zeros((F, 2, H, W), f32), valid=np.zeros((F, 2, H, W), np.uint8), raw=np.zeros((F, H, W), np.uint8),
               counts=np.zeros((F, 5), np.int64), err_sums=np.zeros((F, 2)))
    for f in range(F):
        moving = np.zeros((H, W), bool)
        for d, (n, A, Bs) in enumerate(((f + 1, flows_fw, flows_bw), (f - 1, flows_bw, flows_fw))):
            err, valid, over = _direction(A[f], Bs[n] if 0 <= n < F else None, Fm[f, d], alpha, beta, threshold, epipolar)
            out["err"][f, d], out["valid"][f, d] = err, valid
            out["counts"][f, d], out["counts"][f, 2 + d] = valid.sum(), over.sum()
            if epipolar:
                out["err_sums"][f, d] = math.fsum(err[valid].astype(np.float64))
            moving |= over
        out["raw"][f] = np.where(moving, 0, 255)
        out["counts"][f, 4] = moving.sum()
    return out


def erode(mask, k):
    """cv2.erode(mask, ones((k, k))) of (F, H, W) or (H, W) uint8 images: the minimum over the k x k window centred on each pixel,
    pixels outside the image not contributing (they are padded with 255)."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and k % 2 == 1 and k >= 1
    r = k // 2
    H, W = mask.shape[-2:]
    pad = [(0, 0)] * (mask.ndim - 2) + [(r, r), (r, r)]
    padded = np.pad(mask, pad, constant_values=255)
    out = np.full(mask.shape, 255, np.uint8)
    for dy in range(k):
        for dx in range(k):
            out = np.minimum(out, padded[..., dy:dy + H, dx:dx + W])
    return out


# ---- a synthetic scene: a static wavy surface, a camera moving sideways, a disc in front that moves up ----
def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def surface(x, y):
    """The background's distance along -z at (x, y): 4 +- 0.35."""
    return 4.0 + 0.2 * np.sin(1.7 * x + 0.3) + 0.15 * np.cos(1.3 * y - 0.2)


DISC_DEPTH, DISC_RADIUS, DISC_STEP = 2.5, 0.36, 0.11          # the plane z = -2.5; its centre moves +0.11 in y per frame


def disc_centre(t, F):
    return np.array([0.05, DISC_STEP * (t - (F - 1) / 2)])


def make_scene(F, H, W, noise=0.0, seed=0):
    """dict: K (3, 3), poses (F, 3, 4) camera-to-world (x right, y up, z backwards), flows_fw / flows_bw (F, H, W, 2) fp32 -- the
    true pixel motion of the surface point seen at each pixel towards the next / previous frame (zero at the sequence ends), plus
    Gaussian noise of `noise` pixels -- and disc (F, H, W) bool, the pixels that see the disc.  All geometry in float64."""
    rng = np.random.default_rng(seed)
    K = np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1.0]])
    poses = np.zeros((F, 3, 4))
    for t in range(F):
        poses[t, :, :3] = rotation(*rng.uniform(-0.01, 0.01, 3))
        poses[t, :, 3] = [0.12 * (t - (F - 1) / 2), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    # the ray of a pixel in camera axes (y up, z backwards), then in the world
    cam_dirs = np.stack([(xs - K[0, 2]) / K[0, 0], -(ys - K[1, 2]) / K[1, 1], -np.ones_like(xs)], -1)

    def project(X, t):                                          # world points (H, W, 3) -> pixels of frame t
        Xc = (X - poses[t, :, 3]) @ poses[t, :, :3]             # R^-1 (X - t) for a rotation
        return np.stack([K[0, 0] * Xc[..., 0] / -Xc[..., 2] + K[0, 2], K[1, 1] * -Xc[..., 1] / -Xc[..., 2] + K[1, 2]], -1)

    points, disc = [], []
    for t in range(F):
        C, dirs = poses[t, :, 3], cam_dirs @ poses[t, :, :3].T
        s = (-4.0 - C[2]) / dirs[..., 2]
        for _ in range(60):                                     # the wavy surface z = -surface(x, y): a contraction in s
            P = C + s[..., None] * dirs
            s = (-surface(P[..., 0], P[..., 1]) - C[2]) / dirs[..., 2]
        back = C + s[..., None] * dirs
        sd = (-DISC_DEPTH - C[2]) / dirs[..., 2]
        front = C + sd[..., None] * dirs
        hit = np.linalg.norm(front[..., :2] - disc_centre(t, F), axis=-1) <= DISC_RADIUS
        points.append(np.where(hit[..., None], front, back))
        disc.append(hit)
    flows = {+1: np.zeros((F, H, W, 2)), -1: np.zeros((F, H, W, 2))}
    pix = np.stack([xs, ys], -1)
    for step in (+1, -1):
        for t in range(F):
            n = t + step
            if not 0 <= n < F:
                continue
            shift = np.append(disc_centre(n, F) - disc_centre(t, F), 0.0)
            moved = points[t] + np.where(disc[t][..., None], shift, 0.0)
            flows[step][t] = project(moved, n) - pix
            if noise:
                flows[step][t] += rng.normal(0, noise, (H, W, 2))
    return dict(K=K, poses=poses, flows_fw=flows[+1].astype(f32), flows_bw=flows[-1].astype(f32), disc=np.stack(disc))
