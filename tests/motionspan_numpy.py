"""numpy restatement of nsff_motion_span and nsff_mask_propagate (csrc/motionspan.hip): the epipolar test against every neighbour
f +- 1 .. f +- span a pixel reaches by chaining optical flow, and "dynamic" carried along the same chain -- operation for operation
in the order include/nsff_render.h states, through numpy's own fp32 operations (one rounding each), plus the same code in float64
(``dtype=np.float64``), the matrices of every neighbour f +- k in float64, and motion_numpy's synthetic scene with the disc's
centre given per frame.

tests/test_motionspan_host.py asks the method's conditions of this twin alone; the GPU tests compare the kernels with the fp32
functions bit for bit.  ``known``, the hop and the scene's pieces are motion_numpy's and parallax_numpy's."""
import numpy as np

import motion_numpy as mnp
import parallax_numpy as pnp

f32 = np.float32
MAX_SPAN = MAX_REACH = 8                                         # NSFF_MOTION_MAX_SPAN, NSFF_PROPAGATE_MAX_REACH
UNKNOWN = mnp.UNKNOWN


def fm_rows(K, poses, span):
    """(F, 2, span, 3, 3) float64, the definition restated from the parallax rows: with G = M_n M_f^-1 and e = M_n (C_f - C_n) of the
    neighbour n = f + k (d = 0) / f - k (d = 1), a pixel x of f is seen in n on the line through e and G x, e x (G x) = [e]_x G x;
    scaled to unit Frobenius norm; zeros beyond the sequence ends and for coincident centres."""
    rows = pnp.rows(K, poses, span)
    out = np.zeros(rows.shape[:3] + (3, 3))
    for idx in np.ndindex(*rows.shape[:3]):
        G, e = rows[idx][:9].reshape(3, 3), rows[idx][9:]
        Fm = np.cross(e, G.T).T                                  # column i is e x (column i of G)
        norm = np.linalg.norm(Fm)
        if norm > 0:
            out[idx] = Fm / norm
    return out


def hop_scale(span):
    """(span,) fp32: 1 / sqrt(k), computed in float64 and rounded once."""
    return np.array([1.0 / np.sqrt(float(k)) for k in range(1, span + 1)]).astype(f32)


def _grid(H, W, dtype):
    return np.meshgrid(np.arange(H, dtype=dtype), np.arange(W, dtype=dtype), indexing="ij")


def _inputs(flows_fw, flows_bw, valid):
    flows = (np.asarray(flows_fw), np.asarray(flows_bw))
    assert flows[0].dtype == flows[1].dtype == np.float32 and flows[0].shape == flows[1].shape and flows[0].ndim == 4
    valid = None if valid is None else np.asarray(valid)
    assert valid is None or (valid.dtype == np.uint8 and valid.shape == (flows[0].shape[0], 2) + flows[0].shape[1:3])
    return flows, valid


def _start(flows, valid, f, d, dtype):
    A = flows[d][f]
    alive = mnp.known(A)
    if valid is not None:
        alive = alive & (valid[f, d] != 0)
    return alive, A[..., 0].astype(dtype), A[..., 1].astype(dtype)


def motion_span(flows_fw, flows_bw, Fm, scale, span, valid=None, threshold=1.0, dtype=f32):
    """flows (F, H, W, 2) fp32, Fm (F, 2, span, 3, 3), scale (span), valid (F, 2, H, W) uint8 or None -> dict: err (F, 2, H, W),
    hops (F, 2, H, W) uint8, raw (F, H, W) uint8 (0 dynamic, 255 static), counts (F, 3) int64 [over fw, over bw, dynamic]."""
    flows, valid = _inputs(flows_fw, flows_bw, valid)
    assert 1 <= span <= MAX_SPAN
    F, H, W = flows[0].shape[:3]
    Fm, scale = np.asarray(Fm), np.asarray(scale)
    assert Fm.shape == (F, 2, span, 3, 3) and scale.shape == (span,) and (dtype != f32 or Fm.dtype == scale.dtype == np.float32)
    Fm, scale, threshold = Fm.astype(dtype), scale.astype(dtype), dtype(threshold)
    ys, xs = _grid(H, W, dtype)
    out = dict(err=np.zeros((F, 2, H, W), dtype), hops=np.zeros((F, 2, H, W), np.uint8), raw=np.zeros((F, H, W), np.uint8),
               counts=np.zeros((F, 3), np.int64))
    for f in range(F):
        moving = np.zeros((H, W), bool)
        for d, s in enumerate((+1, -1)):
            alive, u, v = _start(flows, valid, f, d, dtype)
            best, hops = np.zeros((H, W), dtype), np.zeros((H, W), np.uint8)
            for k in range(1, span + 1):
                nb = f + s * k
                if not 0 <= nb < F:
                    break
                M = Fm[f, d, k - 1]
                with np.errstate(all="ignore"):
                    qx, qy = xs + u, ys + v
                    l0 = (M[0, 0] * xs + M[0, 1] * ys) + M[0, 2]
                    l1 = (M[1, 0] * xs + M[1, 1] * ys) + M[1, 2]
                    l2 = (M[2, 0] * xs + M[2, 1] * ys) + M[2, 2]
                    r = (l0 * qx + l1 * qy) + l2
                    n = l0 * l0 + l1 * l1
                    e = np.abs(r) / np.sqrt(n)
                    take = alive & np.isfinite(n) & (n > 0)
                    scaled = e * scale[k - 1]
                    assert scaled.dtype == dtype
                    best = np.where(take, np.fmax(best, scaled), best)      # fmaxf: a NaN e leaves best as it is
                    hops = hops + take.astype(np.uint8)
                    if k < span and 0 <= nb + s < F:
                        bu, bv, ok = pnp._hop(flows[d][nb], qx, qy, None if valid is None else valid[nb, d], None, dtype)
                        alive = alive & ok
                        u, v = u + bu, v + bv
            over = (hops > 0) & (best > threshold)
            out["err"][f, d] = np.where(hops > 0, best, dtype(UNKNOWN))
            out["hops"][f, d] = hops
            out["counts"][f, d] = over.sum()
            moving |= over
        out["raw"][f] = np.where(moving, 0, 255)
        out["counts"][f, 2] = moving.sum()
    return out


def propagate(src, flows_fw, flows_bw, reach, valid=None, dtype=f32):
    """src (F, H, W) uint8 (0 dynamic), flows (F, H, W, 2) fp32, valid (F, 2, H, W) uint8 or None -> dst (F, H, W) uint8, hits
    (F, H, W) uint8, zero_counts (F,) int64."""
    flows, valid = _inputs(flows_fw, flows_bw, valid)
    src = np.asarray(src)
    assert 1 <= reach <= MAX_REACH and src.dtype == np.uint8 and src.shape == flows[0].shape[:3]
    F, H, W = src.shape
    ys, xs = _grid(H, W, dtype)
    dst, hits_out = np.zeros_like(src), np.zeros_like(src)
    for f in range(F):
        hits = np.zeros((H, W), np.uint8)
        for d, s in enumerate((+1, -1)):
            alive, u, v = _start(flows, valid, f, d, dtype)
            for k in range(1, reach + 1):
                nb = f + s * k
                if not 0 <= nb < F:
                    break
                with np.errstate(all="ignore"):
                    qx, qy = xs + u, ys + v
                    inside = (qx >= 0) & (qx <= dtype(W - 1)) & (qy >= 0) & (qy <= dtype(H - 1))
                    xi = np.clip(np.nan_to_num(np.rint(qx)), 0, W - 1).astype(np.int64)      # (clipped only where not inside, and unused there)
                    yi = np.clip(np.nan_to_num(np.rint(qy)), 0, H - 1).astype(np.int64)
                    hits = hits + (alive & inside & (src[nb][yi, xi] == 0)).astype(np.uint8)
                    if k < reach and 0 <= nb + s < F:
                        bu, bv, ok = pnp._hop(flows[d][nb], qx, qy, None if valid is None else valid[nb, d], None, dtype)
                        alive = alive & ok
                        u, v = u + bu, v + bv
        dst[f] = np.where((src[f] == 0) | (hits > 0), 0, src[f])
        hits_out[f] = hits
    return dst, hits_out, (dst == 0).reshape(F, -1).sum(1).astype(np.int64)


def make_scene_steps(F, H, W, centres, noise=0.0, seed=0):
    """motion_numpy.make_scene with the disc's centre per frame as an argument: centres (F, 2), the disc's (x, y) in the plane
    z = -DISC_DEPTH at each frame.  The same dict: K, poses, flows_fw / flows_bw (F, H, W, 2) fp32, disc (F, H, W) bool; the random
    numbers are drawn in make_scene's order."""
    centres = np.asarray(centres, np.float64)
    assert centres.shape == (F, 2)
    rng = np.random.default_rng(seed)
    K = np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1.0]])
    poses = np.zeros((F, 3, 4))
    for t in range(F):
        poses[t, :, :3] = mnp.rotation(*rng.uniform(-0.01, 0.01, 3))
        poses[t, :, 3] = [0.12 * (t - (F - 1) / 2), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cam_dirs = np.stack([(xs - K[0, 2]) / K[0, 0], -(ys - K[1, 2]) / K[1, 1], -np.ones_like(xs)], -1)

    def project(X, t):                                          # world points (H, W, 3) -> pixels of frame t
        Xc = (X - poses[t, :, 3]) @ poses[t, :, :3]
        return np.stack([K[0, 0] * Xc[..., 0] / -Xc[..., 2] + K[0, 2], K[1, 1] * -Xc[..., 1] / -Xc[..., 2] + K[1, 2]], -1)

    points, disc = [], []
    for t in range(F):
        C, dirs = poses[t, :, 3], cam_dirs @ poses[t, :, :3].T
        s = (-4.0 - C[2]) / dirs[..., 2]
        for _ in range(60):                                     # the wavy surface z = -surface(x, y): a contraction in s
            P = C + s[..., None] * dirs
            s = (-mnp.surface(P[..., 0], P[..., 1]) - C[2]) / dirs[..., 2]
        back = C + s[..., None] * dirs
        sd = (-mnp.DISC_DEPTH - C[2]) / dirs[..., 2]
        front = C + sd[..., None] * dirs
        hit = np.linalg.norm(front[..., :2] - centres[t], axis=-1) <= mnp.DISC_RADIUS
        points.append(np.where(hit[..., None], front, back))
        disc.append(hit)
    flows = {+1: np.zeros((F, H, W, 2)), -1: np.zeros((F, H, W, 2))}
    pix = np.stack([xs, ys], -1)
    for step in (+1, -1):
        for t in range(F):
            n = t + step
            if not 0 <= n < F:
                continue
            shift = np.append(centres[n] - centres[t], 0.0)
            moved = points[t] + np.where(disc[t][..., None], shift, 0.0)
            flows[step][t] = project(moved, n) - pix
            if noise:
                flows[step][t] += rng.normal(0, noise, (H, W, 2))
    return dict(K=K, poses=poses, flows_fw=flows[+1].astype(f32), flows_bw=flows[-1].astype(f32), disc=np.stack(disc))


# the two scenes of DESIGN.md section 11.3, nine frames each
SLOW_STEP = 0.011                                                # 0.011 a frame at depth 2.5 is about 0.62 px at 72 x 128
PAUSE_INDEX = (0, 1, 2, 3, 3, 3, 4, 5, 6)                        # the disc stands still in frames 3, 4, 5


def slow_centres(F=9):
    return np.array([[0.05, SLOW_STEP * (t - (F - 1) / 2)] for t in range(F)])


def pause_centres():
    """The disc's usual step of 0.11 a frame with a pause of three frames: y = 0.11 times the index (from the image's middle upwards;
    in the last frames part of the disc has left the image)."""
    return np.array([[0.05, mnp.DISC_STEP * i] for i in PAUSE_INDEX])


def recall_and_background(raw, disc):
    """Per frame: the share of the disc's pixels that raw calls dynamic (0), and the share of the other pixels it calls dynamic."""
    F = len(raw)
    hit = raw == 0
    return (np.array([hit[f][disc[f]].mean() for f in range(F)]), np.array([hit[f][~disc[f]].mean() for f in range(F)]))
