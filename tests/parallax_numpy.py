"""numpy restatement of nsff_disparity_span (csrc/parallax.hip): the triangulation of a static pixel over several frames by chaining
optical flow, operation for operation in the order include/nsff_render.h states, through numpy's own fp32 operations (one rounding
each), plus the same code in float64 (``dtype=np.float64``) and the parallax rows of every neighbour f +- k in float64.

tests/test_parallax_host.py asks the method's coverage and accuracy conditions of this twin alone; the GPU tests compare the kernel
with the fp32 function bit for bit.  The grid, ``known`` and the synthetic scene are disparity_numpy's and motion_numpy's."""
import numpy as np

import disparity_numpy as dnp
import motion_numpy as mnp

f32 = np.float32
MAX_SPAN = 8                                                     # NSFF_DISPARITY_MAX_SPAN


def rows(K, poses, span):
    """(F, 2, span, 12) float64, the definition restated: row k - 1 of frame f and direction d (0: n = f + k, 1: n = f - k) holds the
    nine entries of M_n M_f^-1 and the three of e = M_n (C_f - C_n); zeros beyond the sequence ends and for coincident centres."""
    K, poses = np.asarray(K, np.float64), np.asarray(poses, np.float64)
    F = len(poses)
    M = K @ np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(poses[:, :, :3])
    C = poses[:, :, 3]
    out = np.zeros((F, 2, span, 12))
    for f in range(F):
        for d, s in enumerate((+1, -1)):
            for k in range(1, span + 1):
                nb = f + s * k
                if 0 <= nb < F and np.linalg.norm(C[f] - C[nb]) > 1e-12 * max(1.0, np.linalg.norm(C[f]), np.linalg.norm(C[nb])):
                    out[f, d, k - 1, :9] = (M[nb] @ np.linalg.inv(M[f])).ravel()
                    out[f, d, k - 1, 9:] = M[nb] @ (C[f] - C[nb])
    return out


def _hop(B, qx, qy, valid_n, masks_n, dtype):
    """B (H, W, 2) fp32 sampled bilinearly at q by the rule of nsff_motion_maps -> (b_u, b_v, hop_ok).  The taps are read from q
    clamped into the image: the identity where q is inside, where alone the hop is ok."""
    H, W = B.shape[:2]
    inside = (qx >= 0) & (qx <= dtype(W - 1)) & (qy >= 0) & (qy <= dtype(H - 1))
    x0f, y0f = np.floor(qx), np.floor(qy)
    ax, ay = qx - x0f, qy - y0f
    x0 = np.clip(np.nan_to_num(x0f), 0, W - 1).astype(np.int64)
    y0 = np.clip(np.nan_to_num(y0f), 0, H - 1).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    taps = ((y0, x0), (y0, x1), (y1, x0), (y1, x1))
    b00, b01, b10, b11 = (B[t] for t in taps)
    ok = inside & mnp.known(b00) & mnp.known(b01) & mnp.known(b10) & mnp.known(b11)
    for plane in (valid_n, masks_n):
        if plane is not None:
            for t in taps:
                ok &= plane[t] != 0
    omx, omy = dtype(1) - ax, dtype(1) - ay
    b = []
    for c in range(2):
        top = b00[..., c].astype(dtype) * omx + b01[..., c].astype(dtype) * ax
        bot = b10[..., c].astype(dtype) * omx + b11[..., c].astype(dtype) * ax
        b.append((top * omy) + (bot * ay))
    return b[0], b[1], ok


def sparse_span(flows_fw, flows_bw, Pm, span, valid=None, masks=None, min_parallax=0.5, dtype=f32):
    """flows (F, H, W, 2) fp32, Pm (F, 2, span, 12) the parallax rows of the neighbours f +- 1 .. f +- span, valid (F, 2, H, W) uint8
    or None, masks (F, H, W) uint8 or None (0 dynamic) -> n (F, H, W), c (F, H, W), votes (F, H, W) uint8, counts (F,) int64."""
    flows = (np.asarray(flows_fw), np.asarray(flows_bw))
    assert flows[0].dtype == flows[1].dtype == np.float32 and flows[0].shape == flows[1].shape and flows[0].ndim == 4
    assert 1 <= span <= MAX_SPAN
    F, H, W = flows[0].shape[:3]
    Pm = np.asarray(Pm)
    assert Pm.shape == (F, 2, span, 12) and (dtype != f32 or Pm.dtype == np.float32)
    Pm = Pm.astype(dtype)
    valid = None if valid is None else np.asarray(valid)
    masks = None if masks is None else np.asarray(masks)
    mp = dtype(min_parallax)
    mp2 = mp * mp
    ys, xs = dnp._grid(H, W, dtype)
    n_out, c_out = np.zeros((F, H, W), dtype), np.zeros((F, H, W), dtype)
    v_out = np.zeros((F, H, W), np.uint8)
    counts = np.zeros(F, np.int64)
    one, zero = dtype(1), dtype(0)
    for f in range(F):
        num, den, par = (np.zeros((H, W), dtype) for _ in range(3))
        votes = np.zeros((H, W), np.uint8)
        for d, s in enumerate((+1, -1)):
            A = flows[d][f]
            alive = mnp.known(A)
            if valid is not None:
                alive &= valid[f, d] != 0
            if masks is not None:
                alive &= masks[f] != 0
            u, v = A[..., 0].astype(dtype), A[..., 1].astype(dtype)
            for k in range(1, span + 1):
                nb = f + s * k
                if not 0 <= nb < F:
                    break
                P = Pm[f, d, k - 1]
                with np.errstate(all="ignore"):
                    hx = (P[0] * xs + P[1] * ys) + P[2]
                    hy = (P[3] * xs + P[4] * ys) + P[5]
                    hz = (P[6] * xs + P[7] * ys) + P[8]
                    up, vp = xs + u, ys + v
                    r = one / hz
                    ax, ay = (P[9] - up * P[11]) * r, (P[10] - vp * P[11]) * r
                    bx, by = up - hx * r, vp - hy * r
                    p2 = bx * bx + by * by
                    ab = ax * bx + ay * by
                    aa = ax * ax + ay * ay
                    vote = alive & bool(P.any()) & (hz > 0) & (p2 >= mp2)
                    num = num + np.where(vote, ab, zero)
                    den = den + np.where(vote, aa, zero)
                    par = par + np.where(vote, p2, zero)
                    votes = votes + vote.astype(np.uint8)
                    if k < span and 0 <= nb + s < F:
                        bu, bv, ok = _hop(flows[d][nb], up, vp, None if valid is None else valid[nb, d],
                                          None if masks is None else masks[nb], dtype)
                        alive = alive & ok
                        u, v = u + bu, v + bv
        with np.errstate(all="ignore"):
            kn = (den > 0) & (num > 0)
            c = np.where(kn, par, zero)
            n = np.where(kn, par * (num / den), zero)
        assert c.dtype == n.dtype == dtype
        n_out[f], c_out[f], v_out[f], counts[f] = n, c, votes, kn.sum()
    return n_out, c_out, v_out, counts


def scene_inputs(scene, erode=15):
    """What depth.disparity_maps is given on a scene: masks = the motion twin's raw map eroded, valid = its forward-backward check."""
    maps = mnp.motion_maps(scene["flows_fw"], scene["flows_bw"], dnp.mnp_fundamental(scene["K"], scene["poses"]))
    return dict(masks=mnp.erode(maps["raw"], erode), valid=maps["valid"])


def static_stats(n, c, scene):
    """(known fraction, mean relative error, known): over the static (non-disc) pixels of every frame, the share with a measured
    disparity and the mean of |n / c - 1/depth| / (1/depth) over those."""
    static = ~scene["disc"]
    kn = (c > 0) & static
    truth = 1.0 / scene["depth"]
    with np.errstate(all="ignore"):
        d = n.astype(np.float64) / c.astype(np.float64)
    err = float(np.mean(np.abs(d[kn] - truth[kn]) / truth[kn])) if kn.any() else float("nan")
    return float(kn.sum() / static.sum()), err, kn
