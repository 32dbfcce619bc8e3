"""numpy restatement of the disparity stages of csrc/depth.hip -- nsff_disparity_sparse, _push, _pull, _relax and the whole
nsff_disparity_dense -- operation for operation in the order include/nsff_render.h states, through numpy's own fp32 operations (one
rounding each), plus the same code in float64 (``dtype=np.float64``), and the synthetic scene the method is tried on.

tests/test_disparity_host.py asks the method's accuracy condition of this twin alone; the GPU tests compare the kernels with the
fp32 functions bit for bit."""
import numpy as np

import motion_numpy as mnp

f32 = np.float32
known_flow = mnp.known


def _grid(H, W, dtype):
    return np.meshgrid(np.arange(H, dtype=dtype), np.arange(W, dtype=dtype), indexing="ij")


def sparse(flows_fw, flows_bw, Pm, valid=None, masks=None, min_parallax=0.5, dtype=f32):
    """flows (F, H, W, 2) fp32, Pm (F, 2, 12) the parallax rows (nine entries of M_n M_f^-1, three of e), valid (F, 2, H, W) uint8
    or None, masks (F, H, W) uint8 or None (0 dynamic) -> n (F, H, W), c (F, H, W), counts (F,) int64."""
    flows = (np.asarray(flows_fw), np.asarray(flows_bw))
    assert flows[0].dtype == flows[1].dtype == np.float32 and flows[0].shape == flows[1].shape and flows[0].ndim == 4
    F, H, W = flows[0].shape[:3]
    Pm = np.asarray(Pm)
    assert Pm.shape == (F, 2, 12) and (dtype != f32 or Pm.dtype == np.float32)
    Pm = Pm.astype(dtype)
    mp = dtype(min_parallax)
    mp2 = mp * mp
    ys, xs = _grid(H, W, dtype)
    n_out, c_out = np.zeros((F, H, W), dtype), np.zeros((F, H, W), dtype)
    counts = np.zeros(F, np.int64)
    one = dtype(1)
    for f in range(F):
        num, den, par = (np.zeros((H, W), dtype) for _ in range(3))
        for d in range(2):
            P = Pm[f, d]
            A = flows[d][f]
            vote = np.full((H, W), bool(P.any())) & known_flow(A)
            if valid is not None:
                vote &= np.asarray(valid)[f, d] != 0
            if masks is not None:
                vote &= np.asarray(masks)[f] != 0
            with np.errstate(all="ignore"):
                u, v = A[..., 0].astype(dtype), A[..., 1].astype(dtype)
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
                vote &= (hz > 0) & (p2 >= mp2)
            zero = dtype(0)
            num = num + np.where(vote, ab, zero)
            den = den + np.where(vote, aa, zero)
            par = par + np.where(vote, p2, zero)
        with np.errstate(all="ignore"):
            kn = (den > 0) & (num > 0)
            c = np.where(kn, par, dtype(0))
            n = np.where(kn, par * (num / den), dtype(0))
        assert c.dtype == n.dtype == dtype
        n_out[f], c_out[f], counts[f] = n, c, kn.sum()
    return n_out, c_out, counts


def push(c, n, grey):
    """One pyramid step of (F, H, W) planes -> (F, ceil(H/2), ceil(W/2)): c and n summed over the clipped 2 x 2 block in row-major
    order, grey summed the same way and divided by the block's pixel count."""
    F, H, W = c.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    dtype = c.dtype.type
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    y1, x1 = 2 * yy + 1, 2 * xx + 1
    hx, hy = x1 < W, y1 < H
    x1c, y1c = np.minimum(x1, W - 1), np.minimum(y1, H - 1)
    out = []
    with np.errstate(all="ignore"):
        for a in (c, n, grey):
            s = a[:, 2 * yy, 2 * xx]
            s = np.where(hx, s + a[:, 2 * yy, x1c], s)
            s = np.where(hy, s + a[:, y1c, 2 * xx], s)
            s = np.where(hx & hy, s + a[:, y1c, x1c], s)
            out.append(s.astype(dtype))
        count = ((1 + hx) * (1 + hy)).astype(dtype)
        out[2] = out[2] / count
    return out[0], out[1], out[2]


def pull(c, n, parent, hw=None):
    """d = n / c where c > 0, else the parent's value at (y >> 1, x >> 1); parent None: 0 (the top).  c None: the nearest-neighbour
    upsampling of the parent alone to hw = (H, W)."""
    if c is None:
        H, W = hw
    else:
        H, W = c.shape[1:]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if c is None:
        return parent[:, yy >> 1, xx >> 1].copy()
    dtype = c.dtype.type
    below = np.zeros_like(c) if parent is None else parent[:, yy >> 1, xx >> 1]
    with np.errstate(all="ignore"):
        return np.where(c > 0, n / c, below).astype(dtype)


def _shift(a, dy, dx):
    """a at (y + dy, x + dx), read from the clamped address, and whether that pixel is inside the image."""
    H, W = a.shape[1:]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inside = (yy + dy >= 0) & (yy + dy < H) & (xx + dx >= 0) & (xx + dx < W)
    return a[:, np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)], inside


def relax(d, n, c, grey, lam=8.0, sigma=0.05, iters=1):
    """`iters` weighted-Jacobi iterations: d' = (n + lam S) / (c + lam Wt), S = sum g d_q, Wt = sum g over the neighbours left,
    right, up, down inside the image, g = 1 / (1 + ((grey_p - grey_q) / sigma)^2); d' = d where the denominator is not > 0."""
    dtype = d.dtype.type
    lam, sigma, one, zero = dtype(lam), dtype(sigma), dtype(1), dtype(0)
    gs = []
    with np.errstate(all="ignore"):
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            q, inside = _shift(grey, dy, dx)
            t = (grey - q) / sigma
            gs.append((np.where(inside, one / (one + t * t), zero).astype(dtype), inside, dy, dx))
        for _ in range(iters):
            S, Wt = np.zeros_like(d), np.zeros_like(d)
            for g, inside, dy, dx in gs:
                dq, _ = _shift(d, dy, dx)
                S = S + np.where(inside, g * dq, zero)
                Wt = Wt + g
            num = n + lam * S
            den = c + lam * Wt
            d = np.where(den > 0, num / den, d).astype(dtype)
    return d


def pyramid_sizes(H, W):
    sizes = [(H, W)]
    while sizes[-1] != (1, 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def dense(n, c, grey, levels=3, iters=30, lam=8.0, sigma=0.05):
    """The whole densification: push to 1 x 1, pull down to level `levels` (the top itself where levels equals the pyramid's
    height), then at each of the finest `levels` levels the nearest-neighbour upsampling of the level above (at the top: its own
    pulled value) as the start of `iters` relax iterations."""
    assert n.dtype == c.dtype == grey.dtype and n.shape == c.shape == grey.shape
    sizes = pyramid_sizes(*n.shape[1:])
    L = len(sizes)
    assert 1 <= levels <= L
    pyr = [(c, n, grey)]
    for _ in range(L - 1):
        pyr.append(push(*pyr[-1]))
    start = min(levels, L - 1)                                   # the coarsest level that is pulled down to
    d = None
    for l in range(L - 1, start - 1, -1):
        d = pull(pyr[l][0], pyr[l][1], d)
    for l in range(levels - 1, -1, -1):
        if l < L - 1:
            d = pull(None, None, d, sizes[l])
        d = relax(d, pyr[l][1], pyr[l][0], pyr[l][2], lam, sigma, iters)
    return d


# ---- the host side: the parallax rows, in float64 ----
def parallax_rows(K, poses):
    """(F, 2, 12) float64, the definition restated: the nine entries of M_n M_f^-1 and the three of e = M_n (C_f - C_n)."""
    K, poses = np.asarray(K, np.float64), np.asarray(poses, np.float64)
    F = len(poses)
    M = K @ np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(poses[:, :, :3])
    C = poses[:, :, 3]
    out = np.zeros((F, 2, 12))
    for f in range(F):
        for d, nb in enumerate((f + 1, f - 1)):
            if 0 <= nb < F and np.linalg.norm(C[f] - C[nb]) > 1e-12 * max(1.0, np.linalg.norm(C[f]), np.linalg.norm(C[nb])):
                out[f, d, :9] = (M[nb] @ np.linalg.inv(M[f])).ravel()
                out[f, d, 9:] = M[nb] @ (C[f] - C[nb])
    return out


# ---- the synthetic scene: motion_numpy's, plus its true depth and a guide image ----
def make_scene(F, H, W, noise=0.0, seed=0):
    """motion_numpy.make_scene plus ``depth`` (F, H, W) float64 -- the distance along the camera's viewing axis of the surface point
    each pixel sees (the disc where it is hit), by the same fixed-point intersection -- and ``guide`` (F, H, W) fp32 on a 0..1 scale:
    the background 0.45 + 0.1 sin(0.3 x + 0.2 y) in pixel coordinates, the disc 0.9."""
    s = mnp.make_scene(F, H, W, noise=noise, seed=seed)
    K, poses = s["K"], s["poses"]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cam_dirs = np.stack([(xs - K[0, 2]) / K[0, 0], -(ys - K[1, 2]) / K[1, 1], -np.ones_like(xs)], -1)
    depth = np.zeros((F, H, W))
    for t in range(F):
        C, dirs = poses[t, :, 3], cam_dirs @ poses[t, :, :3].T
        sb = (-4.0 - C[2]) / dirs[..., 2]
        for _ in range(60):
            P = C + sb[..., None] * dirs
            sb = (-mnp.surface(P[..., 0], P[..., 1]) - C[2]) / dirs[..., 2]
        sd = (-mnp.DISC_DEPTH - C[2]) / dirs[..., 2]
        front = C + sd[..., None] * dirs
        hit = np.linalg.norm(front[..., :2] - mnp.disc_centre(t, F), axis=-1) <= mnp.DISC_RADIUS
        assert np.array_equal(hit, s["disc"][t])
        depth[t] = np.where(hit, sd, sb)                         # cam_dirs has z = -1: the ray parameter is the depth along the axis
    guide = np.where(s["disc"], 0.9, 0.45 + 0.1 * np.sin(0.3 * xs + 0.2 * ys)).astype(f32)
    return dict(s, depth=depth, guide=guide)


def scene_disparity(scene, erode=15, min_parallax=0.5, levels=3, iters=30, lam=8.0, sigma=0.05, dtype=f32):
    """The method on a scene, as depth.disparity_maps chains it: masks = the motion twin's raw eroded, valid = its check."""
    Fm = mnp_fundamental(scene["K"], scene["poses"])
    maps = mnp.motion_maps(scene["flows_fw"], scene["flows_bw"], Fm)
    masks = mnp.erode(maps["raw"], erode)
    rows = parallax_rows(scene["K"], scene["poses"])
    Pm = rows.astype(f32) if dtype == f32 else rows
    n, c, counts = sparse(scene["flows_fw"], scene["flows_bw"], Pm, valid=maps["valid"], masks=masks, min_parallax=min_parallax, dtype=dtype)
    d = dense(n, c, scene["guide"].astype(dtype), levels=levels, iters=iters, lam=lam, sigma=sigma)
    return dict(disps=d, n=n, c=c, counts=counts, masks=masks, valid=maps["valid"])


def mnp_fundamental(K, poses):
    from nsff_pl_amd import motion
    return motion.fundamental_matrices(K, poses).numpy()


def static_error(d, scene):
    """(ratio, method, constant): the mean of |d - 1/depth| / (1/depth) over the non-disc pixels, for d and for the best constant
    (the median true disparity of those pixels)."""
    truth = 1.0 / scene["depth"]
    sel = ~scene["disc"]
    t = truth[sel]
    method = float(np.mean(np.abs(np.asarray(d, np.float64)[sel] - t) / t))
    const = float(np.mean(np.abs(np.median(t) - t) / t))
    return method / const, method, const
