"""The plane splat and the MPI composite of time interpolation (csrc/interp.hip), restated in numpy.

float64 from the fp32 inputs by default: what the kernels are compared with.  `dtype=np.float32` runs the SAME formulas with every
step rounded to fp32, sums taken sequentially -- the distance between the two is the rounding an honest fp32 implementation
cannot avoid, and the tests' tolerances are a multiple of it (tests/test_interp_kernels.py).

* projection: models/rendering.py:405-414 with datasets/ray_utils.py:127-151 (`ndc2world`, (N,3) branch) in its operation order;
  the splat target is px + (u - px) (the reference forms the optical flow u - px first, softsplat.py:17-18 adds the pixel back);
* splat: models/softsplat.py:19-43 -- floor, four bilinear weights, corners outside the frame dropped -- of [r, g, b, a, 1];
  the 'average' normalisation (softsplat.py:303-326: divide by the splatted ones, exact zeros replaced by one) is `normalise`;
* composite: models/rendering.py:439-458, front to back.

numpy only; nothing of the package under test is imported here.
"""
import numpy as np

TILE_X, TILE_Y, HALO = 32, 8, 4


def _ndc2world(x, y, z, K, eps=1e-6):
    T = x.dtype.type
    fx, fy, cx, cy = T(K[0, 0]), T(K[1, 1]), T(K[0, 2]), T(K[1, 2])
    rz = T(2) / (z - T(1) - T(eps))
    return -rz * x * cx / fx, -rz * y * cy / fy, rz


def projection_matrix(K, c2w, dtype=np.float64):
    """P = K @ w2c with the y and z rows of w2c flipped (rendering.py:390-394)"""
    pose = np.eye(4, dtype=dtype)
    pose[:3] = np.asarray(c2w, dtype)
    w2c = np.linalg.inv(pose)[:3].astype(dtype)
    w2c[1:] *= -1
    return (np.asarray(K, dtype) @ w2c).astype(dtype)


def landing_positions(xyz, flow, K, c2w, scale, W, H, dtype=np.float64):
    """(ox, oy), each (H*W, S): where sample (pixel, plane) lands after `scale` of its scene flow.  `scale` is taken as the fp32
    number the kernel is handed."""
    T = np.dtype(dtype).type
    xyz, flow = np.asarray(xyz, np.float32).astype(dtype), np.asarray(flow, np.float32).astype(dtype)
    n, S = xyz.shape[:2]
    assert n == H * W, (n, W, H)
    scale = T(np.float32(scale))
    P = projection_matrix(K, c2w, dtype)
    with np.errstate(all="ignore"):
        pw = _ndc2world(xyz[..., 0], xyz[..., 1], xyz[..., 2], K)
        q = xyz + flow
        qw = _ndc2world(q[..., 0], q[..., 1], q[..., 2], K)
        qw = [p + scale * (w - p) for p, w in zip(pw, qw)]
        uvd = [(P[r, 0] * qw[0] + P[r, 1] * qw[1] + P[r, 2] * qw[2]) + P[r, 3] for r in range(3)]
        u, v = uvd[0] / uvd[2], uvd[1] / uvd[2]
        px = np.tile(np.arange(W, dtype=dtype), H)[:, None]
        py = np.repeat(np.arange(H, dtype=dtype), W)[:, None]
        return px + (u - px), py + (v - py)


def _corners(ox, oy, W, H):
    """north-west cells (int64; a landing that is not finite or far outside gets a cell no corner of which is in the frame), and the
    four (cx, cy, weight, in frame) of softsplat.py:27-43"""
    T = ox.dtype.type
    with np.errstate(all="ignore"):
        fx, fy = np.floor(ox), np.floor(oy)
        ok = np.isfinite(fx) & np.isfinite(fy) & (fx >= -2) & (fx <= W) & (fy >= -2) & (fy <= H)
    nwx, nwy = np.where(ok, fx, -4).astype(np.int64), np.where(ok, fy, -4).astype(np.int64)
    oxs, oys = np.where(ok, ox, T(0)), np.where(ok, oy, T(0))
    sex, sey = (nwx + 1).astype(T), (nwy + 1).astype(T)
    wx, wy = nwx.astype(T), nwy.astype(T)
    out = []
    for cx, cy, wgt in ((nwx, nwy, (sex - oxs) * (sey - oys)), (nwx + 1, nwy, (oxs - wx) * (sey - oys)),
                        (nwx, nwy + 1, (sex - oxs) * (oys - wy)), (nwx + 1, nwy + 1, (oxs - wx) * (oys - wy))):
        out.append((cx, cy, wgt, ok & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)))
    return ok, nwx, nwy, out


def scatter_landings(ox, oy, rgb, alpha, W, H, keep=None):
    """(H*W, S, 5) sums of [r, g, b, a, 1] * bilinear weight at the landings (ox, oy) (H*W, S), in the dtype of ox; keep (H*W, S)
    bool: only these samples"""
    T = ox.dtype.type
    n, S = ox.shape
    src = np.concatenate([np.asarray(rgb, np.float32).reshape(n, S, 3), np.asarray(alpha, np.float32).reshape(n, S, 1),
                          np.ones((n, S, 1), np.float32)], -1).astype(T)
    plane = np.broadcast_to(np.arange(S), (n, S))
    out = np.zeros((H * W * S, 5), T)
    for cx, cy, wgt, m in _corners(ox, oy, W, H)[3]:
        m = m if keep is None else m & keep
        cell = (cy[m] * W + cx[m]) * S + plane[m]
        np.add.at(out, cell, src[m] * wgt[m][:, None])              # in sample order: sequential sums in dtype T
    return out.reshape(H * W, S, 5)


def splat_accum_ref(xyz, flow, rgb, alpha, K, c2w, scale, W, H, dtype=np.float64):
    """What nsff_splat_planes accumulates: (H*W, S, 5), channels r, g, b, a, norm"""
    ox, oy = landing_positions(xyz, flow, K, c2w, scale, W, H, dtype)
    return scatter_landings(ox, oy, rgb, alpha, W, H)


def normalise(accum):
    """the 'average' splat: channels / norm with exact zeros of the norm replaced by one -> (..., 4)"""
    norm = accum[..., 4:].copy()
    norm[norm == 0] = 1
    return accum[..., :4] / norm


def landing_stats(xyz, flow, K, c2w, scale, W, H, dtype=np.float64):
    """(near (H*W, S) bool, tiles (H*W, S) int, records): near = the landing cell is within HALO pixels of the sample's own pixel
    (-4 <= d < 4 in x and y); tiles = distinct 32 x 8 destination tiles that hold a corner inside the frame; records = sum of
    `tiles` over the samples that are not near = the (sample, destination tile) records the binned far path writes."""
    ox, oy = landing_positions(xyz, flow, K, c2w, scale, W, H, dtype)
    ok, nwx, nwy, corners = _corners(ox, oy, W, H)
    px = np.tile(np.arange(W), H)[:, None]
    py = np.repeat(np.arange(H), W)[:, None]
    dx, dy = nwx - px, nwy - py
    near = ok & (dx >= -HALO) & (dx < HALO) & (dy >= -HALO) & (dy < HALO)
    tiles_x = (W + TILE_X - 1) // TILE_X
    ids = np.stack([np.where(m, (cy // TILE_Y) * tiles_x + cx // TILE_X, -1) for cx, cy, _, m in corners], -1)
    ids = np.sort(ids, -1)
    distinct = (ids[..., :1] >= 0).astype(np.int64).sum(-1) + ((ids[..., 1:] != ids[..., :-1]) & (ids[..., 1:] >= 0)).sum(-1)
    return near, distinct, int(distinct[~near].sum())


def compose_planes(accum_fw, accum_bw, static_rgb, static_alpha, dt, dtype=np.float64):
    """per plane colour (n, S, 3) and alpha (n, S) of rendering.py:450-455; dt is taken as the fp32 number the kernel is handed"""
    T = np.dtype(dtype).type
    dt = T(np.float32(dt))
    fw = normalise(np.asarray(accum_fw)[..., :5].astype(dtype))
    bw = normalise(np.asarray(accum_bw)[..., :5].astype(dtype))
    s_rgb, s_a = np.asarray(static_rgb, np.float32).astype(dtype), np.asarray(static_alpha, np.float32).astype(dtype)[..., None]
    c_rgb = fw[..., :3] * fw[..., 3:] * (T(1) - dt) + bw[..., :3] * bw[..., 3:] * dt + s_rgb * s_a
    c_a = T(1) - (T(1) - (fw[..., 3:] * (T(1) - dt) + bw[..., 3:] * dt)) * (T(1) - s_a)
    return c_rgb, c_a[..., 0]


def mpi_composite_ref(accum_fw, accum_bw, static_rgb, static_alpha, zs, dt):
    """What nsff_mpi_composite computes, in float64: ((n, 3) rgb, (n) depth).  accum_*: (n, S, >=5), zs: (n, S)."""
    c_rgb, c_a = compose_planes(accum_fw, accum_bw, static_rgb, static_alpha, dt)
    trans = np.cumprod(1 - c_a, 1)
    trans = np.concatenate([np.ones_like(trans[:, :1]), trans[:, :-1]], 1)       # exclusive: what is in front of plane s
    return (trans[..., None] * c_rgb).sum(1), (trans * c_a * np.asarray(zs, np.float32).astype(np.float64)).sum(1)


def mpi_composite_fp32(accum_fw, accum_bw, static_rgb, static_alpha, zs, dt):
    """the reference's own loop (rendering.py:456-458) with every step rounded to fp32: ((n, 3) rgb, (n) depth)"""
    F = np.float32
    c_rgb, c_a = compose_planes(accum_fw, accum_bw, static_rgb, static_alpha, dt, F)
    zs = np.asarray(zs, F)
    n, S = c_a.shape
    rgb, depth, A = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
    for s in range(S):
        rgb += (F(1) - A)[:, None] * c_rgb[:, s]
        depth += (F(1) - A) * c_a[:, s] * zs[:, s]
        A += (F(1) - A) * c_a[:, s]
    return rgb, depth


def mpi_composite_chunked_fp32(accum_fw, accum_bw, static_rgb, static_alpha, zs, dt, chunk=64, drop_carry_at=None):
    """fp32 restatement of the kernel's scheme: `chunk` planes at a time, transmittance inside a chunk as an exclusive product,
    the product of the chunks in front carried along.  drop_carry_at=k resets the carry to 1 before chunk k (a deliberate bug,
    for the tests' self-check)."""
    F = np.float32
    c_rgb, c_a = compose_planes(accum_fw, accum_bw, static_rgb, static_alpha, dt, F)
    zs = np.asarray(zs, F)
    n, S = c_a.shape
    rgb, depth, carry = np.zeros((n, 3), F), np.zeros(n, F), np.ones(n, F)
    for k, s0 in enumerate(range(0, S, chunk)):
        if drop_carry_at == k:
            carry = np.ones(n, F)
        om = F(1) - c_a[:, s0:s0 + chunk]
        incl = np.cumprod(om, 1, dtype=F)
        excl = np.concatenate([np.ones((n, 1), F), incl[:, :-1]], 1)
        T = carry[:, None] * excl
        rgb += (T[..., None] * c_rgb[:, s0:s0 + chunk]).sum(1, dtype=F)
        depth += (T * c_a[:, s0:s0 + chunk] * zs[:, s0:s0 + chunk]).sum(1, dtype=F)
        carry = carry * incl[:, -1]
    return rgb, depth
