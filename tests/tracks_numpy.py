"""numpy twin of the track layer (nsff_pl_amd/tracks.py, csrc/tracks.hip): the chain rule, the step's projection, the line rule and the
trail image, in fp32 -- numpy's own fp32 operations, one rounding each, in the order the header states, so that the kernels can be
compared bit for bit -- or in float64, the form tests/test_tracks_host.py checks against golden g30 (the reference's own forward,
chained in float64 by tests/golden/make_golden_tracks.py).

A `field` here is any callable ``(xyz (R, S, 3), t (R,) ints, direction) -> flow (R, S, 3)`` in the dtype of xyz: :func:`oracle_field` wraps
the oracle's numpy ``nerf_forward`` (dynamic trunk only, one flow head: the query of the reference's render_transient_warping)."""
import contextlib

import numpy as np

import flow_numpy as fnp

f32 = np.float32
UNKNOWN = fnp.UNKNOWN
Z_FAR = 0.95
MAX_COORD = 32768.0


def zero_rule(xyz):
    """(...,) bool: the flow of this point is zeroed -- (z + 1) * 0.5 > 0.95 in the dtype of xyz, one rounding per operation."""
    dt = xyz.dtype.type
    return (xyz[..., 2] + dt(1)) * dt(0.5) > dt(Z_FAR)


def step(xyz, t, alive, flow, direction, max_t):
    """One step: (xyz', t', alive', applied flow) of xyz (R, S, 3), t (R,) int32, alive (R,) bool and the head's flow (R, S, 3)."""
    can = alive & ((t < max_t) if direction > 0 else (t > 0))
    f = np.where(zero_rule(xyz)[..., None], xyz.dtype.type(0), flow)
    nxt = np.where(can[:, None, None], xyz + f, xyz)
    assert nxt.dtype == xyz.dtype
    return nxt, np.where(can, t + (1 if direction > 0 else -1), t).astype(np.int32), can, np.where(can[:, None, None], f, xyz.dtype.type(0))


def advect(field, xyz, ts, steps, max_t):
    """The chain of tracks.advect in the dtype of xyz: {'xyz' (n+1, R, S, 3), 't' (n+1, R) int32, 'alive' (n+1, R) bool, 'flow' (n, R, S, 3)}
    -- 'flow' is what moved the points: the head's output after the zero rule, 0 for a row that could not step."""
    n, direction = abs(steps), (1 if steps > 0 else -1)
    path, t, alive, flows = [np.asarray(xyz)], [np.asarray(ts, np.int32)], [np.ones(len(ts), bool)], []
    for _ in range(n):
        flow = np.asarray(field(path[-1], t[-1], direction), path[-1].dtype)
        x, tt, a, moved = step(path[-1], t[-1], alive[-1], flow, direction, max_t)
        flows.append(moved)
        path.append(x), t.append(tt), alive.append(a)
    return dict(xyz=np.stack(path), t=np.stack(t), alive=np.stack(alive), flow=np.stack(flows))


def project(xyz, t, K4, Ps, fixed_view=False):
    """(uv (R, S, 2), depth (R, S)) of xyz (R, S, 3) seen by Ps[t[r]] -- Ps (n, 3, 4) -- or by the one view Ps (3, 4): fp32 in, the
    kernel's chain bit for bit (flow_numpy.ndc2world, then ((p0 X + p1 Y) + p2 Z) + p3); float64 in, the same formulas in float64."""
    Ps = np.asarray(Ps).reshape(-1, 3, 4)
    P = Ps[np.zeros(len(t), int) if fixed_view else np.clip(t, 0, len(Ps) - 1)][:, None]      # (R, 1, 3, 4)
    if xyz.dtype == np.float32:
        assert Ps.dtype == np.float32
        world, eps = fnp.ndc2world(xyz, K4), f32(1e-8)
    else:
        fx, fy, cx, cy = (float(v) for v in K4)
        P = P.astype(np.float64)
        Rz = 2 / ((xyz[..., 2] - 1) - 1e-6)
        world, eps = np.stack([(((-Rz) * xyz[..., 0]) * cx) / fx, (((-Rz) * xyz[..., 1]) * cy) / fy, Rz], -1), 1e-8
    X, Y, Z = world[..., 0:1], world[..., 1:2], world[..., 2:3]
    with np.errstate(all="ignore"):
        uvd = ((P[..., 0] * X + P[..., 1] * Y) + P[..., 2] * Z) + P[..., 3]
        uv = uvd[..., :2] / (np.abs(uvd[..., 2:]) + eps)
        uv = np.where((uvd[..., 2] > 0)[..., None], uv, xyz.dtype.type(UNKNOWN))
    assert uv.dtype == xyz.dtype
    return uv, uvd[..., 2]


def project_path(path, t, K4, Ps, fixed_view=False):
    """project() of every slab of a path (n+1, R, S, 3) at its own times t (n+1, R)."""
    out = [project(x, tt, K4, Ps, fixed_view) for x, tt in zip(path, t)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- the field of the oracle ----
@contextlib.contextmanager
def _oracle_dtype(orc, dtype):
    old = orc.F
    orc.F = dtype
    try:
        yield
    finally:
        orc.F = old


def oracle_field(orc, field, freqs, emb_t, dtype=np.float32):
    """The flow heads of an oracle field description (oracle.nsff_oracle.field_from_module) as a `field` callable.  dtype float64:
    the oracle's own statements evaluated in float64 (its number format is the module constant ``F``, swapped for the call)."""
    cfg = field["cfg"]
    params = {k: v.astype(dtype) for k, v in field["params"].items()}
    emb_t = np.asarray(emb_t, dtype)

    def run(xyz, t, direction):
        R, S = xyz.shape[:2]
        with _oracle_dtype(orc, dtype):
            x = orc.pos_embedding(xyz.reshape(-1, 3).astype(dtype), np.asarray(freqs, dtype))
            rows = np.repeat(emb_t[t], S, 0)
            pad = np.zeros((R * S, cfg["in_dir"] + cfg["in_a"]), dtype)
            out = orc.nerf_forward(params, cfg, np.concatenate([x, pad, rows], 1), output_static=False,
                                   output_transient_flow=("fw",) if direction > 0 else ("bw",))
        return np.asarray(out[:, 4:7], dtype).reshape(R, S, 3)
    return run


# ---- trails ----
def line_pixels(x0, y0, x1, y1):
    """The N + 1 pixels of the segment (x0, y0) -> (x1, y1), N = max(|dx|, |dy|), in integers: pixel i is
    (x0 + floor((2 i dx + N) / (2 N)), y0 + floor((2 i dy + N) / (2 N))); N = 0: the one pixel."""
    dx, dy = int(x1) - int(x0), int(y1) - int(y0)
    N = max(abs(dx), abs(dy))
    if N == 0:
        return [(int(x0), int(y0))]
    return [(int(x0) + (2 * i * dx + N) // (2 * N), int(y0) + (2 * i * dy + N) // (2 * N)) for i in range(N + 1)]      # (// floors)


def round_end(u):
    """floor(u + 0.5f) in fp32"""
    return int(np.floor(f32(u) + f32(0.5)))


def canvas(H, W, uv, ok):
    """(H, W) uint32 keys ((j + 1) << 20) | q of the winning segment per pixel, 0 where none: uv (n+1, Q, 2) fp32, ok (n+1, Q) bool."""
    uv, ok = np.asarray(uv, f32), np.asarray(ok, bool)
    n, Q = uv.shape[0] - 1, uv.shape[1]
    keys = np.zeros((H, W), np.uint32)
    with np.errstate(invalid="ignore"):
        fine = ok & (np.abs(uv) < f32(MAX_COORD)).all(-1)          # (NaN, infinities and UNKNOWN fail)
    for j in range(n):
        for q in range(Q):
            if not (fine[j, q] and fine[j + 1, q]):
                continue
            x0, y0, x1, y1 = round_end(uv[j, q, 0]), round_end(uv[j, q, 1]), round_end(uv[j + 1, q, 0]), round_end(uv[j + 1, q, 1])
            if max(abs(x1 - x0), abs(y1 - y0)) > H + W:
                continue
            key = ((j + 1) << 20) | q
            for x, y in line_pixels(x0, y0, x1, y1):
                if 0 <= x < W and 0 <= y < H:
                    keys[y, x] = max(keys[y, x], key)
    return keys


def draw(image, uv, ok, lut):
    """The trail image of tracks.draw: lut[(255 (j + 1)) // n] where a key is set, the image elsewhere."""
    image, lut = np.asarray(image, np.uint8), np.asarray(lut, np.uint8)
    n = len(uv) - 1
    keys = canvas(image.shape[0], image.shape[1], uv, ok)
    out = image.copy()
    hit = keys != 0
    out[hit] = lut[(255 * (keys[hit] >> 20).astype(np.int64)) // n]
    return out
