"""The numpy twin of csrc/optflow.hip (TV-L1 optical flow), one numpy operation per kernel operation and in the kernel's order, stage
by stage as include/nsff_render.h states them; in fp32 it is what the GPU tests compare bit for bit.  `dtype` switches the same code
to float64.  Images and planes are (n, H, W); a flow state is (6, P, H, W) = u1 | u2 | p11 | p12 | p21 | p22, the per-warp constants
(5, P, H, W) = Ix | Iy | g | rho_c | I1w.  Also the synthetic two-motion pair the accuracy condition is stated on."""
import numpy as np

F32 = np.float32


def grey(images, dtype=F32):
    """(n, H, W, 3) uint8 -> (0.299 R + 0.587 G) + 0.114 B on the 0..255 scale; (n, H, W) floats pass through."""
    images = np.asarray(images)
    if images.dtype != np.uint8:
        return images.astype(dtype)
    c = images.astype(dtype)
    return (dtype(0.299) * c[..., 0] + dtype(0.587) * c[..., 1]) + dtype(0.114) * c[..., 2]


def _binomial(a, axis):
    """[1, 4, 6, 4, 1] / 16 along `axis`, replicated border: (((a[-2] + a[+2]) + (a[-1] + a[+1]) * 4) + a[0] * 6) * 0.0625."""
    n, dt = a.shape[axis], a.dtype.type
    idx = np.arange(n)
    t = lambda d: np.take(a, np.clip(idx + d, 0, n - 1), axis=axis)
    return (((t(-2) + t(2)) + (t(-1) + t(1)) * dt(4)) + a * dt(6)) * dt(0.0625)


def down(planes):
    """One pyramid step: blur, horizontal pass first, then every second pixel from (0, 0)."""
    return np.ascontiguousarray(_binomial(_binomial(planes, 2), 1)[:, ::2, ::2])


def n_levels(H, W, levels):
    """The levels in use: clipped so that the coarsest keeps both sides >= 4."""
    n = 0
    for l in range(levels):
        if l > 0 and (H < 4 or W < 4):
            break
        n, H, W = n + 1, (H + 1) // 2, (W + 1) // 2
    return n


def _bilinear(planes, cx, cy):
    """planes (n, h, w) at the coordinates cx, cy (n or 1, H, W), already clamped into the level."""
    dt = planes.dtype.type
    h, w = planes.shape[1:]
    fx, fy = np.floor(cx), np.floor(cy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = cx - fx, cy - fy
    n = np.arange(planes.shape[0])[:, None, None]
    omx, omy = dt(1) - ax, dt(1) - ay
    top = planes[n, y0, x0] * omx + planes[n, y0, x1] * ax
    bot = planes[n, y1, x0] * omx + planes[n, y1, x1] * ax
    return (top * omy) + (bot * ay)


def up(planes, out_hw):
    """Coarse planes to the finer level out_hw: bilinear at (x / 2, y / 2) clamped to the level, values times 2."""
    dt = planes.dtype.type
    h, w = planes.shape[1:]
    H, W = out_hw
    assert ((H + 1) // 2, (W + 1) // 2) == (h, w)
    cx = np.minimum(np.arange(W, dtype=dt) * dt(0.5), dt(w - 1))[None, None, :] + np.zeros((1, H, 1), dt)
    cy = np.minimum(np.arange(H, dtype=dt) * dt(0.5), dt(h - 1))[None, :, None] + np.zeros((1, 1, W), dt)
    return _bilinear(planes, cx, cy) * dt(2)


_NETWORK = ((1, 2), (4, 5), (7, 8), (0, 1), (3, 4), (6, 7), (1, 2), (4, 5), (7, 8), (0, 3), (5, 8), (4, 7), (3, 6), (1, 4), (2, 5),
            (4, 7), (4, 2), (6, 4), (4, 2))


def median(planes):
    """3 x 3 median, replicated border: the kernel's nineteen exchanges (swap when b < a), element 4 of the result."""
    n, H, W = planes.shape
    ys, xs = np.arange(H), np.arange(W)
    v = [planes[:, np.clip(ys + j, 0, H - 1)][:, :, np.clip(xs + i, 0, W - 1)] for j in (-1, 0, 1) for i in (-1, 0, 1)]
    for a, b in _NETWORK:
        sw = v[b] < v[a]
        v[a], v[b] = np.where(sw, v[b], v[a]), np.where(sw, v[a], v[b])
    return v[4]


def warp(I0, I1, u):
    """I0, I1 (P, H, W), u (2, P, H, W) -> consts (5, P, H, W)."""
    dt = I0.dtype.type
    P, H, W = I0.shape
    ys, xs = np.arange(H), np.arange(W)
    Dx = (I1[:, :, np.minimum(xs + 1, W - 1)] - I1[:, :, np.maximum(xs - 1, 0)]) * dt(0.5)
    Dy = (I1[:, np.minimum(ys + 1, H - 1)] - I1[:, np.maximum(ys - 1, 0)]) * dt(0.5)
    u1, u2 = u[0], u[1]
    cx = np.minimum(np.maximum(xs.astype(dt)[None, None, :] + u1, dt(0)), dt(W - 1))
    cy = np.minimum(np.maximum(ys.astype(dt)[None, :, None] + u2, dt(0)), dt(H - 1))
    I1w, Ix, Iy = _bilinear(I1, cx, cy), _bilinear(Dx, cx, cy), _bilinear(Dy, cx, cy)
    g = Ix * Ix + Iy * Iy
    rho_c = ((I1w - Ix * u1) - Iy * u2) - I0
    return np.stack([Ix, Iy, g, rho_c, I1w])


def _back(p, axis):
    """The divergence's backward difference: p first, p - p(-1) inside, -p(-1) last."""
    out = np.empty_like(p)
    first, last = [slice(None)] * 3, [slice(None)] * 3
    inner, inner_b, before_last = [slice(None)] * 3, [slice(None)] * 3, [slice(None)] * 3
    first[axis], last[axis], before_last[axis] = slice(0, 1), slice(-1, None), slice(-2, -1)
    inner[axis], inner_b[axis] = slice(1, -1), slice(0, -2)
    out[tuple(inner)] = p[tuple(inner)] - p[tuple(inner_b)]
    out[tuple(first)] = p[tuple(first)]
    out[tuple(last)] = -p[tuple(before_last)]
    return out


def _forward(u, axis):
    """Forward difference, zero in the last column / row."""
    out = np.zeros_like(u)
    a, b, c = [slice(None)] * 3, [slice(None)] * 3, [slice(None)] * 3
    a[axis], b[axis], c[axis] = slice(0, -1), slice(1, None), slice(0, -1)
    out[tuple(a)] = u[tuple(b)] - u[tuple(c)]
    return out


def iterate(consts, state, iters, lam=0.15, theta=0.3, tau=0.25):
    """`iters` iterations; returns the new state (6, P, H, W)."""
    dt = state.dtype.type
    lam, theta, tau = dt(lam), dt(theta), dt(tau)
    l_t, taut = lam * theta, tau / theta
    Ix, Iy, g, rho_c = consts[0], consts[1], consts[2], consts[3]
    u1, u2, p11, p12, p21, p22 = (state[i].copy() for i in range(6))
    lg = l_t * g
    big = g > dt(1e-10)
    for _ in range(iters):
        rho = (rho_c + Ix * u1) + Iy * u2
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = (-rho) / g
        f = np.where(rho < -lg, l_t, np.where(rho > lg, -l_t, np.where(big, ratio, dt(0))))
        v1, v2 = u1 + f * Ix, u2 + f * Iy
        u1 = v1 + theta * (_back(p11, 2) + _back(p12, 1))
        u2 = v2 + theta * (_back(p21, 2) + _back(p22, 1))
        ux, uy = _forward(u1, 2), _forward(u1, 1)
        den = dt(1) + taut * np.sqrt(ux * ux + uy * uy)
        p11, p12 = (p11 + taut * ux) / den, (p12 + taut * uy) / den
        ux, uy = _forward(u2, 2), _forward(u2, 1)
        den = dt(1) + taut * np.sqrt(ux * ux + uy * uy)
        p21, p22 = (p21 + taut * ux) / den, (p22 + taut * uy) / den
    return np.stack([u1, u2, p11, p12, p21, p22])


def optical_flow(images0, images1, levels=5, warps=5, iters=30, lam=0.15, theta=0.3, tau=0.25, median_filter=True, dtype=F32):
    """The whole estimate: (P, H, W, 2), x first."""
    pyr0, pyr1 = [grey(images0, dtype)], [grey(images1, dtype)]
    P, H, W = pyr0[0].shape
    for _ in range(n_levels(H, W, levels) - 1):
        pyr0.append(down(pyr0[-1])), pyr1.append(down(pyr1[-1]))
    state = None
    for I0, I1 in zip(pyr0[::-1], pyr1[::-1]):
        new = np.zeros((6,) + I0.shape, dtype)
        if state is not None:
            new[:2] = up(state[:2].reshape((2 * P,) + state.shape[2:]), I0.shape[1:]).reshape((2,) + I0.shape)
        state = new
        for _ in range(warps):
            state = iterate(warp(I0, I1, state[:2]), state, iters, lam, theta, tau)
            if median_filter:
                state[:2] = median(state[:2].reshape((2 * P,) + I0.shape[1:])).reshape((2,) + I0.shape)
    return np.ascontiguousarray(np.stack([state[0], state[1]], -1))


# ---- the synthetic two-motion pair ----
BACKGROUND_MOTION, DISC_MOTION = (-2.0, 0.7), (3.0, -1.5)


def _texture(rng, n=24, top=0.9):
    """A sum of n sinusoids with spatial frequencies below `top` rad / px, as a function of (x, y)."""
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.15, top, n)
    kx, ky, ph, amp = mag * np.cos(ang), mag * np.sin(ang), rng.uniform(0, 2 * np.pi, n), rng.uniform(0.5, 1.0, n)
    return lambda x, y: sum(a * np.sin(p + fx * x + fy * y) for a, p, fx, fy in zip(amp, ph, kx, ky))


def make_pair(H, W, seed=0):
    """dict: images0 / images1 (1, H, W) fp32 on the 0..255 scale, flow (1, H, W, 2) float64 -- the true motion of what images0
    shows at each pixel -- disc (H, W) bool, the disc in images0, and rim (H, W) float64, the distance from the disc's rim in pixels.
    The background moves by BACKGROUND_MOTION, a disc of radius 0.22 W in front of it by DISC_MOTION; each has its own texture."""
    rng = np.random.default_rng(seed)
    back, front = _texture(rng), _texture(rng)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cx, cy, radius = 0.5 * W, 0.5 * H, 0.22 * W

    def frame(t):
        bx, by = BACKGROUND_MOTION[0] * t, BACKGROUND_MOTION[1] * t
        dx, dy = DISC_MOTION[0] * t, DISC_MOTION[1] * t
        dist = np.hypot(xs - dx - cx, ys - dy - cy)
        return np.where(dist <= radius, front(xs - dx, ys - dy), back(xs - bx, ys - by)), dist

    (a, dist), (b, _) = frame(0), frame(1)
    lo, hi = min(a.min(), b.min()), max(a.max(), b.max())
    scale = lambda img: ((img - lo) * (255.0 / (hi - lo))).astype(F32)[None]
    disc = dist <= radius
    flow = np.where(disc[..., None], np.array(DISC_MOTION), np.array(BACKGROUND_MOTION))[None]
    return dict(images0=scale(a), images1=scale(b), flow=flow, disc=disc, rim=np.abs(dist - radius))


def interior_epe(flow, pair, rim=6, border=8):
    """(the estimate's mean end-point error, the zero flow's) over the pixels more than `rim` px from the disc's rim and more than
    `border` px from the image border."""
    H, W = pair["disc"].shape
    ys, xs = np.mgrid[0:H, 0:W]
    keep = (pair["rim"] > rim) & (np.minimum(xs, W - 1 - xs) > border) & (np.minimum(ys, H - 1 - ys) > border)
    truth = pair["flow"][0]
    err = np.linalg.norm(np.asarray(flow, np.float64).reshape(H, W, 2) - truth, axis=-1)
    return float(err[keep].mean()), float(np.linalg.norm(truth, axis=-1)[keep].mean())
