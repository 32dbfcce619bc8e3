"""The numpy twin of csrc/flowmedian.hip (nsff_flow_median, the image-guided weighted median of a flow map) as include/nsff_render.h
states it: the window stack, fp32 weights one operation per step, INTEGER weights, a stable sort per component, int64 cumulative
weights and the first index that reaches half the total.  The GPU tests compare the kernels with it at every pixel.  Also the
contrast pair the method conditions are stated on: optflow_numpy.make_pair's two motions with an image edge on the motion edge."""
import numpy as np

import motion_numpy
import optflow_numpy

F32 = np.float32
MAX_RADIUS = 7
WEIGHT_ONE = 65535


def spatial_table(radius, sigma_s):
    """(2r+1, 2r+1) fp32: 1 + (dx^2 + dy^2) / sigma_s^2, formed in float64 from the fp32 sigma_s and rounded once."""
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    ss = float(F32(sigma_s)) ** 2
    return (1.0 + (d[None, :] ** 2 + d[:, None] ** 2) / ss).astype(F32)


def weighted_median(flow, grey, valid=None, radius=7, sigma_i=12.75, sigma_s=7.0):
    """flow (P, H, W, 2) fp32, grey (P, H, W) fp32, valid (P, H, W) uint8 or None -> (P, H, W, 2) fp32."""
    flow, grey = np.asarray(flow), np.asarray(grey)
    assert flow.dtype == np.float32 and grey.dtype == np.float32 and flow.ndim == 4 and flow.shape[-1] == 2
    P, H, W = grey.shape
    assert flow.shape[:3] == (P, H, W) and 1 <= radius <= MAX_RADIUS
    r, n = radius, (2 * radius + 1) ** 2
    s = spatial_table(r, sigma_s)
    sig = F32(sigma_i)
    kn = motion_numpy.known(flow)
    allowed = kn if valid is None else kn & (np.asarray(valid) != 0)
    pad = lambda a, fill: np.pad(a, [(0, 0), (r, r), (r, r)] + [(0, 0)] * (a.ndim - 3), constant_values=fill)
    pf, pg, pa = pad(flow, 0), pad(grey, 0), pad(allowed, False)
    vals = np.zeros((2, P, H, W, n), F32)                                        # the window is the last axis: sorted in place
    wq = np.zeros((P, H, W, n), np.int32)
    j = 0
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sl = (slice(None), slice(r + dy, r + dy + H), slice(r + dx, r + dx + W))
            with np.errstate(all="ignore"):
                di = (pg[sl] - grey) / sig
                w = F32(1) / ((F32(1) + di * di) * s[dy + r, dx + r])
                q = np.rint(w * F32(WEIGHT_ONE))
            assert q.dtype == np.float32
            cand = pa[sl] if (dx or dy) else np.ones((P, H, W), bool)            # the centre votes whatever `valid` says
            q = np.where(cand & np.isfinite(q), q, 0)                            # (outside the image pa is False)
            wq[..., j] = q.astype(np.int32) if (dx or dy) else WEIGHT_ONE
            for c in range(2):
                vals[c, ..., j] = np.where(cand, pf[sl][..., c], 0)              # weight 0: the value cannot matter
            j += 1
    total = wq.sum(-1, dtype=np.int64)
    out = np.empty_like(flow)
    for c in range(2):
        order = np.argsort(vals[c], axis=-1, kind="stable")
        sv = np.take_along_axis(vals[c], order, -1)
        cw = np.cumsum(np.take_along_axis(wq, order, -1), axis=-1, dtype=np.int64)
        first = np.argmax(2 * cw >= total[..., None], axis=-1)
        out[..., c] = np.take_along_axis(sv, first[..., None], -1)[..., 0]
    return np.where(kn[..., None], out, flow)


def make_contrast_pair(H, W, seed=0):
    """optflow_numpy.make_pair's pair with an image edge on the motion edge: the same motions, centre, radius and textures (drawn in
    the same order), each texture value t mapped to t / 24 * 0.5 + 0.5, the background 30 + 100 * that and the disc 150 + 100 * that;
    no rescaling by min / max.  The same dict."""
    rng = np.random.default_rng(seed)
    back, front = optflow_numpy._texture(rng), optflow_numpy._texture(rng)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cx, cy, radius = 0.5 * W, 0.5 * H, 0.22 * W
    unit = lambda t: t / 24 * 0.5 + 0.5

    def frame(t):
        bx, by = optflow_numpy.BACKGROUND_MOTION[0] * t, optflow_numpy.BACKGROUND_MOTION[1] * t
        dx, dy = optflow_numpy.DISC_MOTION[0] * t, optflow_numpy.DISC_MOTION[1] * t
        dist = np.hypot(xs - dx - cx, ys - dy - cy)
        return np.where(dist <= radius, 150 + 100 * unit(front(xs - dx, ys - dy)), 30 + 100 * unit(back(xs - bx, ys - by))), dist

    (a, dist), (b, _) = frame(0), frame(1)
    disc = dist <= radius
    flow = np.where(disc[..., None], np.array(optflow_numpy.DISC_MOTION), np.array(optflow_numpy.BACKGROUND_MOTION))[None]
    return dict(images0=a.astype(F32)[None], images1=b.astype(F32)[None], flow=flow, disc=disc, rim=np.abs(dist - radius))


def rim_epe(flow, pair, rim=6, border=8):
    """(rim, interior, whole): the mean end-point error over the pixels within `rim` px of the disc's rim and more than `border` px
    from the image border, over the rest, and over the whole image."""
    H, W = pair["disc"].shape
    ys, xs = np.mgrid[0:H, 0:W]
    at_rim = (pair["rim"] <= rim) & (np.minimum(xs, W - 1 - xs) > border) & (np.minimum(ys, H - 1 - ys) > border)
    err = np.linalg.norm(np.asarray(flow, np.float64).reshape(H, W, 2) - pair["flow"][0], axis=-1)
    return float(err[at_rim].mean()), float(err[~at_rim].mean()), float(err.mean())


def chain(pair, levels=4, warps=5, iters=30):
    """The twin's whole chain on a pair: flow both ways (the images swapped), the forward-backward check, -> (flow (1, H, W, 2) fp32,
    valid (1, H, W) uint8) of the forward direction."""
    kw = dict(levels=levels, warps=warps, iters=iters)
    fw = optflow_numpy.optical_flow(pair["images0"], pair["images1"], **kw)
    bw = optflow_numpy.optical_flow(pair["images1"], pair["images0"], **kw)
    zero = np.zeros_like(fw)
    valid = motion_numpy.motion_maps(np.concatenate([fw, zero]), np.concatenate([zero, bw]), None)["valid"]
    return fw, valid[:1, 0]
