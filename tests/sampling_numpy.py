"""numpy restatements of the sampling chain and the stand-alone geometry stages of csrc/rays.hip / csrc/rng.hip.

Two kinds, as in ssim_numpy.py / resize_numpy.py / flow_numpy.py:
  *64      float64 references of the OPERATION (oracle/nsff_oracle.py's formulas with every step in float64): what a kernel is held
           to under a tolerance.
  *32      the kernel's own fp32 arithmetic, one rounding per operation in the kernel's order (numpy float32 arrays round every
           elementwise operation once; csrc/rays.hip is built with -ffp-contract=off and coarse_from_draw of csrc/rng.hip carries
           `#pragma clang fp contract(off)`): what a kernel is held to bit for bit, or -- sample_pdf32_scan -- what shows on the host
           that the reference arithmetic alone passes a tolerance and that a named mutation does not.
Nothing here is tuned on a GPU result.
"""
import numpy as np

F = np.float32
WAVE = 64


# ---- inverse-CDF sampling ----
def _broadcast_u(u, n, dtype):
    u = np.asarray(u, dtype)
    return np.broadcast_to(u, (n, u.shape[-1]))


def sample_pdf64(bins, weights, u, eps=1e-5):
    """oracle.sample_pdf (reference rendering.py:10-49) with every step in float64.  bins (n, M + 1), weights (n, M), u (n_imp,) shared
    or (n, n_imp) per ray -> (n, n_imp) float64.  searchsorted(right=True); denom < eps -> 1."""
    bins, weights = np.asarray(bins, np.float64), np.asarray(weights, np.float64)
    n, m = weights.shape
    w = weights + eps
    pdf = w / w.sum(1, keepdims=True)
    cdf = np.concatenate([np.zeros((n, 1)), np.cumsum(pdf, 1)], 1)
    u = _broadcast_u(u, n, np.float64)
    inds = (cdf[:, None, :] <= u[:, :, None]).sum(-1)
    below, above = np.maximum(inds - 1, 0), np.minimum(inds, m)
    cdf_b, cdf_a = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    bin_b, bin_a = np.take_along_axis(bins, below, 1), np.take_along_axis(bins, above, 1)
    denom = cdf_a - cdf_b
    denom = np.where(denom < eps, 1.0, denom)
    return bin_b + (u - cdf_b) / denom * (bin_a - bin_b)


def _wave_sum32(v):
    """wave_sum: xor butterfly over the 64 lanes (offsets 32, 16, ... 1); v (n, 64) float32 -> (n,) (every lane holds the same sum)"""
    lanes = np.arange(WAVE)
    off = WAVE // 2
    while off:
        v = v + v[:, lanes ^ off]
        off >>= 1
    return v[:, 0]


def _wave_scan_add32(v):
    """wave_scan_add: Hillis-Steele inclusive scan over the 64 lanes (offsets 1, 2, ... 32); v (n, 64) float32"""
    off = 1
    while off < WAVE:
        up = np.zeros_like(v)
        up[:, off:] = v[:, :-off]
        v = np.where(np.arange(WAVE) >= off, v + up, v)
        off <<= 1
    return v


def cdf32_scan(weights, eps=1e-5, carry=True):
    """The CDF of sample_pdf_ray in its own fp32 order: per-lane partial sums of w + eps (lane l owns bins l, l + 64, ...), their
    wave sum, pdf = (w + eps) / total, per 64-bin chunk an inclusive Hillis-Steele scan plus the carry (the previous chunk's lane
    63).  carry=False restarts every chunk at 0 -- the mutation.  (n, M) -> (n, M + 1) float32."""
    w = np.asarray(weights, F)
    n, m = w.shape
    eps = F(eps)
    m_pad = -(-m // WAVE) * WAVE
    we = np.zeros((n, m_pad), F)
    we[:, :m] = w + eps
    part = np.zeros((n, WAVE), F)
    for c in range(m_pad // WAVE):                       # (a lane adds its bins in ascending order; a bin past M adds nothing)
        sl = we[:, c * WAVE:(c + 1) * WAVE]
        part = np.where(np.arange(WAVE) + c * WAVE < m, part + sl, part)
    total = _wave_sum32(part)[:, None]
    pdf = np.where(np.arange(m_pad) < m, we / total, F(0)).astype(F)
    cdf = np.zeros((n, m_pad + 1), F)
    run = np.zeros((n, 1), F)
    for c in range(m_pad // WAVE):
        inc = _wave_scan_add32(pdf[:, c * WAVE:(c + 1) * WAVE]) + run
        cdf[:, 1 + c * WAVE:1 + (c + 1) * WAVE] = inc
        if carry:
            run = inc[:, WAVE - 1:WAVE]
    return cdf[:, :m + 1]


def sample_pdf32_scan(bins, weights, u, eps=1e-5, carry=True, search="count"):
    """sample_pdf_ray in fp32: cdf32_scan, searchsorted(right=True), s = bb + (u - cb) / denom * (ba - bb) with one rounding per
    operation.  search="count": the number of CDF entries <= u, as oracle.sample_pdf states searchsorted; search="bisect": the
    kernel's binary search over [0, M + 1).  On a non-decreasing CDF the two are the same number.  With the carry dropped the CDF
    falls back to ~0 at every chunk seam and they differ: the count shifts the index of nearly every sample by the entries of the
    later chunks that lie below u, the bisection goes wrong only for the samples whose probes cross a seam."""
    bins = np.asarray(bins, F)
    n, m = np.asarray(weights).shape
    cdf = cdf32_scan(weights, eps, carry)
    u = _broadcast_u(u, n, F)
    if search == "count":
        lo = (cdf[:, None, :] <= u[:, :, None]).sum(-1)
    else:
        assert search == "bisect"
        lo = np.zeros(u.shape, np.int64)
        hi = np.full(u.shape, m + 1, np.int64)
        while (lo < hi).any():
            live = lo < hi
            mid = (lo + hi) >> 1
            le = np.take_along_axis(cdf, np.minimum(mid, m), 1) <= u
            lo = np.where(live & le, mid + 1, lo)
            hi = np.where(live & ~le, mid, hi)
    below, above = np.maximum(lo - 1, 0), np.minimum(lo, m)
    cb, ca = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    bb, ba = np.take_along_axis(bins, below, 1), np.take_along_axis(bins, above, 1)
    denom = ca - cb
    denom = np.where(denom < F(eps), F(1), denom)
    return (bb + (u - cb) / denom * (ba - bb)).astype(F)


def fine_samples64(rays, z_lin, zs_coarse, w_static, w_transient, u_s, u_t):
    """The fine depths of render_rays (reference rendering.py:314-348) in float64: bins = interval mid points of z_lin, weights =
    w[:, 1:-1], zs_fine = sort(cat(zs_coarse, samples...)).  w_transient / u_t may be None (one set).  `rays` only gives the ray
    count (the points o + d z are one fp32 multiply-add pair, held bit for bit by the test).
    -> samples_static, samples_transient (or None), zs_fine"""
    z = np.asarray(z_lin, np.float64)
    n = np.asarray(rays).shape[0]
    mids = np.broadcast_to(0.5 * (z[:-1] + z[1:]), (n, z.shape[0] - 1))
    s_s = sample_pdf64(mids, np.asarray(w_static)[:, 1:-1], u_s)
    s_t = None if w_transient is None else sample_pdf64(mids, np.asarray(w_transient)[:, 1:-1], u_t)
    parts = [np.asarray(zs_coarse, np.float64), s_s] + ([] if s_t is None else [s_t])
    return s_s, s_t, np.sort(np.concatenate(parts, 1), 1)


# ---- coarse depths ----
def coarse32(rays, z_lin, perturb, rnd):
    """coarse_samples_kernel / coarse_from_draw: lower, upper (interval mid points, the ends of z_lin at the ends), t = perturb *
    rnd, span = upper - lower, z = lower + span * t; xyz = o + (d * z).  perturb = 0: z = z_lin.  -> zs (n, S), xyz (n, S, 3) float32"""
    rays, z_lin = np.asarray(rays, F), np.asarray(z_lin, F)
    n, S = rays.shape[0], z_lin.shape[0]
    if perturb > 0:
        mids = F(0.5) * (z_lin[:-1] + z_lin[1:])
        lower = np.concatenate([z_lin[:1], mids])
        upper = np.concatenate([mids, z_lin[-1:]])
        t = F(perturb) * np.asarray(rnd, F).reshape(n, S)
        span = upper - lower
        zs = (lower + span * t).astype(F)
    else:
        zs = np.broadcast_to(z_lin, (n, S)).copy()
    return zs, points32(rays, zs)


def points32(rays, zs):
    """o + (d * z) in fp32, product rounded before the sum"""
    rays, zs = np.asarray(rays, F), np.asarray(zs, F)
    return (rays[:, None, 0:3] + rays[:, None, 3:6] * zs[..., None]).astype(F)


# ---- merge + sort ----
def rank_sort(values, stable=True):
    """fine_samples_kernel's rank sort of every row: element i goes to slot #{j: v_j < v_i or (v_j == v_i and j < i)}.  Slots nobody
    writes stay NaN.  stable=False is the mutation: ties are broken by `<=` on the value alone (#{j != i: v_j <= v_i}), which gives
    tied elements one rank and leaves the slot below them unwritten."""
    v = np.asarray(values, F)
    n, m = v.shape
    idx = np.arange(m)
    less = v[:, None, :] < v[:, :, None]                              # [row, i, j]: v_j < v_i
    equal = v[:, None, :] == v[:, :, None]
    tie = (idx[None, :] < idx[:, None]) if stable else (idx[None, :] != idx[:, None])
    rank = (less | (equal & tie[None])).sum(-1)
    out = np.full((n, m), np.nan, F)
    np.put_along_axis(out, rank, v, 1)
    return out


# ---- frustum visibility ----
def frustum_count64(xyz_ndc, K4, w2c, n_cams, n_frames, frame, H, W):
    """frustum_count in float64, after oracle.ndc_to_world + oracle.world_visibility, summed over the cameras of one frame.
    w2c: (n_cams * n_frames, 12) rows of the inverse poses; row c * n_frames + frame is camera c.  A frame outside the table is
    seen by no camera.
    -> counts (P,), margins (P, 3): the smallest |cam_z| over all cameras, and over the cameras in front the smallest distance of
    u to {0, W} and of v to {0, H} in pixels (inf where no camera is in front) -- how far each decision is from flipping."""
    p = np.asarray(xyz_ndc, np.float64)
    fx, fy, cx, cy = (float(v) for v in K4)
    counts = np.zeros(p.shape[0])
    margins = np.full((p.shape[0], 3), np.inf)
    if frame < 0 or frame >= n_frames:
        return counts, margins
    rz = 2.0 / (p[:, 2] - 1.0 - 1e-6)
    rx = -rz * p[:, 0] * cx / fx
    ry = -rz * p[:, 1] * cy / fy
    world = np.stack([rx, ry, rz], 0)
    table = np.asarray(w2c, np.float64).reshape(n_cams * n_frames, 3, 4)
    for c in range(n_cams):
        m = table[c * n_frames + frame]
        cam = m[:, :3] @ world + m[:, 3:]
        front = cam[2] < 0
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (fx * cam[0] + cx * -cam[2]) / -cam[2]
            v = (fy * -cam[1] + cy * -cam[2]) / -cam[2]
            inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
            d_u = np.where(front, np.minimum(np.abs(u), np.abs(u - W)), np.inf)
            d_v = np.where(front, np.minimum(np.abs(v), np.abs(v - H)), np.inf)
        counts += front & inside
        margins = np.minimum(margins, np.stack([np.abs(cam[2]), d_u, d_v], 1))
    return counts, margins


# ---- flow warp ----
def warp32(raw, xyz, zs, z_far):
    """warp_points_kernel: x + flow head (record offsets 8..10 forward, 11..13 backward), one fp32 add per component; a point with
    zs > z_far (strictly) gets + 0.  raw (P, stride >= 14), xyz (P, 3), zs (P,) -> xyz_fw, xyz_bw float32"""
    raw, xyz, zs = np.asarray(raw, F), np.asarray(xyz, F), np.asarray(zs, F)
    far = (zs > F(z_far))[:, None]
    return (xyz + np.where(far, F(0), raw[:, 8:11])).astype(F), (xyz + np.where(far, F(0), raw[:, 11:14])).astype(F)
