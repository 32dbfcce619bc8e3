"""Seeded inputs of tests/test_sampling_host.py (which proves on the CPU that they meet their conditions) and of
tests/test_sampling_kernels.py (which runs the kernels on them).  Every builder is cached: a reference is computed once and shared.

Sampling inputs: weights = rand ** 4 (most bins nearly empty, a few heavy: the shape of compositing weights), with special rows
  zero      all-zero row (the pdf is eps / (M eps): uniform)
  first     one spike of 1 in the first bin, everything else 0
  last      one spike in the last bin
  seam      one spike in bin 64, the first bin of the CDF's second 64-bin chunk (M > 64)
u: shared deterministic linspace(0, 1, n_imp) -- exact 0 and exact 1 included -- and per-ray random.

What counts as one CASE for the host test's caps and the recorded figures: one M of the direct nsff_sample_pdf test (all its
n_rays x n_imp x both u forms pooled) and one row of the nsff_fine_samples table (its sets and both u forms pooled).  A finer
split cannot hold the cap on loose tolerances by construction: with n_imp = 1 the shared u is [0], which sits in the first bin, and
on a spike row whose spike is elsewhere that bin is on the `denom < 2 eps` switch whatever the weights of the other rows are.

The special rows are loose by construction, not by accident of the seed: the all-zero row is a near-empty ray (sum(w + eps) = M
eps), where parity.sample_tolerance's weight-noise term alone is 0.012 M bin widths -- above a quarter of a bin from M = 21 on;
on a spike row u = 0 and u = 1 fall into empty bins unless the spike is there.  Among the 37 rays of a direct launch they are 4;
among the 7 rays of the fine table they are 4 as well, and no seed brings a table row with one set (the zero row alone is 1 / 7) or
with n_imp = 3 or 5 (the end points are 2 of 3 shared u) under 10 %.  The host test therefore holds the fine table's cap on the
plain rand ** 4 rows and prints the share over all rows next to it; the special rows' samples are held bit for bit to
nsff_sample_pdf's (assertion 2 of the GPU test), which the direct test holds to float64 with every row under the cap.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import scenes
import sampling_numpy as SN

F = np.float32
EPS = 1e-5

PDF_M = (1, 63, 64, 65, 128, 129, 191, 257)
PDF_RAYS = (1, 5, 37)
PDF_IMP = (1, 64, 65, 130)
FINE_RAYS = 7
# (S, n_imp, sets) of the nsff_fine_samples shapes (what each reaches: test_sampling_host.py::test_fine_table_reaches_the_named_routes)
FINE_TABLE = ((3, 1, 1), (64, 64, 2), (65, 17, 1), (67, 5, 2), (66, 33, 2), (128, 128, 2), (130, 64, 1), (257, 3, 2))
TIE_TABLE = ((65, 17, 2), (64, 64, 2))
TIE_SAME, TIE_ZERO, TIE_EDGE, TIE_EDGE_AT = 4, 5, 6, 3          # rays of a tie case: all coarse depths one number / zero weights in both sets / zs_coarse[3] = bins[0]
COARSE_S = (1, 2, 3, 64, 65)
COARSE_RAYS = (1, 5, 300)
COARSE_PERTURB = (0.0, 0.5, 1.0)


def special_rows(M):
    """name -> spike bin (None: the all-zero row), in the order they are placed"""
    rows = [("zero", None), ("first", 0), ("last", M - 1)]
    if M > 64:
        rows.append(("seam", 64))
    return rows


def _weights(rng, n, M, first_special=0, place=None):
    """(n, M) rand ** 4 with the special rows at rows 0, 1, ... as far as n reaches, starting at special row `first_special`
    (a single-row case rotates through them); place: indices of the special rows wanted (default all)"""
    w = (rng.rand(n, M) ** 4).astype(F)
    rows = special_rows(M)
    rows = rows if place is None else [rows[i] for i in place if i < len(rows)]
    for r in range(min(n, len(rows))):
        _, spike = rows[(first_special + r) % len(rows)]
        w[r] = 0
        if spike is not None:
            w[r, spike] = 1.0
    return w


def u_shared(n_imp):
    return torch.linspace(0, 1, n_imp).numpy()


@functools.lru_cache(maxsize=None)
def pdf_case(M, n_rays, n_imp):
    """inputs of one direct nsff_sample_pdf launch pair: per-ray bins (strictly increasing, 0 .. 1), weights, the two u forms"""
    rng = np.random.RandomState(1000 * M + 10 * n_rays + PDF_IMP.index(n_imp))
    steps = rng.uniform(0.5, 1.5, (n_rays, M + 1))
    edges = np.cumsum(steps, 1)
    bins = ((edges - edges[:, :1]) / (edges[:, -1:] - edges[:, :1])).astype(F)
    assert (np.diff(bins, axis=1) > 0).all()
    w = _weights(rng, n_rays, M, first_special=PDF_IMP.index(n_imp) if n_rays == 1 else 0)
    u = {"shared": u_shared(n_imp), "per_ray": rng.rand(n_rays, n_imp).astype(F)}
    return SimpleNamespace(M=M, n_rays=n_rays, n_imp=n_imp, bins=bins, weights=w, u=u)


@functools.lru_cache(maxsize=None)
def pdf_reference(M, n_rays, n_imp, form):
    """(float64 samples, parity.sample_tolerance) of one launch"""
    import parity
    c = pdf_case(M, n_rays, n_imp)
    return SN.sample_pdf64(c.bins, c.weights, c.u[form], EPS), parity.sample_tolerance(c.bins, c.weights, c.u[form], EPS)


@functools.lru_cache(maxsize=None)
def fine_case(S, n_imp, sets, ties=False):
    """inputs of one nsff_fine_samples shape: 7 rays, zs_coarse = coarse32(perturb = 1), weights (7, S) per set (the kernel reads
    w[:, 1:-1]).  The special rows are split between the sets -- static: zero, first; transient: last, seam (one set: all four) --
    so that every one is present and the share of samples on the loose tolerance stays under the cap at n_imp = 3."""
    rng = np.random.RandomState(7000 + 100 * S + n_imp + (50 if ties else 0))
    rays = scenes.synthetic_rays(FINE_RAYS, S)[0].numpy()
    z_lin = torch.linspace(0, 1, S).numpy()
    zs_coarse, _ = SN.coarse32(rays, z_lin, 1.0, rng.rand(FINE_RAYS, S).astype(F))
    M = S - 2
    w = []
    for k in range(sets):
        inner = _weights(rng, FINE_RAYS, M, place=None if sets == 1 else ((0, 1), (2, 3))[k])
        full = (rng.rand(FINE_RAYS, S) ** 4).astype(F)                   # (the end weights are read by nobody: random, not zero)
        full[:, 1:-1] = inner
        w.append(full)
    mids = F(0.5) * (z_lin[:-1] + z_lin[1:])
    if ties:
        zs_coarse[TIE_SAME] = F(0.5)
        for full in w:
            full[TIE_ZERO, 1:-1] = 0
        zs_coarse[TIE_EDGE, TIE_EDGE_AT] = mids[0]
    u = {"shared": [u_shared(n_imp)] * sets, "per_ray": [rng.rand(FINE_RAYS, n_imp).astype(F) for _ in range(sets)]}
    return SimpleNamespace(S=S, n_imp=n_imp, sets=sets, M=M, Sf=S + sets * n_imp, rays=rays, z_lin=z_lin, zs_coarse=zs_coarse,
                           w=w, u=u, mids=np.broadcast_to(mids, (FINE_RAYS, S - 1)).copy())


@functools.lru_cache(maxsize=None)
def fine_reference(S, n_imp, sets, form, ties=False):
    """per set (float64 samples, tolerance), and the float64 zs_fine"""
    import parity
    c = fine_case(S, n_imp, sets, ties)
    s_s, s_t, zs = SN.fine_samples64(c.rays, c.z_lin, c.zs_coarse, c.w[0], c.w[1] if sets == 2 else None,
                                     c.u[form][0], c.u[form][1] if sets == 2 else None)
    tol = [parity.sample_tolerance(c.mids, c.w[k][:, 1:-1], c.u[form][k], EPS) for k in range(sets)]
    return [s_s, s_t][:sets], tol, zs


def sampling_cases():
    """{case name: [(bins, interior weights, u, plain rows)]} -- every launch of section 3, grouped into the cases of the module
    docstring; plain rows: boolean (n,), False on the special rows"""
    def plain(w):
        return (w != 0).sum(1) > 1

    out = {}
    for M in PDF_M:
        out[f"pdf M={M}"] = [(c.bins, c.weights, c.u[form], plain(c.weights)) for n in PDF_RAYS for k in PDF_IMP
                             for c in [pdf_case(M, n, k)] for form in ("shared", "per_ray")]
    for S, n_imp, sets in FINE_TABLE:
        c = fine_case(S, n_imp, sets)
        out[f"fine S={S} n_imp={n_imp} sets={sets}"] = [(c.mids, c.w[k][:, 1:-1], c.u[form][k], plain(c.w[k][:, 1:-1]))
                                                        for k in range(sets) for form in ("shared", "per_ray")]
    return out


# ---- coarse depths ----
@functools.lru_cache(maxsize=None)
def coarse_case(S, n_rays):
    rng = np.random.RandomState(300 + 7 * S + n_rays)
    rays = scenes.synthetic_rays(n_rays, 40 + S)[0].numpy()
    return SimpleNamespace(rays=rays, z_lin=torch.linspace(0, 1, S).numpy(), rnd=rng.rand(n_rays, S).astype(F))


# ---- frustum visibility ----
VIS_P = (1, 255, 256, 257, 1000)
VIS_CAMS = (1, 3)


class VisDataset(scenes.DatasetStub):
    """scenes.DatasetStub with n_cams training cameras: poses (n_cams * N_frames, 3, 4), camera c of frame f at row c * N_frames + f"""

    def __init__(self, n_cams, seed=5):
        super().__init__(seed)
        self.cam_train = list(range(n_cams))
        self.poses = np.concatenate([scenes.DatasetStub(seed + 11 * c).poses for c in range(n_cams)], 0)


def vis_table64(dataset):
    """(n_cams * n_frames, 12) float64 inverse poses (ray_geometry.world_to_camera_table inverts in fp32)"""
    p = np.asarray(dataset.poses, np.float64)
    pose4 = np.tile(np.eye(4), (p.shape[0], 1, 1))
    pose4[:, :3] = p
    return np.linalg.inv(pose4)[:, :3].reshape(-1, 12)


@functools.lru_cache(maxsize=None)
def vis_points(n=1000, seed=5):
    """NDC points in a seeded shuffle (a prefix is a sample of the whole): points on scenes' wide-NDC rays (half of them), points
    behind the cameras (z > 1, a fifth), points with z close to 1 (a fifth, z = 1 included), points far outside (a tenth)"""
    rng = np.random.RandomState(900 + seed)
    rays = scenes.wide_rays(n, seed)[0].numpy()
    z = rng.uniform(0, 1, n).astype(F)
    kind = rng.choice(4, n, p=[0.5, 0.2, 0.2, 0.1])
    z[kind == 1] = rng.uniform(1.2, 3.0, (kind == 1).sum())
    near1 = np.array([1e-2, 1e-3, 1e-4, 1e-5, 0.0])
    z[kind == 2] = (1.0 - near1[rng.randint(0, near1.size, (kind == 2).sum())])
    pts = (rays[:, 0:3] + rays[:, 3:6] * z[:, None]).astype(F)
    pts[kind == 2, 2] = z[kind == 2]                      # (o_z + d_z z is not z: set the NDC depth itself)
    pts[kind == 1, 2] = z[kind == 1]
    pts[kind == 3, :2] *= 4
    return pts


def vis_frames(n_frames):
    return (0, n_frames - 1)


def vis_undecided(margins, dataset, table64):
    """a point is undecided within RTOL x W px of a u boundary, RTOL x H px of a v boundary, or RTOL x max|t| of cam_z = 0"""
    import parity
    W, H = dataset.img_wh
    t_max = np.abs(table64.reshape(-1, 3, 4)[:, :, 3]).max()
    return (margins[:, 0] < parity.RTOL * t_max) | (margins[:, 1] < parity.RTOL * W) | (margins[:, 2] < parity.RTOL * H)


@functools.lru_cache(maxsize=None)
def vis_case(n_cams, frame):
    ds = VisDataset(n_cams)
    K = ds.Ks[0].numpy()
    K4 = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    table = vis_table64(ds)
    pts = vis_points()
    counts, margins = SN.frustum_count64(pts, K4, table, n_cams, ds.N_frames, frame, ds.img_wh[1], ds.img_wh[0])
    return SimpleNamespace(dataset=ds, K=K, K4=K4, table=table, points=pts, counts=counts, margins=margins,
                           undecided=vis_undecided(margins, ds, table))


# ---- flow warp ----
WARP_P = (1, 85, 86, 1000)
WARP_Z_FAR = 0.95


@functools.lru_cache(maxsize=None)
def warp_case(P, stride=16):
    """records, points, depths: every third depth is exactly z_far (not far: the flow is added), every third the next float above
    it (far: unchanged), the others random on both sides"""
    rng = np.random.RandomState(60 + P)
    raw = rng.uniform(-1, 1, (P, stride)).astype(F)
    xyz = rng.uniform(-1, 1, (P, 3)).astype(F)
    zs = rng.uniform(0.8, 1.0, P).astype(F)
    zs[0::3] = F(WARP_Z_FAR)
    zs[1::3] = np.nextafter(F(WARP_Z_FAR), F(2))
    return SimpleNamespace(raw=raw, xyz=xyz, zs=zs)
