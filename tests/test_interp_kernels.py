"""The kernels of csrc/interp.hip, called directly (`_lib.splat_planes`, `_lib.mpi_composite`), against the float64 restatement
in tests/splat_ref.py -- on the routes tests/test_interpolate.py does not take: more than 64 planes (the composite's carry across
64-plane chunks), record overflow (a workspace smaller than the far records need), frames of more than SPLAT_MAX_TILES tiles,
the quiet downgrades to the atomic route (misaligned / too short workspace), accumulators and workspace that are NOT fresh zero
pages (NaN / 0xFF prefill), one workspace serving two splats.

What is compared.  The splat's five ACCUMULATOR channels (r, g, b, a, norm) of every (pixel, plane) cell, before the
normalisation rgb/norm, a/norm: that ratio cancels a sample that is counted twice (a duplicate destination tile, a record consumed by
both the gather and the overflow atomics, a halo cell owned by two tiles), the sums do not.  No cell and no sample is left out:
the landing fractions of `multi_tile_case` are >= 0.25 away from an integer, so the fp32 and the float64 projection floor to the
same cell for every sample (asserted below).

Tolerances are measured on the REFERENCE side, never on the kernels: the largest distance between the fp32 restatement (same
formulas, every step rounded to fp32, sequential sums) and the float64 one on the test's own inputs, times 4 (the kernels sum in
another order, contract multiply-adds, and the composite's product scan associates differently).  The CPU tests recompute them, so
these figures are a record, not the source:

  accumulators, absolute, per (shape, direction); largest |fp32 - float64| (largest accumulator magnitude)
    (W, H, S)          forward            backward
    (96, 40, 24)       1.98e-5 (3.56)     2.32e-5 (3.50)
    (70, 19, 11)       1.21e-5 (2.86)     1.15e-5 (3.01)
    (40, 24, 130)      8.83e-6 (3.30)     8.25e-6 (3.19)
    (33, 9, 5)         3.30e-6 (1.90)     3.56e-6 (1.83)
    (1, 1, 1)          0 (nothing lands)  0 (nothing lands)
    (3, 2, 1)          0 (nothing lands)  9.34e-8 (0.25)
    (193, 4089, 2)     1.30e-3 (4.67)     -- (forward only)
  The smallest single contribution to the norm channel is 0.25 x 0.25 = 0.0625 (fractions of SPLAT_SHIFTS), so a missing or
  doubled sample is more than two orders of magnitude outside 4 x these, one order on the tall frame (every bound < 0.0625 / 10,
  asserted).  The tall frame's figure is the fp32 spacing of a landing coordinate near 4000 (2.4e-4 px) times the sums it enters;
  that is why the frame of more than 3072 tiles is 193 x 4089 (7 x 512 tiles) and not a narrower, taller one: at 5 x 24580 the
  same measurement gives 5.0e-3, and 4 x that is no longer below 0.0625 / 10.

  composite, relative to the largest reference magnitude, per S (largest over dt in {1e-3, 0.4, 0.999}, rgb and depth)
    S      1        63       64       65       128      129      130      256
    fp32   7.96e-8  3.85e-7  4.11e-7  4.71e-7  6.73e-7  7.11e-7  7.45e-7  7.10e-7
  With the carry across chunks dropped, the same scheme in fp32 is more than 1e5 bounds away at S = 65, 128, 129, 130, 256 (asserted > 100).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import parity
import splat_ref as R
import test_interpolate as TI
from test_interpolate import multi_tile_case
import nsff_pl_amd as A
from oracle import nsff_oracle as orc

MAX_TILES = 3072                                       # SPLAT_MAX_TILES of csrc/interp.hip
SAFETY = 4.0
MIN_CONTRIBUTION = 0.0625
ACCUM_SHAPES = ((96, 40, 24), (70, 19, 11), (40, 24, 130), (33, 9, 5), (1, 1, 1), (3, 2, 1))
OVERFLOW_SHAPES = ((96, 40, 24), (70, 19, 11))
TALL_SHAPE = (193, 4089, 2)
COMPOSITE_S = (1, 63, 64, 65, 128, 129, 130, 256)
COMPOSITE_DTS = (1e-3, 0.4, 0.999)
COMPOSITE_HW = (7, 3)
OPAQUE_AT = (0, 62, 63, 64, 65, -1)                    # plane of the fully opaque static sample of pixels 0..5 (-1: S - 1)
TRANSPARENT_PIXELS = (6, 7, 8)
# recorded measurements (see the docstring); the CPU tests recompute them
ACCUM_FIGURES = {(96, 40, 24): (1.98e-5, 2.32e-5), (70, 19, 11): (1.21e-5, 1.15e-5), (40, 24, 130): (8.83e-6, 8.25e-6),
                 (33, 9, 5): (3.30e-6, 3.56e-6), (1, 1, 1): (0.0, 0.0), (3, 2, 1): (0.0, 9.34e-8), (193, 4089, 2): (1.30e-3,)}
COMPOSITE_FIGURES = {1: 7.96e-8, 63: 3.85e-7, 64: 4.11e-7, 65: 4.71e-7, 128: 6.73e-7, 129: 7.11e-7, 130: 7.45e-7, 256: 7.10e-7}


# ---- the cases: inputs, float64 reference, measured bound -- computed once per shape and shared ----
@functools.lru_cache(maxsize=None)
def splat_case(W, H, S, directions=("fw", "bw")):
    res_t, res_tp1, dt, K, c2w, _, _ = multi_tile_case(W, H, S)
    c = SimpleNamespace(W=W, H=H, S=S, K=K, c2w=c2w, dt=dt, xyz=res_t["xyzs_fine"], res_t=res_t, res_tp1=res_tp1, dirs={})
    for name, res, key, scale in (("fw", res_t, "transient_flows_fw", dt), ("bw", res_tp1, "transient_flows_bw", 1 - dt)):
        if name not in directions:
            continue
        args = (c.xyz, res[key], res["transient_rgbs_fine"], res["transient_alphas_fine"], K, c2w, scale, W, H)
        ref = R.splat_accum_ref(*args)
        measured = float(np.abs(R.splat_accum_ref(*args, dtype=np.float32) - ref).max())
        near, tiles, records = R.landing_stats(c.xyz, res[key], K, c2w, scale, W, H)
        c.dirs[name] = SimpleNamespace(flow=res[key], rgb=res["transient_rgbs_fine"], alpha=res["transient_alphas_fine"], scale=scale,
                                       ref=ref, measured=measured, bound=SAFETY * measured, near=near, tiles=tiles, records=records)
    return c


def tall_case():
    return splat_case(*TALL_SHAPE, ("fw",))


def tile_count(W, H):
    return -(-W // TI.SPLAT_TILE_X) * -(-H // TI.SPLAT_TILE_Y)


def work_head_bytes(W, H, S):
    """bytes of the workspace's integer head (four counters per (tile, plane group) block + 8, rounded up to 32)"""
    n_blocks = tile_count(W, H) * -(-S // TI.SPLAT_PLANES)
    return ((4 * n_blocks + 8) * 4 + 31) // 32 * 32


@functools.lru_cache(maxsize=None)
def composite_inputs(S):
    """Synthetic accumulators (21, S, 8) x 2, static colour / alpha, depths.  Pixels 0..5 have one fully opaque static sample (plane
    OPAQUE_AT, where S has it), 6..8 are transparent throughout (6: nothing landed anywhere), the others draw their alphas at a
    per-pixel scale from 0.003 to 0.1 -- the transmittance at the last plane of a 256-plane pixel then ranges from ~0.7 to ~0, so
    every chunk carries weight somewhere -- with a fifth of the cells empty (all five channels 0: the norm-0 branch)."""
    rng = np.random.RandomState(100 + S)
    n = COMPOSITE_HW[0] * COMPOSITE_HW[1]
    a_scale = np.array([0.003, 0.01, 0.03, 0.1])[np.arange(n) % 4][:, None]

    def accum(shift):
        norm = rng.uniform(MIN_CONTRIBUTION, 3.0, (n, S))
        alpha = rng.uniform(0.05, 0.95, (n, S)) * a_scale
        alpha[list(TRANSPARENT_PIXELS)] = 0
        out = np.zeros((n, S, 8), np.float32)
        out[..., :3] = rng.uniform(0.05, 0.95, (n, S, 3)) * norm[..., None]
        out[..., 3] = alpha * norm
        out[..., 4] = norm
        out[rng.rand(n, S) < 0.2] = 0
        out[9 + (np.arange(S) + shift) % (n - 9), np.arange(S)] = 0          # (at least one empty cell per plane, also at S = 1)
        out[TRANSPARENT_PIXELS[0]] = 0
        return out
    fw, bw = accum(0), accum(5)
    s_rgb = rng.uniform(0.05, 0.95, (n, S, 3)).astype(np.float32)
    s_a = (rng.uniform(0.05, 0.95, (n, S)) * a_scale).astype(np.float32)
    s_a[list(TRANSPARENT_PIXELS)] = 0
    opaque = {}
    for pix, at in enumerate(OPAQUE_AT):
        at = S - 1 if at < 0 else at
        if at < S:
            s_a[pix, at] = 1.0
            opaque[pix] = at
    zs = np.sort(rng.uniform(-0.9, 0.8, (n, S)), 1).astype(np.float32)
    return SimpleNamespace(fw=fw, bw=bw, s_rgb=s_rgb, s_a=s_a, zs=zs, opaque=opaque, n=n)


@functools.lru_cache(maxsize=None)
def composite_case(S):
    """float64 reference per dt and the bound of this S: SAFETY x the largest fp32-sequential distance, relative to max |ref|"""
    c = composite_inputs(S)
    refs, measured = {}, 0.0
    for dt in COMPOSITE_DTS:
        refs[dt] = R.mpi_composite_ref(c.fw, c.bw, c.s_rgb, c.s_a, c.zs, dt)
        seq = R.mpi_composite_fp32(c.fw, c.bw, c.s_rgb, c.s_a, c.zs, dt)
        measured = max([measured] + [parity.max_rel_err(g, w) for g, w in zip(seq, refs[dt])])
    return SimpleNamespace(inputs=c, refs=refs, measured=measured, bound=SAFETY * measured)


def composite_excess(got, want, bound):
    """largest max-norm relative error of (rgb, depth) over the bound"""
    return max(parity.max_rel_err(g, w) for g, w in zip(got, want)) / bound


# ---- CPU: the restatement itself ----
def _scatter_average(inp, flow):
    """softsplat_average's (C, h, w) image / (2, h, w) flow interface on scatter_landings: identity geometry, the landing of
    pixel (x, y) is (x + flow_x, y + flow_y) exactly.  C <= 4 channels ride in r, g, b, a."""
    C, h, w = inp.shape
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all="ignore"):
        ox, oy = (xs + flow[0]).reshape(-1, 1), (ys + flow[1]).reshape(-1, 1)
    src = np.zeros((h * w, 1, 4), np.float32)
    src[:, 0, :C] = inp.reshape(C, -1).T
    acc = R.scatter_landings(ox, oy, src[..., :3], src[..., 3], w, h)
    return R.normalise(acc)[:, 0, :C].T.reshape(C, h, w)


def test_restatement_reproduces_the_known_answer_splat_cases():
    """The four hand-derived cases of tests/test_interpolate.py (integer shift, half pixel, collision + bounds, weights summing to one):
    the restatement's scatter, normalised the reference's way, gives the hand-derived answer and what orc.softsplat_average gives.
    The landings are handed over as px + flow: two of the cases land ON pixel centres, where any projection arithmetic (the float64
    one too) may floor to either side -- the 'average' discontinuity described in test_interpolate.py."""
    inp = np.arange(24, dtype=np.float32).reshape(2, 3, 4) + 1
    flow = np.zeros((2, 3, 4), np.float32)
    flow[0], flow[1] = 1, -1
    want = np.zeros_like(inp)
    want[:, :2, 1:] = inp[:, 1:, :3]
    assert np.array_equal(_scatter_average(inp, flow), want)
    assert np.array_equal(_scatter_average(inp, flow), orc.softsplat_average(inp, flow))

    inp = np.array([[[2.0, 4.0, 8.0, 16.0]]], np.float32)
    flow = np.zeros((2, 1, 4), np.float32)
    flow[0] = 0.5
    assert np.allclose(_scatter_average(inp, flow), [[[2.0, 3.0, 6.0, 12.0]]], rtol=1e-12)
    assert np.allclose(_scatter_average(inp, flow), orc.softsplat_average(inp, flow), rtol=1e-6)

    inp = np.array([[[1.0, 5.0, 9.0]]], np.float32)
    flow = np.zeros((2, 1, 3), np.float32)
    flow[0] = [1.0, 0.0, -7.0]
    assert np.allclose(_scatter_average(inp, flow), [[[0.0, 3.0, 0.0]]], rtol=1e-12)
    flow[0] = [np.nan, 0.0, 1e30]
    assert np.allclose(_scatter_average(inp, flow), [[[0.0, 5.0, 0.0]]], rtol=1e-12)
    with np.errstate(all="ignore"):
        assert np.allclose(_scatter_average(inp, flow), orc.softsplat_average(inp, flow))

    rng = np.random.RandomState(0)
    inp = np.ones((1, 9, 11), np.float32)
    flow = rng.uniform(-0.9, 0.9, (2, 9, 11)).astype(np.float32)
    out = _scatter_average(inp, flow)
    assert np.all((np.abs(out - 1) < 1e-12) | (out == 0))
    assert np.abs(out - orc.softsplat_average(inp, flow)).max() < 1e-5


def test_restatement_projects_identity_geometry_onto_px_plus_shift():
    """Through the projection: with multi_tile_case's identity pose the float64 landing is the sample's pixel plus its crafted
    shift (to the 1e-5 px the fp32 inputs allow), and the half-pixel / random known-answer cases hold through the whole
    splat_accum_ref."""
    res_t, _, dt, K, c2w, (W, H), (sx, sy) = multi_tile_case(33, 9, 5)
    ox, oy = R.landing_positions(res_t["xyzs_fine"], res_t["transient_flows_fw"], K, c2w, dt, W, H)
    px, py = np.tile(np.arange(W), H)[:, None], np.repeat(np.arange(H), W)[:, None]
    assert np.abs(ox - (px + sx)).max() < 1e-4 and np.abs(oy - (py + sy)).max() < 1e-4
    # a 4 x 1 image, every sample moved half a pixel to the right
    w, h = 4, 1
    xyz = np.zeros((w * h, 1, 3), np.float32)
    xyz[:, 0, 0] = np.arange(w) / (w / 2) - 1
    xyz[:, 0, 1] = 1.0
    xyz[:, 0, 2] = -0.5
    flow = np.zeros_like(xyz)
    flow[:, 0, 0] = 0.5 / (w / 2)
    Kc = np.array([[80.0, 0, w / 2], [0, 80.0, h / 2], [0, 0, 1]], np.float32)
    rgb = np.zeros((w * h, 1, 3), np.float32)
    rgb[:, 0, 0] = [2.0, 4.0, 8.0, 16.0]
    acc = R.splat_accum_ref(xyz, flow, rgb, np.zeros((w * h, 1), np.float32), Kc, np.eye(4)[:3], 1.0, w, h)
    assert np.allclose(R.normalise(acc)[:, 0, 0], [2.0, 3.0, 6.0, 12.0], rtol=1e-6)
    assert np.allclose(acc[:, 0, 4], [0.5, 1.0, 1.0, 1.0], rtol=1e-6)
    # a 11 x 9 image of ones, random shifts below one pixel (none within 1e-3 of a pixel centre): weights sum to one
    w, h = 11, 9
    rng = np.random.RandomState(0)
    f_px = rng.uniform(-0.9, 0.9, (2, h, w)).astype(np.float32)
    assert np.abs(f_px - np.round(f_px)).min() > 1e-3
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    xyz = np.stack([xs / (w / 2) - 1, 1 - ys / (h / 2), np.full((h, w), -0.5)], -1).reshape(h * w, 1, 3).astype(np.float32)
    flow = np.stack([f_px[0] / (w / 2), -f_px[1] / (h / 2), np.zeros((h, w))], -1).reshape(h * w, 1, 3).astype(np.float32)
    Kc = np.array([[80.0, 0, w / 2], [0, 80.0, h / 2], [0, 0, 1]], np.float32)
    acc = R.splat_accum_ref(xyz, flow, np.ones((h * w, 1, 3), np.float32), np.ones((h * w, 1), np.float32), Kc, np.eye(4)[:3], 1.0, w, h)
    out = R.normalise(acc)[:, 0, :].reshape(h, w, 4)
    assert np.all((np.abs(out - 1) < 1e-12) | (out == 0)) and (out != 0).any()
    want = orc.softsplat_average(np.ones((1, h, w), np.float32), f_px)[0]
    assert np.array_equal(out[..., 0] != 0, want != 0) and np.abs(out[..., 0] - want).max() < 1e-5
    assert np.abs(acc[:, 0, 4].sum() - sum(wgt[m].sum() for _, _, wgt, m in R._corners(
        *R.landing_positions(xyz, flow, Kc, np.eye(4)[:3], 1.0, w, h), w, h)[3])) < 1e-9


def test_restatement_agrees_with_the_oracle_above_64_planes():
    c = splat_case(40, 24, 130)
    with np.errstate(all="ignore"):
        o_rgb, o_depth = orc.interpolate(c.res_t, c.res_tp1, c.dt, c.K, c.c2w, (c.W, c.H))
    rgb, depth = R.mpi_composite_ref(c.dirs["fw"].ref, c.dirs["bw"].ref, c.res_t["static_rgbs_fine"],
                                     c.res_t["static_alphas_fine"], c.res_t["zs_fine"], c.dt)
    assert np.abs(o_rgb).max() > 0.3
    parity.assert_close("rgb", rgb.reshape(c.H, c.W, 3), o_rgb, parity.RTOL)
    parity.assert_close("depth", depth.reshape(c.H, c.W), o_depth, parity.RTOL)


@pytest.mark.parametrize("shape", ACCUM_SHAPES + (TALL_SHAPE, (24, 16, 256)))
def test_no_sample_sits_on_a_floor_boundary(shape):
    """fp32 and float64 landings floor to the same cell for EVERY sample of every case: nothing is excluded from a comparison"""
    W, H, S = shape
    res_t, res_tp1, dt, K, c2w, _, _ = multi_tile_case(W, H, S)
    for flow, scale in ((res_t["transient_flows_fw"], dt), (res_tp1["transient_flows_bw"], 1 - dt)):
        o64 = R.landing_positions(res_t["xyzs_fine"], flow, K, c2w, scale, W, H)
        o32 = R.landing_positions(res_t["xyzs_fine"], flow, K, c2w, scale, W, H, np.float32)
        for a, b in zip(o64, o32):
            assert np.isfinite(a).all() and np.array_equal(np.floor(a), np.floor(b))
            frac = a - np.floor(a)
            assert frac.min() > 0.2 and frac.max() < 0.8


@pytest.mark.parametrize("shape", ACCUM_SHAPES + (TALL_SHAPE,))
def test_accumulator_bounds_are_the_recorded_fp32_distance(shape):
    c = tall_case() if shape == TALL_SHAPE else splat_case(*shape)
    for d, figure in zip(c.dirs.values(), ACCUM_FIGURES[shape]):
        print(f"{shape}: max |accum| {np.abs(d.ref).max():.3f}, fp32 - float64 {d.measured:.3e}, bound {d.bound:.3e}")
        assert d.bound == SAFETY * d.measured and d.bound < MIN_CONTRIBUTION / 10
        assert abs(d.measured - figure) <= 0.1 * figure, (d.measured, figure)      # the docstring's table is current
        hit = d.ref[..., 4][d.ref[..., 4] > 0]
        assert hit.size == 0 or hit.min() > MIN_CONTRIBUTION * 0.99                 # one sample less is >= 0.0625 in the norm


def test_splat_cases_cover_the_routes_they_are_meant_for():
    for shape in ACCUM_SHAPES:
        c = splat_case(*shape)
        for d in c.dirs.values():                           # the full workspace holds every record: 'full' is the pure binned route
            assert d.records <= 2 * c.W * c.H * c.S
    for shape in ACCUM_SHAPES[:4]:
        assert all(d.records > 0 and (d.near & (d.tiles > 0)).sum() > 0 for d in splat_case(*shape).dirs.values())
    for shape in OVERFLOW_SHAPES:
        for d in splat_case(*shape).dirs.values():
            for capacity in overflow_capacities(d.records)[:-1]:
                assert 0 < capacity < d.records
            far = ~d.near
            assert (far & (d.tiles == 2)).sum() >= 50 and (far & (d.tiles == 4)).sum() >= 10
            assert d.records > (far & (d.tiles > 0)).sum()              # more records than far samples: 2 per sample is no ceiling
    W, H, S = TALL_SHAPE
    d = tall_case().dirs["fw"]
    assert tile_count(W, H) > MAX_TILES and (~d.near & (d.tiles > 0)).sum() >= 50
    assert max(tile_count(W, H) for W, H, _ in ACCUM_SHAPES) <= MAX_TILES


def overflow_capacities(needed):
    return (1, needed // 2, needed - 1, needed)


@pytest.mark.parametrize("S", COMPOSITE_S)
def test_composite_inputs_hold_the_named_cells(S):
    c = composite_inputs(S)
    assert c.n == 21 and c.n % 4 != 0
    for acc in (c.fw, c.bw):
        empty = acc[..., 4] == 0
        assert empty[len(OPAQUE_AT) + len(TRANSPARENT_PIXELS):].any() and not acc[empty].any()       # norm 0 <=> all channels 0
        assert (acc[..., 4][~empty] >= MIN_CONTRIBUTION).all()
    want = {p: (S - 1 if at < 0 else at) for p, at in enumerate(OPAQUE_AT) if (S - 1 if at < 0 else at) < S}
    assert c.opaque == want and {0, S - 1} <= set(c.opaque.values())
    for pix, at in c.opaque.items():
        assert c.s_a[pix, at] == 1.0
    if S >= 130:
        assert set(c.opaque.values()) == {0, 62, 63, 64, 65, S - 1}
    _, c_a = R.compose_planes(c.fw, c.bw, c.s_rgb, c.s_a, 0.4)
    assert (c_a[list(TRANSPARENT_PIXELS)] == 0).all()
    plain = c_a[len(OPAQUE_AT) + len(TRANSPARENT_PIXELS):]
    assert (plain < 1).all() and np.prod(1 - plain, 1).max() > 0.3        # the last chunk still carries weight in some pixel


@pytest.mark.parametrize("S", COMPOSITE_S)
def test_composite_tolerance_notices_a_dropped_carry(S):
    """Self-test of the composite bound (4 x the fp32-sequential distance): the kernel's scheme restated in fp32 -- 64 planes per
    chunk, carry across chunks -- stays inside it at every S; with the carry reset to 1 at the second chunk it does not."""
    case, c = composite_case(S), composite_inputs(S)
    print(f"S={S}: fp32 sequential - float64 {case.measured:.3e}, bound {case.bound:.3e}")
    assert case.bound == SAFETY * case.measured and 0 < case.bound < 1e-5
    assert abs(case.measured - COMPOSITE_FIGURES[S]) <= 0.1 * COMPOSITE_FIGURES[S]           # the docstring's table is current
    for dt in COMPOSITE_DTS:
        good = R.mpi_composite_chunked_fp32(c.fw, c.bw, c.s_rgb, c.s_a, c.zs, dt)
        assert composite_excess(good, case.refs[dt], case.bound) <= 1, (S, dt)
        if S > 64:
            bad = R.mpi_composite_chunked_fp32(c.fw, c.bw, c.s_rgb, c.s_a, c.zs, dt, drop_carry_at=1)
            excess = composite_excess(bad, case.refs[dt], case.bound)
            print(f"S={S} dt={dt}: carry dropped at the second chunk: {excess:.3g} bounds")
            assert excess > 100, (S, dt)


# ---- GPU ----
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _splat(c, d, accum, work):
    """one nsff_splat_planes call of direction d of case c into accum (n, S, 8)"""
    from nsff_pl_amd import _lib
    P = R.projection_matrix(c.K, c.c2w, np.float32)
    K4 = [c.K[0, 0], c.K[1, 1], c.K[0, 2], c.K[1, 2]]
    _lib.splat_planes(c.H, c.W, c.S, K4, P.reshape(-1), d.scale, _dev(c.xyz), _dev(d.flow), _dev(d.rgb), _dev(d.alpha), accum, work)


def _nan_accum(c, k=1):
    return torch.full((k, c.W * c.H, c.S, 8), float("nan"), device=DEV)


def _ff_bytes(n, offset=0):
    """n bytes of 0xFF that start `offset` bytes into a 512-byte aligned allocation"""
    whole = torch.full((n + offset,), 0xFF, dtype=torch.uint8, device=DEV)
    assert whole.data_ptr() % 512 == 0
    return whole[offset:]


def _check_accum(what, accum, d, other=None):
    got = accum.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: cells left unwritten (NaN prefill shows)"
    assert not got[..., 5:].any(), f"{what}: padding channels"
    err = np.abs(got[..., :5] - d.ref).reshape(-1, 5).max(0)
    print(f"{what}: GPU - float64 per channel {' '.join(f'{e:.3e}' for e in err)}, bound {d.bound:.3e}")
    assert err.max() <= d.bound, f"{what}: {err.max():.3e} > {d.bound:.3e}"
    if other is not None:
        gap = float(np.abs(got - other.cpu().numpy().astype(np.float64)).max())
        print(f"{what}: against the atomic route {gap:.3e}")
        assert gap <= d.bound, f"{what}: differs from work=None by {gap:.3e} > {d.bound:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["full", "none", "misaligned", "short"])
@pytest.mark.parametrize("shape", ACCUM_SHAPES, ids=str)
def test_hip_splat_accumulators_match_float64(shape, variant, hip_lib):
    """All five channels of every cell, forward then backward flows through ONE workspace (as interpolate() does), accumulators
    prefilled with NaN and the workspace with 0xFF.  full: binned route; none / misaligned (16 bytes into an allocation) / short
    (head + 31 bytes): the atomic route -- a downgraded workspace is not written at all."""
    from nsff_pl_amd import _lib
    c = splat_case(*shape)
    W, H, S = shape
    head = work_head_bytes(W, H, S)
    full = _lib.splat_work_bytes(H, W, S)
    assert full == head + 2 * W * H * S * 32
    work = {"full": lambda: _ff_bytes(full), "none": lambda: None, "misaligned": lambda: _ff_bytes(full, 16),
            "short": lambda: _ff_bytes(head + 31)}[variant]()
    if work is not None:
        assert work.data_ptr() % 32 == (16 if variant == "misaligned" else 0) and work.is_contiguous()
    accum = _nan_accum(c, 2)
    for k, d in enumerate(c.dirs.values()):
        _splat(c, d, accum[k], work)
    torch.cuda.synchronize()
    for k, (name, d) in enumerate(c.dirs.items()):
        _check_accum(f"{shape} {variant} {name}", accum[k], d)
    if variant == "full":
        # the binned route ran: the head's first array (records per destination block) counts exactly the far records of the
        # splat that used the workspace last, and that many record slots behind the head were written
        n_blocks = tile_count(W, H) * -(-S // TI.SPLAT_PLANES)
        ints = work[:head].view(torch.int32)
        last = list(c.dirs.values())[-1]
        assert int(ints[:n_blocks].sum()) == last.records and int(ints[2 * n_blocks]) == last.records      # count[], start[n_blocks]
        records = work[head:].view(torch.int32).view(-1, 8)
        written = int((records[:, 7] == 0).sum())                           # (a record's last word is written as 0.f; prefill: -1)
        assert written == max(d.records for d in c.dirs.values())
    elif work is not None:
        assert bool((work == 0xFF).all()), "a downgraded workspace was written"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", OVERFLOW_SHAPES, ids=str)
def test_hip_splat_record_overflow_matches_float64(shape, hip_lib):
    """Workspaces that hold 1, half, all but one and exactly all of the far records: what does not fit goes through the atomics of
    splat_bin_kernel, the gather stops at the capacity, and no record is used by both."""
    c = splat_case(*shape)
    head = work_head_bytes(*shape)
    for name, d in c.dirs.items():
        atomic = _nan_accum(c)[0]
        _splat(c, d, atomic, None)
        for capacity in overflow_capacities(d.records):
            accum = _nan_accum(c)[0]
            _splat(c, d, accum, _ff_bytes(head + 32 * capacity))
            torch.cuda.synchronize()
            _check_accum(f"{shape} {name} capacity {capacity} of {d.records}", accum, d, other=atomic)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["full", "none"])
def test_hip_splat_frame_of_more_than_max_tiles(variant, hip_lib):
    """7 x 512 = 3584 tiles > SPLAT_MAX_TILES: the host must drop the workspace (the kernels' LDS histogram has 3072 entries) and
    the far samples take the atomic route; the workspace handed over stays untouched."""
    from nsff_pl_amd import _lib
    W, H, S = TALL_SHAPE
    c = tall_case()
    d = c.dirs["fw"]
    work = _ff_bytes(_lib.splat_work_bytes(H, W, S)) if variant == "full" else None
    accum = _nan_accum(c)[0]
    _splat(c, d, accum, work)
    torch.cuda.synchronize()
    _check_accum(f"{TALL_SHAPE} {variant}", accum, d)
    if work is not None:
        assert bool((work == 0xFF).all()), "workspace written on a frame of more than MAX_TILES tiles"


@pytest.mark.gpu
@pytest.mark.parametrize("S", COMPOSITE_S)
def test_hip_mpi_composite_matches_float64(S, hip_lib):
    """21 pixels (not a multiple of the 4 wavefronts of a workgroup), plane counts on both sides of the 64-plane chunk, ragged last
    chunks, norm-0 cells, opaque planes at the chunk seam.  What lies behind a fully opaque plane contributes exactly 0: replacing
    it leaves those pixels bit-identical."""
    from nsff_pl_amd import _lib
    case, c = composite_case(S), composite_inputs(S)
    h, w = COMPOSITE_HW

    def run(fw, bw, s_rgb, s_a, zs, dt):
        rgb = torch.full((h, w, 3), float("nan"), device=DEV)
        depth = torch.full((h, w), float("nan"), device=DEV)
        _lib.mpi_composite(h, w, S, dt, _dev(fw), _dev(bw), _dev(s_rgb), _dev(s_a), _dev(zs), rgb, depth)
        return rgb.cpu().numpy().reshape(-1, 3), depth.cpu().numpy().reshape(-1)
    rng = np.random.RandomState(7)
    behind = np.zeros((c.n, S), bool)
    for pix, at in c.opaque.items():
        behind[pix, at + 1:] = True
    fw2, bw2, s_rgb2, s_a2, zs2 = (x.copy() for x in (c.fw, c.bw, c.s_rgb, c.s_a, c.zs))
    for x in (fw2, bw2):
        x[behind] = 0
        x[behind, :5] = rng.uniform(0.5, 2.0, (int(behind.sum()), 5))
    s_rgb2[behind], s_a2[behind], zs2[behind] = 0.9, 0.7, 0.5
    for dt in COMPOSITE_DTS:
        got = run(c.fw, c.bw, c.s_rgb, c.s_a, c.zs, dt)
        errs = [parity.max_rel_err(g, r) for g, r in zip(got, case.refs[dt])]
        print(f"S={S} dt={dt}: GPU - float64 rgb {errs[0]:.3e} depth {errs[1]:.3e}, bound {case.bound:.3e}")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert max(errs) <= case.bound, (S, dt, errs, case.bound)
        again = run(fw2, bw2, s_rgb2, s_a2, zs2, dt)
        pix = sorted(c.opaque)
        assert np.array_equal(got[0][pix], again[0][pix]) and np.array_equal(got[1][pix], again[1][pix])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(40, 24, 130), (24, 16, 256)], ids=str)
def test_hip_interpolate_above_64_planes_matches_oracle(shape, hip_lib):
    W, H, S = shape
    res_t, res_tp1, dt, K, c2w, wh, _ = multi_tile_case(W, H, S)
    with np.errstate(all="ignore"):
        o_rgb, o_depth = orc.interpolate(res_t, res_tp1, dt, K, c2w, wh)
    g_rgb, g_depth = A.interpolate({k: torch.from_numpy(v).to(DEV) for k, v in res_t.items()},
                                   {k: torch.from_numpy(v).to(DEV) for k, v in res_tp1.items()}, dt, K, c2w, wh)
    assert np.abs(o_rgb).max() > 0.3
    parity.assert_close(f"rgb {shape}", g_rgb.cpu().numpy(), o_rgb, parity.RTOL)
    parity.assert_close(f"depth {shape}", g_depth.cpu().numpy(), o_depth, parity.RTOL)
    bad = (np.abs(g_rgb.cpu().numpy() - o_rgb).max(-1) > 1e-4 * np.abs(o_rgb).max()).sum()
    assert bad == 0, f"{bad} pixels differ"
