"""The sampling chain (coarse_samples_kernel, sample_pdf_kernel, fine_samples_kernel of csrc/rays.hip, the fused coarse depths of
csrc/rng.hip) and the stand-alone geometry stages (nsff_frustum_visibility, nsff_warp_points), called directly through `_lib`, on
the routes the golden scenes never reach: more than 64 interior bins (the CDF's carry across 64-bin chunks), merged depth counts
that are no multiple of 4 (the scalar tail of the rank loop, the placement of `merged` behind S + 3 & ~3 bins), exact ties in the
merge, NULL sample outputs, draws of more than one grid-stride pass, several training cameras, frames outside the camera table,
point counts around the 256-thread block, the strict zs > z_far.

References: tests/sampling_numpy.py -- float64 restatements under parity.sample_tolerance (its constants as they are) where the
operation is ill-conditioned, fp32 restatements bit for bit where it is one rounding per operation.  tests/test_sampling_host.py
shows on the CPU that the inputs (tests/sampling_cases.py) meet the conditions these comparisons rest on and that a dropped carry /
an unstable rank would fail them.  Every output is NaN before the launch and carries one spare row that must stay NaN.
These kernels do not depend on the field precision: nothing here is parametrised over it.
"""
import numpy as np
import pytest
import torch

import common
import parity
import sampling_cases as SC
import sampling_numpy as SN
import scenes
import nsff_pl_amd as A
from nsff_pl_amd import _lib, ray_geometry

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FORMS = ("shared", "per_ray")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in tensors)


# ---- nsff_sample_pdf ----
def _sample_pdf(bins, weights, u, per_ray, n_imp):
    """-> (n, n_imp) samples; the output has a spare row behind the last ray, which no wave may write"""
    n = weights.shape[0]
    out = _nan(n + 1, n_imp)
    _lib.sample_pdf(_dev(bins), _dev(weights), _dev(u), per_ray, SC.EPS, out[:n])
    assert _untouched(out[n:]), "a wave without a ray wrote samples"
    return out[:n].cpu().numpy()


@pytest.mark.parametrize("M", SC.PDF_M)
def test_hip_sample_pdf_matches_float64(M, hip_lib):
    """M on both sides of the 64-bin chunk (1, 63, 64, 65, 128, 129, 191, 257), ray counts that leave waves of the last workgroup
    idle, n_imp on both sides of a wave, u shared (0 and 1 included) and per ray: every sample inside parity.sample_tolerance of
    the float64 draw"""
    worst, used, equal, total = -np.inf, 0.0, 0, 0
    for n_rays in SC.PDF_RAYS:
        for n_imp in SC.PDF_IMP:
            c = SC.pdf_case(M, n_rays, n_imp)
            for form in FORMS:
                want, tol = SC.pdf_reference(M, n_rays, n_imp, form)
                got = _sample_pdf(c.bins, c.weights, c.u[form], form == "per_ray", n_imp)
                assert np.isfinite(got).all(), (M, n_rays, n_imp, form)
                err = np.abs(got - want)
                worst, used = max(worst, float((err - tol).max())), max(used, float((err / tol).max()))
                twin = SN.sample_pdf32_scan(c.bins, c.weights, c.u[form], SC.EPS, search="bisect")
                equal += int((got.view(np.int32) == twin.view(np.int32)).sum())
                total += got.size
                parity.assert_samples_close(f"M={M} n_rays={n_rays} n_imp={n_imp} {form}", got, want, tol)
    print(f"pdf M={M}: worst excess {worst:.3e} ({100 * used:.3f} % of the tolerance used); {equal} of {total} samples have the "
          "bits of the fp32 restatement")


# ---- nsff_fine_samples ----
def _fine(c, form, keep=True):
    """one nsff_fine_samples call on case c -> samples per set (None when not kept), zs_fine, xyz_fine as numpy; every output has a
    spare ray that must stay NaN"""
    n, per_ray = SC.FINE_RAYS, form == "per_ray"
    samples = [_nan(n + 1, c.n_imp) if keep and k < c.sets else None for k in range(2)]
    zs_fine, xyz_fine = _nan(n + 1, c.Sf), _nan(n + 1, c.Sf, 3)
    w = [_dev(c.w[k]) if k < c.sets else None for k in range(2)]
    u = [_dev(c.u[form][k]) if k < c.sets else None for k in range(2)]
    _lib.fine_samples(_dev(c.rays), _dev(c.z_lin), _dev(c.zs_coarse), c.n_imp, w[0], w[1], u[0], u[1], per_ray,
                      None if samples[0] is None else samples[0][:n], None if samples[1] is None else samples[1][:n],
                      zs_fine[:n], xyz_fine[:n])
    assert _untouched(zs_fine[n:], xyz_fine[n:], *[s[n:] for s in samples if s is not None]), "written behind the last ray"
    return [None if s is None else s[:n].cpu().numpy() for s in samples], zs_fine[:n].cpu().numpy(), xyz_fine[:n].cpu().numpy()


def _check_merge(what, c, samples, zs_fine, xyz_fine):
    """assertions 3 and 4: zs_fine is the sort of the coarse depths and the kernel's own samples, xyz_fine is o + (d * z)"""
    assert not np.isnan(zs_fine).any() and not np.isnan(xyz_fine).any(), f"{what}: slots left unwritten"
    merged = np.concatenate([c.zs_coarse] + [s for s in samples[:c.sets]], 1)
    assert _same_bits(zs_fine, np.sort(merged, 1)), f"{what}: zs_fine is not sort(cat(zs_coarse, samples))"
    assert _same_bits(xyz_fine, SN.points32(c.rays, zs_fine)), f"{what}: xyz_fine is not o + d * zs_fine"


@pytest.mark.parametrize("S,n_imp,sets", SC.FINE_TABLE)
def test_hip_fine_samples_routes(S, n_imp, sets, hip_lib):
    """SC.FINE_TABLE: M = 1, the goldens' shape, scalar tails of 2 and 1 in the rank loop, M = 63 / 64 / 65 / 126 / 128 / 255"""
    c = SC.fine_case(S, n_imp, sets)
    worst, used = -np.inf, 0.0
    for form in FORMS:
        what = f"S={S} n_imp={n_imp} sets={sets} {form}"
        refs, tols, zs64 = SC.fine_reference(S, n_imp, sets, form)
        samples, zs_fine, xyz_fine = _fine(c, form)
        for k in range(sets):
            assert np.isfinite(samples[k]).all(), what
            err = np.abs(samples[k] - refs[k])
            worst, used = max(worst, float((err - tols[k]).max())), max(used, float((err / tols[k]).max()))
            parity.assert_samples_close(f"{what} set {k}", samples[k], refs[k], tols[k])                      # 1
            direct = _sample_pdf(c.mids, c.w[k][:, 1:-1], c.u[form][k], form == "per_ray", n_imp)
            assert _same_bits(samples[k], direct), f"{what} set {k}: not nsff_sample_pdf's bits"              # 2
        _check_merge(what, c, samples, zs_fine, xyz_fine)                                                     # 3, 4
        tol = np.max([t.max(1) for t in tols], 0)[:, None]
        parity.assert_samples_close(f"{what} zs_fine", zs_fine, zs64, tol)
        none, zs_again, xyz_again = _fine(c, form, keep=False)                                                # 5
        assert none == [None, None]
        assert _same_bits(zs_again, zs_fine) and _same_bits(xyz_again, xyz_fine), f"{what}: NULL sample outputs change the merge"
    print(f"fine S={S} n_imp={n_imp} sets={sets}: worst excess {worst:.3e} ({100 * used:.3f} % of the tolerance used)")


@pytest.mark.parametrize("S,n_imp,sets", SC.TIE_TABLE)
def test_hip_fine_samples_breaks_ties_stably(S, n_imp, sets, hip_lib):
    """exact ties in the merge -- all coarse depths one number, n_imp exact pairs of static and transient samples, a coarse depth
    equal to the u = 0 sample of both sets: every slot is written once (an unstable tie-break leaves NaN, test_sampling_host.py)"""
    c = SC.fine_case(S, n_imp, sets, ties=True)
    for form in FORMS:
        samples, zs_fine, xyz_fine = _fine(c, form)
        if form == "shared":
            assert _same_bits(samples[0][SC.TIE_ZERO], samples[1][SC.TIE_ZERO])
            assert samples[0][SC.TIE_EDGE, 0] == samples[1][SC.TIE_EDGE, 0] == c.zs_coarse[SC.TIE_EDGE, SC.TIE_EDGE_AT]
        _check_merge(f"ties S={S} n_imp={n_imp} {form}", c, samples, zs_fine, xyz_fine)
        _, zs_again, xyz_again = _fine(c, form, keep=False)
        assert _same_bits(zs_again, zs_fine) and _same_bits(xyz_again, xyz_fine)


# ---- nsff_coarse_samples, stand-alone and fused into the draw ----
@pytest.mark.parametrize("S", SC.COARSE_S)
def test_hip_coarse_samples_match_fp32(S, hip_lib):
    for n_rays in SC.COARSE_RAYS:
        c = SC.coarse_case(S, n_rays)
        for perturb in SC.COARSE_PERTURB:
            zs, xyz = _nan(n_rays + 1, S), _nan(n_rays + 1, S, 3)
            _lib.coarse_samples(_dev(c.rays), _dev(c.z_lin), perturb, _dev(c.rnd) if perturb > 0 else None, zs[:n_rays], xyz[:n_rays])
            assert _untouched(zs[n_rays:], xyz[n_rays:])
            want_zs, want_xyz = SN.coarse32(c.rays, c.z_lin, perturb, c.rnd)
            assert _same_bits(zs[:n_rays].cpu().numpy(), want_zs), (S, n_rays, perturb)
            assert _same_bits(xyz[:n_rays].cpu().numpy(), want_xyz), (S, n_rays, perturb)


def _rng_grid():
    """blocks of torch's (and nsff_rng_draws') launch geometry on this device, as `_lib.fused_draws` derives them"""
    _lib.fused_draws([("rand", (1,))], DEV)
    return _lib._DEVICE_RNG_GEOMETRY[DEV.index]


@pytest.mark.parametrize("shape", [(5, 3), (300, 65), (1024, 64), "above one pass"], ids=str)
def test_hip_fused_coarse_depths_equal_the_separate_launches(shape, hip_lib):
    """nsff_rng_draws_coarse against torch.rand + nsff_coarse_samples from the same generator state: the same depths and points bit
    for bit, the generator left in the same state, with the draw kept and with the draw consumed by the launch alone; the last
    shape has more elements than one grid-stride pass (1024 x grid) of the draw's geometry"""
    grid = _rng_grid()
    if shape == "above one pass":
        shape = (1024 * grid // 64 + 232, 64)
        assert shape[0] * shape[1] > 1024 * grid
    else:
        assert shape[0] * shape[1] <= 1024 * grid
    n_rays, S = shape
    print(f"fused coarse depths {shape}: {n_rays * S} elements, one grid-stride pass of {grid} blocks is {1024 * grid}")
    rays, z_lin = scenes.synthetic_rays(n_rays, 9)[0].to(DEV), torch.linspace(0, 1, S, device=DEV)
    for perturb in (0.5, 1.0):
        torch.manual_seed(4242)
        torch.rand(3, device=DEV)
        rnd = torch.rand(n_rays, S, device=DEV)
        after = torch.rand(4, device=DEV)
        want_zs, want_xyz = _nan(n_rays, S), _nan(n_rays, S, 3)
        _lib.coarse_samples(rays, z_lin, perturb, rnd, want_zs, want_xyz)
        for keep in (True, False):
            torch.manual_seed(4242)
            torch.rand(3, device=DEV)
            zs, xyz = _nan(n_rays, S), _nan(n_rays, S, 3)
            outs = _lib.fused_draws([("rand", (n_rays, S))], DEV, [keep], coarse=(rays, z_lin, perturb, zs, xyz))
            assert torch.equal(after, torch.rand(4, device=DEV)), "the generator is not where torch.rand leaves it"
            assert (outs[0] is not None) == keep
            if keep:
                assert torch.equal(outs[0].view(torch.int32), rnd.view(torch.int32))
            assert torch.equal(zs.view(torch.int32), want_zs.view(torch.int32)), (shape, perturb, keep)
            assert torch.equal(xyz.view(torch.int32), want_xyz.view(torch.int32)), (shape, perturb, keep)
    # the stand-alone launch this was compared with is itself the fp32 restatement's (a few rows of it, checked on the host)
    rows = slice(0, min(n_rays, 64))
    zs32, xyz32 = SN.coarse32(rays[rows].cpu().numpy(), z_lin.cpu().numpy(), 1.0, rnd[rows].cpu().numpy())
    assert _same_bits(want_zs[rows].cpu().numpy(), zs32) and _same_bits(want_xyz[rows].cpu().numpy(), xyz32)


# ---- refusals ----
def test_hip_sampling_entry_points_refuse_what_they_cannot_run(hip_lib):
    """NSFF_ERR_INVALID, and nothing written: fewer than 3 coarse depths, no importance sample, no bin, a shape whose scratch
    exceeds 64 KB of LDS.  No ray at all is not an error."""
    n = 3

    def fine(S, n_imp, n_rays=n):
        outs = [_nan(n, max(n_imp, 1)), _nan(n, max(n_imp, 1)), _nan(n, S + 2 * max(n_imp, 1)), _nan(n, S + 2 * max(n_imp, 1), 3)]
        args = (_dev(np.zeros((n_rays, 6))), torch.linspace(0, 1, S, device=DEV), _dev(np.zeros((n_rays, S))), n_imp,
                _dev(np.ones((n_rays, S))), _dev(np.ones((n_rays, S))), _dev(np.zeros(max(n_imp, 1))), _dev(np.zeros(max(n_imp, 1))), 0)
        return args, outs

    for S, n_imp in ((2, 4), (1, 4), (8, 0), (8, -1), (3000, 1)):
        args, outs = fine(S, n_imp)
        with pytest.raises(RuntimeError, match="nsff_fine_samples failed: NSFF_ERR_INVALID"):
            _lib.fine_samples(*args, *outs)
        assert _untouched(*outs), (S, n_imp)
    args, outs = fine(8, 4, n_rays=0)
    _lib.fine_samples(*args, *outs)
    assert _untouched(*outs)

    def pdf(M, n_imp, n_rays=n):
        out = _nan(n, n_imp)
        return (_dev(np.zeros((n_rays, M + 1))), _dev(np.ones((n_rays, M))), _dev(np.zeros(max(n_imp, 1))), 0, SC.EPS, out[:n_rays]), out

    for M, n_imp in ((0, 4), (8, 0), (4096, 4)):                 # 4 waves x (M + 1) floats: 4096 bins are 16 bytes above 64 KB
        args, out = pdf(M, n_imp)
        with pytest.raises(RuntimeError, match="nsff_sample_pdf failed: NSFF_ERR_INVALID"):
            _lib.sample_pdf(*args)
        assert _untouched(out), (M, n_imp)
    args, out = pdf(8, 4, n_rays=0)
    _lib.sample_pdf(*args)
    assert _untouched(out)
    args, out = pdf(4095, 4)                                    # exactly 64 KB: runs
    _lib.sample_pdf(*args)
    assert bool(torch.isfinite(out).all())


# ---- nsff_frustum_visibility ----
def _ts(frame):
    return torch.full((4,), frame, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("n_cams", SC.VIS_CAMS)
def test_hip_training_view_visibility_matches_float64(n_cams, hip_lib):
    """one and three training cameras, the first and the last frame of the table, point counts around the 256-thread block: the
    count equals the float64 frustum_count on every point that is not within fp32 reach of a decision boundary (at most 2 % are,
    test_sampling_host.py); a frame outside the table is seen by no camera; no point gives an empty tensor"""
    ds = SC.VisDataset(n_cams)
    for frame in SC.vis_frames(ds.N_frames):
        c = SC.vis_case(n_cams, frame)
        assert c.undecided.mean() <= 0.02
        for P in SC.VIS_P:
            got = ray_geometry.training_view_visibility(_dev(c.points[:P]), ds, _ts(frame)).cpu().numpy()
            assert got.shape == (P,) and np.isfinite(got).all()
            keep = ~c.undecided[:P]
            wrong = int((got[keep] != c.counts[:P][keep]).sum())
            print(f"n_cams={n_cams} frame={frame} P={P}: {wrong} wrong of {int(keep.sum())} decided, "
                  f"{int((got[~keep] != c.counts[:P][~keep]).sum())} of {int((~keep).sum())} undecided differ")
            assert wrong == 0
            assert ((got[~keep] >= 0) & (got[~keep] <= n_cams)).all()
    for frame in (-1, ds.N_frames):
        got = ray_geometry.training_view_visibility(_dev(SC.vis_points()), ds, _ts(frame))
        assert got.shape == (1000,) and not bool(got.any())
    empty = ray_geometry.training_view_visibility(torch.empty(0, 3, device=DEV), ds, _ts(0))
    assert empty.shape == (0,) and empty.is_cuda


def test_hip_visibility_counts_are_the_composites_inline_mask(hip_lib):
    """the g5 scene rendered with dataset= (one training camera): where the stand-alone stage counts no camera for a sample point
    of the render, the composite has put the dynamic density to softplus(-10); where it counts one, the coarse density is what
    the render without dataset= gives (the coarse points are the same in both renders)"""
    cfg, meta, rays, ts, models, emb, dataset, _ = common.build_case("g5_nsff_test_vis", A.NeRF, A.PosEmbedding)
    for m in models.values():
        m.to(DEV)
    emb["t"].to(DEV)

    def render(ds):
        with torch.no_grad():
            return A.render_rays(models, emb, rays.to(DEV), ts.to(DEV), scenes.N_FRAMES - 1, cfg["N_samples"], 0, 0,
                                 cfg["N_importance"], 1024 * 32, test_time=True, **scenes.render_kwargs(cfg, ds))
    masked, plain = render(dataset), render(None)
    floor = float(np.log1p(np.exp(-10.0)))
    for typ in ("coarse", "fine"):
        pts = masked[f"xyzs_{typ}"].reshape(-1, 3)
        count = ray_geometry.training_view_visibility(pts, dataset, ts.to(DEV)).reshape(masked[f"transient_sigmas_{typ}"].shape)
        sig = masked[f"transient_sigmas_{typ}"]
        hidden = count == 0
        assert bool(hidden.any()) and bool((~hidden).any())
        values = torch.unique(sig[hidden])
        assert values.numel() == 1 and abs(float(values[0]) - floor) <= 1e-6 * floor, values
        assert not bool((sig[~hidden] == values[0]).any())
        if typ == "coarse":
            assert torch.equal(masked["xyzs_coarse"], plain["xyzs_coarse"])
            assert torch.equal(sig[~hidden], plain["transient_sigmas_coarse"][~hidden])


# ---- nsff_warp_points ----
@pytest.mark.parametrize("P", SC.WARP_P)
def test_hip_warp_points_match_fp32(P, hip_lib):
    """3 P on both sides of a 256-thread block; depths exactly z_far (the flow is added) and one float above (unchanged)"""
    c = SC.warp_case(P, _lib.RAW_STRIDE)
    fw, bw = _nan(P + 1, 3), _nan(P + 1, 3)
    _lib.warp_points(_dev(c.raw), _dev(c.xyz), _dev(c.zs), SC.WARP_Z_FAR, fw[:P], bw[:P])
    assert _untouched(fw[P:], bw[P:])
    want_fw, want_bw = SN.warp32(c.raw, c.xyz, c.zs, SC.WARP_Z_FAR)
    assert _same_bits(fw[:P].cpu().numpy(), want_fw) and _same_bits(bw[:P].cpu().numpy(), want_bw)
