"""GPU checks of the scene scale (csrc/scale.hip behind nsff_pl_amd/scene.py) on the cases of golden g29, against the numpy
restatement tests/scene_numpy.py (itself checked against the reference's numbers in test_scene_scale_host.py).

Selections, pixel indices and counts are exact, so they are compared bit for bit -- the depths too, the projection being the same
fma chains on both sides.  Means and centred moments: a sum of at most 700 fp64 terms, each rounded once, is within
700 * 1.1e-16 ~ 8e-14 of the exact sum relative to the sum of the terms' magnitudes, on either side; the bound is 1e-12 of that
sum.  nearest_depth and the candidates against the restatement: 1e-12 relative, same branch.  Against the golden (the reference
with scipy's float32 mean of y) the bound is the measured deviation of test_scene_scale_host.py, 4 x 2.28e-8.
"""
import os

import numpy as np
import pytest
import torch

import scene_numpy as sn
from nsff_pl_amd import _lib, scene, frames, RayBank

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("c0", "c1", "c2", "c3", "c4", "c4b")
F32MEAN_BOUND = 4 * 2.28e-8                     # test_scene_scale_host.py: measured on g29, times 4


@pytest.fixture(scope="module")
def g29():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g29_scene_scale.npz")))


@pytest.fixture(scope="module")
def restated(g29):
    return {c: sn.nearest_depth(*(g29[f"{c}/{k}"] for k in ("K", "w2c", "points", "vis", "disps"))) for c in CASES}


@pytest.fixture(scope="module")
def computed(g29):
    """case -> (nearest_depth, table) of the package, computed once"""
    out = {}
    for c in CASES:
        G = lambda k: g29[f"{c}/{k}"]
        out[c] = scene.nearest_depth(G("K"), G("w2c"), G("points"), G("vis"), torch.from_numpy(G("disps")).cuda(), return_table=True)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("case", CASES)
def test_case_matches_the_restatement(g29, restated, computed, case):
    nd, t = computed[case]
    want_nd, frs = restated[case]
    for f, fr in enumerate(frs):
        assert np.array_equal(t["pix"][f], fr["pix"])
        assert t["n_vis"][f] == fr["n_vis"]
        assert np.array_equal(_bits(t["disp_os"][f]), _bits(fr["disp_os"])), (t["disp_os"][f], fr["disp_os"])
        assert np.array_equal(_bits(t["depth_os"][f]), _bits(fr["depth_os"])), (t["depth_os"][f], fr["depth_os"])
        assert _bits(t["p95_disp"][f:f + 1])[0] == _bits(np.array([fr["p95_disp"]]))[0] and t["p5_depth"][f] == fr["p5_depth"]
        for k in ("mean_x", "mean_y", "sxx", "sxy", "syy"):
            err = abs(t[k][f] - fr[k])
            print(f"{case} frame {f} {k}: |diff| {err:.2e}, bound {1e-12 * fr['abs_terms'][k]:.2e}")
            assert err <= 1e-12 * fr["abs_terms"][k], k
        assert bool(t["used_regression"][f]) == bool(fr["used_regression"])
        assert abs(t["candidate"][f] - fr["candidate"]) <= 1e-12 * abs(fr["candidate"])
    assert abs(nd - want_nd) <= 1e-12 * abs(want_nd)
    golden = float(g29[f"{case}/nearest_depth"])
    print(f"{case}: nearest_depth {nd!r}, golden {golden!r}, rel {abs(nd - golden) / golden:.2e}")
    assert abs(nd - golden) <= F32MEAN_BOUND * golden


def _raw(g29, case, frames_=None, work=None):
    """nsff_scene_scale on a case (or some of its frames): the four tables as numpy arrays"""
    G = lambda k: g29[f"{case}/{k}"]
    sel = slice(None) if frames_ is None else frames_
    disps = torch.from_numpy(np.ascontiguousarray(G("disps")[sel])).cuda()
    F, H, W = disps.shape
    lo, hi, _ = scene.percentile_ranks(H * W, 95, np.float32)
    out = _lib.scene_scale(torch.from_numpy(G("points")).cuda(), torch.from_numpy(np.ascontiguousarray(G("vis")[sel])).cuda(),
                           torch.from_numpy(np.ascontiguousarray(G("w2c")[sel][:, :3])).cuda(), torch.from_numpy(G("K")).cuda(),
                           disps, (lo, hi), want_pix=True, work=work)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("case", ("c0", "c1", "c2"))
def test_a_frame_alone_gives_its_batch_bits(g29, case):
    batch = _raw(g29, case)
    for f in range(batch[0].shape[0]):
        alone = _raw(g29, case, slice(f, f + 1))
        for a, b in zip(alone, batch):
            assert a[0].tobytes() == b[f].tobytes()


def test_two_calls_on_one_workspace_agree(g29):
    """The second call finds the workspace as the first left it; a third finds it filled with ones: tickets and histograms are
    cleared by the call itself."""
    F, W, H, N = 3, 67, 31, 700
    work = torch.empty(_lib.scene_scale_work_bytes(F, N, H, W), dtype=torch.uint8, device="cuda")
    first = _raw(g29, "c1", work=work)
    second = _raw(g29, "c1", work=work)
    work.fill_(0xFF)
    third = _raw(g29, "c1", work=work)
    fresh = _raw(g29, "c1")
    for a, b, c, d in zip(first, second, third, fresh):
        assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()
    assert int(work[:16].view(torch.int32)[:F].abs().sum()) == 0                 # the frame tickets are back at zero


def test_zeros_at_the_selected_ranks_come_back_positive(g29):
    """-0 ranks as +0 and the order statistic comes back as +0: 20 zeros of both signs cover the ranks 398 and 399 of 420 values
    (390 negative ones below them, 10 positive above).  With them ranked by their bits the -0.0 would sort below the +0.0 -- and
    next to the negative values -- and one of them would come back as it is."""
    G = lambda k: g29[f"c3/{k}"]
    rng = np.random.default_rng(3)
    vals = np.concatenate([-rng.uniform(0.1, 5.0, 390), np.where(np.arange(20) % 2 == 0, -0.0, 0.0), rng.uniform(0.1, 5.0, 10)])
    disps = torch.from_numpy(rng.permutation(vals).astype(np.float32).reshape(1, 20, 21)).cuda()
    lo, hi, _ = scene.percentile_ranks(420, 95, np.float32)
    assert (lo, hi) == (398, 399)
    for ranks, want in (((398, 399), (0.0, 0.0)), ((390, 409), (0.0, 0.0)), ((389, 410), None)):
        _, disp_os, _, _ = _lib.scene_scale(torch.from_numpy(G("points")).cuda(), torch.from_numpy(G("vis")).cuda(),
                                            torch.from_numpy(np.ascontiguousarray(G("w2c")[:, :3])).cuda(), torch.from_numpy(G("K")).cuda(),
                                            disps, ranks)
        got = disp_os.cpu().numpy()[0]
        if want is None:                                                           # the neighbours of the run of zeros
            srt = np.sort(vals.astype(np.float32))
            assert got[0] == srt[389] < 0 and got[1] == srt[410] > 0
        else:
            assert _bits(got).tolist() == [0, 0], got                              # +0.0, not -0.0
    want95, _, _, lo_v, hi_v = sn.percentile_linear(disps.cpu().numpy(), 95)
    assert _bits(np.array([lo_v, hi_v])).tolist() == [0, 0] and want95 == 0.0


def test_scene_from_colmap_gives_the_reference_poses(g29):
    G = lambda k: g29[f"c1/{k}"]
    F, W, H, N = 3, 67, 31, 700
    disps = torch.from_numpy(G("disps")).cuda()
    vis = scene.visibility_matrix(G("point_index"), G("image_id"), N, G("start_end"))
    d = scene.scene_from_colmap(G("K"), (W, H), (W, H), G("w2c"), G("points"), vis, disps)
    golden = float(G("nearest_depth"))
    assert abs(d["nearest_depth"] - golden) <= F32MEAN_BOUND * golden
    assert d["poses"].shape == (F, 3, 4) and d["poses"].dtype == np.float64
    # only the translations carry the scale: t / s, so |d t| <= bound * |t|; the rotations are the reference's to rounding
    assert np.abs(d["poses"][..., :3] - G("poses")[..., :3]).max() <= 1e-12
    assert np.abs(d["poses"][..., 3] - G("poses")[..., 3]).max() <= F32MEAN_BOUND * np.abs(G("poses")[..., 3]).max() + 1e-12
    # Ps = K [R | -R t / s] in fp32: the same relative bound on its last column, plus the fp32 rounding of two float64 formulas
    Ps = d["Ps"][0].numpy()
    assert np.abs(Ps - G("Ps")).max() <= (F32MEAN_BOUND + 2 ** -22) * np.abs(G("Ps")).max()
    assert torch.equal(d["Ks"][0], torch.from_numpy(G("K"))) and torch.equal(d["K"], torch.from_numpy(G("K")))
    # ... and the ray bank takes the result as it is
    images = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device="cuda")
    masks = torch.ones(F, H, W, dtype=torch.uint8, device="cuda")
    bank = RayBank.from_frames(d["K"], d["poses"], images, disps, masks, None, None, (W, H))
    assert bank.records.shape == (F, H * W, _lib.RAY_RECORD) and bool(torch.isfinite(bank.records).all())
    assert torch.equal(bank.Ps.cpu(), d["Ps"]) and bank.sample(16)["rays"].shape == (16, 6)


def test_native_size_disparities_are_resized_first(g29):
    G = lambda k: g29[f"c0/{k}"]
    rng = np.random.default_rng(7)
    native = torch.from_numpy(rng.uniform(0.1, 0.7, (3, 53, 91)).astype(np.float32)).cuda()
    nd, t = scene.nearest_depth(G("K"), G("w2c"), G("points"), G("vis"), native, img_wh=(40, 24), return_table=True)
    nd2, t2 = scene.nearest_depth(G("K"), G("w2c"), G("points"), G("vis"), frames.resize_disps(native, (40, 24)), return_table=True)
    assert nd == nd2
    for k in t:
        assert np.asarray(t[k]).tobytes() == np.asarray(t2[k]).tobytes(), k
    want, _ = sn.nearest_depth(G("K"), G("w2c"), G("points"), G("vis"), frames.resize_disps(native, (40, 24)).cpu().numpy())
    assert abs(nd - want) <= 1e-12 * abs(want)


def test_refusals_on_the_device(g29):
    """The reference's own failures, by name.  An identity camera keeps the arithmetic exact: c = p and depth = p.z, so equal
    z give bit-identical 1/depth (mean-centred sum exactly 0) and z = 0 a division by zero."""
    K, vis = g29["c3/K"], g29["c3/vis"]
    disps = torch.from_numpy(g29["c3/disps"]).cuda()
    w2c = np.eye(4)[None]
    rng = np.random.default_rng(11)
    pts = np.stack([rng.uniform(-1.5, 1.5, 64), rng.uniform(-1.5, 1.5, 64), rng.uniform(3.0, 8.0, 64)], 1)
    assert np.isfinite(scene.nearest_depth(K, w2c, pts, vis, disps))
    one = np.zeros_like(vis)
    one[0, 5] = 1
    with pytest.raises(ValueError, match="frame 0 has 1 visible points"):
        scene.nearest_depth(K, w2c, pts, one, disps)
    flat = pts.copy()
    flat[:, 2] = 4.0
    with pytest.raises(ValueError, match="all 1/depth values of frame 0 are identical"):
        scene.nearest_depth(K, w2c, flat, vis, disps)
    nan = disps.clone()
    nan[0, 3, 4] = float("nan")
    with pytest.raises(ValueError, match="frame 0 has 1 NaN disparities"):
        scene.nearest_depth(K, w2c, pts, vis, nan)
    plane = pts.copy()
    plane[int(np.flatnonzero(vis[0])[0]), 2] = 0.0                              # in the camera's plane: pix -2
    with pytest.raises(ValueError, match="frame 0 has 1 visible points whose projection is not finite"):
        scene.nearest_depth(K, w2c, plane, vis, disps)
