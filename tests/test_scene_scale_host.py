"""Host checks (no GPU) of the scene scale: the numpy restatement tests/scene_numpy.py against golden g29 (the reference's own
statements of datasets/monocular.py:85-132 with scipy's linregress and numpy's percentile, tests/golden/make_golden_scene.py);
scene.py's host arithmetic (regression table, percentile ranks, poses) against both; visibility_matrix against the reference's
loop; the header / symbol contract; nsff_scene_scale's argument validation (no launch) and the Python layer's refusals.

The float32-mean deviation.  scipy forms ymean = np.mean(y) in y's float32; the restatement and scene.py use float64.  Measured
on g29, |nearest_depth_fp64 - golden| / golden: c0 1.77e-8, c1 0 (the minimum comes from the depth-percentile branch), c2 2.28e-8,
c3 1.11e-8, c4 9.5e-9, c4b 1.2e-16; the intercepts differ by 1.0e-8 .. 2.2e-7 relative.  The bound below is 4 x the largest
(other seeds' rounding), capped at 1e-5 so that it cannot hide a wrong pixel or rank (one wrong gather among 300 moves the slope
by about 1e-3).  With scipy's float32 mean restated (f32mean=True) the restatement gives the golden's number to 1e-15.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import scene_numpy as sn
from nsff_pl_amd import _lib, scene, frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g29_scene_scale.npz")
CASES = dict(c0=(3, 40, 24, 300), c1=(3, 67, 31, 700), c2=(2, 40, 24, 300), c3=(1, 21, 20, 64), c4=(1, 41, 1, 64),
             c4b=(1, 41, 1, 64))                                                  # F, W, H, N
MEASURED_F32MEAN = 2.28e-8                      # the largest of the figures above
F32MEAN_BOUND = min(4 * MEASURED_F32MEAN, 1e-5)


@pytest.fixture(scope="module")
def g29():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def restated(g29):
    """case -> (nearest_depth, frames) of the restatement, computed once"""
    return {c: sn.nearest_depth(*(g29[f"{c}/{k}"] for k in ("K", "w2c", "points", "vis", "disps"))) for c in CASES}


def test_golden_covers_the_cases(g29):
    assert [str(c) for c in g29["cases"]] == list(CASES)
    assert os.path.getsize(GOLDEN) < 500_000
    for c, (F, W, H, N) in CASES.items():
        assert g29[f"{c}/disps"].shape == (F, H, W) and g29[f"{c}/disps"].dtype == np.float32
        assert g29[f"{c}/vis"].shape == (F, N) and g29[f"{c}/points"].shape == (N, 3) and g29[f"{c}/K"].dtype == np.float32
    r2 = {c: g29[f"{c}/rvalue"] ** 2 for c in CASES}
    assert all(((v < 0.85) | (v > 0.95)).all() for v in r2.values())
    assert (r2["c0"] > 0.95).all() and r2["c1"][1] < 0.85 and r2["c2"][1] == 0.0           # both branches run
    pix, vis = g29["c1/pix"][2], g29["c1/vis"][2] == 1
    u, v = pix[vis] % 67, pix[vis] // 67
    assert (u == 0).any() and (u == 66).any() and (v == 0).any() and (v == 30).any()       # the clip, on every side
    d = g29["c2/disps"][0]
    assert (d == np.round(d)).all() and (d < 0).any() and np.signbit(d[d == 0]).any()
    assert g29["c2/disp_os"][0, 0] == g29["c2/disp_os"][0, 1] == 1500.0 and (d == 1500.0).sum() > 90   # ties across rank lo
    assert (g29["c2/disps"][1] == 7.0).all()
    assert (g29["c4b/vis"] == 1).sum() == 2
    assert sn.percentile_linear(g29["c3/disps"], 95)[1:3] == (398, 399) and sn.percentile_linear(g29["c4/disps"], 95)[1:3] == (38, 39)


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_matches_the_reference(g29, restated, case):
    G = lambda k: g29[f"{case}/{k}"]
    nd, frs = restated[case]
    for f, fr in enumerate(frs):
        assert np.array_equal(fr["pix"], G("pix")[f])
        assert fr["n_vis"] == int((G("vis")[f] == 1).sum())
        assert fr["p95_disp"] == G("p95_disp")[f] and fr["p95_disp"].dtype == np.float32
        assert fr["p5_depth"] == G("p5_depth")[f]
        assert np.array_equal(fr["disp_os"], G("disp_os")[f]) and np.array_equal(fr["depth_os"], G("depth_os")[f])
        assert abs(fr["slope"] - G("slope")[f]) <= 1e-12 * abs(G("slope")[f])
        assert abs(fr["r"] - G("rvalue")[f]) <= 1e-12
        assert fr["used_regression"] == (G("rvalue")[f] ** 2 > 0.9)
        rel = abs(fr["intercept"] - G("intercept")[f]) / abs(G("intercept")[f])
        print(f"{case} frame {f}: intercept fp64 mean vs scipy {rel:.2e}")
        assert abs(fr["intercept_f32mean"] - G("intercept")[f]) <= 1e-12 * abs(G("intercept")[f])
    golden = float(G("nearest_depth"))
    print(f"{case}: |nearest_depth_fp64 - golden| / golden = {abs(nd - golden) / golden:.3e}")
    assert abs(nd - golden) <= F32MEAN_BOUND * golden
    nd32, _ = sn.nearest_depth(G("K"), G("w2c"), G("points"), G("vis"), G("disps"), f32mean=True)
    assert abs(nd32 - golden) <= 1e-12 * golden
    poses, Ps = sn.poses_and_Ps(G("K"), G("w2c"), golden)
    assert np.abs(poses - G("poses")).max() <= 1e-12 and np.abs(Ps - G("Ps")).max() <= 1e-12


@pytest.mark.parametrize("case", list(CASES))
def test_host_arithmetic_of_the_package(g29, restated, case):
    """scene.regression_table on the restatement's moments and order statistics (what the kernels return): the reference's
    slope, r, percentiles, branch and candidates; scene.corrected_poses and projection_matrices: its poses and Ps."""
    G = lambda k: g29[f"{case}/{k}"]
    nd, frs = restated[case]
    F, W, H, N = CASES[case]
    stats = np.array([[fr["n_vis"], 0, fr["mean_x"], fr["mean_y"], fr["sxx"], fr["sxy"], fr["syy"], 0] for fr in frs])
    t = scene.regression_table(stats, np.stack([fr["disp_os"] for fr in frs]), np.stack([fr["depth_os"] for fr in frs]), H * W)
    assert np.array_equal(t["p95_disp"], G("p95_disp")) and t["p95_disp"].dtype == np.float32
    assert np.array_equal(t["p5_depth"], G("p5_depth"))
    assert np.array_equal(t["used_regression"], G("rvalue") ** 2 > 0.9)
    assert np.allclose(t["slope"], G("slope"), rtol=1e-12, atol=0) and np.allclose(t["r"], G("rvalue"), rtol=0, atol=1e-12)
    assert np.abs(t["candidate"] - G("candidate")).max() <= F32MEAN_BOUND * np.abs(G("candidate")).max()
    assert scene.percentile_ranks(H * W, 95, np.float32)[:2] == sn.percentile_linear(G("disps")[0], 95)[1:3]
    golden = float(G("nearest_depth"))
    poses = scene.corrected_poses(G("w2c"), golden)
    assert np.abs(poses - G("poses")).max() <= 1e-12
    Ks, Ps = frames.projection_matrices(G("K"), poses)
    scale = np.abs(G("Ps")).max(axis=(1, 2), keepdims=True)
    assert np.abs(Ps[0].numpy() - G("Ps")).max() <= 2 ** -22 * scale.max()       # fp32 outputs of two float64 formulas
    assert torch.equal(Ks[0], torch.from_numpy(G("K")))


@pytest.mark.skipif(int(np.__version__.split(".")[0]) < 2, reason="np.percentile formed its virtual index differently before "
                    "numpy 2; the restatements follow the numpy 2.x the golden was made with (g29 pins them either way)")
def test_percentile_restatements_are_numpys():
    """Both restatements against np.percentile itself."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 21, 41, 420, 960, 2077, 147456):
        a32 = rng.normal(size=n).astype(np.float32)
        a64 = rng.normal(size=n)
        for a, q in ((a32, 95), (a64, 5), (a32, 5), (a64, 95)):
            want = np.percentile(a, q)
            value, lo, hi, lo_v, hi_v = sn.percentile_linear(a, q)
            assert value == want and value.dtype == want.dtype, (n, q)
            rlo, rhi, g = scene.percentile_ranks(n, q, a.dtype)
            assert (rlo, rhi) == (lo, hi) and scene.lerp(lo_v, hi_v, g) == want, (n, q)


def test_visibility_matrix_follows_the_reference_rule(g29):
    for c, (F, W, H, N) in CASES.items():
        pi, ii, (start, end) = g29[f"{c}/point_index"], g29[f"{c}/image_id"], g29[f"{c}/start_end"]
        assert ((ii - 1 < start) | (ii - 1 >= end)).sum() >= 6                   # ids outside the frame range are in the list
        got = scene.visibility_matrix(pi, ii, N, (start, end))
        assert got.dtype == np.uint8 and np.array_equal(got, g29[f"{c}/vis"])
        assert np.array_equal(got, sn.visibility(pi, ii, N, int(start), int(end)))
    assert np.array_equal(scene.visibility_matrix(torch.tensor([0, 1, 1]), torch.tensor([3, 3, 9]), 2, (2, 4)), [[1, 1], [0, 0]])
    with pytest.raises(ValueError, match="point indices"):
        scene.visibility_matrix([5], [3], 2, (2, 4))
    with pytest.raises(ValueError, match="start < end"):
        scene.visibility_matrix([0], [3], 2, (4, 4))


def test_header_symbols_and_abi():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    for sym in ("nsff_scene_scale", "nsff_scene_scale_work_bytes"):
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.nsff_abi_version() == _lib.ABI_VERSION == 32
    assert C.sizeof(_lib.SceneScaleArgs) == 16 + 8 + 8 * 10 + 8
    assert "scale.hip" in open(os.path.join(ROOT, "nsff_pl_amd", "csrc", "Makefile")).read()
    import nsff_pl_amd
    assert nsff_pl_amd.scene is scene and nsff_pl_amd.nearest_depth is scene.nearest_depth
    assert nsff_pl_amd.scene_from_colmap is scene.scene_from_colmap and nsff_pl_amd.visibility_matrix is scene.visibility_matrix


def _args(**kw):
    """Arguments that pass every check but the one under test (fake, aligned device addresses: nothing is launched)."""
    F, N, H, W = 2, 300, 24, 40
    a = _lib.SceneScaleArgs(n_frames=F, n_points=N, H=H, W=W, disp_rank=(C.c_int32 * 2)(911, 912),
                            work_bytes=_lib.scene_scale_work_bytes(F, N, H, W))
    for i, name in enumerate(("points", "vis", "w2c", "K", "disps", "stats", "disp_os", "depth_os", "pix", "work")):
        setattr(a, name, 0x10000 * (i + 1))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_entry_refuses_by_name():
    lib = _lib.load()
    call = lambda a: lib.nsff_scene_scale(C.byref(a), None)
    assert lib.nsff_scene_scale(None, None) == -2
    assert call(_args(n_points=0)) == -1 and call(_args(n_frames=0)) == -1 and call(_args(n_frames=65536)) == -1
    assert call(_args(H=0)) == -1 and call(_args(H=65536, W=65536)) == -1
    for bad in ((-1, 5), (5, 960), (960, 960), (0, 2 ** 31 - 1)):
        assert call(_args(disp_rank=(C.c_int32 * 2)(*bad))) == -1
    for name in ("points", "vis", "w2c", "K", "disps", "stats", "disp_os", "depth_os", "work"):
        assert call(_args(**{name: None})) == -2, name
    assert call(_args(work_bytes=_lib.scene_scale_work_bytes(2, 300, 24, 40) - 1)) == -1
    assert call(_args(work=0x10008)) == -3 and call(_args(points=0x10004)) == -3 and call(_args(disps=0x10002)) == -3
    assert call(_args(pix=0x10002)) == -3
    # the workspace: tickets and partials, 2 x (4 + 8) x 256 histogram counters and N depths per frame
    assert _lib.scene_scale_work_bytes(2, 300, 24, 40) == 16 + 8 * 6 * 2 * 2 + 4 * 2 * 2 * 12 * 256 + 8 * 2 * 300
    assert _lib.scene_scale_work_bytes(1, 0, 24, 40) == 0 and _lib.scene_scale_work_bytes(0, 5, 24, 40) == 0
    assert _lib.scene_scale_work_bytes(1, 5, 65536, 65536) == 0


def test_python_layer_refuses_by_name(g29):
    G = lambda k: g29[f"c0/{k}"]
    with pytest.raises(RuntimeError, match="nearest_depth: disps must be a GPU tensor"):
        scene.nearest_depth(G("K"), G("w2c"), G("points"), G("vis"), torch.from_numpy(G("disps")))
    with pytest.raises(RuntimeError, match="nearest_depth: disps must be a GPU tensor"):
        scene.nearest_depth(G("K"), G("w2c"), G("points"), G("vis"), G("disps"))
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        _lib.scene_scale(*(torch.from_numpy(np.ascontiguousarray(G(k))) for k in ("points", "vis", "w2c", "K", "disps")), (0, 1))
    good = np.array([[5, 0, 0.3, 0.4, 1.0, 0.9, 1.0, 0]], np.float64)
    os2, dz = np.zeros((1, 2), np.float32), np.ones((1, 2))
    assert scene.regression_table(good, os2, dz, 960)["used_regression"].tolist() == [False]
    for col, value, what in ((0, 1, "frame 0 has 1 visible points"), (4, 0.0, "all 1/depth values of frame 0 are identical"),
                             (1, 2, "frame 0 has 2 visible points whose projection is not finite"),
                             (7, 3, "frame 0 has 3 NaN disparities")):
        bad = good.copy()
        bad[0, col] = value
        with pytest.raises(ValueError, match=what):
            scene.regression_table(bad, os2, dz, 960)
