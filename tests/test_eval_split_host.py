"""CPU checks of the test-split layer: camera paths and time indices (nsff_pl_amd/paths.py) against golden g25 (the reference's
own create_spiral_poses / create_wander_path and its split statements, tests/golden/make_golden_eval.py), eval.py's frame
names, the score table, the numpy restatement tests/frame_finish_numpy.py against the reference's PSNR and depth images, and
nsff_frame_finish's argument validation (no launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import frame_finish_numpy as ffn
from nsff_pl_amd import _lib, evaluate, paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH_TOL = 1e-9          # absolute, float64 on both sides: the numpy slerp against scipy's, and the order of operations
PSNR_TOL = 1e-4          # the project's relative bar


@pytest.fixture(scope="module")
def g25():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g25_eval.npz")))


def test_golden_is_the_one_described(g25):
    assert g25["poses"].shape == (13, 3, 4) and g25["poses"].dtype == np.float64
    assert g25["path/test_spiral"].shape == (78, 3, 4) and g25["path/test_spiral4"].shape == (60, 3, 4)
    assert g25["rgb"].min() < 0 and g25["rgb"].max() > 1                                     # the clip has work to do
    assert g25["mask"][1].all() and not g25["mask"][2].any()
    assert np.isnan(g25["depth"][1]).sum() == 40 and np.isposinf(g25["depth"][2]).sum() == 25
    assert (g25["depth"][3] < 0).all() and np.ptp(g25["depth"][4]) == 0 and np.isneginf(g25["depth"][5]).sum() == 25
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g25_eval.npz")) < 200_000


@pytest.mark.parametrize("split,n", [("test", 13), ("test_spiral", 78), ("test_spiral4", 60), ("test_fixview3_interp5", 13)])
def test_split_paths_match_the_reference(g25, split, n):
    got, ts, interp = paths.split_path(g25["poses"], split)
    want = g25["path/" + split]
    assert got.shape == want.shape == (n, 3, 4) and got.dtype == np.float64
    err = np.abs(got - want).max()
    print(f"{split}: max abs pose error {err:.2e}")
    assert err <= PATH_TOL
    assert ts.dtype == np.int64 and np.array_equal(ts, g25["ts/" + split])
    assert interp == (5 if split.startswith("test_fixview") else 0)


def test_split_times_by_rule(g25):
    poses = g25["poses"]
    assert paths.split_path(poses, "test")[1].tolist() == list(range(13))
    assert paths.split_path(poses, "test_fixview3_interp5")[1].tolist() == list(range(13))
    assert paths.split_path(poses, "test_spiral")[1].tolist() == [int(i / 78 * 13) for i in range(78)]
    assert paths.split_path(poses, "test_spiral4")[1].tolist() == [4] * 60
    fix = paths.split_path(poses, "test_fixview3_interp5")[0]
    assert np.array_equal(fix, np.broadcast_to(poses[3], (13, 3, 4)))
    got = paths.split_path(poses, "test")[0]
    assert np.array_equal(got, poses) and got is not poses


def test_spiral_and_wander_directly(g25):
    poses = g25["poses"]
    got = paths.spiral_poses(poses, [0.3, 0.1, 0.7], 40)
    assert np.abs(got - g25["spiral_direct"]).max() <= PATH_TOL
    R = got[:, :, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.allclose(np.linalg.det(R), 1)
    # key times are reproduced: pose k * 40 / 12 ... only t = 0 lands on a key here; the 78-pose path hits key 2 at pose 13
    whole = paths.split_path(poses, "test_spiral")[0]
    assert np.abs(whole[13, :, :3] - poses[2, :, :3]).max() < 1e-12
    w = paths.wander_path(poses[4], 0.25, 60)
    four = np.concatenate([poses[4], [[0, 0, 0, 1.0]]], 0)
    assert w.shape == (60, 3, 4) and np.abs(paths.wander_path(four, 0.25, 60) - w).max() == 0
    assert np.abs(w[:, :, :3] - poses[4, :, :3]).max() == 0                                   # a pure translation of the camera
    # slerp through a large turn: half way between identity and a 2.4 rad turn about z is the 1.2 rad turn
    c, s = np.cos(2.4), np.sin(2.4)
    two = np.stack([np.eye(3), np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])])
    mid = paths.slerp_rotations(two, [0.5])[0]
    assert np.abs(mid - [[np.cos(1.2), -np.sin(1.2), 0], [np.sin(1.2), np.cos(1.2), 0], [0, 0, 1]]).max() < 1e-14


def test_frame_names_and_counts():
    assert paths.frame_names(3) == ["000", "001", "002"]
    assert paths.frame_names(3, 3) == ["000_000", "000_033", "000_066", "001_000", "001_033", "001_066", "002_000"]
    names = paths.frame_names(13, 5)
    assert len(names) == 12 * 5 + 1 and names[:6] == ["000_000", "000_020", "000_040", "000_060", "000_080", "001_000"]
    assert names[-1] == "012_000" and len(paths.frame_names(4, 3)) == 10
    assert len(paths.frame_names(78)) == 78 and paths.frame_names(78)[-1] == "077"


@pytest.mark.parametrize("bad", ["val", "train", "test_", "test_spiralx", "test_fixview3", "test_fixview_interp5",
                                 "test_fixview3_interp", "test_fixview3_interp5x", "test_spiral-1", ""])
def test_unknown_splits_are_refused_by_name(g25, bad):
    with pytest.raises(ValueError, match=r"'test', 'test_spiral', 'test_spiral\{X\}' or 'test_fixview\{X\}_interp\{Y\}'"):
        paths.split_path(g25["poses"], bad)


def test_bad_targets_and_poses_are_refused(g25):
    for split in ("test_spiral13", "test_fixview13_interp2"):
        with pytest.raises(ValueError, match="outside the sequence of 13 frames"):
            paths.split_path(g25["poses"], split)
    with pytest.raises(ValueError, match=r"\(N, 3, 4\)"):
        paths.split_path(g25["poses"][0], "test")
    with pytest.raises(ValueError, match="at least two"):
        paths.spiral_poses(g25["poses"][:1], [1, 1, 0], 6)


def test_score_table_formats_like_eval():
    scores = evaluate.SequenceScores()
    assert len(scores) == 0 and scores.psnrs.shape == (0, 2)
    rows = np.array([[30.0, 20.0, 0.95, 0.9], [32.0, np.nan, 0.97, np.nan], [31.0, 22.0, 0.9, 0.8]])
    scores._rows = [torch.tensor(r, dtype=torch.float32) for r in rows]
    assert scores.psnrs.shape == scores.ssims.shape == (3, 2) and scores.psnrs.dtype == np.float64
    assert np.isnan(scores.psnrs[1, 1]) and np.isnan(scores.ssims[1, 1])
    mp, ms = scores.means()
    assert mp.tolist() == [31.0, 21.0]                                                      # nanmean skips the empty mask
    assert np.allclose(ms, [0.94, 0.85], atol=1e-7)
    assert scores.table() == ["Score \t Whole image  \t Dynamic only", "-" * 37,
                              "PSNR  \t 31.0000 \t 21.0000", "SSIM  \t 0.9400 \t 0.8500"]


def test_scores_are_saved_as_eval_names_them(tmp_path):
    scores = evaluate.SequenceScores()
    scores._rows = [torch.tensor([30.0, 0.0, 0.9, 0.0]), torch.tensor([28.0, 0.0, 0.8, 0.0])]
    scores.save(str(tmp_path / "out"))
    assert np.array_equal(np.load(tmp_path / "out" / "psnr.npy"), [[30.0, 0.0], [28.0, 0.0]])
    assert np.load(tmp_path / "out" / "ssim.npy").shape == (2, 2)


# ---- the numpy restatement against the reference's own statements ----
def test_restatement_reproduces_the_reference_depth_images(g25):
    idx = ffn.depth_u8(g25["depth"])
    assert np.array_equal(idx, g25["depth_u8"])
    assert np.array_equal(g25["lut"][idx], g25["depth_rgb_u8"])
    assert not idx[4].any()                                                                   # ma == mi: 0 / 1e-8
    assert idx[2].max() == 255 and (idx[2] == 255).sum() == 25 and (idx[5] == 0).sum() == 25  # +inf on top, -inf at the bottom
    rng = ffn.depth_range(g25["depth"])
    assert rng.dtype == np.float32 and rng[2, 1] == np.finfo(np.float32).max and rng[5, 0] == -np.finfo(np.float32).max
    assert rng[4].tolist() == [1.75, 1.75] and rng[1, 0] == 0.0                              # NaN counts as 0


def test_restatement_reproduces_the_reference_psnr(g25):
    gt, rgb, mask = g25["gt"], g25["rgb"], g25["mask"]
    sums = ffn.error_sums(gt, rgb, mask == 0)
    assert sums[:, 2].tolist() == [(mask[0] == 0).sum(), 0, 19 * 33]
    whole, valid = ffn.psnr_from_sums(sums, 19 * 33)
    want = g25["psnr"]
    assert np.abs(whole - want[:, 0]).max() <= PSNR_TOL * np.abs(want[:, 0]).max()
    assert np.isnan(valid[1]) and np.isnan(want[1, 1]) and valid[2] == whole[2]
    assert np.abs(valid[[0, 2]] - want[[0, 2], 1]).max() <= PSNR_TOL * np.abs(want[[0, 2], 1]).max()
    u8 = ffn.rgb_u8(rgb)
    assert u8.dtype == np.uint8 and u8.min() == 0 and u8.max() == 255


# ---- C ABI ----
_BUF = (C.c_double * 64)()                                  # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15


def _args(**kw):
    a = _lib.FrameFinishArgs(n_frames=2, H=4, W=5, rgb=_P, gt=_P, valid=_P, depth=_P, lut=_P, rgb_clipped=_P, rgb_u8=_P,
                             sums=_P, depth_range=_P, depth_u8=_P, depth_rgb_u8=_P, scratch=_P, scratch_bytes=1 << 20)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_abi_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_frame_finish(C.byref(_args(**kw)), None)
    assert lib.nsff_frame_finish(None, None) == -2
    assert call(rgb=None) == -1                                                               # no image
    for bad in (dict(H=0), dict(W=0), dict(H=-3), dict(n_frames=0), dict(n_frames=70000), dict(H=65536, W=32768),
                dict(lut=None),                                                               # depth_rgb_u8 without its table
                dict(gt=None), dict(depth=None), dict(depth_range=None),                      # outputs without their inputs
                dict(depth=None, depth_u8=None, depth_rgb_u8=None),                           # (depth_range still asks for depth)
                dict(scratch_bytes=8),
                dict(rgb_clipped=None, rgb_u8=None, sums=None, depth_range=None, depth_u8=None, depth_rgb_u8=None)):
        assert call(**bad) == -1, bad
    assert call(scratch=None) == -2
    assert call(scratch=_P + 8) == -3 and call(sums=_P + 4) == -3 and call(rgb=_P + 2) == -3 and call(depth=_P + 1) == -3
    assert C.sizeof(_lib.FrameFinishArgs) == 16 + 11 * 8 + 8 + 8
    need = lib.nsff_frame_finish_scratch_bytes
    assert need(0, 4, 5) == 0 and need(1, 0, 5) == 0 and need(1, 65536, 32768) == 0
    assert need(1, 1, 1) == 16 + 32 and need(3, 19, 33) == 16 + 3 * 32                         # 627 pixels: one workgroup a frame
    assert need(2, 37, 71) == 16 + 2 * 3 * 32 and need(5, 288, 512) == 32 + 5 * 144 * 32      # 2627 pixels: three; 147456: 144


def test_header_declares_the_symbols_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint nsff_frame_finish\(const NsffFrameFinishArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_frame_finish_scratch_bytes\(int32_t n_frames, int32_t H, int32_t W\);", header)
    for sym in ("nsff_frame_finish", "nsff_frame_finish_scratch_bytes"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym)
    assert callable(_lib.frame_finish) and callable(_lib.frame_finish_scratch_bytes)
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header)
    assert _lib.load().nsff_abi_version() == _lib.ABI_VERSION == 32


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from nsff_pl_amd import metrics
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.finish_frames(torch.zeros(1, 4, 5, 3))
    with pytest.raises(RuntimeError, match=r"\(F, H, W, 3\)"):
        metrics.finish_frames(torch.zeros(4, 5, 3))
    with pytest.raises(ValueError, match="needs gt"):
        metrics.finish_frames(torch.zeros(1, 4, 5, 3), valid_mask=torch.ones(1, 4, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="nothing to compute"):
        metrics.finish_frames(torch.zeros(1, 4, 5, 3), images=False)
    pool = evaluate.PinnedPool()
    assert pool.dtype == torch.float32 and evaluate.PinnedPool(depth=3, dtype=torch.uint8).dtype == torch.uint8
