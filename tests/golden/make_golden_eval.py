"""Generate tests/golden/g25_eval.npz by RUNNING THE REFERENCE's test-split paths, PSNR and depth visualisation.

Build-container only, like make_golden.py (whose stand-ins for kornia / datasets it imports): the reference (kwea123/nsff_pl,
read-only, absent on the GPU box) supplies the code that computes, this file only the inputs:

* ``datasets/colmap_utils.py``'s own ``create_spiral_poses`` (scipy's Slerp) and ``create_wander_path`` on a 13-pose scene;
* the split block of ``datasets/monocular.py`` (``elif self.split == 'test': ... n_poses=60)``) and the time rule of its
  ``__getitem__`` (``if self.split == 'test': t = idx ... else: t = 0``) are read from the reference's file when this tool runs
  and executed on a stand-in ``self`` -- the dataset class itself decodes files with cv2 / torchvision, neither installed;
* ``metrics.psnr`` with and without ``mask == 0`` on the clipped frames, as eval.py:233, 238 call it (kornia.losses is a stand-in
  module: the SSIM half has its own golden);
* ``utils/visualization.py`` is loaded by path with stand-ins for ``cv2.applyColorMap`` (= ``lut[x]``, which also records the
  index image it was handed) and ``torchvision.transforms.ToTensor`` (PIL image -> (3, H, W) / 255), and ``visualize_depth`` runs
  as eval.py's ``save_depth`` calls it: on ``nan_to_num(depth)``, the result scaled by 255 and cast to uint8.

Only inputs and results are written; no reference source travels.

    python tests/golden/make_golden_eval.py                 # rewrites tests/golden/g25_eval.npz

Keys: poses (13,3,4) float64; for each split S in SPLITS ``path/S`` (n,3,4) float64 and ``ts/S`` (n,) int64; ``spiral_direct``
(40,3,4) = create_spiral_poses(poses, [0.3, 0.1, 0.7], 40); rgb / gt (3,19,33,3) fp32, mask (3,19,33) uint8 (frame 1 all
dynamic: no valid pixel; frame 2 all static), psnr (3,2) fp32 [whole, mask == 0]; depth (6,19,33) fp32 (plain, with NaNs, with
+inf, all-negative, constant, with -inf), lut (256,3) uint8, depth_u8 (6,19,33), depth_rgb_u8 (6,19,33,3) uint8.
"""
import importlib.util
import os
import sys
import textwrap
import types
import warnings

import numpy as np
import torch

import make_golden
from make_golden_records import rotation

HERE = os.path.dirname(os.path.abspath(__file__))
N_POSES = 13
SPLITS = ("test", "test_spiral", "test_spiral4", "test_fixview3_interp5")
H, W = 19, 33


def scene_poses():
    rng = np.random.default_rng(25)
    poses = np.zeros((N_POSES, 3, 4))
    angles = np.cumsum(rng.uniform(-0.06, 0.09, (N_POSES, 3)), 0)
    xyz = np.cumsum(rng.uniform(-0.02, 0.12, (N_POSES, 3)), 0)
    for t in range(N_POSES):
        poses[t, :, :3] = rotation(*angles[t])
        poses[t, :, 3] = xyz[t] - xyz[N_POSES // 2]
    return poses


def reference_block(first_mark, last_mark, max_lines):
    """The dedented statements of datasets/monocular.py from the line holding first_mark to the next one holding last_mark."""
    path = os.path.join(make_golden.REF, "datasets", "monocular.py")
    with open(path) as f:
        lines = f.readlines()
    first = next(i for i, l in enumerate(lines) if first_mark in l)
    last = next(i for i in range(first, len(lines)) if last_mark in lines[i])
    assert last - first < max_lines, "the reference's block is not where it was"
    block = textwrap.dedent("".join(lines[first:last + 1]))
    if block.startswith("elif"):
        block = block[2:]                                   # the chain's first arm, run on its own
    return compile(block, path, "exec")


def reference_splits(poses, colmap_utils):
    split_block = reference_block("elif self.split == 'test':", "n_poses=60)", 24)
    time_block = reference_block(" if self.split == 'test':", "else: t = 0", 12)
    out = {}
    for split in SPLITS:
        me = types.SimpleNamespace(split=split, poses=poses.copy(), N_frames=len(poses), image_paths=[])
        exec(split_block, {"np": np, "colmap_utils": colmap_utils, "self": me})
        path = np.asarray(me.poses_test, dtype=np.float64)[:, :3, :]            # (the wander path is a list of 4 x 4 matrices)
        ts = []
        for idx in range(len(path)):
            scope = {"self": me, "idx": idx}
            exec(time_block, scope)
            ts.append(scope["t"])
        out["path/" + split], out["ts/" + split] = path, np.asarray(ts, dtype=np.int64)
    return out


def image_case():
    rng = np.random.default_rng(26)
    gt = rng.random((3, H, W, 3), dtype=np.float32)
    rgb = (gt + 0.2 * rng.standard_normal((3, H, W, 3))).astype(np.float32)      # leaves [0, 1] on both sides
    mask = (rng.random((3, H, W)) < 0.3).astype(np.uint8)
    mask[1], mask[2] = 1, 0
    return gt, rgb, mask


def reference_psnr(gt, rgb, mask):
    kornia_losses = types.ModuleType("kornia.losses")
    kornia_losses.ssim_loss = None
    sys.modules["kornia.losses"] = kornia_losses
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(make_golden.REF, "metrics.py"))
    metrics = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(metrics)
    out = np.zeros((len(gt), 2), np.float32)
    for i in range(len(gt)):
        img_gt, img_pred = torch.from_numpy(gt[i]), torch.clip(torch.from_numpy(rgb[i]), 0, 1)
        out[i, 0] = metrics.psnr(img_gt, img_pred).item()
        out[i, 1] = metrics.psnr(img_gt, img_pred, torch.from_numpy(mask[i]) == 0).item()
    return out


def depth_case():
    rng = np.random.default_rng(27)
    d = (rng.random((6, H, W)) * 3 + 0.2).astype(np.float32)
    d[1].flat[rng.choice(H * W, 40, replace=False)] = np.nan
    d[2].flat[rng.choice(H * W, 25, replace=False)] = np.inf
    d[3] = -d[3]
    d[4] = np.float32(1.75)
    d[5].flat[rng.choice(H * W, 25, replace=False)] = -np.inf
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    return d, lut


def reference_depth_images(depth, lut):
    seen = []
    cv2 = types.ModuleType("cv2")
    cv2.COLORMAP_JET, cv2.COLORMAP_BONE = 2, 1

    def apply_color_map(x, cmap):
        assert x.dtype == np.uint8 and cmap == cv2.COLORMAP_JET
        seen.append(x.copy())
        return lut[x]
    cv2.applyColorMap = apply_color_map
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")

    class ToTensor:                                         # torchvision transforms/functional.py::to_tensor of a uint8 image
        def __call__(self, pic):
            return torch.from_numpy(np.asarray(pic)).permute(2, 0, 1).to(torch.float32).div(255)
    tvt.ToTensor = ToTensor
    tv.transforms = tvt
    sys.modules.update({"cv2": cv2, "torchvision": tv, "torchvision.transforms": tvt})
    spec = importlib.util.spec_from_file_location("ref_visualization", os.path.join(make_golden.REF, "utils", "visualization.py"))
    vis = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vis)
    images = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (overflow warnings of the +-inf frames)
        for frame in depth:                                 # eval.py's save_depth
            depth_pred = np.nan_to_num(torch.from_numpy(frame).view(H, W).numpy())
            img = vis.visualize_depth(torch.from_numpy(depth_pred)).permute(1, 2, 0).numpy()
            images.append((img * 255).astype(np.uint8))
    return np.stack(seen), np.stack(images)


def main():
    make_golden.import_reference()
    from datasets import colmap_utils
    poses = scene_poses()
    out = dict(poses=poses, **reference_splits(poses, colmap_utils))
    out["spiral_direct"] = colmap_utils.create_spiral_poses(poses, np.array([0.3, 0.1, 0.7]), n_poses=40)
    assert out["path/test_spiral"].shape == (78, 3, 4) and out["path/test_spiral4"].shape == (60, 3, 4)
    assert out["ts/test_spiral4"].tolist() == [4] * 60 and out["path/test_fixview3_interp5"].shape == (13, 3, 4)
    gt, rgb, mask = image_case()
    out.update(gt=gt, rgb=rgb, mask=mask, psnr=reference_psnr(gt, rgb, mask))
    assert np.isnan(out["psnr"][1, 1]) and out["psnr"][2, 1] == out["psnr"][2, 0]
    depth, lut = depth_case()
    depth_u8, depth_rgb_u8 = reference_depth_images(depth, lut)
    assert not depth_u8[4].any() and np.array_equal(depth_rgb_u8, lut[depth_u8])
    out.update(depth=depth, lut=lut, depth_u8=depth_u8, depth_rgb_u8=depth_rgb_u8)
    path = os.path.join(HERE, "g25_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
