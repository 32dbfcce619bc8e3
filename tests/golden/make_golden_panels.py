"""Generate tests/golden/g27_panels.npz by RUNNING THE REFERENCE's validation-panel statements.

Build-container only, like make_golden_eval.py: the reference (kwea123/nsff_pl, read-only, absent on the GPU box) supplies the code
that computes, this file only the inputs and the stand-ins for packages that are not installed:

* ``utils/visualization.py`` is loaded by path and its ``visualize_depth``, ``visualize_mask`` and ``blend_images`` run themselves;
* the statements of ``train.py``'s validation step from ``W, H = self.hparams.img_wh`` to ``img_grid = make_grid(...)`` (the error
  maps, their blends and ``img_list``) are read from the reference's file when this tool runs and executed on stand-in inputs.

Only inputs and results are written; no reference source travels.  Three things the reference does NOT pin here:

* ``cv2.addWeighted`` -- cv2 is not installed.  The stand-in is its documented formula ``saturate(round(a * alpha + b * beta + gamma))``
  in the integer form ``min(255, ((a + b) >> 1) + 2 + ((a + b) & 1))`` for alpha = beta = .5, gamma = 2.2; main() checks that form
  against fp32 and fp64 evaluation for all 65 536 byte pairs (the fraction is always .2 or .7: no rounding tie).
  ``cv2.applyColorMap`` is a table lookup ``lut[x]`` with a random table per colour map, which also records the index image.
* ``torchvision.utils.make_grid`` -- torchvision is not installed.  It is restated from its documented layout: ``nrow`` images
  per row, ``padding=2`` pixels of ``pad_value=0`` in front of every tile and behind the last row and column.  ``ToTensor`` is the
  uint8 image / 255 in fp32; main() checks that ``255 * x`` truncated returns every byte.
* ``metrics.ssim`` -- kornia is not installed.  The stand-in returns 1 - tests/ssim_numpy.py's loss map rounded to fp32; the loss
  map is stored as the INPUT ``ssim_loss``, so the golden pins what is done with the map, not the map.

The float images the reference hands to ``SummaryWriter.add_image`` are stored as that writer stores them: ``255 * x`` clipped to
0..255 and truncated to uint8.

One platform condition: torch's vectorised CPU sqrt is not correctly rounded everywhere, numpy's is, so the reference's fp32
``rmse_map`` may differ from numpy's by an ulp.  main() walks the seeds from SEED upwards to the first one for which the
reference's RMSE index image equals tests/panel_numpy.py's everywhere, asserts that, and stores the seed.

    python tests/golden/make_golden_panels.py               # rewrites tests/golden/g27_panels.npz

Keys: shared inputs gt, pred, transient_alpha, static_rgb, ssim_loss (19, 33[, 3]) fp32, lut_depth, lut_mask (256, 3) uint8, seed;
shared results rmse_map, ssim_map fp32, rmse_u8, ssim_u8 (19, 33) uint8, rmse_blend_u8, ssim_blend_u8 (19, 33, 3) uint8; and per
case ``cN/`` (N = 0..3) the inputs depth [, static_depth] [, mask] [, disp] (19, 33) fp32 with ``cN/tiles`` and the result
``cN/grid_u8`` (GH, 107, 3) uint8.  Cases: c0 3 tiles, depth with NaN and +-inf; c1 6 tiles, static depth with NaN; c2 8 tiles,
constant disparity; c3 8 tiles, no dynamic pixel (mask all 0).
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
import panel_numpy as pn
import ssim_numpy

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 19, 33
SEED = 2700
CASES = ((3, "nan_inf_depth"), (6, "nan_static_depth"), (8, "constant_disp"), (8, "all_static"))


def add_weighted(a, alpha, b, beta, gamma):
    assert a.dtype == b.dtype == np.uint8 and alpha == 0.5 and beta == 0.5 and gamma == 2.2
    s = a.astype(np.int32) + b.astype(np.int32)
    return np.minimum(255, (s >> 1) + 2 + (s & 1)).astype(np.uint8)


def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    tensor = torch.stack(list(tensor), 0)
    nmaps, ch, h, w = tensor.shape
    xmaps = min(nrow, nmaps)
    ymaps = -(-nmaps // xmaps)
    grid = tensor.new_full((ch, (h + padding) * ymaps + padding, (w + padding) * xmaps + padding), pad_value)
    for k in range(nmaps):
        y, x = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        grid[:, y:y + h, x:x + w] = tensor[k]
    return grid


def load_visualization(luts, seen):
    cv2 = types.ModuleType("cv2")
    cv2.COLORMAP_JET, cv2.COLORMAP_BONE = 2, 1

    def apply_color_map(x, cmap):
        assert x.dtype == np.uint8
        seen.append((cmap, x.copy()))
        return luts[cmap][x]
    cv2.applyColorMap, cv2.addWeighted = apply_color_map, add_weighted
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
    return vis


def reference_block(first_mark, last_mark, max_lines):
    """The dedented statements of train.py from the line holding first_mark to the next one holding last_mark."""
    path = os.path.join(make_golden.REF, "train.py")
    with open(path) as f:
        lines = f.readlines()
    first = next(i for i, l in enumerate(lines) if first_mark in l)
    last = next(i for i in range(first, len(lines)) if last_mark in lines[i])
    assert last - first < max_lines, "the reference's block is not where it was"
    return compile(textwrap.dedent("".join(lines[first:last + 1])), path, "exec")


def to_u8(chw):
    """SummaryWriter.add_image's conversion of a float CHW image, as HWC."""
    x = chw.permute(1, 2, 0).numpy()
    return np.clip(255 * x, 0, 255).astype(np.uint8)


def shared_inputs(seed):
    rng = np.random.default_rng(seed)
    gt = rng.random((H, W, 3), dtype=np.float32)
    pred = (gt + 0.2 * rng.standard_normal((H, W, 3))).astype(np.float32)          # leaves [0, 1] on both sides
    alpha = rng.random((H, W), dtype=np.float32)
    static_rgb = (rng.random((H, W, 3), dtype=np.float32) * 1.4 - 0.2).astype(np.float32)
    luts = {2: rng.integers(0, 256, (256, 3), dtype=np.uint8), 1: rng.integers(0, 256, (256, 3), dtype=np.uint8)}
    return rng, gt, pred, alpha, static_rgb, luts


def case_inputs(rng, n_tiles, kind):
    c = {"depth": (rng.random((H, W)) * 3 + 0.2).astype(np.float32)}
    if kind == "nan_inf_depth":
        d = c["depth"].reshape(-1)
        where = rng.permutation(d.size)
        d[where[:30]], d[where[30:33]], d[where[33:36]] = np.nan, np.inf, -np.inf
    if n_tiles >= 6:
        c["static_depth"] = (rng.random((H, W)) * 5 + 0.1).astype(np.float32)
        if kind == "nan_static_depth":
            c["static_depth"].reshape(-1)[rng.permutation(H * W)[:25]] = np.nan
    if n_tiles == 8:
        c["mask"] = (rng.random((H, W)) < 0.3).astype(np.float32)
        c["disp"] = rng.random((H, W), dtype=np.float32)
        if kind == "constant_disp":
            c["disp"][:] = np.float32(0.375)
        if kind == "all_static":
            c["mask"][:] = 0
    return c


def run_reference(block, vis, gt, pred, alpha, static_rgb, loss, c, n_tiles):
    metrics = types.SimpleNamespace(ssim=lambda image_gt, image_pred, reduction: torch.from_numpy(np.float32(1) - loss))
    results = {"rgb_fine": torch.from_numpy(pred).view(-1, 3), "depth_fine": torch.from_numpy(c["depth"]).view(-1)}
    if n_tiles >= 6:
        results.update({"transient_alpha_fine": torch.from_numpy(alpha).view(-1), "_static_rgb_fine": torch.from_numpy(static_rgb).view(-1, 3),
                        "_static_depth_fine": torch.from_numpy(c["static_depth"]).view(-1)})
    batch = {k: torch.from_numpy(c[k]).view(-1) for k in ("mask", "disp") if k in c}
    me = types.SimpleNamespace(hparams=types.SimpleNamespace(img_wh=(W, H)), output_transient=n_tiles >= 6)
    scope = {"self": me, "torch": torch, "metrics": metrics, "results": results, "batch": batch, "rgbs": torch.from_numpy(gt).view(-1, 3),
             "blend_images": vis.blend_images, "visualize_depth": vis.visualize_depth, "visualize_mask": vis.visualize_mask,
             "make_grid": make_grid, **{k: v for k, v in batch.items()}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (overflow / invalid-cast warnings of the NaN and +-inf frames)
        exec(block, scope)
    return scope


def check_stand_ins():
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    want = add_weighted(a, 0.5, b, 0.5, 2.2)
    assert np.array_equal(want, pn.blend_float(a, b, np.float32)) and np.array_equal(want, pn.blend_float(a, b, np.float64))
    byte = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).numpy()
    assert np.array_equal((255 * byte).astype(np.uint8), np.arange(256))


def generate(seed, block):
    rng, gt, pred, alpha, static_rgb, luts = shared_inputs(seed)
    loss = ssim_numpy.ssim_loss(gt.astype(np.float64), np.clip(pred, 0, 1).astype(np.float64)).astype(np.float32)
    out = dict(gt=gt, pred=pred, transient_alpha=alpha, static_rgb=static_rgb, ssim_loss=loss, lut_depth=luts[2], lut_mask=luts[1],
               seed=np.int64(seed))
    for i, (n_tiles, kind) in enumerate(CASES):
        c = case_inputs(rng, n_tiles, kind)
        seen = []
        vis = load_visualization(luts, seen)
        scope = run_reference(block, vis, gt, pred, alpha, static_rgb, loss, c, n_tiles)
        assert len(scope["img_list"]) == n_tiles and len(seen) == {3: 3, 6: 5, 8: 7}[n_tiles]
        assert [cmap for cmap, _ in seen] == [2, 2, 2, 1, 2, 1, 2][:len(seen)]
        shared = dict(rmse_map=scope["rmse_map"].numpy(), ssim_map=scope["ssim_map"].numpy(), rmse_u8=seen[0][1], ssim_u8=seen[1][1],
                      rmse_blend_u8=to_u8(scope["rmse_map_blend"]), ssim_blend_u8=to_u8(scope["ssim_map_blend"]))
        for k, v in shared.items():
            assert k not in out or np.array_equal(out[k], v), k                  # the error panels do not depend on the case
            out[k] = v
        out.update({f"c{i}/{k}": v for k, v in c.items()})
        out[f"c{i}/tiles"] = np.int64(n_tiles)
        out[f"c{i}/grid_u8"] = to_u8(scope["img_grid"])
        assert out[f"c{i}/grid_u8"].shape == (-(-n_tiles // 3) * (H + 2) + 2, 3 * (W + 2) + 2, 3)
    return out


def main():
    check_stand_ins()
    block = reference_block("W, H = self.hparams.img_wh", "img_grid = make_grid(", 30)
    for seed in range(SEED, SEED + 50):
        out = generate(seed, block)
        mine = pn.index_image(-pn.rmse_map(out["gt"], out["pred"])[None])[0]
        if np.array_equal(mine, out["rmse_u8"]):
            break
        print(f"seed {seed}: the reference's RMSE index image differs from numpy's in {(mine != out['rmse_u8']).sum()} pixels; next")
    assert np.array_equal(mine, out["rmse_u8"]), "no seed in range gives equal RMSE index images"
    ulp = np.abs(out["rmse_map"].view(np.int32).astype(np.int64) - pn.rmse_map(out["gt"], out["pred"]).view(np.int32)).max()
    print(f"seed {seed}: RMSE index images equal; fp32 rmse_map differs from numpy's by at most {ulp} ulp")
    assert ulp <= 1
    path = os.path.join(HERE, "g27_panels.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
