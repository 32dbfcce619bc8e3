"""Generate tests/golden/g28_resize.npz by RUNNING THE REFERENCE's two PIL resize statements.

Build-container only, like make_golden_panels.py: the reference (kwea123/nsff_pl, read-only, absent on the GPU box) supplies the
statements, this file only the inputs.  ``img = img.resize(self.img_wh, Image.LANCZOS)`` and
``mask = mask.resize(self.img_wh, Image.NEAREST)`` are read from datasets/monocular.py when this tool runs and executed on synthetic
8-bit frames with the installed Pillow; only inputs, results and the Pillow version are written.  The two cv2 statements
(INTER_NEAREST on the disparity, INTER_LINEAR inside flowlib.resize_flow) cannot run here -- cv2 is not installed -- and are not
in the file: those rules are pinned to their statement in include/nsff_render.h only.

    python tests/golden/make_golden_resize.py               # rewrites tests/golden/g28_resize.npz

Keys: ``n_cases``, ``pillow``; per case ``cN/src`` (F, h, w, 3) uint8, ``cN/dst`` (F, H, W, 3) uint8, ``cN/mask_src`` (F, h, w)
uint8, ``cN/mask_dst`` (F, H, W) uint8.  Even frames are uniform noise, odd frames 0/255 patterns (blocks of random size), so
that both clips between and after the passes fire; a case of one frame is half noise, half pattern.  Cases (h x w -> H x W):
  c0 F = 2  45 x 80 -> 19 x 33    both passes, ratios 2.37 and 2.42
  c1 F = 2  23 x 40 -> 31 x 57    upscale
  c2 F = 2  19 x 70 -> 19 x 33    horizontal pass only
  c3 F = 2  40 x 33 -> 19 x 33    vertical pass only
  c4 F = 2  19 x 33 -> 19 x 33    identity
  c5 F = 2  96 x 160 -> 12 x 20   8x: ksize 49, the widest table the kernel takes
  c6 F = 1  150 x 530 -> 70 x 261 three 128-pixel tile columns and five 16-row tile rows, ragged in both axes
"""
import os
import types

import numpy as np
import PIL
from PIL import Image

import make_golden

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 2800
CASES = ((2, 45, 80, 19, 33), (2, 23, 40, 31, 57), (2, 19, 70, 19, 33), (2, 40, 33, 19, 33), (2, 19, 33, 19, 33),
         (2, 96, 160, 12, 20), (1, 150, 530, 70, 261))


def reference_statement(mark):
    """The one dedented statement of datasets/monocular.py that holds `mark` (its first occurrence)."""
    path = os.path.join(make_golden.REF, "datasets", "monocular.py")
    with open(path) as f:
        line = next(l for l in f if mark in l)
    return compile(line.strip(), path, "exec")


def pattern(rng, shape):
    """0/255 blocks of random size: sharp edges, where the Lanczos lobes leave 0..255 on both sides"""
    h, w = shape[:2]
    by, bx = int(rng.integers(2, 7)), int(rng.integers(2, 7))
    cells = rng.integers(0, 2, (-(-h // by), -(-w // bx)) + tuple(shape[2:]), dtype=np.uint8) * 255
    return np.repeat(np.repeat(cells, by, 0), bx, 1)[:h, :w]


def frame(rng, kind, shape):
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "pattern":
        return pattern(rng, shape)
    out = rng.integers(0, 256, shape, dtype=np.uint8)           # one frame: upper half noise, lower half pattern
    out[shape[0] // 2:] = pattern(rng, shape)[shape[0] // 2:]
    return out


def main():
    lanczos = reference_statement("img.resize(self.img_wh, Image.LANCZOS)")
    nearest = reference_statement("mask.resize(self.img_wh, Image.NEAREST)")
    rng = np.random.default_rng(SEED)
    out = {"n_cases": np.int64(len(CASES)), "pillow": np.array(PIL.__version__)}
    for i, (F, h, w, H, W) in enumerate(CASES):
        me = types.SimpleNamespace(img_wh=(W, H))
        kinds = ["both"] if F == 1 else ["noise" if f % 2 == 0 else "pattern" for f in range(F)]
        src = np.stack([frame(rng, k, (h, w, 3)) for k in kinds])
        mask_src = np.stack([frame(rng, k, (h, w)) for k in kinds])
        dst, mask_dst = [], []
        for f in range(F):
            scope = {"self": me, "Image": Image, "img": Image.fromarray(src[f]).convert("RGB"),
                     "mask": Image.fromarray(mask_src[f]).convert("L")}
            exec(lanczos, scope)
            exec(nearest, scope)
            dst.append(np.asarray(scope["img"]))
            mask_dst.append(np.asarray(scope["mask"]))
        dst, mask_dst = np.stack(dst), np.stack(mask_dst)
        assert dst.shape == (F, H, W, 3) and mask_dst.shape == (F, H, W) and dst.dtype == mask_dst.dtype == np.uint8
        if (h, w) != (H, W):
            assert (dst == 0).any() and (dst == 255).any()      # both clips fired
        out.update({f"c{i}/src": src, f"c{i}/dst": dst, f"c{i}/mask_src": mask_src, f"c{i}/mask_dst": mask_dst})
    path = os.path.join(HERE, "g28_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)
    assert os.path.getsize(path) < 500_000


if __name__ == "__main__":
    main()
