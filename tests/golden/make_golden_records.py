"""Generate tests/golden/g24_ray_records.npz by RUNNING THE REFERENCE's ray generation on a three-frame scene.

Build-container only, like make_golden.py (whose kornia / datasets stand-ins it imports): the reference (kwea123/nsff_pl,
read-only, absent on the GPU box) supplies the code that computes, this file only the inputs and the column placement:

* the rays and ``uv`` come from the reference's ``datasets/ray_utils.py`` -- ``get_ray_directions(return_uv=True)``, ``get_rays``,
  ``get_ndc_rays`` -- called per frame with the near-plane shift of the training split (1 unless the camera sits behind z = -1);
* ``Ps`` comes from the reference's OWN statements: the block of ``datasets/monocular.py`` that fills ``self.Ps`` / ``self.Ks`` is
  read from the reference's file when this tool runs and executed on a stand-in object that holds ``N_frames``, ``poses``, ``K``.

The dataset class itself cannot be constructed here (it decodes files with cv2 / PIL / torchvision, none installed), so its
decoded inputs are synthesised and placed in the 16 columns the training split uses (rays 0-5, rgb 6-8, t 9, disparity 10, mask
11, uv + forward flow 12-13, uv + backward flow 14-15; the last frame has no forward and the first no backward flow file, so
those are zero).  ``ToTensor`` of a uint8 image is a division by 255 in fp32 (torchvision transforms/functional.py::to_tensor).
Only data is written; no reference source travels.

    python tests/golden/make_golden_records.py              # rewrites tests/golden/g24_ray_records.npz

Scene: F = 3 frames, H x W = 19 x 33 (627 pixels: three 256-pixel blocks with a ragged tail), fx != fy, small rotations about
all three axes, c2w[2,3] = 0.3, -1.7, -1.0 (both branches of shift_near and their boundary), random uint8 images and masks,
flows ~ 3 N(0,1) that are non-zero ALSO in the two slots a builder must ignore (frame F-1 forward, frame 0 backward).
Keys: K, poses (float64), images, masks (uint8), disps, flows_fw, flows_bw (fp32), records (F, H*W, 16) fp32, Ps (1, F, 3, 4) fp32.
"""
import os
import textwrap
import types

import numpy as np
import torch

import make_golden

HERE = os.path.dirname(os.path.abspath(__file__))
F, H, W = 3, 19, 33
K = np.array([[37.0, 0, 16.5], [0, 41.0, 9.5], [0, 0, 1]])
TZ = (0.3, -1.7, -1.0)


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def scene():
    rng = np.random.default_rng(24)
    poses = np.zeros((F, 3, 4))
    for t in range(F):
        poses[t, :, :3] = rotation(*rng.uniform(-0.08, 0.08, 3))
        poses[t, :, 3] = [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), TZ[t]]
    return dict(K=K, poses=poses,
                images=rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8),
                masks=rng.choice(np.array([0, 255, 128], np.uint8), (F, H, W), p=[0.6, 0.3, 0.1]),
                disps=(rng.random((F, H, W)) * 2 + 0.05).astype(np.float32),
                flows_fw=(3 * rng.standard_normal((F, H, W, 2))).astype(np.float32),
                flows_bw=(3 * rng.standard_normal((F, H, W, 2))).astype(np.float32))


def reference_projection(poses):
    """(1, F, 3, 4) fp32: the reference's own projection-matrix statements, read from its file and run on a stand-in ``self``."""
    path = os.path.join(make_golden.REF, "datasets", "monocular.py")
    with open(path) as f:
        lines = f.readlines()
    first = next(i for i, l in enumerate(lines) if "create projection matrix" in l)
    last = next(i for i in range(first, len(lines)) if lines[i].lstrip().startswith("self.Ks"))
    block = textwrap.dedent("".join(lines[first:last + 1]))
    assert "self.Ps" in block and last - first < 12, "the reference's projection block is not where it was"
    me = types.SimpleNamespace(N_frames=len(poses), poses=poses, K=K)
    exec(compile(block, path, "exec"), {"np": np, "torch": torch, "self": me})
    assert np.array_equal(me.Ks.numpy()[0], K.astype(np.float32))
    return me.Ps


def reference_records(s, ray_utils):
    """(F, H*W, 16) fp32: the reference's ray functions per frame, the synthetic frame data beside them."""
    n = H * W
    unit = lambda u8: torch.from_numpy(u8).to(torch.float32).div(255)
    flows = {k: torch.from_numpy(s[k]).clone() for k in ("flows_fw", "flows_bw")}
    flows["flows_fw"][F - 1] = 0                        # no forward flow file after the last frame ...
    flows["flows_bw"][0] = 0                            # ... and no backward one before the first
    cam_dirs, uv = ray_utils.get_ray_directions(H, W, s["K"], return_uv=True)
    out = torch.empty(F, n, 16)
    for t, pose in enumerate(s["poses"]):
        shift = max(1.0, -float(pose[2, 3]))
        o, d = ray_utils.get_ndc_rays(s["K"], 1.0, shift, *ray_utils.get_rays(cam_dirs, torch.FloatTensor(pose)))
        out[t, :, 0:3], out[t, :, 3:6] = o, d
        out[t, :, 6:9] = unit(s["images"][t]).view(n, 3)
        out[t, :, 9] = t
        out[t, :, 10] = torch.from_numpy(s["disps"][t]).view(n)
        out[t, :, 11] = unit(s["masks"][t]).view(n)
        out[t, :, 12:14] = uv + flows["flows_fw"][t].view(n, 2)
        out[t, :, 14:16] = uv + flows["flows_bw"][t].view(n, 2)
    return out


def main():
    make_golden.import_reference()
    from datasets import ray_utils
    s = scene()
    Ps = reference_projection(s["poses"])
    records = reference_records(s, ray_utils)
    assert records.shape == (F, H * W, 16) and records.dtype == torch.float32
    assert Ps.shape == (1, F, 3, 4) and Ps.dtype == torch.float32
    path = os.path.join(HERE, "g24_ray_records.npz")
    np.savez_compressed(path, records=records.numpy(), Ps=Ps.numpy(), **s)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
