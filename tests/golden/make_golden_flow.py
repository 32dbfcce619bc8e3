"""Generate tests/golden/g26_flow.npz by RUNNING THE REFERENCE's ndc2world, geometric flow loss and flowlib on a three-frame scene.

Build-container only, like make_golden.py (whose kornia / datasets stand-ins it imports): the reference (kwea123/nsff_pl,
read-only, absent on the GPU box) supplies the code that computes, this file only the inputs:

* the scene is golden g24's (make_golden_records.py): ``K``, ``Ps`` (the reference's own projection statements), the flows and the
  masks of three 19 x 33 frames at times 0, 1, 2 (``max_t = 2``: frame 2 has no forward and frame 0 no backward neighbour);
* ``xyz_fw`` / ``xyz_bw``: a point on each pixel's reference NDC ray (g24's records) at a random depth plus a small random offset,
  NDC z in [-1, 0.95] -- the range rendered points stay in, flows being zeroed beyond 0.95 (rendering.py:187-188).  Depths whose
  world point would come within 0.1 of the target camera's plane are drawn again (the projection is ill-conditioned there and
  pins nothing); eight points per frame and direction are then moved to z >= 1 (behind every camera), which with the points the
  scene itself puts behind a target camera serve the validity flag only;
* ``world_fw`` / ``world_bw``: ``datasets/ray_utils.ndc2world`` of them, fp32, as the loss calls it; ``uv64_*`` / ``depth64_*``: the same
  function and the loss's projection formula evaluated in float64 (the yardstick for the fp32 ``uv``);
* ``flow_fw_l`` / ``flow_bw_l``: the two geometric terms of the reference's ``NeRFWLoss.forward`` (losses.py:99-124), run as
  make_golden.py's loss cases run it (``lambda_geo = 0.04``, buffers ``Ks`` / ``Ps`` / ``max_t``) with targets ``uv = pixel + flow``; the
  other inputs of ``forward`` are random fillers whose terms are not recorded.  Each term equals lambda / 2 times the mean L1
  difference between projected and target pixel over the valid rays: projection, clamp and validity rule in one number;
* ``datasets/flowlib.flow_to_image`` (imported with an empty ``cv2`` module) of every frame of the dataset's flows and of the
  induced maps (tests/flow_numpy.py's, unknown pixels 1e10 included; no NaN), with its default scale and with a given ``maxrad``:
  ``img_gt_*`` / ``img_ind_*`` and ``img_gt_*_given`` (maxrad ``GIVEN``) / ``img_ind_*_given`` (each frame on its ground truth's radius,
  ``given_ind_*``).

Only inputs and results are written; no reference source travels.

    python tests/golden/make_golden_flow.py                 # rewrites tests/golden/g26_flow.npz
"""
import os
import sys
import types

import numpy as np
import torch

import make_golden

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import flow_numpy as fnp  # noqa: E402

F, H, W = 3, 19, 33
MAX_T = 2
LAMBDA_GEO = 0.04
GIVEN = 7.5
N_BEHIND = 8


def depth64(world64, P64):
    return (P64[:, None, 2, :3] * world64).sum(-1) + P64[:, None, 2, 3]


def scene_points(g24, ray_utils):
    rng = np.random.default_rng(26)
    rec = g24["records"]
    o, d = rec[..., 0:3].astype(np.float64), rec[..., 3:6].astype(np.float64)
    Ps = g24["Ps"][0].astype(np.float64)
    K64 = torch.from_numpy(g24["K"])
    ts = np.arange(F)
    out = {}
    for tag, idx in (("fw", np.minimum(ts + 1, MAX_T)), ("bw", np.maximum(ts - 1, 0))):
        s = rng.uniform(0, 0.975, (F, H * W))
        off = rng.uniform(-0.02, 0.02, (F, H * W, 3))
        for _ in range(50):
            xyz = o + d * s[..., None] + off
            xyz[..., 2] = np.clip(xyz[..., 2], -1, 0.95)
            world = ray_utils.ndc2world(torch.from_numpy(xyz.reshape(-1, 3)), K64).numpy().reshape(F, H * W, 3)
            close = np.abs(depth64(world, Ps[idx])) < 0.1
            if not close.any():
                break
            s[close] = rng.uniform(0, 0.975, int(close.sum()))
        assert not close.any()
        for f in range(F):
            where = rng.choice(H * W, N_BEHIND, replace=False)
            xyz[f, where, 2] = rng.uniform(1.0, 2.0, N_BEHIND)
            xyz[f, where[0], 2] = 1.0
        out["xyz_" + tag] = xyz.astype(np.float32)
    return out


def reference_world(xyz, K, ray_utils):
    """ndc2world in fp32, as the loss calls it."""
    Ks = torch.tensor(K, dtype=torch.float32)
    return ray_utils.ndc2world(torch.from_numpy(xyz.reshape(-1, 3)), Ks).numpy().reshape(xyz.shape)


def float64_uv(xyz, K, Ps, idx, ray_utils):
    """ndc2world on float64 tensors, then the projection of losses.py:105-106 / 110-111 written out in float64."""
    world = ray_utils.ndc2world(torch.from_numpy(xyz.astype(np.float64).reshape(-1, 3)), torch.from_numpy(K)).numpy()
    world = world.reshape(xyz.shape)
    P = Ps.astype(np.float64)[idx][:, None]                                     # (F, 1, 3, 4)
    uvd = (P[..., :3] * world[..., None, :]).sum(-1) + P[..., 3]
    return uvd[..., :2] / (np.abs(uvd[..., 2:]) + 1e-8), uvd[..., 2]


def reference_flow_terms(pts, g24, ref_losses):
    """flow_fw_l / flow_bw_l of NeRFWLoss.forward on all F * H * W rays at once."""
    n = F * H * W
    g = torch.Generator().manual_seed(26)
    S = 4
    loss_fn = ref_losses.NeRFWLoss(lambda_geo=LAMBDA_GEO, thickness=1, topk=1.0)
    loss_fn.register_buffer("Ks", torch.tensor(g24["K"], dtype=torch.float32)[None])
    loss_fn.register_buffer("Ps", torch.from_numpy(g24["Ps"]))
    loss_fn.max_t = MAX_T
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs, ys], -1).reshape(1, H * W, 2)
    rnd = lambda *shape: torch.rand(*shape, generator=g)
    weights = torch.softmax(rnd(n, S), -1)
    inputs = dict(rgb_fine=rnd(n, 3), depth_fine=rnd(n), transient_weights_fine=weights, static_weights_fine=weights.flip(-1),
                  xyz_fw=torch.from_numpy(pts["xyz_fw"]).reshape(n, 3), xyz_bw=torch.from_numpy(pts["xyz_bw"]).reshape(n, 3),
                  disocc_fw=rnd(n, 1) + 0.1, disocc_bw=rnd(n, 1) + 0.1, rgb_fw=rnd(n, 3), rgb_bw=rnd(n, 3),
                  disoccs_fw=rnd(n, S, 1) + 0.1, disoccs_bw=rnd(n, S, 1) + 0.1, xyzs_fine=rnd(n, S, 3) - 0.5,
                  xyzs_fw=rnd(n, S, 3) - 0.5, xyzs_bw=rnd(n, S, 3) - 0.5, xyzs_fw_bw=rnd(n, S, 3) - 0.5, xyzs_bw_fw=rnd(n, S, 3) - 0.5)
    targets = dict(rgbs=rnd(n, 3), disps=rnd(n) + 0.1, cam_ids=torch.zeros(n, dtype=torch.long),
                   ts=torch.arange(F).repeat_interleave(H * W),
                   uv_fw=(pix + torch.from_numpy(g24["flows_fw"]).reshape(F, H * W, 2)).reshape(n, 2),
                   uv_bw=(pix + torch.from_numpy(g24["flows_bw"]).reshape(F, H * W, 2)).reshape(n, 2))
    with torch.no_grad():
        terms = loss_fn(inputs, targets, epoch=5, output_transient_flow=["fw", "bw"])
    return float(terms["flow_fw_l"]), float(terms["flow_bw_l"])


def reference_images(flowlib, flows, maxrad=None):
    """flow_to_image per frame; flowlib writes into its argument, so each frame goes in as a copy."""
    out = []
    for i, fr in enumerate(flows):
        if maxrad is None:
            out.append(flowlib.flow_to_image(fr.copy()))
        else:
            out.append(flowlib.flow_to_image(fr.copy(), maxrad=float(np.broadcast_to(maxrad, (len(flows),))[i])))
    out = np.stack(out)
    assert out.dtype == np.uint8 and out.shape == flows.shape[:3] + (3,)
    return out


def main():
    make_golden.import_reference()
    from datasets import ray_utils
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from datasets import flowlib
    sys.path.insert(0, make_golden.REF)
    import losses as ref_losses
    g24 = dict(np.load(os.path.join(HERE, "g24_ray_records.npz")))
    K, Ps = g24["K"], g24["Ps"][0]
    K4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    ts = np.arange(F)
    out = dict(K=K, Ps=g24["Ps"], flows_fw=g24["flows_fw"], flows_bw=g24["flows_bw"], masks=g24["masks"],
               ts=ts.astype(np.int32), max_t=np.int32(MAX_T), lambda_geo=np.float64(LAMBDA_GEO), given=np.float64(GIVEN))
    pts = scene_points(g24, ray_utils)
    out.update(pts)
    for tag, idx in (("fw", np.minimum(ts + 1, MAX_T)), ("bw", np.maximum(ts - 1, 0))):
        xyz = pts["xyz_" + tag]
        assert xyz.dtype == np.float32 and not np.isnan(xyz).any()
        out["world_" + tag] = reference_world(xyz, K, ray_utils)
        out["uv64_" + tag], out["depth64_" + tag] = float64_uv(xyz, K, Ps, idx, ray_utils)
        induced = fnp.induced_flow(xyz, K4, Ps, ts, MAX_T, H, W, tag)
        assert not np.isnan(induced).any()
        gt = g24["flows_" + tag]
        gt_rad = fnp.maxrad(gt)
        out["given_ind_" + tag] = gt_rad
        out["img_gt_" + tag] = reference_images(flowlib, gt)
        out["img_gt_" + tag + "_given"] = reference_images(flowlib, gt, GIVEN)
        out["img_ind_" + tag] = reference_images(flowlib, induced)
        out["img_ind_" + tag + "_given"] = reference_images(flowlib, induced, gt_rad)
        known = fnp.known(induced)
        print(f"{tag}: valid pixels per frame {known.reshape(F, -1).sum(1).tolist()} of {H * W}; depth64 > 0: "
              f"{(out['depth64_' + tag] > 0).sum(1).tolist()}")
    out["flow_fw_l"], out["flow_bw_l"] = (np.float64(v) for v in reference_flow_terms(pts, g24, ref_losses))
    print("flow_fw_l", out["flow_fw_l"], "flow_bw_l", out["flow_bw_l"])
    path = os.path.join(HERE, "g26_flow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300_000


if __name__ == "__main__":
    main()
