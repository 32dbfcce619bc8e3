"""From decoded frames to what a training run needs: the ray bank's records and the loss's projection matrices.

The reference builds both in its dataset constructor (datasets/monocular.py:127-187), frame by frame on the CPU, after it has
decoded and resized the files.  Decoding and resizing stay with the caller; everything after them is here:

* :func:`projection_matrices` -- ``Ks`` (1,3,3) and ``Ps`` (1,F,3,4), monocular.py:127-134, on the host in float64;
* :func:`build_records`       -- the (F, H*W, 16) records of monocular.py:136-184 for all frames in ONE launch
                                 (``nsff_ray_records``): NDC rays (the arithmetic of :func:`evaluate.frame_rays`, bit for bit),
                                 rgb, t, disparity, mask, ``uv + flow_fw``, ``uv + flow_bw``.

Inputs are GPU tensors already at the target resolution, channels LAST: images (F,H,W,3) uint8 or fp32 in [0,1], disparities
(F,H,W) fp32, masks (F,H,W) uint8 or fp32, flows (F,H,W,2) fp32 in pixels.  uint8 values are divided by 255 on the device, as
torchvision's ``ToTensor`` does.  ``sampling.RayBank.from_frames`` wraps both functions.
"""
import numpy as np
import torch

from . import _lib


def _poses_f32(poses):
    poses = torch.as_tensor(np.asarray(poses.detach().cpu() if isinstance(poses, torch.Tensor) else poses), dtype=torch.float32)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"poses must be (N_frames, 3, 4) camera-to-world matrices, got {tuple(poses.shape)}")
    return poses


def projection_matrices(K, poses):
    """(Ks (1,3,3), Ps (1,F,3,4)) fp32 on the CPU, the world -> pixel matrices the geometric loss projects with (what
    monocular.py:127-134 computes).  A pose [R | t] maps camera to world, so world -> camera is [R^-1 | -R^-1 t]; the poses' camera
    axes are x right, y up, z backwards while a pinhole K expects y down and z forwards, hence diag(1, -1, -1) in between:
    Ps[t] = K diag(1,-1,-1) [R^-1 | -R^-1 t].  float64 throughout, rounded once."""
    K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    poses = np.asarray(poses.detach().cpu() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64)
    if K.shape != (3, 3) or poses.ndim != 3 or poses.shape[1:] != (3, 4):
        raise ValueError(f"projection_matrices: K must be (3,3) and poses (N_frames,3,4), got {K.shape} and {poses.shape}")
    R_inv = np.linalg.inv(poses[:, :, :3])             # = R^T for a rotation; the inverse keeps a scaled or sheared pose exact
    w2c = np.concatenate([R_inv, -R_inv @ poses[:, :, 3:]], axis=2)
    Ps = K @ np.diag([1.0, -1.0, -1.0]) @ w2c
    return torch.tensor(K, dtype=torch.float32)[None], torch.tensor(Ps, dtype=torch.float32)[None]


def _stack(x, what, none_is_zero=False):
    """A list of per-frame tensors -> one stacked tensor (a copy).  none_is_zero (the two flow lists only): a None entry stands
    for the flow a frame does not have and becomes zeros; anywhere else a None entry is refused."""
    if isinstance(x, (list, tuple)):
        some = next((f for f in x if f is not None), None)
        if some is None and none_is_zero:
            return None
        if not all(isinstance(f, torch.Tensor) or (f is None and none_is_zero) for f in x):
            raise TypeError(f"build_records: every entry of the {what} list must be a tensor"
                            + (" or None" if none_is_zero else ""))
        x = torch.stack([torch.zeros_like(some) if f is None else f for f in x])
    return x


def frame_table(poses, device):
    """(F, 16) fp32 on `device`: row-major c2w | shift_near = -min(-1, c2w[2,3]) (monocular.py:152) | 3 unused."""
    poses = _poses_f32(poses)
    table = torch.zeros(poses.shape[0], _lib.FRAME_TABLE)
    table[:, :12] = poses.reshape(-1, 12)
    table[:, 12] = -torch.clamp(poses[:, 2, 3], max=-1.0)
    return table.to(device)


def build_records(K, poses, images, disps, masks, flows_fw=None, flows_bw=None, out=None, first_frame=0, n_frames=None,
                  near=1.0):
    """(F, H*W, 16) fp32 ray records on the inputs' device, one ``nsff_ray_records`` launch.

    K (3,3); poses (F,3,4); images (F,H,W,3) uint8 / fp32; disps (F,H,W) fp32; masks (F,H,W) uint8 / fp32; flows_fw / flows_bw
    (F,H,W,2) fp32 or None (zero flow) -- each stacked or a list of F per-frame tensors (a None entry of a flow list is zero
    flow).  A list is stacked first, one extra copy of that input on the device: pass stacked tensors to avoid it.
    Frame F-1's forward and frame 0's backward flow are taken as zero whatever is passed there.  ``out``: write into this
    (F, H*W, 16) tensor; ``first_frame`` / ``n_frames``: only that range of frames is built (the rest of ``out`` is left alone).
    """
    images, disps, masks = _stack(images, "images"), _stack(disps, "disps"), _stack(masks, "masks")
    flows_fw, flows_bw = _stack(flows_fw, "flows_fw", True), _stack(flows_bw, "flows_bw", True)
    for t, what in ((images, "images"), (disps, "disps"), (masks, "masks")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"build_records: {what} must be a tensor or a list of per-frame tensors")
    if images.dim() != 4 or images.shape[-1] != 3:
        hint = " -- this looks channels-first (F,3,H,W): permute(0, 2, 3, 1) it" if images.dim() == 4 and images.shape[1] == 3 else ""
        raise ValueError(f"build_records: images must be channels-last (F,H,W,3), got {tuple(images.shape)}{hint}")
    F, H, W = (int(v) for v in images.shape[:3])
    for t, what, shape in ((disps, "disps", (F, H, W)), (masks, "masks", (F, H, W)), (flows_fw, "flows_fw", (F, H, W, 2)),
                           (flows_bw, "flows_bw", (F, H, W, 2))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"build_records: {what} must be {shape} to go with images {tuple(images.shape)}, "
                             f"got {tuple(t.shape)}")
    K = torch.as_tensor(np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K), dtype=torch.float32)
    poses = _poses_f32(poses)
    if tuple(K.shape) != (3, 3) or poses.shape[0] != F:
        raise ValueError(f"build_records: K must be (3,3) and poses ({F},3,4), got {tuple(K.shape)} and {tuple(poses.shape)}")
    _lib.require_gpu_tensor(images, "build_records: images")
    dev = images.device
    for t, what in ((disps, "disps"), (masks, "masks"), (flows_fw, "flows_fw"), (flows_bw, "flows_bw"), (out, "out")):
        if t is not None:
            _lib.require_gpu_tensor(t, f"build_records: {what}")
            if t.device != dev:
                raise RuntimeError(f"build_records: {what} is on {t.device}, images on {dev}")
    if out is None:
        out = torch.empty(F, H * W, _lib.RAY_RECORD, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != (F, H * W, _lib.RAY_RECORD):
        raise ValueError(f"build_records: out must be ({F}, {H}*{W}, {_lib.RAY_RECORD}), got {tuple(out.shape)}")
    count = F - first_frame if n_frames is None else n_frames
    _lib.ray_records([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], frame_table(poses, dev), images.contiguous(), disps.contiguous(),
                     masks.contiguous(), None if flows_fw is None else flows_fw.contiguous(),
                     None if flows_bw is None else flows_bw.contiguous(), near, first_frame, count, out)
    return out
