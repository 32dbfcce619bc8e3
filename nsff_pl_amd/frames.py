"""From decoded frames to what a training run needs: the ray bank's records and the loss's projection matrices.

The reference builds both in its dataset constructor (datasets/monocular.py:127-187), frame by frame on the CPU, after it has
decoded and resized the files.  Decoding stays with the caller; everything after it is here:

* :func:`resize_frames`       -- the reference's four resize statements on decoded frames at their native sizes
                                 (``nsff_frame_resize``, one launch per kind): :func:`resize_images` PIL's 8-bit LANCZOS byte
                                 for byte, :func:`resize_masks` PIL's NEAREST, :func:`resize_disps` cv2's INTER_NEAREST,
                                 :func:`resize_flows` ``flowlib.resize_flow``; :func:`scaled_intrinsics` is the K that goes
                                 with them (monocular.py:61-65).  The per-axis tables are built on the host once per
                                 (filter, n_in, n_out) and kept per device;
* :func:`projection_matrices` -- ``Ks`` (1,3,3) and ``Ps`` (1,F,3,4), monocular.py:127-134, on the host in float64;
* :func:`build_records`       -- the (F, H*W, 16) records of monocular.py:136-184 for all frames in ONE launch
                                 (``nsff_ray_records``): NDC rays (the arithmetic of :func:`evaluate.frame_rays`, bit for bit),
                                 rgb, t, disparity, mask, ``uv + flow_fw``, ``uv + flow_bw``.

:func:`build_records`' inputs are GPU tensors at the target resolution (what :func:`resize_frames` returns), channels LAST: images (F,H,W,3) uint8 or fp32 in [0,1], disparities
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


# ---- resizing decoded frames to the training resolution (csrc/resize.hip) ----
_TABLES = {}                    # (device, filter, n_in, n_out) -> (start, count, weights) on that device


def _table(dev, filt, n_in, n_out):
    """The (filter, n_in, n_out) table of one axis on `dev`: built once on the host (nsff_resize_table), then kept."""
    key = (str(dev), int(filt), int(n_in), int(n_out))
    if key not in _TABLES:
        _TABLES[key] = tuple(None if t is None else t.to(dev) for t in _lib.resize_table(filt, n_in, n_out))
    return _TABLES[key]


def _wh(img_wh, who):
    if not isinstance(img_wh, (tuple, list)) or len(img_wh) != 2 or not all(isinstance(v, (int, np.integer)) and v >= 1 for v in img_wh):
        raise ValueError(f"{who}: img_wh must be (width, height), two positive integers, got {img_wh!r}")
    return int(img_wh[0]), int(img_wh[1])


def _resize_stack(x, what, who):
    """One input kind as a stacked tensor: a list of per-frame tensors (all of one size) is stacked, one copy."""
    if isinstance(x, (list, tuple)):
        if not x or not all(isinstance(f, torch.Tensor) for f in x):
            raise TypeError(f"{who}: every entry of the {what} list must be a tensor")
        if len({tuple(f.shape) for f in x}) != 1:
            raise ValueError(f"{who}: the frames of the {what} list differ in shape: {sorted({tuple(f.shape) for f in x})}")
        x = torch.stack(list(x))
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{who}: {what} must be a tensor or a list of per-frame tensors")
    _lib.require_gpu_tensor(x, f"{who}: {what}")
    return x


def _resize(x, img_wh, filt, dtype, channels, what, who):
    """x (F, h, w[, C]) -> (F, H, W[, C]) with filter `filt`; an input already at img_wh comes back as a copy."""
    W, H = _wh(img_wh, who)
    x = _resize_stack(x, what, who)
    want = 3 if channels is None else 4
    if x.dim() != want or (channels is not None and x.shape[-1] not in channels):
        hint = ""
        if channels is not None and x.dim() == 4 and x.shape[1] in channels:
            hint = f" -- this looks channels-first (F,{x.shape[1]},h,w): permute(0, 2, 3, 1) it"
        shape = "(F,h,w)" if channels is None else f"(F,h,w,C) with C in {tuple(channels)}"
        raise ValueError(f"{who}: {what} must be channels-last {shape}, got {tuple(x.shape)}{hint}")
    if x.dtype != dtype:
        extra = " (the Lanczos rule is Pillow's 8-bit one: resize the decoded bytes, not ToTensor's floats)" if filt == _lib.RESIZE_LANCZOS_U8 else ""
        raise TypeError(f"{who}: {what} must be {dtype}, got {x.dtype}{extra}")
    F, h, w = (int(v) for v in x.shape[:3])
    if (w, h) == (W, H):
        return x.clone(memory_format=torch.contiguous_format)
    xt, yt = _table(x.device, filt, w, W), _table(x.device, filt, h, H)
    src = x.contiguous().reshape(F, h, w, -1)
    out = torch.empty((F, H, W) + tuple(x.shape[3:]), dtype=dtype, device=x.device)
    ratio = (np.float32(W / w), np.float32(H / h)) if filt == _lib.RESIZE_LINEAR_CV else (1.0, 1.0)
    _lib.frame_resize(filt, src, out.view(F, H, W, -1), xt, yt, ratio)
    return out


def resize_images(images, img_wh):
    """(F,h,w,C) uint8, C = 3 (or 1) -> (F,H,W,C) uint8 with img_wh = (W, H): PIL's ``img.resize(img_wh, Image.LANCZOS)``
    (monocular.py:146-147) byte for byte, both 8-bit passes in one launch.  Downscales up to 8x, any upscale."""
    return _resize(images, img_wh, _lib.RESIZE_LANCZOS_U8, torch.uint8, (1, 3), "images", "resize_images")


def resize_masks(masks, img_wh):
    """(F,h,w) uint8 -> (F,H,W) uint8: PIL's ``mask.resize(img_wh, Image.NEAREST)`` (monocular.py:162-163)."""
    return _resize(masks, img_wh, _lib.RESIZE_NEAREST_PIL, torch.uint8, None, "masks", "resize_masks")


def resize_disps(disps, img_wh):
    """(F,h,w) fp32 -> (F,H,W) fp32: ``cv2.resize(disp, img_wh, interpolation=cv2.INTER_NEAREST)`` (monocular.py:158-159)."""
    return _resize(disps, img_wh, _lib.RESIZE_NEAREST_CV, torch.float32, None, "disps", "resize_disps")


def resize_flows(flows, img_wh):
    """(F,h,w,2) fp32 -> (F,H,W,2) fp32: ``flowlib.resize_flow(flow, W, H)`` -- cv2's bilinear resize, then u *= W/w, v *= H/h
    (flowlib.py:320-338).  None passes through."""
    if isinstance(flows, (list, tuple)):                        # build_records' convention: a None entry is a frame without flow
        some = next((f for f in flows if f is not None), None)
        flows = None if some is None else [torch.zeros_like(some) if f is None else f for f in flows]
    if flows is None:
        return None
    return _resize(flows, img_wh, _lib.RESIZE_LINEAR_CV, torch.float32, (2,), "flows", "resize_flows")


def resize_frames(images, disps, masks, flows_fw=None, flows_bw=None, img_wh=None):
    """Decoded frames at their native sizes -> the dict ``build_records(K, poses, **d)`` takes, everything at img_wh = (W, H).
    Each kind may have its own source size; inputs are stacked GPU tensors or lists of per-frame tensors, channels last."""
    if img_wh is None:
        raise ValueError("resize_frames: img_wh = (width, height) is required")
    return dict(images=resize_images(images, img_wh), disps=resize_disps(disps, img_wh), masks=resize_masks(masks, img_wh),
                flows_fw=resize_flows(flows_fw, img_wh), flows_bw=resize_flows(flows_bw, img_wh))


def scaled_intrinsics(K_or_f, src_wh, img_wh):
    """(3,3) fp32 intrinsics at img_wh from the calibration at src_wh = (W, H), monocular.py:61-65: a focal length f gives
    [[f,0,W/2],[0,f,H/2],[0,0,1]] in fp32; a (3,3) K is taken as it is; then row 0 *= w/W and row 1 *= h/H."""
    (W, H), (w, h) = _wh(src_wh, "scaled_intrinsics"), _wh(img_wh, "scaled_intrinsics")
    if isinstance(K_or_f, torch.Tensor):
        K_or_f = K_or_f.detach().cpu().numpy()
    if np.ndim(K_or_f) == 0:
        f = float(K_or_f)
        K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=np.float32)
    else:
        K = np.array(K_or_f, dtype=np.float32)
        if K.shape != (3, 3):
            raise ValueError(f"scaled_intrinsics: K must be (3,3) or a focal length, got {K.shape}")
    K[0] *= w / W
    K[1] *= h / H
    return torch.from_numpy(K)
