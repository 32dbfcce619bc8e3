"""The image panels of the reference trainer's validation step, composed on the GPU (train.py:209-235, 254-257).

After every validation frame the reference copies six full-frame fp32 tensors and the ground truth to the host and builds, with
numpy / cv2 / PIL / torchvision, what a person training a scene looks at:

* ``'reconstruction/decomposition'`` -- ``make_grid([gt, prediction, depth, transient alpha, static rgb, static depth, 1 - mask,
  -disparity], nrow=3)`` (train.py:224-233; the depth and mask tiles through ``utils/visualization.py:6-29``);
* ``'error_map/rmse'`` / ``'error_map/ssim'`` -- ``blend_images(prediction, visualize_depth(-map), 0.5)`` of the per-pixel RMSE
  and of the reference's SSIM map (train.py:215-219, utils/visualization.py:32-44);
* with ``--hard_sampling``, ``'misc/moving_ssim'``: the SSIM blend of the ray bank's middle frame (train.py:254-257).

Here all of it is one ``nsff_ssim`` launch (the loss map) and one ``nsff_val_panels`` call (two launches, csrc/metrics.hip) on
tensors that already sit on the GPU; the results are uint8 HWC images on the GPU (``.permute(0, 3, 1, 2)`` gives the CHW layout of
``SummaryWriter.add_image(..., dataformats='NCHW')``; the reference's float image is this byte / 255).  There is no CPU path.

Colour tables: ``lut_depth`` / ``lut_mask`` (256, 3) uint8 stand for ``cv2.applyColorMap(., COLORMAP_JET)`` / ``(., COLORMAP_BONE)`` and
are used as given, as in :func:`nsff_pl_amd.metrics.finish_frames` (the reference hands cv2's BGR bytes to PIL unchanged; pass
cv2's table for the reference's colours).  Without a table the index image is written to all three channels (grey panels).
"""
import torch

from . import _lib

TAGS = ("reconstruction/decomposition", "error_map/rmse", "error_map/ssim", "rmse_u8", "ssim_u8", "ranges")
SSIM_TAGS = ("error_map/ssim", "ssim_u8")
SSIM_MIN = 6                    # nsff_ssim's reflect padding needs H, W >= 6


def _lut(lut, dev):
    return None if lut is None else torch.as_tensor(lut).to(device=dev, dtype=torch.uint8).reshape(256, 3).contiguous()


def _field(t, F, n, last=None):
    if t is None:
        return None
    return t.to(torch.float32).reshape((F, n) if last is None else (F, n, last)).contiguous()


def scratch_bytes(F, H, W):
    """Bytes of the zeroed uint8 ``scratch`` tensor a caller in a loop may keep for F frames of H x W."""
    return _lib.val_panels_scratch_bytes(F, H, W)


def validation_panels(results, batch, img_wh, lut_depth=None, lut_mask=None, output_transient=True, scratch=None, want=None):
    """The panels of one validation frame -- or of F frames stacked along a leading dimension -- from ``render_rays``' test-time
    dict and the validation batch, all on the GPU.

    results: ``rgb_fine`` (H*W, 3), ``depth_fine`` (H*W) and, with output_transient, ``transient_alpha_fine``, ``_static_rgb_fine``,
    ``_static_depth_fine``; batch: ``rgbs`` (H*W, 3) and optionally ``mask`` (H*W; 0 static, 1 dynamic) and ``disp`` (H*W).  For F frames
    every tensor carries (F, H*W[, 3]).  img_wh = (W, H).  want: the tags to produce (default: all of :data:`TAGS`);
    ``'ranges'`` always comes along.

    Returns {tag: GPU tensor}: ``'reconstruction/decomposition'`` (F, GH, GW, 3) uint8 with GW = 3 (W + 2) + 2 and
    GH = rows (H + 2) + 2; ``'error_map/rmse'`` and ``'error_map/ssim'`` (F, H, W, 3) uint8; ``'rmse_u8'`` and ``'ssim_u8'``
    (F, H, W) uint8, the index images behind the two blends; ``'ranges'`` (F, 5, 2) fp32, min and max of [depth, static depth,
    -disp, -rmse, -ssim] after nan_to_num (rows of absent fields are NaN).  Frames below 6 x 6 have no SSIM (``nsff_ssim``'s
    limit): ``'error_map/ssim'`` and ``'ssim_u8'`` are refused there by name (the default asks for them); ``want`` without the two
    gives the rest."""
    W, H = (int(v) for v in img_wh)
    pred = results["rgb_fine"]
    _lib.require_gpu_tensor(pred, "validation_panels: rgb_fine")
    n = H * W
    if pred.numel() % (n * 3):
        raise ValueError(f"validation_panels: rgb_fine has {pred.numel()} values, not a multiple of {H} x {W} x 3")
    F, dev = pred.numel() // (n * 3), pred.device
    small = H < SSIM_MIN or W < SSIM_MIN
    want = set(TAGS if want is None else want) | {"ranges"}
    unknown = want - set(TAGS)
    if unknown:
        raise ValueError(f"validation_panels: unknown tags {sorted(unknown)} (one of {list(TAGS)})")
    refused = sorted(want & set(SSIM_TAGS)) if small else []
    if refused:
        raise ValueError(f"validation_panels: {refused} need frames of at least {SSIM_MIN} x {SSIM_MIN} pixels (the SSIM window's "
                         f"reflect padding), got {H} x {W}; pass want= without them for the other panels")
    pred = _field(pred, F, n, 3)
    gt = _field(batch["rgbs"], F, n, 3)
    kw = dict(gt=gt, depth=_field(results["depth_fine"], F, n), mask=_field(batch.get("mask"), F, n),
              disp=_field(batch.get("disp"), F, n), lut_depth=_lut(lut_depth, dev), lut_mask=_lut(lut_mask, dev))
    if output_transient:
        kw.update(transient_alpha=_field(results["transient_alpha_fine"], F, n), static_rgb=_field(results["_static_rgb_fine"], F, n, 3),
                  static_depth=_field(results["_static_depth_fine"], F, n))
    if want & set(SSIM_TAGS):
        loss = torch.empty(F, H, W, 3, dtype=torch.float32, device=dev)
        _lib.ssim(gt.view(F, H, W, 3), torch.clip(pred, 0, 1).view(F, H, W, 3), map=loss)     # train.py:211, 218
        kw["ssim_loss"] = loss
    n_tiles = 3 + (3 if output_transient else 0) + (kw["mask"] is not None) + (kw["disp"] is not None)
    GH, GW = _lib.panel_grid_shape(H, W, n_tiles)
    u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
    out = {"ranges": torch.full((F, 5, 2), float("nan"), dtype=torch.float32, device=dev)}
    names = {"reconstruction/decomposition": ("grid_u8", (F, GH, GW, 3)), "error_map/rmse": ("rmse_blend_u8", (F, H, W, 3)),
             "error_map/ssim": ("ssim_blend_u8", (F, H, W, 3)), "rmse_u8": ("rmse_u8", (F, H, W)), "ssim_u8": ("ssim_u8", (F, H, W))}
    for tag, (arg, shape) in names.items():
        if tag in want:
            out[tag] = kw[arg] = u8(*shape)
    _lib.val_panels(F, H, W, pred, ranges=out["ranges"], scratch=scratch, **kw)
    return out


def error_blend(gt, pred, kind="ssim", lut=None, clip_ssim=True):
    """``blend_images(clip(pred), visualize_depth(-map), 0.5)`` (utils/visualization.py:32-44) of F arbitrary frame pairs gt / pred
    (F, H, W, 3) fp32 (or one (H, W, 3) pair): (F, H, W, 3) uint8 on the GPU.  kind='rmse': the map of train.py:215; kind='ssim': the
    reference's SSIM map of train.py:218 -- of (gt, clip(pred)), or with clip_ssim=False of (gt, pred) as given, which is what
    train.py:252 feeds its 'misc/moving_ssim' panel.  The blended image is always the CLIPPED prediction's 8-bit image.  lut: the
    colour table of visualize_depth (None: grey)."""
    if kind not in ("ssim", "rmse"):
        raise ValueError(f"error_blend: kind={kind!r} is not one of 'ssim', 'rmse'")
    _lib.require_gpu_tensor(pred, "error_blend: pred")
    if gt.dim() == 3:
        gt, pred = gt.unsqueeze(0), pred.unsqueeze(0)
    if gt.dim() != 4 or gt.shape[-1] != 3 or pred.shape != gt.shape:
        raise ValueError(f"error_blend: need (F, H, W, 3) image pairs of one shape, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    gt, pred = gt.to(torch.float32).contiguous(), pred.to(torch.float32).contiguous()
    F, H, W = (int(v) for v in gt.shape[:3])
    dev = pred.device
    out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    ranges = torch.empty(F, 5, 2, dtype=torch.float32, device=dev)
    if kind == "rmse":
        _lib.val_panels(F, H, W, pred, gt=gt, lut_depth=_lut(lut, dev), ranges=ranges, rmse_blend_u8=out)
        return out
    if H < SSIM_MIN or W < SSIM_MIN:
        raise ValueError(f"error_blend: kind='ssim' needs frames of at least {SSIM_MIN} x {SSIM_MIN} pixels, got {H} x {W}")
    loss = torch.empty_like(gt)
    _lib.ssim(gt, torch.clip(pred, 0, 1) if clip_ssim else pred, map=loss)
    _lib.val_panels(F, H, W, pred, ssim_loss=loss, lut_depth=_lut(lut, dev), ranges=ranges, ssim_blend_u8=out)
    return out
