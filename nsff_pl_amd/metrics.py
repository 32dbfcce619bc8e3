"""The reference's quality metrics (metrics.py:6-49): ``mse``, ``psnr``, ``ssim`` and ``lpips`` with the reference's signatures,
and ``ssim_maps`` / ``lpips_frames`` for batches of frames.

``ssim`` is what the reference computes, which is NOT the standard SSIM: the reference calls kornia 0.5.4's
``ssim_loss(gt, pred, window_size=11, reduction='none')`` -- ``loss = clamp((1 - ssim) / 2, 0, 1)`` per pixel and channel --
and returns ``1 - loss``, i.e. ``(1 + ssim) / 2`` wherever ssim >= -1 (so 0.5 where standard SSIM is 0).  The published
numbers of BASELINE.md (0.9672 full frame, 0.9321 inside the dynamic mask) are on this scale.  The map, its reductions and
the channel-mean map of hard sampling come from one HIP launch (``nsff_ssim``, csrc/metrics.hip); there is no CPU path.

``lpips`` (metrics.py:36-49) takes an :class:`nsff_pl_amd.lpips.LPIPS` as its ``lpips_model`` -- LPIPS 0.1, AlexNet, spatial,
``normalize=True`` as the reference calls it -- and runs the network in one ``nsff_lpips`` call (csrc/lpips.hip).  The trained
weights come from the caller; values on them are unpinned (the arithmetic is pinned on seeded random weights).

``finish_frames`` / ``psnr_frames`` are the per-frame finishing work of the reference's eval.py for F frames at once
(``nsff_frame_finish``, csrc/metrics.hip): the clipped image, the 8-bit image eval.py writes, the squared-error sums behind
``metrics.psnr`` over the whole frame and over a mask, and the normalised 8-bit depth of ``utils/visualization.visualize_depth``
-- no boolean indexing, no host synchronisation.
"""
import torch

from . import _lib


def _check_window(window_size):
    if int(window_size) != 11:
        raise ValueError(f"ssim: window_size={window_size} is not supported (the gfx950 kernel is built for the reference's "
                         "window_size=11)")


def _check_reduction(reduction):
    if reduction not in ("mean", "none"):
        raise ValueError(f"ssim: reduction={reduction!r} is not supported ('mean' or 'none', as the reference's metrics.ssim)")


def mse(image_gt, image_pred, valid_mask=None, reduction='mean'):
    """metrics.py:6-12."""
    value = (image_gt - image_pred) ** 2
    if valid_mask is not None:
        value = value[valid_mask]
    if reduction == 'mean':
        return torch.mean(value)
    return value


def psnr(image_gt, image_pred, valid_mask=None, reduction='mean'):
    """metrics.py:15-16."""
    return -10 * torch.log10(mse(image_gt, image_pred, valid_mask, reduction))


def ssim(image_gt, image_pred, valid_mask=None, window_size=11, reduction='mean'):
    """metrics.py:19-33: image_gt / image_pred (H, W, 3) fp32 on the GPU, valid_mask (H, W) bool or None.

    reduction='mean': the scalar ``1 - mean(loss)`` over the (masked) pixels and channels (device tensor, fp32);
    reduction='none': ``1 - loss``, (H, W, 3) -- or (n, 3) for the n pixels of valid_mask.  See the module docstring for the
    scale of this value."""
    _check_window(window_size)
    _check_reduction(reduction)
    if image_gt.dim() != 3 or image_gt.shape[-1] != 3:
        raise RuntimeError(f"ssim: need (H, W, 3) images, got {tuple(image_gt.shape)}")
    gt, pred = image_gt.unsqueeze(0).contiguous(), image_pred.unsqueeze(0).contiguous()
    H, W = int(gt.shape[1]), int(gt.shape[2])
    if reduction == 'none':
        loss = torch.empty_like(gt)
        _lib.ssim(gt, pred, map=loss)
        value = 1 - loss[0]
        return value if valid_mask is None else value[valid_mask]
    sums = torch.empty(1, 3, dtype=torch.float64, device=gt.device)
    mask = None if valid_mask is None else valid_mask.reshape(1, H * W).to(torch.uint8).contiguous()
    _lib.ssim(gt, pred, mask=mask, sums=sums)
    if valid_mask is None:
        return (1 - sums[0, 0] / (3 * H * W)).float()
    return (1 - sums[0, 1] / (3 * sums[0, 2])).float()


def ssim_maps(gt, pred, valid_mask=None, window_size=11):
    """Batched form for F frames: gt / pred (F, H, W, 3), valid_mask (F, H, W) or None, one launch.

    Returns ``(ssim_map, frame_ssim, frame_ssim_mask)``: the reference's ``ssim(..., reduction='none')`` of every frame
    (F, H, W, 3), its ``reduction='mean'`` per frame (F,), and the same over each frame's valid_mask (F,; None without a
    mask; NaN for a frame whose mask is empty) -- all fp32."""
    _check_window(window_size)
    gt, pred = gt.contiguous(), pred.contiguous()
    F, H, W = (int(v) for v in gt.shape[:3])
    loss = torch.empty_like(gt)
    sums = torch.empty(F, 3, dtype=torch.float64, device=gt.device)
    mask = None if valid_mask is None else valid_mask.reshape(F, H * W).to(torch.uint8).contiguous()
    _lib.ssim(gt, pred, mask=mask, map=loss, sums=sums)
    frame = (1 - sums[:, 0] / (3 * H * W)).float()
    frame_mask = None if mask is None else (1 - sums[:, 1] / (3 * sums[:, 2])).float()
    return 1 - loss, frame, frame_mask


@torch.no_grad()
def lpips(lpips_model, image_gt, image_pred, valid_mask=None, reduction='mean'):
    """metrics.py:36-49: image_gt / image_pred (H, W, 3) fp32 in [0, 1] on the GPU, valid_mask (H, W) bool or None.

    reduction='mean': the mean of the spatial map over the (masked) pixels -- a device scalar (fp32) from the kernel's fp64 sums,
    no boolean indexing; NaN for a mask without a pixel, as the reference's mean of an empty selection.  Any other reduction:
    the map (H, W), or its (n,) selection by valid_mask."""
    if image_gt.dim() != 3 or image_gt.shape[-1] != 3:
        raise RuntimeError(f"lpips: need (H, W, 3) images, got {tuple(image_gt.shape)}")
    gt, pred = image_gt.unsqueeze(0), image_pred.unsqueeze(0)
    H, W = int(gt.shape[1]), int(gt.shape[2])
    if reduction != 'mean':
        value, _ = lpips_model.score(gt, pred, normalize=True)
        return value[0] if valid_mask is None else value[0][valid_mask]
    _, sums = lpips_model.score(gt, pred, valid=None if valid_mask is None else valid_mask.reshape(1, H, W), want_map=False,
                                want_sums=True, normalize=True)
    if valid_mask is None:
        return (sums[0, 0] / (H * W)).float()
    return (sums[0, 1] / sums[0, 2]).float()


@torch.no_grad()
def lpips_frames(model, gt, pred, valid_mask=None):
    """Batched form for F frames: gt / pred (F, H, W, 3) in [0, 1], valid_mask (F, H, W) or None, one ``nsff_lpips`` call whose
    launch count does not depend on F.

    Returns ``(lpips_map, frame_lpips, frame_lpips_mask)``: the spatial map (F, H, W), its mean per frame (F,), and the mean over
    each frame's valid_mask (F,; None without a mask; NaN for a frame whose mask is empty) -- all fp32."""
    F, H, W = (int(v) for v in gt.shape[:3])
    value, sums = model.score(gt, pred, valid=valid_mask, want_sums=True, normalize=True)
    frame = (sums[:, 0] / (H * W)).float()
    frame_mask = None if valid_mask is None else (sums[:, 1] / sums[:, 2]).float()
    return value, frame, frame_mask


def _frames4(t, what, last):
    if t.dim() != 4 or t.shape[-1] != last:
        raise RuntimeError(f"{what}: need (F, H, W, {last}) frames, got {tuple(t.shape)}")
    return t.contiguous()


def finish_frames(rgb, gt=None, valid_mask=None, depth=None, lut=None, images=True, scratch=None):
    """eval.py's finishing work on F frames in one ``nsff_frame_finish`` call (two launches, no host sync).

    rgb (F, H, W, 3) fp32, the raw ``rgb_fine``; gt (F, H, W, 3) fp32; valid_mask (F, H, W) bool / uint8, non-zero = the pixel
    counts (eval.py passes ``mask == 0``); depth (F, H, W) fp32; lut (256, 3) uint8, the colour table that stands for
    ``cv2.applyColorMap``.  Returns a dict of GPU tensors:

    * ``rgb_clipped`` (F, H, W, 3) fp32 and ``rgb_u8`` (F, H, W, 3) uint8 = ``(255 * clip(rgb, 0, 1)).astype(uint8)`` (eval.py:222-223)
      -- unless ``images=False``;
    * with gt: ``sums`` (F, 3) fp64 = [sum of (gt - clip(rgb))**2, the same over the valid pixels, valid pixels] (see
      :func:`psnr_from_sums`);
    * with depth: ``depth_range`` (F, 2) fp32, min and max of ``nan_to_num(depth)`` per frame, and ``depth_u8`` (F, H, W) uint8, the
      index image of ``visualize_depth``; with lut as well ``depth_rgb_u8`` (F, H, W, 3) uint8 = ``lut[depth_u8]``.

    scratch: a zeroed uint8 tensor of ``_lib.frame_finish_scratch_bytes(F, H, W)`` bytes that callers in a loop may keep."""
    rgb = _frames4(rgb, "finish_frames: rgb", 3)
    F, H, W = (int(v) for v in rgb.shape[:3])
    dev = rgb.device
    out = {}
    if images:
        out["rgb_clipped"] = torch.empty_like(rgb)
        out["rgb_u8"] = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    if gt is not None:
        gt = _frames4(gt, "finish_frames: gt", 3)
        out["sums"] = torch.empty(F, 3, dtype=torch.float64, device=dev)
    elif valid_mask is not None:
        raise ValueError("finish_frames: valid_mask selects the pixels of the error sums and needs gt")
    if valid_mask is not None:
        valid_mask = valid_mask.reshape(F, H, W)
        valid_mask = (valid_mask if valid_mask.dtype in (torch.bool, torch.uint8) else valid_mask != 0).contiguous()
    if depth is not None:
        depth = depth.reshape(F, H, W).contiguous()
        out["depth_range"] = torch.empty(F, 2, dtype=torch.float32, device=dev)
        out["depth_u8"] = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
        if lut is not None:
            lut = torch.as_tensor(lut).to(device=dev, dtype=torch.uint8).reshape(256, 3).contiguous()
            out["depth_rgb_u8"] = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    if not out:
        raise ValueError("finish_frames: nothing to compute (images=False without gt or depth)")
    _lib.frame_finish(rgb, gt=gt, valid=valid_mask, depth=depth, lut=lut if "depth_rgb_u8" in out else None, scratch=scratch, **out)
    return out


def psnr_from_sums(sums, n_pixels):
    """``(psnr (F,), psnr_valid (F,))`` fp32 from the ``sums`` of :func:`finish_frames`: ``-10 log10(sum / count)`` in fp64 with
    ``count = 3 * n_pixels`` and ``3 * valid pixels``; NaN where a frame has no valid pixel (the reference's ``mean()`` of an empty
    selection)."""
    whole = -10 * torch.log10(sums[:, 0] / (3 * n_pixels))
    valid = -10 * torch.log10(sums[:, 1] / (3 * sums[:, 2]))
    return whole.float(), valid.float()


def psnr_frames(gt, rgb, valid_mask=None):
    """metrics.psnr(gt, clip(rgb, 0, 1)) of F frames -- over the whole frame and over valid_mask -- from one pass over the images:
    ``(psnr (F,), psnr_valid (F,))`` fp32 on the GPU; psnr_valid is NaN for a frame without a valid pixel (and without a mask)."""
    out = finish_frames(rgb, gt=gt, valid_mask=valid_mask, images=False)
    return psnr_from_sums(out["sums"], int(rgb.shape[1]) * int(rgb.shape[2]))
