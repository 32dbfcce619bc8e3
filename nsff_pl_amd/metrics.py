"""The reference's quality metrics (metrics.py:6-33): ``mse``, ``psnr`` and ``ssim`` with the reference's signatures, and
``ssim_maps`` for batches of frames.

``ssim`` is what the reference computes, which is NOT the standard SSIM: the reference calls kornia 0.5.4's
``ssim_loss(gt, pred, window_size=11, reduction='none')`` -- ``loss = clamp((1 - ssim) / 2, 0, 1)`` per pixel and channel --
and returns ``1 - loss``, i.e. ``(1 + ssim) / 2`` wherever ssim >= -1 (so 0.5 where standard SSIM is 0).  The published
numbers of BASELINE.md (0.9672 full frame, 0.9321 inside the dynamic mask) are on this scale.  The map, its reductions and
the channel-mean map of hard sampling come from one HIP launch (``nsff_ssim``, csrc/metrics.hip); there is no CPU path.
LPIPS (metrics.py:36-51) needs AlexNet weights and is not provided.
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
