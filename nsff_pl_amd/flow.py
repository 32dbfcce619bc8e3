"""Induced optical flow of rendered frames: what the reference's ``test.ipynb`` does with the test-time outputs ``xyz_fw`` /
``xyz_bw`` (rendering.py:280-287) -- project them into the neighbouring frame, subtract the pixel, colour the result with
``flowlib.flow_to_image`` and compare it with the dataset's flow -- on the GPU, for F frames and both directions per call
(``nsff_flow_maps``, csrc/flow.hip; there is no CPU path).

* :func:`induced_flow`   -- ``xyz_fw`` / ``xyz_bw`` -> pixel motion (F, H, W, 2), the geometric loss's projection (losses.py:99-116):
                            a pixel that the loss would leave out (behind the target camera, or no neighbouring frame on that side)
                            is :data:`UNKNOWN` in both components, which the Middlebury convention (``|.| > 1e7``) calls unknown.
* :func:`flow_to_image`  -- ``flowlib.flow_to_image`` (flowlib.py:132-239): (F, H, W, 2) -> (F, H, W, 3) uint8, with the frame's own
                            maximum radius or a given one (so that a prediction and its ground truth share a scale).
* :func:`flow_epe`       -- end-point error sums and counts per frame over [all pixels, mask != 0, mask == 0];
  :func:`epe_from_sums`  -- their means (NaN where nothing was counted).

Two divergences from flowlib, both on values it handles badly: ``flow_error`` zeroes the prediction only where the ground truth is
unknown -- here a pixel where EITHER side is unknown (or NaN) is left out, and the counts say how many remain; ``flow_to_image``'s
``max(-1, np.max(rad))`` is -1 when any radius is NaN and flips every colour -- here a NaN pixel is simply unknown (black).
"""
import numpy as np
import torch

from . import _lib

UNKNOWN = _lib.FLOW_UNKNOWN


def _maps(t, what, last=2, gpu=True):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{what}: need a tensor, got {type(t).__name__}")
    if t.dim() != 4 or t.shape[-1] != last:
        raise RuntimeError(f"{what}: need (F, H, W, {last}) maps, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: need float32, got {t.dtype}")
    if gpu:
        _lib.require_gpu_tensor(t, what)
    return t.contiguous()


def _host(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def induced_flow(xyz_fw, xyz_bw, K, Ps, ts, max_t, img_wh):
    """``{'flow_fw', 'flow_bw'}``, each (F, H, W, 2) fp32 on the GPU (only the directions whose points are given).

    xyz_fw / xyz_bw: (F, H*W, 3) fp32 NDC points of F whole frames -- (H*W, 3) for one -- or None; K (3,3) or (1,3,3) intrinsics;
    Ps (N,3,4) or (1,N,3,4) world -> pixel matrices (:func:`nsff_pl_amd.frames.projection_matrices`); ts: the time index of every
    frame -- an int, a list or an (F,) tensor; max_t = N_frames - 1; img_wh = (W, H)."""
    w, h = (int(v) for v in img_wh)
    pts = {}
    for name, x in (("xyz_fw", xyz_fw), ("xyz_bw", xyz_bw)):
        if x is None:
            continue
        if not isinstance(x, torch.Tensor):
            raise RuntimeError(f"induced_flow: {name} must be a tensor, got {type(x).__name__}")
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[1] != h * w or x.shape[2] != 3:
            raise RuntimeError(f"induced_flow: {name} must be (F, H*W, 3) = (F, {h * w}, 3) for img_wh {(w, h)}, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"induced_flow: {name} must be float32, got {x.dtype}")
        _lib.require_gpu_tensor(x, f"induced_flow: {name}")
        pts[name] = x.contiguous()
    if not pts:
        raise ValueError("induced_flow: neither xyz_fw nor xyz_bw is given")
    F = {int(x.shape[0]) for x in pts.values()}
    if len(F) != 1:
        raise RuntimeError(f"induced_flow: xyz_fw and xyz_bw hold different numbers of frames {sorted(F)}")
    F = F.pop()
    dev = next(iter(pts.values())).device
    K = _host(K)
    if K.shape == (1, 3, 3):
        K = K[0]
    if K.shape != (3, 3):
        raise RuntimeError(f"induced_flow: K must be (3,3) or (1,3,3), got {K.shape}")
    if not isinstance(Ps, torch.Tensor):
        Ps = torch.as_tensor(np.asarray(Ps), dtype=torch.float32)
    if Ps.dim() == 4 and Ps.shape[0] == 1:
        Ps = Ps[0]
    if Ps.dim() != 3 or tuple(Ps.shape[1:]) != (3, 4):
        raise RuntimeError(f"induced_flow: Ps must be (N,3,4) or (1,N,3,4), got {tuple(Ps.shape)}")
    max_t = int(max_t)
    if not 0 <= max_t < Ps.shape[0]:
        raise ValueError(f"induced_flow: max_t = {max_t} is outside the {Ps.shape[0]} projection matrices")
    Ps = Ps.to(device=dev, dtype=torch.float32).contiguous()
    if isinstance(ts, torch.Tensor):
        ts = ts.reshape(-1).to(device=dev, dtype=torch.int32)
    else:
        host_ts = np.asarray(ts, dtype=np.int64).reshape(-1)
        if ((host_ts < 0) | (host_ts > max_t)).any():
            raise ValueError(f"induced_flow: ts {host_ts.tolist()} outside 0 .. max_t = {max_t}")
        ts = torch.as_tensor(host_ts, dtype=torch.int32).to(dev)
    if ts.numel() == 1 and F > 1:
        ts = ts.expand(F)
    if ts.numel() != F:
        raise RuntimeError(f"induced_flow: {F} frames need {F} time indices, got {ts.numel()}")
    ts = ts.contiguous()
    out = {("flow" + name[3:]): torch.empty(F, h, w, 2, dtype=torch.float32, device=dev) for name in pts}
    _lib.flow_maps(F, h, w, xyz=(pts.get("xyz_fw"), pts.get("xyz_bw")), K4=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), Ps=Ps, ts=ts,
                   max_t=max_t, flow=(out.get("flow_fw"), out.get("flow_bw")))
    return out


def _scale(maxrad, F, dev, what):
    """(F, 2, 2) fp32 scale table of nsff_flow_maps from a scalar or (F,) maxrad (every entry of a frame alike)."""
    if isinstance(maxrad, torch.Tensor):
        _lib.require_gpu_tensor(maxrad, what)
        m = maxrad.to(torch.float32).reshape(-1)
    else:
        m = torch.as_tensor(np.asarray(maxrad, dtype=np.float32).reshape(-1)).to(dev)
    if m.numel() not in (1, F):
        raise RuntimeError(f"{what}: maxrad must be a scalar or ({F},) values, got {m.numel()}")
    return m.reshape(-1, 1, 1).expand(F, 2, 2).contiguous()


def flow_to_image(flow, maxrad=None, scratch=None):
    """``flowlib.flow_to_image`` of (F, H, W, 2) fp32 flows -- (H, W, 2) for one -- on the GPU: ``(image_u8, maxrad)``, (F, H, W, 3)
    uint8 and the (F,) fp32 radius each frame was scaled by: its own largest ``sqrt(u^2 + v^2)`` over the known pixels, or the given
    ``maxrad`` (a scalar or (F,) values).  Unknown (``|.| > 1e7``) and NaN pixels are black; a zero field is white."""
    single = isinstance(flow, torch.Tensor) and flow.dim() == 3 and flow.shape[-1] == 2
    flow = _maps(flow.unsqueeze(0) if single else flow, "flow_to_image: flow")
    F, H, W = (int(v) for v in flow.shape[:3])
    image = torch.empty(F, H, W, 3, dtype=torch.uint8, device=flow.device)
    if maxrad is None:
        rad = torch.empty(F, 2, 2, dtype=torch.float32, device=flow.device)
        _lib.flow_maps(F, H, W, flow=(flow, None), maxrad=rad, image=(image, None), scratch=scratch)
    else:
        rad = _scale(maxrad, F, flow.device, "flow_to_image")
        _lib.flow_maps(F, H, W, flow=(flow, None), scale=rad, image=(image, None))
    return (image[0], rad[0, 0, 0]) if single else (image, rad[:, 0, 0])


def flow_epe(gt, pred, mask=None, scratch=None):
    """End-point error of (F, H, W, 2) fp32 flows: ``(sums (F, 3) fp64, counts (F, 3) int64)`` on the GPU for [all counted pixels, those
    with mask != 0 (dynamic), those with mask == 0 (static)]; without a mask the last two stay 0.  A pixel counts when both flows
    are known (``|.| <= 1e7``, not NaN) and the ground truth is non-zero in a component (``flowlib.flow_error``)."""
    _maps(gt, "flow_epe: gt", gpu=False), _maps(pred, "flow_epe: pred", gpu=False)       # shapes first, by name
    gt, pred = _maps(gt, "flow_epe: gt"), _maps(pred, "flow_epe: pred")
    if gt.shape != pred.shape:
        raise RuntimeError(f"flow_epe: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} differ in shape")
    F, H, W = (int(v) for v in gt.shape[:3])
    if mask is not None:
        _lib.require_gpu_tensor(mask, "flow_epe: mask")
        if mask.numel() != F * H * W:
            raise RuntimeError(f"flow_epe: mask must be ({F}, {H}, {W}), got {tuple(mask.shape)}")
        mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).reshape(F, H, W).contiguous()
    sums = torch.empty(F, 2, 3, dtype=torch.float64, device=gt.device)
    counts = torch.empty(F, 2, 3, dtype=torch.int64, device=gt.device)
    _lib.flow_maps(F, H, W, flow=(pred, None), gt=(gt, None), mask=mask, epe_sums=sums, epe_counts=counts, scratch=scratch)
    return sums[:, 0], counts[:, 0]


def epe_from_sums(sums, counts):
    """Mean end-point error, fp64, NaN where nothing was counted."""
    return torch.where(counts > 0, sums / counts.clamp(min=1), torch.full_like(sums, float("nan")))
