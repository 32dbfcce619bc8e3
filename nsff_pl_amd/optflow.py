"""Dense optical flow between frames, on the GPU (``nsff_optflow``, csrc/optflow.hip; there is no CPU path).

The reference gets its ``flow_fw`` / ``flow_bw`` from RAFT (preprocess.py:106-120), a network whose weights this project can neither
ship nor run.  This module is a CLASSICAL STAND-IN, not RAFT's flow: TV-L1 (Zach, Pock and Bischof 2007, in the fixed-iteration
form of Sanchez, Meinhardt-Llopis and Facciolo, IPOL 2013) on a grey pyramid -- stencils and point-wise arithmetic only,
deterministic, no host synchronisation.  With it the chain images -> :func:`nsff_pl_amd.frames.resize_images` -> flow ->
:func:`nsff_pl_amd.motion.flow_consistency` -> :func:`nsff_pl_amd.motion.motion_masks` -> ray records needs no network; the
monocular disparity has a classical stand-in of its own, :mod:`nsff_pl_amd.depth`.

* :func:`optical_flow`   -- (P, H, W, 2) fp32: the pixel motion from ``images0[p]`` to ``images1[p]``, x first;
* :func:`sequence_flows` -- ``{'flows_fw', 'flows_bw'[, 'valid']}`` of F frames in the reference's convention, both directions as
                            one batch of 2 (F - 1) pairs;
* :func:`refine_flow`    -- the image-guided weighted median of a flow map (``nsff_flow_median``, csrc/flowmedian.hip): sharpens the
                            flow at motion edges that are image edges too; ``sequence_flows(refine=True)`` applies it.

Known limits.  A displacement beyond the pyramid's reach (a few pixels at the coarsest level, so roughly ``2 ** levels`` pixels) is
not found, and an untextured region has no data term: its flow is whatever the smoothness term fills in from its rim.  The
parameters are the IPOL article's defaults and are untuned on real sequences.  TV-L1 rounds a motion edge off; :func:`refine_flow`
moves it back to the image edge it belongs to, and gains nothing where the two sides of a motion edge have the same grey levels.
"""
import torch

from . import _lib, motion

MIN_SIZE = _lib.OPTFLOW_MIN_SIZE
DEFAULT_FUSED = bool(_lib.OPTFLOW_FUSED)      # the measured default route
TILE, K = _lib.OPTFLOW_TILE, _lib.OPTFLOW_K   # the fused route's tile side and iterations per launch on batches that fill the machine
SMALL_TILE, SMALL_K = 16, 2                   # ... and on batches that do not
SMALL_BELOW = 512                             # tiles of TILE x TILE pixels in the batch: two per compute unit
MEDIAN_MAX_RADIUS = _lib.FLOW_MEDIAN_MAX_RADIUS
DEFAULT_MEDIAN_TILED = bool(_lib.FLOW_MEDIAN_TILED)   # refine_flow's measured default route: 7 to 12 x the plain one at 512 x 288
GREY_SIGMA = 12.75                            # 0.05 of the grey stage's 0..255 scale, as nsff_pl_amd.depth.GREY_SIGMA


def default_route(n_pairs, H, W):
    """(tile, k) of the fused route that ``fused=None`` takes.  Measured at 512 x 288: on 58 pairs (8352
    tiles of 32 x 32) the whole call is fastest with (32, 3), 1.69 x the plain route; on one pair (144 tiles, fewer than compute
    units) with (16, 2), 1.13 x the plain route, where (32, 3) is slower than plain.  Where the better choice changes between those
    two sizes has not been measured; the switch stands at two 32 x 32 tiles per compute unit."""
    tiles = int(n_pairs) * (-(-int(H) // TILE)) * (-(-int(W) // TILE))
    return (TILE, K) if tiles >= SMALL_BELOW else (SMALL_TILE, SMALL_K)


def _images(images0, images1, who):
    for t, what in ((images0, "images0"), (images1, "images1")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {what}: need a tensor, got {type(t).__name__}")
        if t.dtype not in (torch.uint8, torch.float32):
            raise RuntimeError(f"{who}: {what}: need uint8 colour frames or float32 grey frames, got {t.dtype}")
        colour = t.dtype == torch.uint8
        if (colour and (t.dim() != 4 or t.shape[-1] != 3)) or (not colour and t.dim() != 3):
            hint = " -- this looks channels-first (P,3,H,W): permute(0, 2, 3, 1) it" if t.dim() == 4 and t.shape[1] == 3 else ""
            raise RuntimeError(f"{who}: {what}: need channels-last (P, H, W, 3) uint8 or grey (P, H, W) float32, got {tuple(t.shape)} "
                               f"{t.dtype}{hint}")
    if images0.dtype != images1.dtype:
        raise RuntimeError(f"{who}: images0 is {images0.dtype}, images1 {images1.dtype}")
    if images0.shape != images1.shape:
        raise RuntimeError(f"{who}: images0 {tuple(images0.shape)} and images1 {tuple(images1.shape)} differ in shape")
    if images0.shape[0] < 1 or min(images0.shape[1:3]) < MIN_SIZE:
        raise RuntimeError(f"{who}: need at least one pair of frames of {MIN_SIZE} x {MIN_SIZE} pixels or more, got {tuple(images0.shape)}")
    for t, what in ((images0, "images0"), (images1, "images1")):
        _lib.require_gpu_tensor(t, f"{who}: {what}")
    if images0.device != images1.device:
        raise RuntimeError(f"{who}: images0 is on {images0.device}, images1 on {images1.device}")
    return images0.contiguous(), images1.contiguous()


def _check_params(who, levels, warps, iters, lam, theta, tau):
    for name, v, top in (("levels", levels, 16), ("warps", warps, 1000), ("iters", iters, 100000)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
            raise ValueError(f"{who}: {name} must be an integer from 1 to {top}, got {v!r}")
    for name, v in (("lam", lam), ("theta", theta), ("tau", tau)):
        if not 0 < float(v) < float("inf"):
            raise ValueError(f"{who}: {name} must be a finite number > 0, got {v}")


def scratch_bytes(n_pairs, H, W, levels=5):
    """The size of the ``scratch`` tensor (uint8) that :func:`optical_flow` takes for this shape."""
    return _lib.optflow_scratch_bytes(n_pairs, H, W, levels)


def optical_flow(images0, images1, levels=5, warps=5, iters=30, lam=0.15, theta=0.3, tau=0.25, median=True, fused=None, scratch=None):
    """TV-L1 flow of P image pairs: (P, H, W, 2) fp32 on the GPU, the pixel motion from ``images0[p]`` to ``images1[p]``, x first.

    images0 / images1: (P, H, W, 3) uint8 frames as :func:`nsff_pl_amd.frames.resize_images` returns them (grey is
    ``0.299 R + 0.587 G + 0.114 B`` on the 0..255 scale), or grey (P, H, W) fp32 on that scale; 16 x 16 pixels and more.
    ``levels`` pyramid levels (clipped so that the coarsest keeps both sides >= 4), ``warps`` warps per level, ``iters`` iterations
    per warp; ``lam`` the data weight (larger: closer to the images, less smooth), ``theta`` the coupling and ``tau`` the dual step --
    the IPOL defaults, untuned on real sequences.  ``median``: a 3 x 3 median of the flow after every warp.  ``fused``: True runs
    the iterations several per launch on tiles held in LDS, False one per launch; both give the same bits, None picks the measured
    default (:func:`default_route`).  ``scratch``: a uint8 tensor of :func:`scratch_bytes` bytes, any content (a fresh one when None).
    Nothing synchronises: with a ``scratch`` of the caller's the call is capturable into a graph."""
    _check_params("optical_flow", levels, warps, iters, lam, theta, tau)
    images0, images1 = _images(images0, images1, "optical_flow")
    P, H, W = (int(v) for v in images0.shape[:3])
    flow = torch.empty(P, H, W, 2, dtype=torch.float32, device=images0.device)
    tile, k = default_route(P, H, W) if fused is None else (0, 0)
    return _lib.optflow(images0, images1, flow, levels=levels, warps=warps, iters=iters, lam=lam, theta=theta, tau=tau, median=median,
                        fused=DEFAULT_FUSED if fused is None else bool(fused), tile=tile, k=k, scratch=scratch)


def _check_refine(who, radius, sigma_i, sigma_s):
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= MEDIAN_MAX_RADIUS:
        raise ValueError(f"{who}: radius must be an integer from 1 to {MEDIAN_MAX_RADIUS}, got {radius!r}")
    for name, v in (("sigma_i", sigma_i), ("sigma_s", sigma_s)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < float(v) <= 3.0e38:
            raise ValueError(f"{who}: {name} must be a finite number > 0, got {v!r}")


def refine_flow(flows, images_or_grey, valid=None, radius=7, sigma_i=GREY_SIGMA, sigma_s=7.0, tiled=None):
    """The image-guided weighted median of ``flows`` (P, H, W, 2) fp32 ("Classic+NL", Sun, Roth and Black 2010; one pass): a new
    (P, H, W, 2) fp32 tensor in which each flow component is the weighted median of its neighbours in a (2 radius + 1)^2 window.  A
    neighbour weighs ``1 / ((1 + ((grey_q - grey_p) / sigma_i)^2) (1 + |q - p|^2 / sigma_s^2))``, rounded to an integer of 16 bits, and
    nothing where its own flow is unknown (NaN or beyond 1e7) or ``valid`` is 0 there; the centre always votes, so a pixel whose flow
    failed the check is filled in from neighbours that look like it.  A pixel whose own flow is unknown is copied.

    ``images_or_grey``: the frames the flows START from, (P, H, W, 3) uint8 -- grey is the grey stage's ``0.299 R + 0.587 G +
    0.114 B`` on the 0..255 scale -- or a finite guide (P, H, W) fp32; ``sigma_i`` is in the guide's units (12.75 is 0.05 of 0..255).
    ``valid`` (P, H, W) uint8 or None: one direction of :func:`nsff_pl_amd.motion.flow_consistency`, e.g. ``valid[:, 0]`` for forward
    flows.  ``radius`` 1 .. 7.  ``tiled``: True holds tiles in LDS and a pixel's weights in registers, False is the kernel that restates
    the definition; both give the same bits, None picks the measured default.  One launch, nothing synchronises, capturable.
    The weights are starting values that nobody has tuned on real sequences; the filter gains nothing at a motion edge that is no
    image edge."""
    who = "refine_flow"
    _check_refine(who, radius, sigma_i, sigma_s)
    if not isinstance(flows, torch.Tensor):
        raise RuntimeError(f"{who}: flows: need a tensor, got {type(flows).__name__}")
    if flows.dtype != torch.float32 or flows.dim() != 4 or flows.shape[-1] != 2 or flows.numel() == 0:
        raise RuntimeError(f"{who}: flows: need (P, H, W, 2) float32 with P, H, W >= 1, got {tuple(flows.shape)} {flows.dtype}")
    _lib.require_gpu_tensor(flows, f"{who}: flows")
    shape, dev = tuple(int(v) for v in flows.shape[:3]), flows.device
    guide = motion._guide(who, images_or_grey, shape, dev, "the flows")
    valid = motion._uint8_maps(who, "valid", valid, shape, dev)
    return _lib.flow_median(flows.contiguous(), motion._grey(guide), torch.empty(shape + (2,), dtype=torch.float32, device=dev), valid=valid,
                            radius=radius, sigma_i=sigma_i, sigma_s=sigma_s, tiled=DEFAULT_MEDIAN_TILED if tiled is None else bool(tiled))


def sequence_flows(images, check=True, alpha=0.01, beta=0.5, refine=False, **kw):
    """The flows of a sequence of F >= 2 frames, ``images`` (F, H, W, 3) uint8 or (F, H, W) fp32: ``{'flows_fw', 'flows_bw'}``, each
    (F, H, W, 2) fp32.  ``flows_fw[t]`` goes from frame t to t + 1 and is zero for the last frame, ``flows_bw[t]`` from t to t - 1 and
    is zero for the first -- the reference's convention (datasets/monocular.py:167-179), what ``motion.motion_masks``,
    ``RayBank.from_frames``, ``frames.build_records`` and ``flow.flow_epe`` take.  Both directions run as one batch of 2 (F - 1)
    pairs.  ``check``: also ``'valid'`` (F, 2, H, W) uint8, :func:`nsff_pl_amd.motion.flow_consistency` with ``alpha`` / ``beta``.
    ``refine``: True, or a dict of :func:`refine_flow` keywords, passes the 2 (F - 1) real maps through :func:`refine_flow` as one
    batch, each guided by the frame it starts from and with its direction of the consistency check (computed whatever ``check``
    says) as ``valid``; the all-zero end maps stay zero, and ``'valid'`` is then the check of the refined flows.
    ``**kw`` goes to :func:`optical_flow`."""
    if not isinstance(images, torch.Tensor):
        raise RuntimeError(f"sequence_flows: images: need a tensor, got {type(images).__name__}")
    if images.dim() < 3 or images.shape[0] < 2:
        raise RuntimeError(f"sequence_flows: images: need a sequence of two frames or more, got {tuple(images.shape)}")
    if not isinstance(refine, (bool, dict)):
        raise ValueError(f"sequence_flows: refine must be True, False or a dict of refine_flow keywords, got {refine!r}")
    F = int(images.shape[0])
    starts = torch.cat([images[:-1], images[1:]])                       # the frame each of the 2 (F - 1) flows starts from
    both = optical_flow(starts, torch.cat([images[1:], images[:-1]]), **kw)
    zero = torch.zeros_like(both[:1])
    out = dict(flows_fw=torch.cat([both[:F - 1], zero]), flows_bw=torch.cat([zero, both[F - 1:]]))
    if refine is not False:
        valid = motion.flow_consistency(out["flows_fw"], out["flows_bw"], alpha=alpha, beta=beta)
        both = refine_flow(both, starts, valid=torch.cat([valid[:F - 1, 0], valid[1:, 1]]), **(refine if isinstance(refine, dict) else {}))
        out = dict(flows_fw=torch.cat([both[:F - 1], zero]), flows_bw=torch.cat([zero, both[F - 1:]]))
    if check:
        out["valid"] = motion.flow_consistency(out["flows_fw"], out["flows_bw"], alpha=alpha, beta=beta)
    return out
