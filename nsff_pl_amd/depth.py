"""Disparity maps from optical flow and camera poses, on the GPU (``nsff_disparity_sparse`` / ``nsff_disparity_dense``,
csrc/depth.hip, and ``nsff_disparity_span``, csrc/parallax.hip; there is no CPU path).

The reference takes its ``disps/*`` from DPT-large (preprocess.py:106-115), a network whose weights this project can neither ship
nor run.  This module is a CLASSICAL STAND-IN, not DPT's disparity.  For a STATIC pixel, optical flow plus two camera poses is a
depth measurement -- motion parallax: the pixel's displacement against where a point at infinity would land, divided by what a unit
of disparity would move it.  Where there is no measurement (dynamic pixels, occlusions, too little parallax) an image-guided fill
-- a 2 x 2 push-pull pyramid, then a few edge-aware Jacobi relaxations per level -- gives a dense map.  With it the chain images ->
:func:`nsff_pl_amd.frames.resize_images` -> :func:`nsff_pl_amd.optflow.sequence_flows` -> :func:`nsff_pl_amd.motion.motion_masks`
-> :func:`disparity_maps` -> ``RayBank.from_frames`` needs no network at all.

* :func:`parallax_matrices` -- (F, 2, 12) fp32 on the host: per frame and direction, what turns a pixel and its flow into a disparity
  (``span`` > 1: (F, 2, span, 12), a row for each of the neighbours f +- 1 .. f +- span);
* :func:`triangulate`       -- the measurement alone: ``{'sparse', 'conf', 'known', 'counts'}`` (``span`` > 1: and ``'votes'``);
* :func:`densify`           -- the fill alone: (F, H, W) fp32 from a sparse map, its confidence and a guide image;
* :func:`disparity_maps`    -- both: ``{'disps', 'sparse', 'conf', 'known', 'stats'}`` (``span`` > 1: and ``'votes'``);
* :func:`sequence_geometry` -- flows, masks and disparities of a stack of frames in one call (``span=...`` goes to ``disparity_maps``).

``span`` (1 .. ``_lib.DISPARITY_MAX_SPAN``; 1 is the default and the route described above, unchanged).  With ``span`` > 1 a pixel
is followed along the flow -- its own flow to f +- 1, then the bilinearly sampled flow of f +- 1 at the place it landed, and so on
-- for up to ``span`` frames each way, and is triangulated against every baseline it reaches in one least-squares vote
(``nsff_disparity_span``, one launch).  The parallax grows with the number of frames k, the chained flow's noise only like sqrt(k).
A chain ends for good at the first hop that leaves the image or lands on a tap whose flow is unknown, that fails the
forward-backward check or that is dynamic: the masks at a hop are the same ``masks`` / ``valid`` arguments, read in the frame
the chain has reached.

Units.  ``disps`` is positive, larger is nearer, in the units of the poses it was given (1 / distance along the viewing axis): what
``scene.nearest_depth`` regresses against; the depth loss is shift- and scale-invariant anyway.  It goes unchanged into
``RayBank.from_frames(disps=...)``, :func:`nsff_pl_amd.frames.build_records`, :func:`nsff_pl_amd.frames.resize_disps` and
``scene.nearest_depth``.

Known limit.  A dynamic pixel has no multi-view constraint.  Its disparity is filled in from its static surround, so a person in
front of a wall gets roughly the wall's or the floor's disparity, not their own.  ``known`` and ``conf`` say where the map is
measured and where it is filled.  Under near-pure camera rotation nothing is measured: coincident camera centres give a zero row
and that direction has no vote.  With ``span=1`` a slow camera measures nothing either: where the parallax between neighbouring
frames stays below ``min_parallax`` most pixels are rejected and the map is filled in from almost nothing, or a frame comes out
all zero (``stats.empty_frames``).  ``span`` > 1 is the cure as far as the sequence reaches: on the synthetic scene of the tests,
rescaled so that one frame's parallax is too small, span 1 knows no static pixel and span 2 about 0.7 of them; with enough
parallax span 3 has about two thirds of span 1's error.  A sequence shorter than ``span`` uses the baselines it has.
"""
import numpy as np
import torch

from . import _lib, motion, optflow

DEFAULT_FUSED = bool(_lib.DISPARITY_FUSED)    # the measured default route
TILE, K = _lib.DISPARITY_TILE, _lib.DISPARITY_K   # the fused route's tile side and iterations per launch on batches that fill the machine
SMALL_TILE, SMALL_K = 16, 2                   # ... and on batches that do not
SMALL_BELOW = 512                             # tiles of TILE x TILE pixels in the batch: two per compute unit
GREY_SIGMA = 12.75                            # 0.05 of the 0..255 scale of optflow's grey stage


def _check_span(who, span):
    return motion._check_span(who, span, hi=_lib.DISPARITY_MAX_SPAN)


def parallax_matrices(K, poses, rounded=True, span=1):
    """(F, 2, 12): per frame f and direction d (0: the neighbour n = f + 1, 1: n = f - 1) the nine entries of ``M_n M_f^-1``, row-major,
    and the three of ``e = M_n (C_f - C_n)``.  K (3,3) or (1,3,3); poses (F,3,4) camera-to-world.  From the world -> pixel convention
    of :func:`nsff_pl_amd.frames.projection_matrices`, with ``M = K diag(1,-1,-1) R^-1`` and the camera centre C: a pixel
    ``x = (u, v, 1)`` of f at depth ``1 / delta`` appears in n at ``delta e + h``, ``h = M_n M_f^-1 x``.  float64 throughout, rounded
    once to fp32 (``rounded=False`` returns the float64 values); NOT normalised, because e carries the units of the poses.  A row is
    all zeros where there is no neighbour (the sequence ends) and where the two camera centres coincide
    (:data:`nsff_pl_amd.motion.COINCIDENT`'s rule): the kernel reads a zero row as "no vote".  ``span`` > 1: (F, 2, span, 12), row
    k - 1 built for the neighbour n = f + k / f - k by the same formula and the same rules."""
    span = _check_span("parallax_matrices", span)
    F, pairs = motion.camera_pairs("parallax_matrices", K, poses, span)
    out = np.zeros((F, 2, span, 12))
    for f, d, k, M_n, M_f_inv, base in pairs:
        row = np.concatenate([(M_n @ M_f_inv).ravel(), M_n @ base])
        if np.isfinite(row).all():
            out[f, d, k - 1] = row
    if span == 1:
        out = out[:, :, 0]
    return torch.tensor(out, dtype=torch.float32) if rounded else out


def _check_dense(who, levels, iters, lam, sigma):
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1:
        raise ValueError(f"{who}: levels must be an integer >= 1, got {levels!r}")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= 100000:
        raise ValueError(f"{who}: iters must be an integer from 0 to 100000, got {iters!r}")
    if not 0 <= float(lam) < float("inf"):
        raise ValueError(f"{who}: lam must be a finite number >= 0, got {lam}")
    if not 0 < float(sigma) < float("inf"):
        raise ValueError(f"{who}: sigma must be a finite number > 0, got {sigma}")


def _check_parallax(who, min_parallax):
    if not 0 <= float(min_parallax) < float("inf"):
        raise ValueError(f"{who}: min_parallax must be a finite number >= 0, got {min_parallax}")


def triangulate(flows_fw, flows_bw, K, poses, valid=None, masks=None, min_parallax=0.5, scratch=None, span=1):
    """The disparity of the static pixels of F frames by motion parallax; one launch, everything stays on the GPU.

    flows_fw / flows_bw (F, H, W, 2) fp32 pixels on the GPU (unknown flow: ``|.| > 1e7``); K (3,3); poses (F,3,4) camera-to-world;
    ``valid`` (F, 2, H, W) uint8, the forward-backward check of :func:`nsff_pl_amd.motion.flow_consistency` / ``motion_masks``;
    ``masks`` (F, H, W) uint8, 0 dynamic / non-zero static, the polarity of ``motion_masks``.  A direction votes where it has a
    neighbour with a distinct camera centre, the flow is known, valid and static, the point at infinity lies in front of the
    neighbour and the parallax is at least ``min_parallax`` pixels; the votes are combined by least squares.  Returns a dict:

    * ``'sparse'`` (F, H, W) fp32: the disparity where known, 0 elsewhere;
    * ``'conf'``   (F, H, W) fp32: the squared parallax in px^2 summed over the voting directions, 0 where not known;
    * ``'known'``  (F, H, W) bool;
    * ``'counts'`` (F,) int64 on the GPU: the known pixels of each frame.

    ``span`` (1 .. ``_lib.DISPARITY_MAX_SPAN``): 1 measures against the neighbours f +- 1 alone (``nsff_disparity_sparse``); more
    follows every pixel along the flow for up to ``span`` frames each way and lets it vote against every baseline it reaches
    (``nsff_disparity_span``; the module text says how a chain ends), and adds

    * ``'votes'`` (F, H, W) uint8: the votes of each pixel, at most 2 ``span``.

    ``scratch``: a uint8 tensor of ``_lib.disparity_sparse_scratch_bytes(F, H, W)`` bytes (the same size for every span), zero
    before its first use and left zero (a fresh one when None)."""
    out = _triangulate("triangulate", flows_fw, flows_bw, K, poses, valid, masks, min_parallax, scratch, span)
    del out["n"]
    return out


def _triangulate(who, flows_fw, flows_bw, K, poses, valid, masks, min_parallax, scratch, span=1):
    _check_parallax(who, min_parallax)
    span = _check_span(who, span)
    flows_fw, flows_bw = motion._flows(flows_fw, flows_bw, who)
    F, H, W = (int(v) for v in flows_fw.shape[:3])
    dev = flows_fw.device
    Pm = parallax_matrices(K, poses, span=span)
    if Pm.shape[0] != F:
        raise RuntimeError(f"{who}: {F} frames of flow need {F} poses, got {Pm.shape[0]}")
    valid = motion._uint8_maps(who, "valid", valid, (F, 2, H, W), dev, take_bool=True)
    masks = motion._uint8_maps(who, "masks", masks, (F, H, W), dev, take_bool=True)
    counts = torch.empty(F, dtype=torch.int64, device=dev)
    extra = {}
    if span == 1:
        n, c = _lib.disparity_sparse(flows_fw, flows_bw, Pm.to(dev), valid=valid, masks=masks, min_parallax=min_parallax, counts=counts,
                                     scratch=scratch)
    else:
        n, c, extra["votes"] = _lib.disparity_span(flows_fw, flows_bw, Pm.to(dev), span, valid=valid, masks=masks,
                                                   min_parallax=min_parallax, counts=counts, scratch=scratch)
    known = c > 0
    return dict(sparse=torch.where(known, n / c, torch.zeros_like(n)), conf=c, known=known, counts=counts, n=n, **extra)


def default_route(n_frames, H, W):
    """(fused, tile, k) that ``fused=None`` takes.  Measured at 512 x 288, 3 levels, 30 iterations: on 30
    frames (4320 tiles of 32 x 32) the whole densification is fastest with (32, 3), 1.28 x the plain route; on one frame (144 tiles,
    fewer than compute units) with (16, 2), 1.37 x the plain route, where (32, 3) is within 5 % of plain.  Where the better choice
    changes between those two sizes has not been measured; the switch stands where optflow's does, at two 32 x 32 tiles per compute
    unit."""
    tiles = int(n_frames) * (-(-int(H) // TILE)) * (-(-int(W) // TILE))
    return (DEFAULT_FUSED,) + ((TILE, K) if tiles >= SMALL_BELOW else (SMALL_TILE, SMALL_K))


def scratch_bytes(n_frames, H, W):
    """The size of the ``scratch`` tensor (uint8) that :func:`densify` takes for this shape."""
    return _lib.disparity_dense_scratch_bytes(n_frames, H, W)


def densify(sparse, conf, images_or_grey, levels=3, iters=30, lam=8.0, sigma=GREY_SIGMA, fused=None, scratch=None):
    """A dense disparity map (F, H, W) fp32 from a sparse one: minimises ``conf (d - sparse)^2 + lam sum g (d_p - d_q)^2`` over the
    four-neighbour edges, approximately, coarse to fine.

    ``sparse`` / ``conf`` (F, H, W) fp32 as :func:`triangulate` returns them (``conf`` 0: no data at that pixel).
    ``images_or_grey``: the frames, (F, H, W, 3) uint8 -- grey is what :mod:`nsff_pl_amd.optflow`'s grey stage makes of them,
    ``0.299 R + 0.587 G + 0.114 B`` on the 0..255 scale -- or a guide (F, H, W) fp32 of the caller's on any scale.  The pyramid halves
    2 x 2 down to 1 x 1, so its top holds the confidence-weighted mean of the frame; missing data is filled from the level above,
    and each of the finest ``levels`` levels runs ``iters`` Jacobi iterations with the edge weight
    ``g = 1 / (1 + ((grey_p - grey_q) / sigma)^2)``.  ``sigma`` is in the guide's units: the default 12.75 is 0.05 of the grey
    stage's 0..255 scale (for a 0..1 guide pass 0.05).  ``lam`` 8, ``levels`` 3, ``iters`` 30 and that sigma are starting values
    that nobody has tuned on real data.  ``fused``: True runs the iterations several per launch on tiles held in LDS, False one per
    launch; both give the same bits, None picks the measured default.  ``scratch``: a uint8 tensor of :func:`scratch_bytes` bytes,
    any content (a fresh one when None).  A frame with no known pixel comes out all zero.  Nothing synchronises."""
    who = "densify"
    for t, what in ((sparse, "sparse"), (conf, "conf")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {what}: need a tensor, got {type(t).__name__}")
        if t.dim() != 3 or t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {what}: need (F, H, W) float32, got {tuple(t.shape)} {t.dtype}")
    for t, what in ((sparse, "sparse"), (conf, "conf")):
        _lib.require_gpu_tensor(t, f"{who}: {what}")
    if sparse.shape != conf.shape or sparse.device != conf.device:
        raise RuntimeError(f"{who}: sparse {tuple(sparse.shape)} on {sparse.device} and conf {tuple(conf.shape)} on {conf.device} differ")
    conf = conf.contiguous()
    return _densify(who, conf * sparse.contiguous(), conf, images_or_grey, levels, iters, lam, sigma, fused, scratch)


def _densify(who, n, c, images_or_grey, levels, iters, lam, sigma, fused, scratch):
    _check_dense(who, levels, iters, lam, sigma)
    F, H, W = (int(v) for v in c.shape)
    top = _lib.disparity_levels(H, W)
    if levels > top:
        raise ValueError(f"{who}: levels must be an integer from 1 to {top} for {H} x {W} frames, got {levels}")
    grey = motion._grey(motion._guide(who, images_or_grey, (F, H, W), c.device, "the disparity"))
    route, tile, k = default_route(F, H, W) if fused is None else (bool(fused), 0, 0)
    disps = torch.empty(F, H, W, dtype=torch.float32, device=c.device)
    return _lib.disparity_dense(n, c, grey, disps, levels=levels, iters=iters, lam=lam, sigma=sigma, fused=route, tile=tile, k=k,
                                scratch=scratch)


class DisparityStats:
    """Per-frame counts of :func:`disparity_maps`, kept on the GPU; nothing is read back before a property is asked for.

    ``counts`` (F,) int64: the pixels of each frame whose disparity is measured, not filled."""

    def __init__(self, counts, n_pixels):
        self.gpu_counts, self.n_pixels = counts, int(n_pixels)

    @property
    def counts(self):
        return self.gpu_counts.cpu().numpy()

    @property
    def known_fraction(self):
        """(F,): the share of a frame's pixels with a measured disparity; 0 marks a frame that came out all zero."""
        return self.counts / self.n_pixels

    @property
    def empty_frames(self):
        """The indices of the frames without a single measured pixel: their ``disps`` are all zero."""
        return np.flatnonzero(self.counts == 0)


def disparity_maps(images, flows_fw, flows_bw, K, poses, masks=None, valid=None, min_parallax=0.5, levels=3, iters=30, lam=8.0,
                   sigma=GREY_SIGMA, fused=None, scratch=None, span=1):
    """Disparity maps of F frames from their optical flow and camera poses: :func:`triangulate`, then :func:`densify` guided by
    ``images`` ((F, H, W, 3) uint8 frames or an (F, H, W) fp32 guide); everything stays on the GPU.  Returns a dict:

    * ``'disps'``  (F, H, W) fp32, positive, larger is nearer, in the units of ``poses``;
    * ``'sparse'``, ``'conf'``, ``'known'`` as :func:`triangulate` returns them: where the map is measured and how well;
    * ``'stats'``  a :class:`DisparityStats`.

    ``masks`` / ``valid``: what :func:`nsff_pl_amd.motion.motion_masks` returns as ``'mask'`` / ``'valid'``; without ``masks``
    every pixel counts as static and a moving object gets a wrong disparity of its own instead of its surround's.  The parameters
    are starting values that nobody has tuned on real data (see :func:`densify`).  A frame with no known pixel -- a single frame, a
    sequence shot from one spot, flows that all fail the check -- comes out ALL ZERO: ``stats.known_fraction`` / ``stats.empty_frames``
    detect it.  ``span`` as for :func:`triangulate`: more than 1 measures over several frames by chained flow -- the cure for a slow
    camera -- and adds ``'votes'``.  ``scratch`` as for :func:`densify`.  See the module text for the units and the method's known
    limit."""
    who = "disparity_maps"
    _check_dense(who, levels, iters, lam, sigma)
    tri = _triangulate(who, flows_fw, flows_bw, K, poses, valid, masks, min_parallax, None, span)
    n = tri.pop("n")
    F, H, W = (int(v) for v in n.shape)
    disps = _densify(who, n, tri["conf"], images, levels, iters, lam, sigma, fused, scratch)
    extra = {"votes": tri["votes"]} if "votes" in tri else {}
    return dict(disps=disps, sparse=tri["sparse"], conf=tri["conf"], known=tri["known"], stats=DisparityStats(tri["counts"], H * W), **extra)


def sequence_geometry(images, K, poses, flow_kw=None, mask_kw=None, **disparity_kw):
    """images (F, H, W, 3) uint8 + K + poses -> ``{'disps', 'masks', 'flows_fw', 'flows_bw', 'valid', 'known', 'conf', 'stats',
    'motion_stats'}``: :func:`nsff_pl_amd.optflow.sequence_flows` -> :func:`nsff_pl_amd.motion.motion_masks` ->
    :func:`disparity_maps`, what ``RayBank.from_frames(K, poses, images, disps, masks, flows_fw, flows_bw)`` takes besides the
    frames.  ``flow_kw`` / ``mask_kw`` go to the first two, ``**disparity_kw`` (``span=...`` among them; then ``'votes'`` is returned
    too) to the last."""
    flows = optflow.sequence_flows(images, check=False, **(flow_kw or {}))
    mm = motion.motion_masks(flows["flows_fw"], flows["flows_bw"], K, poses, **(mask_kw or {}))
    out = disparity_maps(images, flows["flows_fw"], flows["flows_bw"], K, poses, masks=mm["mask"], valid=mm["valid"], **disparity_kw)
    extra = {"votes": out["votes"]} if "votes" in out else {}
    return dict(disps=out["disps"], masks=mm["mask"], flows_fw=flows["flows_fw"], flows_bw=flows["flows_bw"], valid=mm["valid"],
                known=out["known"], conf=out["conf"], stats=out["stats"], motion_stats=mm["stats"], **extra)
