"""Motion masks from optical flow and camera poses, on the GPU (``nsff_motion_maps`` / ``nsff_mask_erode``, csrc/motion.hip; there
is no CPU path).

The reference makes its masks with Mask-RCNN (third_party/predict_mask.py:52-64), which needs detectron2 and a hand-picked class
list.  The original NSFF pipeline's geometric route needs neither: a pixel is moving if its optical flow leaves the epipolar line
that the two camera poses predict for it; a pixel whose flow fails the forward-backward check is occluded or unreliable and has no
vote.  What remains of the reference here is the 15 x 15 erosion that ends its script (line 63), which widens the dynamic area.

* :func:`fundamental_matrices` -- (F, 2, 3, 3) fp32 on the host: ``Fm[f][d]`` maps a pixel of frame f to its line in frame f + 1 (d = 0)
                                  / f - 1 (d = 1); with ``span`` > 1 (F, 2, span, 3, 3), the lines in f +- 1 .. f +- span;
* :func:`flow_consistency`     -- the forward-backward check alone: ``valid`` (F, 2, H, W) uint8;
* :func:`motion_masks`         -- the whole of it: ``{'mask', 'raw', 'err', 'valid', 'stats'}``;
* :func:`erode`                -- ``cv2.erode(mask, ones((k, k)))`` on (F, H, W) uint8 masks from any source;
* :func:`propagate`            -- "dynamic" carried along the chained flow from the frames f +- 1 .. f +- reach, on masks from any
                                  source (``nsff_mask_propagate``, csrc/motionspan.hip).

Several frames.  One frame's test misses an object that drifts less than ``threshold`` a frame off its epipolar line -- in every
frame -- and an object that pauses, in the frames of the pause; a Mask-RCNN mask misses neither.  ``motion_masks(span=S)`` follows
a pixel along the flow for up to S frames and tests it against every line it reaches (``nsff_motion_span``), each hop's error
scaled by ``hop_scale`` (default ``1 / sqrt(k)``: a chained flow's noise grows like sqrt(k), a steady drift like k);
``motion_masks(reach=R)`` then marks a pixel dynamic if the chain meets a dynamic pixel within R frames.

Polarity.  ``'mask'`` and ``'raw'`` hold 0 where a pixel is DYNAMIC and 255 where it is static -- what the reference's
``masks/*.png`` hold, and ``mask == 0`` is "Dynamic only" in its eval.py.  They go unchanged into
``RayBank.from_frames(masks=...)``, :func:`nsff_pl_amd.frames.build_records` and ``evaluate.evaluate_split(masks=...)``.
``evaluate.flow_frames`` and :func:`nsff_pl_amd.flow.flow_epe` take the COMPLEMENT, where non-zero means dynamic: pass
``mask == 0``.

Known limit.  An object that moves along its own epipolar line is invisible to this test, and under near-pure camera rotation
every line degenerates: coincident camera centres give a zero matrix and that direction has no vote.  Propagation also carries a
FALSE positive along the flow for ``reach`` frames; the ``1 / sqrt(k)`` scaling is a noise model that nobody has tuned on real
flow; ``valid`` gates every hop, so occluded pixels neither vote nor propagate.
"""
import numpy as np
import torch

from . import _lib
from .flow import _host

UNKNOWN = _lib.FLOW_UNKNOWN
ERODE_MAX_K = _lib.ERODE_MAX_K
MAX_SPAN, MAX_REACH = _lib.MOTION_MAX_SPAN, _lib.PROPAGATE_MAX_REACH
COINCIDENT = 1e-12            # two camera centres closer than this times max(1, their norms) count as one


def camera_pairs(who, K, poses, span):
    """``(F, pairs)`` of a sequence: K (3,3) or (1,3,3), poses (F,3,4) camera-to-world, refused in ``who``'s name.  ``pairs`` yields
    ``(f, d, k, M[n], M_inv[f], C[f] - C[n])`` in float64 for every frame f, direction d (0: n = f + k, 1: n = f - k) and
    k = 1 .. span whose neighbour n exists and whose camera centres C are distinct (:data:`COINCIDENT`), with
    ``M = K diag(1,-1,-1) R^-1``."""
    K, poses = _host(K), _host(poses)
    if K.shape == (1, 3, 3):
        K = K[0]
    if K.shape != (3, 3):
        raise RuntimeError(f"{who}: K must be (3,3) or (1,3,3), got {K.shape}")
    if poses.ndim != 3 or poses.shape[1:] != (3, 4):
        raise RuntimeError(f"{who}: poses must be (F,3,4) camera-to-world matrices, got {poses.shape}")
    F = len(poses)
    M = K @ np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(poses[:, :, :3])
    M_inv = np.linalg.inv(M)
    C = poses[:, :, 3]

    def pairs():
        for f in range(F):
            for d, s in enumerate((+1, -1)):
                for k in range(1, span + 1):
                    n = f + s * k
                    if not 0 <= n < F:
                        break
                    base = C[f] - C[n]
                    if np.linalg.norm(base) <= COINCIDENT * max(1.0, np.linalg.norm(C[f]), np.linalg.norm(C[n])):
                        continue
                    yield f, d, k, M[n], M_inv[f], base
    return F, pairs()


def fundamental_matrices(K, poses, rounded=True, span=1):
    """(F, 2, 3, 3): ``Fm[f][0]`` maps a homogeneous pixel (x, y, 1) of frame f to its epipolar line in frame f + 1, ``Fm[f][1]`` to
    its line in frame f - 1.  K (3,3) or (1,3,3); poses (F,3,4) camera-to-world.  From the world -> pixel convention of
    :func:`nsff_pl_amd.frames.projection_matrices`, ``P = K diag(1,-1,-1) [R^-1 | -R^-1 t]``: with ``M = K diag(1,-1,-1) R^-1`` and
    the camera centre t, a pixel x of f is seen in n at ``M_n (t_f - t_n) + lambda M_n M_f^-1 x``, so its line is
    ``[M_n (t_f - t_n)]_x M_n M_f^-1 x``.  float64 throughout, each matrix scaled to unit Frobenius norm and rounded once to fp32
    (``rounded=False`` returns the float64 values).  A zero matrix stands where there is no neighbour (the sequence ends) and where
    the two camera centres coincide (closer than 1e-12 of their size): the kernel then has ``n = 0`` and the direction no vote.
    ``span`` > 1: (F, 2, span, 3, 3), row k - 1 built for the neighbour n = f + k / f - k by the same formula and the same rules;
    row 0 has the bits of ``span=1``."""
    span = _check_span("fundamental_matrices", span)
    F, pairs = camera_pairs("fundamental_matrices", K, poses, span)
    out = np.zeros((F, 2, span, 3, 3))
    for f, d, k, M_n, M_f_inv, base in pairs:
        e = M_n @ base
        cross = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
        Fm = cross @ M_n @ M_f_inv
        norm = np.linalg.norm(Fm)
        if np.isfinite(norm) and norm > 0:
            out[f, d, k - 1] = Fm / norm
    if span == 1:
        out = out[:, :, 0]
    return torch.tensor(out, dtype=torch.float32) if rounded else out


def _flows(flows_fw, flows_bw, who):
    for t, what in ((flows_fw, "flows_fw"), (flows_bw, "flows_bw")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {what}: need a tensor, got {type(t).__name__}")
        if t.dim() != 4 or t.shape[-1] != 2:
            raise RuntimeError(f"{who}: {what}: need (F, H, W, 2) maps, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {what}: need float32, got {t.dtype}")
    if flows_fw.shape != flows_bw.shape:
        raise RuntimeError(f"{who}: flows_fw {tuple(flows_fw.shape)} and flows_bw {tuple(flows_bw.shape)} differ in shape")
    for t, what in ((flows_fw, "flows_fw"), (flows_bw, "flows_bw")):
        _lib.require_gpu_tensor(t, f"{who}: {what}")
    if flows_fw.device != flows_bw.device:
        raise RuntimeError(f"{who}: flows_fw is on {flows_fw.device}, flows_bw on {flows_bw.device}")
    return flows_fw.contiguous(), flows_bw.contiguous()


def _uint8_maps(who, what, t, shape, dev=None, take_bool=False, refusal=None):
    """An optional uint8 map of ``shape``, contiguous -- with ``dev``, on the GPU and on the flows' device.  ``take_bool``: a bool
    map is converted; ``refusal``: the caller's one sentence for a wrong type, dtype or shape."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(refusal or f"{who}: {what}: need a tensor, got {type(t).__name__}")
    if take_bool and t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype != torch.uint8 or tuple(t.shape) != shape:
        raise RuntimeError(refusal or f"{who}: {what}: need {shape} uint8, got {tuple(t.shape)} {t.dtype}")
    if dev is not None:
        _lib.require_gpu_tensor(t, f"{who}: {what}")
        if t.device != dev:
            raise RuntimeError(f"{who}: {what} is on {t.device}, the flows on {dev}")
    return t.contiguous()


def _guide(who, images_or_grey, shape, dev, of):
    """Checks a guide for maps of ``shape`` on ``dev``, uint8 frames or a grey fp32 guide of the caller's, and returns it contiguous
    (:func:`_grey` makes the guide of it); ``of``: what else is on ``dev``, "the disparity" or "the flows"."""
    t = images_or_grey
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{who}: images: need a tensor, got {type(t).__name__}")
    colour = t.dtype == torch.uint8
    if t.dtype not in (torch.uint8, torch.float32) or tuple(t.shape) != (shape + (3,) if colour else shape):
        raise RuntimeError(f"{who}: images: need channels-last {shape + (3,)} uint8 frames or a grey {shape} float32 guide, got "
                           f"{tuple(t.shape)} {t.dtype}")
    _lib.require_gpu_tensor(t, f"{who}: images")
    if t.device != dev:
        raise RuntimeError(f"{who}: images are on {t.device}, {of} on {dev}")
    return t.contiguous()


def _grey(guide):
    return _lib.optflow_grey(guide) if guide.dtype == torch.uint8 else guide


def _check_scalars(who, **values):
    for name, v in values.items():
        if not float(v) >= 0:
            raise ValueError(f"{who}: {name} must be a number >= 0, got {v}")


def _check_k(k, who):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > ERODE_MAX_K or k % 2 == 0:
        raise ValueError(f"{who}: the window k must be an odd integer from 1 to {ERODE_MAX_K}, got {k!r}")
    return int(k)


def _check_span(who, span, what="span", lo=1, hi=None):
    hi = MAX_SPAN if hi is None else hi
    if isinstance(span, bool) or not isinstance(span, (int, np.integer)) or span < lo or span > hi:
        raise ValueError(f"{who}: {what} must be an integer from {lo} to {hi}, got {span!r}")
    return int(span)


def default_hop_scale(span):
    """(span,) fp32: ``1 / sqrt(k)`` for k = 1 .. span, computed in float64 and rounded once."""
    return (1.0 / np.sqrt(np.arange(1, span + 1, dtype=np.float64))).astype(np.float32)


def _hop_scale(who, hop_scale, span):
    if hop_scale is None:
        return default_hop_scale(span)
    hs = _host(hop_scale).reshape(-1)
    if hs.shape != (span,) or not (np.isfinite(hs).all() and (hs >= 0).all()):
        raise ValueError(f"{who}: hop_scale must hold {span} finite numbers >= 0, got {hop_scale!r}")
    return hs.astype(np.float32)


def flow_consistency(flows_fw, flows_bw, alpha=0.01, beta=0.5):
    """The forward-backward check alone: ``valid`` (F, 2, H, W) uint8 on the GPU, 1 where the frame has a neighbour on that side, the
    flow is known, its target lies inside the image, the four taps of the opposite flow there are known and
    ``|a + b|^2 <= alpha (|a|^2 + |b|^2) + beta``.  This is ``nsff_motion_maps`` with its ``epipolar`` flag off: no matrices are
    read and ``valid`` is defined without the ``line_ok`` term of :func:`motion_masks`."""
    flows_fw, flows_bw = _flows(flows_fw, flows_bw, "flow_consistency")
    _check_scalars("flow_consistency", alpha=alpha, beta=beta)
    F, H, W = (int(v) for v in flows_fw.shape[:3])
    valid = torch.empty(F, 2, H, W, dtype=torch.uint8, device=flows_fw.device)
    _lib.motion_maps(flows_fw, flows_bw, None, alpha=alpha, beta=beta, valid=valid)
    return valid


class MotionStats:
    """Per-frame counts and sums of :func:`motion_masks`, kept on the GPU; nothing is read back before a property is asked for.

    ``counts`` (F, 5) int64 [valid fw, valid bw, over fw, over bw, dynamic pixels of 'raw'], ``err_sums`` (F, 2) fp64 (the sum of
    the epipolar error over each direction's valid pixels), ``dynamic`` (F,) int64 (the zero pixels of the eroded 'mask').  ``counts``
    and ``err_sums`` are always the single-frame test's.  With ``span`` > 1: ``span_counts`` (F, 3) int64 [over fw, over bw, dynamic
    pixels] of the chained test; with ``reach`` > 0: ``propagated`` (F,) int64, the zero pixels of 'raw' after the propagation.
    Both are None where that step did not run."""

    def __init__(self, counts, err_sums, dynamic, n_pixels, span_counts=None, propagated=None):
        self.gpu_counts, self.gpu_err_sums, self.gpu_dynamic, self.n_pixels = counts, err_sums, dynamic, int(n_pixels)
        self.gpu_span_counts, self.gpu_propagated = span_counts, propagated

    @property
    def span_counts(self):
        return None if self.gpu_span_counts is None else self.gpu_span_counts.cpu().numpy()

    @property
    def propagated(self):
        return None if self.gpu_propagated is None else self.gpu_propagated.cpu().numpy()

    @property
    def counts(self):
        return self.gpu_counts.cpu().numpy()

    @property
    def err_sums(self):
        return self.gpu_err_sums.cpu().numpy()

    @property
    def dynamic(self):
        return self.gpu_dynamic.cpu().numpy()

    @property
    def valid_fraction(self):
        """(F, 2): the share of a frame's pixels with a vote, per direction."""
        return self.counts[:, 0:2] / self.n_pixels

    @property
    def mean_err(self):
        """(F, 2): the mean epipolar error over the valid pixels, NaN where there is none."""
        n = self.counts[:, 0:2]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, self.err_sums / n, np.nan)

    @property
    def dynamic_fraction(self):
        """(F,): the share of a frame's pixels that the eroded mask calls dynamic."""
        return self.dynamic / self.n_pixels


def motion_masks(flows_fw, flows_bw, K, poses, threshold=1.0, erode=15, alpha=0.01, beta=0.5, scratch=None, span=1, reach=0,
                 hop_scale=None):
    """Motion masks of F frames from their optical flow and camera poses; two launches (one more with ``span`` > 1, one more with
    ``reach`` > 0), everything stays on the GPU.

    flows_fw / flows_bw (F, H, W, 2) fp32 pixels on the GPU, as ``RayBank.from_frames`` takes them (unknown flow: ``|.| > 1e7``);
    K (3,3); poses (F,3,4) camera-to-world.  Returns a dict:

    * ``'mask'``  (F, H, W) uint8, 0 dynamic / 255 static, ``'raw'`` eroded with an ``erode`` x ``erode`` window (odd, 1 .. 31);
    * ``'raw'``   (F, H, W) uint8 before the erosion: 0 where a direction is valid and its error exceeds ``threshold``;
    * ``'err'``   (F, 2, H, W) fp32: the distance in pixels of ``pixel + flow`` from the pixel's epipolar line in the neighbour,
                  :data:`UNKNOWN` where there is no neighbour, the flow is unknown or the line is degenerate;
    * ``'valid'`` (F, 2, H, W) uint8: :func:`flow_consistency`'s check and a proper line;
    * ``'stats'`` a :class:`MotionStats`.

    ``span`` > 1 (up to 8): the chained test.  ``'err'`` and ``'valid'`` stay the single-frame ones; ``'raw'`` is 0 where, in a
    direction, the largest of the scaled errors ``err_k * hop_scale[k - 1]`` over the neighbours f +- 1 .. f +- span that the chain
    reaches exceeds ``threshold``; ``'err_span'`` (F, 2, H, W) fp32 holds that largest value (:data:`UNKNOWN` where no neighbour
    was measured) and ``'hops'`` (F, 2, H, W) uint8 the number of neighbours measured.  ``hop_scale``: ``span`` numbers, None for
    ``1 / sqrt(k)``.  ``reach`` > 0 (up to 8): ``'raw'`` is then also 0 where the chained flow meets a dynamic pixel of ``'raw'``
    within ``reach`` frames (:func:`propagate`), and ``'hits'`` (F, H, W) uint8 counts those meetings.  ``'mask'`` and
    ``stats.dynamic`` always come from the final ``'raw'``.

    ``threshold`` is in pixels; its default of 1 is a starting value that nobody has tuned on real data -- look at ``'err'`` on your
    own sequence before trusting it.  ``alpha`` / ``beta``: the forward-backward check's relative and absolute slack.  ``scratch``:
    a uint8 tensor of ``_lib.motion_maps_scratch_bytes(F, H, W)`` bytes, zero before its first use and left zero (a fresh one when
    None).  See the module text for the masks' polarity and the method's known limit."""
    k = _check_k(erode, "motion_masks")
    span = _check_span("motion_masks", span)
    reach = _check_span("motion_masks", reach, "reach", 0, MAX_REACH)
    _check_scalars("motion_masks", threshold=threshold, alpha=alpha, beta=beta)
    if span == 1 and hop_scale is not None:
        raise ValueError("motion_masks: hop_scale goes with span > 1")
    flows_fw, flows_bw = _flows(flows_fw, flows_bw, "motion_masks")
    F, H, W = (int(v) for v in flows_fw.shape[:3])
    dev = flows_fw.device
    Fs = fundamental_matrices(K, poses, span=span)
    Fm = Fs if span == 1 else Fs[:, :, 0].contiguous()
    if Fm.shape[0] != F:
        raise RuntimeError(f"motion_masks: {F} frames of flow need {F} poses, got {Fm.shape[0]}")
    if scratch is None:
        scratch = torch.zeros(max(_lib.motion_maps_scratch_bytes(F, H, W), 16), dtype=torch.uint8, device=dev)
    out = dict(err=torch.empty(F, 2, H, W, dtype=torch.float32, device=dev), valid=torch.empty(F, 2, H, W, dtype=torch.uint8, device=dev),
               raw=torch.empty(F, H, W, dtype=torch.uint8, device=dev))
    counts = torch.empty(F, 5, dtype=torch.int64, device=dev)
    err_sums = torch.empty(F, 2, dtype=torch.float64, device=dev)
    dynamic = torch.empty(F, dtype=torch.int64, device=dev)
    _lib.motion_maps(flows_fw, flows_bw, Fm.to(dev), alpha=alpha, beta=beta, threshold=threshold, counts=counts, err_sums=err_sums,
                     scratch=scratch, **out)
    span_counts = propagated = None
    if span > 1:                                                  # the maps' scratch is the larger: it serves the two calls below too
        out["err_span"] = torch.empty(F, 2, H, W, dtype=torch.float32, device=dev)
        out["hops"] = torch.empty(F, 2, H, W, dtype=torch.uint8, device=dev)
        span_counts = torch.empty(F, 3, dtype=torch.int64, device=dev)
        _lib.motion_span(flows_fw, flows_bw, Fs.to(dev), torch.from_numpy(_hop_scale("motion_masks", hop_scale, span)).to(dev), span,
                         valid=out["valid"], threshold=threshold, err=out["err_span"], hops=out["hops"], raw=out["raw"],
                         counts=span_counts, scratch=scratch)
    if reach > 0:
        out["hits"] = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
        propagated = torch.empty(F, dtype=torch.int64, device=dev)
        out["raw"] = _lib.mask_propagate(out["raw"], flows_fw, flows_bw, reach, valid=out["valid"], hits=out["hits"],
                                         zero_counts=propagated, scratch=scratch)
    out["mask"] = torch.empty_like(out["raw"])
    _lib.mask_erode(out["raw"], out["mask"], k, zero_counts=dynamic, scratch=scratch)
    out["stats"] = MotionStats(counts, err_sums, dynamic, H * W, span_counts, propagated)
    return out


def propagate(masks_u8, flows_fw, flows_bw, valid=None, reach=2, return_hits=False):
    """"Dynamic" carried along the flow, on (F, H, W) uint8 masks from any source (0 dynamic, the reference's polarity): a pixel of
    frame f becomes 0 if it is 0 already or if its flow, chained for up to ``reach`` frames forwards or backwards (the hop of
    :func:`motion_masks` with ``span``), lands -- rounded to the nearest pixel -- on a 0 of the frame it reaches; every other pixel
    keeps its value.  flows_fw / flows_bw (F, H, W, 2) fp32; ``valid`` (F, 2, H, W) uint8, optional, gates the start and every hop
    (:func:`flow_consistency`'s check: an occluded pixel does not propagate).  ``reach`` 1 .. 8.  ``return_hits``: also the
    (F, H, W) uint8 count of zeros met, at most ``2 * reach``.  A false positive travels as far as a true one."""
    if not isinstance(masks_u8, torch.Tensor):
        raise RuntimeError(f"propagate: masks: need a tensor, got {type(masks_u8).__name__}")
    if masks_u8.dim() != 3:
        raise RuntimeError(f"propagate: masks: need (F, H, W) images, got {tuple(masks_u8.shape)}")
    if masks_u8.dtype != torch.uint8:
        raise RuntimeError(f"propagate: masks: need uint8, got {masks_u8.dtype}")
    reach = _check_span("propagate", reach, "reach", 1, MAX_REACH)
    flows_fw, flows_bw = _flows(flows_fw, flows_bw, "propagate")
    if tuple(flows_fw.shape[:3]) != tuple(masks_u8.shape):
        raise RuntimeError(f"propagate: masks {tuple(masks_u8.shape)} do not go with flows {tuple(flows_fw.shape)}")
    valid = _uint8_maps("propagate", "valid", valid, (masks_u8.shape[0], 2) + tuple(masks_u8.shape[1:]),
                        refusal="propagate: valid: need a (F, 2, H, W) uint8 tensor")
    src = masks_u8.contiguous()
    hits = torch.empty_like(src) if return_hits else None
    dst = _lib.mask_propagate(src, flows_fw, flows_bw, reach, valid=valid, hits=hits)
    return (dst, hits) if return_hits else dst


def erode(mask_u8, k=15, return_counts=False):
    """``cv2.erode(mask, np.ones((k, k)))`` of (F, H, W) uint8 masks -- (H, W) for one -- on the GPU, any values: every pixel becomes
    the minimum of the k x k window centred on it; pixels outside the image do not contribute, so an image smaller than the window
    is legal.  k odd, 1 .. 31; k = 1 copies.  On 0 / 255 masks this WIDENS the zero (dynamic) area by k // 2 pixels, which is what
    the reference does with k = 15 to its Mask-RCNN masks (predict_mask.py:63).  ``return_counts``: also the (F,) int64 count of
    zero pixels of each eroded frame, on the GPU."""
    if not isinstance(mask_u8, torch.Tensor):
        raise RuntimeError(f"erode: mask: need a tensor, got {type(mask_u8).__name__}")
    single = mask_u8.dim() == 2
    if mask_u8.dim() not in (2, 3):
        raise RuntimeError(f"erode: mask: need (F, H, W) or (H, W) images, got {tuple(mask_u8.shape)}")
    if mask_u8.dtype != torch.uint8:
        raise RuntimeError(f"erode: mask: need uint8, got {mask_u8.dtype}")
    k = _check_k(k, "erode")
    _lib.require_gpu_tensor(mask_u8, "erode: mask")
    src = (mask_u8[None] if single else mask_u8).contiguous()
    dst = torch.empty_like(src)
    counts = torch.empty(src.shape[0], dtype=torch.int64, device=src.device) if return_counts else None
    _lib.mask_erode(src, dst, k, zero_counts=counts)
    dst = dst[0] if single else dst
    return (dst, counts) if return_counts else dst
