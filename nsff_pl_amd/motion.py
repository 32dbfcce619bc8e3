"""Motion masks from optical flow and camera poses, on the GPU (``nsff_motion_maps`` / ``nsff_mask_erode``, csrc/motion.hip; there
is no CPU path).

The reference makes its masks with Mask-RCNN (third_party/predict_mask.py:52-64), which needs detectron2 and a hand-picked class
list.  The original NSFF pipeline's geometric route needs neither: a pixel is moving if its optical flow leaves the epipolar line
that the two camera poses predict for it; a pixel whose flow fails the forward-backward check is occluded or unreliable and has no
vote.  What remains of the reference here is the 15 x 15 erosion that ends its script (line 63), which widens the dynamic area.

* :func:`fundamental_matrices` -- (F, 2, 3, 3) fp32 on the host: ``Fm[f][d]`` maps a pixel of frame f to its line in frame f + 1 (d = 0)
                                  / f - 1 (d = 1);
* :func:`flow_consistency`     -- the forward-backward check alone: ``valid`` (F, 2, H, W) uint8;
* :func:`motion_masks`         -- the whole of it: ``{'mask', 'raw', 'err', 'valid', 'stats'}``;
* :func:`erode`                -- ``cv2.erode(mask, ones((k, k)))`` on (F, H, W) uint8 masks from any source.

Polarity.  ``'mask'`` and ``'raw'`` hold 0 where a pixel is DYNAMIC and 255 where it is static -- what the reference's
``masks/*.png`` hold, and ``mask == 0`` is "Dynamic only" in its eval.py.  They go unchanged into
``RayBank.from_frames(masks=...)``, :func:`nsff_pl_amd.frames.build_records` and ``evaluate.evaluate_split(masks=...)``.
``evaluate.flow_frames`` and :func:`nsff_pl_amd.flow.flow_epe` take the COMPLEMENT, where non-zero means dynamic: pass
``mask == 0``.

Known limit.  An object that moves along its own epipolar line is invisible to this test, and under near-pure camera rotation
every line degenerates: coincident camera centres give a zero matrix and that direction has no vote.
"""
import numpy as np
import torch

from . import _lib

UNKNOWN = _lib.FLOW_UNKNOWN
ERODE_MAX_K = _lib.ERODE_MAX_K
COINCIDENT = 1e-12            # two camera centres closer than this times max(1, their norms) count as one


def _host(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def fundamental_matrices(K, poses, rounded=True):
    """(F, 2, 3, 3): ``Fm[f][0]`` maps a homogeneous pixel (x, y, 1) of frame f to its epipolar line in frame f + 1, ``Fm[f][1]`` to
    its line in frame f - 1.  K (3,3) or (1,3,3); poses (F,3,4) camera-to-world.  From the world -> pixel convention of
    :func:`nsff_pl_amd.frames.projection_matrices`, ``P = K diag(1,-1,-1) [R^-1 | -R^-1 t]``: with ``M = K diag(1,-1,-1) R^-1`` and
    the camera centre t, a pixel x of f is seen in n at ``M_n (t_f - t_n) + lambda M_n M_f^-1 x``, so its line is
    ``[M_n (t_f - t_n)]_x M_n M_f^-1 x``.  float64 throughout, each matrix scaled to unit Frobenius norm and rounded once to fp32
    (``rounded=False`` returns the float64 values).  A zero matrix stands where there is no neighbour (the sequence ends) and where
    the two camera centres coincide (closer than 1e-12 of their size): the kernel then has ``n = 0`` and the direction no vote."""
    K, poses = _host(K), _host(poses)
    if K.shape == (1, 3, 3):
        K = K[0]
    if K.shape != (3, 3):
        raise RuntimeError(f"fundamental_matrices: K must be (3,3) or (1,3,3), got {K.shape}")
    if poses.ndim != 3 or poses.shape[1:] != (3, 4):
        raise RuntimeError(f"fundamental_matrices: poses must be (F,3,4) camera-to-world matrices, got {poses.shape}")
    F = len(poses)
    M = K @ np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(poses[:, :, :3])
    M_inv = np.linalg.inv(M)
    C = poses[:, :, 3]
    out = np.zeros((F, 2, 3, 3))
    for f in range(F):
        for d, n in enumerate((f + 1, f - 1)):
            if not 0 <= n < F:
                continue
            base = C[f] - C[n]
            if np.linalg.norm(base) <= COINCIDENT * max(1.0, np.linalg.norm(C[f]), np.linalg.norm(C[n])):
                continue
            e = M[n] @ base
            cross = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
            Fm = cross @ M[n] @ M_inv[f]
            norm = np.linalg.norm(Fm)
            if np.isfinite(norm) and norm > 0:
                out[f, d] = Fm / norm
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


def _check_scalars(who, **values):
    for name, v in values.items():
        if not float(v) >= 0:
            raise ValueError(f"{who}: {name} must be a number >= 0, got {v}")


def _check_k(k, who):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > ERODE_MAX_K or k % 2 == 0:
        raise ValueError(f"{who}: the window k must be an odd integer from 1 to {ERODE_MAX_K}, got {k!r}")
    return int(k)


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
    the epipolar error over each direction's valid pixels), ``dynamic`` (F,) int64 (the zero pixels of the eroded 'mask')."""

    def __init__(self, counts, err_sums, dynamic, n_pixels):
        self.gpu_counts, self.gpu_err_sums, self.gpu_dynamic, self.n_pixels = counts, err_sums, dynamic, int(n_pixels)

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


def motion_masks(flows_fw, flows_bw, K, poses, threshold=1.0, erode=15, alpha=0.01, beta=0.5, scratch=None):
    """Motion masks of F frames from their optical flow and camera poses; two launches, everything stays on the GPU.

    flows_fw / flows_bw (F, H, W, 2) fp32 pixels on the GPU, as ``RayBank.from_frames`` takes them (unknown flow: ``|.| > 1e7``);
    K (3,3); poses (F,3,4) camera-to-world.  Returns a dict:

    * ``'mask'``  (F, H, W) uint8, 0 dynamic / 255 static, ``'raw'`` eroded with an ``erode`` x ``erode`` window (odd, 1 .. 31);
    * ``'raw'``   (F, H, W) uint8 before the erosion: 0 where a direction is valid and its error exceeds ``threshold``;
    * ``'err'``   (F, 2, H, W) fp32: the distance in pixels of ``pixel + flow`` from the pixel's epipolar line in the neighbour,
                  :data:`UNKNOWN` where there is no neighbour, the flow is unknown or the line is degenerate;
    * ``'valid'`` (F, 2, H, W) uint8: :func:`flow_consistency`'s check and a proper line;
    * ``'stats'`` a :class:`MotionStats`.

    ``threshold`` is in pixels; its default of 1 is a starting value that nobody has tuned on real data -- look at ``'err'`` on your
    own sequence before trusting it.  ``alpha`` / ``beta``: the forward-backward check's relative and absolute slack.  ``scratch``:
    a uint8 tensor of ``_lib.motion_maps_scratch_bytes(F, H, W)`` bytes, zero before its first use and left zero (a fresh one when
    None).  See the module text for the masks' polarity and the method's known limit."""
    k = _check_k(erode, "motion_masks")
    _check_scalars("motion_masks", threshold=threshold, alpha=alpha, beta=beta)
    flows_fw, flows_bw = _flows(flows_fw, flows_bw, "motion_masks")
    F, H, W = (int(v) for v in flows_fw.shape[:3])
    dev = flows_fw.device
    Fm = fundamental_matrices(K, poses)
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
    out["mask"] = torch.empty_like(out["raw"])
    _lib.mask_erode(out["raw"], out["mask"], k, zero_counts=dynamic, scratch=scratch)
    out["stats"] = MotionStats(counts, err_sums, dynamic, H * W)
    return out


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
