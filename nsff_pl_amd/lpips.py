"""LPIPS 0.1 with ``net='alex'``, ``spatial=True`` on the GPU: the object the reference's eval.py:178 calls ``lpips_model``.

The network runs in one ``nsff_lpips`` call (csrc/lpips.hip): AlexNet's five convolutions as implicit GEMM on the fp32 MFMA, the
per-layer normalised feature distance, its bilinear upsampling and the sum over the five layers.  There is no CPU path.

The trained values are not part of this library: :meth:`LPIPS.from_state_dict` takes them from the caller, e.g.

    sd = lpips.LPIPS(net='alex', spatial=True).state_dict()         # the public ``lpips`` package
    model = nsff_pl_amd.LPIPS.from_state_dict(sd)

The arithmetic is pinned against a float64 restatement of the graph on seeded random weights (tests/lpips_torch.py); values on
the published weights are unpinned.
"""
import torch

from . import _lib

_CONV_INDEX = (0, 3, 6, 8, 10)                    # torchvision AlexNet ``features`` indices of the five convolutions
# the LPIPS module wraps the same layers in five slices, keeping the index each has in ``features``
_LPIPS_CONV = tuple(f"net.slice{l + 1}.{i}" for l, i in enumerate(_CONV_INDEX))
_TV_CONV = tuple(f"features.{i}" for i in _CONV_INDEX)
_LIN = tuple(f"lin{l}.model.1.weight" for l in range(5))


def _ambiguous(shape):
    return len(shape) == 4 and shape[1] == 3 and shape[3] == 3


class LPIPS:
    """``model(in0, in1, normalize=False)`` -> (F, 1, H, W), as ``lpips.LPIPS(net='alex', spatial=True)`` in eval mode.

    conv_w / conv_b: the five AlexNet convolutions' weights (cout, cin, k, k) and biases; lin: the five 1x1 ``lin`` weights, any
    shape with cout elements.  The tensors are kept by reference and packed for the kernels on first use; the pack is redone
    when one of them changes (``(data_ptr, _version)``, as :mod:`nsff_pl_amd.packing` does for the models)."""

    def __init__(self, conv_w, conv_b, lin, device="cuda"):
        if not (len(conv_w) == len(conv_b) == len(lin) == 5):
            raise ValueError("LPIPS: need five convolution weights, five biases and five lin weights")
        self._tensors = tuple(conv_w) + tuple(conv_b) + tuple(lin)
        for l, shape in enumerate(_lib.LPIPS_CONV_SHAPES):
            if tuple(conv_w[l].shape) != shape or conv_b[l].numel() != shape[0] or lin[l].numel() != shape[0]:
                raise ValueError(f"LPIPS: layer {l} has weight {tuple(conv_w[l].shape)}, bias {tuple(conv_b[l].shape)} and lin "
                                 f"{tuple(lin[l].shape)}; AlexNet's is {shape} with {shape[0]} outputs")
        self.device = torch.device(device)
        self._key = None
        self._packed = None
        self._workspace = {}

    @classmethod
    def from_state_dict(cls, sd, device="cuda"):
        """From the state dict of the public ``lpips`` package's module (keys ``net.slice{1..5}.{0,3,6,8,10}.weight|bias`` and
        ``lin{0..4}.model.1.weight``) or from a torchvision AlexNet's (``features.{0,3,6,8,10}.weight|bias``) merged with the
        ``lin*`` keys.  The key names are those of the public packages as published; neither package is available to this
        project's tests, which exercise the mapping on state dicts built with these names.  Raises ``KeyError`` listing every
        key that is missing."""
        conv = _LPIPS_CONV if any(k.startswith("net.slice") for k in sd) else _TV_CONV
        names = [f"{c}.weight" for c in conv] + [f"{c}.bias" for c in conv] + list(_LIN)
        missing = [n for n in names if n not in sd]
        if missing:
            raise KeyError(f"LPIPS.from_state_dict: missing {', '.join(missing)}")
        t = [sd[n] for n in names]
        return cls(t[0:5], t[5:10], t[10:15], device=device)

    def packed(self):
        """The packed device buffer of the current weights."""
        key = tuple((t.data_ptr(), t._version) for t in self._tensors)
        if key != self._key:
            if self.device.type != "cuda":
                raise RuntimeError("LPIPS runs only on the HIP kernels of libnsff_hip.so (no CPU fallback): device must be a GPU")
            dev = [t.detach().to(device=self.device, dtype=torch.float32).contiguous() for t in self._tensors]
            self._packed = _lib.lpips_pack(dev[0:5], dev[5:10], [t.reshape(-1) for t in dev[10:15]])
            self._key = key
        return self._packed

    def score(self, gt, pred, valid=None, want_map=True, want_sums=False, normalize=False):
        """gt / pred (F, H, W, 3) fp32 GPU frames, valid (F, H, W) bool / uint8 or None.  Returns ``(map, sums)``: the spatial map
        (F, H, W) fp32 and the per-frame fp64 sums (F, 3) [map, map over valid, valid pixels]; either is None unless asked for."""
        if gt.dim() != 4 or gt.shape[-1] != 3 or pred.shape != gt.shape:
            raise RuntimeError(f"lpips: need (F, H, W, 3) image pairs of one shape, got {tuple(gt.shape)} and {tuple(pred.shape)}")
        F, H, W = (int(v) for v in gt.shape[:3])
        _lib.lpips_dims(H, W)                                     # refuses an image that is too small by name
        _lib.require_gpu_tensor(gt, "lpips: image_gt")
        _lib.require_gpu_tensor(pred, "lpips: image_pred")
        gt, pred = gt.float().contiguous(), pred.float().contiguous()
        if valid is not None:
            valid = valid.reshape(F, H * W)
            valid = (valid if valid.dtype in (torch.bool, torch.uint8) else valid != 0).contiguous()
        key = (gt.device, F, H, W)
        if key not in self._workspace:
            self._workspace = {key: torch.empty(_lib.lpips_workspace_bytes(F, H, W), dtype=torch.uint8, device=gt.device)}
        out_map = torch.empty(F, H, W, dtype=torch.float32, device=gt.device) if want_map else None
        sums = torch.empty(F, 3, dtype=torch.float64, device=gt.device) if want_sums else None
        _lib.lpips(self.packed(), gt, pred, valid=valid, map=out_map, sums=sums, normalize=normalize, workspace=self._workspace[key])
        return out_map, sums

    def __call__(self, in0, in1, normalize=False):
        """in0 / in1 (F, 3, H, W), as the reference feeds it, or (F, H, W, 3); the layout is read off the axis of size 3, and a
        (F, 3, H, 3) input -- either layout -- is refused.  normalize=True for images in [0, 1] (else [-1, 1])."""
        if in0.dim() != 4 or in0.shape != in1.shape:
            raise RuntimeError(f"LPIPS: need two (F, 3, H, W) or (F, H, W, 3) batches of one shape, got {tuple(in0.shape)} and "
                               f"{tuple(in1.shape)}")
        if _ambiguous(in0.shape):
            raise RuntimeError(f"LPIPS: a batch of shape {tuple(in0.shape)} is (F, 3, H, 3) channels-first and (F, H, 3, 3) "
                               "channels-last alike; call score() with (F, H, W, 3) frames")
        if in0.shape[3] == 3:
            a, b = in0, in1
        elif in0.shape[1] == 3:
            a, b = in0.permute(0, 2, 3, 1), in1.permute(0, 2, 3, 1)
        else:
            raise RuntimeError(f"LPIPS: no axis of size 3 at position 1 or 3 in {tuple(in0.shape)}")
        value, _ = self.score(a, b, normalize=normalize)
        return value.unsqueeze(1)
