"""Chained scene-flow tracks: follow points through the trained flow field over several frames, and draw their motion trails.

``render_rays`` shows the flow heads one step at a time (``transient_flows_fw/bw``, ``xyz_fw/bw``); :func:`advect` chains them: a point
at time ``t`` is moved by the forward (backward) head of the dynamic trunk queried at ``(x, E_t[t])``, then queried again one frame
later (earlier) where it landed, ``|steps|`` times -- the query mode the reference's ``render_transient_warping`` uses
(rendering.py:98-126), its ``flows[zs > z_far] = 0`` rule restated on the point (on NDC rays ``zs = (z + 1) / 2``).  A field whose
one-step flow looks fine but drifts when chained shows here and nowhere else.

Per step: the time rows ``E_t[t_j]``, one ``nsff_field_query`` (dynamic trunk only, one flow head) and one ``nsff_track_step``
(csrc/tracks.hip), all on the current stream with no host synchronisation in between; there is no CPU path.  A row that runs out
of frames (``t = max_t`` going forward, ``t = 0`` going backward) stops where it is and is flagged in ``alive``; it is never NaN.

* :func:`advect` -- the paths, their times and liveness, and with cameras their pixels and depths;
* :func:`draw`   -- deterministic trails of projected tracks on a copy of an 8-bit image (``nsff_track_draw``).
"""
import numpy as np
import torch

from . import _lib
from . import range_check
from .flow import UNKNOWN, _host                              # noqa: F401  (UNKNOWN: the uv of a point behind its camera)


def _cameras(Ps, K, max_t, dev):
    """(Ps (n, 3, 4) on dev, fixed_view, K4) of advect's camera arguments."""
    if K is None:
        raise ValueError("advect: Ps is given without K")
    K = _host(K)
    if K.shape == (1, 3, 3):
        K = K[0]
    if K.shape != (3, 3):
        raise RuntimeError(f"advect: K must be (3,3) or (1,3,3), got {K.shape}")
    if not isinstance(Ps, torch.Tensor):
        Ps = torch.as_tensor(np.asarray(Ps), dtype=torch.float32)
    fixed = Ps.dim() == 2
    if fixed:
        Ps = Ps.unsqueeze(0)
    elif Ps.dim() == 4 and Ps.shape[0] == 1:
        Ps = Ps[0]
    if Ps.dim() != 3 or tuple(Ps.shape[1:]) != (3, 4):
        raise RuntimeError(f"advect: Ps must be (N,3,4), (1,N,3,4) or one (3,4) view, got {tuple(Ps.shape)}")
    if not fixed and max_t >= Ps.shape[0]:
        raise ValueError(f"advect: max_t = {max_t} is outside the {Ps.shape[0]} projection matrices")
    return Ps.to(device=dev, dtype=torch.float32).contiguous(), fixed, (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


@torch.no_grad()
def advect(model, embeddings, xyz, ts, steps, max_t, Ps=None, K=None, chunk=None):
    """Follow points through ``|steps|`` frames of the scene-flow field.

    model: the fine ``NeRF`` (``encode_transient`` and ``output_flow``); embeddings: ``{'xyz', 't'}``; xyz: (R, S, 3) -- or (R, 3), S = 1 --
    fp32 NDC points on the GPU, the S points of a row sharing a time; ts: (R,) integer start times in ``0 .. max_t``; steps: a
    non-zero int, > 0 along the forward head, < 0 along the backward head; max_t = N_frames - 1.  With n = |steps|, per step j and row:
    ``can = alive[j] and t_j < max_t`` (backward: ``t_j > 0``); ``x_{j+1} = x_j + f(x_j, E_t[t_j])`` where ``can`` (f = 0 where
    ``(z + 1) / 2 > 0.95``), else ``x_j``; ``t_{j+1} = t_j +- 1`` where ``can``; ``alive[j+1] = can``.

    Returns ``{'xyz': (n+1, R, S, 3) fp32, 't': (n+1, R) int32, 'alive': (n+1, R) bool}`` and, with cameras, ``'uv'`` (n+1, R, S, 2) fp32
    pixels -- :data:`UNKNOWN` in both components behind the camera -- and ``'depth'`` (n+1, R, S).  Ps: (N, 3, 4) or (1, N, 3, 4)
    world -> pixel matrices (:func:`nsff_pl_amd.frames.projection_matrices`), step j seen by the camera of its own time ``t_j``, or one
    (3, 4) fixed view; K as for :func:`nsff_pl_amd.flow.induced_flow`.  chunk: at most this many rows per pass."""
    if not isinstance(xyz, torch.Tensor):
        raise RuntimeError(f"advect: xyz must be a tensor, got {type(xyz).__name__}")
    if xyz.dtype != torch.float32:
        raise RuntimeError(f"advect: xyz must be float32, got {xyz.dtype}")
    if xyz.dim() == 2:
        xyz = xyz.unsqueeze(1)
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.shape[1] < 1:
        raise RuntimeError(f"advect: xyz must be (R, S, 3) or (R, 3), got {tuple(xyz.shape)}")
    if not (getattr(model, "encode_transient", False) and getattr(model, "has_flow_heads", hasattr(model, "transient_flow_fw"))):
        raise RuntimeError("advect: the model has no scene-flow heads (NeRF('fine', encode_transient=True, output_flow=True)): "
                           "there is no flow to follow")
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps == 0:
        raise ValueError(f"advect: steps must be a non-zero integer (> 0 forward, < 0 backward), got {steps!r}")
    n, direction = abs(int(steps)), (1 if steps > 0 else -1)
    max_t = int(max_t)
    if max_t < 0:
        raise ValueError(f"advect: max_t = {max_t} is negative")
    dev = xyz.device
    R, S = int(xyz.shape[0]), int(xyz.shape[1])
    if R * S > _lib.TRACK_MAX_POINTS:
        raise ValueError(f"advect: {R} x {S} points exceed {_lib.TRACK_MAX_POINTS}; pass them in several calls")
    if isinstance(ts, torch.Tensor):
        if ts.dtype.is_floating_point or ts.dtype == torch.bool or ts.dim() != 1 or ts.shape[0] != R:
            raise RuntimeError(f"advect: ts must be ({R},) integer start times, got {tuple(ts.shape)} {ts.dtype}")
        ts = ts.to(device=dev, dtype=torch.int32)
        if R and bool(((ts < 0) | (ts > max_t)).any()):       # (the one synchronisation of a call, before its first launch)
            raise ValueError(f"advect: ts outside 0 .. max_t = {max_t}")
    else:
        host_ts = np.asarray(ts)
        if host_ts.dtype.kind not in "iu" or host_ts.shape != (R,):
            raise RuntimeError(f"advect: ts must be ({R},) integer start times, got {host_ts.shape} {host_ts.dtype}")
        if ((host_ts < 0) | (host_ts > max_t)).any():
            raise ValueError(f"advect: ts outside 0 .. max_t = {max_t}")
        ts = torch.as_tensor(host_ts.astype(np.int32)).to(dev)
    cams = None if Ps is None else _cameras(Ps, K, max_t, dev)
    if Ps is None and K is not None:
        raise ValueError("advect: K is given without Ps")
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"advect: chunk must be at least one row, got {chunk}")
    _lib.require_gpu_tensor(xyz, "advect: xyz")              # (after the shapes: every refusal above is the same on any device)
    rows = R if chunk is None else int(chunk)
    freqs = [float(f) for f in embeddings['xyz'].freqs]
    xyz = xyz.contiguous()

    def run():
        with torch.cuda.device(dev):
            path = torch.empty(n + 1, R, S, 3, dtype=torch.float32, device=dev)
            t = torch.empty(n + 1, R, dtype=torch.int32, device=dev)
            alive = torch.empty(n + 1, R, dtype=torch.uint8, device=dev)
            path[0], t[0] = xyz, ts
            alive[0].fill_(1)
            out = {'xyz': path, 't': t, 'alive': alive.view(torch.bool)}
            cam = {}
            if cams is not None:
                out['uv'] = torch.empty(n + 1, R, S, 2, dtype=torch.float32, device=dev)
                out['depth'] = torch.empty(n + 1, R, S, dtype=torch.float32, device=dev)
                cam = dict(Ps=cams[0], fixed_view=cams[1], K4=cams[2])
            for r0 in range(0, R, max(rows, 1)):
                r1 = min(r0 + rows, R)
                P = (r1 - r0) * S
                raw = torch.empty(P, _lib.RAW_STRIDE, dtype=torch.float32, device=dev)   # (reused step after step: stream order)
                view = lambda j: dict(uv=out['uv'][j, r0:r1], depth=out['depth'][j, r0:r1]) if cams is not None else {}
                if cams is not None:                              # slab 0: the same kernel, nothing moves
                    _lib.track_step(r1 - r0, S, direction, max_t, path[0, r0:r1], t[0, r0:r1], alive[0, r0:r1], **cam, **view(0))
                for j in range(n):
                    rows_t = embeddings['t'](t[j, r0:r1].long()).detach().contiguous().float()
                    _lib.field_query(model, raw, P, S, static_mode=0, transient_mode=2, flow_heads=1, xyz=path[j, r0:r1],
                                     freqs=freqs, t_emb=rows_t)
                    _lib.track_step(r1 - r0, S, direction, max_t, path[j, r0:r1], t[j, r0:r1], alive[j, r0:r1], raw=raw,
                                    xyz_out=path[j + 1, r0:r1], t_out=t[j + 1, r0:r1], alive_out=alive[j + 1, r0:r1], **cam, **view(j + 1))
            return out
    if R == 0:
        return run()
    return range_check.checked("advect", dev, run, can_fallback=True)


def default_lut():
    """(256, 3) uint8 RGB ramp blue -> cyan -> yellow -> red: the colour of a trail's step when no table is given."""
    i = np.arange(256)
    r = np.clip(3 * i - 255, 0, 255)
    g = np.where(i < 170, np.clip(3 * i, 0, 255), np.clip(3 * (255 - i), 0, 255))
    b = np.clip(255 - 3 * i + 255, 0, 255) * (i < 170)
    return np.stack([r, g, b], -1).astype(np.uint8)


def _lut(lut, dev):
    lut = torch.as_tensor(default_lut() if lut is None else lut)
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise RuntimeError(f"draw: lut must be a (256, 3) uint8 colour table, got {tuple(lut.shape)} {lut.dtype}")
    return lut.to(dev).contiguous()


@torch.no_grad()
def draw(image_u8, uv, ok, lut=None, scratch=None):
    """Motion trails on a copy of an (H, W, 3) uint8 GPU image: ``nsff_track_draw``, deterministic.

    uv: (n+1, Q, 2) fp32 pixels of Q tracks over n steps -- or advect's (n+1, R, S, 2); ok: (n+1, Q) bool / uint8, or advect's (n+1, R)
    ``alive`` (a row's S points share it).  Segment j of a track, ``uv[j] -> uv[j+1]``, is drawn when both ends are ok, not
    :data:`UNKNOWN`, finite with ``|u|, |v| < 32768``, and at most H + W pixels long; it is coloured ``lut[(255 * (j+1)) // n]``
    (lut: (256, 3) uint8, default the depth panels' colour table), and where trails cross the later step -- among equal steps the
    higher track index -- wins.  Q < 2**20 and n < 2**11."""
    if not all(isinstance(v, torch.Tensor) for v in (image_u8, uv, ok)):
        raise RuntimeError("draw: image_u8, uv and ok must be tensors")
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[-1] != 3:
        raise RuntimeError(f"draw: image_u8 must be an (H, W, 3) uint8 image, got {tuple(image_u8.shape)} {image_u8.dtype}")
    if uv.dtype != torch.float32 or uv.dim() not in (3, 4) or uv.shape[-1] != 2 or uv.shape[0] < 2:
        raise RuntimeError(f"draw: uv must be (n+1, Q, 2) or (n+1, R, S, 2) float32 with n >= 1, got {tuple(uv.shape)} {uv.dtype}")
    n = int(uv.shape[0]) - 1
    if ok.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"draw: ok must be bool or uint8, got {ok.dtype}")
    if uv.dim() == 4 and tuple(ok.shape) == tuple(uv.shape[:2]):
        ok = ok.unsqueeze(-1).expand(uv.shape[:3])
    if tuple(ok.shape) != tuple(uv.shape[:-1]):
        raise RuntimeError(f"draw: ok must be {tuple(uv.shape[:-1])} like uv{' or ' + str(tuple(uv.shape[:2])) if uv.dim() == 4 else ''}, "
                           f"got {tuple(ok.shape)}")
    uv = uv.reshape(n + 1, -1, 2).contiguous()
    Q = int(uv.shape[1])
    if Q >= _lib.TRACK_MAX_TRACKS:
        raise ValueError(f"draw: {Q} tracks, the pixel key holds fewer than 2**20")
    if n >= _lib.TRACK_MAX_STEPS:
        raise ValueError(f"draw: {n} steps, the pixel key holds fewer than 2**11")
    for v, what in ((image_u8, "image_u8"), (uv, "uv"), (ok, "ok")):
        _lib.require_gpu_tensor(v, "draw: " + what)
    ok = ok.reshape(n + 1, Q).contiguous().view(torch.uint8)
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    dev = image_u8.device
    with torch.cuda.device(dev):
        need = _lib.track_draw_scratch_bytes(H, W)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        _lib.track_draw(H, W, n, Q, uv, ok, image_u8.contiguous(), _lut(lut, dev), out, scratch)
    return out
