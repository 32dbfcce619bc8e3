"""Frame-level callers of ``render_rays``: on-device ray generation, the chunked evaluation loop
and PSNR -- the renderer-side pieces of the reference's ``eval.py`` / ``datasets/monocular.py``.

* :func:`frame_rays`    -- NDC rays of a pinhole frame generated on the GPU
                           (reference datasets/ray_utils.py:7-106 as called at monocular.py:268-276);
                           the reference builds them on the CPU and uploads 3.5 MB per frame.
* :func:`render_frame`  -- the ray-chunk loop of ``eval.f`` (eval.py:81-110): ``test_time=True``,
                           ``perturb = noise_std = 0``, per-key concatenation.  Results stay on the GPU and
                           ``keys=`` selects what is kept (the reference copies EVERY key of every chunk
                           to the host with a blocking ``.cpu()``, eval.py:106-107; ``to_cpu=True`` does that).
                           ``to_host=`` is the asynchronous form of the same egress (row N4): the kept keys of
                           chunk i travel to PINNED host buffers on a copy stream while chunk i+1 renders.
* :func:`render_frame_sharded` -- the same frame split across the ranks of ``torch.distributed``
                           with one pixel all-gather (:mod:`nsff_pl_amd.dist`).
* :func:`psnr`          -- metrics.py:6-16.
* :func:`ssim`          -- metrics.py:19-33 (the reference's SSIM scale, see :mod:`nsff_pl_amd.metrics`).
* :func:`render_split`  -- ``python eval.py --split ...`` for ``test``, ``test_spiral``, ``test_spiral{X}`` and
                           ``test_fixview{X}_interp{Y}``: the split's camera path and times (:mod:`nsff_pl_amd.paths`), rays per
                           pose on demand, :func:`render_sequence`, and the 8-bit frames eval.py writes (eval.py:183-184, 213-214,
                           222-223; the depth image of ``save_depth``) finished on the GPU (``nsff_frame_finish``).
* :class:`SequenceScores`, :func:`evaluate_split` -- the PSNR / SSIM table of split ``test`` (eval.py:173-176, 230-255), with
                           its LPIPS row when given an :class:`nsff_pl_amd.lpips.LPIPS` (eval.py:176-178, 235, 240).
* :func:`flow_frames`, :class:`FlowScores` -- the flow panel of the reference's test.ipynb: the induced optical flow of every
                           training pose, its colour image beside the dataset's flow, and the end-point error (``nsff_flow_maps``).
* :func:`track_panel`   -- a frame with the motion trails of its dynamic surface: chained scene-flow tracks both ways in time
                           (:mod:`nsff_pl_amd.tracks`: ``nsff_track_step``, ``nsff_track_draw``).
"""
import os

import numpy as np
import torch

from . import _lib
from . import dist as ndist
from .rendering import render_rays


def frame_rays(K, c2w, H, W, near=1.0, device="cuda", first_pixel=0, n_pixels=None):
    """(n_pixels, 6) NDC rays of the frame with intrinsics K (3,3) and pose c2w (3,4).

    Same conventions as the reference dataset: pixel order row-major, no +0.5 centring,
    ``shift_near = -min(-1, c2w[2,3])`` (monocular.py:270).
    """
    K = torch.as_tensor(K, dtype=torch.float32).cpu()
    c2w = torch.as_tensor(c2w, dtype=torch.float32).cpu()
    n = H * W - first_pixel if n_pixels is None else n_pixels
    shift_near = -min(-1.0, float(c2w[2, 3]))
    rays = torch.empty(n, 6, device=device, dtype=torch.float32)
    with torch.cuda.device(rays.device):
        _lib.frame_rays([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], c2w.reshape(-1).tolist(), H, W, near, shift_near,
                        first_pixel, n, rays)
    return rays


_COPY_STREAM = {}


class PinnedPool:
    """Page-locked host buffers for ``render_frame(..., to_host=pool)``, reused frame after frame (hipHostMalloc is slow)
    WITHOUT handing the same memory to two live frames: the pool keeps ``depth`` buffer sets and rotates through them, so
    a returned :class:`HostFrame` stays valid until ``depth`` further frames have been rendered into the same pool
    (``depth=2``: frames t and t+1 of a time interpolation can be held together).  Before a set is written again the pool
    waits for the copies of the frame that last used it, so ``sync=False`` frames never race each other."""

    def __init__(self, depth=2, dtype=torch.float32):
        if depth < 1:
            raise ValueError("PinnedPool depth must be >= 1")
        self.depth, self._turn, self.dtype = int(depth), 0, dtype
        self._sets = [dict() for _ in range(self.depth)]     # slot -> {(key, shape): tensor}
        self._last = [None] * self.depth                     # slot -> the HostFrame that was handed this set

    def next_slot(self):
        slot = self._turn % self.depth
        self._turn += 1
        old = self._last[slot]
        if old is not None:
            old.wait()                                        # its copies must have landed before the set is rewritten
            old.stale = True
        return slot

    def buffer(self, slot, key, shape):
        ck = (key, tuple(shape))
        bufs = self._sets[slot]
        if ck not in bufs:
            bufs[ck] = torch.empty(*shape, dtype=self.dtype, pin_memory=True)
        return bufs[ck]


class HostFrame(dict):
    """Result of ``render_frame(..., to_host=...)``: {key: pinned host tensor}.  The device-to-host copies may still be
    in flight on the copy stream; ``wait()`` (or ``render_frame(..., sync=True)``, the default) blocks until they landed.
    ``stale`` turns True once a :class:`PinnedPool` has handed this frame's buffers to a later frame."""
    event = None
    stale = False

    def wait(self):
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        return self


@torch.no_grad()
def render_frame(models, embeddings, rays, ts, max_t, N_samples, N_importance, chunk=1024 * 32,
                 keys=None, to_cpu=False, to_host=None, sync=True, graph=None, **kwargs):
    """Batched inference on the rays of one frame (reference eval.py:81-110).

    keys: iterable of result keys to keep (default: all, like the reference).
    to_cpu=True: the reference's egress -- a blocking ``.cpu()`` of every kept key after every chunk (eval.py:106-107).
    to_host=True | PinnedPool | {key: pinned tensor}: asynchronous egress -- the kept keys of each chunk are copied into
    frame-sized page-locked host buffers on a side stream while the next chunk renders; returns a :class:`HostFrame` of
    host tensors (``sync=False`` leaves the last copies in flight: call ``.wait()``).  ``True`` allocates FRESH buffers
    for this call (no two frames ever share memory); a :class:`PinnedPool` reuses ``depth`` rotating buffer sets (a frame
    is valid until ``depth`` later frames went through the pool); a dict supplies caller-owned buffers per key.
    graph: a :class:`nsff_pl_amd.graphs.GraphedRender` built with this call's flags (test_time=True, perturb = noise_std = 0):
    every chunk is one replayed hipGraph (one capture per distinct chunk size); kept tensors are copied out of the graph's
    buffers, so the returned frame is the caller's.
    """
    B = rays.shape[0]
    results = {}
    host, copy_stream = None, None
    if to_host:
        dev = rays.device
        if dev not in _COPY_STREAM:
            _COPY_STREAM[dev] = torch.cuda.Stream(device=dev)
        copy_stream = _COPY_STREAM[dev]
        host = HostFrame()
        given = to_host if isinstance(to_host, dict) else {}
        pool = to_host if isinstance(to_host, PinnedPool) else None
        slot = pool.next_slot() if pool is not None else None
    for i in range(0, B, chunk):
        kw = dict(kwargs)
        for per_ray in ("view_dir", "t_embedded", "a_embedded"):
            if per_ray in kw and kw[per_ray] is not None:
                kw[per_ray] = kw[per_ray][i:i + chunk]
        if graph is not None:
            out = graph(rays[i:i + chunk], None if ts is None else ts[i:i + chunk])
            out = {k: v.clone() for k, v in out.items() if keys is None or k in keys}    # (the graph owns its outputs)
        else:
            out = render_rays(models, embeddings, rays[i:i + chunk], None if ts is None else ts[i:i + chunk],
                              max_t, N_samples, 0, 0, N_importance, chunk, test_time=True, **kw)
        kept = {k: v for k, v in out.items() if keys is None or k in keys}
        if host is not None:
            done = torch.cuda.Event()
            done.record()                                     # this chunk's kernels, on the render stream
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(done)
                for k, v in kept.items():
                    if k not in host:
                        shape = (B,) + tuple(v.shape[1:])
                        if k in given:
                            host[k] = given[k]
                        elif pool is not None:
                            host[k] = pool.buffer(slot, k, shape)
                        else:
                            host[k] = torch.empty(*shape, dtype=torch.float32, pin_memory=True)
                        if tuple(host[k].shape) != shape or not host[k].is_pinned():
                            raise ValueError(f"to_host['{k}'] must be a pinned float32 tensor of shape {shape}")
                    host[k][i:i + v.shape[0]].copy_(v, non_blocking=True)
                    v.record_stream(copy_stream)              # the allocator must not recycle it before the copy ran
            continue
        for k, v in kept.items():
            results.setdefault(k, []).append(v.cpu() if to_cpu else v)
    if host is not None:
        host.event = torch.cuda.Event()
        host.event.record(copy_stream)
        if pool is not None:
            pool._last[slot] = host
        return host.wait() if sync else host
    return {k: v[0] if len(v) == 1 else torch.cat(v, 0) for k, v in results.items()}


@torch.no_grad()
def render_frame_sharded(models, embeddings, rays, ts, max_t, N_samples, N_importance, chunk=1024 * 32,
                         gather_keys=ndist.DEFAULT_PIXEL_KEYS, **kwargs):
    """Every rank passes the full frame; rank r renders block r; pixels are all-gathered (one collective)."""
    def fn(models_, embeddings_, rays_, ts_, *a, **kw):
        return render_frame(models_, embeddings_, rays_, ts_, max_t, N_samples, N_importance, chunk,
                            keys=gather_keys, **kw)
    merged, _ = ndist.render_rays_sharded(fn, models, embeddings, rays, ts, gather_keys=gather_keys, **kwargs)
    return merged


def render_sequence_sharded(models, embeddings, samples, max_t, N_samples, N_importance, img_wh, chunk=1024 * 32,
                            gather_keys=ndist.DEFAULT_PIXEL_KEYS, **kwargs):
    """The plain frame loop (``interp == 0``) of :func:`render_sequence` with the rays of every frame sharded over the ranks:
    rank r renders block r of each frame, and the ONE pixel all-gather of frame k runs on a side stream while frame k + 1
    renders (:func:`nsff_pl_amd.dist.all_gather_pixels_async`).  Yields ``(name, rgb (h,w,3), depth (h,w))``
    with the complete image on every rank, values clipped like eval.py:218-222 -- one frame behind the renders."""
    import torch.distributed as dist
    w, h = img_wh
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    pending = None

    def emit(item):
        name, handle = item
        px = handle.wait()
        return name, torch.clip(px['rgb_fine'].view(h, w, 3), 0, 1), px['depth_fine'].view(h, w)
    for i, sample in enumerate(samples):
        rays, ts = sample['rays'], sample.get('ts')
        bounds = [ndist.shard_bounds(rays.shape[0], world, r) for r in range(world)]
        lo, hi = bounds[rank]
        kw = dict(kwargs)
        for per_ray in ("view_dir", "t_embedded", "a_embedded"):
            if per_ray in kw and kw[per_ray] is not None:
                kw[per_ray] = kw[per_ray][lo:hi]
        # (the scope is entered per frame, not around the generator's yields: the caller's own launches between two frames keep
        # the process default, and an abandoned generator leaves nothing changed)
        with ndist.beside_a_collective():
            local = render_frame(models, embeddings, rays[lo:hi], None if ts is None else ts[lo:hi], max_t, N_samples,
                                 N_importance, chunk, keys=gather_keys, **kw)
        handle = ndist.all_gather_pixels_async(local, gather_keys, counts=[b - a for a, b in bounds])
        if pending is not None:
            yield emit(pending)                     # frame i - 1: its gather ran beside this frame's render
        pending = (f"{i:03d}", handle)
    if pending is not None:
        yield emit(pending)


def render_sequence(models, embeddings, samples, max_t, N_samples, N_importance, img_wh, chunk=1024 * 32, interp=0,
                    K=None, **kwargs):
    """The frame loop of the reference's ``eval.py`` (:171-222) as a generator of ``(name, rgb (h,w,3), depth (h,w))``
    GPU tensors, values clipped like there.

    samples: sequence of dicts ``{'rays': (h*w,6) [, 'ts': (h*w,) long] [, 'c2w': (3,4)]}`` (what the dataset yields).
    interp == 0: one image per sample (splits ``test`` / ``test_spiral``), named ``'{i:03d}'``.
    interp  > 0: the fixed-view time interpolation of split ``test_fixview*_interp{N}`` (:176-213): frame i is rendered
    once, re-used as the left end of the next pair (``last_results``), frame i+1 is rendered at ``ts + 1`` and
    ``interp - 1`` in-between images come from :func:`nsff_pl_amd.interpolate`; names ``'{i:03d}_{int(dt*100):03d}'``;
    the last sample only closes the sequence.  ``kwargs`` must then ask for ``output_transient_flow=['fw','bw']``."""
    from .interpolation import interpolate
    w, h = img_wh
    n = len(samples)
    last = None
    for i, sample in enumerate(samples):
        rays = sample['rays']
        ts = sample.get('ts')
        if interp > 0 and i == n - 1:                                   # eval.py:172-180: last frame closes the sequence
            yield f"{i:03d}_000", torch.clip(last['rgb_fine'].view(h, w, 3), 0, 1), last['depth_fine'].view(h, w)
            return
        res = last if last is not None else render_frame(models, embeddings, rays, ts, max_t, N_samples, N_importance,
                                                         chunk, **kwargs)
        if interp > 0:
            nxt = render_frame(models, embeddings, rays, ts + 1, max_t, N_samples, N_importance, chunk, **kwargs)
            for j in range(interp):
                dt = j / interp
                if j == 0:
                    img, depth = res['rgb_fine'].view(h, w, 3), res['depth_fine'].view(h, w)
                else:
                    img, depth = interpolate(res, nxt, dt, K, sample['c2w'], (w, h))
                yield f"{i:03d}_{int(dt * 100):03d}", torch.clip(img, 0, 1), depth
            last = nxt
        else:
            yield f"{i:03d}", torch.clip(res['rgb_fine'].view(h, w, 3), 0, 1), res['depth_fine'].view(h, w)


def psnr(image_pred, image_gt, valid_mask=None):
    """-10 log10(mean squared error) (reference metrics.py:6-16)."""
    err = (image_pred - image_gt) ** 2
    if valid_mask is not None:
        err = err[valid_mask]
    return -10 * torch.log10(err.mean())


def ssim(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """The reference's SSIM metric (metrics.py:19-33, kornia 0.5.4 window 11) of one (H, W, 3) frame, in this module's
    (pred, gt) argument order: one HIP launch, see :func:`nsff_pl_amd.metrics.ssim`."""
    from . import metrics
    return metrics.ssim(image_gt, image_pred, valid_mask=valid_mask, reduction=reduction)


class SplitSamples:
    """The samples of a test split as the reference's dataset yields them (monocular.py:256-278), made on demand: item i holds
    the NDC rays of pose i (one ``nsff_frame_rays`` launch), its time index for every ray and the pose -- never more than the
    frame being rendered."""

    def __init__(self, K, poses_test, ts, img_wh, device):
        self.K, self.poses, self.ts, self.img_wh, self.device = K, poses_test, ts, img_wh, device

    def __len__(self):
        return len(self.poses)

    def __getitem__(self, i):
        if not 0 <= i < len(self.poses):
            raise IndexError(i)
        w, h = self.img_wh
        c2w = torch.as_tensor(self.poses[i], dtype=torch.float32)
        return {'rays': frame_rays(self.K, c2w, h, w, device=self.device),
                'ts': torch.full((h * w,), int(self.ts[i]), dtype=torch.long, device=self.device), 'c2w': c2w}

    def __iter__(self):
        return (self[i] for i in range(len(self)))


def _split_frames(models, embeddings, K, poses, split, img_wh, N_samples, N_importance, chunk, kwargs):
    """(names, generator of render_sequence's (name, rgb, depth)) of a split; eval.py:134-141 for the flow outputs."""
    from . import paths
    poses_test, ts, interp = paths.split_path(poses, split)
    device = next(next(iter(models.values())).parameters()).device
    K = torch.as_tensor(np.asarray(K, dtype=np.float64) if not torch.is_tensor(K) else K, dtype=torch.float32).cpu()
    kw = dict(kwargs)
    if interp > 0:
        kw['output_transient'] = True
        kw['output_transient_flow'] = ['fw', 'bw']
    samples = SplitSamples(K, poses_test, ts, img_wh, device)
    frames = render_sequence(models, embeddings, samples, len(poses) - 1, N_samples, N_importance, img_wh, chunk=chunk,
                             interp=interp, K=K, **kw)
    return paths.frame_names(len(poses_test), interp), frames


def render_split(models, embeddings, K, poses, split, img_wh, N_samples, N_importance, chunk=1024 * 32, depth=False, lut=None,
                 to_host=False, **kwargs):
    """``python eval.py --split SPLIT`` as a generator of ``(name, rgb_u8 (h,w,3) uint8, depth image or None)``.

    K (3,3) intrinsics, poses (N,3,4) the dataset's poses (max_t = N - 1), split one of ``test``, ``test_spiral``,
    ``test_spiral{X}``, ``test_fixview{X}_interp{Y}`` (:func:`nsff_pl_amd.paths.split_path`; Y > 0 turns on the transient and
    flow outputs, eval.py:136-138).  Names and frame count are eval.py's: ``'{i:03d}'``, or ``'{i:03d}_{int(dt*100):03d}'`` with
    ``(N-1) Y + 1`` frames.  rgb_u8 is ``(255 * clip(rgb_fine, 0, 1)).astype(uint8)``; with ``depth=True`` the third item is the
    image of ``save_depth`` (eval.py:113-118): ``lut[index]`` (h,w,3) for a (256,3) uint8 colour table ``lut`` (what
    ``cv2.applyColorMap`` looks up), the index image (h,w) without one.  Frames are GPU tensors; ``to_host=True`` yields
    page-locked host tensors instead, copied on the copy stream while the next frame renders (a yielded frame stays valid
    until two further frames have been taken from the generator)."""
    from . import metrics
    w, h = img_wh
    names, frames = _split_frames(models, embeddings, K, poses, split, img_wh, N_samples, N_importance, chunk, kwargs)
    pool = PinnedPool(depth=4, dtype=torch.uint8) if to_host else None
    scratch, pending = None, None

    def land(item):
        name, host = item
        host.wait()
        return name, host['rgb_u8'], host.get('depth')
    for name, (_, rgb, dep) in zip(names, frames):
        if scratch is None and depth:
            scratch = torch.zeros(_lib.frame_finish_scratch_bytes(1, h, w), dtype=torch.uint8, device=rgb.device)
        out = metrics.finish_frames(rgb.reshape(1, h, w, 3), depth=dep.reshape(1, h, w) if depth else None, lut=lut,
                                    scratch=scratch)
        img = out['rgb_u8'][0]
        dimg = (out['depth_rgb_u8'][0] if 'depth_rgb_u8' in out else out['depth_u8'][0]) if depth else None
        if pool is None:
            yield name, img, dimg
            continue
        dev = img.device
        if dev not in _COPY_STREAM:
            _COPY_STREAM[dev] = torch.cuda.Stream(device=dev)
        copy_stream = _COPY_STREAM[dev]
        slot = pool.next_slot()
        host = HostFrame()
        done = torch.cuda.Event()
        done.record()                                         # this frame's finishing launches, on the render stream
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(done)
            for key, t in (('rgb_u8', img), ('depth', dimg)):
                if t is not None:
                    host[key] = pool.buffer(slot, key, tuple(t.shape))
                    host[key].copy_(t, non_blocking=True)
                    t.record_stream(copy_stream)
            host.event = torch.cuda.Event()
            host.event.record(copy_stream)
        pool._last[slot] = host
        if pending is not None:
            yield land(pending)                               # frame i - 1: its copy ran beside this frame's render
        pending = (name, host)
    if pending is not None:
        yield land(pending)


class SequenceScores:
    """The score arrays of eval.py's split ``test`` (:173-176, 230-255): PSNR and SSIM per frame over the whole image (column 0)
    and over ``mask == 0`` (column 1; 0 for a frame scored without a mask, NaN for a mask that leaves no pixel).  ``add`` runs
    one ``nsff_frame_finish`` and one ``nsff_ssim`` call per frame and keeps the values on the GPU; nothing is read back before
    ``psnrs`` / ``ssims`` are asked for.

    With ``lpips_model`` (an :class:`nsff_pl_amd.lpips.LPIPS`) ``add`` also scores ``metrics.lpips`` on the clipped frame
    (eval.py:235, 240: one ``nsff_lpips`` call for both columns), ``lpipss`` is the third (N, 2) array, ``means`` returns three
    arrays, ``table`` ends with eval.py:255's line and ``save`` writes ``lpips.npy``; without one everything is as before."""

    def __init__(self, lpips_model=None):
        self.lpips_model = lpips_model
        self._rows = []                                        # per frame: (4,) fp32 GPU tensor [psnr, psnr_m, ssim, ssim_m]
        self._lpips_rows = []                                  # per frame: (2,) fp32 GPU tensor [lpips, lpips_m]
        self._scratch = {}
        self.last = None                                       # finish_frames' outputs of the last frame added

    def add(self, img_gt, rgb, mask=None):
        """img_gt (h,w,3) fp32, rgb (h,w,3) fp32 (raw or clipped), mask (h,w) or None -- non-zero marks the dynamic pixels that
        column 1 leaves out (eval.py:237-239 passes ``mask == 0``)."""
        from . import metrics
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        gt = img_gt.reshape(1, h, w, 3).contiguous()
        valid = None if mask is None else (mask.reshape(1, h, w) == 0)
        key = (rgb.device, h, w)
        if key not in self._scratch:
            self._scratch[key] = torch.zeros(_lib.frame_finish_scratch_bytes(1, h, w), dtype=torch.uint8, device=rgb.device)
        out = metrics.finish_frames(rgb.reshape(1, h, w, 3), gt=gt, valid_mask=valid, scratch=self._scratch[key])
        p, pm = metrics.psnr_from_sums(out['sums'], h * w)
        _, s, sm = metrics.ssim_maps(gt, out['rgb_clipped'], valid)
        zero = torch.zeros_like(p)
        self._rows.append(torch.cat([p, zero if mask is None else pm, s, zero if mask is None else sm]))
        if self.lpips_model is not None:
            _, l, lm = metrics.lpips_frames(self.lpips_model, gt, out['rgb_clipped'], valid)
            self._lpips_rows.append(torch.cat([l, zero if mask is None else lm]))
        self.last = out
        return out

    def __len__(self):
        return len(self._rows)

    def _table(self):
        if not self._rows:
            return np.zeros((0, 4))
        return torch.stack(self._rows).double().cpu().numpy()

    @property
    def psnrs(self):
        return self._table()[:, 0:2]

    @property
    def ssims(self):
        return self._table()[:, 2:4]

    @property
    def lpipss(self):
        """(N, 2), eval.py's ``lpipss``; needs ``lpips_model``."""
        if self.lpips_model is None:
            raise AttributeError("SequenceScores: no lpipss without an lpips_model")
        if not self._lpips_rows:
            return np.zeros((0, 2))
        return torch.stack(self._lpips_rows).double().cpu().numpy()

    def means(self):
        """(mean_psnr (2,), mean_ssim (2,)) -- and mean_lpips (2,) with an lpips_model: np.nanmean over the frames
        (eval.py:243-245)."""
        means = np.nanmean(self.psnrs, 0), np.nanmean(self.ssims, 0)
        return means if self.lpips_model is None else means + (np.nanmean(self.lpipss, 0),)

    def table(self):
        """The lines eval.py:251-254 prints, and :255 with an lpips_model."""
        return format_scores(*self.means())

    def save(self, dir_name):
        os.makedirs(dir_name, exist_ok=True)
        np.save(os.path.join(dir_name, 'psnr.npy'), self.psnrs)
        np.save(os.path.join(dir_name, 'ssim.npy'), self.ssims)
        if self.lpips_model is not None:
            np.save(os.path.join(dir_name, 'lpips.npy'), self.lpipss)


def format_scores(mean_psnr, mean_ssim, mean_lpips=None):
    """eval.py:251-254: header, rule, PSNR row, SSIM row -- a list of lines; with mean_lpips the LPIPS row of :255 as well."""
    lines = ['Score \t Whole image  \t Dynamic only',
             '-------------------------------------',
             f'PSNR  \t {mean_psnr[0]:.4f} \t {mean_psnr[1]:.4f}',
             f'SSIM  \t {mean_ssim[0]:.4f} \t {mean_ssim[1]:.4f}']
    if mean_lpips is not None:
        lines.append(f'LPIPS \t {mean_lpips[0]:.4f} \t {mean_lpips[1]:.4f}')
    return lines


def evaluate_split(models, embeddings, K, poses, img_wh, N_samples, N_importance, images_gt, masks=None, chunk=1024 * 32,
                   sink=None, lpips_model=None, **kwargs):
    """Render split ``test`` and score it against the ground truth in one loop (eval.py:181-240): images_gt (N,h,w,3) fp32 GPU
    frames (or a sequence of them), masks (N,h,w) or None.  ``sink(name, rgb_u8)`` receives every 8-bit frame (a GPU tensor of
    the frame just scored) when given.  lpips_model: an :class:`nsff_pl_amd.lpips.LPIPS` adds the LPIPS scores.  Returns the
    :class:`SequenceScores`."""
    if len(images_gt) != len(poses) or (masks is not None and len(masks) != len(poses)):
        raise ValueError(f"evaluate_split: {len(poses)} poses need as many ground-truth frames"
                         f"{'' if masks is None else ' and masks'}, got {len(images_gt)}"
                         f"{'' if masks is None else ' and ' + str(len(masks))}")
    names, frames = _split_frames(models, embeddings, K, poses, 'test', img_wh, N_samples, N_importance, chunk, kwargs)
    scores = SequenceScores(lpips_model=lpips_model)
    for i, (name, (_, rgb, _)) in enumerate(zip(names, frames)):
        out = scores.add(images_gt[i], rgb, None if masks is None else masks[i])
        if sink is not None:
            sink(name, out['rgb_u8'][0])
    return scores


class FlowScores:
    """End-point error of the induced flow per frame: ``epe`` (N, 2 directions [fw, bw], 3 selections [all, dynamic = mask != 0,
    static = mask == 0]) in pixels, NaN where nothing was counted (no ground truth, an edge frame's missing neighbour, no mask).
    ``add`` keeps the sums and counts of ``nsff_flow_maps`` on the GPU; nothing is read back before ``epe`` / ``counts`` are asked
    for."""

    def __init__(self):
        self._sums, self._counts = [], []                      # per frame: (2, 3) fp64 / int64 GPU tensors

    def add(self, sums, counts):
        self._sums.append(sums.reshape(2, 3))
        self._counts.append(counts.reshape(2, 3))

    def __len__(self):
        return len(self._sums)

    @property
    def counts(self):
        if not self._counts:
            return np.zeros((0, 2, 3), np.int64)
        return torch.stack(self._counts).cpu().numpy()

    @property
    def epe(self):
        if not self._sums:
            return np.zeros((0, 2, 3))
        from . import flow
        return flow.epe_from_sums(torch.stack(self._sums), torch.stack(self._counts)).cpu().numpy()

    def means(self):
        """(2, 3): np.nanmean over the frames, per direction and selection (NaN where no frame has a value)."""
        epe = self.epe
        out = np.full((2, 3), np.nan)
        if len(epe):
            have = ~np.isnan(epe).all(0)
            out[have] = np.nanmean(epe[:, have], 0)
        return out

    def table(self):
        """Lines in the manner of :func:`format_scores`."""
        m = self.means()
        return ['EPE   \t Whole image  \t Dynamic only \t Static only',
                '---------------------------------------------------',
                f'fw    \t {m[0, 0]:.4f} \t {m[0, 1]:.4f} \t {m[0, 2]:.4f}',
                f'bw    \t {m[1, 0]:.4f} \t {m[1, 1]:.4f} \t {m[1, 2]:.4f}']

    def save(self, dir_name):
        os.makedirs(dir_name, exist_ok=True)
        np.save(os.path.join(dir_name, 'epe.npy'), self.epe)
        np.save(os.path.join(dir_name, 'epe_counts.npy'), self.counts)


class FlowFrames:
    """What :func:`flow_frames` returns: an iterator of ``(name, maps)`` whose ``scores`` (:class:`FlowScores`) fill as it runs."""

    def __init__(self, generator, scores):
        self._generator, self.scores = generator, scores

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._generator)

    def close(self):
        self._generator.close()


def flow_frames(models, embeddings, K, poses, img_wh, N_samples, N_importance, chunk=1024 * 32, frames=None, flows_fw=None,
                flows_bw=None, masks=None, maxrad=None, to_host=False, **kwargs):
    """The flow panel of the reference's test.ipynb for the training poses, on the GPU: an iterator of ``(name, maps)`` with a
    ``scores`` attribute (:class:`FlowScores`).

    K (3,3), poses (N,3,4) the dataset's poses (frame i is rendered from pose i at time i, max_t = N - 1); ``frames``: the pose
    indices to do (default all).  Each frame is rendered with ``output_transient=True, output_transient_flow=['fw','bw']``, its
    expected warped points ``xyz_fw`` / ``xyz_bw`` go through ``nsff_flow_maps`` (:mod:`nsff_pl_amd.flow`), and ``maps`` holds
    ``flow_fw`` / ``flow_bw`` (h,w,2) fp32 -- :data:`nsff_pl_amd.flow.UNKNOWN` where a pixel has no valid projection, as in all of
    frame N-1's forward and frame 0's backward map -- and their colour images ``flow_fw_u8`` / ``flow_bw_u8`` (h,w,3) uint8.
    flows_fw / flows_bw (N,h,w,2) fp32 GPU tensors, the dataset's flow: ``gt_fw_u8`` / ``gt_bw_u8`` join them, prediction and ground
    truth are coloured on the ground truth's largest radius, and the end-point error of every frame goes to ``scores`` -- over the
    whole frame and, with masks (N,h,w; non-zero = dynamic), over the dynamic and the static pixels.  ``maxrad``: colour everything on
    this radius instead.  Names are eval.py's ``'{i:03d}'``.  ``to_host=True`` yields page-locked host tensors instead, copied on the
    copy stream while the next frame renders (a yielded frame stays valid until two further frames have been taken)."""
    model = models['fine']
    if not getattr(model, "has_flow_heads", False):
        raise RuntimeError("flow_frames: models['fine'] has no scene-flow heads (NeRF(..., encode_transient=True, output_flow=True)): "
                           "there are no warped points to project")
    n = len(poses)
    todo = list(range(n)) if frames is None else [int(i) for i in frames]
    if any(not 0 <= i < n for i in todo):
        raise ValueError(f"flow_frames: frames {todo} outside the sequence of {n} poses")
    w, h = (int(v) for v in img_wh)
    for t, what, last in ((flows_fw, "flows_fw", (h, w, 2)), (flows_bw, "flows_bw", (h, w, 2)), (masks, "masks", (h, w))):
        if t is not None:
            _lib.require_gpu_tensor(t, f"flow_frames: {what}")
            if tuple(t.shape) != (n,) + last:
                raise RuntimeError(f"flow_frames: {what} must be {(n,) + last}, got {tuple(t.shape)}")
    if (flows_fw is None) != (flows_bw is None):
        raise ValueError("flow_frames: flows_fw and flows_bw go together (a frame without a neighbour on one side has zero flow "
                         "there, as in the ray records)")
    scores = FlowScores()
    return FlowFrames(_flow_frames(models, embeddings, K, poses, (w, h), N_samples, N_importance, chunk, todo, flows_fw, flows_bw,
                                   masks, maxrad, to_host, scores, kwargs), scores)


def _flow_frames(models, embeddings, K, poses, img_wh, N_samples, N_importance, chunk, todo, flows_fw, flows_bw, masks, maxrad,
                 to_host, scores, kwargs):
    from . import flow, paths
    from . import frames as nframes
    w, h = img_wh
    n = len(poses)
    device = next(models['fine'].parameters()).device
    K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64).reshape(3, 3)
    K4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    Ps = nframes.projection_matrices(K, poses)[1][0].to(device).contiguous()
    K = torch.as_tensor(K, dtype=torch.float32)
    names = paths.frame_names(n)
    kw = dict(kwargs, output_transient=True, output_transient_flow=['fw', 'bw'])
    gts = (flows_fw, flows_bw)
    have_gt = any(g is not None for g in gts)
    scratch = torch.zeros(_lib.flow_maps_scratch_bytes(1, h, w), dtype=torch.uint8, device=device)
    scale = None if maxrad is None else flow._scale(maxrad, 1, device, "flow_frames")
    pools = (PinnedPool(depth=4), PinnedPool(depth=4, dtype=torch.uint8)) if to_host else None
    pending = None

    def land(item):
        name, host = item
        host.wait()
        return name, dict(host)
    for i in todo:
        pose = torch.as_tensor(np.asarray(poses[i]), dtype=torch.float32)
        rays = frame_rays(K, pose, h, w, device=device)
        ts = torch.full((h * w,), i, dtype=torch.long, device=device)
        res = render_frame(models, embeddings, rays, ts, n - 1, N_samples, N_importance, chunk, keys=('xyz_fw', 'xyz_bw'), **kw)
        gt = tuple(None if g is None else g[i:i + 1].contiguous() for g in gts)
        out = {'flow_fw': torch.empty(1, h, w, 2, device=device), 'flow_bw': torch.empty(1, h, w, 2, device=device)}
        for k in ('flow_fw_u8', 'flow_bw_u8') + tuple(f'gt_{d}_u8' for d, g in zip(('fw', 'bw'), gt) if g is not None):
            out[k] = torch.empty(1, h, w, 3, dtype=torch.uint8, device=device)
        sums = torch.empty(1, 2, 3, dtype=torch.float64, device=device) if have_gt else None
        counts = torch.empty(1, 2, 3, dtype=torch.int64, device=device) if have_gt else None
        # prediction and ground truth share the ground truth's radius unless one is given
        rad = torch.empty(1, 2, 2, device=device)
        _lib.flow_maps(1, h, w, xyz=(res['xyz_fw'].view(1, h * w, 3), res['xyz_bw'].view(1, h * w, 3)), K4=K4, Ps=Ps,
                       ts=ts[:1].to(torch.int32), max_t=n - 1, flow=(out['flow_fw'], out['flow_bw']), gt=gt,
                       mask=None if masks is None or not have_gt else _mask_u8(masks[i:i + 1]), epe_sums=sums,
                       epe_counts=counts, maxrad=rad, scale=scale, share_gt_scale=have_gt and scale is None,
                       image=(out['flow_fw_u8'], out['flow_bw_u8']), gt_image=(out.get('gt_fw_u8'), out.get('gt_bw_u8')),
                       scratch=scratch)
        if have_gt:
            scores.add(sums[0], counts[0])
        else:
            nan = torch.full((2, 3), float('nan'), dtype=torch.float64, device=device)
            scores.add(nan, torch.zeros(2, 3, dtype=torch.int64, device=device))
        maps = {k: v[0] for k, v in out.items()}
        if pools is None:
            yield names[i], maps
            continue
        if device not in _COPY_STREAM:
            _COPY_STREAM[device] = torch.cuda.Stream(device=device)
        copy_stream = _COPY_STREAM[device]
        slots = [p.next_slot() for p in pools]
        host = HostFrame()
        done = torch.cuda.Event()
        done.record()                                         # this frame's launches, on the render stream
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(done)
            for key, t in maps.items():
                which = 1 if t.dtype == torch.uint8 else 0
                host[key] = pools[which].buffer(slots[which], key, tuple(t.shape))
                host[key].copy_(t, non_blocking=True)
                t.record_stream(copy_stream)
            host.event = torch.cuda.Event()
            host.event.record(copy_stream)
        for p, s in zip(pools, slots):
            p._last[s] = host
        if pending is not None:
            yield land(pending)                               # frame i - 1: its copy ran beside this frame's render
        pending = (names[i], host)
    if pending is not None:
        yield land(pending)


@torch.no_grad()
def track_panel(models, embeddings, K, poses, t0, img_wh, N_samples, N_importance, steps, stride=16, min_alpha=0.5, lut=None,
                chunk=1024 * 32, **kwargs):
    """Frame ``t0`` with the motion trails of its dynamic surface: ``(rgb_u8 (h, w, 3) uint8, tracks)``, all on the GPU.

    K (3,3), poses (N,3,4) the dataset's poses (max_t = N - 1).  Frame t0 is rendered at its own pose; the expected surface point
    ``xyz_fine`` of every ``stride``-th pixel of every ``stride``-th row whose ``transient_alpha_fine >= min_alpha`` is followed
    ``steps`` frames forward and ``steps`` frames backward through the scene-flow field (:func:`nsff_pl_amd.tracks.advect`), every step
    is projected with the fixed camera of pose t0, and both families of trails are drawn on the finished 8-bit frame
    (:func:`nsff_pl_amd.metrics.finish_frames`, :func:`nsff_pl_amd.tracks.draw`; lut: its (256, 3) colour table), the backward family
    last.  ``tracks = {'fw', 'bw'}`` (advect's dicts over ALL the strided pixels, one point a row), ``'pixels'`` (Q,) their flat pixel
    indices and ``'selected'`` (Q,) bool, which of them passed min_alpha: only those are drawn -- nothing here waits for the GPU to
    learn how many there are."""
    from . import frames as nframes
    from . import metrics, tracks
    model = models['fine']
    if not getattr(model, "has_flow_heads", False):
        raise RuntimeError("track_panel: models['fine'] has no scene-flow heads (NeRF(..., encode_transient=True, output_flow=True)): "
                           "there is no flow to follow")
    n = len(poses)
    t0, steps, stride = int(t0), int(steps), int(stride)
    if not 0 <= t0 < n:
        raise ValueError(f"track_panel: t0 = {t0} is outside the sequence of {n} poses")
    if steps < 1 or stride < 1:
        raise ValueError(f"track_panel: steps and stride must be positive, got {steps} and {stride}")
    w, h = (int(v) for v in img_wh)
    device = next(model.parameters()).device
    K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64).reshape(3, 3)
    view = nframes.projection_matrices(K, poses)[1][0][t0].to(device).contiguous()
    rays = frame_rays(torch.as_tensor(K, dtype=torch.float32), torch.as_tensor(np.asarray(poses[t0]), dtype=torch.float32), h, w,
                      device=device)
    ts = torch.full((h * w,), t0, dtype=torch.long, device=device)
    res = render_frame(models, embeddings, rays, ts, n - 1, N_samples, N_importance, chunk,
                       keys=('rgb_fine', 'xyz_fine', 'transient_alpha_fine'),
                       **dict(kwargs, output_transient=True, output_transient_flow=['fw', 'bw']))
    image = metrics.finish_frames(res['rgb_fine'].view(1, h, w, 3))['rgb_u8'][0]
    ys, xs = torch.meshgrid(torch.arange(0, h, stride, device=device), torch.arange(0, w, stride, device=device), indexing="ij")
    pixels = (ys * w + xs).reshape(-1)
    selected = res['transient_alpha_fine'][pixels] >= min_alpha
    points = res['xyz_fine'][pixels].contiguous()
    out = {'pixels': pixels, 'selected': selected}
    for key, k in (('fw', steps), ('bw', -steps)):
        out[key] = tracks.advect(model, embeddings, points, ts[pixels], k, n - 1, Ps=view, K=K)
        image = tracks.draw(image, out[key]['uv'], out[key]['alive'] & selected, lut)
    return image, out


def _mask_u8(mask):
    return (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()
