"""On-device training-ray bank with the reference's SSIM-driven hard sampling (``--hard_sampling``).

The reference's training dataset (datasets/monocular.py:136-187, 217-250) keeps every frame's rays as (H*W, 16) records on the
host, picks a frame outside a +-5 window of the previous one, draws ``batch_size`` pixels -- uniformly, or with
``--hard_sampling`` in proportion to ``weights[t]`` by ``np.random.choice`` -- and the DataLoader copies the batch to the GPU.
Every validation pass (train.py:246-253) recomputes those weights, frame by frame on the CPU, as ``1 - ssim_map.mean(-1)``
between the ground truth and ``tmp_rgb``, the latest fine prediction of every training pixel (train.py:140-143, 184-185).

:class:`RayBank` holds the records, weights and ``tmp_rgb`` on the GPU:

* ``sample``         -- frame choice on the host (a seeded numpy Generator, the reference's window rule), uniforms from
                        ``torch.rand``, then ONE launch (``nsff_ray_draw``) that draws the pixels from the frame's fp64 CDF
                        (or uniformly) and gathers the record columns into the batch tensors: the batch never crosses PCIe;
* ``record``         -- ``tmp_rgb[ts, rand_idx] = rgb_fine`` (one ``index_put_``, capturable);
* ``update_weights`` -- one ``nsff_ssim`` launch over all frames writing the weights, one ``nsff_cdf`` launch (fp64 scan).

Deviations from the reference, on purpose: a frame whose weights sum to 0 or to a non-finite value draws uniformly (the
reference's ``np.random.choice`` raises); when the +-5 window leaves no frame (11 frames or fewer) the frame is drawn from all
frames (the reference's ``np.random.choice([])`` raises); one ``last_t`` per bank, not one per DataLoader worker.
``state_dict`` carries the weights and ``tmp_rgb`` (the reference's TODO at monocular.py:235).

``RayBank.from_frames`` builds the records themselves on the GPU from decoded frames, poses and flow (one launch,
:mod:`nsff_pl_amd.frames`) and keeps the loss's ``Ks`` / ``Ps``; ``frame_sample`` is the validation split's full-frame sample.
"""
import numpy as np
import torch

from . import _lib

WINDOW = 5                      # monocular.py:228  w_size


class RayBank:
    """records: (N_frames, H*W, 16) fp32 in monocular.py:180-183's column layout (rays_o, rays_d, rgb, t, disp, mask, uv_fw,
    uv_bw), or a dict {t: (H*W, 16)} like the reference's ``rays_dict``; img_wh = (W, H).  The bank may be built on the CPU
    (state handling); ``sample`` / ``update_weights`` need it on the GPU (``.to('cuda')``)."""

    def __init__(self, records, img_wh, hard_sampling=False, seed=None, device=None):
        if isinstance(records, dict):
            records = torch.stack([torch.as_tensor(records[t]) for t in range(len(records))])
        records = torch.as_tensor(records, dtype=torch.float32)
        W, H = (int(v) for v in img_wh)
        if records.dim() != 3 or records.shape[1] != H * W or records.shape[2] != _lib.RAY_RECORD:
            raise ValueError(f"RayBank: records must be (N_frames, {H}*{W}, {_lib.RAY_RECORD}), got {tuple(records.shape)}")
        if device is not None:
            records = records.to(device)
        self.img_wh = (W, H)
        self.n_frames = int(records.shape[0])
        self.hard_sampling = bool(hard_sampling)
        self.records = records.contiguous()
        self.rgb = self.records[..., 6:9].contiguous()                   # ground truth as (F, H*W, 3) for the SSIM launch
        dev = self.records.device
        self.weights = torch.ones(self.n_frames, H * W, device=dev)      # monocular.py:186-187
        self.tmp_rgb = torch.zeros(self.n_frames, H * W, 3, device=dev)  # train.py:142
        self._cdf = None                                                 # fp64 CDF of `weights`, rebuilt when stale
        self.rng = np.random.default_rng(seed)
        self.last_t = -1
        self.Ks = self.Ps = None                                         # set by from_frames (monocular.py:127-134)

    @classmethod
    def from_frames(cls, K, poses, images, disps, masks, flows_fw, flows_bw, img_wh, hard_sampling=False, seed=None, resize=False):
        """The bank of decoded frames (GPU tensors at the target resolution, see :func:`frames.build_records`): the records
        come from one launch, and ``Ks`` (1,3,3) / ``Ps`` (1,F,3,4) are what the loss projects with, so
        ``NSFFTrainer(..., Ks=bank.Ks, Ps=bank.Ps, ray_bank=bank)`` is the whole set-up.  ``resize=True``: the frames come at
        their native sizes and go through :func:`frames.resize_frames` to img_wh first (K is the one at img_wh:
        :func:`frames.scaled_intrinsics`)."""
        from . import frames
        if resize:
            d = frames.resize_frames(images, disps, masks, flows_fw, flows_bw, img_wh)
            images, disps, masks, flows_fw, flows_bw = d["images"], d["disps"], d["masks"], d["flows_fw"], d["flows_bw"]
        records = frames.build_records(K, poses, images, disps, masks, flows_fw, flows_bw)
        bank = cls(records, img_wh, hard_sampling=hard_sampling, seed=seed)
        Ks, Ps = frames.projection_matrices(K, poses)
        bank.Ks, bank.Ps = Ks.to(records.device), Ps.to(records.device)
        return bank

    def to(self, device):
        for k in ("records", "rgb", "weights", "tmp_rgb", "Ks", "Ps"):
            if getattr(self, k) is not None:
                setattr(self, k, getattr(self, k).to(device))
        self._cdf = None
        return self

    # ---- host side: which frame (monocular.py:222-232) ----
    def next_frame(self):
        """Uniform the first time, then uniform over the frames outside last_t +- 5."""
        if self.last_t == -1:
            t = int(self.rng.integers(self.n_frames))
        else:
            lo, hi = self.last_t - WINDOW, self.last_t + WINDOW
            valid = [i for i in range(self.n_frames) if not lo <= i <= hi]
            t = int(self.rng.choice(valid)) if valid else int(self.rng.integers(self.n_frames))
        self.last_t = t
        return t

    def batch_spec(self, batch_size):
        """{key: (shape, dtype)} of a batch from :meth:`sample` (the reference's keys; + rand_idx with hard sampling)."""
        spec = {"rays": ((batch_size, 6), torch.float32), "rgbs": ((batch_size, 3), torch.float32),
                "ts": ((batch_size,), torch.int64), "cam_ids": ((batch_size,), torch.int64),
                "disps": ((batch_size,), torch.float32), "rays_mask": ((batch_size,), torch.float32),
                "uv_fw": ((batch_size, 2), torch.float32), "uv_bw": ((batch_size, 2), torch.float32)}
        if self.hard_sampling:
            spec["rand_idx"] = ((batch_size,), torch.int64)
        return spec

    # ---- device side ----
    def _refresh_cdf(self):
        if self._cdf is None:
            cdf = torch.empty(self.weights.shape, dtype=torch.float64, device=self.weights.device)
            _lib.cdf(self.weights, cdf)
            self._cdf = cdf
        return self._cdf

    def sample(self, batch_size, generator=None, frame=None):
        """One training batch (monocular.py:233-250): the reference's dict, + 'rand_idx' with hard sampling.  frame=None
        chooses it by the window rule; the pixels come from one draw-and-gather launch."""
        _lib.require_gpu_tensor(self.records, "RayBank.records")
        t = self.next_frame() if frame is None else int(frame)
        dev = self.records.device
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in self.batch_spec(batch_size).items()}
        u = torch.rand(batch_size, device=dev, generator=generator)
        _lib.ray_draw(self.records, t, u, self._refresh_cdf() if self.hard_sampling else None, out)
        return out

    def frame_sample(self, t):
        """Frame t as the validation split hands it to ``validation_step`` (monocular.py:252-294): {'rays' (H*W,6),
        'ts' (H*W) int64, 'rgbs' (H*W,3), 'disp' (H*W), 'mask' (H*W)}, read from the records."""
        r = self.records[int(t)]
        return {"rays": r[:, :6].contiguous(), "ts": r[:, 9].long(), "rgbs": r[:, 6:9].contiguous(),
                "disp": r[:, 10].contiguous(), "mask": r[:, 11].contiguous()}

    def frame_images(self, t):
        """``(ground truth, tmp_rgb)`` of frame t as (H, W, 3) views: the pair train.py:250-251 compares."""
        W, H = self.img_wh
        return self.rgb[int(t)].view(H, W, 3), self.tmp_rgb[int(t)].view(H, W, 3)

    @torch.no_grad()
    def record(self, batch, rgb_fine):
        """train.py:184-185: tmp_rgb[ts, rand_idx] = rgb_fine (capturable)."""
        self.tmp_rgb.index_put_((batch["ts"], batch["rand_idx"]), rgb_fine.detach().to(self.tmp_rgb.dtype))

    @torch.no_grad()
    def update_weights(self):
        """train.py:246-253 for every frame at once: weights = 1 - ssim(rgb, tmp_rgb, reduction='none').mean(-1) (= the
        channel-mean SSIM loss), one SSIM launch; then the fp64 CDF, one launch."""
        _lib.require_gpu_tensor(self.records, "RayBank.records")
        W, H = self.img_wh
        shape = (self.n_frames, H, W, 3)
        _lib.ssim(self.rgb.view(shape), self.tmp_rgb.view(shape), mean_map=self.weights)
        if self._cdf is None:
            self._cdf = torch.empty(self.weights.shape, dtype=torch.float64, device=self.weights.device)
        _lib.cdf(self.weights, self._cdf)

    def cdf(self):
        """The fp64 per-frame CDF the draws use (computed if stale)."""
        return self._refresh_cdf()

    def state_dict(self):
        return {"weights": self.weights.detach().clone(), "tmp_rgb": self.tmp_rgb.detach().clone()}

    def load_state_dict(self, state):
        with torch.no_grad():
            for k in ("weights", "tmp_rgb"):
                v = state[k]
                if tuple(v.shape) != tuple(getattr(self, k).shape):
                    raise ValueError(f"RayBank.load_state_dict: {k} has shape {tuple(v.shape)}, the bank "
                                     f"{tuple(getattr(self, k).shape)}")
                getattr(self, k).copy_(v)
        self._cdf = None
