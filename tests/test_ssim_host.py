"""CPU checks of the SSIM metric and the ray bank: the float64 restatement against a direct double loop and closed forms,
the C-ABI's argument validation of nsff_ssim / nsff_cdf / nsff_ray_draw (no launch), and RayBank's host logic."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssim_numpy as sn
from nsff_pl_amd import _lib, metrics
from nsff_pl_amd.sampling import RayBank, WINDOW


@pytest.mark.parametrize("H,W,full", [(13, 9, True), (6, 6, True), (288, 512, False)])
def test_restatement_equals_direct_double_loop(H, W, full):
    rng = np.random.default_rng(H * 1000 + W)
    gt, pred = rng.random((H, W, 3)), rng.random((H, W, 3))
    want = sn.ssim_loss(gt, pred)
    if full:
        pixels = None
    else:                                   # every border pixel of the reflect padding's reach + a random interior sample
        ys = sorted(set(range(7)) | set(range(H - 7, H)) | set(rng.integers(0, H, 6).tolist()))
        xs = sorted(set(range(7)) | set(range(W - 7, W)) | set(rng.integers(0, W, 6).tolist()))
        pixels = [(y, x) for y in ys for x in (0, 3, 5, W - 1, W - 4)] + [(y, x) for y in (0, 5, H - 1) for x in xs]
    got = sn.ssim_loss_direct(gt, pred, pixels)
    for (y, x), v in got.items():
        np.testing.assert_allclose(want[y, x], v, rtol=0, atol=1e-12)


def test_closed_forms():
    rng = np.random.default_rng(1)
    img = rng.random((10, 12, 3))
    assert abs(sn.ssim(img, img) - 1) < 1e-8                          # 1 up to the 1e-12 of the denominator
    c1, c2 = 0.3, 0.7
    a, b = np.full((8, 8, 3), c1), np.full((8, 8, 3), c2)
    want = (1 + (2 * c1 * c2 + sn.C1) / (c1 ** 2 + c2 ** 2 + sn.C1)) / 2
    assert abs(sn.ssim(a, b) - want) < 1e-8
    np.testing.assert_allclose(sn.ssim(a, b, reduction="none"), want, atol=1e-8)


def negative_ssim_pair(H=12, W=12):
    """A checkerboard against its inverse: sigma12 < 0, so ssim < 0 away from nothing (every pixel)."""
    yy, xx = np.mgrid[:H, :W]
    x = ((yy + xx) % 2).astype(np.float64)[..., None].repeat(3, -1) * 0.8 + 0.1
    return x, 1 - x


def test_negative_ssim_uses_the_054_clamp_form():
    x, y = negative_ssim_pair()
    s = sn.ssim_index(x[..., 0], y[..., 0])
    assert (s < 0).all()
    loss = sn.ssim_loss(x, y)[..., 0]
    np.testing.assert_allclose(loss, (1 - s) / 2)                     # kornia 0.5.4
    assert (loss > 0.5).all()
    assert (sn.loss_form_pre_054(s) == 0.5).all()                     # the older form would give 0.5 here


def test_c_abi_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value

    def args(**kw):
        a = _lib.SsimArgs(n_frames=1, H=8, W=8, window=11, gt=p, pred=p, map=p)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.nsff_ssim(None, None) == -2
    for bad in (dict(H=5), dict(W=5), dict(n_frames=0), dict(n_frames=-3), dict(window=7), dict(map=None)):
        assert lib.nsff_ssim(C.byref(args(**bad)), None) == -1, bad
    assert lib.nsff_ssim(C.byref(args(gt=None)), None) == -2
    assert lib.nsff_ssim(C.byref(args(pred=None)), None) == -2
    assert lib.nsff_ssim(C.byref(args(map=None, sums=p)), None) == -2                 # sums need the scratch
    assert lib.nsff_ssim(C.byref(args(map=None, sums=p, scratch=p, scratch_bytes=4)), None) == -1   # too small
    assert lib.nsff_ssim(C.byref(args(map=None, sums=p, scratch=p + 4, scratch_bytes=1 << 20)), None) == -3
    assert lib.nsff_ssim_scratch_bytes(1, 5, 8) == 0 and lib.nsff_ssim_scratch_bytes(0, 8, 8) == 0
    assert lib.nsff_ssim_scratch_bytes(2, 288, 512) == 16 + 16 * 2 * 8 * 18
    assert lib.nsff_cdf(None, 1, 4, None, None) == -2 and lib.nsff_cdf(None, -1, 4, None, None) == -1
    assert lib.nsff_cdf(None, 0, 4, None, None) == 0
    d = _lib.RayDrawArgs(n_frames=2, n_pixels=64, frame=0, batch=8)
    assert lib.nsff_ray_draw(None, None) == -2 and lib.nsff_ray_draw(C.byref(d), None) == -2
    for k, v in (("frame", 2), ("frame", -1), ("n_pixels", 0), ("batch", -1)):
        bad = _lib.RayDrawArgs(n_frames=2, n_pixels=64, frame=0, batch=8)
        setattr(bad, k, v)
        assert lib.nsff_ray_draw(C.byref(bad), None) == -1, (k, v)
    assert C.sizeof(_lib.SsimArgs) == 16 + 7 * 8 + 8 and C.sizeof(_lib.RayDrawArgs) == 32 + 12 * 8


def test_metrics_refuse_cpu_tensors_and_other_windows():
    img = torch.rand(8, 8, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.ssim(img, img)
    with pytest.raises(ValueError, match="window_size"):
        metrics.ssim(img, img, window_size=7)
    with pytest.raises(ValueError, match="reduction"):
        metrics.ssim(img, img, reduction="sum")
    assert float(metrics.psnr(torch.zeros(4, 3), torch.full((4, 3), 0.1))) == pytest.approx(20.0, abs=1e-5)


def _records(n_frames, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    rec = torch.rand(n_frames, H * W, 16, generator=g)
    rec[..., 9] = torch.arange(n_frames, dtype=torch.float32)[:, None]
    return rec


def test_ray_bank_frame_window_rule():
    bank = RayBank(_records(30, 6, 8), (8, 6), seed=7)
    last, seen = None, set()
    for _ in range(10_000):
        t = bank.next_frame()
        assert 0 <= t < 30
        if last is not None:
            assert abs(t - last) > WINDOW, (last, t)
        seen.add(t)
        last = t
    assert seen == set(range(30))
    small = RayBank(_records(8, 6, 8), (8, 6), seed=1)             # the window covers every frame: all frames are allowed
    assert all(0 <= small.next_frame() < 8 for _ in range(100))
    a, b = RayBank(_records(30, 6, 8), (8, 6), seed=3), RayBank(_records(30, 6, 8), (8, 6), seed=3)
    assert [a.next_frame() for _ in range(50)] == [b.next_frame() for _ in range(50)]


def test_ray_bank_batch_keys_and_state_round_trip():
    rec = _records(4, 6, 8)
    bank = RayBank({t: rec[t] for t in range(4)}, (8, 6), hard_sampling=True)
    spec = bank.batch_spec(32)
    ref_keys = {"rays", "rgbs", "ts", "cam_ids", "disps", "rays_mask", "uv_fw", "uv_bw"}   # monocular.py:240-247
    assert set(spec) == ref_keys | {"rand_idx"}
    assert set(RayBank(rec, (8, 6)).batch_spec(32)) == ref_keys
    assert spec["rays"] == ((32, 6), torch.float32) and spec["ts"][1] == spec["rand_idx"][1] == torch.int64
    assert bank.weights.shape == (4, 48) and bool((bank.weights == 1).all())
    assert bank.tmp_rgb.shape == (4, 48, 3) and not bool(bank.tmp_rgb.any())
    bank.weights.uniform_()
    bank.tmp_rgb.uniform_()
    state = bank.state_dict()
    other = RayBank(rec, (8, 6), hard_sampling=True)
    other.load_state_dict(state)
    assert torch.equal(other.weights, bank.weights) and torch.equal(other.tmp_rgb, bank.tmp_rgb)
    bank.weights.zero_()                                              # the state is a copy
    assert torch.equal(state["weights"], other.weights)
    with pytest.raises(ValueError):
        RayBank(rec, (8, 7))
    with pytest.raises(RuntimeError, match="GPU"):
        bank.sample(4)


def test_validation_hparam_defaults_to_none():
    from nsff_pl_amd.training import NSFFTrainer
    assert NSFFTrainer.DEFAULTS["img_wh"] is None
