"""MI355X checks of the SSIM kernel (nsff_ssim) against the float64 restatement of tests/ssim_numpy.py, of the fp64 CDF and
the draw-and-gather launch of the ray bank, and of the trainer's hard-sampling path (train.py:140-143, 184-185, 200-253)."""
import numpy as np
import pytest
import torch

import scenes
import ssim_numpy as sn
import nsff_pl_amd as A
from nsff_pl_amd import _lib, metrics, evaluate
from nsff_pl_amd.sampling import RayBank

DEV = torch.device("cuda:0")
MAP_TOL, MEAN_TOL = 1e-4, 1e-5
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.asarray(a, np.float32)).to(DEV)


def _check_pair(gt, pred, mask=None):
    """Every reduction of metrics.ssim against the restatement."""
    g, p = _dev(gt), _dev(pred)
    want_map = sn.ssim(gt, pred, reduction="none")
    got_map = metrics.ssim(g, p, reduction="none").cpu().numpy()
    assert np.abs(got_map - want_map).max() <= MAP_TOL
    assert abs(float(metrics.ssim(g, p)) - sn.ssim(gt, pred)) <= MEAN_TOL
    assert abs(float(evaluate.ssim(p, g)) - sn.ssim(gt, pred)) <= MEAN_TOL
    if mask is not None:
        m = torch.as_tensor(mask).to(DEV)
        assert abs(float(metrics.ssim(g, p, m)) - sn.ssim(gt, pred, mask)) <= MEAN_TOL
        got = metrics.ssim(g, p, m, reduction="none").cpu().numpy()
        assert got.shape == (int(mask.sum()), 3)
        assert np.abs(got - sn.ssim(gt, pred, mask, reduction="none")).max() <= MAP_TOL


@pytest.mark.parametrize("H,W", [(48, 64), (23, 37), (6, 6), (288, 512)])
def test_ssim_random_images(hip_lib, H, W):
    rng = np.random.default_rng(H + W)
    gt = rng.random((H, W, 3))
    pred = np.clip(gt + rng.normal(0, 0.1, gt.shape), 0, 1)
    _check_pair(gt, pred, rng.random((H, W)) < 0.4)
    _check_pair(gt, rng.random((H, W, 3)))


def test_ssim_near_flat_images(hip_lib):
    """Constant plus 1e-3 noise: the variance terms are differences of nearly equal numbers."""
    rng = np.random.default_rng(5)
    for c in (0.5, 0.9):
        gt = c + 1e-3 * rng.standard_normal((64, 80, 3))
        pred = c + 1e-3 * rng.standard_normal((64, 80, 3))
        _check_pair(gt, pred, rng.random((64, 80)) < 0.5)


def test_ssim_rendered_frame(hip_lib):
    cfg = dict(scenes.CASES["g4_nsff_test"])
    H, W = 24, 40
    rays, ts = scenes.synthetic_rays(H * W, 3)
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
    for m in list(models.values()) + [emb["t"]]:
        m.to(DEV)
    with torch.no_grad():
        res = A.render_rays(models, emb, rays.to(DEV), ts.to(DEV), scenes.N_FRAMES - 1, cfg["N_samples"], 0, 0,
                            cfg["N_importance"], 1024 * 32, test_time=True, **scenes.render_kwargs(cfg))
    pred = res["rgb_fine"].view(H, W, 3).clamp(0, 1).cpu().numpy().astype(np.float64)
    gt = np.clip(pred + np.random.default_rng(0).normal(0, 0.05, pred.shape), 0, 1)
    _check_pair(gt, pred, (np.arange(H * W) % 3 == 0).reshape(H, W))


def test_ssim_closed_forms_on_the_gpu(hip_lib):
    rng = np.random.default_rng(2)
    img = _dev(0.2 + 0.8 * rng.random((30, 20, 3)))
    assert float(metrics.ssim(img, img)) == 1.0
    assert bool((metrics.ssim(img, img, reduction="none") == 1).all())
    c1, c2 = 0.3, 0.7
    want = (1 + (2 * c1 * c2 + sn.C1) / (c1 ** 2 + c2 ** 2 + sn.C1)) / 2
    got = metrics.ssim(_dev(np.full((9, 11, 3), c1)), _dev(np.full((9, 11, 3), c2)), reduction="none").cpu().numpy()
    assert np.abs(got - want).max() <= 1e-6
    # negative SSIM: kornia 0.5.4's clamp((1 - ssim) / 2, 0, 1), not the older clamp(1 - ssim, 0, 1) / 2
    yy, xx = np.mgrid[:12, :14]
    x = ((yy + xx) % 2).astype(np.float64)[..., None].repeat(3, -1) * 0.8 + 0.1
    loss = 1 - metrics.ssim(_dev(x), _dev(1 - x), reduction="none").cpu().numpy()
    s = sn.ssim_index(x[..., 0], 1 - x[..., 0])
    assert (s < 0).all() and (loss > 0.5).all()
    assert np.abs(loss[..., 0] - (1 - s) / 2).max() <= MAP_TOL


def _frames(F, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(F, H, W, 3, generator=g)
    pred = (gt + 0.1 * torch.randn(F, H, W, 3, generator=g)).clamp(0, 1)
    return gt.to(DEV), pred.to(DEV), (torch.rand(F, H, W, generator=g) < 0.3).to(DEV)


def test_batched_launch_is_bitwise_the_single_frame_launches(hip_lib):
    F, H, W = 24, 45, 70
    gt, pred, mask = _frames(F, H, W, 11)

    def run(g, p, m):
        n = g.shape[0]
        loss, mean, sums = torch.empty_like(g), torch.empty(n, H * W, device=DEV), torch.empty(n, 3, dtype=torch.float64, device=DEV)
        _lib.ssim(g, p, mask=m.reshape(n, H * W).contiguous(), map=loss, mean_map=mean, sums=sums)
        return loss, mean, sums
    batched = run(gt, pred, mask)
    again = run(gt, pred, mask)
    for a, b in zip(batched, again):
        assert torch.equal(a, b)
    for f in range(F):
        single = run(gt[f:f + 1], pred[f:f + 1], mask[f:f + 1])
        for a, b in zip(batched, single):
            assert torch.equal(a[f:f + 1], b), f
    # the reductions are those of the map
    loss, mean, sums = batched
    np.testing.assert_allclose(sums[:, 0].cpu().numpy(), loss.double().sum((1, 2, 3)).cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(sums[:, 2].cpu().numpy(), mask.sum((1, 2)).double().cpu().numpy(), rtol=0)
    torch.testing.assert_close(mean, loss.mean(-1).reshape(F, H * W), rtol=0, atol=1e-7)
    smap, frame, frame_mask = metrics.ssim_maps(gt, pred, mask)
    for f in (0, 13):
        want = sn.ssim(gt[f].cpu().numpy(), pred[f].cpu().numpy(), mask[f].cpu().numpy())
        assert abs(float(frame_mask[f]) - want) <= MEAN_TOL
        assert abs(float(frame[f]) - float(metrics.ssim(gt[f], pred[f]))) <= 1e-6


def _bank_records(F, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    rays, _ = scenes.synthetic_rays(F * H * W, seed)
    rec = torch.cat([rays.view(F, H * W, 6), torch.rand(F, H * W, 3, generator=g),
                     torch.arange(F, dtype=torch.float32)[:, None, None].expand(F, H * W, 1),
                     torch.rand(F, H * W, 1, generator=g) * 2 + 0.1, (torch.rand(F, H * W, 1, generator=g) < 0.3).float(),
                     torch.rand(F, H * W, 4, generator=g) * 100], -1)
    return rec.contiguous()


def test_update_weights_is_the_reference_weight_map_and_cdf_is_fp64_cumsum(hip_lib):
    F, H, W = 5, 36, 50
    bank = RayBank(_bank_records(F, H, W), (W, H), hard_sampling=True, device=DEV)
    bank.tmp_rgb.copy_((bank.rgb + 0.2 * torch.randn(bank.rgb.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))).clamp(0, 1))
    bank.update_weights()
    for f in range(F):
        want = 1 - metrics.ssim(bank.rgb[f].view(H, W, 3), bank.tmp_rgb[f].view(H, W, 3), reduction="none").mean(-1)
        torch.testing.assert_close(bank.weights[f], want.reshape(-1), rtol=0, atol=1e-6)
    np.testing.assert_allclose(bank.cdf().cpu().numpy(), np.cumsum(bank.weights.double().cpu().numpy(), 1), rtol=1e-13)
    # fp32 multiples of 2^-24 sum exactly in fp64 whatever the order: the scan must be exactly numpy's
    for n in (147456, 4097, 1):
        w = torch.rand(3, n, device=DEV, generator=torch.Generator(DEV).manual_seed(n))
        out = torch.empty(3, n, dtype=torch.float64, device=DEV)
        _lib.cdf(w, out)
        assert np.array_equal(out.cpu().numpy(), np.cumsum(w.double().cpu().numpy(), 1))


def test_draws_follow_the_weights(hip_lib):
    F, H, W = 3, 16, 24
    N = H * W
    bank = RayBank(_bank_records(F, H, W), (W, H), hard_sampling=True, device=DEV)
    w = torch.zeros(F, N)
    w[0] = (torch.arange(N) % 7).float()                            # a known map, one pixel in 7 with weight 0
    w[1] = 0                                                          # all-zero frame: uniform
    w[2] = 1.0
    w[2, N // 2:] = 0
    bank.weights.copy_(w)
    bank.load_state_dict(bank.state_dict())                           # (CDF rebuilt from the new weights)
    n_draw = 1_000_000
    gen = torch.Generator(DEV).manual_seed(123)
    for f in range(F):
        batch = bank.sample(n_draw, generator=gen, frame=f)
        idx = batch["rand_idx"]
        assert int(idx.min()) >= 0 and int(idx.max()) < N
        counts = torch.bincount(idx, minlength=N).double().cpu().numpy()
        p = w[f].double().numpy()
        p = np.full(N, 1.0 / N) if p.sum() == 0 else p / p.sum()
        assert counts[p == 0].sum() == 0                              # a zero-weight pixel is never drawn
        exp = p * n_draw
        nz = exp > 0
        chi2 = float((((counts - exp) ** 2)[nz] / exp[nz]).sum())
        df = int(nz.sum()) - 1
        z = 3.09                                                      # p = 0.001, Wilson-Hilferty
        assert chi2 < df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3, (f, chi2, df)


def test_gathered_batches_are_the_records(hip_lib):
    F, H, W = 4, 12, 20
    rec = _bank_records(F, H, W, 3)
    for hard in (True, False):
        bank = RayBank(rec, (W, H), hard_sampling=hard, device=DEV)
        if hard:
            bank.weights.copy_(torch.rand(F, H * W, device=DEV))
            bank.load_state_dict(bank.state_dict())
        batch = bank.sample(777, generator=torch.Generator(DEV).manual_seed(9), frame=2)
        if hard:
            idx = batch["rand_idx"]
        else:
            assert "rand_idx" not in batch
            u = torch.rand(777, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
            idx = (u.double() * (H * W)).floor().long().clamp(max=H * W - 1)
        r = bank.records[2, idx]
        assert torch.equal(batch["rays"], r[:, :6]) and torch.equal(batch["rgbs"], r[:, 6:9])
        assert torch.equal(batch["ts"], r[:, 9].long()) and batch["ts"].dtype == torch.int64
        assert torch.equal(batch["cam_ids"], torch.zeros_like(batch["ts"]))
        assert torch.equal(batch["disps"], r[:, 10]) and torch.equal(batch["rays_mask"], r[:, 11])
        assert torch.equal(batch["uv_fw"], r[:, 12:14]) and torch.equal(batch["uv_bw"], r[:, 14:16])


def test_hard_sampling_finds_the_bad_half(hip_lib):
    F, H, W = 2, 48, 64
    bank = RayBank(_bank_records(F, H, W, 5), (W, H), hard_sampling=True, device=DEV)
    pred = bank.rgb.clone().view(F, H, W, 3)
    noise = 0.3 * torch.randn(F, H, W // 2, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    pred[:, :, W // 2:] = (pred[:, :, W // 2:] + noise).clamp(0, 1)
    bank.tmp_rgb.copy_(pred.view(F, H * W, 3))
    bank.update_weights()
    idx = bank.sample(200_000, generator=torch.Generator(DEV).manual_seed(0), frame=1)["rand_idx"]
    right = float(((idx % W) >= W // 2).double().mean())
    assert right >= 0.9, right


def _trainer(bank, graph, img_wh, lr=5e-4):
    from nsff_pl_amd.training import NSFFTrainer
    cfg = scenes.CASES["g3_nsff_train"]
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
    Ks, Ps, _ = scenes.camera_buffers()
    hp = dict(N_samples=32, N_importance=32, perturb=0, noise_std=0, img_wh=img_wh, lr=lr)
    tr = NSFFTrainer(models, emb, scenes.N_FRAMES, hp, Ks, Ps, output_transient_flow=cfg["flow"], graph=graph,
                     ray_bank=bank).to(DEV)
    tr.on_train_epoch_start(scenes.LOSS_EPOCH)
    return tr


def test_trainer_hard_sampling(hip_lib):
    H, W = 12, 16
    rec = _bank_records(scenes.N_FRAMES, H, W, 8)
    A.set_precision("f16x3")
    try:
        bank = RayBank(rec, (W, H), hard_sampling=True, seed=0, device=DEV)
        tr = _trainer(bank, False, (W, H))
        seen, record = [], bank.record

        def spy(batch, rgb_fine):
            seen.append(rgb_fine.detach().clone())
            record(batch, rgb_fine)
        bank.record = spy
        gen = torch.Generator(DEV).manual_seed(77)
        batches = []
        for _ in range(3):
            batch = bank.sample(64, generator=gen)
            batches.append({k: v.clone() for k, v in batch.items()})
            tr.step(batch)
            idx, ts = batch["rand_idx"], batch["ts"]
            _, inv, cnt = torch.unique(idx, return_inverse=True, return_counts=True)
            once = cnt[inv] == 1
            assert torch.equal(bank.tmp_rgb[ts[once], idx[once]], seen[-1][once])
        assert len(seen) == 3
        # validation with img_wh: val_ssim (+ the masked pair), and the weights are recomputed
        t = 4
        vb = {"rays": bank.records[t, :, :6].contiguous(), "rgbs": bank.records[t, :, 6:9].contiguous(),
              "ts": torch.full((H * W,), t, dtype=torch.long, device=DEV), "mask": bank.records[t, :, 11].contiguous()}
        before = bank.weights.clone()
        log = tr.validation_step(vb)
        assert set(log) == {"val_psnr", "val_ssim", "val_psnr_mask", "val_ssim_mask"}
        assert 0 < float(log["val_ssim"]) <= 1 and np.isfinite(float(log["val_psnr_mask"]))
        assert not torch.equal(before, bank.weights)
        want = 1 - metrics.ssim(bank.rgb[0].view(H, W, 3), bank.tmp_rgb[0].view(H, W, 3), reduction="none").mean(-1)
        torch.testing.assert_close(bank.weights[0], want.reshape(-1), rtol=0, atol=1e-6)
        # checkpoint -> fresh trainer -> load_checkpoint restores the bank
        ckpt = tr.checkpoint()
        assert set(ckpt["ray_bank"]) == {"weights", "tmp_rgb"}
        fresh_bank = RayBank(rec, (W, H), hard_sampling=True, device=DEV)
        fresh = _trainer(fresh_bank, False, (W, H))
        fresh.load_checkpoint(ckpt)
        assert torch.equal(fresh_bank.weights, bank.weights) and torch.equal(fresh_bank.tmp_rgb, bank.tmp_rgb)
        assert torch.equal(fresh_bank.cdf(), bank.cdf())
        # the same draws through the captured step record the same tmp_rgb (lr = 0: both runs render with the same weights
        # at every step -- with lr > 0 eager and replayed runs drift apart in their digits, as any two training runs do)
        gbank = RayBank(rec, (W, H), hard_sampling=True, device=DEV)
        tg = _trainer(gbank, True, (W, H), lr=0.0)
        eager_bank = RayBank(rec, (W, H), hard_sampling=True, device=DEV)
        te = _trainer(eager_bank, False, (W, H), lr=0.0)
        for b in batches:
            tg.step({k: v.clone() for k, v in b.items()})
            te.step({k: v.clone() for k, v in b.items()})
        torch.cuda.synchronize()
        written = eager_bank.tmp_rgb.abs().sum(-1) > 0
        assert torch.equal(written, gbank.tmp_rgb.abs().sum(-1) > 0)
        torch.testing.assert_close(gbank.tmp_rgb, eager_bank.tmp_rgb, rtol=0, atol=1e-5)
        # without img_wh (and without a bank) validation reports what it always did
        plain = _trainer(None, False, None)
        assert set(plain.validation_step(vb)) == {"val_psnr"}
        assert "ray_bank" not in plain.checkpoint()
    finally:
        A.set_precision(A.config.DEFAULT_PRECISION)
