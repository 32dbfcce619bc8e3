"""MI355X checks of the ray-bank builder (nsff_ray_records behind frames.build_records / RayBank.from_frames) on golden g24:
the reference's own records of a 3-frame 19 x 33 scene (tests/golden/make_golden_records.py).  Ray columns at the 1e-5 bar of
test_frame_rays_match_reference (the same arithmetic) and bit-equal to evaluate.frame_rays; every other column exact."""
import os

import numpy as np
import pytest
import torch

import parity
import records_ref
import scenes
import nsff_pl_amd as A
from nsff_pl_amd import evaluate, frames
from nsff_pl_amd.sampling import RayBank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
RAY_TOL = 1e-5
F, H, W = 3, 19, 33
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g24():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g24_ray_records.npz")))


@pytest.fixture(scope="module")
def inputs(g24):
    return {k: torch.from_numpy(g24[k]).to(DEV) for k in ("images", "disps", "masks", "flows_fw", "flows_bw")}


@pytest.fixture(scope="module")
def built(g24, inputs, hip_lib):
    """The golden scene's records from uint8 images and masks, computed once (tests read it, none writes it)."""
    return frames.build_records(g24["K"], g24["poses"], **inputs)


def _check_against_golden(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    for t in range(want.shape[0]):
        err = parity.assert_close(f"frame {t} ndc rays", got[t, :, :6], want[t, :, :6], RAY_TOL)
        print(f"frame {t}: ray columns max-norm rel err {err:.2e}")
    for name, cols in (("rgb", slice(6, 9)), ("t", 9), ("disp", 10), ("mask", 11), ("uv_fw", slice(12, 14)),
                       ("uv_bw", slice(14, 16))):
        assert np.array_equal(got[..., cols], want[..., cols]), name


def test_uint8_inputs_match_the_golden(g24, built):
    assert tuple(built.shape) == (F, H * W, 16) and built.device.type == "cuda"
    _check_against_golden(built, g24["records"])


def test_float_inputs_and_lists_give_the_same_bits(g24, inputs, built):
    as_float = dict(inputs, images=(inputs["images"].cpu().float() / 255).to(DEV),
                    masks=(inputs["masks"].cpu().float() / 255).to(DEV))
    assert torch.equal(frames.build_records(g24["K"], g24["poses"], **as_float), built)
    mixed = dict(inputs, masks=as_float["masks"])                                          # uint8 images with fp32 masks
    assert torch.equal(frames.build_records(g24["K"], g24["poses"], **mixed), built)
    lists = {k: list(v) for k, v in inputs.items()}
    lists["flows_fw"][F - 1] = None                                                        # the flow a frame does not have
    lists["flows_bw"][0] = None
    assert torch.equal(frames.build_records(torch.tensor(g24["K"]), torch.tensor(g24["poses"]), **lists), built)
    for name in ("images", "disps", "masks"):                                              # ... only a flow may be missing
        holed = dict(lists, **{name: [None] + lists[name][1:]})
        with pytest.raises(TypeError, match=name):
            frames.build_records(g24["K"], g24["poses"], **holed)


def test_ray_columns_are_frame_rays_bit_for_bit(g24, built):
    for t in range(F):
        rays = evaluate.frame_rays(g24["K"], g24["poses"][t], H, W, device=DEV)
        assert torch.equal(built[t, :, :6], rays), t


def test_missing_flows_leave_uv(g24, inputs, built):
    uv = torch.from_numpy(records_ref.uv_grid(H, W)).to(DEV)
    assert float(inputs["flows_fw"][F - 1].abs().min()) > 0 and float(inputs["flows_bw"][0].abs().min()) > 0
    assert torch.equal(built[F - 1, :, 12:14], uv) and torch.equal(built[0, :, 14:16], uv)
    assert not torch.equal(built[0, :, 12:14], uv) and not torch.equal(built[F - 1, :, 14:16], uv)
    none = frames.build_records(g24["K"], g24["poses"], inputs["images"], inputs["disps"], inputs["masks"])
    assert torch.equal(none[..., 12:14], uv.expand(F, -1, -1)) and torch.equal(none[..., 14:16], uv.expand(F, -1, -1))
    assert torch.equal(none[..., :12], built[..., :12])
    only_bw = frames.build_records(g24["K"], g24["poses"], inputs["images"], inputs["disps"], inputs["masks"],
                                   flows_bw=inputs["flows_bw"])
    assert torch.equal(only_bw[..., 12:14], uv.expand(F, -1, -1)) and torch.equal(only_bw[..., 14:16], built[..., 14:16])


@pytest.mark.parametrize("first,count", [(0, 1), (1, 1), (1, 2), (2, 1), (0, 3), (1, 0), (3, 0)])
def test_frame_ranges_write_their_slice_only(g24, inputs, built, first, count):
    out = torch.full((F, H * W, 16), -7.0, device=DEV)
    got = frames.build_records(g24["K"], g24["poses"], out=out, first_frame=first, n_frames=count, **inputs)
    assert got is out
    assert torch.equal(out[first:first + count], built[first:first + count])
    rest = torch.cat([out[:first], out[first + count:]])
    assert bool((rest == -7.0).all())


def test_bad_ranges_and_outputs_are_refused(g24, inputs):
    for kw in (dict(first_frame=1, n_frames=3), dict(first_frame=-1), dict(n_frames=-1), dict(first_frame=4)):
        with pytest.raises(RuntimeError, match="NSFF_ERR_INVALID"):
            frames.build_records(g24["K"], g24["poses"], **kw, **inputs)
    with pytest.raises(ValueError, match="out must be"):
        frames.build_records(g24["K"], g24["poses"], out=torch.empty(F, H * W + 1, 16, device=DEV), **inputs)
    with pytest.raises(RuntimeError, match="uint8 or float32"):
        frames.build_records(g24["K"], g24["poses"], **dict(inputs, images=inputs["images"].to(torch.int32)))
    with pytest.raises(RuntimeError, match="GPU"):
        frames.build_records(g24["K"], g24["poses"], **dict(inputs, disps=inputs["disps"].cpu()))


def test_bank_from_frames_samples_the_golden(g24, inputs, built):
    bank = RayBank.from_frames(g24["K"], g24["poses"], inputs["images"], inputs["disps"], inputs["masks"], inputs["flows_fw"],
                               inputs["flows_bw"], (W, H), seed=0)
    assert torch.equal(bank.records, built) and not bank.hard_sampling
    assert bank.Ks.device == bank.Ps.device == bank.records.device
    assert parity.max_rel_err(bank.Ps.cpu().numpy(), g24["Ps"]) <= 1e-6
    assert np.array_equal(bank.Ks.cpu().numpy()[0], g24["K"].astype(np.float32))
    batch = bank.sample(64, generator=torch.Generator(DEV).manual_seed(3), frame=1)
    u = torch.rand(64, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    idx = (u.double() * (H * W)).floor().long().clamp(max=H * W - 1).cpu().numpy()
    # ... the same pixels as uv_fw - flow_fw names them (exact where the fp32 sum was: compare rounded)
    flow = g24["flows_fw"][1].reshape(-1, 2)[idx]
    uv = np.rint(batch["uv_fw"].cpu().numpy().astype(np.float64) - flow)
    assert np.array_equal(uv[:, 1] * W + uv[:, 0], idx)
    want = g24["records"][1, idx]
    got = {k: v.cpu().numpy() for k, v in batch.items()}
    parity.assert_close("sampled ndc rays", got["rays"], want[:, :6], RAY_TOL)
    assert np.array_equal(got["rays"], built[1].cpu().numpy()[idx, :6])
    assert np.array_equal(got["rgbs"], want[:, 6:9]) and np.array_equal(got["ts"], np.ones(64, np.int64))
    assert np.array_equal(got["disps"], want[:, 10]) and np.array_equal(got["rays_mask"], want[:, 11])
    assert np.array_equal(got["uv_fw"], want[:, 12:14]) and np.array_equal(got["uv_bw"], want[:, 14:16])
    # to() carries the projection matrices
    assert bank.to("cpu").Ps.device.type == "cpu" and bank.Ks.device.type == "cpu"


def test_frame_sample_is_the_golden_frame(g24, inputs, built):
    bank = RayBank.from_frames(g24["K"], g24["poses"], inputs["images"], inputs["disps"], inputs["masks"], None, None, (W, H))
    s, want = bank.frame_sample(2), g24["records"][2]
    assert set(s) == {"rays", "ts", "rgbs", "disp", "mask"} and all(v.is_cuda and v.is_contiguous() for v in s.values())
    assert s["ts"].dtype == torch.int64 and bool((s["ts"] == 2).all()) and tuple(s["ts"].shape) == (H * W,)
    assert torch.equal(s["rays"], evaluate.frame_rays(g24["K"], g24["poses"][2], H, W, device=DEV))
    parity.assert_close("frame 2 ndc rays", s["rays"].cpu().numpy(), want[:, :6], RAY_TOL)
    assert np.array_equal(s["rgbs"].cpu().numpy(), want[:, 6:9]) and np.array_equal(s["disp"].cpu().numpy(), want[:, 10])
    assert np.array_equal(s["mask"].cpu().numpy(), want[:, 11])


def _camera_path(n):
    """n small-motion poses in the reference's convention (right-up-back), looking down -z."""
    rng = np.random.default_rng(7)
    poses = np.zeros((n, 3, 4))
    for t in range(n):
        a = rng.uniform(-0.05, 0.05)
        poses[t, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        poses[t, :, 3] = rng.uniform(-0.1, 0.1, 3)
    return poses


def test_one_training_step_on_a_bank_built_from_frames(hip_lib):
    """The whole set-up the builder exists for: frames -> bank -> NSFFTrainer(Ks=bank.Ks, Ps=bank.Ps, ray_bank=bank) -> step."""
    from nsff_pl_amd.training import NSFFTrainer
    n, h, w = scenes.N_FRAMES, 12, 16
    g = torch.Generator(DEV).manual_seed(11)
    K = np.array([[20.0, 0, w / 2], [0, 20.0, h / 2], [0, 0, 1]])
    bank = RayBank.from_frames(K, _camera_path(n),
                               torch.randint(0, 256, (n, h, w, 3), device=DEV, generator=g, dtype=torch.uint8),
                               torch.rand(n, h, w, device=DEV, generator=g) * 2 + 0.1,
                               (torch.rand(n, h, w, device=DEV, generator=g) < 0.3).to(torch.uint8) * 255,
                               torch.randn(n, h, w, 2, device=DEV, generator=g), torch.randn(n, h, w, 2, device=DEV, generator=g),
                               (w, h), seed=0)
    assert tuple(bank.Ps.shape) == (1, n, 3, 4)
    cfg = scenes.CASES["g3_nsff_train"]
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
    hp = dict(N_samples=32, N_importance=32, perturb=0, noise_std=0, img_wh=(w, h))
    tr = NSFFTrainer(models, emb, n, hp, Ks=bank.Ks, Ps=bank.Ps, output_transient_flow=cfg["flow"], ray_bank=bank).to(DEV)
    tr.on_train_epoch_start(scenes.LOSS_EPOCH)
    batch = bank.sample(64, generator=g, frame=7)
    assert bool((batch["rays_mask"].unique().cpu() == torch.tensor([0.0, 1.0])).all())
    log = tr.step(batch)
    torch.cuda.synchronize()
    terms = {k: float(v) for k, v in log.items() if k.startswith("train/")}
    assert {"train/col_l", "train/disp_l", "train/flow_fw_l", "train/flow_bw_l", "train/loss"} <= set(terms), sorted(terms)
    assert all(np.isfinite(v) for v in terms.values()), terms
    # ... and the bank's full-frame sample is what validation_step takes
    val = tr.validation_step(bank.frame_sample(n // 2))
    assert {"val_psnr", "val_ssim", "val_psnr_mask", "val_ssim_mask"} <= set(val), sorted(val)
    assert all(np.isfinite(float(v)) for v in val.values()), val
