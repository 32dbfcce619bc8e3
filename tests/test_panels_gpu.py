"""MI355X checks of nsff_val_panels (csrc/frames.hip) and the layers on it (panels.validation_panels / error_blend,
NSFFTrainer.validation_step(panels=...)) against the numpy fp32 restatement tests/panel_numpy.py (itself checked against the
reference's statements in tests/test_panels_host.py).

Shapes (F, H, W): (1, 1, 1) one pixel, grid only, ma == mi everywhere; (1, 6, 6) the smallest frame SSIM takes; (3, 19, 33) odd
H * W -- frames 1 and 2 start at flat pixels 627 and 1254, 627 = 156 quads + 3, and GW = 107 is odd, so the 3-byte grid rows land
at every byte offset; (2, 37, 71) 2627 pixels -- three workgroups, i.e. three partials, a frame; (2, 129, 511), with eight tiles
only, 65 919 pixels -- 65 workgroups a frame, the last one ragged, so lane 0 of the frame's last workgroup folds two partials
(blocks 0 and 64) before the butterfly; H * W is odd, so frame 0 takes the 16-byte path and frame 1 the element path.  Tile counts
3, 6, 7, 8; the colour tables given (6 and 8 tiles) and NULL (3 and 7)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import frame_finish_numpy as ffn
import panel_numpy as pn
import scenes
import ssim_numpy as sn
import nsff_pl_amd as A
from nsff_pl_amd import _lib, panels
from nsff_pl_amd.sampling import RayBank
from test_split_frames_gpu import case as frame_case, edge_values

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (1, 6, 6), (3, 19, 33), (2, 37, 71)]
TILES = [3, 6, 7, 8]
WRAP_SHAPE = (2, 129, 511)
MAP_TOL = 1e-4           # the project's SSIM map bar
U8_OUT = ("grid_u8", "rmse_u8", "ssim_u8", "rmse_blend_u8", "ssim_blend_u8")

_INPUTS, _WANT = {}, {}


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).to(DEV)          # (a copy: the shared cases are read-only)


def with_edges(rng, a):
    edges, flat = edge_values(), a.reshape(-1)
    where = rng.permutation(flat.size)[:min(len(edges), flat.size // 2)]
    flat[where] = edges[:len(where)]
    return a


def inputs(shape):
    """The fp32 inputs of one shape, computed once and shared (read-only): gt / pred / depth / lut_depth are
    test_split_frames_gpu.case's (edge values around k / 255 in pred; NaN, +-inf, negative and constant depths), the rest is
    seeded the same way; ssim_loss is nsff_ssim's own map of (gt, clip(pred)), read back."""
    if shape in _INPUTS:
        return _INPUTS[shape]
    F, H, W = shape
    c = frame_case(shape)
    rng = np.random.default_rng(7000 + 1000 * F + 10 * H + W)
    i = dict(gt=c["gt"], pred=c["rgb"], depth=c["depth"], lut_depth=c["lut"], lut_mask=rng.integers(0, 256, (256, 3), dtype=np.uint8))
    i["static_rgb"] = with_edges(rng, (rng.random((F, H, W, 3), dtype=np.float32) * 1.6 - 0.3).astype(np.float32))
    i["transient_alpha"] = with_edges(rng, rng.random((F, H, W), dtype=np.float32))
    i["static_depth"] = (rng.random((F, H, W)) * 5 + 0.1).astype(np.float32)
    i["static_depth"].reshape(-1)[rng.permutation(F * H * W)[:max(F * H * W // 20, 1)]] = np.nan
    i["mask"] = (rng.random((F, H, W)) < 0.3).astype(np.float32)
    i["disp"] = (rng.random((F, H, W)) * 2 + 0.1).astype(np.float32)
    i["disp"][-1] = np.float32(0.375)                                           # a constant disparity: ma == mi
    if H >= 6 and W >= 6:
        loss = torch.empty(F, H, W, 3, device=DEV)
        _lib.ssim(dev(i["gt"]), dev(np.clip(i["pred"], 0, 1)), map=loss)
        i["ssim_loss"] = loss.cpu().numpy()
    for v in i.values():
        v.setflags(write=False)
    _INPUTS[shape] = i
    return i


def selection(shape, tiles, frames=slice(None)):
    """The keyword inputs of one (shape, tile count): numpy arrays."""
    i = inputs(shape)
    names = ["pred", "gt", "depth"] + (["ssim_loss"] if "ssim_loss" in i else [])
    if tiles >= 6:
        names += ["transient_alpha", "static_rgb", "static_depth"]
    if tiles >= 7:
        names += ["mask"]
    if tiles == 8:
        names += ["disp"]
    kw = {n: i[n][frames] for n in names}
    if tiles in (6, 8):
        kw.update(lut_depth=i["lut_depth"], lut_mask=i["lut_mask"])
    return kw


def want(shape, tiles):
    if (shape, tiles) not in _WANT:
        _WANT[shape, tiles] = pn.panels(**selection(shape, tiles))
    return _WANT[shape, tiles]


def run(shape, kw, scratch=None, only=None):
    """One nsff_val_panels call with every output the inputs allow (prefilled with 0xAB: every byte must be written)."""
    F, H, W = shape
    tiles = 3 + (3 if "transient_alpha" in kw else 0) + ("mask" in kw) + ("disp" in kw)
    GH, GW = _lib.panel_grid_shape(H, W, tiles)
    shapes = dict(grid_u8=(F, GH, GW, 3), rmse_u8=(F, H, W), rmse_blend_u8=(F, H, W, 3))
    if "ssim_loss" in kw:
        shapes.update(ssim_u8=(F, H, W), ssim_blend_u8=(F, H, W, 3))
    out = {k: torch.full(s, 0xAB, dtype=torch.uint8, device=DEV) for k, s in shapes.items() if only is None or k in only}
    out["ranges"] = torch.full((F, 5, 2), float("nan"), device=DEV)
    _lib.val_panels(F, H, W, scratch=scratch, **{k: dev(v) for k, v in kw.items()}, **out)
    torch.cuda.synchronize()
    return out


def assert_equal(got, ref, label):
    for key, w in ref.items():
        g = got[key].cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (label, key)
        bad = int(((g != w) & ~(np.isnan(g) & np.isnan(w))).sum()) if key == "ranges" else int((g != w).sum())
        print(f"{label} {key}: {bad} of {g.size} values differ")
        assert bad == 0, (label, key)
    assert set(got) == set(ref), label


@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("shape", SHAPES)
def test_panels_equal_numpy_exactly(hip_lib, shape, tiles):
    """Grid, index images, blends and ranges -- the SSIM panels included: both sides consume nsff_ssim's loss map."""
    ref = want(shape, tiles)
    assert ("ssim_u8" in ref) == (shape[1] >= 6)
    assert_equal(run(shape, selection(shape, tiles)), ref, f"{shape} {tiles} tiles")
    if shape == (1, 1, 1):                                                      # ma == mi everywhere: index 0 in every colour tile
        assert not ref["rmse_u8"].any() and ref["grid_u8"].shape == (1, (tiles + 2) // 3 * 3 + 2, 11, 3)


def test_panels_equal_numpy_exactly_where_the_fold_wraps(hip_lib):
    assert_equal(run(WRAP_SHAPE, selection(WRAP_SHAPE, 8)), want(WRAP_SHAPE, 8), f"{WRAP_SHAPE} 8 tiles")


# (seeds for which the float64 reference's span is at least 0.05: a condition on the reference alone, asserted below)
@pytest.mark.parametrize("shape,seed,levels", [((1, 6, 6), 615, 2), ((1, 19, 33), 1933, 1), ((1, 37, 71), 3771, 1)])
def test_ssim_index_image_end_to_end_bound(hip_lib, shape, seed, levels):
    """ssim_u8 through validation_panels (nsff_ssim in fp32 on the device) against the restatement on ssim_numpy's float64 map:
    an index is 255 (x - mi) / (ma - mi), and x, mi and ma each carry at most MAP_TOL, so it moves by at most
    ceil(255 * 3 * MAP_TOL / span) levels."""
    F, H, W = shape
    rng = np.random.default_rng(seed)
    gt = rng.random((H, W, 3), dtype=np.float32)
    pred = np.clip(gt + 0.2 * rng.standard_normal((H, W, 3)), 0, 1).astype(np.float32)
    loss64 = sn.ssim_loss(gt.astype(np.float64), pred.astype(np.float64))
    ref_map = (1 - loss64).mean(-1)
    span = ref_map.max() - ref_map.min()
    bound = math.ceil(255 * 3 * MAP_TOL / span)
    print(f"{shape}: float64 span {span:.4f}, bound {bound} levels")
    assert span >= 0.05 and bound == levels
    ref = pn.index_image(-pn.ssim_map(loss64.astype(np.float32))[None])[0]
    res = {"rgb_fine": dev(pred).view(-1, 3), "depth_fine": torch.zeros(H * W, device=DEV)}
    got = panels.validation_panels(res, {"rgbs": dev(gt).view(-1, 3)}, (W, H), output_transient=False, want=("ssim_u8",))
    assert set(got) == {"ssim_u8", "ranges"}
    diff = np.abs(got["ssim_u8"][0].cpu().numpy().astype(int) - ref.astype(int))
    print(f"{shape}: {int((diff > 0).sum())} of {diff.size} indices differ, by at most {diff.max()}")
    assert diff.max() <= bound


@pytest.mark.parametrize("shape,tiles", [((3, 19, 33), 8), ((2, 37, 71), 7), (WRAP_SHAPE, 8)])
def test_batch_equals_single_frames(hip_lib, shape, tiles):
    batched = run(shape, selection(shape, tiles))
    for f in range(shape[0]):
        single = run((1,) + shape[1:], selection(shape, tiles, slice(f, f + 1)))
        for k, v in batched.items():
            assert torch.equal(v[f:f + 1].view(torch.uint8 if k != "ranges" else torch.int32),
                               single[k].view(torch.uint8 if k != "ranges" else torch.int32)), (f, k)


def test_scratch_is_reusable(hip_lib):
    shape, tiles = (2, 37, 71), 8
    scratch = torch.zeros(_lib.val_panels_scratch_bytes(*shape), dtype=torch.uint8, device=DEV)
    assert scratch.numel() == 16 + 2 * 3 * 40
    first = run(shape, selection(shape, tiles), scratch=scratch)
    assert not scratch[:16].any()                                               # the ticket counters are back at zero
    second = run(shape, selection(shape, tiles), scratch=scratch)
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8)), k
    assert_equal(second, want(shape, tiles), "second call")
    other = run((1, 37, 71), selection(shape, tiles, slice(1, 2)), scratch=scratch)     # ... and for another batch size
    assert torch.equal(other["grid_u8"], first["grid_u8"][1:2])


def test_unaligned_arrays_take_the_element_path(hip_lib):
    """Inputs 4 bytes and byte outputs 1 byte off a 16-byte boundary: the same bytes."""
    shape, tiles = (3, 19, 33), 8
    F, H, W = shape
    kw = selection(shape, tiles)

    def shifted(a, by=1):
        t = dev(a)
        buf = torch.empty(t.numel() + by, dtype=t.dtype, device=DEV)
        buf[by:].copy_(t.reshape(-1))
        return buf[by:].view(t.shape)
    ins = {k: (dev(v) if k.startswith("lut") else shifted(v)) for k, v in kw.items()}
    GH, GW = _lib.panel_grid_shape(H, W, tiles)
    shapes = dict(grid_u8=(F, GH, GW, 3), rmse_u8=(F, H, W), rmse_blend_u8=(F, H, W, 3), ssim_u8=(F, H, W), ssim_blend_u8=(F, H, W, 3))
    out = {k: shifted(np.full(s, 0xAB, np.uint8)) for k, s in shapes.items()}
    out["ranges"] = torch.full((F, 5, 2), float("nan"), device=DEV)
    assert ins["pred"].data_ptr() % 16 == 4 and out["rmse_u8"].data_ptr() % 4 == 1
    _lib.val_panels(F, H, W, **ins, **out)
    torch.cuda.synchronize()
    assert_equal(out, want(shape, tiles), "unaligned")


def test_golden_through_validation_panels(hip_lib):
    """g27 (the reference's statements) through the public entry: the grid and the RMSE panels byte for byte; the SSIM panels
    start from nsff_ssim's fp32 map instead of the golden's float64 one, so their indices carry the end-to-end bound."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g27_panels.npz")))
    H, W = g["gt"].shape[:2]
    span = float(g["ssim_map"].max() - g["ssim_map"].min())
    bound = math.ceil(255 * 3 * MAP_TOL / span)
    assert span >= 0.05 and bound == 1
    for i in range(4):
        tiles = int(g[f"c{i}/tiles"])
        res = {"rgb_fine": dev(g["pred"]).view(-1, 3), "depth_fine": dev(g[f"c{i}/depth"]).view(-1)}
        batch = {"rgbs": dev(g["gt"]).view(-1, 3)}
        if tiles >= 6:
            res.update({"transient_alpha_fine": dev(g["transient_alpha"]).view(-1), "_static_rgb_fine": dev(g["static_rgb"]).view(-1, 3),
                        "_static_depth_fine": dev(g[f"c{i}/static_depth"]).view(-1)})
        if tiles == 8:
            batch.update(mask=dev(g[f"c{i}/mask"]).view(-1), disp=dev(g[f"c{i}/disp"]).view(-1))
        out = panels.validation_panels(res, batch, (W, H), lut_depth=g["lut_depth"], lut_mask=dev(g["lut_mask"]),
                                       output_transient=tiles >= 6)
        assert set(out) == set(panels.TAGS)
        got = {k: v[0].cpu().numpy() for k, v in out.items()}
        for tag, key in (("reconstruction/decomposition", f"c{i}/grid_u8"), ("rmse_u8", "rmse_u8"), ("error_map/rmse", "rmse_blend_u8")):
            assert got[tag].shape == g[key].shape and np.array_equal(got[tag], g[key]), (i, tag)
        diff = np.abs(got["ssim_u8"].astype(int) - g["ssim_u8"].astype(int))
        print(f"case {i}: {int((diff > 0).sum())} of {diff.size} SSIM indices differ from the golden, by at most {diff.max()}")
        assert diff.max() <= bound
        assert np.array_equal(got["error_map/ssim"], pn.blend(ffn.rgb_u8(g["pred"]), g["lut_depth"][got["ssim_u8"]]))
        same = diff == 0
        assert np.array_equal(got["error_map/ssim"][same], g["ssim_blend_u8"][same])


def test_small_frames_refuse_the_ssim_panels_by_name(hip_lib):
    res = {"rgb_fine": torch.rand(20, 3, device=DEV), "depth_fine": torch.rand(20, device=DEV)}
    batch = {"rgbs": torch.rand(20, 3, device=DEV)}
    with pytest.raises(ValueError, match=r"error_map/ssim.*ssim_u8"):
        panels.validation_panels(res, batch, (4, 5), output_transient=False)
    rest = [t for t in panels.TAGS if t not in panels.SSIM_TAGS]
    out = panels.validation_panels(res, batch, (4, 5), output_transient=False, want=rest)
    assert set(out) == set(rest) and tuple(out["reconstruction/decomposition"].shape) == (1, 9, 20, 3)
    with pytest.raises(ValueError, match="6 x 6"):
        panels.error_blend(batch["rgbs"].view(5, 4, 3), res["rgb_fine"].view(5, 4, 3), "ssim")
    assert tuple(panels.error_blend(batch["rgbs"].view(5, 4, 3), res["rgb_fine"].view(5, 4, 3), "rmse").shape) == (1, 5, 4, 3)


def test_invalid_argument_sets_are_refused_without_a_launch(hip_lib):
    shape, tiles = (1, 6, 6), 8
    F, H, W = shape
    ins = {k: dev(v) for k, v in selection(shape, tiles).items()}
    GH, GW = _lib.panel_grid_shape(H, W, tiles)
    outs = dict(ranges=torch.full((F, 5, 2), -7.0, device=DEV), grid_u8=torch.full((F, GH, GW, 3), 0xAB, dtype=torch.uint8, device=DEV))
    outs.update({k: torch.full((F, H, W) + ((3,) if "blend" in k else ()), 0xAB, dtype=torch.uint8, device=DEV)
                 for k in ("rmse_u8", "ssim_u8", "rmse_blend_u8", "ssim_blend_u8")})
    scratch = torch.zeros(max(_lib.val_panels_scratch_bytes(F, H, W), 16), dtype=torch.uint8, device=DEV)

    def call(drop, keep_out):
        a = _lib.ValPanelsArgs(n_frames=F, H=H, W=W, scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
        for k, t in ins.items():
            if k not in drop:
                setattr(a, k, t.data_ptr())
        for k in keep_out + ["ranges"]:
            setattr(a, k, outs[k].data_ptr())
        return _lib.load().nsff_val_panels(C.byref(a), torch.cuda.current_stream().cuda_stream)
    assert call(["pred"], ["grid_u8"]) == -1                                    # grid_u8 without pred
    assert call(["ssim_loss"], ["ssim_u8"]) == -1                               # ssim_u8 without ssim_loss
    assert call(["gt"], ["rmse_u8"]) == -1 and call(["gt"], ["rmse_blend_u8"]) == -1
    assert call(["static_rgb"], ["grid_u8"]) == -1 and call(["transient_alpha", "static_depth"], ["grid_u8"]) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 0xAB).all()) for k, t in outs.items() if k != "ranges") and bool((outs["ranges"] == -7).all())
    assert not scratch.any()
    assert call([], list(U8_OUT)) == 0                                          # the full set is taken
    torch.cuda.synchronize()
    assert not any(bool((t == 0xAB).all()) for k, t in outs.items() if k != "ranges")


# ---- the trainer ----
def _bank_records(F, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    rays, _ = scenes.synthetic_rays(F * H * W, seed)
    rec = torch.cat([rays.view(F, H * W, 6), torch.rand(F, H * W, 3, generator=g),
                     torch.arange(F, dtype=torch.float32)[:, None, None].expand(F, H * W, 1),
                     torch.rand(F, H * W, 1, generator=g) * 2 + 0.1, (torch.rand(F, H * W, 1, generator=g) < 0.3).float(),
                     torch.rand(F, H * W, 4, generator=g) * 100], -1)
    return rec.contiguous()


@pytest.fixture(scope="module")
def trainer(hip_lib):
    from nsff_pl_amd.training import NSFFTrainer
    H, W = 12, 16
    bank = RayBank(_bank_records(scenes.N_FRAMES, H, W, 8), (W, H), hard_sampling=True, seed=0, device=DEV)
    g = torch.Generator(DEV).manual_seed(3)                                     # recorded predictions that leave [0, 1]
    bank.tmp_rgb.copy_(bank.rgb + 0.2 * torch.randn(bank.rgb.shape, device=DEV, generator=g))
    cfg = scenes.CASES["g3_nsff_train"]
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
    Ks, Ps, _ = scenes.camera_buffers()
    hp = dict(N_samples=32, N_importance=32, perturb=0, noise_std=0, img_wh=(W, H))
    tr = NSFFTrainer(models, emb, scenes.N_FRAMES, hp, Ks, Ps, output_transient_flow=cfg["flow"], ray_bank=bank).to(DEV)
    tr.on_train_epoch_start(scenes.LOSS_EPOCH)
    return tr, bank, bank.frame_sample(4), (H, W)


def test_trainer_panels_off_is_unchanged(trainer):
    tr, bank, vb, _ = trainer
    plain = tr.validation_step(vb)
    with_panels = tr.validation_step(vb, panels=True)
    assert "panels" not in plain and set(plain) == {"val_psnr", "val_ssim", "val_psnr_mask", "val_ssim_mask"}
    assert set(with_panels) == set(plain) | {"panels"}
    for k, v in plain.items():
        assert torch.equal(v, with_panels[k]), k
    assert set(tr.validation_step(vb, panels=False)) == set(plain)


def test_trainer_panels_equal_numpy_on_the_forward_outputs(trainer):
    tr, bank, vb, (H, W) = trainer
    rng = np.random.default_rng(5)
    luts = dict(lut_depth=torch.tensor(rng.integers(0, 256, (256, 3), dtype=np.uint8)),
                lut_mask=rng.integers(0, 256, (256, 3), dtype=np.uint8))
    log = tr.validation_step(vb, panels=luts)
    res = tr.forward(vb["rays"], vb["ts"], test_time=True, output_transient=True, output_transient_flow=[])
    frame = lambda t, *last: t.float().reshape(1, H, W, *last).contiguous()
    kw = dict(pred=frame(res["rgb_fine"], 3), gt=frame(vb["rgbs"], 3), depth=frame(res["depth_fine"]),
              transient_alpha=frame(res["transient_alpha_fine"]), static_rgb=frame(res["_static_rgb_fine"], 3),
              static_depth=frame(res["_static_depth_fine"]), mask=frame(vb["mask"]), disp=frame(vb["disp"]))
    loss = torch.empty(1, H, W, 3, device=DEV)
    _lib.ssim(kw["gt"], torch.clip(kw["pred"], 0, 1), map=loss)
    ref = pn.panels(ssim_loss=loss.cpu().numpy(), lut_depth=luts["lut_depth"].numpy(), lut_mask=luts["lut_mask"],
                    **{k: v.cpu().numpy() for k, v in kw.items()})
    got = log["panels"]
    assert set(got) == set(panels.TAGS) | {"misc/moving_ssim"} and all(v.is_cuda for v in got.values())
    names = {"reconstruction/decomposition": "grid_u8", "error_map/rmse": "rmse_blend_u8", "error_map/ssim": "ssim_blend_u8",
             "rmse_u8": "rmse_u8", "ssim_u8": "ssim_u8", "ranges": "ranges"}
    assert_equal({v: got[k] for k, v in names.items()}, ref, "trainer")
    assert tuple(got["reconstruction/decomposition"].shape) == (1, 3 * (H + 2) + 2, 3 * (W + 2) + 2, 3)
    # the bank's middle frame: the SSIM of (gt, tmp_rgb) as recorded, blended over the clipped tmp_rgb
    mid = bank.n_frames // 2
    gt_mid, tmp_mid = bank.frame_images(mid)
    moving = got["misc/moving_ssim"]
    assert torch.equal(moving, panels.error_blend(gt_mid, tmp_mid, "ssim", lut=luts["lut_depth"], clip_ssim=False))
    assert float(tmp_mid.min()) < 0 and float(tmp_mid.max()) > 1
    loss = torch.empty(1, H, W, 3, device=DEV)
    _lib.ssim(gt_mid.unsqueeze(0).contiguous(), tmp_mid.unsqueeze(0).contiguous(), map=loss)
    ref = pn.panels(pred=tmp_mid.unsqueeze(0).cpu().numpy(), ssim_loss=loss.cpu().numpy(), lut_depth=luts["lut_depth"].numpy())
    assert np.array_equal(moving.cpu().numpy(), ref["ssim_blend_u8"])
    torch.testing.assert_close(bank.weights[mid], loss.mean(-1).reshape(-1), rtol=0, atol=1e-6)   # ... after the re-weighting
