"""MI355X checks of nsff_frame_finish (csrc/frames.hip) against the numpy fp32 restatement tests/frame_finish_numpy.py (itself
checked against the reference's statements in tests/test_eval_split_host.py), and of the split layer on top of it
(evaluate.render_split / SequenceScores / evaluate_split) against the existing render path.

Shapes (F, H, W): (1, 1, 1) one pixel; (3, 19, 33) odd H * W with F > 1 -- frames 1 and 2 start at flat pixels 627 and 1254,
neither a multiple of four, and 627 = 156 quads + 3; (2, 37, 71) 2627 pixels -- three workgroups, i.e. three partials, a frame;
(1, 6, 6) the smallest frame SSIM takes; (2, 129, 511) 65 919 pixels -- 65 workgroups a frame, the last one ragged, so lane 0 of the
frame's last workgroup folds two partials (blocks 0 and 64) before the butterfly and every other lane one; H * W is odd, so frame 0
takes the 16-byte path and frame 1 the element path."""
import numpy as np
import pytest
import torch

import frame_finish_numpy as ffn
import scenes
import nsff_pl_amd as A
from nsff_pl_amd import _lib, evaluate, metrics

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 19, 33), (2, 37, 71), (1, 6, 6), (2, 129, 511)]
DEPTH_KINDS = {(1, 1, 1): ["plain"], (3, 19, 33): ["nan", "posinf", "negative"], (2, 37, 71): ["constant", "neginf"],
               (1, 6, 6): ["nan_posinf"], (2, 129, 511): ["negative", "nan"]}
# relative: both sides add the same fp32 squares in float64, the reference with math.fsum (correctly rounded).  Any order of n
# non-negative terms is within (n - 1) * 2^-53 < 9e-13 for n <= 7881 terms; at (2, 129, 511) a term passes through at most 29
# additions on the device (12 in its lane, 6 + 3 in its workgroup, 2 + 6 in the frame's last workgroup): 29 * 2^-53 < 4e-15
SUM_TOL = 1e-12
PSNR_TOL = 1e-4          # the project's relative bar


def edge_values():
    """0, 1 and k / 255 with its two fp32 neighbours: where (255 * x) truncated changes its value."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.concatenate([[0.0, 1.0, -0.0], k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1))]).astype(np.float32)


_CASES = {}


def case(shape):
    """Inputs and the numpy results of one shape, computed once and shared (read-only)."""
    if shape in _CASES:
        return _CASES[shape]
    F, H, W = shape
    rng = np.random.default_rng(1000 * F + 10 * H + W)
    gt = rng.random((F, H, W, 3), dtype=np.float32)
    rgb = (rng.random((F, H, W, 3), dtype=np.float32) * 1.6 - 0.3).astype(np.float32)       # below 0 and above 1
    edges = edge_values()
    flat = rgb.reshape(-1)
    where = rng.permutation(flat.size)[:min(len(edges), flat.size // 2)]
    flat[where] = edges[:len(where)]
    valid = rng.random((F, H, W)) < 0.6
    depth = (rng.random((F, H, W)) * 3 + 0.2).astype(np.float32)
    for f, kind in enumerate(DEPTH_KINDS[shape]):
        d = depth[f].reshape(-1)
        some = rng.permutation(d.size)[:max(d.size // 20, 1)]
        if kind in ("nan", "nan_posinf"):
            d[some] = np.nan
        if kind in ("posinf", "nan_posinf"):
            d[rng.permutation(d.size)[:2]] = np.inf
        if kind == "neginf":
            d[some] = -np.inf
        if kind == "negative":
            d *= -1
        if kind == "constant":
            d[:] = np.float32(2.5)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    idx = ffn.depth_u8(depth)
    c = dict(gt=gt, rgb=rgb, valid=valid, depth=depth, lut=lut, rgb_u8=ffn.rgb_u8(rgb), rgb_clipped=np.clip(rgb, 0, 1),
             depth_u8=idx, depth_rgb_u8=lut[idx], depth_range=ffn.depth_range(depth), sums=ffn.error_sums(gt, rgb, valid))
    for v in c.values():
        v.setflags(write=False)
    _CASES[shape] = c
    return c


def dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)                 # (a copy: the shared cases are read-only)


def finish(c, frames=slice(None), **kw):
    out = metrics.finish_frames(dev(c["rgb"][frames]), gt=dev(c["gt"][frames]), valid_mask=dev(c["valid"][frames]),
                                depth=dev(c["depth"][frames]), lut=dev(c["lut"]), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_eight_bit_outputs_equal_numpy_exactly(hip_lib, shape):
    c = case(shape)
    out = finish(c)
    for key in ("rgb_u8", "depth_u8", "depth_rgb_u8", "rgb_clipped", "depth_range"):
        got = out[key].cpu().numpy()
        assert got.shape == c[key].shape and got.dtype == c[key].dtype, key
        bad = int((got != c[key]).sum())
        print(f"{shape} {key}: {bad} of {got.size} values differ")
        assert bad == 0, key
    if "constant" in DEPTH_KINDS[shape]:
        assert not c["depth_u8"][DEPTH_KINDS[shape].index("constant")].any()                 # ma == mi: all zeros


@pytest.mark.parametrize("shape", SHAPES)
def test_error_sums_match_float64(hip_lib, shape):
    c = case(shape)
    got = finish(c)["sums"].cpu().numpy()
    want = c["sums"]
    rel = np.abs(got[:, :2] - want[:, :2]) / np.maximum(np.abs(want[:, :2]), 1e-300)
    print(f"{shape}: sums max relative error {rel.max():.2e}")
    assert rel.max() <= SUM_TOL
    assert np.array_equal(got[:, 2], want[:, 2])                                              # the pixel count is exact
    p, pv = metrics.psnr_frames(dev(c["gt"]), dev(c["rgb"]), dev(c["valid"]))
    wp, wpv = ffn.psnr_from_sums(want, shape[1] * shape[2])
    assert p.dtype == torch.float32 and tuple(p.shape) == (shape[0],)
    ok = np.isfinite(wpv)
    assert np.abs(p.cpu().numpy() - wp).max() <= PSNR_TOL * np.abs(wp).max()
    assert np.array_equal(np.isnan(pv.cpu().numpy()), np.isnan(wpv))
    if ok.any():
        assert np.abs(pv.cpu().numpy()[ok] - wpv[ok]).max() <= PSNR_TOL * np.abs(wpv[ok]).max()


def test_psnr_and_depth_images_match_the_reference_golden(hip_lib):
    import os
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_eval.npz")))
    p, pv = metrics.psnr_frames(dev(g["gt"]), dev(g["rgb"]), dev(g["mask"] == 0))
    p, pv, want = p.cpu().numpy(), pv.cpu().numpy(), g["psnr"]
    print("psnr", p, pv, "reference", want.T)
    assert np.abs(p - want[:, 0]).max() <= PSNR_TOL * np.abs(want[:, 0]).max()
    assert np.isnan(pv[1]) and np.isnan(want[1, 1])                                           # frame 1: no valid pixel
    assert np.abs(pv[[0, 2]] - want[[0, 2], 1]).max() <= PSNR_TOL * np.abs(want[[0, 2], 1]).max()
    assert pv[2] == p[2]                                                                      # frame 2: every pixel valid
    out = metrics.finish_frames(dev(g["rgb"]).repeat(2, 1, 1, 1), depth=dev(g["depth"]), lut=dev(g["lut"]))
    assert np.array_equal(out["depth_u8"].cpu().numpy(), g["depth_u8"])
    assert np.array_equal(out["depth_rgb_u8"].cpu().numpy(), g["depth_rgb_u8"])


def test_empty_and_full_masks(hip_lib):
    c = case((3, 19, 33))
    rgb, gt = dev(c["rgb"]), dev(c["gt"])
    valid = torch.zeros(3, 19, 33, dtype=torch.bool, device=DEV)
    valid[1] = True
    valid[2, 7, 11] = True
    out = metrics.finish_frames(rgb, gt=gt, valid_mask=valid, images=False)
    assert set(out) == {"sums"}
    sums = out["sums"].cpu().numpy()
    assert sums[0, 1] == 0 and sums[:, 2].tolist() == [0, 627, 1]
    assert sums[1, 1] == sums[1, 0]                                                           # same squares, same order
    p, pv = (t.cpu().numpy() for t in metrics.psnr_from_sums(out["sums"], 627))
    assert np.isnan(pv[0]) and pv[1] == p[1] and np.isfinite(pv[2])
    e = np.float32(c["gt"][2, 7, 11]) - np.clip(c["rgb"][2, 7, 11], 0, 1)
    assert sums[2, 1] == float(np.sum((e * e).astype(np.float64)))                            # three fp32 squares: exact in fp64
    none = metrics.finish_frames(rgb, gt=gt, images=False)["sums"].cpu().numpy()              # no mask: nothing selected
    assert np.array_equal(none[:, 0], sums[:, 0]) and not none[:, 1:].any()
    assert np.isnan(metrics.psnr_frames(gt, rgb)[1].cpu().numpy()).all()


@pytest.mark.parametrize("shape", [(3, 19, 33), (2, 37, 71), (2, 129, 511)])
def test_a_batch_is_bit_identical_to_single_frames(hip_lib, shape):
    c = case(shape)
    batch = finish(c)
    for f in range(shape[0]):
        one = finish(c, slice(f, f + 1))
        for key, t in one.items():
            assert torch.equal(t[0], batch[key][f]), (key, f)
    rng = batch["depth_range"].cpu().numpy()
    assert len({tuple(r) for r in rng}) == shape[0]                                           # every frame its own range
    again = finish(c)
    assert all(torch.equal(again[k], batch[k]) for k in batch)                                # and run to run


def test_scratch_is_reusable_and_unaligned_views_take_the_narrow_path(hip_lib):
    """The same numbers from arrays that start one element into their allocation (4-byte aligned fp32, odd uint8 addresses),
    through the ctypes layer with caller-owned outputs and one scratch buffer used twice (a call returns its counter words to
    zero; the partials behind them are rewritten before they are read)."""
    shape = (3, 19, 33)
    c = case(shape)
    F, H, W = shape

    def shifted(a):
        t = dev(a)
        store = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        view = store[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view
    scratch = torch.zeros(_lib.frame_finish_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    for turn in range(2):
        outs = dict(rgb_clipped=shifted(np.zeros((F, H, W, 3), np.float32)), rgb_u8=shifted(np.zeros((F, H, W, 3), np.uint8)),
                    sums=torch.empty(F, 3, dtype=torch.float64, device=DEV), depth_range=torch.empty(F, 2, device=DEV),
                    depth_u8=shifted(np.zeros((F, H, W), np.uint8)), depth_rgb_u8=shifted(np.zeros((F, H, W, 3), np.uint8)))
        _lib.frame_finish(shifted(c["rgb"]), gt=shifted(c["gt"]), valid=shifted(c["valid"]), depth=shifted(c["depth"]),
                          lut=dev(c["lut"]), scratch=scratch, **outs)
        torch.cuda.synchronize()
        assert not scratch[:16].any(), turn                                                  # the frame counters are zero again
        for key in ("rgb_u8", "depth_u8", "depth_rgb_u8", "rgb_clipped", "depth_range"):
            assert np.array_equal(outs[key].cpu().numpy(), c[key]), (key, turn)
        assert torch.equal(outs["sums"], finish(c)["sums"])                                  # the wide path adds in the same order


def test_the_call_is_capturable(hip_lib):
    """No synchronisation and no allocation inside nsff_frame_finish: two launches recorded into a graph and replayed on new data."""
    shape = (2, 37, 71)
    c = case(shape)
    F, H, W = shape
    rgb, gt, valid, depth = dev(c["rgb"]), dev(c["gt"]), dev(c["valid"]), dev(c["depth"])
    lut = dev(c["lut"])
    outs = dict(rgb_clipped=torch.empty_like(rgb), rgb_u8=torch.empty(F, H, W, 3, dtype=torch.uint8, device=DEV),
                sums=torch.empty(F, 3, dtype=torch.float64, device=DEV), depth_range=torch.empty(F, 2, device=DEV),
                depth_u8=torch.empty(F, H, W, dtype=torch.uint8, device=DEV),
                depth_rgb_u8=torch.empty(F, H, W, 3, dtype=torch.uint8, device=DEV))
    scratch = torch.zeros(_lib.frame_finish_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.frame_finish(rgb, gt=gt, valid=valid, depth=depth, lut=lut, scratch=scratch, **outs)     # warm-up outside the graph
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.frame_finish(rgb, gt=gt, valid=valid, depth=depth, lut=lut, scratch=scratch, **outs)
    rgb.copy_(rgb.flip(0))
    depth.copy_(depth.flip(0))
    gt.copy_(gt.flip(0))
    valid.copy_(valid.flip(0))
    for t in outs.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for key in ("rgb_u8", "depth_u8", "depth_rgb_u8", "rgb_clipped", "depth_range"):
        assert np.array_equal(outs[key].cpu().numpy(), c[key][::-1]), key
    assert torch.equal(outs["sums"], finish(c)["sums"].flip(0))
    assert not scratch[:16].any()


# ---- the split layer on a seeded tiny NSFF model: 12 x 16 pixels, 4 frames ----
W_IMG, H_IMG, N_POSES = 16, 12, 4
K = np.array([[18.0, 0, 8.0], [0, 19.0, 6.0], [0, 0, 1]])


def tiny_poses():
    rng = np.random.default_rng(4)
    poses = np.zeros((N_POSES, 3, 4))
    for t in range(N_POSES):
        ax, ay, az = rng.uniform(-0.05, 0.05, 3)
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        poses[t, :, :3] = Rz @ Ry @ Rx
        poses[t, :, 3] = [0.1 * t - 0.15, rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1)]
    return poses


@pytest.fixture(scope="module")
def tiny(hip_lib):
    """Model, embeddings and the plain renders of the four dataset poses at times 0..3 and at times 1..4 from pose 1."""
    cfg = dict(scenes.INTERP_CFG)
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
    for m in list(models.values()) + [emb["t"]]:
        m.to(DEV)
    poses = tiny_poses()
    common_kw = dict(N_samples=cfg["N_samples"], N_importance=cfg["N_importance"])
    flow_kw = dict(output_transient=True, output_transient_flow=["fw", "bw"])

    def render(pose, t):
        rays = evaluate.frame_rays(K, pose, H_IMG, W_IMG, device=DEV)
        ts = torch.full((H_IMG * W_IMG,), t, dtype=torch.long, device=DEV)
        return evaluate.render_frame(models, emb, rays, ts, N_POSES - 1, cfg["N_samples"], cfg["N_importance"], **flow_kw)
    plain = [render(poses[i], i) for i in range(N_POSES)]
    return dict(models=models, emb=emb, poses=poses, kw=common_kw, flow_kw=flow_kw, plain=plain, render=render)


def u8_of(rgb):
    return (255 * torch.clip(rgb.view(H_IMG, W_IMG, 3), 0, 1).cpu().numpy()).astype(np.uint8)


def test_render_split_test_frames_are_the_quantised_renders(tiny):
    frames = list(evaluate.render_split(tiny["models"], tiny["emb"], K, tiny["poses"], "test", (W_IMG, H_IMG), depth=True,
                                        **tiny["kw"], **tiny["flow_kw"]))
    assert [f[0] for f in frames] == ["000", "001", "002", "003"]
    for (name, img, dimg), res in zip(frames, tiny["plain"]):
        assert img.dtype == torch.uint8 and tuple(img.shape) == (H_IMG, W_IMG, 3) and img.is_cuda
        assert np.array_equal(img.cpu().numpy(), u8_of(res["rgb_fine"])), name
        want = ffn.depth_u8(res["depth_fine"].view(1, H_IMG, W_IMG).cpu().numpy())[0]
        assert dimg.dtype == torch.uint8 and np.array_equal(dimg.cpu().numpy(), want), name
    lut = np.random.default_rng(0).integers(0, 256, (256, 3), dtype=np.uint8)
    host = list(evaluate.render_split(tiny["models"], tiny["emb"], K, tiny["poses"], "test", (W_IMG, H_IMG), depth=True, lut=lut,
                                      to_host=True, **tiny["kw"], **tiny["flow_kw"]))
    assert [f[0] for f in host] == ["000", "001", "002", "003"]
    for (name, img, dimg), (_, dev_img, dev_idx) in zip(host, frames):
        assert not img.is_cuda and img.is_pinned() and img.dtype == torch.uint8
        assert torch.equal(img, dev_img.cpu()), name
        assert tuple(dimg.shape) == (H_IMG, W_IMG, 3) and np.array_equal(dimg.numpy(), lut[dev_idx.cpu().numpy()]), name
    no_depth = next(iter(evaluate.render_split(tiny["models"], tiny["emb"], K, tiny["poses"], "test", (W_IMG, H_IMG),
                                               **tiny["kw"], **tiny["flow_kw"])))
    assert no_depth[2] is None and torch.equal(no_depth[1], frames[0][1])


def test_render_split_fixview_interpolates_like_eval(tiny):
    frames = list(evaluate.render_split(tiny["models"], tiny["emb"], K, tiny["poses"], "test_fixview1_interp3", (W_IMG, H_IMG),
                                        **tiny["kw"]))                                        # the flow outputs are turned on inside
    assert [f[0] for f in frames] == ["000_000", "000_033", "000_066", "001_000", "001_033", "001_066", "002_000", "002_033",
                                      "002_066", "003_000"]
    at = [tiny["render"](tiny["poses"][1], t) for t in range(N_POSES)]                        # pose 1 at times 0..3
    for i in range(N_POSES):
        assert np.array_equal(frames[3 * i][1].cpu().numpy(), u8_of(at[i]["rgb_fine"])), i
    # the in-between frames: interpolate() called directly.  Its splat adds with atomics, so two runs agree to the 1e-5 of
    # test_render_sequence_mirrors_the_eval_loop, not to the bit: 255 * 1e-5 is far below one level, so a truncated value moves
    # by at most one
    for i, j in ((0, 1), (1, 2), (2, 1)):
        img, _ = A.interpolate(at[i], at[i + 1], j / 3, torch.from_numpy(K), torch.from_numpy(tiny["poses"][1]), (W_IMG, H_IMG))
        diff = np.abs(frames[3 * i + j][1].cpu().numpy().astype(int) - u8_of(img).astype(int))
        print(f"in-between {i}+{j}/3: {int((diff > 0).sum())} of {diff.size} values one level apart")
        assert diff.max() <= 1 and (diff > 0).mean() <= 0.01


def test_render_split_spiral_frames_and_times(tiny):
    gen = evaluate.render_split(tiny["models"], tiny["emb"], K, tiny["poses"], "test_spiral2", (W_IMG, H_IMG), **tiny["kw"],
                                **tiny["flow_kw"])
    name, img, _ = next(gen)
    gen.close()
    from nsff_pl_amd import paths
    path, ts, _ = paths.split_path(tiny["poses"], "test_spiral2")
    assert name == "000" and len(path) == 60 and ts.tolist() == [2] * 60
    assert np.array_equal(img.cpu().numpy(), u8_of(tiny["render"](path[0], 2)["rgb_fine"]))
    with pytest.raises(ValueError, match="test_fixview"):
        next(evaluate.render_split(tiny["models"], tiny["emb"], K, tiny["poses"], "val", (W_IMG, H_IMG), **tiny["kw"]))


def test_evaluate_split_scores_match_the_per_frame_metrics(tiny):
    rng = np.random.default_rng(9)
    gts = torch.stack([torch.clip(r["rgb_fine"].view(H_IMG, W_IMG, 3) + 0.1 * dev(rng.standard_normal((H_IMG, W_IMG, 3))
                                                                                     .astype(np.float32)), 0, 1)
                       for r in tiny["plain"]])
    masks = dev((rng.random((N_POSES, H_IMG, W_IMG)) < 0.4).astype(np.float32))
    masks[2] = 1                                                                              # frame 2: nothing static
    seen = []
    scores = evaluate.evaluate_split(tiny["models"], tiny["emb"], K, tiny["poses"], (W_IMG, H_IMG), images_gt=gts, masks=masks,
                                     sink=lambda name, img: seen.append((name, img.clone())), **tiny["kw"], **tiny["flow_kw"])
    assert len(scores) == N_POSES and [s[0] for s in seen] == ["000", "001", "002", "003"]
    psnrs, ssims = scores.psnrs, scores.ssims
    assert psnrs.shape == ssims.shape == (N_POSES, 2)
    for i, res in enumerate(tiny["plain"]):
        pred = torch.clip(res["rgb_fine"].view(H_IMG, W_IMG, 3), 0, 1)
        assert np.array_equal(seen[i][1].cpu().numpy(), u8_of(res["rgb_fine"]))
        want = [float(metrics.psnr(gts[i], pred)), float(metrics.ssim(gts[i], pred))]
        assert abs(psnrs[i, 0] - want[0]) <= PSNR_TOL * abs(want[0]) and abs(ssims[i, 0] - want[1]) <= PSNR_TOL * abs(want[1])
        if i == 2:
            assert np.isnan(psnrs[i, 1]) and np.isnan(ssims[i, 1])
            continue
        want = [float(metrics.psnr(gts[i], pred, masks[i] == 0)), float(metrics.ssim(gts[i], pred, masks[i] == 0))]
        assert abs(psnrs[i, 1] - want[0]) <= PSNR_TOL * abs(want[0]) and abs(ssims[i, 1] - want[1]) <= PSNR_TOL * abs(want[1])
    mp, ms = scores.means()
    assert np.isfinite(mp).all() and np.isfinite(ms).all() and scores.table()[2].startswith("PSNR  \t ")
    bare = evaluate.SequenceScores()
    bare.add(gts[0], tiny["plain"][0]["rgb_fine"].view(H_IMG, W_IMG, 3))
    assert bare.psnrs[0, 1] == 0 and bare.ssims[0, 1] == 0 and bare.psnrs[0, 0] == psnrs[0, 0]   # eval.py:174-175 without a mask
