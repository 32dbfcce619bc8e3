"""MI355X checks of nsff_flow_maps (csrc/flow.hip) against the numpy fp32 restatement tests/flow_numpy.py (itself checked against
the reference's statements in tests/test_flow_host.py), and of evaluate.flow_frames on top of it.

Shapes (F, H, W): (1, 1, 1) one pixel; (3, 19, 33) the g26 scene -- frames at t = 0, 1, 2 with max_t = 2, so both edge rules fire,
and 627 pixels a frame: frames 1 and 2 start off any 16-byte alignment of the points (the dword path of the LDS copy) and off
4-byte alignment of the images; (2, 37, 71) 2627 pixels, odd: a workgroup covers 1024 pixels, so a frame is two full workgroups
and a partial one of 579 -- three partials for the frame's last workgroup to add, which is the smallest number at which the
order of that addition matters; (2, 129, 511) 65 919 pixels, odd -- 65 workgroups a frame, the last one ragged, so lane 0 of the
frame's last workgroup folds two partials (blocks 0 and 64) before the butterfly and every other lane one.

Colour images are compared with the twin over EVERY pixel (the radius is the same fp32 operations on both sides, so no pixel
near radius 1 needs leaving out; only atan2f differs from numpy's): at most one level, at most 1 % of the values."""
import os

import numpy as np
import pytest
import torch

import flow_numpy as fnp
import scenes
import nsff_pl_amd as A
from nsff_pl_amd import _lib, evaluate, flow

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (3, 19, 33), (2, 37, 71), (2, 129, 511)]
# relative: both sides add the same fp32 terms in float64, the reference with math.fsum (correctly rounded).  Any order of n
# non-negative terms is within (n - 1) * 2^-53 < 3e-13 for n <= 2627 terms; at (2, 129, 511) a term passes through at most 21
# additions on the device (4 in its lane, 6 + 3 in its workgroup, 2 + 6 in the frame's last workgroup): 21 * 2^-53 < 3e-15
SUM_TOL = 1e-12
COLOUR_DIFFER = 0.01


def golden(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name)))


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


_CASES = {}


def case(shape):
    """Inputs and the numpy results of one shape, computed once and shared (read-only)."""
    if shape in _CASES:
        return _CASES[shape]
    F, H, W = shape
    rng = np.random.default_rng(2600 + 10 * H + W)
    if shape == (3, 19, 33):
        g = golden("g26_flow.npz")
        c = dict(K=g["K"], Ps=g["Ps"][0], ts=g["ts"].astype(np.int64), max_t=int(g["max_t"]), xyz_fw=g["xyz_fw"], xyz_bw=g["xyz_bw"],
                 gt_fw=g["flows_fw"], gt_bw=g["flows_bw"], mask=g["masks"])
    else:
        n_poses = F + 2
        K = np.array([[1.3 * W + 7, 0, W / 2], [0, 1.4 * W + 5, H / 2], [0, 0, 1.0]])
        poses = np.zeros((n_poses, 3, 4))
        for t in range(n_poses):
            poses[t, :, :3] = rotation(*rng.uniform(-0.06, 0.06, 3))
            poses[t, :, 3] = rng.uniform(-0.2, 0.2, 3)
        Ps = A.projection_matrices(K, poses)[1][0].numpy()
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        c = dict(K=K, Ps=Ps, ts=np.arange(1, F + 1), max_t=n_poses - 1)
        for tag in ("fw", "bw"):
            # world points in front of every camera that project near their pixel (reference world2ndc, ray_utils.py:119-123) ...
            Z = -rng.uniform(1.5, 8.0, (F, H, W))
            X = (xs - K[0, 2] + rng.normal(0, 3, (F, H, W))) / K[0, 0] * -Z
            Y = -(ys - K[1, 2] + rng.normal(0, 3, (F, H, W))) / K[1, 1] * -Z
            ndc = np.stack([-K[0, 0] / K[0, 2] * X / Z, -K[1, 1] / K[1, 2] * Y / Z, 1 + 2 / Z], -1).reshape(F, H * W, 3)
            if H * W > 1:                                   # ... and a few at z >= 1, behind all of them
                for f in range(F):
                    ndc[f, rng.choice(H * W, max(H * W // 40, 1), replace=False), 2] = rng.uniform(1.0, 1.5)
            c["xyz_" + tag] = ndc.astype(np.float32)
            gt = (3 * rng.standard_normal((F, H, W, 2))).astype(np.float32)
            if H * W > 1:
                flat = gt.reshape(-1, 2)
                some = rng.permutation(len(flat))
                k = max(len(flat) // 30, 1)
                flat[some[:k]] = 0                          # zero ground truth: not counted
                flat[some[k:2 * k], 1] = 0                  # zero in one component only: counted
                flat[some[2 * k:3 * k]] = fnp.UNKNOWN       # unknown ground truth
            c["gt_" + tag] = gt
        c["mask"] = rng.choice(np.array([0, 255, 128], np.uint8), (F, H, W), p=[0.6, 0.3, 0.1])
    k4 = (c["K"][0, 0], c["K"][1, 1], c["K"][0, 2], c["K"][1, 2])
    for tag in ("fw", "bw"):
        ind = fnp.induced_flow(c["xyz_" + tag], k4, c["Ps"], c["ts"], c["max_t"], H, W, tag)
        c["flow_" + tag] = ind
        c["img_" + tag], c["rad_" + tag], _ = fnp.flow_to_image(ind)
        c["gt_img_" + tag], c["gt_rad_" + tag], _ = fnp.flow_to_image(c["gt_" + tag])
        c["img_shared_" + tag], _, _ = fnp.flow_to_image(ind, c["gt_rad_" + tag])
        c["sums_" + tag], c["counts_" + tag] = fnp.epe_sums(c["gt_" + tag], ind, c["mask"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[shape] = c
    return c


def dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)                 # (a copy: the shared cases are read-only)


def induced(c, shape, frames=slice(None), fw=True, bw=True):
    F, H, W = shape
    out = flow.induced_flow(dev(c["xyz_fw"][frames]) if fw else None, dev(c["xyz_bw"][frames]) if bw else None, c["K"],
                            dev(c["Ps"]), dev(c["ts"][frames]), c["max_t"], (W, H))
    torch.cuda.synchronize()
    return out


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def colour_close(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, what
    diff = np.abs(got.astype(int) - want.astype(int))
    print(f"{what}: {int((diff > 0).sum())} of {diff.size} values differ, largest {int(diff.max())}")
    assert diff.max() <= 1 and (diff > 0).mean() <= COLOUR_DIFFER, what


@pytest.mark.parametrize("shape", SHAPES)
def test_projection_equals_numpy_bit_for_bit(hip_lib, shape):
    c = case(shape)
    out = induced(c, shape)
    assert sorted(out) == ["flow_bw", "flow_fw"]
    for tag in ("fw", "bw"):
        got, want = out["flow_" + tag].cpu().numpy(), c["flow_" + tag]
        unknown = want == fnp.UNKNOWN
        print(f"{shape} {tag}: {int((~fnp.known(want)).sum())} of {want[..., 0].size} pixels unknown; "
              f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} values differ in their bits")
        assert np.array_equal(got == np.float32(flow.UNKNOWN), unknown)                       # UNKNOWN by value
        assert same_bits(got, want), tag
    if shape == (3, 19, 33):                                                                  # the edge rules
        assert (c["flow_fw"][2] == fnp.UNKNOWN).all() and (c["flow_bw"][0] == fnp.UNKNOWN).all()
        assert fnp.known(c["flow_fw"][1]).sum() > 600 and fnp.known(c["flow_bw"][1]).sum() > 600
    else:
        assert fnp.known(c["flow_fw"]).mean() > 0.9 or shape == (1, 1, 1) and fnp.known(c["flow_fw"]).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_maxrad_and_colour_images(hip_lib, shape):
    c = case(shape)
    for tag in ("fw", "bw"):
        for name, src, rad, img in (("induced", "flow_", "rad_", "img_"), ("ground truth", "gt_", "gt_rad_", "gt_img_")):
            got_img, got_rad = flow.flow_to_image(dev(c[src + tag]))
            torch.cuda.synchronize()
            assert got_rad.dtype == torch.float32 and same_bits(got_rad.cpu().numpy(), c[rad + tag]), (name, tag)
            colour_close(got_img.cpu().numpy(), c[img + tag], f"{shape} {name} {tag}")
            assert not got_img.cpu().numpy()[~fnp.known(c[src + tag])].any()                  # unknown pixels are black
        # a given radius: one per frame (the ground truth's), and a scalar
        got_img, got_rad = flow.flow_to_image(dev(c["flow_" + tag]), maxrad=dev(c["gt_rad_" + tag]))
        assert same_bits(got_rad.cpu().numpy(), c["gt_rad_" + tag])
        colour_close(got_img.cpu().numpy(), c["img_shared_" + tag], f"{shape} induced {tag} on the ground truth's radius")
        got_img, got_rad = flow.flow_to_image(dev(c["gt_" + tag]), maxrad=7.5)
        assert (got_rad.cpu().numpy() == np.float32(7.5)).all()
        colour_close(got_img.cpu().numpy(), fnp.flow_to_image(c["gt_" + tag], 7.5)[0], f"{shape} ground truth {tag}, maxrad 7.5")
    one_img, one_rad = flow.flow_to_image(dev(c["gt_fw"][0]))                                  # a single (H, W, 2) map
    assert tuple(one_img.shape) == shape[1:] + (3,) and one_rad.dim() == 0 and float(one_rad) == float(c["gt_rad_fw"][0])


def test_colour_images_match_the_reference_golden(hip_lib):
    g = golden("g26_flow.npz")
    for tag in ("fw", "bw"):
        img, _ = flow.flow_to_image(dev(g["flows_" + tag]))
        near = fnp.flow_to_image(g["flows_" + tag])[2]
        keep = ~np.broadcast_to(near[..., None], img.shape)
        diff = np.abs(img.cpu().numpy().astype(int) - g["img_gt_" + tag].astype(int))[keep]
        print(f"{tag}: {int((diff > 0).sum())} of {diff.size} values differ from flowlib's image")
        assert near.mean() <= 0.01 and diff.max() <= 1 and (diff > 0).mean() <= COLOUR_DIFFER


@pytest.mark.parametrize("shape", SHAPES)
def test_epe_sums_match_float64(hip_lib, shape):
    c = case(shape)
    for tag in ("fw", "bw"):
        sums, counts = flow.flow_epe(dev(c["gt_" + tag]), dev(c["flow_" + tag]), dev(c["mask"]))
        torch.cuda.synchronize()
        assert sums.dtype == torch.float64 and counts.dtype == torch.int64 and tuple(sums.shape) == tuple(counts.shape) == (shape[0], 3)
        got, want = sums.cpu().numpy(), c["sums_" + tag]
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print(f"{shape} {tag}: counts {c['counts_' + tag].tolist()}, sums max relative error {rel.max():.2e}")
        assert rel.max() <= SUM_TOL
        assert np.array_equal(counts.cpu().numpy(), c["counts_" + tag])
        assert (c["counts_" + tag][:, 1] + c["counts_" + tag][:, 2] == c["counts_" + tag][:, 0]).all()
        mean = flow.epe_from_sums(sums, counts).cpu().numpy()
        assert np.array_equal(np.isnan(mean), c["counts_" + tag] == 0)
        bare_s, bare_c = flow.flow_epe(dev(c["gt_" + tag]), dev(c["flow_" + tag]))           # no mask: nothing selected
        assert torch.equal(bare_s[:, 0], sums[:, 0]) and torch.equal(bare_c[:, 0], counts[:, 0])
        assert not bare_s[:, 1:].any() and not bare_c[:, 1:].any()
    if shape != (1, 1, 1):
        assert c["counts_fw"][:, 0].max() > 0 and c["counts_bw"][:, 0].max() > 0


def test_end_point_error_rule_by_hand(hip_lib):
    u = flow.UNKNOWN
    gt = torch.tensor([[[[0, 0], [u, 1.0]], [[1.0, 2.0], [1.0, -1.0]]]], device=DEV)
    pred = torch.tensor([[[[7.0, 7.0], [1.0, 1.0]], [[2.0, u], [4.0, 3.0]]]], device=DEV)
    sums, counts = flow.flow_epe(gt, pred)
    assert sums.tolist() == [[5.0, 0.0, 0.0]] and counts.tolist() == [[1, 0, 0]]              # only the 3-4-5 pixel counts
    gt[0, 0, 0] = torch.tensor([0.0, 0.5])
    pred[0, 0, 0] = torch.tensor([0.0, 2.0])
    sums, counts = flow.flow_epe(gt, pred, torch.tensor([[[1, 1], [0, 0]]], dtype=torch.uint8, device=DEV))
    assert sums.tolist() == [[6.5, 1.5, 5.0]] and counts.tolist() == [[2, 1, 1]]
    assert flow.epe_from_sums(sums, counts).tolist() == [[3.25, 1.5, 5.0]]


@pytest.mark.parametrize("shape", [(3, 19, 33), (2, 37, 71), (2, 129, 511)])
def test_a_batch_is_bit_identical_to_single_frames(hip_lib, shape):
    c = case(shape)
    batch = induced(c, shape)
    b_sums, b_counts = flow.flow_epe(dev(c["gt_fw"]), batch["flow_fw"], dev(c["mask"]))
    b_img, b_rad = flow.flow_to_image(dev(c["gt_bw"]))
    for f in range(shape[0]):
        one = induced(c, shape, slice(f, f + 1))
        for key in one:
            assert torch.equal(one[key][0], batch[key][f]), (key, f)
        sums, counts = flow.flow_epe(dev(c["gt_fw"][f:f + 1]), one["flow_fw"], dev(c["mask"][f:f + 1]))
        assert torch.equal(sums[0], b_sums[f]) and torch.equal(counts[0], b_counts[f]), f
        img, rad = flow.flow_to_image(dev(c["gt_bw"][f:f + 1]))
        assert torch.equal(rad[0], b_rad[f]) and torch.equal(img[0], b_img[f]), f
    again = flow.flow_epe(dev(c["gt_fw"]), batch["flow_fw"], dev(c["mask"]))
    assert torch.equal(again[0], b_sums) and torch.equal(again[1], b_counts)                  # and run to run
    assert len({float(r) for r in b_rad}) == shape[0]                                         # every frame its own radius


def test_each_stage_alone_and_all_in_one_call(hip_lib):
    """NULL points (error and colour of given maps), NULL ground truth (projection only, one direction only), a given radius --
    and the whole of it in ONE nsff_flow_maps call with caller-owned outputs and a scratch buffer used twice."""
    shape = (2, 37, 71)
    c = case(shape)
    F, H, W = shape
    only_fw = induced(c, shape, bw=False)
    assert sorted(only_fw) == ["flow_fw"] and same_bits(only_fw["flow_fw"].cpu().numpy(), c["flow_fw"])
    only_bw = induced(c, shape, fw=False)
    assert sorted(only_bw) == ["flow_bw"] and same_bits(only_bw["flow_bw"].cpu().numpy(), c["flow_bw"])
    scratch = torch.zeros(_lib.flow_maps_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    K = c["K"]
    for turn in range(2):
        out = dict(flow=(torch.empty(F, H, W, 2, device=DEV), torch.empty(F, H, W, 2, device=DEV)),
                   image=(torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV), torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV)),
                   gt_image=(torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV), torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV)),
                   epe_sums=torch.empty(F, 2, 3, dtype=torch.float64, device=DEV),
                   epe_counts=torch.empty(F, 2, 3, dtype=torch.int64, device=DEV), maxrad=torch.empty(F, 2, 2, device=DEV))
        _lib.flow_maps(F, H, W, xyz=(dev(c["xyz_fw"]), dev(c["xyz_bw"])), K4=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), Ps=dev(c["Ps"]),
                       ts=dev(c["ts"].astype(np.int32)), max_t=c["max_t"], gt=(dev(c["gt_fw"]), dev(c["gt_bw"])), mask=dev(c["mask"]),
                       share_gt_scale=True, scratch=scratch, **out)
        torch.cuda.synchronize()
        assert not scratch[:16].any(), turn                                                   # the frame counters are zero again
        for d, tag in enumerate(("fw", "bw")):
            assert same_bits(out["flow"][d].cpu().numpy(), c["flow_" + tag]), (tag, turn)
            assert same_bits(out["maxrad"][:, d, 0].cpu().numpy(), c["rad_" + tag]), (tag, turn)
            assert same_bits(out["maxrad"][:, d, 1].cpu().numpy(), c["gt_rad_" + tag]), (tag, turn)
            colour_close(out["image"][d].cpu().numpy(), c["img_shared_" + tag], f"one call, induced {tag}")
            colour_close(out["gt_image"][d].cpu().numpy(), c["gt_img_" + tag], f"one call, ground truth {tag}")
            assert np.array_equal(out["epe_counts"][:, d].cpu().numpy(), c["counts_" + tag])
            sums = flow.flow_epe(dev(c["gt_" + tag]), dev(c["flow_" + tag]), dev(c["mask"]))[0]
            assert torch.equal(out["epe_sums"][:, d], sums), (tag, turn)                      # the same order of addition


def test_an_all_unknown_frame_and_a_zero_field(hip_lib):
    F, H, W = 2, 19, 33
    maps = torch.full((F, H, W, 2), flow.UNKNOWN, device=DEV)
    maps[1] = 0
    img, rad = flow.flow_to_image(maps)
    assert rad.tolist() == [0.0, 0.0]
    assert not img[0].any()                                                                   # nothing known: black
    assert (img[1] == 255).all()                                                              # a zero field: maxrad 0, white
    gt = torch.full((F, H, W, 2), 1.5, device=DEV)
    sums, counts = flow.flow_epe(gt, maps, torch.ones(F, H, W, dtype=torch.bool, device=DEV))
    assert counts.tolist() == [[0, 0, 0], [H * W, H * W, 0]] and sums[0].tolist() == [0.0, 0.0, 0.0]
    mean = flow.epe_from_sums(sums, counts)
    assert torch.isnan(mean[0]).all() and torch.isnan(mean[1, 2])
    want = float(np.sqrt(np.float32(1.5) * np.float32(1.5) + np.float32(1.5) * np.float32(1.5)))
    assert float(mean[1, 0]) == pytest.approx(want, rel=1e-12) and float(mean[1, 1]) == float(mean[1, 0])
    # points that are all behind the cameras: every pixel UNKNOWN, both directions
    c = case((3, 19, 33))
    xyz = dev(c["xyz_fw"]).clone()
    xyz[..., 2] = 1.25
    out = flow.induced_flow(xyz, xyz, c["K"], dev(c["Ps"]), [0, 1, 2], c["max_t"], (33, 19))
    assert (out["flow_fw"] == flow.UNKNOWN).all() and (out["flow_bw"] == flow.UNKNOWN).all()


def test_nan_and_infinite_points_and_flows(hip_lib):
    shape = (3, 19, 33)
    F, H, W = shape
    c = case(shape)
    rng = np.random.default_rng(7)
    k4 = (c["K"][0, 0], c["K"][1, 1], c["K"][0, 2], c["K"][1, 2])
    xyz = {tag: c["xyz_" + tag].copy() for tag in ("fw", "bw")}
    for tag in xyz:
        flat = xyz[tag].reshape(-1)
        where = rng.permutation(flat.size)[:90]
        flat[where[:30]], flat[where[30:60]], flat[where[60:]] = np.nan, np.inf, -np.inf
    out = flow.induced_flow(dev(xyz["fw"]), dev(xyz["bw"]), c["K"], dev(c["Ps"]), dev(c["ts"]), c["max_t"], (W, H))
    for tag in ("fw", "bw"):
        want = fnp.induced_flow(xyz[tag], k4, c["Ps"], c["ts"], c["max_t"], H, W, tag)
        got = out["flow_" + tag].cpu().numpy()
        nan_point = np.isnan(xyz[tag]).any(-1).reshape(F, H, W)
        assert (got[nan_point] == fnp.UNKNOWN).all()                                          # a NaN point is invalid
        assert np.array_equal(got, want, equal_nan=True), tag
        img, rad = flow.flow_to_image(out["flow_" + tag])                                    # whatever an infinite point gave is unknown
        t_img, t_rad, _ = fnp.flow_to_image(want)
        assert same_bits(rad.cpu().numpy(), t_rad) and np.isfinite(t_rad).all()
        colour_close(img.cpu().numpy(), t_img, f"special points {tag}")
        assert not img.cpu().numpy()[~fnp.known(want)].any()
    gt, pred = c["gt_fw"].copy(), c["flow_fw"].copy()
    for a, seed in ((gt, 1), (pred, 2)):
        flat = a.reshape(-1)
        where = np.random.default_rng(seed).permutation(flat.size)[:90]
        flat[where[:30]], flat[where[30:60]], flat[where[60:]] = np.nan, np.inf, -np.inf
    sums, counts = flow.flow_epe(dev(gt), dev(pred), dev(c["mask"]))
    w_sums, w_counts = fnp.epe_sums(gt, pred, c["mask"])
    assert np.array_equal(counts.cpu().numpy(), w_counts) and np.isfinite(sums.cpu().numpy()).all()
    assert (np.abs(sums.cpu().numpy() - w_sums) <= SUM_TOL * np.abs(w_sums)).all()
    img, rad = flow.flow_to_image(dev(gt))
    t_img, t_rad, _ = fnp.flow_to_image(gt)
    assert same_bits(rad.cpu().numpy(), t_rad)
    colour_close(img.cpu().numpy(), t_img, "special flows")
    assert not img.cpu().numpy()[~fnp.known(gt)].any()                                        # a NaN pixel is simply unknown: black


def test_the_call_is_capturable(hip_lib):
    """No synchronisation and no allocation inside nsff_flow_maps: its two launches recorded into a graph and replayed on new data."""
    shape = (2, 37, 71)
    c = case(shape)
    F, H, W = shape
    K = c["K"]
    xyz = (dev(c["xyz_fw"]), dev(c["xyz_bw"]))
    gt, mask, Ps, ts = (dev(c["gt_fw"]), dev(c["gt_bw"])), dev(c["mask"]), dev(c["Ps"]), dev(c["ts"].astype(np.int32))
    u8 = lambda: torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV)
    out = dict(flow=(torch.zeros(F, H, W, 2, device=DEV), torch.zeros(F, H, W, 2, device=DEV)), image=(u8(), u8()),
               gt_image=(u8(), u8()), epe_sums=torch.zeros(F, 2, 3, dtype=torch.float64, device=DEV),
               epe_counts=torch.zeros(F, 2, 3, dtype=torch.int64, device=DEV), maxrad=torch.zeros(F, 2, 2, device=DEV))
    scratch = torch.zeros(_lib.flow_maps_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    call = lambda: _lib.flow_maps(F, H, W, xyz=xyz, K4=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), Ps=Ps, ts=ts, max_t=c["max_t"], gt=gt,
                                  mask=mask, scratch=scratch, **out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                                # warm-up outside the graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = {k: ([t.clone() for t in v] if isinstance(v, tuple) else v.clone()) for k, v in out.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t in xyz + gt + (mask, ts):                                                           # the frames change places
        t.copy_(t.flip(0))
    for v in out.values():
        for t in (v if isinstance(v, tuple) else (v,)):
            t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, v in out.items():
        for d, t in enumerate(v if isinstance(v, tuple) else (v,)):
            want = eager[k][d] if isinstance(v, tuple) else eager[k]
            assert torch.equal(t, want.flip(0)), (k, d)
    assert same_bits(out["flow"][0].cpu().numpy(), c["flow_fw"][::-1]) and not scratch[:16].any()


# ---- evaluate.flow_frames on a seeded flow-head model: the g24 / g26 cameras, 19 x 33 pixels, 3 frames ----
W_IMG, H_IMG = 33, 19


@pytest.fixture(scope="module")
def tiny(hip_lib):
    cfg = dict(scenes.INTERP_CFG)
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
    for m in list(models.values()) + [emb["t"]]:
        m.to(DEV)
    g24 = golden("g24_ray_records.npz")
    return dict(models=models, emb=emb, K=g24["K"], poses=g24["poses"], flows_fw=dev(g24["flows_fw"]), flows_bw=dev(g24["flows_bw"]),
                masks=dev(g24["masks"]), kw=dict(N_samples=cfg["N_samples"], N_importance=cfg["N_importance"]))


def test_flow_frames_maps_scores_and_names(tiny):
    n = len(tiny["poses"])
    run = evaluate.flow_frames(tiny["models"], tiny["emb"], tiny["K"], tiny["poses"], (W_IMG, H_IMG), flows_fw=tiny["flows_fw"],
                               flows_bw=tiny["flows_bw"], masks=tiny["masks"], **tiny["kw"])
    frames = list(run)
    from nsff_pl_amd import paths
    assert [f[0] for f in frames] == paths.frame_names(n) == ["000", "001", "002"]
    Ps = A.projection_matrices(tiny["K"], tiny["poses"])[1]
    per_frame = []
    for i, (name, maps) in enumerate(frames):
        assert sorted(maps) == ["flow_bw", "flow_bw_u8", "flow_fw", "flow_fw_u8", "gt_bw_u8", "gt_fw_u8"]
        rays = evaluate.frame_rays(tiny["K"], tiny["poses"][i], H_IMG, W_IMG, device=DEV)
        ts = torch.full((H_IMG * W_IMG,), i, dtype=torch.long, device=DEV)
        res = evaluate.render_frame(tiny["models"], tiny["emb"], rays, ts, n - 1, tiny["kw"]["N_samples"], tiny["kw"]["N_importance"],
                                    keys=("xyz_fw", "xyz_bw"), output_transient=True, output_transient_flow=["fw", "bw"])
        want = flow.induced_flow(res["xyz_fw"], res["xyz_bw"], tiny["K"], Ps, i, n - 1, (W_IMG, H_IMG))
        row = []
        for d, tag in enumerate(("fw", "bw")):
            got = maps["flow_" + tag]
            assert tuple(got.shape) == (H_IMG, W_IMG, 2) and got.is_cuda
            assert torch.equal(got.view(torch.int32), want["flow_" + tag][0].view(torch.int32)), (name, tag)
            gt = (tiny["flows_fw"], tiny["flows_bw"])[d][i:i + 1]
            gt_img, gt_rad = flow.flow_to_image(gt)
            assert torch.equal(maps[f"gt_{tag}_u8"], gt_img[0]), (name, tag)
            assert torch.equal(maps[f"flow_{tag}_u8"], flow.flow_to_image(got[None], maxrad=gt_rad)[0][0]), (name, tag)
            sums, counts = flow.flow_epe(gt, got[None], tiny["masks"][i:i + 1])
            row.append(flow.epe_from_sums(sums, counts)[0].cpu().numpy())
        per_frame.append(row)
    assert (frames[n - 1][1]["flow_fw"] == flow.UNKNOWN).all() and (frames[0][1]["flow_bw"] == flow.UNKNOWN).all()
    assert not frames[n - 1][1]["flow_fw_u8"].any()
    scores = run.scores
    per_frame = np.asarray(per_frame)
    assert len(scores) == n and scores.epe.shape == (n, 2, 3)
    assert np.array_equal(scores.epe, per_frame, equal_nan=True)
    assert np.isnan(scores.epe[n - 1, 0]).all() and np.isnan(scores.epe[0, 1]).all() and np.isfinite(scores.epe[1]).all()
    print("EPE per frame\n", scores.epe, "\n" + "\n".join(scores.table()))
    assert np.array_equal(scores.means(), np.nanmean(per_frame, 0))
    assert scores.table()[2].startswith("fw    \t ")


def test_flow_frames_without_ground_truth_a_subset_and_host_frames(tiny):
    plain = list(evaluate.flow_frames(tiny["models"], tiny["emb"], tiny["K"], tiny["poses"], (W_IMG, H_IMG), **tiny["kw"]))
    some = evaluate.flow_frames(tiny["models"], tiny["emb"], tiny["K"], tiny["poses"], (W_IMG, H_IMG), frames=[1], maxrad=4.0,
                                to_host=True, **tiny["kw"])
    host = list(some)
    assert [f[0] for f in host] == ["001"] and sorted(host[0][1]) == ["flow_bw", "flow_bw_u8", "flow_fw", "flow_fw_u8"]
    assert np.isnan(some.scores.epe).all() and some.scores.epe.shape == (1, 2, 3)
    for tag in ("fw", "bw"):
        got = host[0][1]["flow_" + tag]
        assert not got.is_cuda and got.is_pinned() and torch.equal(got, plain[1][1]["flow_" + tag].cpu())
        own = flow.flow_to_image(plain[1][1]["flow_" + tag][None])[0][0]
        assert torch.equal(plain[1][1][f"flow_{tag}_u8"], own)                                # no ground truth: the map's own radius
        given = flow.flow_to_image(plain[1][1]["flow_" + tag][None], maxrad=4.0)[0][0]
        assert torch.equal(host[0][1][f"flow_{tag}_u8"], given.cpu())
    with pytest.raises(ValueError, match="go together"):
        evaluate.flow_frames(tiny["models"], tiny["emb"], tiny["K"], tiny["poses"], (W_IMG, H_IMG), flows_fw=tiny["flows_fw"],
                             **tiny["kw"])
