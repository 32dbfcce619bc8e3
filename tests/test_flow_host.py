"""CPU checks of the induced-flow layer: the C ABI of nsff_flow_maps (declared, exported, bound; argument validation without a
launch), the Python layer's refusals, and the numpy restatement tests/flow_numpy.py against golden g26 -- the reference's own
ndc2world, the two geometric terms of its NeRFWLoss and flowlib.flow_to_image (tests/golden/make_golden_flow.py).

flowlib.flow_error cannot serve as a golden: its ``a[[mask]]`` indexing raises IndexError under numpy 2, so the end-point-error
rule is pinned by cases small enough to work out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import flow_numpy as fnp
from nsff_pl_amd import _lib, evaluate, flow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, H, W = 3, 19, 33
TOL = 1e-4               # the project's relative bar (max-norm)
LOSS_TOL = 1e-5          # a mean of ~1000 fp32 terms against the reference's fp32 mean of the same terms
COLOUR_DIFFER = 0.01     # at most this share of a case's values may differ from the reference's image, by one level at the most
NEAR_ONE = 0.01          # ... pixels whose scaled radius is within 1e-5 of 1 left out: at most this share of a case


@pytest.fixture(scope="module")
def g26():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g26_flow.npz")))


def k4(g):
    K = g["K"]
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def test_golden_is_the_one_described(g26):
    assert g26["xyz_fw"].shape == g26["xyz_bw"].shape == (F, H * W, 3) and g26["xyz_fw"].dtype == np.float32
    assert g26["ts"].tolist() == [0, 1, 2] and int(g26["max_t"]) == 2 and g26["Ps"].shape == (1, 3, 3, 4)
    for tag in ("fw", "bw"):
        z = g26["xyz_" + tag][..., 2]
        assert ((z >= 1).sum(1) == 8).all() and z.min() >= -1 and ((z < 1) <= (z <= np.float32(0.95))).all()
        assert np.abs(g26["depth64_" + tag]).min() >= 0.05                                  # no point near a target camera's plane
        assert (g26["depth64_" + tag] < 0).any()                                            # some behind it
        assert not np.isnan(g26["xyz_" + tag]).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g26_flow.npz")) < 300_000


# ---- the numpy restatement against the reference's own statements ----
@pytest.mark.parametrize("tag", ["fw", "bw"])
def test_restatement_reproduces_the_reference_projection(g26, tag):
    xyz, ts, max_t = g26["xyz_" + tag], g26["ts"], int(g26["max_t"])
    world = fnp.ndc2world(xyz, k4(g26))
    want = g26["world_" + tag]
    err = np.abs(world - want).max() / np.abs(want).max()
    print(f"{tag}: ndc2world max-norm relative error {err:.2e}")
    assert err <= TOL
    uv, valid = fnp.project(xyz, k4(g26), g26["Ps"][0], ts, max_t, tag)
    t_ok = (ts < max_t) if tag == "fw" else (ts > 0)
    assert np.array_equal(valid, (g26["depth64_" + tag] > 0) & t_ok[:, None])               # the validity flags
    assert valid[1].sum() > 600 and 300 < valid[0 if tag == "fw" else 2].sum() < 400 and not valid[2 if tag == "fw" else 0].any()
    want = g26["uv64_" + tag]
    err = np.abs(uv[valid] - want[valid]).max() / np.abs(want[valid]).max()
    print(f"{tag}: uv of {int(valid.sum())} valid pixels, max-norm relative error {err:.2e}")
    assert err <= TOL
    # the reference's loss term is lambda / 2 times the mean L1 distance to the target pixel over the valid rays
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    target = np.stack([xs, ys], -1).reshape(1, H * W, 2) + g26["flows_" + tag].reshape(F, H * W, 2)
    mean_l1 = np.abs(uv[valid].astype(np.float64) - target[valid]).mean()
    want = float(g26[f"flow_{tag}_l"]) / (float(g26["lambda_geo"]) / 2)
    print(f"{tag}: mean L1 {mean_l1:.6f}, reference {want:.6f}")
    assert abs(mean_l1 - want) <= LOSS_TOL * want
    induced = fnp.induced_flow(xyz, k4(g26), g26["Ps"], ts, max_t, H, W, tag)
    assert induced.shape == (F, H, W, 2) and np.array_equal(fnp.known(induced).reshape(F, -1), valid)
    assert (induced.reshape(F, -1, 2)[~valid] == fnp.UNKNOWN).all()


def colour_case(got, near, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    keep = ~np.broadcast_to(near[..., None], got.shape)
    diff = np.abs(got.astype(int) - want.astype(int))[keep]
    print(f"{what}: {int((diff > 0).sum())} of {diff.size} values differ, largest {int(diff.max())}; {int(near.sum())} of {near.size} "
          "pixels near radius 1 left out")
    assert near.mean() <= NEAR_ONE
    assert diff.max() <= 1 and (diff > 0).mean() <= COLOUR_DIFFER


@pytest.mark.parametrize("tag", ["fw", "bw"])
def test_restatement_reproduces_the_reference_colour_images(g26, tag):
    gt = g26["flows_" + tag]
    img, rad, near = fnp.flow_to_image(gt)
    colour_case(img, near, g26[f"img_gt_{tag}"], f"gt {tag}")
    assert np.array_equal(rad, g26["given_ind_" + tag])
    img, rad, near = fnp.flow_to_image(gt, float(g26["given"]))
    colour_case(img, near, g26[f"img_gt_{tag}_given"], f"gt {tag}, maxrad {float(g26['given'])}")
    assert (rad == np.float32(g26["given"])).all()
    induced = fnp.induced_flow(g26["xyz_" + tag], k4(g26), g26["Ps"], g26["ts"], int(g26["max_t"]), H, W, tag)
    img, _, near = fnp.flow_to_image(induced)
    colour_case(img, near, g26[f"img_ind_{tag}"], f"induced {tag}")
    assert not img[~fnp.known(induced)].any()                                                # unknown pixels are black
    img, _, near = fnp.flow_to_image(induced, g26["given_ind_" + tag])
    colour_case(img, near, g26[f"img_ind_{tag}_given"], f"induced {tag} on the ground truth's radius")


def test_colour_wheel_and_the_special_fields():
    wheel = fnp.color_wheel()
    assert wheel.shape == (55, 3) and wheel.dtype == np.float32
    assert wheel[0].tolist() == [1, 0, 0] and wheel[15].tolist() == [1, 1, 0] and wheel[54, 0] == 1
    zero = np.zeros((1, 2, 3, 2), np.float32)
    img, rad, _ = fnp.flow_to_image(zero)
    assert rad.tolist() == [0.0] and (img == 255).all()                                     # a zero field: maxrad 0, white
    unknown = np.full((1, 2, 3, 2), fnp.UNKNOWN, np.float32)
    unknown[0, 0, 0] = np.nan
    img, rad, _ = fnp.flow_to_image(unknown)
    assert rad.tolist() == [0.0] and not img.any()                                          # nothing known: black


def test_end_point_error_rule_by_hand():
    u = fnp.UNKNOWN
    # pixel:          zero gt       unknown gt      unknown prediction   a 3-4-5 error
    gt = np.array([[[[0, 0],        [u, 1.0]],      [[1.0, 2.0],         [1.0, -1.0]]]], np.float32)
    pred = np.array([[[[7.0, 7.0],  [1.0, 1.0]],    [[2.0, u],           [4.0, 3.0]]]], np.float32)
    sums, counts = fnp.epe_sums(gt, pred)
    assert sums.tolist() == [[5.0, 0.0, 0.0]] and counts.tolist() == [[1, 0, 0]]
    gt[0, 0, 0] = [0.0, 0.5]                                                                  # non-zero in one component: counts
    pred[0, 0, 0] = [0.0, 2.0]
    mask = np.array([[[1, 1], [0, 0]]], np.uint8)
    sums, counts = fnp.epe_sums(gt, pred, mask)
    assert sums.tolist() == [[6.5, 1.5, 5.0]] and counts.tolist() == [[2, 1, 1]]
    assert fnp.epe_from_sums(sums, counts).tolist() == [[3.25, 1.5, 5.0]]
    pred[0, 1, 1] = [np.nan, 3.0]                                                             # a NaN prediction is unknown
    gt[0, 0, 0] = [np.inf, 0.5]                                                               # ... and so is an infinite ground truth
    sums, counts = fnp.epe_sums(gt, pred, mask)
    assert counts.tolist() == [[0, 0, 0]] and np.isnan(fnp.epe_from_sums(sums, counts)).all()
    t = flow.epe_from_sums(torch.tensor([[6.5, 0.0, 5.0]], dtype=torch.float64), torch.tensor([[2, 0, 1]]))
    assert t.dtype == torch.float64 and t[0, 0] == 3.25 and torch.isnan(t[0, 1]) and t[0, 2] == 5.0


# ---- C ABI ----
_BUF = (C.c_double * 64)()                                  # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15


def _args(**kw):
    a = _lib.FlowMapsArgs(n_frames=2, H=4, W=5, n_poses=3, max_t=2, fx=10.0, fy=10.0, cx=2.5, cy=2.0, Ps=_P, ts=_P, mask=_P,
                          epe_sums=_P, epe_counts=_P, maxrad=_P, scratch=_P, scratch_bytes=1 << 20)
    for name in ("xyz", "flow", "gt", "image", "gt_image"):
        getattr(a, name)[0] = getattr(a, name)[1] = _P
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(a, k)[0], getattr(a, k)[1] = v
        else:
            setattr(a, k, v)
    return a


def test_c_abi_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_flow_maps(C.byref(_args(**kw)), None)
    none = (None, None)
    assert lib.nsff_flow_maps(None, None) == -2
    for bad in (dict(H=0), dict(W=-1), dict(n_frames=0), dict(n_frames=70000), dict(H=65536, W=32768),
                dict(max_t=3), dict(max_t=-1), dict(n_poses=0), dict(fx=0.0), dict(fy=float("nan")),
                dict(flow=none, xyz=none),                                                    # images and ground truth without a map
                dict(xyz=none, flow=(None, _P)),                                              # ... of their direction
                dict(gt=none),                                                                # sums without a pair; gt images without gt
                dict(epe_counts=None), dict(epe_sums=None),                                   # sums and counts go together
                dict(epe_sums=None, epe_counts=None),                                         # a mask selects nothing then
                dict(maxrad=None),                                                            # images without a scale
                dict(scratch_bytes=8),
                dict(xyz=none, epe_sums=None, epe_counts=None, mask=None, maxrad=None, image=none, gt_image=none)):   # nothing to do
        assert call(**bad) == -1, bad
    assert call(Ps=None) == -2 and call(ts=None) == -2 and call(scratch=None) == -2
    assert call(flow=(None, _P)) == -2                                                        # points without a map to write
    assert call(scratch=_P + 8) == -3 and call(epe_sums=_P + 4) == -3 and call(flow=(_P + 4, _P)) == -3
    assert call(gt=(_P, _P + 4)) == -3 and call(xyz=(_P + 2, _P)) == -3 and call(ts=_P + 1) == -3
    need = lib.nsff_flow_maps_scratch_bytes
    assert need(0, 4, 5) == 0 and need(1, 0, 5) == 0 and need(1, 65536, 32768) == 0
    assert need(1, 1, 1) == 16 + 88 and need(3, 19, 33) == 16 + 3 * 88                        # 627 pixels: one workgroup a frame
    assert need(2, 37, 71) == 16 + 2 * 3 * 88 and need(5, 288, 512) == 32 + 5 * 144 * 88      # 2627 pixels: three; 147456: 144
    assert C.sizeof(_lib.FlowMapsArgs) == 6 * 4 + 4 * 4 + 18 * 8 + 8


def test_header_declares_the_symbols_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint nsff_flow_maps\(const NsffFlowMapsArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_flow_maps_scratch_bytes\(int32_t n_frames, int32_t H, int32_t W\);", header)
    for sym in ("nsff_flow_maps", "nsff_flow_maps_scratch_bytes"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym)
    assert callable(_lib.flow_maps) and callable(_lib.flow_maps_scratch_bytes)
    assert re.search(r"#define NSFF_FLOW_UNKNOWN\s+1e10f", header) and flow.UNKNOWN == 1e10 == float(fnp.UNKNOWN)
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header)
    assert _lib.load().nsff_abi_version() == _lib.ABI_VERSION == 32


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    import nsff_pl_amd as A
    assert A.induced_flow is flow.induced_flow and A.flow_to_image is flow.flow_to_image and A.flow_epe is flow.flow_epe
    K, Ps = np.eye(3), np.zeros((1, 3, 3, 4), np.float32)
    with pytest.raises(RuntimeError, match="induced_flow: xyz_fw must be a GPU tensor"):
        flow.induced_flow(torch.zeros(2, 20, 3), None, K, Ps, [0, 1], 2, (5, 4))
    with pytest.raises(RuntimeError, match=r"induced_flow: xyz_bw must be \(F, H\*W, 3\)"):
        flow.induced_flow(None, torch.zeros(2, 19, 3), K, Ps, [0, 1], 2, (5, 4))
    with pytest.raises(RuntimeError, match="xyz_fw must be float32"):
        flow.induced_flow(torch.zeros(2, 20, 3, dtype=torch.float64), None, K, Ps, [0, 1], 2, (5, 4))
    with pytest.raises(ValueError, match="neither xyz_fw nor xyz_bw"):
        flow.induced_flow(None, None, K, Ps, 0, 2, (5, 4))
    with pytest.raises(RuntimeError, match="flow_to_image: flow must be a GPU tensor"):
        flow.flow_to_image(torch.zeros(1, 4, 5, 2))
    with pytest.raises(RuntimeError, match=r"flow_to_image: flow: need \(F, H, W, 2\)"):
        flow.flow_to_image(torch.zeros(1, 4, 5, 3))
    with pytest.raises(RuntimeError, match="flow_epe: gt must be a GPU tensor"):
        flow.flow_epe(torch.zeros(1, 4, 5, 2), torch.zeros(1, 4, 5, 2))
    with pytest.raises(RuntimeError, match=r"flow_epe: pred: need \(F, H, W, 2\)"):
        flow.flow_epe(torch.zeros(1, 4, 5, 2), torch.zeros(4, 5, 2))

    class NoFlow(torch.nn.Module):
        has_flow_heads = False
    with pytest.raises(RuntimeError, match="no scene-flow heads"):
        evaluate.flow_frames({"fine": NoFlow()}, {}, K, np.zeros((3, 3, 4)), (5, 4), 8, 0)


def test_flow_scores_table_and_files(tmp_path):
    scores = evaluate.FlowScores()
    assert len(scores) == 0 and scores.epe.shape == (0, 2, 3) and np.isnan(scores.means()).all()
    sums = np.array([[[6.0, 2.0, 4.0], [0.0, 0.0, 0.0]], [[9.0, 0.0, 9.0], [8.0, 8.0, 0.0]]])
    counts = np.array([[[3, 1, 2], [0, 0, 0]], [[3, 0, 3], [4, 4, 0]]])
    for s, c in zip(sums, counts):
        scores.add(torch.tensor(s, dtype=torch.float64), torch.tensor(c))
    epe = scores.epe
    assert epe.shape == (2, 2, 3) and epe[0, 0].tolist() == [2.0, 2.0, 2.0] and np.isnan(epe[0, 1]).all()
    assert np.isnan(epe[1, 0, 1]) and epe[1, 1, 0] == 2.0 and np.array_equal(scores.counts, counts)
    m = scores.means()
    assert m[0].tolist() == [2.5, 2.0, 2.5] and m[1, :2].tolist() == [2.0, 2.0] and np.isnan(m[1, 2])    # nanmean over the frames
    lines = scores.table()
    assert lines[2] == "fw    \t 2.5000 \t 2.0000 \t 2.5000" and lines[3].startswith("bw    \t 2.0000 \t 2.0000 \t nan")
    scores.save(str(tmp_path / "out"))
    assert np.array_equal(np.load(tmp_path / "out" / "epe.npy"), epe, equal_nan=True)
    assert np.array_equal(np.load(tmp_path / "out" / "epe_counts.npy"), counts)
