"""CPU checks of the host layer that the frame kernels share: the table-driven binder of nsff_pl_amd/_lib.py refuses CPU tensors by
name before the library is touched, motion.camera_pairs walks exactly the pairs that fundamental_matrices and parallax_matrices
fill, and depth and motion check a span with one function."""
import numpy as np
import pytest
import torch

import motion_numpy as mnp
from nsff_pl_amd import _lib, depth, motion

F, H, W, SPAN = 2, 5, 7, 2
u8, i64 = torch.uint8, torch.int64
z = torch.zeros


def flows():
    return dict(flows_fw=z(F, H, W, 2), flows_bw=z(F, H, W, 2))


# wrapper -> (its keywords as CPU tensors, the first tensor it names)
CPU_CALLS = {
    "ssim": (lambda: dict(gt=z(F, H, W, 3), pred=z(F, H, W, 3), map=z(F, H, W, 3)), "image_gt"),
    "lpips": (lambda: dict(packed=z(8), gt=z(F, 31, 33, 3), pred=z(F, 31, 33, 3), map=z(F, 31, 33)), "image_gt"),
    "frame_finish": (lambda: dict(rgb=z(F, H, W, 3), rgb_u8=z(F, H, W, 3, dtype=u8)), "rgb"),
    "val_panels": (lambda: dict(F=F, H=H, W=W, pred=z(F, H, W, 3), gt=z(F, H, W, 3), ranges=z(F, 5, 2)), "pred"),
    "flow_maps": (lambda: dict(F=F, H=H, W=W, flow=(z(F, H, W, 2), None), maxrad=z(F, 2, 2)), "points / flow"),
    "motion_maps": (lambda: dict(flows(), valid=z(F, 2, H, W, dtype=u8)), "flows_fw"),
    "mask_erode": (lambda: dict(src=z(F, H, W, dtype=u8), dst=z(F, H, W, dtype=u8), k=3, zero_counts=z(F, dtype=i64)), "src"),
    "flow_median": (lambda: dict(flow=z(F, H, W, 2), grey=z(F, H, W), out=z(F, H, W, 2)), "flow"),
    "disparity_sparse": (lambda: dict(flows(), Pm=z(F, 2, 12), counts=z(F, dtype=i64)), "flows_fw"),
    "disparity_span": (lambda: dict(flows(), Pm=z(F, 2, SPAN, 12), span=SPAN, counts=z(F, dtype=i64)), "flows_fw"),
    "motion_span": (lambda: dict(flows(), Fm=z(F, 2, SPAN, 3, 3), hop_scale=z(SPAN), span=SPAN, counts=z(F, 3, dtype=i64)), "flows_fw"),
    "mask_propagate": (lambda: dict(flows(), src=z(F, H, W, dtype=u8), reach=SPAN, zero_counts=z(F, dtype=i64)), "src"),
}


@pytest.mark.parametrize("name", list(CPU_CALLS))
def test_cpu_tensors_are_refused_by_name_before_the_library_is_touched(monkeypatch, name):
    def touched():
        raise AssertionError(f"{name} reached the library")
    monkeypatch.setattr(_lib, "load", touched)
    make, first = CPU_CALLS[name]
    with pytest.raises(RuntimeError, match=f"^{name}: {first} must be a GPU tensor"):
        getattr(_lib, name)(**make())


def sequence(n_frames, seed=3):
    rng = np.random.default_rng(seed)
    K = np.array([[80.0, 0, 16], [0, 80.0, 12], [0, 0, 1.0]])
    poses = np.zeros((n_frames, 3, 4))
    for t in range(n_frames):
        poses[t, :, :3] = mnp.rotation(*rng.uniform(-0.02, 0.02, 3))
        poses[t, :, 3] = [0.1 * t, rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)]
    return K, poses


def walk(K, poses, span):
    n_frames, pairs = motion.camera_pairs("walk", K, poses, span)
    assert n_frames == len(poses)
    return list(pairs)


def test_camera_pairs_of_one_frame_and_of_a_coincident_pair():
    K, poses = sequence(3)
    assert walk(K, poses[:1], 8) == []
    poses[2, :, 3] = poses[1, :, 3]                                # frames 1 and 2 share a centre: no pair of them, either way
    got = walk(K, poses, 2)
    assert [p[:3] for p in got] == [(0, 0, 1), (0, 0, 2), (1, 1, 1), (2, 1, 2)]
    M = K @ np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(poses[:, :, :3])
    for f, d, k, M_n, M_f_inv, base in got:
        n = f + k if d == 0 else f - k
        assert np.array_equal(M_n, M[n]) and np.array_equal(M_f_inv, np.linalg.inv(M)[f])
        assert np.array_equal(base, poses[f, :, 3] - poses[n, :, 3])
    # the two tables are zero exactly where the walk yields nothing
    Fm, Pm = motion.fundamental_matrices(K, poses, span=2, rounded=False), depth.parallax_matrices(K, poses, span=2, rounded=False)
    filled = np.zeros((3, 2, 2), bool)
    for f, d, k in (p[:3] for p in got):
        filled[f, d, k - 1] = True
    assert np.array_equal(Fm.any(axis=(-1, -2)), filled) and np.array_equal(Pm.any(axis=-1), filled)


@pytest.mark.parametrize("n_frames,span,count", [(4, 8, 12), (5, 2, 14), (2, 1, 2), (6, 3, 24)])
def test_camera_pairs_counts_every_neighbour_once_each_way(n_frames, span, count):
    assert count == 2 * sum(max(n_frames - k, 0) for k in range(1, span + 1))
    got = walk(*sequence(n_frames), span)
    assert len(got) == count == len({p[:3] for p in got})
    assert all(0 <= (f + k if d == 0 else f - k) < n_frames and 1 <= k <= span for f, d, k in (p[:3] for p in got))


def test_camera_pairs_refuses_in_the_callers_name():
    K, poses = sequence(3)
    with pytest.raises(RuntimeError, match=r"^parallax_matrices: K must be \(3,3\) or \(1,3,3\), got \(2, 3\)"):
        depth.parallax_matrices(K[:2], poses)
    with pytest.raises(RuntimeError, match=r"^fundamental_matrices: poses must be \(F,3,4\) camera-to-world matrices, got \(3, 4\)"):
        motion.fundamental_matrices(K[None], poses[0])
    assert list(motion.camera_pairs("x", torch.tensor(K)[None], torch.tensor(poses), 1)[1])[0][:3] == (0, 0, 1)


def test_depth_and_motion_check_a_span_alike():
    assert _lib.DISPARITY_MAX_SPAN == motion.MAX_SPAN == 8
    for bad in (0, 9, 2.0, True, None):
        said = []
        for check in (depth._check_span, motion._check_span):
            with pytest.raises(ValueError) as e:
                check("who", bad)
            said.append(str(e.value))
        assert said[0] == said[1] == f"who: span must be an integer from 1 to 8, got {bad!r}"
    assert depth._check_span("who", np.int64(8)) == motion._check_span("who", 8) == 8
