"""CPU checks of the motion-mask layer: the C ABI of nsff_motion_maps / nsff_mask_erode (declared, exported, bound; argument
validation without a launch), motion.fundamental_matrices against the epipolar constraint in float64, the numpy twin's erosion
(tests/motion_numpy.py) against scipy and a case written out by hand, the Python layer's refusals -- and whether the method finds
a moving object at all, on the fp32 twin alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import motion_numpy as mnp
from nsff_pl_amd import _lib, frames, motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI ----
_BUF = (C.c_double * 64)()                                  # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15


def _maps_args(**kw):
    a = _lib.MotionMapsArgs(n_frames=2, H=4, W=5, epipolar=1, alpha=0.01, beta=0.5, threshold=1.0, flow_fw=_P, flow_bw=_P, Fm=_P,
                            err=_P, valid=_P, raw=_P, counts=_P, err_sums=_P, scratch=_P, scratch_bytes=1 << 20)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _erode_args(**kw):
    a = _lib.MaskErodeArgs(n_frames=2, H=4, W=5, k=15, src=_P, dst=_P + 64, zero_counts=_P, scratch=_P, scratch_bytes=1 << 20)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_motion_maps_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_motion_maps(C.byref(_maps_args(**kw)), None)
    assert lib.nsff_motion_maps(None, None) == -2
    for bad in (dict(H=0), dict(W=-1), dict(n_frames=0), dict(n_frames=70000), dict(H=65536, W=32768), dict(epipolar=2),
                dict(epipolar=-1), dict(alpha=-0.1), dict(beta=float("nan")), dict(threshold=-1.0), dict(threshold=float("nan")),
                dict(counts=None), dict(err_sums=None),                                       # counts and sums go together
                dict(err=None, valid=None, raw=None, counts=None, err_sums=None),             # nothing to compute
                dict(scratch_bytes=8)):
        assert call(**bad) == -1, bad
    assert call(flow_fw=None) == -2 and call(flow_bw=None) == -2 and call(Fm=None) == -2 and call(scratch=None) == -2
    assert call(scratch=_P + 8) == -3 and call(flow_fw=_P + 4) == -3 and call(flow_bw=_P + 4) == -3
    assert call(counts=_P + 4) == -3 and call(err_sums=_P + 4) == -3 and call(Fm=_P + 2) == -3 and call(err=_P + 1) == -3
    need = lib.nsff_motion_maps_scratch_bytes
    assert need(0, 4, 5) == 0 and need(1, 0, 5) == 0 and need(1, 65536, 32768) == 0
    assert need(1, 1, 1) == 16 + 40 and need(3, 19, 33) == 16 + 3 * 40                        # one workgroup a frame: five words
    assert need(2, 37, 71) == 16 + 2 * 3 * 40 and need(5, 288, 512) == 32 + 5 * 144 * 40      # 2627 pixels: three; 147456: 144
    assert need(1, 1000, 1) == 16 + 32 * 8                                                    # thin: the erosion's 32 tiles need more
    assert C.sizeof(_lib.MotionMapsArgs) == 4 * 4 + 4 * 4 + 9 * 8 + 8


def test_mask_erode_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_mask_erode(C.byref(_erode_args(**kw)), None)
    assert lib.nsff_mask_erode(None, None) == -2
    for bad in (dict(H=0), dict(W=0), dict(n_frames=0), dict(n_frames=65536), dict(k=0), dict(k=-3), dict(k=2), dict(k=14),
                dict(k=32), dict(k=33), dict(dst=_P), dict(scratch_bytes=8)):
        assert call(**bad) == -1, bad
    assert call(src=None) == -2 and call(dst=None) == -2 and call(scratch=None) == -2
    assert call(scratch=_P + 8) == -3 and call(zero_counts=_P + 4) == -3
    assert C.sizeof(_lib.MaskErodeArgs) == 4 * 4 + 4 * 8 + 8 and _lib.ERODE_MAX_K == motion.ERODE_MAX_K == 31


def test_header_declares_the_symbols_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint nsff_motion_maps\(const NsffMotionMapsArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_motion_maps_scratch_bytes\(int32_t n_frames, int32_t H, int32_t W\);", header)
    assert re.search(r"\bint nsff_mask_erode\(const NsffMaskErodeArgs\* args, void\* stream\);", header)
    for sym in ("nsff_motion_maps", "nsff_motion_maps_scratch_bytes", "nsff_mask_erode"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym)
    assert callable(_lib.motion_maps) and callable(_lib.motion_maps_scratch_bytes) and callable(_lib.mask_erode)
    assert re.search(r"#define NSFF_ERODE_MAX_K\s+31\b", header) and motion.UNKNOWN == 1e10 == float(mnp.UNKNOWN)
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header)
    assert _lib.load().nsff_abi_version() == _lib.ABI_VERSION == 32


# ---- fundamental matrices ----
def test_fundamental_matrices_satisfy_the_epipolar_constraint():
    """For world points in front of both cameras, x_n^T Fm x_f vanishes in float64 before rounding: <= 1e-9 |x_n| |Fm| |x_f|."""
    rng = np.random.default_rng(5)
    F = 5
    K = np.array([[410.0, 0, 255.5], [0, 395.0, 143.2], [0, 0, 1.0]])
    poses = np.zeros((F, 3, 4))
    for t in range(F):
        poses[t, :, :3] = mnp.rotation(*rng.uniform(-0.2, 0.2, 3))
        poses[t, :, 3] = rng.uniform(-0.5, 0.5, 3)
    Fm = motion.fundamental_matrices(K, poses, rounded=False)
    assert Fm.shape == (F, 2, 3, 3) and Fm.dtype == np.float64
    Ps = (K @ np.diag([1.0, -1.0, -1.0]) @ np.concatenate(
        [np.linalg.inv(poses[:, :, :3]), -np.linalg.inv(poses[:, :, :3]) @ poses[:, :, 3:]], 2))      # frames.projection_matrices, float64
    assert np.allclose(Ps, frames.projection_matrices(K, poses)[1][0].numpy(), rtol=1e-6, atol=1e-4)
    X = np.concatenate([rng.uniform(-2, 2, (200, 2)), rng.uniform(-9, -3, (200, 1)), np.ones((200, 1))], 1)   # in front: z < 0
    worst = 0.0
    for f in range(F):
        for d, n in enumerate((f + 1, f - 1)):
            if not 0 <= n < F:
                assert not Fm[f, d].any()                                                     # the sequence ends: a zero matrix
                continue
            assert abs(np.linalg.norm(Fm[f, d]) - 1) <= 1e-12                                 # unit Frobenius norm
            xf, xn = X @ Ps[f].T, X @ Ps[n].T
            assert (xf[:, 2] > 0).all() and (xn[:, 2] > 0).all()
            res = np.abs(np.einsum("pi,ij,pj->p", xn, Fm[f, d], xf))
            worst = max(worst, (res / (np.linalg.norm(xn, axis=1) * np.linalg.norm(xf, axis=1))).max())
    print(f"largest |x_n^T Fm x_f| / (|x_n| |Fm| |x_f|) = {worst:.2e}")
    assert worst <= 1e-9
    rounded = motion.fundamental_matrices(torch.tensor(K)[None], torch.tensor(poses))
    assert rounded.dtype == torch.float32 and not rounded.is_cuda and np.array_equal(rounded.numpy(), Fm.astype(np.float32))


def test_fundamental_matrices_are_zero_without_a_baseline():
    K = np.array([[100.0, 0, 50], [0, 100.0, 40], [0, 0, 1.0]])
    poses = np.zeros((4, 3, 4))
    for t in range(4):
        poses[t, :, :3] = mnp.rotation(0.01 * t, -0.02 * t, 0.0)
        poses[t, :, 3] = [0.1 * t, 0.0, 0.0]
    poses[2, :, 3] = poses[1, :, 3]                              # frames 1 and 2 share a camera centre (a pure rotation between them)
    Fm = motion.fundamental_matrices(K, poses).numpy()
    zero = ~Fm.reshape(4, 2, 9).any(-1)
    assert zero.tolist() == [[False, True], [True, False], [False, True], [True, False]]
    assert not motion.fundamental_matrices(K, poses[:1]).any()  # one frame: no neighbour at all
    with pytest.raises(RuntimeError, match="poses must be"):
        motion.fundamental_matrices(K, np.zeros((3, 4, 4)))
    with pytest.raises(RuntimeError, match="K must be"):
        motion.fundamental_matrices(np.eye(4), poses)


# ---- the twin's erosion ----
def test_twin_erosion_equals_scipy_minimum_filter():
    ndimage = pytest.importorskip("scipy").ndimage
    rng = np.random.default_rng(3)
    for shape, k in (((5, 9), 15), ((37, 150), 15), ((37, 150), 3), ((20, 31), 1), ((23, 40), 31)):
        for img in (rng.choice(np.array([0, 255], np.uint8), shape, p=[0.02, 0.98]), rng.integers(0, 256, shape, dtype=np.uint8)):
            want = ndimage.minimum_filter(img, size=k, mode="constant", cval=255)
            assert np.array_equal(mnp.erode(img, k), want), (shape, k)
    stack = rng.integers(0, 256, (3, 11, 13), dtype=np.uint8)
    assert np.array_equal(mnp.erode(stack, 5), np.stack([mnp.erode(s, 5) for s in stack]))


def test_twin_erosion_by_hand():
    m = np.full((9, 11), 255, np.uint8)
    m[0, 0], m[4, 5], m[8, 10], m[2, 8], m[3, 8] = 7, 0, 100, 50, 20
    w = 255
    want = np.array([[7, 7, w, w, w, w, w, w, w, w, w],
                     [7, 7, w, w, w, w, w, 50, 50, 50, w],
                     [w, w, w, w, w, w, w, 20, 20, 20, w],
                     [w, w, w, w, 0, 0, 0, 20, 20, 20, w],
                     [w, w, w, w, 0, 0, 0, 20, 20, 20, w],
                     [w, w, w, w, 0, 0, 0, w, w, w, w],
                     [w, w, w, w, w, w, w, w, w, w, w],
                     [w, w, w, w, w, w, w, w, w, 100, 100],
                     [w, w, w, w, w, w, w, w, w, 100, 100]], np.uint8)
    assert np.array_equal(mnp.erode(m, 3), want)
    assert np.array_equal(mnp.erode(m, 1), m)
    assert not mnp.erode(m, 15).any()                           # the window reaches the zero at (4, 5) from every pixel
    m[4, 5] = 255
    far = mnp.erode(m, 15)                                      # ... without it: 7 where rows 0 .. 7 and columns 0 .. 7 are in reach
    assert far[0, 0] == 7 and far[7, 7] == 7 and far[8, 7] == 20 and far[8, 0] == 255 and far[8, 3] == 20 and far[0, 8] == 20


# ---- does the method work?  (the fp32 twin alone) ----
@pytest.mark.parametrize("shape", [(4, 37, 71), (3, 64, 96)])
def test_the_method_finds_the_moving_disc_and_nothing_else(shape):
    """A static wavy background, a camera moving sideways, a disc in front that moves up: flow noise sigma 0.05 px, threshold 1.0,
    before erosion.  No background pixel may be flagged; disc recall >= 0.9 on frames with two neighbours, >= 0.7 at the ends.

    Measured on the fp32 twin (seed 1): (4, 37, 71): recall 0.978, 0.983, 0.980, 0.930 (the ends first and last), 87-89 % of pixels
    valid per direction, largest background error 0.195 px; (3, 64, 96): recall 0.958, 0.967, 0.939, 90-91 % valid, 0.197 px."""
    F, H, W = shape
    sc = mnp.make_scene(F, H, W, noise=0.05, seed=1)
    assert sc["disc"].reshape(F, -1).sum(1).min() > 0.1 * H * W                               # the disc is a tenth of the image and more
    out = mnp.motion_maps(sc["flows_fw"], sc["flows_bw"], motion.fundamental_matrices(sc["K"], sc["poses"]).numpy(), threshold=1.0)
    dynamic = out["raw"] == 0
    for f in range(F):
        disc = sc["disc"][f]
        recall = (dynamic[f] & disc).sum() / disc.sum()
        flagged = int((dynamic[f] & ~disc).sum())
        share = out["counts"][f, :2] / (H * W)
        print(f"{shape} frame {f}: recall {recall:.3f}, background pixels flagged {flagged}, valid {share.round(3).tolist()}")
        assert flagged == 0
        assert recall >= (0.9 if 0 < f < F - 1 else 0.7)
        assert out["counts"][f, 4] == dynamic[f].sum() and ((share > 0.8) == [f < F - 1, f > 0]).all()
    # the consistency check alone gives the same votes here (every line is proper), and the pixels the disc is about to cover fail it
    alone = mnp.motion_maps(sc["flows_fw"], sc["flows_bw"], None)
    assert np.array_equal(alone["valid"], out["valid"]) and (alone["raw"] == 255).all() and (alone["err"] == mnp.UNKNOWN).all()
    ys, xs = np.mgrid[0:H, 0:W]
    for f in range(F - 1):
        qx, qy = np.rint(xs + sc["flows_fw"][f, ..., 0]).astype(int), np.rint(ys + sc["flows_fw"][f, ..., 1]).astype(int)
        inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        core = mnp.erode(np.where(sc["disc"][f + 1], 255, 0).astype(np.uint8), 3) == 255      # the next frame's disc without its rim
        covered = ~sc["disc"][f] & inside & core[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
        assert covered.sum() > 0 and not out["valid"][f, 0][covered].any()


# ---- Python layer ----
def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    import nsff_pl_amd as A
    assert A.motion is motion and A.motion_masks is motion.motion_masks and A.flow_consistency is motion.flow_consistency
    assert A.fundamental_matrices is motion.fundamental_matrices
    K, poses = np.eye(3), np.zeros((2, 3, 4))
    fl = torch.zeros(2, 4, 5, 2)
    with pytest.raises(RuntimeError, match="motion_masks: flows_fw must be a GPU tensor"):
        motion.motion_masks(fl, fl, K, poses)
    with pytest.raises(RuntimeError, match=r"motion_masks: flows_bw: need \(F, H, W, 2\)"):
        motion.motion_masks(fl, torch.zeros(2, 4, 5, 3), K, poses)
    with pytest.raises(RuntimeError, match="flows_fw: need float32"):
        motion.motion_masks(fl.double(), fl, K, poses)
    with pytest.raises(RuntimeError, match="differ in shape"):
        motion.motion_masks(fl, torch.zeros(3, 4, 5, 2), K, poses)
    with pytest.raises(RuntimeError, match="flow_consistency: flows_fw must be a GPU tensor"):
        motion.flow_consistency(fl, fl)
    with pytest.raises(RuntimeError, match=r"flow_consistency: flows_fw: need \(F, H, W, 2\)"):
        motion.flow_consistency(torch.zeros(4, 5, 2), fl)
    with pytest.raises(ValueError, match="threshold must be a number >= 0"):
        motion.motion_masks(fl, fl, K, poses, threshold=-1.0)
    for k in (2, 14, 0, 33, 32, 3.0, True):                                                   # even, out of range, not an integer
        with pytest.raises(ValueError, match="window k must be an odd integer from 1 to 31"):
            motion.erode(torch.zeros(1, 4, 5, dtype=torch.uint8), k)
        with pytest.raises(ValueError, match="motion_masks: the window k must be an odd integer"):
            motion.motion_masks(fl, fl, K, poses, erode=k)
    with pytest.raises(RuntimeError, match="erode: mask must be a GPU tensor"):
        motion.erode(torch.zeros(1, 4, 5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="erode: mask: need uint8"):
        motion.erode(torch.zeros(1, 4, 5))
    with pytest.raises(RuntimeError, match=r"erode: mask: need \(F, H, W\) or \(H, W\)"):
        motion.erode(torch.zeros(1, 1, 4, 5, dtype=torch.uint8))
