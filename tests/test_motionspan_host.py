"""CPU checks of the several-frame motion masks: the C ABI of csrc/motionspan.hip (declared, exported, bound; argument validation
without a launch), motion.fundamental_matrices with a span, the Python layer's refusal of a bad span or reach, and the properties
of the numpy twin tests/motionspan_numpy.py that the GPU tests rely on -- span 1 is motion_numpy.motion_maps, the propagation on a
case worked out by hand -- and the method's conditions on a slow and on a pausing object, asked of the twin alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import motion_numpy as mnp
import motionspan_numpy as msn
from nsff_pl_amd import _lib, motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

_BUF = (C.c_double * 128)()                                 # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15
_SCENES = {}


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


# ---- the C ABI ----
def test_header_exports_and_bindings_declare_the_symbols():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint\s+nsff_motion_span\(const NsffMotionSpanArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint\s+nsff_mask_propagate\(const NsffMaskPropagateArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_motion_span_scratch_bytes\(int32_t n_frames, int32_t H, int32_t W\);", header)
    lib = _lib.load()
    for sym in ("nsff_motion_span", "nsff_mask_propagate", "nsff_motion_span_scratch_bytes"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert callable(_lib.motion_span) and callable(_lib.mask_propagate) and callable(_lib.motion_span_scratch_bytes)
    assert re.search(rf"#define NSFF_MOTION_MAX_SPAN\s+{_lib.MOTION_MAX_SPAN}\b", header) and _lib.MOTION_MAX_SPAN == msn.MAX_SPAN == 8
    assert re.search(rf"#define NSFF_PROPAGATE_MAX_REACH\s+{_lib.PROPAGATE_MAX_REACH}\b", header) and _lib.PROPAGATE_MAX_REACH == msn.MAX_REACH == 8
    assert motion.MAX_SPAN == 8 and motion.MAX_REACH == 8
    assert C.sizeof(_lib.MotionSpanArgs) == 16 + 8 + 9 * 8 + 8 + 8 and C.sizeof(_lib.MaskPropagateArgs) == 16 + 7 * 8 + 8 + 8
    # nothing that existed moves
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header) and lib.nsff_abi_version() == _lib.ABI_VERSION == 32
    assert C.sizeof(_lib.MotionMapsArgs) == 16 + 16 + 9 * 8 + 8 and C.sizeof(_lib.MaskErodeArgs) == 16 + 4 * 8 + 8
    makefile = open(os.path.join(ROOT, "nsff_pl_amd", "csrc", "Makefile")).read()
    assert re.search(r"\nmotionspan\.o:.*\n\t.*-ffp-contract=off -c motionspan\.hip", makefile)
    rules = 0
    for rule in makefile.split("\n\n"):                          # the object is on every list that names parallax.o
        for line in rule.splitlines():
            if "parallax.o" in line and not line.startswith(("parallax.o:", "#")):
                assert "motionspan.o" in line, line
                rules += 1
    assert rules >= 6
    small = lib.nsff_motion_span_scratch_bytes
    assert small(3, 37, 71) == 16 + 8 * 2 * 3 * 3 and small(1, 1, 1) == 16 + 16
    assert small(0, 4, 4) == 0 and small(65536, 4, 4) == 0 and small(2, 60000, 60000) == 0
    assert small(30, 288, 512) <= lib.nsff_motion_maps_scratch_bytes(30, 288, 512)      # motion_masks' one scratch serves every call


def _span_args(**kw):
    a = _lib.MotionSpanArgs(n_frames=2, H=8, W=9, span=3, threshold=1.0, flow_fw=_P, flow_bw=_P + 64, Fm=_P + 128, hop_scale=_P + 192,
                            raw=_P + 256)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _prop_args(**kw):
    a = _lib.MaskPropagateArgs(n_frames=2, H=8, W=9, reach=2, src=_P, flow_fw=_P + 256, flow_bw=_P + 320, dst=_P + 512)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def check_refusals():
    """Every refusal the header lists returns its code before anything is launched or dereferenced (the pointers are host memory).
    Also called by the GPU tests, where a launch would be possible."""
    lib = _lib.load()
    nan = float("nan")
    call = lambda **kw: lib.nsff_motion_span(C.byref(_span_args(**kw)), None)
    assert lib.nsff_motion_span(None, None) == -2
    for bad in (dict(span=0), dict(span=-1), dict(span=_lib.MOTION_MAX_SPAN + 1), dict(n_frames=0), dict(n_frames=65536), dict(H=0), dict(W=0),
                dict(H=60000, W=60000), dict(threshold=-0.5), dict(threshold=nan), dict(counts=_P, scratch=_P, scratch_bytes=8)):
        assert call(**bad) == -1, bad
    for missing in ("flow_fw", "flow_bw", "Fm", "hop_scale", "raw"):
        assert call(**{missing: None}) == -2, missing
    assert call(counts=_P) == -2                                  # counts need a scratch
    assert call(flow_fw=_P + 4) == -3 and call(flow_bw=_P + 4) == -3 and call(Fm=_P + 2) == -3 and call(hop_scale=_P + 1) == -3
    assert call(err=_P + 2) == -3 and call(counts=_P + 4, scratch=_P, scratch_bytes=1 << 20) == -3
    assert call(counts=_P, scratch=_P + 8, scratch_bytes=1 << 20) == -3

    call = lambda **kw: lib.nsff_mask_propagate(C.byref(_prop_args(**kw)), None)
    assert lib.nsff_mask_propagate(None, None) == -2
    for bad in (dict(reach=0), dict(reach=-1), dict(reach=_lib.PROPAGATE_MAX_REACH + 1), dict(n_frames=0), dict(n_frames=65536), dict(H=0),
                dict(H=60000, W=60000), dict(dst=_P), dict(dst=_P + 143), dict(src=_P + 512 + 143),      # 2 * 8 * 9 = 144 bytes each
                dict(zero_counts=_P + 768, scratch=_P + 784, scratch_bytes=8)):
        assert call(**bad) == -1, bad
    assert call(dst=_P + 144, zero_counts=_P + 768) == -2         # ... a dst that starts where src ends passes that check
    for missing in ("src", "dst", "flow_fw", "flow_bw"):
        assert call(**{missing: None}) == -2, missing
    assert call(zero_counts=_P + 768) == -2                       # counts need a scratch
    assert call(flow_fw=_P + 260) == -3 and call(flow_bw=_P + 324) == -3
    assert call(zero_counts=_P + 772, scratch=_P + 784, scratch_bytes=1 << 20) == -3
    assert call(zero_counts=_P + 768, scratch=_P + 792, scratch_bytes=1 << 20) == -3


def test_the_calls_reject_bad_arguments_without_a_launch():
    check_refusals()


def test_python_refuses_a_bad_span_or_reach_by_name():
    K, poses = np.eye(3), np.tile(np.eye(4)[:3], (3, 1, 1))
    fw = torch.zeros(3, 8, 9, 2)
    masks = torch.zeros(3, 8, 9, dtype=torch.uint8)
    for bad in (0, 9, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="fundamental_matrices: span must be an integer from 1 to 8"):
            motion.fundamental_matrices(K, poses, span=bad)
        with pytest.raises(ValueError, match="motion_masks: span must be an integer from 1 to 8"):
            motion.motion_masks(fw, fw, K, poses, span=bad)
        with pytest.raises(ValueError, match="propagate: reach must be an integer from 1 to 8"):
            motion.propagate(masks, fw, fw, reach=bad)
    for bad in (9, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="motion_masks: reach must be an integer from 0 to 8"):
            motion.motion_masks(fw, fw, K, poses, reach=bad)
    with pytest.raises(ValueError, match="motion_masks: hop_scale goes with span > 1"):
        motion.motion_masks(fw, fw, K, poses, hop_scale=[1.0])
    with pytest.raises(RuntimeError, match="motion_masks: flows_fw must be a GPU tensor"):      # good ones go on to the next check
        motion.motion_masks(fw, fw, K, poses, span=np.int64(3), reach=2)
    with pytest.raises(RuntimeError, match="propagate: flows_fw must be a GPU tensor"):
        motion.propagate(masks, fw, fw)
    for bad in ([1.0, 0.5], [1.0, -0.5, 0.3], [1.0, float("nan"), 0.3]):
        with pytest.raises(ValueError, match="motion_masks: hop_scale must hold 3 finite numbers >= 0"):
            motion._hop_scale("motion_masks", bad, 3)
    assert np.array_equal(bits(motion.default_hop_scale(8)), bits(msn.hop_scale(8))) and motion.default_hop_scale(8).dtype == np.float32
    assert np.array_equal(bits(motion._hop_scale("x", torch.tensor([1.0, 0.5]), 2)), bits(np.array([1.0, 0.5], f32)))


# ---- the matrices ----
def test_fundamental_matrices_with_a_span():
    sc = mnp.make_scene(6, 37, 71, seed=3)
    K, poses = sc["K"], sc["poses"].copy()
    poses[3, :, 3] = poses[1, :, 3]                              # frames 1 and 3 share a camera centre: a coincident pair at distance 2
    one = motion.fundamental_matrices(K, poses)
    assert one.dtype == torch.float32 and tuple(one.shape) == (6, 2, 3, 3)
    assert np.array_equal(bits(motion.fundamental_matrices(K, poses, span=1).numpy()), bits(one.numpy()))
    got = motion.fundamental_matrices(K, poses, rounded=False, span=3)
    want = msn.fm_rows(K, poses, 3)
    assert got.shape == want.shape == (6, 2, 3, 3, 3) and got.dtype == np.float64
    worst = float(np.abs(got - want).max())                      # every matrix has unit norm (or is zero)
    print(f"span 3 matrices against the twin's definition: worst difference {worst:.3e} of unit norm")
    assert worst <= 1e-6 and np.array_equal(got.any((-1, -2)), want.any((-1, -2)))
    norms = np.linalg.norm(got.reshape(6, 2, 3, 9), axis=-1)
    assert np.all((np.abs(norms - 1) < 1e-12) | (norms == 0))
    rounded = motion.fundamental_matrices(torch.tensor(K)[None], torch.tensor(poses), span=3)
    assert rounded.dtype == torch.float32 and np.array_equal(bits(rounded.numpy()), bits(got.astype(f32)))      # rounded once
    assert np.array_equal(bits(rounded[:, :, 0].numpy()), bits(one.numpy()))                    # row 0 has the bits of span 1
    zero = ~got.any((-1, -2))                                    # (F, 2, span)
    for f in range(6):
        for d, s in enumerate((+1, -1)):
            for k in (1, 2, 3):
                n = f + s * k
                assert zero[f, d, k - 1] == (not 0 <= n < 6 or {f, n} == {1, 3}), (f, d, k)
    # row k - 1 is the one-step matrix of the pair (f, f +- k)
    pair = motion.fundamental_matrices(K, poses[[0, 2]], rounded=False)
    assert np.abs(got[0, 0, 1] - pair[0, 0]).max() <= 1e-12 and np.abs(got[2, 1, 1] - pair[1, 1]).max() <= 1e-12
    # and a true correspondence lies on its line: a static point of frame 0 seen in frame 2
    X = np.array([0.3, -0.2, -4.0])
    M = K @ np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(poses[:, :, :3])
    x0, x2 = M[0] @ (X - poses[0, :, 3]), M[2] @ (X - poses[2, :, 3])
    line = got[0, 0, 1] @ (x0 / x0[2])
    assert abs(line @ (x2 / x2[2])) / np.hypot(line[0], line[1]) < 1e-9


# ---- the twin ----
@pytest.mark.parametrize("noise", [0.0, 0.3])
def test_span_1_is_the_one_frame_test(noise):
    """At span 1, hop_scale = [1], given motion_numpy.motion_maps' valid: that function's raw and over-counts exactly, and its err
    wherever valid."""
    sc = mnp.make_scene(5, 37, 71, noise=noise, seed=3)
    fw, bw = sc["flows_fw"].copy(), sc["flows_bw"].copy()
    rng = np.random.default_rng(5)
    fw[rng.random(fw.shape[:3]) < 0.02] = 1e10                    # some unknown, NaN and far-away flows
    bw[rng.random(bw.shape[:3]) < 0.02, 0] = np.nan
    fw[rng.random(fw.shape[:3]) < 0.02] += f32(500.0)
    Fm = motion.fundamental_matrices(sc["K"], sc["poses"]).numpy()
    want = mnp.motion_maps(fw, bw, Fm)
    got = msn.motion_span(fw, bw, Fm[:, :, None], np.ones(1, f32), 1, valid=want["valid"])
    assert np.array_equal(got["raw"], want["raw"]) and want["counts"][:, 4].sum() > 100
    assert got["counts"].tolist() == want["counts"][:, 2:5].tolist()
    v = want["valid"] != 0
    assert v.sum() > 0.5 * v[1:-1].size and np.array_equal(bits(got["err"])[v], bits(want["err"])[v])
    assert np.array_equal(got["hops"], want["valid"])            # one neighbour measured exactly where the one-frame test is valid
    assert (got["err"][~v] == msn.UNKNOWN).all() and got["err"].dtype == np.float32
    assert np.abs(Fm[:, :, None] - msn.fm_rows(sc["K"], sc["poses"], 1)).max() < 1e-6


def test_propagate_by_hand():
    """Three frames of 1 x 5.  Frame 1 is dynamic at x = 2, frame 2 at x = 4; fw[0] = +1, fw[1] = +0.5, bw[2] = -1, bw[1] = 0."""
    src = np.full((3, 1, 5), 255, np.uint8)
    src[1, 0, 2] = src[2, 0, 4] = 0
    src[0, 0, 0] = 7                                              # any non-zero value is static and is kept
    fw, bw = np.zeros((3, 1, 5, 2), f32), np.zeros((3, 1, 5, 2), f32)
    fw[0, ..., 0], fw[1, ..., 0], bw[2, ..., 0] = 1.0, 0.5, -1.0
    # reach 1.  frame 0: x + 1 lands on frame 1's zero from x = 1.  frame 1 forwards: rint(x + 0.5) = 0, 2, 2, 4, - (4.5 is outside):
    # x = 3 meets frame 2's zero; half-way cases go to the even pixel.  frame 2 backwards: x - 1 = 2 from x = 3.
    dst, hits, zeros = msn.propagate(src, fw, bw, 1)
    assert hits.tolist() == [[[0, 1, 0, 0, 0]], [[0, 0, 0, 1, 0]], [[0, 0, 0, 1, 0]]]
    assert dst.tolist() == [[[7, 0, 255, 255, 255]], [[255, 255, 0, 0, 255]], [[255, 255, 255, 0, 0]]] and zeros.tolist() == [1, 2, 2]
    # reach 2.  frame 0, second step: q = x + 1 + 0.5 in frame 2, rint = 2, 2, 4, - (4.5 outside), - (the first hop left the image):
    # x = 2 meets frame 2's zero.  frame 2, second step: q = x - 1 + 0 in frame 0, which has no zero.
    dst, hits, zeros = msn.propagate(src, fw, bw, 2)
    assert hits.tolist() == [[[0, 1, 1, 0, 0]], [[0, 0, 0, 1, 0]], [[0, 0, 0, 1, 0]]]
    assert dst.tolist() == [[[7, 0, 0, 255, 255]], [[255, 255, 0, 0, 255]], [[255, 255, 255, 0, 0]]] and zeros.tolist() == [2, 2, 2]
    # valid gates the start: frame 0's x = 1 has no forward vote ...
    valid = np.ones((3, 2, 1, 5), np.uint8)
    valid[0, 0, 0, 1] = 0
    assert msn.propagate(src, fw, bw, 2, valid=valid)[1][0].tolist() == [[0, 0, 1, 0, 0]]
    # ... and every hop: frame 0's x = 2 hops through frame 1 at x = 3, whose taps are x = 3 and 4
    valid = np.ones((3, 2, 1, 5), np.uint8)
    valid[1, 0, 0, 4] = 0
    assert msn.propagate(src, fw, bw, 2, valid=valid)[1][0].tolist() == [[0, 1, 0, 0, 0]]
    # an unknown flow at the hop does the same; one at the start stops the chain before its first step
    planted = fw.copy()
    planted[1, 0, 3] = 1e10
    assert msn.propagate(src, planted, bw, 2)[1].tolist() == [[[0, 1, 0, 0, 0]], [[0, 0, 0, 0, 0]], [[0, 0, 0, 1, 0]]]
    # the float64 route agrees on such numbers
    assert np.array_equal(msn.propagate(src, fw, bw, 2, dtype=np.float64)[0], dst)


def scene_case(name):
    """The two scenes of DESIGN.md section 11.3 at F = 9, 72 x 128, noise 0.05, seed 3, with the one-frame twin's result; computed
    once, read-only."""
    if name not in _SCENES:
        centres = msn.slow_centres() if name == "slow" else msn.pause_centres()
        sc = msn.make_scene_steps(9, 72, 128, centres, noise=0.05, seed=3)
        single = mnp.motion_maps(sc["flows_fw"], sc["flows_bw"], msn.fm_rows(sc["K"], sc["poses"], 1)[:, :, 0].astype(f32))
        _SCENES[name] = dict(scene=sc, single=single)
    return _SCENES[name]


def test_make_scene_steps_is_make_scene_with_the_centres_given():
    want = mnp.make_scene(5, 37, 71, noise=0.05, seed=3)
    got = msn.make_scene_steps(5, 37, 71, [mnp.disc_centre(t, 5) for t in range(5)], noise=0.05, seed=3)
    for key in ("K", "poses", "flows_fw", "flows_bw", "disc"):
        assert np.array_equal(got[key], want[key]), key


def test_a_slow_object_is_found_over_four_frames():
    """SLOW: the disc drifts 0.011 a frame (about 0.62 px) off its epipolar line.  Conditions: the one-frame test has recall 0 in
    every frame; span 4 with hop_scale 1 / sqrt(k) has disc recall >= 0.85 in every frame and flags at most 0.01 of the background
    in every frame.

    Measured on the fp32 twin (the float64 twin gives the same figures): recall per frame 0.9152 0.9170 0.9298 0.9429 0.9370
    0.9227 0.9316 0.9199 0.9218, background flagged 0 in every frame."""
    case = scene_case("slow")
    sc, single = case["scene"], case["single"]
    r1, b1 = msn.recall_and_background(single["raw"], sc["disc"])
    Fm = msn.fm_rows(sc["K"], sc["poses"], 4).astype(f32)
    out = msn.motion_span(sc["flows_fw"], sc["flows_bw"], Fm, msn.hop_scale(4), 4, valid=single["valid"])
    r4, b4 = msn.recall_and_background(out["raw"], sc["disc"])
    print(f"SLOW: one-frame recall {np.round(r1, 4).tolist()}, span 4 recall {np.round(r4, 4).tolist()}, background {np.round(b4, 5).tolist()}")
    assert (r1 == 0).all() and (b1 <= 0.01).all()
    assert (r4 >= 0.85).all()
    assert (b4 <= 0.01).all()
    assert out["hops"].max() == 4 and out["counts"][:, 2].tolist() == (out["raw"] == 0).reshape(9, -1).sum(1).tolist()
    out64 = msn.motion_span(sc["flows_fw"], sc["flows_bw"], Fm, msn.hop_scale(4), 4, valid=single["valid"], dtype=np.float64)
    assert (out64["raw"] != out["raw"]).mean() < 1e-3             # the rule does not hang on fp32's rounding


def test_a_pausing_object_is_found_from_its_neighbours():
    """PAUSE: the disc moves 0.11 a frame and stands still in frames 3, 4 and 5, so that in frame 4 neither flow moves.  Conditions:
    the one-frame test has recall 0 in frame 4; propagated with reach 2, frame 4 has disc recall >= 0.85, no frame's recall is
    lower than the one-frame test's, and at most 0.01 of the background is flagged in every frame.

    Measured on the fp32 twin (the float64 twin gives the same figures): one-frame recall 0.9653 0.9808 0.9736 0.9489 0 0.8453
    0.9864 0.9910 0.9491; with reach 2: 0.9653 0.9808 0.9736 0.9628 0.9820 0.9426 0.9864 0.9910 0.9491; background flagged 0 in
    every frame but frame 4, 0.00038 there."""
    case = scene_case("pause")
    sc, single = case["scene"], case["single"]
    r1, b1 = msn.recall_and_background(single["raw"], sc["disc"])
    dst, hits, zeros = msn.propagate(single["raw"], sc["flows_fw"], sc["flows_bw"], 2, valid=single["valid"])
    r2, b2 = msn.recall_and_background(dst, sc["disc"])
    print(f"PAUSE: one-frame recall {np.round(r1, 4).tolist()}, reach 2 recall {np.round(r2, 4).tolist()}, background {np.round(b2, 5).tolist()}")
    assert r1[4] == 0 and (b1 <= 0.01).all()
    assert r2[4] >= 0.85
    assert (r2 >= r1).all()
    assert (b2 <= 0.01).all()
    assert hits.max() <= 4 and zeros.tolist() == (dst == 0).reshape(9, -1).sum(1).tolist()
    assert not (dst[single["raw"] == 0] != 0).any()               # what was dynamic stays dynamic
