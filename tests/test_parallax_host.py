"""CPU checks of the several-frame triangulation: the C ABI of csrc/parallax.hip (declared, exported, bound; argument validation
without a launch), depth.parallax_matrices with a span, the Python layer's refusal of a bad span, and the properties of the numpy
twin tests/parallax_numpy.py that the GPU tests rely on -- span 1 is disparity_numpy.sparse bit for bit, a chain never votes after
a failed hop -- and the method's coverage and accuracy conditions, asked of the twin alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import disparity_numpy as dnp
import parallax_numpy as pnp
from nsff_pl_amd import _lib, depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

_BUF = (C.c_double * 64)()                                  # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15
_SCENES = {}


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def scene_case(noise):
    """make_scene(7, 72, 128, noise, seed=3) with the motion twin's masks (erode 15) and validity; computed once, read-only."""
    if noise not in _SCENES:
        sc = dnp.make_scene(7, 72, 128, noise=noise, seed=3)
        _SCENES[noise] = dict(scene=sc, inputs=pnp.scene_inputs(sc, erode=15), runs={})
    return _SCENES[noise]


def scene_run(noise, span, min_parallax):
    case = scene_case(noise)
    key = (span, min_parallax)
    if key not in case["runs"]:
        sc = case["scene"]
        Pm = pnp.rows(sc["K"], sc["poses"], span).astype(f32)
        case["runs"][key] = pnp.sparse_span(sc["flows_fw"], sc["flows_bw"], Pm, span, min_parallax=min_parallax, **case["inputs"])
    return case["runs"][key]


# ---- the C ABI ----
def test_header_exports_and_bindings_declare_the_symbols():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint\s+nsff_disparity_span\(const NsffDisparitySpanArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_disparity_span_scratch_bytes\(int32_t n_frames, int32_t H, int32_t W\);", header)
    lib = _lib.load()
    for sym in ("nsff_disparity_span", "nsff_disparity_span_scratch_bytes"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert callable(_lib.disparity_span) and callable(_lib.disparity_span_scratch_bytes)
    assert re.search(rf"#define NSFF_DISPARITY_MAX_SPAN\s+{_lib.DISPARITY_MAX_SPAN}\b", header) and _lib.DISPARITY_MAX_SPAN == pnp.MAX_SPAN == 8
    assert C.sizeof(_lib.DisparitySpanArgs) == 16 + 8 + 9 * 8 + 8 + 8
    # nothing that existed moves
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header) and lib.nsff_abi_version() == _lib.ABI_VERSION == 32
    assert C.sizeof(_lib.DisparitySparseArgs) == 16 + 8 * 8 + 8 + 8
    makefile = open(os.path.join(ROOT, "nsff_pl_amd", "csrc", "Makefile")).read()
    assert re.search(r"-ffp-contract=off -c parallax\.hip", makefile) and re.search(r"-ffp-contract=off -c depth\.hip", makefile)
    for target in ("$(OUT):", "timing:", "variant:"):         # the object is on every link line
        rule = makefile[makefile.index("\n" + target):]
        assert "parallax.o" in rule[:rule.index("\n\n")], target
    small = lib.nsff_disparity_span_scratch_bytes
    assert small(3, 37, 71) == lib.nsff_disparity_sparse_scratch_bytes(3, 37, 71) == 16 + 8 * 3 * 3
    assert small(0, 4, 4) == 0 and small(1, 1, 1) == 16 + 8 and small(65536, 4, 4) == 0


def _span_args(**kw):
    a = _lib.DisparitySpanArgs(n_frames=2, H=8, W=9, span=3, min_parallax=0.5, flow_fw=_P, flow_bw=_P + 64, Pm=_P + 128, n=_P + 192,
                               c=_P + 256)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_call_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    nan = float("nan")
    call = lambda **kw: lib.nsff_disparity_span(C.byref(_span_args(**kw)), None)
    assert lib.nsff_disparity_span(None, None) == -2
    for bad in (dict(span=0), dict(span=-1), dict(span=_lib.DISPARITY_MAX_SPAN + 1), dict(n_frames=0), dict(n_frames=65536), dict(H=0),
                dict(H=60000, W=60000), dict(min_parallax=-0.5), dict(min_parallax=nan), dict(counts=_P, scratch=_P, scratch_bytes=8)):
        assert call(**bad) == -1, bad
    for missing in ("flow_fw", "flow_bw", "Pm", "n", "c"):
        assert call(**{missing: None}) == -2, missing
    assert call(counts=_P) == -2                                  # counts need a scratch
    assert call(flow_fw=_P + 4) == -3 and call(Pm=_P + 2) == -3 and call(counts=_P + 4, scratch=_P, scratch_bytes=1 << 20) == -3
    assert call(counts=_P, scratch=_P + 8, scratch_bytes=1 << 20) == -3
    assert call(votes=_P + 1) == -3 and call(votes=_P + 2) == -3  # votes go out as dwords
    assert call(votes=_P + 4, n=None) == -2                       # ... an aligned one passes that check


def test_python_refuses_a_bad_span_by_name():
    K, poses = np.eye(3), np.tile(np.eye(4)[:3], (3, 1, 1))
    fw = torch.zeros(3, 8, 9, 2)
    for bad in (0, 9, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="parallax_matrices: span must be an integer from 1 to 8"):
            depth.parallax_matrices(K, poses, span=bad)
        with pytest.raises(ValueError, match="triangulate: span must be an integer from 1 to 8"):
            depth.triangulate(fw, fw, K, poses, span=bad)
        with pytest.raises(ValueError, match="disparity_maps: span must be an integer from 1 to 8"):
            depth.disparity_maps(torch.zeros(3, 8, 9), fw, fw, K, poses, span=bad)
    with pytest.raises(RuntimeError, match="triangulate: flows_fw must be a GPU tensor"):      # a good span goes on to the next check
        depth.triangulate(fw, fw, K, poses, span=np.int64(3))


# ---- the parallax rows ----
def test_parallax_matrices_with_a_span():
    sc = dnp.make_scene(6, 37, 71, seed=3)
    K, poses = sc["K"], sc["poses"].copy()
    poses[3, :, 3] = poses[1, :, 3]                              # frames 1 and 3 share a camera centre: a coincident pair at distance 2
    one = depth.parallax_matrices(K, poses)
    assert one.dtype == torch.float32 and tuple(one.shape) == (6, 2, 12)
    assert np.array_equal(bits(one.numpy()), bits(dnp.parallax_rows(K, poses).astype(f32)))      # today's call, today's bits
    assert np.array_equal(bits(depth.parallax_matrices(K, poses, span=1).numpy()), bits(one.numpy()))
    got = depth.parallax_matrices(K, poses, rounded=False, span=3)
    want = pnp.rows(K, poses, 3)
    assert got.shape == want.shape == (6, 2, 3, 12) and got.dtype == np.float64
    scale = np.abs(want).max(-1, keepdims=True)
    worst = float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())
    print(f"span 3 rows against the twin's: worst relative difference {worst:.3e}")
    assert worst <= 1e-12 and np.array_equal(got == 0, want == 0)
    rounded = depth.parallax_matrices(torch.tensor(K)[None], torch.tensor(poses), span=3)
    assert rounded.dtype == torch.float32 and np.array_equal(bits(rounded.numpy()), bits(got.astype(f32)))      # rounded once
    assert np.array_equal(bits(rounded[:, :, 0].numpy()), bits(one.numpy()))                   # row 0 is the span 1 row
    zero = ~got.any(-1)                                          # (F, 2, span)
    for f in range(6):
        for d, s in enumerate((+1, -1)):
            for k in (1, 2, 3):
                n = f + s * k
                coincident = {f, n} == {1, 3}
                assert zero[f, d, k - 1] == (not 0 <= n < 6 or coincident), (f, d, k)
    assert zero[1, 0, 1] and zero[3, 1, 1] and not zero[1, 0, 0] and not zero[3, 1, 0] and not zero[1, 0, 2]
    # row k - 1 is the one-step row of the pair (f, f +- k): the projection it states is checked in test_disparity_host.py
    pair = dnp.parallax_rows(K, poses[[0, 2]])
    assert np.abs(got[0, 0, 1] - pair[0, 0]).max() <= 1e-12 * np.abs(pair[0, 0]).max()
    assert np.abs(got[2, 1, 1] - pair[1, 1]).max() <= 1e-12 * np.abs(pair[1, 1]).max()


# ---- the twin ----
@pytest.mark.parametrize("given", ["with", "without"])
def test_span_1_is_the_one_frame_triangulation_bit_for_bit(given):
    sc = dnp.make_scene(7, 72, 128, noise=0.3, seed=3)
    kw = pnp.scene_inputs(sc) if given == "with" else {}
    Pm = dnp.parallax_rows(sc["K"], sc["poses"]).astype(f32)
    want_n, want_c, want_counts = dnp.sparse(sc["flows_fw"], sc["flows_bw"], Pm, **kw)
    n, c, votes, counts = pnp.sparse_span(sc["flows_fw"], sc["flows_bw"], Pm[:, :, None], 1, **kw)
    assert np.array_equal(bits(n), bits(want_n)) and np.array_equal(bits(c), bits(want_c)) and counts.tolist() == want_counts.tolist()
    assert want_counts.sum() > 0.5 * n.size and votes.max() == 2 and votes.dtype == np.uint8
    assert not (c > 0)[votes == 0].any()                          # no vote, nothing known
    assert np.array_equal(bits(Pm[:, :, None]), bits(pnp.rows(sc["K"], sc["poses"], 1).astype(f32)))


@pytest.mark.parametrize("noise,bound", [(0.1, 0.015), (0.3, 0.04)])
def test_coverage_a_slow_camera_is_measured_over_two_frames(noise, bound):
    """min_parallax = 6.0 makes one frame's parallax of about 4 px too small (a slow camera, rescaled).  Condition: span 1 knows no
    static (non-disc) pixel, span 2 at least half of them, with a mean relative error over them of at most 0.015 at noise 0.1 and
    0.04 at noise 0.3.

    Measured on the twin: noise 0.1: span 2 knows 0.7290 of the static pixels, error 0.01066; noise 0.3: 0.6252, error 0.03142."""
    sc = scene_case(noise)["scene"]
    n1, c1, v1, counts1 = scene_run(noise, 1, 6.0)
    frac1, _, _ = pnp.static_stats(n1, c1, sc)
    n2, c2, v2, counts2 = scene_run(noise, 2, 6.0)
    frac2, err2, _ = pnp.static_stats(n2, c2, sc)
    print(f"noise {noise}, min_parallax 6.0: span 1 knows {frac1:.4f} of the static pixels, span 2 {frac2:.4f} with mean relative error {err2:.5f}")
    assert frac1 == 0.0 and not counts1.any() and not v1.any()
    assert frac2 >= 0.5
    assert err2 <= bound
    assert v2.max() <= 2 and counts2.tolist() == (c2 > 0).reshape(7, -1).sum(1).tolist()      # only the two-frame baselines pass


@pytest.mark.parametrize("noise", [0.1, 0.3])
def test_accuracy_three_frames_beat_one(noise):
    """min_parallax = 0.5.  Condition: the mean relative error of span 3 over the known static pixels is at most 0.8 of span 1's;
    the known sets are equal.

    Measured on the twin: noise 0.1: span 1 0.01577, span 3 0.01027 (0.651), span 4 0.00960; noise 0.3: span 1 0.04629, span 3
    0.03278 (0.708), span 4 0.03153; 0.8211 / 0.7951 of the static pixels are known."""
    sc = scene_case(noise)["scene"]
    n1, c1, _, _ = scene_run(noise, 1, 0.5)
    frac1, err1, kn1 = pnp.static_stats(n1, c1, sc)
    n3, c3, v3, _ = scene_run(noise, 3, 0.5)
    frac3, err3, kn3 = pnp.static_stats(n3, c3, sc)
    print(f"noise {noise}, min_parallax 0.5: span 1 error {err1:.5f}, span 3 error {err3:.5f} (ratio {err3 / err1:.3f}); known {frac1:.4f} / {frac3:.4f}")
    assert np.array_equal(kn1, kn3) and frac1 > 0.5
    assert err3 <= 0.8 * err1
    assert v3.max() == 6 and (v3 <= 6).all()


def test_votes_are_bounded_and_a_chain_never_votes_after_a_failed_hop():
    sc = dnp.make_scene(7, 72, 128, noise=0.1, seed=3)
    fw, bw = sc["flows_fw"], sc["flows_bw"]
    for span in (1, 2, 3, 8):
        Pm = pnp.rows(sc["K"], sc["poses"], span).astype(f32)
        votes = pnp.sparse_span(fw, bw, Pm, span)[2]
        assert (votes <= 2 * span).all() and votes.max() == min(2 * span, 6), span      # seven frames: at most six neighbours
    # one unknown forward flow in frame 3 at (y0, x0): the chains of frames 1 and 2 that pass through it stop voting there
    span, y0, x0 = 3, 30, 60
    Pm = pnp.rows(sc["K"], sc["poses"], span).astype(f32)
    planted = fw.copy()
    planted[3, y0, x0] = 1e10
    base = pnp.sparse_span(fw, bw, Pm, span)
    got = pnp.sparse_span(planted, bw, Pm, span)
    changed = got[2] != base[2]
    assert not changed[[0, 4, 5, 6]].any()                        # frame 0 reaches frame 3 with its last vote and never samples it
    ys, xs = np.meshgrid(np.arange(72, dtype=f32), np.arange(128, dtype=f32), indexing="ij")
    lost = base[2].astype(int) - got[2].astype(int)

    def lands_on(qx, qy):                                        # one of the four bilinear taps of q is the planted pixel
        fx, fy = np.floor(qx), np.floor(qy)
        return ((fx == x0) | (fx + 1 == x0)) & ((fy == y0) | (fy + 1 == y0))

    # frame 3 itself: the pixel's own flow is unknown, its forward chain never starts: three votes fewer
    assert changed[3].sum() == 1 and lost[3, y0, x0] == 3
    # frame 2: its first hop samples fw[3] at q = p + fw[2]: the vote of k = 1 stays, those of k = 2 and 3 go
    q2 = (xs + fw[2][..., 0], ys + fw[2][..., 1])
    hit2 = lands_on(*q2)
    assert hit2.any() and np.array_equal(changed[2], hit2) and (lost[2][hit2] == 2).all()
    # frame 1: its second hop does, at q = p + fw[1] + fw[2](p + fw[1]): only the vote of k = 3 goes
    q1 = (xs + fw[1][..., 0], ys + fw[1][..., 1])
    bu, bv, ok = pnp._hop(fw[2], q1[0], q1[1], None, None, f32)
    hit1 = lands_on(xs + (fw[1][..., 0] + bu), ys + (fw[1][..., 1] + bv)) & ok
    assert hit1.any() and np.array_equal(changed[1], hit1) and (lost[1][hit1] == 1).all()
    # and nothing that still votes has changed its numbers
    same = ~changed
    for a, b in zip(got[:2], base[:2]):
        assert np.array_equal(bits(a)[same], bits(b)[same])
