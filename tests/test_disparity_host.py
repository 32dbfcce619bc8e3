"""CPU checks of the disparity layer: the C ABI of csrc/depth.hip (declared, exported, bound; argument validation without a launch;
the host-only entry points), depth.parallax_matrices, the Python layer's refusals, and the properties of the numpy twin
tests/disparity_numpy.py that the GPU tests rely on: cases written out by hand, and the method's accuracy condition on the twin
alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import disparity_numpy as dnp
from nsff_pl_amd import _lib, depth, motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsff_disparity_sparse_scratch_bytes", "nsff_disparity_sparse", "nsff_disparity_push", "nsff_disparity_pull",
           "nsff_disparity_relax", "nsff_disparity_result_slot", "nsff_disparity_levels", "nsff_disparity_dense_scratch_bytes",
           "nsff_disparity_dense")
f32 = np.float32

_BUF = (C.c_double * 64)()                                  # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15
_SCENES = {}


def scene_case(shape):
    """The scene and the twin's result on it in both number formats; computed once, read-only."""
    if shape not in _SCENES:
        sc = dnp.make_scene(*shape, noise=0.05, seed=0)
        _SCENES[shape] = dict(scene=sc, f32=dnp.scene_disparity(sc, dtype=np.float32), f64=dnp.scene_disparity(sc, dtype=np.float64))
    return _SCENES[shape]


# ---- the C ABI ----
def test_header_declares_the_symbols_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint\s+nsff_disparity_sparse\(const NsffDisparitySparseArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint\s+nsff_disparity_relax\(const NsffDisparityRelaxArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint\s+nsff_disparity_dense\(const NsffDisparityDenseArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_disparity_dense_scratch_bytes\(int32_t n_frames, int32_t H, int32_t W\);", header)
    lib = _lib.load()
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\(", header) and sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    for name in ("disparity_sparse", "disparity_push", "disparity_pull", "disparity_relax", "disparity_dense", "disparity_levels",
                 "disparity_dense_scratch_bytes", "disparity_sparse_scratch_bytes", "disparity_result_slot"):
        assert callable(getattr(_lib, name)), name
    for name, value in (("TILE", _lib.DISPARITY_TILE), ("K", _lib.DISPARITY_K), ("FUSED", _lib.DISPARITY_FUSED)):
        assert re.search(rf"#define NSFF_DISPARITY_{name}\s+{value}\b", header), name
    assert (_lib.DISPARITY_TILE, _lib.DISPARITY_K) in _lib.DISPARITY_PAIRS and depth.DEFAULT_FUSED == bool(_lib.DISPARITY_FUSED)
    assert depth.default_route(30, 288, 512) == (depth.DEFAULT_FUSED, _lib.DISPARITY_TILE, _lib.DISPARITY_K)
    assert depth.default_route(1, 288, 512) == (depth.DEFAULT_FUSED, 16, 2) and (16, 2) in _lib.DISPARITY_PAIRS
    assert C.sizeof(_lib.DisparitySparseArgs) == 16 + 8 * 8 + 8 + 8 and C.sizeof(_lib.DisparityRelaxArgs) == 32 + 8 + 5 * 8
    assert C.sizeof(_lib.DisparityDenseArgs) == 32 + 8 + 4 * 8 + 8 + 8
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header) and lib.nsff_abi_version() == _lib.ABI_VERSION == 32
    makefile = open(os.path.join(ROOT, "nsff_pl_amd", "csrc", "Makefile")).read()
    assert re.search(r"-ffp-contract=off -c depth\.hip", makefile)
    for target in ("$(OUT):", "timing:", "variant:"):         # the object is on every link line
        rule = makefile[makefile.index("\n" + target):]
        assert "depth.o" in rule[:rule.index("\n\n")], target


def test_host_only_entry_points():
    lib = _lib.load()
    levels = lib.nsff_disparity_levels
    assert [levels(*hw) for hw in ((1, 1), (1, 2), (2, 2), (3, 3), (19, 33), (288, 512), (129, 511))] == [1, 2, 2, 3, 7, 10, 10]
    assert levels(0, 4) == 0 and levels(4, -1) == 0 and levels(65536, 65536) == 0
    for H, W in ((1, 1), (3, 3), (37, 71), (129, 511)):
        assert levels(H, W) == len(dnp.pyramid_sizes(H, W))
    slot = lib.nsff_disparity_result_slot
    assert [slot(i, 1) for i in (0, 1, 2, 3, 30)] == [0, 1, 0, 1, 0] and [slot(i, 4) for i in (0, 1, 4, 5, 8, 9)] == [0, 1, 1, 0, 0, 1]
    assert slot(-1, 1) == -1 and slot(3, 0) == -1
    need = lib.nsff_disparity_dense_scratch_bytes
    assert need(1, 1, 1) == 16 and need(0, 4, 4) == 0 and need(65536, 4, 4) == 0 and need(1, 0, 4) == 0
    assert need(1, 3, 3) == 4 * (3 * (4 + 4) + 12)               # levels of 9 -> 12, 4 and 1 -> 4 floats; three pyramids above, one plane
    assert need(2, 37, 71) == 4 * (3 * sum((2 * h * w + 3) // 4 * 4 for h, w in dnp.pyramid_sizes(37, 71)[1:]) + (2 * 37 * 71 + 3) // 4 * 4)
    assert depth.scratch_bytes(2, 37, 71) == need(2, 37, 71)
    small = lib.nsff_disparity_sparse_scratch_bytes
    assert small(3, 37, 71) == 16 + 8 * 3 * 3 and small(0, 4, 4) == 0 and small(1, 1, 1) == 16 + 8      # three quad blocks of 1024 px


def _sparse_args(**kw):
    a = _lib.DisparitySparseArgs(n_frames=2, H=8, W=9, min_parallax=0.5, flow_fw=_P, flow_bw=_P + 64, Pm=_P + 128, n=_P + 192, c=_P + 256)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _relax_args(**kw):
    a = _lib.DisparityRelaxArgs(n_frames=2, H=8, W=9, iters=5, fused=1, tile=0, k=0, lam=8.0, sigma=0.05, n=_P, c=_P + 64, grey=_P + 128)
    a.state[0], a.state[1] = _P + 192, _P + 256
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _dense_args(**kw):
    a = _lib.DisparityDenseArgs(n_frames=2, H=8, W=9, levels=3, iters=5, fused=0, tile=0, k=0, lam=8.0, sigma=0.05, n=_P, c=_P + 64,
                                grey=_P + 128, disps=_P + 192, scratch=_P, scratch_bytes=1 << 40)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_calls_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    call = lambda **kw: lib.nsff_disparity_sparse(C.byref(_sparse_args(**kw)), None)
    assert lib.nsff_disparity_sparse(None, None) == -2
    for bad in (dict(n_frames=0), dict(n_frames=65536), dict(H=0), dict(H=60000, W=60000), dict(min_parallax=-0.5), dict(min_parallax=nan),
                dict(counts=_P, scratch=_P, scratch_bytes=8)):
        assert call(**bad) == -1, bad
    for missing in ("flow_fw", "flow_bw", "Pm", "n", "c"):
        assert call(**{missing: None}) == -2, missing
    assert call(counts=_P) == -2                                  # counts need a scratch
    assert call(flow_fw=_P + 4) == -3 and call(Pm=_P + 2) == -3 and call(counts=_P + 4, scratch=_P, scratch_bytes=1 << 20) == -3
    assert call(counts=_P, scratch=_P + 8, scratch_bytes=1 << 20) == -3

    call = lambda **kw: lib.nsff_disparity_relax(C.byref(_relax_args(**kw)), None)
    assert lib.nsff_disparity_relax(None, None) == -2
    for bad in (dict(n_frames=0), dict(W=0), dict(iters=-1), dict(iters=100001), dict(fused=2), dict(fused=-1), dict(sigma=0.0),
                dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(lam=-1.0), dict(lam=nan), dict(lam=inf), dict(tile=32),
                dict(k=4), dict(tile=32, k=5), dict(tile=48, k=4), dict(tile=16, k=4)):
        assert call(**bad) == -1, bad
    assert call(lam=0.0, n=None) == -2 and call(iters=0, c=None) == -2 and call(grey=None) == -2      # lam = 0 and iters = 0 are legal
    a = _relax_args()
    a.state[1] = a.state[0]
    assert lib.nsff_disparity_relax(C.byref(a), None) == -1
    a = _relax_args()
    a.state[0] = None
    assert lib.nsff_disparity_relax(C.byref(a), None) == -2
    assert call(grey=_P + 2) == -3
    assert call(fused=0, tile=7, k=9, n=None) == -2              # the plain route does not look at tile / k

    call = lambda **kw: lib.nsff_disparity_dense(C.byref(_dense_args(**kw)), None)
    assert lib.nsff_disparity_dense(None, None) == -2
    for bad in (dict(levels=0), dict(levels=6), dict(levels=-1), dict(iters=-1), dict(sigma=0.0), dict(lam=-0.5), dict(fused=3),
                dict(fused=1, tile=32, k=5), dict(scratch_bytes=64), dict(n_frames=0)):
        assert call(**bad) == -1, bad                             # (an 8 x 9 frame has five levels: 8x9, 4x5, 2x3, 1x2, 1x1)
    assert call(levels=5, n=None) == -2 and call(disps=None) == -2 and call(scratch=None) == -2
    assert call(scratch=_P + 8) == -3 and call(disps=_P + 2) == -3

    assert lib.nsff_disparity_push(_P, _P, _P, _P + 64, _P + 64, _P + 64, 1, 1, 1, None) == -1        # nothing above 1 x 1
    assert lib.nsff_disparity_push(_P, _P, None, _P + 64, _P + 64, _P + 64, 1, 4, 4, None) == -2
    assert lib.nsff_disparity_push(_P, _P, _P, _P + 64, _P + 66, _P + 64, 1, 4, 4, None) == -3
    assert lib.nsff_disparity_pull(_P, None, _P, _P + 64, 1, 4, 4, None) == -1       # c and n go together
    assert lib.nsff_disparity_pull(None, None, None, _P + 64, 1, 4, 4, None) == -1   # nothing to take the value from
    assert lib.nsff_disparity_pull(_P, _P, None, None, 1, 4, 4, None) == -2 and lib.nsff_disparity_pull(_P, _P, None, _P + 2, 1, 4, 4, None) == -3


def test_python_layer_refuses_bad_input_by_name():
    import nsff_pl_amd as A
    assert A.depth is depth and A.disparity_maps is depth.disparity_maps and A.triangulate is depth.triangulate
    assert {"depth", "disparity_maps", "triangulate", "densify", "parallax_matrices", "sequence_geometry"} <= set(A.__all__)
    fw = torch.zeros(2, 8, 9, 2)
    K, poses = np.eye(3), np.tile(np.eye(4)[:3], (2, 1, 1))
    with pytest.raises(RuntimeError, match="triangulate: flows_fw must be a GPU tensor"):
        depth.triangulate(fw, fw, K, poses)
    with pytest.raises(RuntimeError, match="triangulate: flows_bw: need float32, got torch.float64"):
        depth.triangulate(fw, fw.double(), K, poses)
    with pytest.raises(RuntimeError, match="triangulate: flows_fw: need float32, got torch.float16"):
        depth.triangulate(fw.half(), fw.half(), K, poses)
    with pytest.raises(RuntimeError, match=r"disparity_maps: flows_fw \(2, 8, 9, 2\) and flows_bw \(3, 8, 9, 2\) differ in shape"):
        depth.disparity_maps(torch.zeros(2, 8, 9), fw, torch.zeros(3, 8, 9, 2), K, poses)
    with pytest.raises(RuntimeError, match=r"triangulate: flows_fw: need \(F, H, W, 2\) maps"):
        depth.triangulate(fw[..., 0], fw[..., 0], K, poses)
    with pytest.raises(ValueError, match="triangulate: min_parallax must be a finite number >= 0"):
        depth.triangulate(fw, fw, K, poses, min_parallax=-1.0)
    with pytest.raises(RuntimeError, match=r"parallax_matrices: K must be \(3,3\)"):
        depth.parallax_matrices(np.eye(4), poses)
    with pytest.raises(RuntimeError, match=r"parallax_matrices: poses must be \(F,3,4\)"):
        depth.parallax_matrices(K, np.eye(4))
    plane = torch.zeros(2, 8, 9)
    with pytest.raises(RuntimeError, match="densify: sparse must be a GPU tensor"):
        depth.densify(plane, plane, plane)
    with pytest.raises(RuntimeError, match=r"densify: conf: need \(F, H, W\) float32"):
        depth.densify(plane, plane.double(), plane)
    with pytest.raises(RuntimeError, match="densify: sparse: need a tensor, got ndarray"):
        depth.densify(plane.numpy(), plane, plane)
    for bad, what in ((dict(levels=0), "levels must be an integer >= 1"), (dict(levels=2.0), "levels must be an integer >= 1"),
                      (dict(iters=-1), "iters must be an integer from 0 to 100000"), (dict(iters=True), "iters must be an integer"),
                      (dict(sigma=0.0), "sigma must be a finite number > 0"), (dict(sigma=float("nan")), "sigma must be a finite number > 0"),
                      (dict(lam=-1.0), "lam must be a finite number >= 0"), (dict(lam=float("inf")), "lam must be a finite number >= 0")):
        with pytest.raises(ValueError, match="disparity_maps: " + what):
            depth.disparity_maps(plane, fw, fw, K, poses, **bad)
    assert depth.GREY_SIGMA == 0.05 * 255


# ---- the parallax rows ----
def test_parallax_matrices_zero_rows_and_the_projection_they_state():
    sc = dnp.make_scene(4, 37, 71, seed=3)
    K, poses = sc["K"], sc["poses"].copy()
    poses[2, :, 3] = poses[1, :, 3]                              # frames 1 and 2 share a camera centre
    Pm = depth.parallax_matrices(K, poses, rounded=False)
    assert Pm.shape == (4, 2, 12) and Pm.dtype == np.float64
    zero = ~Pm.any(-1)
    assert zero.tolist() == [[False, True], [True, False], [False, True], [True, False]]      # the ends, and the coincident pair both ways
    assert np.array_equal(Pm, dnp.parallax_rows(K, poses))
    rounded = depth.parallax_matrices(torch.tensor(K)[None], torch.tensor(poses))
    assert rounded.dtype == torch.float32 and np.array_equal(rounded.numpy(), Pm.astype(f32))
    assert zero.tolist() == (~motion.fundamental_matrices(K, poses, rounded=False).reshape(4, 2, 9).any(-1)).tolist()
    # delta e + h is the projection into the neighbour of the point that pixel x of frame f sees at depth 1 / delta
    rng = np.random.default_rng(0)
    worst = 0.0
    for f, d, n in ((0, 0, 1), (1, 1, 0), (2, 0, 3), (3, 1, 2)):
        G, e = Pm[f, d, :9].reshape(3, 3), Pm[f, d, 9:]
        for _ in range(50):
            x = np.array([rng.uniform(0, 70), rng.uniform(0, 36), 1.0])
            delta = rng.uniform(0.05, 2.0)
            ray_cam = np.array([(x[0] - K[0, 2]) / K[0, 0], -(x[1] - K[1, 2]) / K[1, 1], -1.0])      # y up, z backwards
            X = poses[f, :, 3] + (1.0 / delta) * (poses[f, :, :3] @ ray_cam)
            Xc = poses[n, :, :3].T @ (X - poses[n, :, 3])         # a rotation's inverse is its transpose
            direct = np.array([K[0, 0] * Xc[0] / -Xc[2] + K[0, 2], K[1, 1] * -Xc[1] / -Xc[2] + K[1, 2]])
            q = delta * e + G @ x
            worst = max(worst, np.abs(q[:2] / q[2] - direct).max())
    print(f"parallax rows against a direct projection: worst difference {worst:.3e} px")
    assert worst <= 1e-12


# ---- the twin by hand ----
def test_one_pixel_one_direction_sideways_baseline():
    """A 1 x 1 frame whose only pixel sees a point at disparity delta; the next camera stands b to the right, so the point lands
    f b delta pixels to the left: the triangulation must return parallax / (f b), with the squared parallax as its confidence."""
    focal, b, delta = 120.0, 0.25, 0.4
    K = np.array([[focal, 0, 0.0], [0, focal, 0.0], [0, 0, 1]])
    poses = np.tile(np.eye(4)[:3], (2, 1, 1))
    poses[1, 0, 3] = b
    parallax = focal * b * delta
    fw, bw = np.zeros((2, 1, 1, 2), f32), np.zeros((2, 1, 1, 2), f32)
    fw[0, 0, 0, 0] = -parallax
    rows = dnp.parallax_rows(K, poses)
    assert rows[0, 0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, -focal * b, 0, 0]
    n, c, counts = dnp.sparse(fw, bw, rows, dtype=np.float64)
    assert counts.tolist() == [1, 0] and c[0, 0, 0] == parallax ** 2 and abs(n[0, 0, 0] / c[0, 0, 0] - parallax / (focal * b)) <= 1e-15
    assert not n[1].any() and not c[1].any()                      # frame 1: no row forward, no parallax backward
    n, c, counts = dnp.sparse(fw, bw, rows.astype(f32))
    assert n.dtype == c.dtype == f32 and counts.tolist() == [1, 0] and abs(float(n[0, 0, 0]) / float(c[0, 0, 0]) - delta) <= 2e-7 * delta
    # the votes: each of these silences the direction
    for kw in (dict(min_parallax=parallax * 1.01), dict(valid=np.zeros((2, 2, 1, 1), np.uint8)), dict(masks=np.zeros((2, 1, 1), np.uint8))):
        assert dnp.sparse(fw, bw, rows.astype(f32), **kw)[2].tolist() == [0, 0], kw
    wrong = fw.copy()
    wrong[0, 0, 0, 0] = parallax                                  # the point would lie behind the cameras: num < 0
    assert dnp.sparse(wrong, bw, rows.astype(f32))[2].tolist() == [0, 0]
    unknown = fw.copy()
    unknown[0, 0, 0, 1] = 1e10
    assert dnp.sparse(unknown, bw, rows.astype(f32))[2].tolist() == [0, 0]


def test_push_and_pull_of_a_3x3_frame_with_one_known_pixel():
    c, n = np.zeros((1, 3, 3), f32), np.zeros((1, 3, 3), f32)
    c[0, 1, 2], n[0, 1, 2] = 2.0, 1.0                             # disparity 0.5, confidence 2
    grey = np.arange(9, dtype=f32).reshape(1, 3, 3)
    c1, n1, g1 = dnp.push(c, n, grey)
    assert c1.tolist() == [[[0, 2], [0, 0]]] and n1.tolist() == [[[0, 1], [0, 0]]]
    assert g1.tolist() == [[[(0 + 1 + 3 + 4) / 4, (2 + 5) / 2], [(6 + 7) / 2, 8]]]      # the clipped blocks: 4, 2, 2 and 1 pixels
    c2, n2, g2 = dnp.push(c1, n1, g1)
    assert c2.tolist() == [[[2]]] and n2.tolist() == [[[1]]] and g2.tolist() == [[[(2 + 3.5 + 6.5 + 8) / 4]]]
    top = dnp.pull(c2, n2, None)
    assert top.tolist() == [[[0.5]]]
    mid = dnp.pull(c1, n1, top)
    assert mid.tolist() == [[[0.5, 0.5], [0.5, 0.5]]]
    assert dnp.pull(c, n, mid).tolist() == [[[0.5] * 3] * 3]
    assert dnp.pull(None, None, np.array([[[1, 2], [3, 4]]], f32), (3, 3)).tolist() == [[[1, 1, 2], [1, 1, 2], [3, 3, 4]]]
    assert dnp.pull(c2 * 0, n2, None).tolist() == [[[0]]]         # no data at all: the top is 0
    for levels in (1, 2, 3):                                      # a constant is a fixed point of the relaxation
        assert dnp.dense(n, c, grey, levels=levels, iters=4).tolist() == [[[0.5] * 3] * 3]
    assert not dnp.dense(n * 0, c * 0, grey, levels=3, iters=4).any()
    one = np.ones((1, 1, 1), f32)
    assert dnp.dense(one * 3, one * 4, one, levels=1, iters=2).tolist() == [[[0.75]]] and not dnp.dense(one * 0, one * 0, one, levels=1, iters=2).any()


def test_one_relax_iteration_by_hand():
    """A 1 x 3 row, the middle pixel across a strong edge from the right one: g = 1 towards the left, 1 / (1 + 10^2) to the right."""
    d = np.array([[[1.0, 2.0, 4.0]]], f32)
    grey = np.array([[[0.25, 0.25, 0.75]]], f32)
    n, c = np.array([[[0.0, 3.0, 0.0]]], f32), np.array([[[0.0, 2.0, 0.0]]], f32)
    out = dnp.relax(d, n, c, grey, lam=8.0, sigma=0.05, iters=1)
    g = 1 / 101
    want = [(8 * 2.0) / 8, (3 + 8 * (1.0 + g * 4.0)) / (2 + 8 * (1 + g)), (8 * g * 2.0) / (8 * g)]
    assert out.dtype == f32 and np.allclose(out[0, 0], want, rtol=1e-6, atol=0)
    assert np.array_equal(dnp.relax(d, n, c, grey, lam=0.0, iters=3)[0, 0], np.array([1.0, 1.5, 4.0], f32))    # no smoothing: the data, or d itself


# ---- the method, asked of the twin alone ----
@pytest.mark.parametrize("shape", [(4, 37, 71), (3, 64, 96)])
def test_the_method_condition_holds_on_the_twin(shape):
    """make_scene(F, H, W, noise=0.05, seed=0); masks = the motion twin's raw eroded with k = 15, valid from motion_maps, min_parallax
    0.5, sigma 0.05 on the scene's 0..1 guide, lam 8, 3 levels, 30 iterations.  Condition: over the static (non-disc) pixels of every
    frame the mean of |d - 1/depth| / (1/depth) is at most HALF that of the best constant, the median true disparity of those pixels.

    Measured on the twin: (4, 37, 71) ratio 0.2112 in fp32 and 0.2112 in float64 (method 0.00663, constant 0.03139);
    (3, 64, 96) ratio 0.1674 in fp32 and 0.1674 in float64 (method 0.00532, constant 0.03179)."""
    case = scene_case(shape)
    sc = case["scene"]
    for name in ("f32", "f64"):
        d = case[name]["disps"]
        ratio, method, const = dnp.static_error(d, sc)
        print(f"{shape} {name}: ratio {ratio:.4f} (method {method:.5f}, constant {const:.5f}); known {case[name]['counts'].tolist()}")
        assert d.dtype == (f32 if name == "f32" else np.float64) and d.shape == shape
        assert ratio <= 0.5
        assert np.isfinite(d).all() and (d > 0).all() and (case[name]["counts"] > 0).all()
    assert np.abs(case["f32"]["disps"] - case["f64"]["disps"]).max() < 1e-4


def test_the_disc_takes_its_surrounds_disparity_and_an_unknown_frame_is_zero():
    case = scene_case((4, 37, 71))
    sc, r = case["scene"], case["f32"]
    disc = sc["disc"]
    assert not (r["c"][disc] > 0).any() and (r["masks"][disc] == 0).all()         # the disc is masked: nothing is measured on it
    truth = 1.0 / sc["depth"]
    for f in range(4):
        filled, around = r["disps"][f][disc[f]], truth[f][~disc[f]]
        assert np.isfinite(filled).all() and (filled > 0).all()
        assert around.min() <= filled.min() and filled.max() <= around.max()       # the surround's range (about 0.25) ...
        assert np.abs(filled - truth[f][disc[f]]).min() > 0.1                      # ... not the disc's own 0.4: the documented limit
    masks = r["masks"].copy()
    masks[1] = 0                                                  # a frame without a static pixel
    rows = dnp.parallax_rows(sc["K"], sc["poses"]).astype(f32)
    n, c, counts = dnp.sparse(sc["flows_fw"], sc["flows_bw"], rows, valid=r["valid"], masks=masks)
    assert counts[1] == 0 and (counts[[0, 2, 3]] > 0).all() and np.array_equal(n[0], r["n"][0])
    d = dnp.dense(n, c, sc["guide"], levels=3, iters=30)
    assert not d[1].any() and np.array_equal(d[0], r["disps"][0]) and (d[[0, 2, 3]] > 0).all()
