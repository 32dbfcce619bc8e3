"""CPU checks of the optical-flow layer: the C ABI of csrc/optflow.hip (declared, exported, bound; argument validation without a
launch; the host-only entry points), the Python layer's refusals, and the properties of the fp32 twin tests/optflow_numpy.py that
the GPU tests rely on: identical images give exactly zero flow, and the accuracy condition holds on the twin alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import optflow_numpy as onp
from nsff_pl_amd import _lib, optflow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsff_optflow_grey", "nsff_optflow_down", "nsff_optflow_up", "nsff_optflow_median", "nsff_optflow_warp",
           "nsff_optflow_iterate", "nsff_optflow_result_slot", "nsff_optflow_levels", "nsff_optflow_scratch_bytes", "nsff_optflow")

_BUF = (C.c_double * 64)()                                  # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15


def _iter_args(**kw):
    a = _lib.OptflowIterArgs(n_pairs=2, H=8, W=9, iters=5, fused=1, tile=0, k=0, lam=0.15, theta=0.3, tau=0.25, consts=_P)
    a.state[0], a.state[1] = _P + 64, _P + 128
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _flow_args(**kw):
    a = _lib.OptflowArgs(n_pairs=2, H=16, W=20, channels=3, levels=5, warps=2, iters=5, median=1, fused=1, tile=0, k=0, lam=0.15,
                         theta=0.3, tau=0.25, images0=_P, images1=_P + 64, flow=_P + 128, scratch=_P, scratch_bytes=1 << 40)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_header_declares_the_symbols_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint\s+nsff_optflow\(const NsffOptflowArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint\s+nsff_optflow_iterate\(const NsffOptflowIterArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_optflow_scratch_bytes\(int32_t n_pairs, int32_t H, int32_t W, int32_t levels\);", header)
    lib = _lib.load()
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\(", header) and sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    for name in ("optflow", "optflow_iterate", "optflow_warp", "optflow_grey", "optflow_down", "optflow_up", "optflow_median",
                 "optflow_scratch_bytes", "optflow_levels", "optflow_result_slot"):
        assert callable(getattr(_lib, name)), name
    for name, value in (("MIN_SIZE", 16), ("TILE", _lib.OPTFLOW_TILE), ("K", _lib.OPTFLOW_K), ("FUSED", _lib.OPTFLOW_FUSED)):
        assert re.search(rf"#define NSFF_OPTFLOW_{name}\s+{value}\b", header), name
    assert (_lib.OPTFLOW_TILE, _lib.OPTFLOW_K) in _lib.OPTFLOW_PAIRS and optflow.DEFAULT_FUSED == bool(_lib.OPTFLOW_FUSED)
    assert C.sizeof(_lib.OptflowIterArgs) == 8 * 4 + 4 * 4 + 3 * 8 and C.sizeof(_lib.OptflowArgs) == 12 * 4 + 4 * 4 + 4 * 8 + 8
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header) and lib.nsff_abi_version() == _lib.ABI_VERSION == 32
    makefile = open(os.path.join(ROOT, "nsff_pl_amd", "csrc", "Makefile")).read()
    assert re.search(r"-ffp-contract=off -c optflow\.hip", makefile)
    for target in ("$(OUT):", "timing:", "variant:"):         # the object is on every link line
        rule = makefile[makefile.index("\n" + target):]
        assert "optflow.o" in rule[:rule.index("\n\n")], target


def test_host_only_entry_points():
    lib = _lib.load()
    slot = lib.nsff_optflow_result_slot
    assert [slot(i, 1) for i in (1, 2, 3, 30)] == [1, 0, 1, 0] and [slot(i, 4) for i in (1, 4, 5, 8, 9, 11, 30)] == [1, 1, 0, 0, 1, 1, 0]
    assert slot(0, 4) == -1 and slot(3, 0) == -1
    levels = lib.nsff_optflow_levels
    assert levels(288, 512, 5) == 5 and levels(16, 16, 5) == 3 and levels(16, 400, 9) == 3 and levels(144, 256, 4) == 4
    assert levels(72, 96, 9) == 5 and levels(15, 64, 3) == 0 and levels(64, 64, 0) == 0 and levels(64, 64, 17) == 0
    for H, W, n in ((288, 512, 5), (16, 16, 5), (72, 96, 9), (37, 53, 4)):
        assert levels(H, W, n) == onp.n_levels(H, W, n)
    need = lib.nsff_optflow_scratch_bytes
    assert need(0, 64, 64, 3) == 0 and need(1, 15, 64, 3) == 0 and need(1, 64, 64, 0) == 0 and need(40000, 64, 64, 3) == 0
    assert need(1, 16, 16, 5) == 4 * (2 * (256 + 64 + 16) + 19 * 256)
    assert need(3, 17, 19, 2) == 4 * (2 * (972 + 272) + 19 * 972)        # 3 * 17 * 19 = 969 -> 972, 3 * 9 * 10 = 270 -> 272
    assert need(2, 64, 64, 1) == 4 * 21 * 8192 and _lib.optflow_scratch_bytes(2, 64, 64, 1) == optflow.scratch_bytes(2, 64, 64, 1)


def test_iterate_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_optflow_iterate(C.byref(_iter_args(**kw)), None)
    assert lib.nsff_optflow_iterate(None, None) == -2
    for bad in (dict(H=3), dict(W=3), dict(n_pairs=0), dict(n_pairs=65536), dict(H=40000, W=60000), dict(iters=0), dict(iters=100001),
                dict(fused=2), dict(fused=-1), dict(lam=0.0), dict(theta=-0.3), dict(tau=float("nan")), dict(lam=float("inf")),
                dict(tile=32), dict(k=4), dict(tile=32, k=5), dict(tile=48, k=4), dict(tile=16, k=4)):
        assert call(**bad) == -1, bad
    assert call(consts=None) == -2
    for slot in (0, 1):
        a = _iter_args()
        a.state[slot] = None
        assert lib.nsff_optflow_iterate(C.byref(a), None) == -2
    a = _iter_args()
    a.state[1] = a.state[0]
    assert lib.nsff_optflow_iterate(C.byref(a), None) == -1
    assert call(consts=_P + 2) == -3
    a = _iter_args()
    a.state[0] = _P + 66
    assert lib.nsff_optflow_iterate(C.byref(a), None) == -3
    assert call(fused=0, tile=7, k=9, consts=None) == -2   # the plain route does not look at tile / k: it gets as far as the pointers


def test_the_other_calls_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_optflow(C.byref(_flow_args(**kw)), None)
    assert lib.nsff_optflow(None, None) == -2
    for bad in (dict(H=15), dict(W=15), dict(n_pairs=0), dict(n_pairs=32768), dict(channels=2), dict(channels=4), dict(levels=0),
                dict(levels=17), dict(warps=0), dict(warps=1001), dict(iters=0), dict(median=2), dict(fused=3), dict(lam=-1.0),
                dict(theta=0.0), dict(tau=float("nan")), dict(tile=32, k=5), dict(scratch_bytes=1024)):
        assert call(**bad) == -1, bad
    assert call(images0=None) == -2 and call(images1=None) == -2 and call(flow=None) == -2 and call(scratch=None) == -2
    assert call(scratch=_P + 8) == -3 and call(flow=_P + 4) == -3 and call(channels=1, images0=_P + 2) == -3
    assert call(channels=3, images0=_P + 1, images1=None) == -2            # bytes need no alignment
    assert lib.nsff_optflow_grey(None, _P, 1, 4, 4, 3, None) == -2 and lib.nsff_optflow_grey(_P, _P + 64, 1, 4, 4, 2, None) == -1
    assert lib.nsff_optflow_grey(_P + 2, _P + 64, 1, 4, 4, 1, None) == -3 and lib.nsff_optflow_grey(_P, _P + 64, 0, 4, 4, 3, None) == -1
    for fn in (lib.nsff_optflow_down, lib.nsff_optflow_up, lib.nsff_optflow_median):
        assert fn(None, _P, 1, 8, 8, None) == -2 and fn(_P, None, 1, 8, 8, None) == -2 and fn(_P, _P + 66, 1, 8, 8, None) == -3
        assert fn(_P, _P + 64, 0, 8, 8, None) == -1 and fn(_P, _P + 64, 1, 8, 0, None) == -1
    assert lib.nsff_optflow_down(_P, _P + 64, 1, 1, 8, None) == -1 and lib.nsff_optflow_median(_P, _P, 1, 8, 8, None) == -1
    assert lib.nsff_optflow_warp(_P, _P, None, _P + 64, 1, 8, 8, None) == -2 and lib.nsff_optflow_warp(_P, _P, _P, _P + 64, 1, 0, 8, None) == -1
    assert lib.nsff_optflow_warp(_P, _P + 1, _P, _P + 64, 1, 8, 8, None) == -3


def test_python_layer_refuses_bad_input_by_name():
    import nsff_pl_amd as A
    assert A.optflow is optflow and A.optical_flow is optflow.optical_flow and A.sequence_flows is optflow.sequence_flows
    assert {"optflow", "optical_flow", "sequence_flows"} <= set(A.__all__)
    rgb, grey = torch.zeros(2, 16, 20, 3, dtype=torch.uint8), torch.zeros(2, 16, 20)
    with pytest.raises(RuntimeError, match="optical_flow: images0 must be a GPU tensor"):
        optflow.optical_flow(rgb, rgb)
    with pytest.raises(RuntimeError, match="optical_flow: images0 must be a GPU tensor"):
        optflow.optical_flow(grey, grey)
    with pytest.raises(RuntimeError, match="optical_flow: images0: need a tensor, got ndarray"):
        optflow.optical_flow(rgb.numpy(), rgb)
    with pytest.raises(RuntimeError, match=r"images0 \(2, 16, 20, 3\) and images1 \(3, 16, 20, 3\) differ in shape"):
        optflow.optical_flow(rgb, torch.zeros(3, 16, 20, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="images0 is torch.uint8, images1 torch.float32"):
        optflow.optical_flow(rgb, grey)
    with pytest.raises(RuntimeError, match="images1: need uint8 colour frames or float32 grey frames, got torch.float64"):
        optflow.optical_flow(grey, grey.double())
    with pytest.raises(RuntimeError, match=r"looks channels-first \(P,3,H,W\): permute"):
        optflow.optical_flow(torch.zeros(2, 3, 16, 20, dtype=torch.uint8), torch.zeros(2, 3, 16, 20, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"images0: need channels-last \(P, H, W, 3\) uint8 or grey \(P, H, W\) float32"):
        optflow.optical_flow(torch.zeros(2, 16, 20, 3), torch.zeros(2, 16, 20, 3))      # float colour frames
    with pytest.raises(RuntimeError, match="frames of 16 x 16 pixels or more"):
        optflow.optical_flow(torch.zeros(1, 15, 40), torch.zeros(1, 15, 40))
    for bad in (dict(levels=0), dict(levels=2.0), dict(warps=0), dict(iters=True), dict(iters=0)):
        with pytest.raises(ValueError, match="must be an integer from 1 to"):
            optflow.optical_flow(grey, grey, **bad)
    for bad in (dict(lam=0.0), dict(theta=-1.0), dict(tau=float("nan")), dict(lam=float("inf"))):
        with pytest.raises(ValueError, match="must be a finite number > 0"):
            optflow.optical_flow(grey, grey, **bad)
    assert optflow.default_route(58, 288, 512) == (optflow.TILE, optflow.K) == (_lib.OPTFLOW_TILE, _lib.OPTFLOW_K)
    assert optflow.default_route(1, 288, 512) == (16, 2) and optflow.default_route(4, 256, 512) == (32, 3) and (16, 2) in _lib.OPTFLOW_PAIRS
    with pytest.raises(RuntimeError, match="sequence_flows: images: need a sequence of two frames or more"):
        optflow.sequence_flows(rgb[:1])
    with pytest.raises(RuntimeError, match="sequence_flows: images: need a tensor"):
        optflow.sequence_flows([rgb[0], rgb[1]])
    with pytest.raises(RuntimeError, match="optical_flow: images0 must be a GPU tensor"):
        optflow.sequence_flows(rgb)


# ---- the twin alone ----
def test_identical_images_give_exactly_zero_flow():
    """With rho_c = 0 the threshold step returns -0 / g and nothing ever moves: u stays +0 through every level, warp and median."""
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    for med in (True, False):
        flow = onp.optical_flow(img, img, levels=3, warps=2, iters=7, median_filter=med)
        assert flow.shape == (2, 37, 53, 2) and flow.dtype == np.float32 and not flow.any()
    pair = onp.make_pair(40, 48)
    assert not onp.optical_flow(pair["images1"], pair["images1"], levels=9, warps=1, iters=3).any()
    consts = onp.warp(onp.grey(img), onp.grey(img), np.zeros((2, 2, 37, 53), np.float32))
    assert not consts[3].any() and consts[2].max() > 100 and np.array_equal(consts[4], onp.grey(img))     # rho_c = 0, I1w = I1


def test_twin_stages_by_hand():
    ramp = (np.arange(9, dtype=np.float32) * 3)[None, None, :] + (np.arange(7, dtype=np.float32) * 5)[None, :, None]
    small = onp.down(ramp)                                      # a linear ramp survives the blur away from the border
    assert small.shape == (1, 4, 5) and small[0, 1, 1] == ramp[0, 2, 2] and small[0, 2, 3] == ramp[0, 4, 6]
    assert small[0, 0, 0] == (11 * 0 + 4 * 3 + 6) / 16 + (11 * 0 + 4 * 5 + 10) / 16      # the replicated border: rows / columns 0, 0, 0, 1, 2
    big = onp.up(small, (7, 9))
    assert big.shape == (1, 7, 9) and big[0, 2, 2] == 2 * small[0, 1, 1] and big[0, 3, 2] == small[0, 1, 1] + small[0, 2, 1]
    assert big[0, 6, 8] == 2 * small[0, 3, 4]
    assert onp.up(np.ones((1, 4, 5), np.float32), (8, 10))[0, 7, 9] == 2      # the last row / column of an even level: clamped
    grey = onp.grey(np.array([[[[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]]]], np.uint8))
    assert grey.dtype == np.float32 and np.allclose(grey[0, 0], [255, 76.245, 149.685, 29.07], rtol=1e-6)
    m = np.arange(12, dtype=np.float32).reshape(1, 3, 4)
    m[0, 1, 1] = 100.0
    assert onp.median(m).tolist() == [[[1, 2, 3, 3], [4, 6, 7, 7], [8, 9, 10, 10]]]
    flat = np.full((1, 6, 6), 10.0, np.float32)                 # no gradient: g = 0, f = 0, and with p = 0 the flow stays as it is
    state = np.zeros((6, 1, 6, 6), np.float32)
    state[0], state[1] = 0.5, -0.25
    consts = onp.warp(flat, flat, state[:2])
    assert not consts[:4].any() and np.array_equal(onp.iterate(consts, state, 3), state)
    p = np.zeros((6, 1, 4, 5), np.float32)                      # the divergence's border rule on p11 = 1: 1, 0, ..., 0, -1 along x
    p[2] = 1.0
    out = onp.iterate(np.zeros((5, 1, 4, 5), np.float32), p, 1, theta=0.5)
    assert out[0, 0, 2].tolist() == [0.5, 0, 0, 0, -0.5] and not out[1].any()


def test_the_accuracy_condition_holds_on_the_twin():
    """The 144 x 256 two-motion pair, 4 levels, 5 warps, 30 iterations, median on: the mean end-point error over the pixels more than
    6 px from the disc's rim and more than 8 px from the image border is at most one tenth of the zero flow's over the same pixels.

    Measured on the fp32 twin (seed 0): 0.01259 px against 2.501 px (float64, same code: 0.01260 px); whole image 0.119 px."""
    pair = onp.make_pair(144, 256)
    assert 0.1 < pair["disc"].mean() < 0.4 and pair["images0"].min() >= 0 and pair["images0"].max() <= 255
    flow = onp.optical_flow(pair["images0"], pair["images1"], levels=4, warps=5, iters=30)
    epe, zero = onp.interior_epe(flow, pair)
    print(f"fp32 twin: interior end-point error {epe:.5f} px, zero flow {zero:.4f} px")
    assert flow.dtype == np.float32 and 2.0 < zero < 3.0 and epe <= 0.1 * zero
    exact = onp.optical_flow(pair["images0"], pair["images1"], levels=4, warps=5, iters=30, dtype=np.float64)
    assert exact.dtype == np.float64 and onp.interior_epe(exact, pair)[0] <= 0.1 * zero
