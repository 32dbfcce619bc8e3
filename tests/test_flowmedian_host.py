"""CPU checks of the flow-median layer: the C ABI of csrc/flowmedian.hip (declared, exported, bound; argument validation without a
launch), the Python layer's refusals, the twin tests/flowmedian_numpy.py on cases worked out by hand, and the method conditions --
the guided median sharpens the flow at a motion edge that is an image edge -- asked of the twin alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import flowmedian_numpy as fnp
import optflow_numpy as onp
from nsff_pl_amd import _lib, optflow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

_BUF = (C.c_double * 4096)()                                # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15


def _args(**kw):
    a = _lib.FlowMedianArgs(n_pairs=2, H=8, W=9, radius=7, sigma_i=12.75, sigma_s=7.0, tiled=1, flow=_P, grey=_P + 4, valid=_P + 1,
                            out=_P + 2 * 8 * 9 * 8)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_header_declares_the_symbol_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint\s+nsff_flow_median\(const NsffFlowMedianArgs\* args, void\* stream\);", header)
    lib = _lib.load()
    assert "nsff_flow_median" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "nsff_flow_median") and callable(_lib.flow_median)
    assert re.search(rf"#define NSFF_FLOW_MEDIAN_MAX_RADIUS\s+{_lib.FLOW_MEDIAN_MAX_RADIUS}\b", header) and _lib.FLOW_MEDIAN_MAX_RADIUS == 7
    assert re.search(rf"#define NSFF_FLOW_MEDIAN_TILED\s+{_lib.FLOW_MEDIAN_TILED}\b", header)
    assert optflow.DEFAULT_MEDIAN_TILED == bool(_lib.FLOW_MEDIAN_TILED) and optflow.MEDIAN_MAX_RADIUS == fnp.MAX_RADIUS == 7
    assert C.sizeof(_lib.FlowMedianArgs) == 4 * 4 + 4 * 4 + 4 * 8
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header) and lib.nsff_abi_version() == _lib.ABI_VERSION == 32
    makefile = open(os.path.join(ROOT, "nsff_pl_amd", "csrc", "Makefile")).read()
    assert re.search(r"\nflowmedian\.o:.*\n\t.*-ffp-contract=off -c flowmedian\.hip", makefile)
    for target in ("$(OUT):", "timing:", "variant:"):         # the object is on every link line
        rule = makefile[makefile.index("\n" + target):]
        assert "flowmedian.o" in rule[:rule.index("\n\n")], target
    import nsff_pl_amd
    assert nsff_pl_amd.refine_flow is optflow.refine_flow and "refine_flow" in nsff_pl_amd.__all__


def test_the_call_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_flow_median(C.byref(_args(**kw)), None)
    assert lib.nsff_flow_median(None, None) == -2
    for bad in (dict(n_pairs=0), dict(n_pairs=65536), dict(H=0), dict(W=0), dict(H=32769), dict(n_pairs=4, H=32768, W=32768),
                dict(radius=0), dict(radius=8), dict(radius=-1), dict(tiled=2), dict(tiled=-1), dict(sigma_i=0.0), dict(sigma_i=-1.0),
                dict(sigma_i=float("nan")), dict(sigma_i=float("inf")), dict(sigma_s=0.0), dict(sigma_s=float("nan")),
                dict(sigma_s=float("inf"))):
        assert call(**bad) == -1, bad
    assert call(flow=None) == -2 and call(grey=None) == -2 and call(out=None) == -2
    assert call(flow=_P + 4) == -3 and call(out=_P + 2 * 8 * 9 * 8 + 4) == -3 and call(grey=_P + 2) == -3
    # out on flow, and out overlapping flow's last / first pixel
    assert call(out=_P) == -1 and call(out=_P + 2 * 8 * 9 * 8 - 8) == -1 and call(flow=_P + 2 * 8 * 9 * 8 - 8 + 2 * 8 * 9 * 8) == -1
    assert call(valid=None, flow=None) == -2                  # valid is optional: the call gets as far as the pointers


def test_the_python_layer_rejects_bad_arguments_by_name():
    flows, grey = torch.zeros(2, 8, 9, 2), torch.zeros(2, 8, 9)
    for kw, what in ((dict(radius=0), "radius"), (dict(radius=8), "radius"), (dict(radius=2.0), "radius"), (dict(radius=True), "radius"),
                     (dict(sigma_i=0.0), "sigma_i"), (dict(sigma_i=float("nan")), "sigma_i"), (dict(sigma_s=-1.0), "sigma_s"),
                     (dict(sigma_s=float("inf")), "sigma_s"), (dict(sigma_s="7"), "sigma_s")):
        with pytest.raises(ValueError, match=f"refine_flow: {what}"):
            optflow.refine_flow(flows, grey, **kw)
    for bad, what in ((np.zeros((2, 8, 9, 2), F32), "flows: need a tensor"), (flows.double(), "flows: need"), (flows[..., 0], "flows: need"),
                      (torch.zeros(2, 2, 8, 9), "flows: need"), (torch.zeros(0, 8, 9, 2), "flows: need"), (flows, "flows must be a GPU tensor")):
        with pytest.raises(RuntimeError, match=f"refine_flow: {what}"):
            optflow.refine_flow(bad, grey)
    with pytest.raises(ValueError, match="sequence_flows: refine must be"):
        optflow.sequence_flows(torch.zeros(3, 16, 16), refine=1)
    with pytest.raises(RuntimeError, match="flow_median: flow must be a GPU tensor"):
        _lib.flow_median(flows, grey, torch.zeros_like(flows))


def _uniform(vals):
    """A one-row flow whose u holds `vals` and whose v their negatives, with a constant guide and a wide sigma_s: all weights equal."""
    vals = np.asarray(vals, F32)
    flow = np.stack([vals, -vals], -1)[None, None]
    return flow, np.full((1, 1, len(vals)), 100, F32)


def test_twin_equal_weights_give_the_plain_lower_median():
    # sigma_s = 1e9: every spatial factor rounds to 1, the guide is constant: every weight 65535
    assert (fnp.spatial_table(7, 1e9) == 1).all()
    flow, grey = _uniform([5, 1, 4, 2, 3, 9])
    out = fnp.weighted_median(flow, grey, None, 7, 12.75, 1e9)
    assert (out[0, 0, :, 0] == 3).all()                      # six values: the lower of the two middle ones, 3 and 4
    assert (out[0, 0, :, 1] == -4).all()                     # ... and of the negatives -4 and -3
    flow, grey = _uniform([5, 1, 4, 2, 3])
    out = fnp.weighted_median(flow, grey, None, 7, 12.75, 1e9)
    assert (out[0, 0, :, 0] == 3).all() and (out[0, 0, :, 1] == -3).all()
    # radius 1 in a row: windows of three, of two at the ends (no replicated border): the lower of the two
    out = fnp.weighted_median(flow, grey, None, 1, 12.75, 1e9)
    assert out[0, 0, :, 0].tolist() == [1, 4, 2, 3, 2]


def test_twin_one_pixel_and_a_window_larger_than_the_image():
    one = np.array([[[[1.5, -2.5]]]], F32)
    assert (fnp.weighted_median(one, np.zeros((1, 1, 1), F32), None, 7) == one).all()
    assert (fnp.weighted_median(one, np.zeros((1, 1, 1), F32), np.zeros((1, 1, 1), np.uint8), 1) == one).all()
    rng = np.random.default_rng(0)
    flow = rng.normal(0, 2, (1, 3, 4, 2)).astype(F32)
    out = fnp.weighted_median(flow, np.zeros((1, 3, 4), F32), None, 7, 12.75, 1e9)       # every window is the whole image: 12 equal weights
    for c in range(2):
        assert (out[..., c] == np.sort(flow[..., c].ravel())[5]).all()


def test_twin_weights_by_hand():
    # three pixels in a row, radius 1, sigma_s = 1: s = 2 beside the centre; sigma_i = 10 with grey 0 | 10 | 30
    flow = np.array([[[[0, 0], [10, 10], [20, 20]]]], F32)
    grey = np.array([[[0, 10, 30]]], F32)
    out = fnp.weighted_median(flow, grey, None, 1, 10.0, 1.0)
    # centre pixel: weights 65535 / ((1 + 1) 2) = 16383.75 -> 16384, 65535, 65535 / ((1 + 4) 2) = 6553.5 -> 6554 (ties to even);
    # total 88473: the left one alone is short of half, left + centre reach it
    assert F32(65535) / F32(4) == F32(16383.75) and np.rint(F32(6553.5)) == 6554
    assert out[0, 0, 1].tolist() == [10, 10]
    # left pixel: itself 65535 against 16384: stays 0; right pixel: itself against 6554: stays 20
    assert out[0, 0, 0].tolist() == [0, 0] and out[0, 0, 2].tolist() == [20, 20]
    # an edge in the guide keeps a flow edge where the plain median moves it: five pixels, the middle one looks like the right side
    flow = np.array([[[[0, 0], [0, 0], [0, 0], [8, 8], [8, 8]]]], F32)
    grey = np.array([[[0, 0, 200, 200, 200]]], F32)
    assert fnp.weighted_median(flow, grey, None, 2, 12.75, 7.0)[0, 0, 2].tolist() == [8, 8]
    assert fnp.weighted_median(flow, grey, None, 2, 1e9, 7.0)[0, 0, 2].tolist() == [0, 0]


def test_twin_unknown_and_invalid_pixels():
    nan, inf = np.nan, np.inf
    flow = np.array([[[[1, 1], [1e10, 0], [3, 3], [nan, 2], [5, 5], [2, -inf], [7, 7]]]], F32)
    grey = np.full((1, 1, 7), 50, F32)
    out = fnp.weighted_median(flow, grey, None, 7, 12.75, 1e9)
    # the unknown centres are copied, bits unchanged
    for x in (1, 3, 5):
        assert out[0, 0, x].tobytes() == flow[0, 0, x].tobytes()
    # the known ones see 1, 3, 5, 7 with equal weights: the lower middle one
    for x in (0, 2, 4, 6):
        assert out[0, 0, x].tolist() == [3, 3]
    # valid == 0 takes a neighbour's vote, not the centre's own: with 1 and 3 invalid, pixel 0 sees {1, 5, 7} and pixel 4 {5, 7}
    valid = np.array([[[0, 1, 0, 1, 1, 1, 1]]], np.uint8)
    out = fnp.weighted_median(flow, grey, valid, 7, 12.75, 1e9)
    assert out[0, 0, 0].tolist() == [5, 5] and out[0, 0, 2].tolist() == [5, 5] and out[0, 0, 4].tolist() == [5, 5]
    assert out[0, 0, 6].tolist() == [5, 5]
    for x in (1, 3, 5):
        assert out[0, 0, x].tobytes() == flow[0, 0, x].tobytes()
    # everything else invalid: a pixel keeps its own flow
    out = fnp.weighted_median(flow, grey, np.zeros((1, 1, 7), np.uint8), 7, 12.75, 1e9)
    assert out.tobytes() == flow.tobytes()


def test_twin_ties_and_signed_zeros():
    flow, grey = _uniform([2, 2, 2, 1, 1, 3, 3])
    out = fnp.weighted_median(flow, grey, None, 7, 12.75, 1e9)
    assert (out[0, 0, :, 0] == 2).all() and (out[0, 0, :, 1] == -2).all()
    flow, grey = _uniform([1, 1, 3, 3])                      # two and two: the lower value reaches exactly half
    out = fnp.weighted_median(flow, grey, None, 7, 12.75, 1e9)
    assert (out[0, 0, :, 0] == 1).all() and (out[0, 0, :, 1] == -3).all()
    # -0 and +0 are one value: {-1, -0, +0, +0, 2}: the median is zero, of either sign
    flow = np.array([[[[-1, -1], [-0.0, 0.0], [0.0, -0.0], [0.0, 0.0], [2, 2]]]], F32)
    out = fnp.weighted_median(flow, np.full((1, 1, 5), 7, F32), None, 7, 12.75, 1e9)
    assert (out == 0).all()
    # {-0, +0, 1, 1}: -0 and +0 together are half; as two values neither would be
    flow = np.array([[[[0.0, 0.0], [-0.0, -0.0], [1, 1], [1, 1]]]], F32)
    out = fnp.weighted_median(flow, np.full((1, 1, 4), 7, F32), None, 7, 12.75, 1e9)
    assert (out == 0).all()


def test_contrast_pair_is_make_pair_with_an_image_edge():
    pair, plain = fnp.make_contrast_pair(48, 80, 3), onp.make_pair(48, 80, 3)
    assert (pair["disc"] == plain["disc"]).all() and (pair["flow"] == plain["flow"]).all() and (pair["rim"] == plain["rim"]).all()
    img = pair["images0"][0]
    assert img.dtype == np.float32 and img[pair["disc"]].min() >= 150 and img[pair["disc"]].max() <= 250
    assert img[~pair["disc"]].min() >= 30 and img[~pair["disc"]].max() <= 130
    # the same textures: inside the disc the two images are affine in each other
    a, b = img[pair["disc"]].astype(np.float64), plain["images0"][0][pair["disc"]].astype(np.float64)
    assert abs(np.corrcoef(a, b)[0, 1] - 1) < 1e-6


_CHAINS = {}


def _chain(seed):
    if seed not in _CHAINS:
        pair = fnp.make_contrast_pair(144, 256, seed)
        _CHAINS[seed] = (pair,) + fnp.chain(pair, levels=4, warps=5, iters=30)
    return _CHAINS[seed]


@pytest.mark.parametrize("seed", [0, 1])
def test_method_conditions_on_the_twin(seed):
    """fp32 twin, (144, 256), levels 4, warps 5, iters 30, radius 7.  Measured, rim / interior EPE in pixels:
    seed 0: unrefined 0.873 / 0.0177; with valid 0.116 / 0.0169; without valid 0.297; guide off (sigma_i = 1e9) 0.698
    seed 1: unrefined 0.945 / 0.0175; with valid 0.154 / 0.0167; without valid 0.392; guide off 0.744."""
    pair, fw, valid = _chain(seed)
    grey = pair["images0"]
    rim0, interior0, whole0 = fnp.rim_epe(fw, pair)
    rim_v, interior_v, whole_v = fnp.rim_epe(fnp.weighted_median(fw, grey, valid, 7), pair)
    rim_n, interior_n, whole_n = fnp.rim_epe(fnp.weighted_median(fw, grey, None, 7), pair)
    rim_g, interior_g, whole_g = fnp.rim_epe(fnp.weighted_median(fw, grey, valid, 7, sigma_i=1e9), pair)
    print(f"\nseed {seed}: rim / interior / whole EPE: unrefined {rim0:.4f} / {interior0:.4f} / {whole0:.4f}; with valid {rim_v:.4f} / "
          f"{interior_v:.4f} / {whole_v:.4f} ({rim_v / rim0:.3f} of the rim); without valid {rim_n:.4f} / {interior_n:.4f} / {whole_n:.4f} "
          f"({rim_n / rim0:.3f}); guide off {rim_g:.4f} / {interior_g:.4f} / {whole_g:.4f} ({rim_g / rim_v:.2f} x the guided rim)")
    assert rim_v <= 0.25 * rim0
    assert rim_n <= 0.5 * rim0
    assert interior_v <= interior0 and interior_n <= interior0
    assert rim_g >= 2 * rim_v
