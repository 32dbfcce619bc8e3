"""Host checks (no GPU) of the validation panels: the numpy restatement tests/panel_numpy.py against golden g27 (the reference's
own validation-panel statements, tests/golden/make_golden_panels.py), the integer form of the blend, nsff_val_panels' argument
validation (no launch) and the Python layer's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import panel_numpy as pn
from nsff_pl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 19, 33


@pytest.fixture(scope="module")
def g27():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g27_panels.npz")))


def case_inputs(g, i):
    tiles = int(g[f"c{i}/tiles"])
    kw = dict(pred=g["pred"][None], gt=g["gt"][None], depth=g[f"c{i}/depth"][None], ssim_loss=g["ssim_loss"][None],
              lut_depth=g["lut_depth"], lut_mask=g["lut_mask"])
    if tiles >= 6:
        kw.update(transient_alpha=g["transient_alpha"][None], static_rgb=g["static_rgb"][None], static_depth=g[f"c{i}/static_depth"][None])
    if tiles == 8:
        kw.update(mask=g[f"c{i}/mask"][None], disp=g[f"c{i}/disp"][None])
    return tiles, kw


def test_golden_covers_the_cases(g27):
    assert [int(g27[f"c{i}/tiles"]) for i in range(4)] == [3, 6, 8, 8]
    d = g27["c0/depth"]
    assert np.isnan(d).sum() == 30 and np.isposinf(d).sum() == 3 and np.isneginf(d).sum() == 3
    assert np.isnan(g27["c1/static_depth"]).sum() == 25
    assert np.unique(g27["c2/disp"]).size == 1 and 0 < g27["c2/mask"].mean() < 1
    assert not g27["c3/mask"].any()                                                            # no dynamic pixel
    assert g27["pred"].min() < 0 and g27["pred"].max() > 1 and g27["static_rgb"].min() < 0 and g27["static_rgb"].max() > 1
    assert all(g27[k].dtype == np.float32 for k in ("gt", "pred", "ssim_loss", "rmse_map", "ssim_map"))


@pytest.mark.parametrize("i", range(4))
def test_restatement_reproduces_the_reference_panels_exactly(g27, i):
    tiles, kw = case_inputs(g27, i)
    out = pn.panels(**kw)
    grid = out["grid_u8"][0]
    assert grid.shape == g27[f"c{i}/grid_u8"].shape == (-(-tiles // 3) * (H + 2) + 2, 3 * (W + 2) + 2, 3)
    for key, want in (("grid_u8", g27[f"c{i}/grid_u8"]), ("rmse_u8", g27["rmse_u8"]), ("ssim_u8", g27["ssim_u8"]),
                      ("rmse_blend_u8", g27["rmse_blend_u8"]), ("ssim_blend_u8", g27["ssim_blend_u8"])):
        got = out[key][0]
        bad = int((got != want).sum())
        print(f"case {i} {key}: {bad} of {got.size} bytes differ")
        assert got.dtype == np.uint8 and bad == 0, key                                        # no pixel excluded
    assert np.array_equal(pn.ssim_map(g27["ssim_loss"]), g27["ssim_map"])
    ulp = np.abs(pn.rmse_map(g27["gt"], g27["pred"]).view(np.int32).astype(np.int64) - g27["rmse_map"].view(np.int32))
    assert ulp.max() <= 1                                   # (torch's vectorised CPU sqrt; the index image above is equal everywhere)


def test_grid_layout_padding_and_unfilled_cells(g27):
    _, kw = case_inputs(g27, 2)
    grid = pn.panels(**kw)["grid_u8"][0]
    inside = np.zeros(grid.shape[:2], bool)
    for k in range(8):
        y, x = (k // 3) * (H + 2) + 2, (k % 3) * (W + 2) + 2
        inside[y:y + H, x:x + W] = True
    assert not grid[~inside].any() and not g27["c2/grid_u8"][~inside].any()                   # padding and the ninth cell
    assert np.array_equal(grid[2:2 + H, 2:2 + W], pn.float_u8(g27["gt"]))
    const = grid[2 * (H + 2) + 2:2 * (H + 2) + 2 + H, (W + 2) + 2:(W + 2) + 2 + W]             # the -disp tile: ma == mi, index 0
    assert (const == g27["lut_depth"][0]).all()
    ranges = pn.panels(**kw)["ranges"][0]
    assert ranges[2].tolist() == [-0.375, -0.375] and ranges[3, 1] <= 0 and ranges[4, 1] <= 0
    assert np.isnan(pn.panels(pred=kw["pred"], gt=kw["gt"])["ranges"][0, [0, 1, 2, 4]]).all()


def test_integer_blend_equals_the_rounded_formula_for_every_byte_pair():
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    want = pn.blend(a, b)
    assert np.array_equal(want, pn.blend_float(a, b, np.float32)) and np.array_equal(want, pn.blend_float(a, b, np.float64))
    assert want.max() == 255 and want[0, 0] == 2 and want[0, 1] == 3
    byte = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).numpy()              # ToTensor, then 255 x truncated
    assert np.array_equal((255 * byte).astype(np.uint8), np.arange(256))


def test_truncation_clamps_where_numpy_is_undefined():
    v = np.array([-3.0, -0.0, 0.999, 254.999, 255.0, 300.0, np.nan, np.inf, -np.inf], np.float32)
    assert pn.trunc_u8(v).tolist() == [0, 0, 0, 254, 255, 255, 0, 255, 0]


# ---- C ABI ----
_BUF = (C.c_double * 64)()                                  # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15
_ALL = _lib._PANEL_IN + _lib._PANEL_LUT + _lib._PANEL_OUT


def _args(**kw):
    a = _lib.ValPanelsArgs(n_frames=2, H=4, W=5, scratch=_P, scratch_bytes=1 << 20, **{n: _P for n in _ALL})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_abi_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_val_panels(C.byref(_args(**kw)), None)
    assert lib.nsff_val_panels(None, None) == -2
    none = lambda *names: {n: None for n in names}
    outs = [n for n in _lib._PANEL_OUT if n != "ranges"]
    for bad in (dict(pred=None),                                                              # grid_u8 (anything) without pred
                dict(pred=None, **none(*[n for n in outs if n != "grid_u8"])),
                dict(ssim_loss=None), dict(ssim_loss=None, ssim_blend_u8=None), dict(ssim_loss=None, ssim_u8=None),
                dict(gt=None), dict(gt=None, grid_u8=None), dict(gt=None, grid_u8=None, rmse_u8=None),
                dict(gt=None, grid_u8=None, rmse_blend_u8=None),                              # rmse_* / the grid without gt
                dict(depth=None),                                                             # the grid's third tile
                dict(transient_alpha=None), dict(static_rgb=None), dict(static_depth=None),   # a transient set given in part
                dict(transient_alpha=None, static_rgb=None), dict(static_rgb=None, static_depth=None),
                dict(ranges=None), dict(ranges=None, **none(*outs)),
                dict(H=0), dict(W=0), dict(H=-3), dict(n_frames=0), dict(n_frames=70000), dict(H=65536, W=32768),
                dict(scratch_bytes=8)):
        assert call(**bad) == -1, bad
    assert call(**none("gt", "depth", "static_depth", "transient_alpha", "static_rgb", "disp", "ssim_loss", *outs)) == -1   # no field
    assert call(scratch=None) == -2
    assert call(scratch=_P + 8) == -3 and call(pred=_P + 2) == -3 and call(mask=_P + 1) == -3 and call(ranges=_P + 2) == -3
    assert C.sizeof(_lib.ValPanelsArgs) == 16 + 17 * 8 + 8 + 8
    need = lib.nsff_val_panels_scratch_bytes
    assert need(0, 4, 5) == 0 and need(1, 0, 5) == 0 and need(1, 65536, 32768) == 0
    assert need(1, 1, 1) == 16 + 40 and need(3, 19, 33) == 16 + 3 * 40                        # 627 pixels: one workgroup a frame
    assert need(2, 37, 71) == 16 + 2 * 3 * 40 and need(5, 288, 512) == 32 + 5 * 144 * 40     # 2627 pixels: three; 147456: 144


def test_header_declares_the_symbols_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint nsff_val_panels\(const NsffValPanelsArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_val_panels_scratch_bytes\(int32_t n_frames, int32_t H, int32_t W\);", header)
    for sym in ("nsff_val_panels", "nsff_val_panels_scratch_bytes"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym)
    assert callable(_lib.val_panels) and callable(_lib.val_panels_scratch_bytes)
    assert "platform-defined" in header[header.index("NsffFrameFinishArgs;"):header.index("NsffValPanelsArgs;")]
    assert _lib.load().nsff_abi_version() == _lib.ABI_VERSION


def test_python_layer_refuses_cpu_tensors_small_ssim_frames_and_unknown_tags():
    import inspect
    import nsff_pl_amd as A
    from nsff_pl_amd import panels, training
    assert A.panels is panels and A.validation_panels is panels.validation_panels and A.error_blend is panels.error_blend
    assert _lib.panel_grid_shape(19, 33, 3) == (23, 107) and _lib.panel_grid_shape(19, 33, 7) == (65, 107)
    assert _lib.panel_grid_shape(1, 1, 8) == (11, 11)
    res = {"rgb_fine": torch.zeros(6 * 6, 3), "depth_fine": torch.zeros(6 * 6)}
    with pytest.raises(RuntimeError, match="GPU tensor"):
        panels.validation_panels(res, {"rgbs": torch.zeros(36, 3)}, (6, 6), output_transient=False)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        panels.error_blend(torch.zeros(6, 6, 3), torch.zeros(6, 6, 3))
    with pytest.raises(ValueError, match="kind"):
        panels.error_blend(torch.zeros(6, 6, 3), torch.zeros(6, 6, 3), kind="lpips")
    sig = inspect.signature(training.NSFFTrainer.validation_step)
    assert list(sig.parameters) == ["self", "batch", "panels"] and sig.parameters["panels"].default is None
