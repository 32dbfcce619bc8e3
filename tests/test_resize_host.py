"""Host checks (no GPU) of the frame resize: the numpy restatement tests/resize_numpy.py against golden g28 (the reference's own
two PIL statements, tests/golden/make_golden_resize.py) and, where PIL imports, against Pillow directly; nsff_resize_table
against the restatement's tables, entry for entry; the scale limit; scaled_intrinsics; nsff_frame_resize's argument validation
(no launch) and the Python layer's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import resize_numpy as rn
from nsff_pl_amd import _lib, frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((45, 80, 19, 33), (23, 40, 31, 57), (19, 70, 19, 33), (40, 33, 19, 33), (19, 33, 19, 33), (96, 160, 12, 20),
          (150, 530, 70, 261))                                                    # h, w -> H, W of the golden cases
SWEEP = sorted({(40, 19), (128, 51), (1280, 512), (720, 288), (3840, 512), (8, 1), (1, 8), (1, 1), (7, 7)}
               | {(n_in, n_out) for n_in in (1, 2, 3, 5, 8, 13, 21, 34, 37, 55) for n_out in (1, 2, 3, 4, 7, 11, 19, 33, 57)})


@pytest.fixture(scope="module")
def g28():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g28_resize.npz")))


def test_golden_covers_the_cases(g28):
    assert int(g28["n_cases"]) == len(SHAPES)
    for i, (h, w, H, W) in enumerate(SHAPES):
        F = 1 if i == 6 else 2
        assert g28[f"c{i}/src"].shape == (F, h, w, 3) and g28[f"c{i}/dst"].shape == (F, H, W, 3)
        assert g28[f"c{i}/mask_src"].shape == (F, h, w) and g28[f"c{i}/mask_dst"].shape == (F, H, W)
    assert rn.lanczos_ksize(96, 12) == rn.lanczos_ksize(160, 20) == 49
    pat = g28["c0/src"][1]
    assert set(np.unique(pat)) == {0, 255} and len(np.unique(g28["c0/src"][0])) > 200
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g28_resize.npz")) < 500_000


def _unclipped_range(img, img_wh):
    """(min, max) of acc >> 22 over both passes of the restatement, before the clip"""
    W, H = img_wh
    lo, hi = 0, 255
    x = img.astype(np.int64)
    for axis, n_out in ((1, W), (0, H)):
        if x.shape[axis] == n_out:
            continue
        start, count, weights = rn.lanczos_table(x.shape[axis], n_out)
        src = np.moveaxis(x, axis, 0)
        acc = np.stack([(1 << 21) + np.tensordot(weights[i, :count[i]].astype(np.int64), src[start[i]:start[i] + count[i]], axes=(0, 0))
                        for i in range(n_out)]) >> 22
        lo, hi = min(lo, int(acc.min())), max(hi, int(acc.max()))
        x = np.moveaxis(np.clip(acc, 0, 255), 0, axis)
    return lo, hi


def test_both_clips_fire_on_the_pattern_frames(g28):
    lo, hi = _unclipped_range(g28["c0/src"][1], (33, 19))
    assert lo < 0 and hi > 255


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_restatement_reproduces_the_reference_bytes(g28, i):
    h, w, H, W = SHAPES[i]
    got = rn.resize_lanczos(g28[f"c{i}/src"], (W, H))
    bad = int((got != g28[f"c{i}/dst"]).sum())
    print(f"case {i} lanczos: {bad} of {got.size} bytes differ")
    assert got.dtype == np.uint8 and got.shape == g28[f"c{i}/dst"].shape and bad == 0
    got = rn.resize_nearest_pil(g28[f"c{i}/mask_src"], (W, H))
    bad = int((got != g28[f"c{i}/mask_dst"]).sum())
    print(f"case {i} nearest: {bad} of {got.size} bytes differ")
    assert got.dtype == np.uint8 and bad == 0


def _same_tables(filt, n_in, n_out):
    want, got = rn.table(filt, n_in, n_out), _lib.resize_table(filt, n_in, n_out)
    assert _lib.resize_ksize(filt, n_in, n_out) == (1 if want[2] is None else want[2].shape[1])
    for name, a, b in zip(("start", "count", "weights"), want, got):
        if a is None:
            assert b is None
            continue
        b = b.numpy()
        assert a.dtype == b.dtype and a.shape == b.shape, (filt, n_in, n_out, name)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (filt, n_in, n_out, name)       # fp32 weights by their bits


@pytest.mark.parametrize("filt", range(4))
def test_c_tables_equal_the_restatement_exactly(filt):
    pairs = sorted({(h, H) for h, _, H, _ in SHAPES} | {(w, W) for _, w, _, W in SHAPES} | set(SWEEP))
    n = 0
    for n_in, n_out in pairs:
        if filt == rn.LANCZOS_U8 and rn.lanczos_ksize(n_in, n_out) > rn.MAX_KSIZE:
            assert _lib.resize_ksize(filt, n_in, n_out) == _lib.ERR_UNSUPPORTED     # (only downscales beyond 8x)
            assert n_in > 8 * n_out
            continue
        _same_tables(filt, n_in, n_out)
        n += 1
    assert (40, 19) in pairs and (128, 51) in pairs and n >= 90


def test_tables_have_the_stated_properties():
    assert rn.nearest_pil_table(40, 19)[0].tolist() != [int((i + 0.5) * (40 / 19)) for i in range(19)]      # the running sum
    assert rn.nearest_pil_table(128, 51)[0].tolist() != [int((i + 0.5) * (128 / 51)) for i in range(51)]
    assert rn.nearest_cv_table(10, 5)[0].tolist() == [0, 2, 4, 6, 8]
    s, c, w = rn.lanczos_table(80, 33)
    assert w.shape == (33, rn.lanczos_ksize(80, 33)) == (33, 2 * 8 + 1) and (s >= 0).all() and (s + c <= 80).all()
    assert all(not w[i, c[i]:].any() for i in range(33)) and np.abs(w.sum(1) - (1 << 22)).max() <= 17   # rounded per tap
    s, c, w = rn.linear_cv_table(5, 11)
    assert s[0] == 0 and w[0].tolist() == [1.0, 0.0] and s[-1] == 4 and c[-1] == 1 and w[-1].tolist() == [1.0, 0.0]
    assert rn.lanczos_ksize(23, 31) == 7 and rn.lanczos_ksize(3840, 512) == 47


def test_a_table_wider_than_49_taps_is_refused():
    lib = _lib.load()
    assert _lib.RESIZE_MAX_KSIZE == rn.MAX_KSIZE == 2 * 24 + 1
    assert rn.lanczos_ksize(97, 12) == 51 and _lib.resize_ksize(_lib.RESIZE_LANCZOS_U8, 97, 12) == _lib.ERR_UNSUPPORTED == -5
    assert _lib.resize_ksize(_lib.RESIZE_LANCZOS_U8, 96, 12) == 49
    buf = (C.c_int32 * 4096)()
    assert lib.nsff_resize_table(_lib.RESIZE_LANCZOS_U8, 97, 12, buf, buf, buf) == -5
    with pytest.raises(RuntimeError, match="8x"):
        _lib.resize_table(_lib.RESIZE_LANCZOS_U8, 97, 12)
    assert _lib.resize_ksize(_lib.RESIZE_NEAREST_PIL, 9700, 12) == 1 and _lib.resize_ksize(_lib.RESIZE_LINEAR_CV, 9700, 12) == 2
    assert _lib.resize_ksize(7, 10, 10) == -1 and _lib.resize_ksize(0, 0, 10) == -1 and _lib.resize_ksize(0, 10, 0) == -1
    assert lib.nsff_resize_table(_lib.RESIZE_LANCZOS_U8, 10, 5, None, buf, buf) == -2
    assert lib.nsff_resize_table(_lib.RESIZE_LANCZOS_U8, 10, 5, buf, buf, None) == -2
    assert lib.nsff_resize_table(_lib.RESIZE_NEAREST_CV, 10, 5, buf, buf, None) == 0


def test_scaled_intrinsics_is_the_reference_rule():
    for f, src, dst in ((1111.1, (1280, 720), (512, 288)), (523.7, (45, 80), (33, 19)), (800.0, (640, 480), (640, 480))):
        K = frames.scaled_intrinsics(f, src, dst)
        assert K.dtype == torch.float32 and np.array_equal(K.numpy(), rn.scaled_intrinsics(f, src, dst))
    K0 = np.array([[900.0, 0, 640], [0, 900.0, 360], [0, 0, 1]], np.float32)
    want = K0.copy()
    want[0] *= 512 / 1280
    want[1] *= 288 / 720
    assert np.array_equal(frames.scaled_intrinsics(K0, (1280, 720), (512, 288)).numpy(), want)
    assert np.array_equal(frames.scaled_intrinsics(torch.tensor(K0), (1280, 720), (512, 288)).numpy(), want)
    with pytest.raises(ValueError, match="3,3"):
        frames.scaled_intrinsics(np.zeros((3, 4)), (4, 4), (2, 2))
    with pytest.raises(ValueError, match="img_wh"):
        frames.scaled_intrinsics(1.0, (4, 4), (0, 2))


# ---- C ABI ----
_BUF = (C.c_double * 64)()                                  # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15
_PTRS = ("src", "dst", "x_start", "x_count", "x_weights", "y_start", "y_count", "y_weights")


def _args(filt=0, **kw):
    a = _lib.FrameResizeArgs(n_frames=2, filter=filt, channels=2 if filt == 3 else 1, src_h=45, src_w=80, dst_h=19, dst_w=33,
                             **{n: _P for n in _PTRS})
    a.ksize_x, a.ksize_y = _lib.resize_ksize(filt, 80, 33), _lib.resize_ksize(filt, 45, 19)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_abi_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda filt=0, **kw: lib.nsff_frame_resize(C.byref(_args(filt, **kw)), None)
    assert lib.nsff_frame_resize(None, None) == -2
    for filt in range(4):
        for bad in (dict(filter=4), dict(filter=-1), dict(n_frames=0), dict(n_frames=70000), dict(src_h=0), dict(src_w=-1),
                    dict(dst_h=0), dict(dst_w=0), dict(channels=0), dict(channels=4), dict(src_h=65536, src_w=32768),
                    dict(ksize_x=3), dict(ksize_y=5)):
            assert call(filt, **bad) == -1, (filt, bad)
        for name in ("src", "dst", "x_start", "y_start"):
            assert call(filt, **{name: None}) == -2, (filt, name)
        assert call(filt, x_start=_P + 2) == -3 and call(filt, y_weights=_P + 1) == -3
    for filt in (0, 3):
        for name in ("x_count", "y_count", "x_weights", "y_weights"):
            assert call(filt, **{name: None}) == -2, (filt, name)
    assert call(3, channels=3) == -1                                              # the bilinear kernel carries two ratios
    assert call(2, src=_P + 2) == -3 and call(3, dst=_P + 1) == -3                # fp32 images; bytes need no alignment
    assert call(0, src_h=97, dst_h=12, ksize_y=51) == -5 and call(0, src_w=400, dst_w=33, ksize_x=75) == -5
    assert C.sizeof(_lib.FrameResizeArgs) == 4 * 4 + 4 * 4 + 2 * 4 + 2 * 4 + 8 * 8


def test_header_declares_the_symbols_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint nsff_frame_resize\(const NsffFrameResizeArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint nsff_resize_ksize\(int32_t filter, int32_t n_in, int32_t n_out\);", header)
    assert re.search(r"\bint nsff_resize_table\(int32_t filter, int32_t n_in, int32_t n_out, int32_t\* start, int32_t\* count, "
                     r"void\* weights\);", header)
    for sym in ("nsff_frame_resize", "nsff_resize_ksize", "nsff_resize_table"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym)
    for name, value in (("LANCZOS_U8", 0), ("NEAREST_PIL", 1), ("NEAREST_CV", 2), ("LINEAR_CV", 3), ("MAX_KSIZE", 49)):
        assert re.search(rf"#define NSFF_RESIZE_{name}\s+{value}\b", header) and getattr(_lib, f"RESIZE_{name}") == value
    assert re.search(r"#define NSFF_ERR_UNSUPPORTED\s+-5\b", header)
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header)
    assert _lib.load().nsff_abi_version() == _lib.ABI_VERSION == 32


def test_python_layer_refuses_by_name():
    import inspect
    import nsff_pl_amd as A
    from nsff_pl_amd import sampling
    for name in ("resize_images", "resize_masks", "resize_disps", "resize_flows", "resize_frames", "scaled_intrinsics"):
        assert getattr(A, name) is getattr(frames, name) and name in A.__all__
    with pytest.raises(RuntimeError, match="resize_images: images must be a GPU tensor"):
        frames.resize_images(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(RuntimeError, match="resize_disps: disps must be a GPU tensor"):
        frames.resize_disps([torch.zeros(8, 8)], (4, 4))
    with pytest.raises(TypeError, match="resize_masks: masks must be a tensor"):
        frames.resize_masks(np.zeros((1, 8, 8), np.uint8), (4, 4))
    with pytest.raises(ValueError, match="img_wh"):
        frames.resize_images(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 0))
    with pytest.raises(ValueError, match="img_wh"):
        frames.resize_frames(None, None, None)
    assert frames.resize_flows(None, (4, 4)) is None and frames.resize_flows([None, None], (4, 4)) is None
    sig = inspect.signature(sampling.RayBank.from_frames)
    assert sig.parameters["resize"].default is False and list(sig.parameters)[-1] == "resize"
    assert list(inspect.signature(frames.resize_frames).parameters) == ["images", "disps", "masks", "flows_fw", "flows_bw", "img_wh"]


def test_restatement_equals_pillow_on_the_sweep():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(28)
    for (h, H), (w, W) in zip(SWEEP, SWEEP[::-1]):
        if max(rn.lanczos_ksize(h, H), rn.lanczos_ksize(w, W)) > rn.MAX_KSIZE:
            continue
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if (h + w) % 2:
            img = (img > 127).astype(np.uint8) * 255
        assert np.array_equal(rn.resize_lanczos(img, (W, H)), np.asarray(Image.fromarray(img).resize((W, H), Image.LANCZOS))), (h, w, H, W)
        mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
        assert np.array_equal(rn.resize_nearest_pil(mask[None], (W, H))[0],
                              np.asarray(Image.fromarray(mask).resize((W, H), Image.NEAREST))), (h, w, H, W)
    one = np.arange(139, dtype=np.uint8)[None]
    for n_in in range(1, 140):
        for n_out in range(1, 70):
            got = np.asarray(Image.fromarray(one[:, :n_in]).resize((n_out, 1), Image.NEAREST))[0]
            assert np.array_equal(got, one[0, rn.nearest_pil_table(n_in, n_out)[0]]), (n_in, n_out)
