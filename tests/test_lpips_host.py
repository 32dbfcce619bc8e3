"""Host checks (no GPU) of the LPIPS metric: the new C-ABI entries are declared, exported and bound; the layer-size arithmetic
against torch's own conv2d / max_pool2d output shapes; the workspace size; the two state-dict spellings; the refusals that
happen before any launch; and the score table with and without its LPIPS row."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_torch as lt
from nsff_pl_amd import LPIPS, _lib, evaluate, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nsff_lpips_packed_bytes", "nsff_lpips_pack", "nsff_lpips_dims", "nsff_lpips_workspace_bytes", "nsff_lpips")
SIZES = (31, 32, 37, 83, 288, 512)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} is not declared in the header"
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym)
    assert "typedef struct NsffLpipsArgs" in header and "typedef struct NsffLpipsWeights" in header
    assert _lib.load().nsff_abi_version() == _lib.ABI_VERSION == 32
    assert re.search(r"#define NSFF_LPIPS_MIN_SIZE\s+31\b", header) and _lib.LPIPS_MIN_SIZE == 31
    assert C.sizeof(_lib.LpipsArgs) == 16 + 8 * 8 and C.sizeof(_lib.LpipsWeights) == 15 * 8


def _torch_dims(H, W):
    x = torch.zeros(1, 3, H, W)
    dims = []
    for l, (cin, cout, k, stride, pad) in enumerate(lt.CONV):
        if lt.POOL_BEFORE[l]:
            x = F.max_pool2d(x, 3, 2)
        x = F.conv2d(x, torch.zeros(cout, cin, k, k), stride=stride, padding=pad)
        dims.append(tuple(x.shape[2:]))
    return tuple(dims)


@pytest.mark.parametrize("H", SIZES)
def test_layer_sizes_match_torch(H):
    for W in SIZES:
        assert _lib.lpips_dims(H, W) == _torch_dims(H, W), (H, W)
    if H == 288:
        assert _lib.lpips_dims(288, 512) == ((71, 127), (35, 63), (17, 31), (17, 31), (17, 31))
    if H == 31:
        assert _lib.lpips_dims(31, 31) == ((7, 7), (3, 3), (1, 1), (1, 1), (1, 1))


def _align256(x):
    return (x + 255) // 256 * 256


def _workspace_bytes(n_frames, H, W):
    """What include/nsff_render.h promises room for: five taps and two pooled maps of 2F images, the five small maps of F frames,
    the reduction's counters and three 8-byte words per workgroup of 1024 pixels -- every region padded to 256 bytes."""
    dims = _torch_dims(H, W)
    pooled = [tuple((n - 3) // 2 + 1 for n in dims[i]) for i in range(2)]
    total = 0
    for (h, w), (_, cout, _, _, _) in zip(dims, lt.CONV):
        total += _align256(4 * 2 * n_frames * h * w * cout)
    for (h, w), (_, cout, _, _, _) in zip(pooled, lt.CONV[:2]):
        total += _align256(4 * 2 * n_frames * h * w * cout)
    total += _align256(4 * n_frames * sum(h * w for h, w in dims))
    blocks = (H * W + 1023) // 1024
    total += _align256((4 * n_frames + 15) // 16 * 16 + 8 * 3 * n_frames * blocks)
    return total


def test_workspace_and_packed_bytes():
    for n_frames, H, W in ((1, 31, 31), (1, 37, 83), (3, 96, 160), (1, 288, 512), (30, 288, 512)):
        assert _lib.lpips_workspace_bytes(n_frames, H, W) == _workspace_bytes(n_frames, H, W), (n_frames, H, W)
    for n_frames, H, W in ((0, 64, 64), (1, 30, 64), (1, 64, 30), (32768, 64, 64)):
        assert _lib.lpips_workspace_bytes(n_frames, H, W) == 0
    k_padded = [cin * k * k for cin, _, k, _, _ in lt.CONV]
    assert all(k % 32 == 0 for k in k_padded[1:])                 # whole k steps of 32 from the second layer on
    k_padded[0] = 11 * 36                                         # conv1: each kernel row's 33 (kx, c) and 3 zero rows
    floats = sum(cout * (kp + 2) for (_, cout, _, _, _), kp in zip(lt.CONV, k_padded))
    assert _lib.load().nsff_lpips_packed_bytes() == 4 * floats


def test_both_state_dict_spellings_give_the_same_tensors():
    w = lt.random_weights(5)
    a = LPIPS.from_state_dict(lt.lpips_state_dict(w))
    sd = lt.torchvision_state_dict(w)
    sd["classifier.1.weight"] = torch.zeros(1)                    # what a whole AlexNet carries besides
    b = LPIPS.from_state_dict(sd)
    want = w["conv_w"] + w["conv_b"] + w["lin"]
    assert len(a._tensors) == len(b._tensors) == 15
    for ta, tb, tw in zip(a._tensors, b._tensors, want):
        assert ta is tw and tb is tw


def test_a_missing_key_is_named():
    for make, gone in ((lt.lpips_state_dict, ("net.slice3.6.bias", "lin4.model.1.weight")),
                       (lt.torchvision_state_dict, ("features.8.weight",))):
        sd = make(lt.random_weights(5))
        for k in gone:
            del sd[k]
        with pytest.raises(KeyError) as e:
            LPIPS.from_state_dict(sd)
        for k in gone:
            assert k in str(e.value)
    w = lt.random_weights(5)
    w["conv_w"][2] = w["conv_w"][2][:, :100]
    with pytest.raises(ValueError, match="layer 2"):
        LPIPS(w["conv_w"], w["conv_b"], w["lin"])


class _NoLaunch:
    """Stands in for the loaded library's nsff_lpips / nsff_lpips_pack: a call means a refusal came too late."""

    def __init__(self, monkeypatch):
        self.calls = 0
        lib = _lib.load()
        for name in ("nsff_lpips", "nsff_lpips_pack"):
            monkeypatch.setattr(lib, name, self._called, raising=True)

    def _called(self, *a):
        self.calls += 1
        return 0


def test_refusals_come_before_any_launch(monkeypatch):
    spy = _NoLaunch(monkeypatch)
    model = LPIPS.from_state_dict(lt.lpips_state_dict(lt.random_weights(5)))
    img = torch.rand(40, 40, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):         # CPU tensors: no CPU fallback
        metrics.lpips(model, img, img)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        model(img.permute(2, 0, 1)[None], img.permute(2, 0, 1)[None], normalize=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        metrics.lpips_frames(model, img[None], img[None])
    with pytest.raises(ValueError, match="31 x 31"):              # too small, by name
        _lib.lpips_dims(30, 64)
    with pytest.raises(ValueError, match="31 x 31"):
        _lib.lpips_dims(64, 7)
    assert spy.calls == 0


def test_c_entry_validates_without_launching():
    """nsff_lpips returns its error codes before touching the device (no GPU here: a launch would fail differently)."""
    lib = _lib.load()
    fake = 0x1000                                                 # a non-null, aligned address that is never dereferenced
    base = dict(n_frames=1, H=64, W=64, normalize=1, gt=fake, pred=fake, packed=fake, map=fake, workspace=fake,
                workspace_bytes=_lib.lpips_workspace_bytes(1, 64, 64))
    call = lambda **kw: lib.nsff_lpips(C.byref(_lib.LpipsArgs(**{**base, **kw})), None)
    assert lib.nsff_lpips(None, None) == -2
    assert call(H=30) == -1 and call(W=30) == -1 and call(n_frames=0) == -1 and call(n_frames=32768) == -1
    assert call(gt=None) == -2 and call(pred=None) == -2 and call(packed=None) == -2 and call(workspace=None) == -2
    assert call(map=None) == -1                                   # nothing to compute
    assert call(valid=fake) == -1                                 # a mask without sums
    assert call(workspace_bytes=base["workspace_bytes"] - 1) == -1
    assert call(workspace=fake + 4) == -3 and call(packed=fake + 4) == -3 and call(gt=fake + 2) == -3
    assert lib.nsff_lpips_pack(None, fake, None) == -2
    assert lib.nsff_lpips_pack(C.byref(_lib.LpipsWeights()), fake, None) == -2
    hw = (C.c_int32 * 10)()
    assert lib.nsff_lpips_dims(30, 64, hw) == -1 and lib.nsff_lpips_dims(64, 64, None) == -2


def test_mismatched_shapes_and_3x3_are_refused(monkeypatch):
    spy = _NoLaunch(monkeypatch)
    model = LPIPS.from_state_dict(lt.lpips_state_dict(lt.random_weights(5)))
    with pytest.raises(RuntimeError, match="one shape"):
        model(torch.rand(1, 3, 40, 40), torch.rand(1, 3, 40, 41))
    with pytest.raises(RuntimeError, match="one shape"):
        metrics.lpips(model, torch.rand(40, 40, 3), torch.rand(40, 48, 3))
    with pytest.raises(RuntimeError, match=r"\(H, W, 3\)"):
        metrics.lpips(model, torch.rand(3, 40, 40), torch.rand(3, 40, 40))
    with pytest.raises(RuntimeError, match="alike"):              # (F, 3, H, 3): channels-first and channels-last at once
        model(torch.rand(2, 3, 40, 3), torch.rand(2, 3, 40, 3))
    with pytest.raises(RuntimeError, match="size 3"):
        model(torch.rand(2, 4, 40, 40), torch.rand(2, 4, 40, 40))
    with pytest.raises(ValueError, match="31 x 31"):              # too small, whatever the device
        model(torch.rand(1, 3, 30, 40), torch.rand(1, 3, 30, 40))
    with pytest.raises(ValueError, match="31 x 31"):
        metrics.lpips(model, torch.rand(64, 30, 3), torch.rand(64, 30, 3))
    assert spy.calls == 0


def test_format_scores_with_and_without_the_lpips_row():
    p, s, l = np.array([30.12346, 25.5]), np.array([0.96721, 0.93214]), np.array([0.06141, 0.12345])
    four = evaluate.format_scores(p, s)
    assert four == ['Score \t Whole image  \t Dynamic only', '-------------------------------------',
                    'PSNR  \t 30.1235 \t 25.5000', 'SSIM  \t 0.9672 \t 0.9321']
    assert evaluate.format_scores(p, s, None) == four
    five = evaluate.format_scores(p, s, l)
    assert five[:4] == four and five[4] == 'LPIPS \t 0.0614 \t 0.1235' and len(five) == 5
    assert evaluate.format_scores(p, s, mean_lpips=l) == five


def test_sequence_scores_without_a_model_is_unchanged(tmp_path):
    scores = evaluate.SequenceScores()
    assert scores.lpips_model is None and len(scores) == 0
    assert scores.psnrs.shape == (0, 2) and scores.ssims.shape == (0, 2)
    with pytest.raises(AttributeError):
        scores.lpipss
    scores._rows.append(torch.tensor([30.0, 25.0, 0.9, 0.8]))
    assert len(scores.means()) == 2 and len(scores.table()) == 4
    scores.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["psnr.npy", "ssim.npy"]
