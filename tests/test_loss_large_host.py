"""Host side of the fused loss above 4096 rays (csrc/loss.hip: nsff_nerfw_loss_ex): symbols, workspace arithmetic, argument
refusal, the dispatch rule of fused_loss, and the numpy restatement of the selection rule the GPU tests hold both device paths to."""
import ctypes as C

import numpy as np
import pytest
import torch

import scenes
import select_rule
from nsff_pl_amd import _lib, fused_loss
from nsff_pl_amd.losses import NeRFWLoss


def test_new_loss_symbols_are_exported_and_bound():
    lib = _lib.load()
    for sym in ("nsff_nerfw_loss_work_bytes", "nsff_nerfw_loss_ex", "nsff_last_loss_path"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert _lib.last_loss_path() in (0, 1, 2)
    assert fused_loss.MAX_RAYS == 4096 and fused_loss.MAX_RAYS_SELECT == _lib.LOSS_MAX_RAYS >= 262144
    assert fused_loss.TERMS == select_rule.TERMS


def test_workspace_bytes_are_positive_and_monotone_up_to_the_bound():
    bound = _lib.LOSS_MAX_RAYS
    sizes = [1, 2, 255, 256, 333, 1024, 1025, 4096, 4097, 8192, 65536, 65537, 262144, bound - 1, bound]
    got = [_lib.nerfw_loss_work_bytes(n) for n in sizes]
    assert all(b > 0 for b in got), got
    assert all(a <= b for a, b in zip(got, got[1:])), got
    assert got[-1] < 1 << 20                        # a few hundred KB at the bound
    for n in (bound + 1, 2 * bound, 0, -5):
        assert _lib.nerfw_loss_work_bytes(n) == 0, n


INVALID, NULL, ALIGN = -1, -2, -3            # NSFF_ERR_* (test_error_codes_are_the_header_s)


def _fake_args(n):
    """every pointer non-null but never dereferenced: the calls below must be refused before any launch"""
    a = _lib.LossArgs(n_rays=n, n_samples=64, n_keep=60, n_frames=30, max_t=29, topk=1.0, thickness=1)
    for name, typ in _lib.LossArgs._fields_:
        if typ is C.c_void_p:
            setattr(a, name, 4096)
    return a


@pytest.mark.parametrize("mode", [1, 2])
def test_loss_ex_refuses_a_missing_or_small_workspace_without_a_launch(mode):
    lib = _lib.load()
    n = 8192
    need = _lib.nerfw_loss_work_bytes(n)
    a = _fake_args(n)
    assert lib.nsff_nerfw_loss_ex(C.byref(a), mode, None, need, None) == NULL
    assert lib.nsff_nerfw_loss_ex(C.byref(a), mode, 1 << 20, need - 1, None) == INVALID
    assert lib.nsff_nerfw_loss_ex(C.byref(a), mode, 1 << 20, 0, None) == INVALID
    assert lib.nsff_nerfw_loss_ex(C.byref(a), mode, (1 << 20) + 4, need, None) == ALIGN
    assert lib.nsff_nerfw_loss_ex(None, mode, 1 << 20, need, None) == NULL
    for bad in (0, _lib.LOSS_MAX_RAYS + 1):
        assert lib.nsff_nerfw_loss_ex(C.byref(_fake_args(bad)), mode, 1 << 20, 1 << 30, None) == INVALID
    # nsff_nerfw_loss keeps its own bound
    assert lib.nsff_nerfw_loss(C.byref(_fake_args(4097)), mode, None) == INVALID
    assert _lib.last_loss_path() == 0 or torch.cuda.is_available()      # nothing above launched anything


def test_error_codes_are_the_header_s():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsff_render.h")).read()
    codes = dict(re.findall(r"#define\s+(NSFF_ERR_[A-Z]+)\s+\(?(-?\d+)\)?", header))
    assert (int(codes["NSFF_ERR_INVALID"]), int(codes["NSFF_ERR_NULL"]), int(codes["NSFF_ERR_ALIGN"])) == (INVALID, NULL, ALIGN), codes
    assert int(re.search(r"#define\s+NSFF_LOSS_MAX_RAYS\s+(\d+)", header).group(1)) == _lib.LOSS_MAX_RAYS


@pytest.mark.parametrize("n", [16, 4096, 4097, 8192])
def test_fused_loss_is_not_applicable_to_cpu_tensors(n, monkeypatch):
    monkeypatch.delenv("NSFF_FUSED_LOSS", raising=False)
    loss = NeRFWLoss()
    ts = select_rule.synthetic_ts(n, scenes.N_FRAMES, 1)
    render = select_rule.synthetic_render(n, 4, 1)
    targets = scenes.synthetic_targets(n, ts, 1)
    for mode in (None, "radix", "rank"):
        if mode is None:
            monkeypatch.delenv("NSFF_LOSS_SELECT", raising=False)
        else:
            monkeypatch.setenv("NSFF_LOSS_SELECT", mode)
        assert fused_loss.applicable(loss, render, targets, dict(output_transient_flow=["fw", "bw", "disocc"])) is False


def test_select_path_follows_the_size_and_the_override(monkeypatch):
    monkeypatch.delenv("NSFF_LOSS_SELECT", raising=False)
    assert [fused_loss.select_path(n) for n in (0, 1, 4096, 4097, 262144, fused_loss.MAX_RAYS_SELECT, fused_loss.MAX_RAYS_SELECT + 1)] == \
        [None, "rank", "rank", "radix", "radix", "radix", None]
    monkeypatch.setenv("NSFF_LOSS_SELECT", "radix")
    assert [fused_loss.select_path(n) for n in (1, 4096, 4097)] == ["radix"] * 3
    monkeypatch.setenv("NSFF_LOSS_SELECT", "rank")
    assert [fused_loss.select_path(n) for n in (1, 4096, 4097, 65536)] == ["rank", "rank", None, None]
    monkeypatch.setenv("NSFF_LOSS_SELECT", "quick")
    with pytest.raises(ValueError):
        fused_loss.select_path(16)


@pytest.mark.parametrize("n", [1, 2, 7, 256, 333, 4097])
def test_numpy_selection_rule_equals_torch_on_tie_free_data(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    assert len(set(x.tolist())) == n
    val, idx = select_rule.median(x.numpy())
    assert val == float(torch.median(x)) and x[idx] == val
    for topk in (0.05, 0.3, 0.5, 0.7, 0.999, 1.0):
        v = torch.rand(n, generator=g)
        sel, K, M = select_rule.select(v.numpy(), topk)
        assert M == n and K == (n if topk >= 1 else int(topk * n)) == int(sel.sum())
        if K:
            top, at = torch.topk(v, K)
            assert sorted(np.flatnonzero(sel).tolist()) == sorted(at.tolist())
            coef, term = select_rule.reduce_term(v.numpy(), topk)
            assert abs(term - float(top.double().mean())) <= 1e-12
            assert np.array_equal(coef != 0, sel) and np.all(coef[sel] == np.float32(1) / np.float32(K))
        else:
            assert not sel.any() and select_rule.reduce_term(v.numpy(), topk)[1] == 0.0
        # a masked population: negative entries are outside it
        vm = torch.where(torch.rand(n, generator=g) < 0.4, torch.full((n,), -1.0), v)
        sel, K, M = select_rule.select(vm.numpy(), topk, masked=True)
        inside = vm[vm >= 0]
        assert M == inside.numel() and K == (M if topk >= 1 else int(topk * M)) == int(sel.sum())
        if K:
            assert np.allclose(np.sort(vm.numpy()[sel]), np.sort(torch.topk(inside, K)[0].numpy()), rtol=0, atol=0)


def test_numpy_selection_rule_breaks_ties_by_the_lower_index():
    v = np.array([1.0, 3.0, 3.0, 0.5, 3.0, 3.0, 2.0], np.float32)
    sel, K, M = select_rule.select(v, 3 / 7 + 1e-9)
    assert (K, M) == (3, 7) and np.flatnonzero(sel).tolist() == [1, 2, 4]
    assert select_rule.median(np.array([2.0, 1.0, 2.0, 2.0, 3.0], np.float32)) == (2.0, 2)       # ranks: 1, 0, 2 <- , 3, 4
    assert select_rule.median(np.full(6, 7.0, np.float32)) == (7.0, 2)
    vm = np.array([-1.0, 5.0, 5.0, -1.0, 5.0], np.float32)
    sel, K, M = select_rule.select(vm, 0.7, masked=True)
    assert (K, M) == (2, 3) and np.flatnonzero(sel).tolist() == [1, 2]
