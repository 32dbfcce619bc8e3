"""TEST INFRASTRUCTURE: how much a weight gradient of tests/torch_path.py cancels, and what a one-product fp16 backward does to it.

A weight gradient is a sum over points, dW = sum_p dpre_p (x) h_p, db = sum_p dpre_p.  Any per-product rounding error is bounded by
the sum of the absolute products,

    A_W = |dpre|^T |h|,   A_b = sum_p |dpre_p|,

and kappa = ||A||_1 / ||g||_1 says how much the sum cancels (1: every term has the same sign).  At seeded weights kappa is small;
on a batch a network has been trained on, the total gradient shrinks while the terms do not, and kappa grows.

``LinHook`` replaces ``torch_path._lin`` (every linear layer of the torch expression, the unfolded ``*_xyz_encoding_final``
included) by a node whose backward is the same algebra and, in float64, adds each call's A into ``hook.A``.  Options:

* ``emulate=True``: the backward of a one-product fp16 kernel -- dpre, h and W rounded to fp16, dpre and h with a power of two
  per point so that nothing underflows (the per-point block floating point of the data-gradient chain), products accumulated in
  float64.  Data gradients (dpre W) and weight gradients (dpre^T h) both take the rounded operands.
* ``drop=f``: a planted defect -- in every call, the points with the smallest max |dpre_p| whose share of that call's ||A_W||_1
  adds up to f are left out of dW and db (not out of the data gradient): what an underflowing scale at the hand-off from the
  data-gradient chain to the weight-gradient GEMM does.
"""
import torch
import torch.nn.functional as F

import torch_path

U16 = 2.0 ** -11                     # fp16 unit roundoff


def round16_rows(x):
    """x (P, n) float64 rounded to fp16 with a power of two per row that brings the row's largest magnitude to [1, 2)."""
    m = x.abs().amax(1, keepdim=True)
    e = torch.where(m > 0, torch.floor(torch.log2(torch.where(m > 0, m, torch.ones_like(m)))), torch.zeros_like(m))
    s = torch.exp2(-e)
    return (x * s).half().double() / s


def round16(x):
    """x rounded to fp16 with one power of two for the whole tensor (weights: the largest magnitude to [1, 2))."""
    m = float(x.abs().max())
    s = 2.0 ** -torch.floor(torch.log2(torch.tensor(m))).item() if m > 0 else 1.0
    return (x * s).half().double() / s


class _Lin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, hook):
        ctx.save_for_backward(x, w)
        ctx.hook = hook
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, dpre):
        x, w = ctx.saved_tensors
        hook = ctx.hook
        d64, x64 = dpre.double(), x.double()
        a_w, a_b = d64.abs().t() @ x64.abs(), d64.abs().sum(0)
        acc = hook.A.get(id(w))
        hook.A[id(w)] = (a_w, a_b) if acc is None else (acc[0] + a_w, acc[1] + a_b)
        hook.calls += 1
        if hook.emulate:
            d_use, x_use, w_use = round16_rows(d64), round16_rows(x64), round16(w.double())
        else:
            d_use, x_use, w_use = dpre, x, w
        dx = (d_use @ w_use).to(x.dtype) if ctx.needs_input_grad[0] else None
        d_wt = d_use
        if hook.drop > 0:
            share = d64.abs().sum(1) * x64.abs().sum(1)          # point p's part of this call's ||A_W||_1
            order = torch.argsort(d64.abs().amax(1))
            cum = torch.cumsum(share[order], 0)
            gone = order[cum <= hook.drop * float(share.sum())]
            d_wt = d_use.clone()
            d_wt[gone] = 0
            hook.dropped += int(gone.numel())
        dw = (d_wt.t() @ x_use).to(w.dtype)
        db = d_wt.sum(0).to(w.dtype)
        return dx, dw, db, None


class LinHook:
    """``with LinHook() as hook: <torch_path evaluation and .backward()>``; then ``hook.A[id(weight)] = (A_W, A_b)`` (float64,
    accumulated over every call of the layer)."""

    def __init__(self, emulate=False, drop=0.0):
        self.emulate, self.drop = emulate, drop
        self.A, self.calls, self.dropped = {}, 0, 0
        self._old = None

    def _lin(self, mod, x):
        layer = mod[0] if isinstance(mod, torch.nn.Sequential) else mod
        return _Lin.apply(x, layer.weight, layer.bias, self)

    def __enter__(self):
        self._old = torch_path._lin
        torch_path._lin = self._lin
        return self

    def __exit__(self, *exc):
        torch_path._lin = self._old
        return False

    def named_A(self, named_params):
        """{name: float64 A tensor (CPU)} for every parameter of (name, tensor) pairs: a Linear's weight / bias get A_W / A_b, a
        parameter the hook never saw (embedding tables) gets |g| -- its own gradient, no cancellation to measure."""
        out = {}
        layer_of = {}
        for name, p in named_params:
            if name.endswith(".weight") and id(p) in self.A:
                layer_of[name.rsplit(".", 1)[0]] = self.A[id(p)]
        for name, p in named_params:
            layer, kind = name.rsplit(".", 1)
            if layer in layer_of:
                out[name] = layer_of[layer][0 if kind == "weight" else 1].detach().cpu()
            else:
                g = torch.zeros_like(p) if p.grad is None else p.grad
                out[name] = g.detach().double().abs().cpu()
        return out


def kappa(A, g64):
    """||A||_1 / ||g||_1 (inf where the gradient is exactly zero and A is not)."""
    a, g = float(A.sum()), float(g64.double().abs().sum())
    return a / g if g > 0 else (0.0 if a == 0 else float("inf"))
