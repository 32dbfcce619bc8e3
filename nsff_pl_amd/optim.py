"""The optimizer of the training step: ``torch.optim.Adam(lr, eps=1e-8, weight_decay)`` as
the reference's ``get_optimizer`` builds it (utils/__init__.py:45-47, train.py:140-146), run by ONE native launch pair
(``nsff_adam_step``, csrc/optim.hip) on flat buffers.

Every parameter becomes a view of one flat fp32 buffer, every ``.grad`` a view of a second one (the buffer the
weight-gradient kernel accumulates into and RCCL all-reduces); the two moment buffers are flat as well.  Step count and
learning rate live on the device, so the step is the same two launches eagerly and inside a hipGraph.  Parameters keep
their shapes, ``state_dict`` keys and identity (``nn.Parameter`` objects are untouched, only their storage moves).

Where this differs from ``torch.optim.Adam`` -- read before swapping it in elsewhere:

* **Parameters without a gradient.**  torch skips parameters whose ``.grad`` is None; here ``.grad`` always exists (a
  slice of the flat buffer, zero after ``zero_grad``).  With ``weight_decay == 0`` (the reference's default, opt.py:84)
  every element is updated every step: a zero gradient only decays the moments, as torch would for a zero-valued gradient.
  With ``weight_decay > 0`` a parameter that never receives a gradient (an unused head) must NOT be decayed, so the step
  runs in its segment form (``nsff_adam_step_segments``): a parameter tensor whose gradient slice is identically zero this
  step keeps its value and its moments, which is what torch does for ``grad is None``.  ``decay_unused=True`` selects the
  plain every-element step instead (one launch fewer).  Known deviation of that test: "unused" is decided from gradient VALUES,
  so a parameter whose true gradient is exactly zero everywhere (a dead ReLU layer, a fully masked loss) is skipped too,
  where torch -- which sees a zero-valued ``.grad`` tensor, not ``None`` -- would still decay it and its moments.
* **One step counter.**  The bias corrections use one global step count (``state[0]``), not torch's per-parameter counts: a
  tensor that receives its first gradient at step N is corrected as at step N, not as at step 1.  The two agree whenever
  every parameter is used from the first step on (the reference's training loop) or ``weight_decay == 0`` with gradients
  that start at step 1; ``load_torch_state_dict`` refuses per-parameter counts that differ.
* **HIP device only.**  There is no CPU implementation (tests drive CPU runs with a torch-op twin, tests/common.py).
* **Shared storage.**  ``module.state_dict()`` tensors are views of the one flat buffer: ``torch.save`` of such a dict
  writes the whole buffer once per file.  Use :func:`detached_state` (or ``NSFFTrainer.checkpoint``) to get clones.
* **Optimizer state.**  ``state_dict`` / ``load_state_dict`` use this class's flat layout; ``torch_state_dict`` /
  ``load_torch_state_dict`` convert to and from ``torch.optim.Adam``'s per-parameter format (resuming a reference /
  torch checkpoint, or handing a run back to torch).

:class:`FlatSGD` and :class:`FlatRAdam` (``--optimizer sgd`` / ``radam``, utils/__init__.py:42-50) sit on the same storage
(``_FlatOptimizer``) with native steps of their own (``nsff_sgd_step``, ``nsff_radam_step``); the points above hold for them
too, what differs is in their docstrings.  ``ranger`` is not offered (see ``NSFFTrainer``).
"""
import torch

from . import _lib


class _FlatOptimizer:
    """Storage and adoption shared by the flat optimizers: the flat parameter / gradient buffers, the views, the device
    learning rate and the segment bookkeeping.  A subclass adds its state buffers and its step."""

    def __init__(self, params, lr, weight_decay, decay_unused, n_state=4):
        name = type(self).__name__
        self.params = [p for p in params]
        if not self.params:
            raise ValueError(f"{name}: no parameters")
        self.decay_unused = bool(decay_unused)
        dev = self.params[0].device
        self._check_device(dev)
        if any(p.dtype != torch.float32 or p.device != dev for p in self.params):
            raise RuntimeError(f"{name}: parameters must be fp32 tensors on one device")
        self.weight_decay = float(weight_decay)
        self.numel = sum(p.numel() for p in self.params)
        self._padded = (self.numel + 3) // 4 * 4               # the kernels work on float4
        self.flat_param = torch.zeros(self._padded, device=dev)
        self.flat_grad = torch.zeros(self._padded, device=dev)
        self.state = torch.zeros(n_state, device=dev)          # [0] = steps taken
        self.lr = torch.tensor(float(lr), device=dev)
        # parameter tensor k = flat elements [seg_start[k], seg_start[k + 1]) -- the segment form of the step (see above)
        offs = [0]
        for p in self.params:
            offs.append(offs[-1] + p.numel())
        self.seg_start = torch.tensor(offs, dtype=torch.int64, device=dev)
        self.seg_used = torch.zeros(len(self.params), dtype=torch.int32, device=dev)
        self.param_groups = [{"lr": self.lr, "params": self.params}]   # (what loggers / schedulers look at)
        with torch.no_grad():
            off = 0
            for p in self.params:
                n = p.numel()
                self.flat_param[off:off + n].copy_(p.detach().reshape(-1))
                off += n
        self.adopt()

    @classmethod
    def _check_device(cls, dev):
        if dev.type != "cuda":
            raise RuntimeError(f"{cls.__name__} runs on the HIP device only (move the models first); there is no CPU path")

    def _segments(self):
        """(seg_start, seg_used) when this step runs in its segment form (weight decay on, ``decay_unused`` off), else Nones."""
        if self.weight_decay != 0 and not self.decay_unused:
            return self.seg_start, self.seg_used
        return None, None

    # -- storage ----------------------------------------------------------------------------------------------
    def adopt(self):
        """(Re-)point every parameter and gradient at its slice of the flat buffers (values are taken from the flat
        buffers; call :meth:`gather` first if the parameters were replaced from outside, e.g. by load_state_dict on
        re-created tensors)."""
        off = 0
        for p in self.params:
            n = p.numel()
            p.data = self.flat_param[off:off + n].view(p.shape)
            p.grad = self.flat_grad[off:off + n].view(p.shape)
            off += n

    def in_place(self):
        """True while every parameter and gradient still aliases its slice of the flat buffers."""
        base_p, base_g, off = self.flat_param.data_ptr(), self.flat_grad.data_ptr(), 0
        for p in self.params:
            g = p.grad
            if p.data_ptr() != base_p + 4 * off or g is None or g.data_ptr() != base_g + 4 * off:
                return False
            off += p.numel()
        return True

    def gather(self):
        """Copy the current parameter values into the flat buffer (after something re-created the tensors), re-adopt."""
        with torch.no_grad():
            off = 0
            for p in self.params:
                n = p.numel()
                if p.data_ptr() != self.flat_param.data_ptr() + 4 * off:
                    self.flat_param[off:off + n].copy_(p.detach().reshape(-1).to(self.flat_param.device))
                off += n
        self.adopt()

    # -- torch.optim surface --------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        self.flat_grad.zero_()

    def set_lr(self, lr):
        self.lr.fill_(float(lr))

    def _per_param(self, flat):
        """Clones of a flat state buffer's slices, one per parameter, in the parameters' shapes."""
        out, off = [], 0
        for p in self.params:
            n = p.numel()
            out.append(flat[off:off + n].view(p.shape).clone())
            off += n
        return out

    def _one_group(self, sd):
        """The single param group of a torch optimizer state dict over this parameter list, or ValueError."""
        groups = sd["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"{type(self).__name__} takes one parameter group")
        g = groups[0]
        if len(g["params"]) != len(self.params):
            raise ValueError(f"optimizer state covers {len(g['params'])} parameters, this optimizer has {len(self.params)}")
        return g

    def _load_per_param(self, sd, g, names, flats):
        """Copy the per-parameter tensors ``names`` of a torch state dict into the flat buffers ``flats`` (parameters without
        state keep zeros); returns the set of per-parameter step counts found."""
        steps = set()
        for flat in flats:
            flat.zero_()
        off = 0
        for key, p in zip(g["params"], self.params):
            n = p.numel()
            st = sd["state"].get(key)
            if st is not None:
                for name, flat in zip(names, flats):
                    if st.get(name) is None:            # (torch SGD: a parameter that has not stepped yet)
                        continue
                    if tuple(st[name].shape) != tuple(p.shape):
                        raise ValueError(f"state of parameter {key} has shape {tuple(st[name].shape)}, expected {tuple(p.shape)}")
                    flat[off:off + n].copy_(st[name].reshape(-1))
                if "step" in st:
                    steps.add(int(st["step"]))
            off += n
        if len(steps) > 1:
            raise ValueError(f"parameters are at different step counts {sorted(steps)}: one shared counter here")
        return steps


class FlatAdam(_FlatOptimizer):
    def __init__(self, params, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decay_unused=False):
        super().__init__(params, lr, weight_decay, decay_unused)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)

    def step(self):
        _lib.adam_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.state, self.lr,
                       self.betas[0], self.betas[1], self.eps, self.weight_decay, *self._segments())

    def reset_state(self):
        self.exp_avg.zero_(); self.exp_avg_sq.zero_(); self.state.zero_()

    def state_dict(self):
        return dict(step=self.state[0:1].clone(), lr=self.lr.clone(), exp_avg=self.exp_avg[:self.numel].clone(),
                    exp_avg_sq=self.exp_avg_sq[:self.numel].clone(), betas=self.betas, eps=self.eps,
                    weight_decay=self.weight_decay)

    def torch_state_dict(self):
        """The same state in ``torch.optim.Adam.state_dict()`` format (cloned tensors, parameter order of ``params``)."""
        state, off = {}, 0
        for i, p in enumerate(self.params):
            n = p.numel()
            state[i] = {"step": self.state[0].detach().clone().cpu(),
                        "exp_avg": self.exp_avg[off:off + n].view(p.shape).clone(),
                        "exp_avg_sq": self.exp_avg_sq[off:off + n].view(p.shape).clone()}
            off += n
        group = {"lr": float(self.lr), "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_torch_state_dict(self, sd):
        """Take over moments, step count and hyper-parameters of a ``torch.optim.Adam.state_dict()`` over the same
        parameters in the same order (one param group, no amsgrad).  Parameters without state keep zero moments."""
        groups = sd["param_groups"]
        if len(groups) != 1 or groups[0].get("amsgrad", False):
            raise ValueError("FlatAdam takes one parameter group without amsgrad")
        g = groups[0]
        if len(g["params"]) != len(self.params):
            raise ValueError(f"optimizer state covers {len(g['params'])} parameters, this optimizer has {len(self.params)}")
        steps = set()
        with torch.no_grad():
            self.exp_avg.zero_(); self.exp_avg_sq.zero_()
            off = 0
            for key, p in zip(g["params"], self.params):
                n = p.numel()
                st = sd["state"].get(key)
                if st is not None:
                    if tuple(st["exp_avg"].shape) != tuple(p.shape):
                        raise ValueError(f"state of parameter {key} has shape {tuple(st['exp_avg'].shape)}, expected {tuple(p.shape)}")
                    self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
                    self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                    steps.add(int(st["step"]))
                off += n
            if len(steps) > 1:
                raise ValueError(f"parameters are at different step counts {sorted(steps)}: one shared counter here")
            self.state.zero_(); self.state[0] = float(steps.pop()) if steps else 0.0
            self.lr.fill_(float(g["lr"]))
        self.betas, self.eps = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        self.weight_decay = float(g.get("weight_decay", 0.0))

    def load_state_dict(self, sd):
        with torch.no_grad():
            self.state.zero_(); self.state[0:1].copy_(sd["step"])
            self.lr.copy_(sd["lr"])
            self.exp_avg[:self.numel].copy_(sd["exp_avg"]); self.exp_avg_sq[:self.numel].copy_(sd["exp_avg_sq"])
        self.betas, self.eps, self.weight_decay = tuple(sd["betas"]), float(sd["eps"]), float(sd["weight_decay"])


class FlatSGD(_FlatOptimizer):
    """``torch.optim.SGD(lr, momentum, weight_decay)`` as the reference's ``get_optimizer`` builds it for ``--optimizer sgd``
    (utils/__init__.py:42-44: dampening 0, no Nesterov) in one native launch (``nsff_sgd_step``) on the flat buffers:
    ``g += wd p; buf = momentum buf + g; p -= lr buf``.  The momentum buffer starts at zero, which reproduces torch's
    first-step ``buf = grad`` exactly; with ``momentum == 0`` no buffer exists.  Parameters without a gradient, the HIP-only
    rule and the shared storage are as described for :class:`FlatAdam` above; ``state[0]`` counts the steps (torch's SGD keeps
    no count, so none is exported).  With ``weight_decay == 0`` and momentum a tensor whose gradient is zero this step still
    moves along its momentum buffer, where torch -- seeing ``grad is None`` -- would hold it; a tensor that never receives a
    gradient has a zero buffer and stays put either way."""

    def __init__(self, params, lr=5e-4, momentum=0.9, weight_decay=0.0, decay_unused=False):
        super().__init__(params, lr, weight_decay, decay_unused)
        self.momentum = float(momentum)
        self.momentum_buffer = torch.zeros_like(self.flat_param) if self.momentum != 0 else None

    def step(self):
        _lib.sgd_step(self.flat_param, self.flat_grad, self.momentum_buffer, self.state, self.lr, self.momentum,
                      self.weight_decay, *self._segments())

    def reset_state(self):
        self.state.zero_()
        if self.momentum_buffer is not None:
            self.momentum_buffer.zero_()

    def state_dict(self):
        buf = None if self.momentum_buffer is None else self.momentum_buffer[:self.numel].clone()
        return dict(step=self.state[0:1].clone(), lr=self.lr.clone(), momentum_buffer=buf, momentum=self.momentum,
                    weight_decay=self.weight_decay)

    def load_state_dict(self, sd):
        if (float(sd["momentum"]) != 0) != (self.momentum_buffer is not None):
            raise ValueError("FlatSGD: the state was saved with another kind of momentum (zero / non-zero)")
        with torch.no_grad():
            self.state.zero_(); self.state[0:1].copy_(sd["step"])
            self.lr.copy_(sd["lr"])
            if self.momentum_buffer is not None:
                self.momentum_buffer[:self.numel].copy_(sd["momentum_buffer"])
        self.momentum, self.weight_decay = float(sd["momentum"]), float(sd["weight_decay"])

    def torch_state_dict(self):
        """The same state in ``torch.optim.SGD.state_dict()`` format (cloned tensors, parameter order of ``params``).  Without
        momentum the per-parameter state is empty, as torch's is; a zero buffer (no step yet) continues in torch exactly as
        its own missing one would."""
        state = {}
        if self.momentum_buffer is not None:
            state = {i: {"momentum_buffer": b} for i, b in enumerate(self._per_param(self.momentum_buffer))}
        group = {"lr": float(self.lr), "momentum": self.momentum, "dampening": 0, "weight_decay": self.weight_decay,
                 "nesterov": False, "maximize": False, "foreach": None, "differentiable": False, "fused": None,
                 "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_torch_state_dict(self, sd):
        """Take over momentum buffers and hyper-parameters of a ``torch.optim.SGD.state_dict()`` over the same parameters in
        the same order (one param group, dampening 0, no Nesterov).  Parameters without a buffer start from zero, which is
        torch's own first step.  torch's SGD keeps no step count: the counter here restarts at zero."""
        g = self._one_group(sd)
        if g.get("dampening", 0) != 0 or g.get("nesterov", False) or g.get("maximize", False):
            raise ValueError("FlatSGD takes dampening 0 without Nesterov or maximize")
        momentum = float(g.get("momentum", 0.0))
        with torch.no_grad():
            if momentum != 0 and self.momentum_buffer is None:
                self.momentum_buffer = torch.zeros_like(self.flat_param)
            if momentum != 0:
                self._load_per_param(sd, g, ("momentum_buffer",), (self.momentum_buffer,))
            else:
                self.momentum_buffer = None
            self.state.zero_()
            self.lr.fill_(float(g["lr"]))
        self.momentum, self.weight_decay = momentum, float(g.get("weight_decay", 0.0))


class FlatRAdam(_FlatOptimizer):
    """RAdam (Liu et al. 2020) with ``betas=(0.9, 0.999)``, ``eps=1e-8`` for the reference's ``--optimizer radam``
    (utils/__init__.py:48-50), as one native launch pair (``nsff_radam_step``): the tick kernel evaluates the rectification
    ``rho_t`` and the bias corrections in double from the device step count, the element kernel updates both moments as Adam
    does and applies ``p -= step m sqrt(bc2) / (sqrt(v) + eps)`` once ``rho_t > 5`` (step 6 for beta2 = 0.999), ``p -= step m``
    before.  Weight decay is decoupled (``p *= 1 - lr wd``).

    **Oracle.**  The reference takes RAdam from the ``torch_optimizer`` package; this class is pinned against
    ``torch.optim.RAdam(..., decoupled_weight_decay=True)`` instead.  To our knowledge the two are the same arithmetic for
    ``weight_decay == 0`` (the reference's default; their thresholds ``>= 5`` and ``> 5`` never differ for beta2 = 0.999) and
    ``torch_optimizer`` decays as ``p -= wd lr p``, i.e. decoupled -- but neither statement was checked against that
    package's source: RAdam with ``weight_decay > 0`` is **unpinned by the reference**.

    One shared step counter, parameters without a gradient, the HIP-only rule and the shared storage: as for
    :class:`FlatAdam` above."""

    def __init__(self, params, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decay_unused=False):
        super().__init__(params, lr, weight_decay, decay_unused, n_state=8)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)

    def step(self):
        _lib.radam_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.state, self.lr,
                        self.betas[0], self.betas[1], self.eps, self.weight_decay, *self._segments())

    reset_state = FlatAdam.reset_state
    state_dict = FlatAdam.state_dict
    load_state_dict = FlatAdam.load_state_dict

    def torch_state_dict(self):
        """The same state in ``torch.optim.RAdam.state_dict()`` format (cloned tensors, parameter order of ``params``)."""
        step = self.state[0].detach().clone().cpu()
        state = {i: {"step": step.clone(), "exp_avg": m, "exp_avg_sq": v}
                 for i, (m, v) in enumerate(zip(self._per_param(self.exp_avg), self._per_param(self.exp_avg_sq)))}
        group = {"lr": float(self.lr), "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                 "decoupled_weight_decay": True, "maximize": False, "foreach": None, "capturable": False,
                 "differentiable": False, "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_torch_state_dict(self, sd):
        """Take over moments, step count and hyper-parameters of a ``torch.optim.RAdam.state_dict()`` over the same parameters
        in the same order (one param group).  Parameters without state keep zero moments.  A state saved with coupled weight
        decay (``decoupled_weight_decay=False`` and ``weight_decay != 0``) is refused: the decay here is decoupled."""
        g = self._one_group(sd)
        if float(g.get("weight_decay", 0.0)) != 0 and not g.get("decoupled_weight_decay", False):
            raise ValueError("FlatRAdam decays the weights decoupled; the state was saved with coupled weight decay")
        with torch.no_grad():
            steps = self._load_per_param(sd, g, ("exp_avg", "exp_avg_sq"), (self.exp_avg, self.exp_avg_sq))
            self.state.zero_(); self.state[0] = float(steps.pop()) if steps else 0.0
            self.lr.fill_(float(g["lr"]))
        self.betas, self.eps = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        self.weight_decay = float(g.get("weight_decay", 0.0))


def detached_state(module):
    """``module.state_dict()`` with every tensor cloned: safe to ``torch.save`` / keep while training goes on (the live
    tensors are views of FlatAdam's one flat buffer and change in place)."""
    return {k: v.detach().clone() for k, v in module.state_dict().items()}
