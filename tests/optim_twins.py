"""Torch-op twins of nsff_pl_amd.optim.FlatSGD / FlatRAdam (what common.cpu_flat_adam is for FlatAdam): the same classes with the
device check off and the step written with torch ops in torch's own single-tensor order, so that the trainer's option handling
can be driven on the CPU and the HIP steps have something to be compared with."""
import math

import torch


def _live_elements(opt):
    """The segment form (weight decay on, decay_unused off): per-element mask of tensors with a non-zero gradient, else None."""
    if not opt.weight_decay or opt.decay_unused:
        return None
    live = torch.zeros_like(opt.flat_param, dtype=torch.bool)
    offs = opt.seg_start.tolist()
    for a, b in zip(offs[:-1], offs[1:]):
        live[a:b] = bool((opt.flat_grad[a:b] != 0).any())
    return live


def _restore_dead(live, bufs, keep):
    if live is not None:
        for buf, old in zip(bufs, keep):
            buf.copy_(torch.where(live, buf, old))


def cpu_flat_sgd():
    from nsff_pl_amd.optim import FlatSGD

    class TorchFlatSGD(FlatSGD):
        @staticmethod
        def _check_device(dev):
            pass

        @torch.no_grad()
        def step(self):
            p, g, b = self.flat_param, self.flat_grad, self.momentum_buffer
            self.state[0] += 1
            bufs = (p,) if b is None else (p, b)
            live = _live_elements(self)
            keep = tuple(x.clone() for x in bufs) if live is not None else None
            if self.weight_decay:
                g = g.add(p, alpha=self.weight_decay)
            if b is not None:
                b.mul_(self.momentum).add_(g)
                g = b
            p.add_(g, alpha=-float(self.lr))
            _restore_dead(live, bufs, keep)
    return TorchFlatSGD


def cpu_flat_radam():
    from nsff_pl_amd.optim import FlatRAdam

    class TorchFlatRAdam(FlatRAdam):
        @staticmethod
        def _check_device(dev):
            pass

        @torch.no_grad()
        def step(self):
            b1, b2 = self.betas
            p, g, m, v = self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq
            self.state[0] += 1
            t, lr = float(self.state[0]), float(self.lr)
            live = _live_elements(self)
            keep = (p.clone(), m.clone(), v.clone()) if live is not None else None
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            if self.weight_decay:
                p.mul_(1 - lr * self.weight_decay)
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            corrected = m / bc1
            rho_inf = 2 / (1 - b2) - 1
            rho_t = rho_inf - 2 * t * (b2 ** t) / bc2
            if rho_t > 5.0:
                rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5
                adaptive = math.sqrt(bc2) / v.sqrt().add_(self.eps)
                p.add_(corrected * lr * adaptive * rect, alpha=-1.0)
            else:
                p.add_(corrected * lr, alpha=-1.0)
            _restore_dead(live, (p, m, v), keep)
    return TorchFlatRAdam
