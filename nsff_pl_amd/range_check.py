"""The f16x3 value-domain flag (include/nsff_render.h: NSFF_RANGE_*, nsff_range_flags) and the checks of
``config.set_range_check`` around ``render_rays``, ``NeRF.forward`` and ``NSFFTrainer.step``."""
import contextlib
import enum
import threading
import warnings

import torch

from . import _lib
from . import config


class RangeFlags(enum.IntFlag):
    """Sources of fp32 values that reached an fp16 split with !(|x| <= 65504) (the bits of NSFF_RANGE_*)."""
    NONE = 0
    ACTIVATIONS = 0x1            # trunk activations / position input rows of an f16x3 inference launch
    SAVED_ACTIVATIONS = 0x2      # activations and input rows of the training forward (the fp16 tiles the backward reads)
    PARAMETERS = 0x4             # parameters at packing time (forward f16x3 pack, backward fp16 pack)
    CODES = 0x8                  # time / appearance / view-direction code columns of an input tile


def describe(flags):
    names = [m.name.lower().replace("_", " ") for m in RangeFlags if m.value and (int(flags) & m.value)]
    return ", ".join(names) or "none"


def _device(device):
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("range_flags: the flag word lives on a GPU")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def range_flags(device=None, clear=True):
    """The device's value-domain word as :class:`RangeFlags` (one nsff_range_flags launch on the current stream, then a
    synchronisation); ``clear``: zero it as well.  The kernels keep recording whatever ``set_range_check`` says."""
    dev = _device(device)
    with torch.cuda.device(dev):
        out = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.range_flags(out, clear)
        return RangeFlags(int(out.item()) & 0xFFFFFFFF)


_local = threading.local()


@contextlib.contextmanager
def suppressed():
    """Inner calls skip their own checks (the trainer checks the whole step once, after the gradient all-reduce)."""
    old = getattr(_local, "off", False)
    _local.off = True
    try:
        yield
    finally:
        _local.off = old


def active():
    """The mode a call should apply now: "off" inside a suppressed region or a graph capture (nothing may sync there)."""
    mode = config.get_range_check()
    if mode == "off" or getattr(_local, "off", False) or torch.cuda.is_current_stream_capturing():
        return "off"
    return mode


@contextlib.contextmanager
def precision(name):
    old = config.get_precision()
    config.set_precision(name)
    try:
        yield
    finally:
        config.set_precision(old)


def report(flags, what, mode, stacklevel=3):
    """warn / raise for a non-empty flag set"""
    msg = (f"{what}: f16x3 operands outside the fp16 range (|x| > 65504) from: {describe(flags)} -- the results are not "
           f"fp32-accurate; use nsff_pl_amd.set_precision('f32') for such a model")
    if mode == "warn":
        warnings.warn(msg, RuntimeWarning, stacklevel=stacklevel)
    else:
        raise RuntimeError(msg)


def checked(what, device, run, can_fallback):
    """run() under the active mode: clear before, read after; "fallback" re-runs a deterministic call in "f32"."""
    mode = active()
    if mode == "off":
        return run()
    range_flags(device, clear=True)
    out = run()
    flags = range_flags(device, clear=False)
    if flags:
        if mode == "fallback" and can_fallback:
            with precision("f32"):
                return run()
        report(flags, what, "warn" if mode == "warn" else "raise", stacklevel=4)
    return out


def all_ranks(flags, device):
    """OR of every rank's flags (per-bit MAX all-reduce), so that all ranks act on the same verdict"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return flags
    bits = torch.tensor([(int(flags) >> i) & 1 for i in range(32)], dtype=torch.int32, device=device)
    dist.all_reduce(bits, op=dist.ReduceOp.MAX)
    return RangeFlags(sum(int(b) << i for i, b in enumerate(bits.tolist())))
