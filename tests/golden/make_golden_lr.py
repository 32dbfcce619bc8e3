"""Generate tests/golden/g23_lr_schedules.npz by RUNNING THE REFERENCE's learning-rate schedulers.

Build-container only, like make_golden.py: the reference (kwea123/nsff_pl, read-only, absent on the GPU box) supplies
``utils/warmup_scheduler.py``, loaded by file path -- ``utils/__init__`` itself imports torch_optimizer, which is not
installed.  The schedulers are built exactly as ``get_scheduler`` (utils/__init__.py:59-76) builds them, on a one-parameter
``torch.optim.Adam(lr=5e-4)``, and stepped once per epoch as Lightning steps an epoch-interval scheduler; the rate in force
during every epoch is recorded as float64.  ``poly`` uses ``torch.optim.lr_scheduler.LambdaLR``, the import the reference's
module lacks (its own poly branch raises NameError).  Only data is written; no reference source travels.

    python tests/golden/make_golden_lr.py                   # rewrites tests/golden/g23_lr_schedules.npz

Keys: ``lr/<scheduler>_w<W>_m<m>`` for {steplr, cosine, poly} x {no warm-up, W=3 m=1, W=3 m=4} at 12 epochs, and
``lr/readme_cosine`` (README.md:227-233: cosine, 50 epochs, no warm-up).  The cosine + warm-up sequences are the reference's
ACTUAL behaviour under this torch (an overshoot at e = W + 1, see nsff_pl_amd.training.lr_at), kept on file for that reason.
"""
import importlib.util
import json
import os
import warnings

import numpy as np
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR, MultiStepLR

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

LR = 5e-4
HP = dict(lr=LR, num_epochs=12, decay_step=[4, 8], decay_gamma=0.1, poly_exp=0.9)
WARMUPS = [(0, 1.0), (3, 1.0), (3, 4.0)]                 # (warmup_epochs, warmup_multiplier)
README = dict(lr=LR, lr_scheduler="cosine", num_epochs=50, warmup_epochs=0, warmup_multiplier=1.0)


def load_warmup():
    spec = importlib.util.spec_from_file_location("ref_warmup_scheduler", os.path.join(REF, "utils", "warmup_scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.GradualWarmupScheduler


def record(GradualWarmupScheduler, kind, num_epochs, W, m, hp=HP):
    """get_scheduler (utils/__init__.py:59-76) on Adam(lr); the rate during epochs 0 .. num_epochs - 1."""
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=hp["lr"], eps=1e-8)
    if kind == "steplr":
        sched = MultiStepLR(opt, milestones=hp["decay_step"], gamma=hp["decay_gamma"])
    elif kind == "cosine":
        sched = CosineAnnealingLR(opt, T_max=num_epochs, eta_min=1e-8)
    else:
        sched = LambdaLR(opt, lambda epoch: (1 - epoch / num_epochs) ** hp["poly_exp"])
    if W > 0:
        sched = GradualWarmupScheduler(opt, multiplier=m, total_epoch=W, after_scheduler=sched)
    out = []
    for _ in range(num_epochs):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return np.asarray(out, dtype=np.float64)


def main():
    warnings.simplefilter("ignore")                      # (the epoch argument of scheduler.step is deprecated in torch)
    Warm = load_warmup()
    save, cases = {}, {}
    for kind in ("steplr", "cosine", "poly"):
        for W, m in WARMUPS:
            key = f"{kind}_w{W}_m{int(m)}"
            save["lr/" + key] = record(Warm, kind, HP["num_epochs"], W, m)
            cases[key] = dict(HP, lr_scheduler=kind, warmup_epochs=W, warmup_multiplier=m)
    save["lr/readme_cosine"] = record(Warm, "cosine", README["num_epochs"], 0, 1.0)
    cases["readme_cosine"] = README
    meta = dict(optimizer="adam", cases=cases, torch=torch.__version__,
                source="reference get_scheduler (utils/__init__.py:59-76) + utils/warmup_scheduler.py")
    save["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "g23_lr_schedules.npz"), **save)
    for k in sorted(save):
        if k != "meta":
            print(k, np.array2string(save[k][:12], precision=4))


if __name__ == "__main__":
    main()
