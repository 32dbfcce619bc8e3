"""Generate tests/golden/g22_loss_large.npz by RUNNING THE REFERENCE's losses.NeRFWLoss (build container only, like make_golden.py).

The seeded synthetic render dict of tests/select_rule.py at 8192 rays x 32 samples, topk 1.0 and 0.5, no per-ray weights (the
reference's weight broadcast only works when every ray is valid, losses.py:163-164), in fp32 and fp64: the eleven terms and, per
consumed input tensor, (sum g, sum |g|, <g, r>) of the gradient of their sum.  Inputs are regenerated from the seed by the test;
only the statistics are stored.

    python tests/golden/make_golden_loss_large.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts the repository and tests/ on the path; the kornia / datasets / softsplat stubs)

N_RAYS, N_SAMPLES, SEED, EPOCH = 8192, 32, 22, 3
FLOW = ["fw", "bw", "disocc"]


def main():
    import scenes
    import select_rule
    make_golden.import_reference()
    import losses as ref_losses
    render = select_rule.synthetic_render(N_RAYS, N_SAMPLES, SEED)
    ts = select_rule.synthetic_ts(N_RAYS, scenes.N_FRAMES, SEED)
    meta = dict(n_rays=N_RAYS, n_samples=N_SAMPLES, seed=SEED, epoch=EPOCH)
    save = {"meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)}
    for topk in (1.0, 0.5):
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            loss_fn = ref_losses.NeRFWLoss(lambda_geo=0.04, thickness=1, topk=topk)
            Ks, Ps, max_t = scenes.camera_buffers()
            loss_fn.register_buffer("Ks", Ks.to(dt)); loss_fn.register_buffer("Ps", Ps.to(dt)); loss_fn.max_t = max_t
            targets = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in scenes.synthetic_targets(N_RAYS, ts, SEED).items()}
            leaves = select_rule.leaves_of(render, dtype=dt)
            ld = loss_fn(leaves, targets, epoch=EPOCH, output_transient_flow=FLOW)
            assert sorted(ld) == sorted(select_rule.TERMS), sorted(ld)
            sum(ld.values()).backward()
            stats = select_rule.grad_statistics({k: v.grad for k, v in leaves.items() if v.grad is not None})
            key = f"{tag}_topk{topk:g}"
            save["terms" + key] = np.frombuffer(json.dumps({k: float(v) for k, v in ld.items()}).encode(), dtype=np.uint8)
            save["stats" + key] = np.frombuffer(json.dumps(stats).encode(), dtype=np.uint8)
            print(f"g22 topk {topk:g} fp{tag}: total {float(sum(ld.values())):.6f}  {len(stats)} tensors")
    np.savez_compressed(os.path.join(HERE, "g22_loss_large.npz"), **save)


if __name__ == "__main__":
    main()
