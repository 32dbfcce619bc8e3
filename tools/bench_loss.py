"""Device-event timings of NeRFWLoss alone (forward + backward) over the batch size: csrc/loss.hip against the torch expression.

    python tools/bench_loss.py                     # one JSON line per (rays, leg): median microseconds, kernel launches
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_loss.py --no-count --sizes 65536     # per-kernel times, separately

Legs: `fused` (the default dispatch: rank counting up to 4096 rays, radix select above), `radix` (NSFF_LOSS_SELECT=radix: the
radix select at every size) and `torch` (NSFF_FUSED_LOSS=0: the torch expression -- what ran above 4096 rays before the radix
select existed).  Median of --reps calls after --warmup; launches = device kernels + memsets of one call (torch.profiler).
Render dicts are random leaves of the right shapes with 192 samples per ray, generated on the device.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nsff_pl_amd import _lib  # noqa: E402
from nsff_pl_amd.losses import NeRFWLoss  # noqa: E402

N_FRAMES = 30
NO_GRAD = ("disocc_fw", "disocc_bw", "disoccs_fw", "disoccs_bw", "xyzs_fine")


def inputs(n, s, dev):
    g = torch.Generator(dev).manual_seed(n)

    def r(*shape):
        return torch.rand(*shape, device=dev, generator=g)

    def points(*lead):
        return torch.cat([r(*lead, 2) * 2 - 1, r(*lead, 1) * 1.7 - 0.9], -1)
    xyzs = points(n, s)
    d = dict(rgb_fine=r(n, 3), rgb_coarse=r(n, 3), depth_fine=r(n) * 1.5 + 0.1, depth_coarse=r(n) * 1.5 + 0.1,
             transient_weights_fine=r(n, s) * 0.1 + 1e-3, static_weights_fine=r(n, s) * 0.1 + 1e-3,
             xyz_fw=points(n), xyz_bw=points(n), rgb_fw=r(n, 3), rgb_bw=r(n, 3),
             disocc_fw=r(n, 1) * 0.9 + 0.1, disocc_bw=r(n, 1) * 0.9 + 0.1,
             disoccs_fw=r(n, s, 1) * 0.9 + 0.1, disoccs_bw=r(n, s, 1) * 0.9 + 0.1,
             xyzs_fine=xyzs, xyzs_fw=xyzs + (r(n, s, 3) - 0.5) * 0.05, xyzs_bw=xyzs + (r(n, s, 3) - 0.5) * 0.05,
             xyzs_fw_bw=xyzs + (r(n, s, 3) - 0.5) * 0.02, xyzs_bw_fw=xyzs + (r(n, s, 3) - 0.5) * 0.02)
    leaves = {k: v.requires_grad_(k not in NO_GRAD) for k, v in d.items()}
    targets = dict(rgbs=r(n, 3), disps=r(n) * 2 + 0.1, ts=torch.randint(0, N_FRAMES, (n,), device=dev, generator=g),
                   cam_ids=torch.zeros(n, dtype=torch.long, device=dev),
                   uv_fw=r(n, 2) * torch.tensor([512.0, 288.0], device=dev), uv_bw=r(n, 2) * torch.tensor([512.0, 288.0], device=dev))
    return leaves, targets


def cameras(dev):
    K = torch.tensor([[400.0, 0, 256.0], [0, 400.0, 144.0], [0, 0, 1]])
    P = K @ torch.cat([torch.diag(torch.tensor([1.0, -1.0, -1.0])), torch.zeros(3, 1)], 1)
    return K[None].to(dev), P[None, None].expand(1, N_FRAMES, 3, 4).contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 8192, 65536, 262144])
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--topk", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-count", action="store_true", help="skip the launch count (torch.profiler), e.g. under rocprofv3")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    loss_fn = NeRFWLoss(lambda_geo=0.04, topk=args.topk)
    Ks, Ps = cameras(dev)
    loss_fn.register_buffer("Ks", Ks); loss_fn.register_buffer("Ps", Ps); loss_fn.max_t = N_FRAMES - 1
    legs = (("fused", {}), ("radix", {"NSFF_LOSS_SELECT": "radix"}), ("torch", {"NSFF_FUSED_LOSS": "0"}))
    for n in args.sizes:
        leaves, targets = inputs(n, args.samples, dev)

        def call():
            for v in leaves.values():
                v.grad = None
            terms = loss_fn(leaves, targets, output_transient_flow=["fw", "bw", "disocc"], epoch=3)
            (terms.total() if hasattr(terms, "total") else sum(terms.values())).backward()
        for leg, env in legs:
            for k in ("NSFF_LOSS_SELECT", "NSFF_FUSED_LOSS"):
                os.environ.pop(k, None)
            os.environ.update(env)
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) * 1e3)
            times.sort()
            row = dict(rays=n, samples=args.samples, topk=args.topk, leg=leg, median_us=round(times[len(times) // 2], 1),
                       min_us=round(times[0], 1), loss_path=None if leg == "torch" else _lib.last_loss_path())
            if not args.no_count:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    call()
                    torch.cuda.synchronize()
                row["launches"] = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
            print(json.dumps(row), flush=True)
        del leaves, targets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
