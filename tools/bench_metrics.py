"""Device-event timings of the SSIM metric and the ray bank (csrc/metrics.hip) at the reference's 512 x 288 frame size.

    python tools/bench_metrics.py                  # JSON line: median microseconds and the HBM byte bound of each case
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_metrics.py --reps 20     # per-kernel times, separately

Cases: one metrics.ssim call (full-frame mean); RayBank.update_weights() over 24 and 100 frames (one SSIM launch writing the
weights + one fp64 CDF launch); one 1024-ray RayBank.sample() (torch.rand + one draw-and-gather launch).  Byte bounds: the SSIM
pass reads gt + pred (2 x 12 B per pixel) and writes the 4-B weight per pixel; the CDF reads 4 B and writes 8 B per pixel.
frames.build_records for 100 frames with uint8 images and masks (csrc/rays.hip::ray_records_kernel): the whole call (frame table
upload + one launch) and the launch alone; it reads 3 + 4 + 1 + 16 B and writes 64 B per pixel.
metrics.finish_frames on 1 and 100 frames with every input and output (csrc/metrics.hip::frame_image_kernel + frame_depth_kernel):
the whole call (output allocation + two launches) and nsff_frame_finish alone on preallocated outputs.  The image pass reads
12 + 12 + 1 + 4 B and writes 12 + 3 B per pixel, the depth pass reads 4 B and writes 1 + 3 B: 52 B per pixel.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nsff_pl_amd import _lib, frames, metrics  # noqa: E402
from nsff_pl_amd.sampling import RayBank  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (MI355X datasheet)


def time_us(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2]


def bench_build_records(dev, g, W, H, reps, F=100):
    K = [[400.0, 0, W / 2], [0, 400.0, H / 2], [0, 0, 1]]
    poses = torch.eye(4)[:3].repeat(F, 1, 1)
    poses[:, :, 3] = torch.rand(F, 3) * 0.2 - 0.1
    images = torch.randint(0, 256, (F, H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    masks = torch.randint(0, 2, (F, H, W), device=dev, generator=g, dtype=torch.uint8) * 255
    disps = torch.rand(F, H, W, device=dev, generator=g)
    fw, bw = (torch.randn(F, H, W, 2, device=dev, generator=g) for _ in range(2))
    rec = torch.empty(F, H * W, 16, device=dev)
    table = frames.frame_table(poses, dev)
    K4 = [K[0][0], K[1][1], K[0][2], K[1][2]]
    launch = lambda: _lib.ray_records(K4, table, images, disps, masks, fw, bw, 1.0, 0, F, rec)
    res = {f"build_records_F{F}_us": time_us(lambda: frames.build_records(K, poses, images, disps, masks, fw, bw, out=rec), reps),
           f"ray_records_F{F}_launch_us": time_us(launch, reps)}
    res[f"ray_records_F{F}_bound_us"] = F * H * W * (3 + 4 + 1 + 16 + 64) / HBM_PEAK * 1e6
    return res


FINISH_BYTES_PER_PIXEL = (12 + 12 + 1 + 4) + (12 + 3) + 4 + (1 + 3)


def bench_finish_frames(dev, g, W, H, reps, F):
    rgb = torch.rand(F, H, W, 3, device=dev, generator=g) * 1.2 - 0.1
    gt = torch.rand(F, H, W, 3, device=dev, generator=g)
    valid = torch.rand(F, H, W, device=dev, generator=g) < 0.7
    depth = torch.rand(F, H, W, device=dev, generator=g) * 4
    lut = torch.randint(0, 256, (256, 3), device=dev, generator=g, dtype=torch.uint8)
    outs = metrics.finish_frames(rgb, gt=gt, valid_mask=valid, depth=depth, lut=lut)
    scratch = torch.zeros(_lib.frame_finish_scratch_bytes(F, H, W), dtype=torch.uint8, device=dev)
    launch = lambda: _lib.frame_finish(rgb, gt=gt, valid=valid, depth=depth, lut=lut, scratch=scratch, **outs)
    return {f"finish_frames_F{F}_us": time_us(lambda: metrics.finish_frames(rgb, gt=gt, valid_mask=valid, depth=depth, lut=lut), reps),
            f"frame_finish_F{F}_launch_us": time_us(launch, reps),
            f"frame_finish_F{F}_bound_us": F * H * W * FINISH_BYTES_PER_PIXEL / HBM_PEAK * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H = 512, 288
    px = W * H
    g = torch.Generator(dev).manual_seed(0)
    out = {"frame": [W, H], "hbm_peak_TBps": HBM_PEAK / 1e12}
    gt = torch.rand(H, W, 3, device=dev, generator=g)
    pred = (gt + 0.05 * torch.randn(H, W, 3, device=dev, generator=g)).clamp(0, 1)
    out["ssim_512x288_us"] = time_us(lambda: metrics.ssim(gt, pred), args.reps)
    for F in (24, 100):
        rec = torch.rand(F, px, 16, device=dev, generator=g)
        bank = RayBank(rec, (W, H), hard_sampling=True, seed=0)
        bank.tmp_rgb.copy_((bank.rgb + 0.05 * torch.randn(bank.rgb.shape, device=dev, generator=g)).clamp(0, 1))
        bytes_ = F * px * (24 + 4) + F * px * (4 + 8)
        t = time_us(bank.update_weights, args.reps)
        out[f"update_weights_F{F}_us"] = t
        out[f"update_weights_F{F}_bound_us"] = bytes_ / HBM_PEAK * 1e6
        if F == 24:
            out["sample_1024_us"] = time_us(lambda: bank.sample(1024, generator=g), args.reps)
        del bank, rec
        torch.cuda.empty_cache()
    out.update(bench_build_records(dev, g, W, H, args.reps))
    for F in (1, 100):
        out.update(bench_finish_frames(dev, g, W, H, args.reps, F))
        torch.cuda.empty_cache()
    print(json.dumps({k: round(v, 2) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
