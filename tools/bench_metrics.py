"""Device-event timings of the SSIM metric and the ray bank (csrc/metrics.hip) at the reference's 512 x 288 frame size.

    python tools/bench_metrics.py                  # JSON line: median microseconds and the HBM byte bound of each case
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_metrics.py --reps 20     # per-kernel times, separately

Cases: one metrics.ssim call (full-frame mean); RayBank.update_weights() over 24 and 100 frames (one SSIM launch writing the
weights + one fp64 CDF launch); one 1024-ray RayBank.sample() (torch.rand + one draw-and-gather launch).  Byte bounds: the SSIM
pass reads gt + pred (2 x 12 B per pixel) and writes the 4-B weight per pixel; the CDF reads 4 B and writes 8 B per pixel.
frames.build_records for 100 frames with uint8 images and masks (csrc/rays.hip::ray_records_kernel): the whole call (frame table
upload + one launch) and the launch alone; it reads 3 + 4 + 1 + 16 B and writes 64 B per pixel.
metrics.finish_frames on 1 and 100 frames with every input and output (csrc/frames.hip::frame_image_kernel + frame_depth_kernel):
the whole call (output allocation + two launches) and nsff_frame_finish alone on preallocated outputs.  The image pass reads
12 + 12 + 1 + 4 B and writes 12 + 3 B per pixel, the depth pass reads 4 B and writes 1 + 3 B: 52 B per pixel.
flow_frames' kernel work on 1 and 100 frames, both directions with ground truth and mask (csrc/flow.hip::flow_map_kernel +
flow_colour_kernel): nsff_flow_maps alone on preallocated outputs, its two launches separately, and the projection alone.  Per pixel and direction the
map pass reads 12 + 8 B and writes 8 B, the colour pass reads 8 + 8 B and writes 3 + 3 B, plus the 1-B mask: 101 B per pixel.
The validation panels (--only panel) on 1 and 30 frames with all eight tiles (csrc/frames.hip::panel_range_kernel +
panel_compose_kernel): nsff_val_panels alone on preallocated outputs and its range launch alone.  The range pass reads gt, pred, depth,
static depth, disp and the SSIM loss map (48 B per pixel); the compose pass reads those again plus alpha, static rgb and mask
(68 B) and writes the two index images, the two blends and nine grid cells (1 + 1 + 3 + 3 + 27 B): 151 B per pixel.
The frame resize (--only resize) of 1 and 30 decoded 1280 x 720 frames to 512 x 288 (csrc/resize.hip): each kernel of
nsff_frame_resize alone on preallocated outputs with the tables already on the device -- Lanczos on uint8 RGB, nearest on the
uint8 mask and the fp32 disparity, bilinear on the fp32 flow.  Byte bound: every source byte read once plus every output byte
written (the nearest kernels read fewer: a source pixel they skip is never touched, so their bound is an upper one).
LPIPS (--only lpips) on 1 and 30 frame pairs (csrc/lpips.hip): nsff_lpips alone on preallocated outputs (map and sums), the whole
LPIPS.score call, and -- in the same run, alternating with it -- the same graph in torch on the GPU (F.conv2d etc. through MIOpen,
fp32, channels-first as the reference feeds it; seeded random weights of AlexNet's shapes): what a user has without this kernel.
Bounds per call: the convolutions' FLOPs over the fp32 MFMA peak, and the bytes that must move (both images, the packed weights
once, the map) over the HBM peak; `act_MB` is what the call actually writes and reads back as taps and pooled maps.
The scene scale (--only scale) on 1, 30 and 100 frames of 512 x 288 disparities with 20 000 COLMAP points (csrc/scale.hip):
nsff_scene_scale alone on preallocated outputs and workspace against the byte bound of each of its kernels (bench_scale states the
arithmetic), the whole scene.nearest_depth call by the host clock, and the reference's per-frame numpy loop, restated in host_numpy_scale, on the same data on the host.
Scene-flow tracks (--only tracks; csrc/tracks.hip): tracks.advect for n = 8 steps at (R, S) = (147456, 1) -- a 512 x 288 frame of surface
points -- and (4096, 128), with the fixed-view projection; nsff_track_step alone on preallocated slabs, with and without cameras,
against the bytes it must move per point (12 B position in, the 12 B of flow, 12 B position out; with cameras 8 + 4 B more) and
against the bytes it touches when every 64-byte record comes in whole (`rec_bound`) -- also at (131072, 128), 16.8 M points on
random records, where the launch is long enough for its traffic to show; the field query of one step alone, and the
step kernel's share of field query + step; nsff_track_draw (three launches) for 10 000 tracks of 8 segments on the frame, against
clearing, reading and resolving the canvas and the image (4 + 4 + 3 + 3 B per pixel) plus the 8 + 1 B per track end.
Motion masks (--only motion; csrc/motion.hip) on 1 and 30 frames: nsff_motion_maps alone on preallocated outputs with its statistics,
nsff_mask_erode alone (k = 15, with the zero count), and the whole motion.motion_masks call (host-side fundamental matrices, their
upload, the allocations and both launches).  Byte bounds: the map pass must read each of the two flows once (8 + 8 B per pixel: a
frame's forward flow is A of its own forward direction and B of the next frame's backward one) and write err and valid of both
directions and raw (2 x (4 + 1) + 1 B): 27 B per pixel; as issued, without any reuse, it asks for 2 x (8 + 8) B of flow: 43 B
(`issued_bound`).  The erosion reads and writes one byte per pixel: 2 B (its halo re-reads come from cache).
TV-L1 optical flow (--only optflow; csrc/optflow.hip) at 512 x 288 on P = 1 and P = 58 pairs (a 30-frame sequence, both
directions), default parameters (5 levels, 5 warps, 30 iterations, median on): each kernel alone at the finest level (device events
around one call on preallocated planes), the 30 iterations of one warp there on the plain route and on every built (tile, k) of the
fused route, taken in turn, and the whole optical_flow call on each route.  Bounds: a launch of the iteration must read the six state
planes and four of the constants and write the six state planes, 64 B per pixel, whether it runs one iteration (plain: 30 launches a
warp) or k (fused: ceil(30 / k)): `iter30_*_bound_us` is that traffic at the HBM peak; `redundancy` is the fused route's share of
repeated arithmetic ((T + 2 k) / T)^2.  No target time: nothing comparable was measured before.
Disparity from flow and poses (--only disparity; csrc/depth.hip) at 512 x 288 on F = 1 and F = 30 frames, default parameters (3 levels,
30 iterations, lambda 8, sigma 12.75): nsff_disparity_sparse alone with valid, masks and its counts (it must read both flows, two
validity bytes and a mask byte and write n and c: 8 + 8 + 2 + 1 + 4 + 4 = 27 B per pixel), the 30 relax iterations of the finest level
on the plain route and on every built (tile, k) of the fused route, taken in turn (a launch reads d, n, c and the grey guide and
writes d, 20 B per pixel, whether it runs one iteration or k: `relax30_*_bound_us` is that traffic at the HBM peak; `redundancy` is
((T + 2 k) / T)^2), the whole nsff_disparity_dense call on each route, and depth.disparity_maps with its default route (host-side
parallax rows, their upload, the grey stage and the allocations included).  --only disparity_resources needs no GPU: the
compiler's report of VGPRs, scratch, LDS and waves per SIMD of every kernel of csrc/depth.hip.
On F = 30 frames also nsff_disparity_span (csrc/parallax.hip) at span 1, 2, 4 and 8 with valid, masks, votes and counts, and
nsff_disparity_sparse on the same inputs, all five taken in turn: `span{S}_us` against `span{S}_bound_us`, the (20 S + 9) B per pixel
it must move at the HBM peak (per direction 10 B for the first vote and 10 B of unique taps per hop; 9 B written), and
`span{S}_bound_fraction`, the bound over the time; `span1_sparse_us` is the one-frame kernel beside span 1.
Motion masks over several frames (--only motionspan; csrc/motionspan.hip) at 512 x 288 on F = 1 and F = 30 frames, on the inputs of
--only disparity: nsff_motion_span at span 1, 2, 4 and 8 with valid, err, hops and counts, nsff_motion_maps and nsff_disparity_span
(the same spans, the yardstick: the same chain with more arithmetic) on the same inputs, nsff_mask_propagate at reach 1, 2 and 4
with valid, hits and counts, all taken in turn, the median of 30 (device events); and the whole motion.motion_masks(span=4, reach=2)
call.  `*_bound_us`: the bytes a call must move at the HBM peak -- the chained test per direction 9 B for the first step (flow,
valid) and 10 B of unique taps per hop, 11 B written (err, hops, raw): (20 S + 9) B per pixel; the propagation one mask byte per
step more, src read and dst and hits written: (22 R + 1) B per pixel -- and `*_bound_fraction` the bound over the time.
--only motionspan_resources needs no GPU: the compiler's report of the two kernels.
The image-guided weighted median of a flow map (--only flowmedian; csrc/flowmedian.hip) at 512 x 288 on P = 1 and P = 58 pairs, radius 3
and radius 7, default weights, with `valid`: nsff_flow_median alone on preallocated tensors, the plain and the tiled route taken in
turn, the median of 30 (device events).  `visits` is what the selection must do whatever the route, 2 components x 32 steps x
(2 r + 1)^2 candidates a pixel, and `*_visits_per_ns` that count over the time.  No target time: nothing comparable was measured before.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.nn.functional as TF  # noqa: E402

from nsff_pl_amd import LPIPS, _lib, frames, metrics, scene  # noqa: E402
from nsff_pl_amd.sampling import RayBank  # noqa: E402

HBM_PEAK = 8.0e12          # B/s (MI355X datasheet)
F32_MFMA_PEAK = 157.3e12   # FLOP/s, v_mfma_f32_32x32x2_f32 (MI355X datasheet: the fp32 vector rate)


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


FLOW_MAP_BYTES_PER_PIXEL = 2 * (12 + 8 + 8) + 1
FLOW_COLOUR_BYTES_PER_PIXEL = 2 * (8 + 8 + 3 + 3)


def bench_flow_frames(dev, g, W, H, reps, F):
    K4 = [400.0, 400.0, W / 2, H / 2]
    n_poses = F + 2
    Ps = torch.zeros(n_poses, 3, 4, device=dev)
    Ps[:, 0, 0], Ps[:, 1, 1], Ps[:, 2, 2] = K4[0], -K4[1], -1.0     # K diag(1, -1, -1) [I | t]
    Ps[:, 0, 2], Ps[:, 1, 2] = -K4[2], -K4[3]
    Ps[:, :, 3] = torch.rand(n_poses, 3, device=dev, generator=g) * 0.2 - 0.1
    ts = torch.arange(1, F + 1, device=dev, dtype=torch.int32)
    xyz = tuple(torch.cat([torch.rand(F, H * W, 2, device=dev, generator=g) * 2 - 1,
                           torch.rand(F, H * W, 1, device=dev, generator=g) * 1.9 - 1], -1).contiguous() for _ in range(2))
    gt = tuple(3 * torch.randn(F, H, W, 2, device=dev, generator=g) for _ in range(2))
    mask = (torch.rand(F, H, W, device=dev, generator=g) < 0.3).to(torch.uint8)
    u8 = lambda: torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    maps = dict(flow=(torch.empty(F, H, W, 2, device=dev), torch.empty(F, H, W, 2, device=dev)),
                epe_sums=torch.empty(F, 2, 3, dtype=torch.float64, device=dev),
                epe_counts=torch.empty(F, 2, 3, dtype=torch.int64, device=dev), maxrad=torch.empty(F, 2, 2, device=dev))
    images = dict(image=(u8(), u8()), gt_image=(u8(), u8()))
    scratch = torch.zeros(_lib.flow_maps_scratch_bytes(F, H, W), dtype=torch.uint8, device=dev)
    both = lambda: _lib.flow_maps(F, H, W, xyz=xyz, K4=K4, Ps=Ps, ts=ts, max_t=n_poses - 1, gt=gt, mask=mask, share_gt_scale=True,
                                  scratch=scratch, **maps, **images)
    first = lambda: _lib.flow_maps(F, H, W, xyz=xyz, K4=K4, Ps=Ps, ts=ts, max_t=n_poses - 1, gt=gt, mask=mask, scratch=scratch, **maps)
    project = lambda: _lib.flow_maps(F, H, W, xyz=xyz, K4=K4, Ps=Ps, ts=ts, max_t=n_poses - 1, flow=maps["flow"])
    second = lambda: _lib.flow_maps(F, H, W, flow=maps["flow"], gt=gt, scale=maps["maxrad"], share_gt_scale=True, **images)
    px = F * H * W
    return {f"flow_frames_F{F}_us": time_us(both, reps),
            f"flow_frames_F{F}_bound_us": px * (FLOW_MAP_BYTES_PER_PIXEL + FLOW_COLOUR_BYTES_PER_PIXEL) / HBM_PEAK * 1e6,
            f"flow_map_F{F}_us": time_us(first, reps),
            f"flow_map_F{F}_bound_us": px * FLOW_MAP_BYTES_PER_PIXEL / HBM_PEAK * 1e6,
            f"flow_project_F{F}_us": time_us(project, reps),               # the map pass without ground truth or reduction
            f"flow_project_F{F}_bound_us": px * 2 * (12 + 8) / HBM_PEAK * 1e6,
            f"flow_colour_F{F}_us": time_us(second, reps),
            f"flow_colour_F{F}_bound_us": px * FLOW_COLOUR_BYTES_PER_PIXEL / HBM_PEAK * 1e6}


PANEL_RANGE_BYTES_PER_PIXEL = 12 + 12 + 4 + 4 + 4 + 12
PANEL_COMPOSE_BYTES_PER_PIXEL = PANEL_RANGE_BYTES_PER_PIXEL + (4 + 12 + 4) + (1 + 1 + 3 + 3 + 9 * 3)


def bench_panels(dev, g, W, H, reps, F):
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=g)
    gt = rand(F, H * W, 3)
    ins = dict(gt=gt, depth=rand(F, H * W) * 4, transient_alpha=rand(F, H * W), static_rgb=rand(F, H * W, 3) * 1.2 - 0.1,
               static_depth=rand(F, H * W) * 4, mask=(rand(F, H * W) < 0.3).float(), disp=rand(F, H * W) * 2, ssim_loss=rand(F, H * W, 3) * 0.2,
               lut_depth=torch.randint(0, 256, (256, 3), device=dev, generator=g, dtype=torch.uint8),
               lut_mask=torch.randint(0, 256, (256, 3), device=dev, generator=g, dtype=torch.uint8))
    pred = gt + 0.1 * torch.randn(F, H * W, 3, device=dev, generator=g)
    GH, GW = _lib.panel_grid_shape(H, W, 8)
    u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
    ranges = torch.empty(F, 5, 2, device=dev)
    outs = dict(grid_u8=u8(F, GH, GW, 3), rmse_u8=u8(F, H * W), ssim_u8=u8(F, H * W), rmse_blend_u8=u8(F, H * W, 3), ssim_blend_u8=u8(F, H * W, 3))
    scratch = torch.zeros(_lib.val_panels_scratch_bytes(F, H, W), dtype=torch.uint8, device=dev)
    both = lambda: _lib.val_panels(F, H, W, pred, ranges=ranges, scratch=scratch, **ins, **outs)
    first = lambda: _lib.val_panels(F, H, W, pred, ranges=ranges, scratch=scratch, **ins)
    px = F * H * W
    return {f"val_panels_F{F}_us": time_us(both, reps),
            f"val_panels_F{F}_bound_us": px * (PANEL_RANGE_BYTES_PER_PIXEL + PANEL_COMPOSE_BYTES_PER_PIXEL) / HBM_PEAK * 1e6,
            f"panel_range_F{F}_us": time_us(first, reps),
            f"panel_range_F{F}_bound_us": px * PANEL_RANGE_BYTES_PER_PIXEL / HBM_PEAK * 1e6}


def bench_resize(dev, g, W, H, reps, F, src_wh=(1280, 720)):
    w, h = src_wh
    cases = (("lanczos_rgb", _lib.RESIZE_LANCZOS_U8, torch.randint(0, 256, (F, h, w, 3), device=dev, generator=g, dtype=torch.uint8)),
             ("nearest_mask", _lib.RESIZE_NEAREST_PIL, torch.randint(0, 256, (F, h, w, 1), device=dev, generator=g, dtype=torch.uint8)),
             ("nearest_disp", _lib.RESIZE_NEAREST_CV, torch.rand(F, h, w, 1, device=dev, generator=g)),
             ("linear_flow", _lib.RESIZE_LINEAR_CV, torch.randn(F, h, w, 2, device=dev, generator=g)))
    res = {}
    for name, filt, src in cases:
        dst = torch.empty(F, H, W, src.shape[3], dtype=src.dtype, device=dev)
        xt, yt = frames._table(dev, filt, w, W), frames._table(dev, filt, h, H)
        res[f"resize_{name}_F{F}_us"] = time_us(lambda: _lib.frame_resize(filt, src, dst, xt, yt, (W / w, H / h)), reps)
        res[f"resize_{name}_F{F}_bound_us"] = (src.numel() * src.element_size() + dst.numel() * dst.element_size()) / HBM_PEAK * 1e6
    return res


def time_alternating_us(fns, reps, warmup=5):
    """Median device time of each of fns, taken in turn within every repetition (they see the same machine state)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) * 1e3)
    return [sorted(t)[len(t) // 2] for t in times]


LPIPS_CONV = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))   # cin, cout, k, stride, pad
LPIPS_LAUNCHES = 10        # nsff_lpips: one memset node, five convolutions, two pools, the distance and the final pass


def torch_lpips(in0, in1, conv_w, conv_b, lin):
    """The LPIPS graph (normalize=True, spatial=True) on (F, 3, H, W) fp32 batches with torch's own kernels."""
    shift = in0.new_tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
    scale = in0.new_tensor([.458, .448, .450]).view(1, 3, 1, 1)
    x = torch.cat([(2 * in0 - 1 - shift) / scale, (2 * in1 - 1 - shift) / scale])
    F, H, W = in0.shape[0], in0.shape[2], in0.shape[3]
    total = 0
    for l, (_, _, _, stride, pad) in enumerate(LPIPS_CONV):
        if l in (1, 2):
            x = TF.max_pool2d(x, 3, 2)
        x = TF.relu(TF.conv2d(x, conv_w[l], conv_b[l], stride=stride, padding=pad))
        n = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
        m = TF.conv2d((n[:F] - n[F:]) ** 2, lin[l])
        total = total + TF.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)
    return total


def bench_lpips(dev, g, W, H, reps, F):
    conv_w = [torch.randn(cout, cin, k, k, device=dev, generator=g) * (2.0 / (cin * k * k)) ** 0.5 for cin, cout, k, _, _ in LPIPS_CONV]
    conv_b = [torch.rand(cout, device=dev, generator=g) * 0.1 - 0.05 for _, cout, _, _, _ in LPIPS_CONV]
    lin = [torch.rand(1, cout, 1, 1, device=dev, generator=g) / cout for _, cout, _, _, _ in LPIPS_CONV]
    model = LPIPS(conv_w, conv_b, lin, device=dev)
    gt = torch.rand(F, H, W, 3, device=dev, generator=g)
    pred = (gt + 0.05 * torch.randn(F, H, W, 3, device=dev, generator=g)).clamp(0, 1)
    valid = torch.rand(F, H, W, device=dev, generator=g) < 0.7
    gt_chw, pred_chw = gt.permute(0, 3, 1, 2).contiguous(), pred.permute(0, 3, 1, 2).contiguous()
    out_map = torch.empty(F, H, W, device=dev)
    sums = torch.empty(F, 3, dtype=torch.float64, device=dev)
    work = torch.empty(_lib.lpips_workspace_bytes(F, H, W), dtype=torch.uint8, device=dev)
    packed = model.packed()
    launch = lambda: _lib.lpips(packed, gt, pred, valid=valid.reshape(F, H * W), map=out_map, sums=sums, normalize=True, workspace=work)
    whole = lambda: model.score(gt, pred, valid=valid, want_sums=True, normalize=True)
    ref = lambda: torch_lpips(gt_chw, pred_chw, conv_w, conv_b, lin)
    launch()
    worst = (out_map - ref()[:, 0]).abs().max().item()           # the two forms being timed compute the same thing
    t_launch, t_whole, t_ref = time_alternating_us((launch, whole, ref), reps)
    dims = _lib.lpips_dims(H, W)
    flops = sum(2 * F * 2 * h * w * cout * cin * k * k for (h, w), (cin, cout, k, _, _) in zip(dims, LPIPS_CONV))
    pooled = [((h - 3) // 2 + 1) * ((w - 3) // 2 + 1) for h, w in dims[:2]]
    act = 4 * 2 * F * (sum(h * w * c[1] for (h, w), c in zip(dims, LPIPS_CONV)) + sum(p * c[1] for p, c in zip(pooled, LPIPS_CONV)))
    must = F * H * W * (2 * 12 + 4 + 1) + packed.numel() * 4 + F * 24
    return {f"lpips_F{F}_launch_us": t_launch, f"lpips_F{F}_score_us": t_whole, f"lpips_F{F}_torch_us": t_ref,
            f"lpips_F{F}_launches": LPIPS_LAUNCHES, f"lpips_F{F}_gflop": flops / 1e9,
            f"lpips_F{F}_flop_bound_us": flops / F32_MFMA_PEAK * 1e6, f"lpips_F{F}_byte_bound_us": must / HBM_PEAK * 1e6,
            f"lpips_F{F}_act_MB": act / 1e6, f"lpips_F{F}_max_abs_diff_vs_torch": worst}


def host_numpy_scale(K, w2c, points, vis, disps):
    """What the reference's nearest_depth loop (datasets/monocular.py:93-116) computes, per frame with numpy on the host, in this
    project's words: project the frame's visible points, truncate and clamp to a pixel, fit disparity = slope / depth + intercept
    by mean-centred moments, and take slope / (95th percentile of the frame - intercept) where r^2 > 0.9, else the 5th percentile
    of the depths; 0.75 x the minimum."""
    K64 = K.astype(np.float64)
    best = 1e8
    for f, frame in enumerate(disps):
        H, W = frame.shape
        seen = points[vis[f] == 1]
        cam = w2c[f, :3, :3] @ seen.T + w2c[f, :3, 3:]
        proj = K64 @ cam
        depth = proj[2]
        col = np.clip(np.trunc(proj[0] / depth), 0, W - 1).astype(np.int64)
        row = np.clip(np.trunc(proj[1] / depth), 0, H - 1).astype(np.int64)
        inv, y = 1.0 / depth, frame[row, col].astype(np.float64)
        di, dy = inv - inv.mean(), y - y.mean()
        sxx, sxy, syy = di @ di, di @ dy, dy @ dy
        slope = sxy / sxx
        intercept = y.mean() - slope * inv.mean()
        if sxy * sxy > 0.9 * sxx * syy:
            best = min(best, slope / (np.percentile(frame, 95) - intercept))
        else:
            best = min(best, np.percentile(depth, 5))
    return 0.75 * best


def bench_scale(dev, g, W, H, reps, F, N=20000):
    """nsff_scene_scale (csrc/scale.hip) on F frames of W x H disparities and N points, 60 % visible per frame, on preallocated
    outputs and workspace.  The byte bounds, per kernel:
      clear   the tickets, partials and histograms written once:           workspace bytes - 8 F N
      points  per frame N visibility bytes, N points (24 B), one gathered disparity (4 B), N depths written (8 B):  37 F N
      disp    the disparities read once per digit pass:                    4 passes x 4 F H W
      depth   the depth array read once per digit pass:                    8 passes x 8 F N
    (the finish kernel moves 2 x 12 x 1 KiB of counters per frame, not counted).  The whole call is 15 launches; the time is the
    call's, so the figure beside the bounds' sum includes their launch gaps.  The comparison is host_numpy_scale, the reference's per-frame numpy loop restated,
    on the same data on the host (wall clock, one run)."""
    import time
    rng = np.random.default_rng(0)
    depth = rng.uniform(2.0, 12.0, N)
    f = 0.9 * W
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
    points = np.stack([rng.uniform(-0.55, 0.55, N) * depth * W / f, rng.uniform(-0.55, 0.55, N) * depth * H / f, depth], 1)
    w2c = np.tile(np.eye(4), (F, 1, 1))
    w2c[:, :3, 3] = rng.normal(size=(F, 3)) * 0.1
    vis = (rng.random((F, N)) < 0.6).astype(np.uint8)
    disps = torch.rand(F, H, W, device=dev, generator=g) * 0.6 + 0.1
    t_points, t_vis = torch.from_numpy(points).to(dev), torch.from_numpy(vis).to(dev)
    t_w2c, t_K = torch.from_numpy(np.ascontiguousarray(w2c[:, :3])).to(dev), torch.from_numpy(K).to(dev)
    lo, hi, _ = scene.percentile_ranks(H * W, 95, np.float32)
    work_bytes = _lib.scene_scale_work_bytes(F, N, H, W)
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    outs = (torch.empty(F, 8, dtype=torch.float64, device=dev), torch.empty(F, 2, device=dev),
            torch.empty(F, 2, dtype=torch.float64, device=dev), None)
    call = lambda: _lib.scene_scale(t_points, t_vis, t_w2c, t_K, disps, (lo, hi), work=work, out=outs)
    res = {f"scale_F{F}_us": time_us(call, reps)}
    bounds = {"clear": work_bytes - 8 * F * N, "points": 37 * F * N, "disp_select": 4 * 4 * F * H * W, "depth_select": 8 * 8 * F * N}
    for k, b in bounds.items():
        res[f"scale_F{F}_{k}_bound_us"] = b / HBM_PEAK * 1e6
    res[f"scale_F{F}_bound_us"] = sum(bounds.values()) / HBM_PEAK * 1e6
    host_disps = disps.cpu().numpy()
    t0 = time.perf_counter()
    want = host_numpy_scale(K, w2c, points, vis, host_disps)
    res[f"scale_F{F}_reference_host_us"] = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    got = scene.nearest_depth(K, w2c, points, vis, disps)
    torch.cuda.synchronize()
    res[f"scale_F{F}_nearest_depth_wall_us"] = (time.perf_counter() - t0) * 1e6
    res[f"scale_F{F}_rel_diff_to_reference"] = abs(got - want) / abs(want)
    return res


def bench_tracks(dev, g, W, H, reps, n=8):
    from nsff_pl_amd import NeRF, PosEmbedding, tracks
    torch.manual_seed(0)
    emb = {"xyz": PosEmbedding(9, 10), "t": torch.nn.Embedding(30, 48).to(dev)}
    model = NeRF("fine", use_viewdir=False, encode_transient=True, in_channels_t=48, output_flow=True).to(dev)
    K = np.array([[400.0, 0, W / 2], [0, 400.0, H / 2], [0, 0, 1]])
    view = torch.tensor([[400.0, 0, -W / 2, 0.1], [0, -400.0, -H / 2, 0.05], [0, 0, -1.0, 0.02]], device=dev)
    freqs = [float(f) for f in emb["xyz"].freqs]
    res = {}
    for R, S in ((W * H, 1), (4096, 128), (131072, 128)):       # (the last: the step kernel alone, large enough to time its traffic)
        P, tag = R * S, f"R{R}_S{S}"
        big = P > 1 << 22
        xyz = torch.cat([torch.rand(R, S, 2, device=dev, generator=g) * 2 - 1, torch.rand(R, S, 1, device=dev, generator=g) * 1.85 - 1], -1)
        ts = torch.randint(0, 20, (R,), device=dev, generator=g, dtype=torch.int32)
        if not big:
            res[f"advect_{tag}_n{n}_us"] = time_us(lambda: tracks.advect(model, emb, xyz, ts, n, 29, Ps=view, K=K), max(reps // 5, 3), warmup=2)
        raw, nxt = torch.empty(P, _lib.RAW_STRIDE, device=dev), torch.empty_like(xyz)
        alive, t_out, a_out = torch.ones(R, dtype=torch.uint8, device=dev), torch.empty_like(ts), torch.empty(R, dtype=torch.uint8, device=dev)
        uv, depth = torch.empty(R, S, 2, device=dev), torch.empty(R, S, device=dev)
        rows = emb["t"](ts.long()).contiguous()
        query = lambda: _lib.field_query(model, raw, P, S, static_mode=0, transient_mode=2, flow_heads=1, xyz=xyz, freqs=freqs, t_emb=rows)
        if big:
            raw.normal_(generator=g)
            query = lambda: None
        step = lambda **cam: _lib.track_step(R, S, 1, 29, xyz, ts, alive, raw=raw, xyz_out=nxt, t_out=t_out, alive_out=a_out, **cam)
        t_query = float("nan") if big else time_us(query, reps)
        t_step = time_us(step, reps)
        t_cam = time_us(lambda: step(K4=(400.0, 400.0, W / 2, H / 2), Ps=view[None], fixed_view=True, uv=uv, depth=depth), reps)
        res.update({f"field_query_{tag}_us": t_query, f"track_step_{tag}_us": t_step, f"track_step_{tag}_bound_us": P * 36 / HBM_PEAK * 1e6,
                    f"track_step_{tag}_rec_bound_us": P * (24 + 64) / HBM_PEAK * 1e6, f"track_step_cam_{tag}_us": t_cam,
                    f"track_step_cam_{tag}_bound_us": P * 48 / HBM_PEAK * 1e6, f"track_step_cam_{tag}_rec_bound_us": P * (36 + 64) / HBM_PEAK * 1e6,
                    f"track_step_cam_{tag}_share_of_step": t_cam / (t_cam + t_query)})
        del raw, nxt, uv, depth, xyz
        torch.cuda.empty_cache()
    Q = 10000
    walk = torch.cat([torch.rand(1, Q, 2, device=dev, generator=g) * torch.tensor([W, H], device=dev),
                      torch.randn(n, Q, 2, device=dev, generator=g) * 3], 0).cumsum(0).contiguous()
    ok = torch.rand(n + 1, Q, device=dev, generator=g) < 0.95
    image = torch.randint(0, 256, (H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    lut, out = torch.as_tensor(tracks.default_lut()).to(dev), torch.empty_like(image)
    scratch = torch.empty(_lib.track_draw_scratch_bytes(H, W), dtype=torch.uint8, device=dev)
    okb = ok.view(torch.uint8)
    res[f"track_draw_Q{Q}_n{n}_us"] = time_us(lambda: _lib.track_draw(H, W, n, Q, walk, okb, image, lut, out, scratch), reps)
    res[f"track_draw_Q{Q}_n{n}_bound_us"] = (H * W * (4 + 4 + 3 + 3) + (n + 1) * Q * 9) / HBM_PEAK * 1e6
    res[f"tracks_draw_Q{Q}_n{n}_call_us"] = time_us(lambda: tracks.draw(image, walk, ok, lut), reps)
    return {k: v for k, v in res.items() if v == v}            # (the large case has no field query: its NaN entries are dropped)


MOTION_MAP_BYTES_PER_PIXEL = (8 + 8) + 2 * (4 + 1) + 1
MOTION_MAP_ISSUED_BYTES_PER_PIXEL = 2 * (8 + 8) + 2 * (4 + 1) + 1


def bench_motion(dev, g, W, H, reps, F):
    from nsff_pl_amd import motion
    K = np.array([[400.0, 0, W / 2], [0, 400.0, H / 2], [0, 0, 1]])
    poses = np.tile(np.eye(4)[:3], (F, 1, 1))
    poses[:, 0, 3] = 0.1 * np.arange(F)
    fw = 3 * torch.randn(F, H, W, 2, device=dev, generator=g)
    bw = -fw + 0.3 * torch.randn(F, H, W, 2, device=dev, generator=g)     # roughly consistent: most pixels take the whole path
    Fm = motion.fundamental_matrices(K, poses).to(dev)
    out = dict(err=torch.empty(F, 2, H, W, device=dev), valid=torch.empty(F, 2, H, W, dtype=torch.uint8, device=dev),
               raw=torch.empty(F, H, W, dtype=torch.uint8, device=dev), counts=torch.empty(F, 5, dtype=torch.int64, device=dev),
               err_sums=torch.empty(F, 2, dtype=torch.float64, device=dev))
    mask, zeros = torch.empty(F, H, W, dtype=torch.uint8, device=dev), torch.empty(F, dtype=torch.int64, device=dev)
    scratch = torch.zeros(_lib.motion_maps_scratch_bytes(F, H, W), dtype=torch.uint8, device=dev)
    maps = lambda: _lib.motion_maps(fw, bw, Fm, scratch=scratch, **out)
    erode = lambda: _lib.mask_erode(out["raw"], mask, 15, zero_counts=zeros, scratch=scratch)
    px = F * H * W
    return {f"motion_maps_F{F}_us": time_us(maps, reps),
            f"motion_maps_F{F}_bound_us": px * MOTION_MAP_BYTES_PER_PIXEL / HBM_PEAK * 1e6,
            f"motion_maps_F{F}_issued_bound_us": px * MOTION_MAP_ISSUED_BYTES_PER_PIXEL / HBM_PEAK * 1e6,
            f"mask_erode_k15_F{F}_us": time_us(erode, reps),
            f"mask_erode_k15_F{F}_bound_us": px * 2 / HBM_PEAK * 1e6,
            f"motion_masks_F{F}_call_us": time_us(lambda: motion.motion_masks(fw, bw, K, poses), reps)}


OPTFLOW_ITER_BYTES_PER_PIXEL = (6 + 4 + 6) * 4     # one launch of the iteration: state and constants in, state out


def bench_optflow(dev, g, W, H, reps, P, iters=30):
    from nsff_pl_amd import optflow
    px = P * H * W
    rgb0 = torch.randint(0, 256, (P, H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    # a smooth textured pair with a known shift, so that the iteration runs on realistic constants
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    wave = lambda dx, dy: sum(a * torch.sin(ph + fx * (xs - dx) + fy * (ys - dy)) for a, ph, fx, fy in
                              ((1.0, 0.3, 0.31, 0.12), (0.8, 1.1, -0.22, 0.41), (0.6, 2.0, 0.55, -0.35), (0.9, 0.7, 0.07, 0.63)))
    I0 = (127.5 + 38 * wave(0.0, 0.0)).expand(P, H, W).contiguous()
    I1 = (127.5 + 38 * wave(2.0, -0.7)).expand(P, H, W).contiguous()
    u = torch.zeros(2, P, H, W, device=dev)
    consts = _lib.optflow_warp(I0, I1, u)
    state, other = torch.zeros(6, P, H, W, device=dev), torch.empty(6, P, H, W, device=dev)
    state = _lib.optflow_iterate(consts, state, 5, fused=False, other=other)      # a non-trivial state
    other = torch.empty_like(state)
    half = _lib.optflow_down(I0)
    tag = f"optflow_P{P}"
    out = {f"{tag}_grey_us": time_us(lambda: _lib.optflow_grey(rgb0), reps),
           f"{tag}_down_us": time_us(lambda: _lib.optflow_down(I0), reps),
           f"{tag}_up_us": time_us(lambda: _lib.optflow_up(half, (H, W)), reps),
           f"{tag}_warp_us": time_us(lambda: _lib.optflow_warp(I0, I1, u), reps),
           f"{tag}_median_us": time_us(lambda: _lib.optflow_median(I0), reps)}
    routes = [("plain", dict(fused=False))] + [(f"fused_T{t}_K{k}", dict(fused=True, tile=t, k=k)) for t, k in _lib.OPTFLOW_PAIRS]
    times = time_alternating_us([lambda kw=kw: _lib.optflow_iterate(consts, state, iters, other=other, **kw) for _, kw in routes], reps)
    for (name, kw), t in zip(routes, times):
        launches = -(-iters // kw.get("k", 1))
        out[f"{tag}_iter{iters}_{name}_us"] = t
        out[f"{tag}_iter{iters}_{name}_bound_us"] = px * OPTFLOW_ITER_BYTES_PER_PIXEL * launches / HBM_PEAK * 1e6
        if kw["fused"]:
            out[f"{tag}_{name}_redundancy"] = ((kw["tile"] + 2 * kw["k"]) / kw["tile"]) ** 2
    scratch = torch.empty(optflow.scratch_bytes(P, H, W), dtype=torch.uint8, device=dev)
    flow = torch.empty(P, H, W, 2, device=dev)
    rgb1 = torch.roll(rgb0, (1, 2), (1, 2))
    calls = time_alternating_us([lambda kw=kw: _lib.optflow(rgb0, rgb1, flow, scratch=scratch, **kw) for _, kw in routes], max(reps // 5, 3), warmup=2)
    for (name, _), t in zip(routes, calls):
        out[f"{tag}_call_{name}_us"] = t
    out[f"{tag}_call_default_us"] = time_us(lambda: optflow.optical_flow(rgb0, rgb1), max(reps // 5, 3), warmup=2)
    return out


def bench_flowmedian(dev, g, W, H, P, reps=30):
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    # two motions with an image edge on the motion edge, a rounded flow edge, noise, and a check that fails near the edge
    dist = torch.hypot(xs - 0.5 * W, ys - 0.5 * H) - 0.22 * W
    disc = dist <= 0
    grey = (torch.where(disc, 200.0, 80.0) + 25 * torch.sin(0.31 * xs + 0.12 * ys)).expand(P, H, W).contiguous()
    grey = grey + 2 * torch.randn(P, H, W, device=dev, generator=g)
    blend = torch.sigmoid(-dist / 3)[..., None]
    flow = (blend * torch.tensor([3.0, -1.5], device=dev) + (1 - blend) * torch.tensor([-2.0, 0.7], device=dev)).expand(P, H, W, 2).contiguous()
    flow = flow + 0.05 * torch.randn(P, H, W, 2, device=dev, generator=g)
    valid = ((dist.abs() > 3) & (torch.rand(P, H, W, device=dev, generator=g) < 0.97)).to(torch.uint8).contiguous()
    out_t = torch.empty_like(flow)
    out = {}
    for r in (3, 7):
        fns = [lambda t=t, r=r: _lib.flow_median(flow, grey, out_t, valid=valid, radius=r, tiled=t) for t in (False, True)]
        times = time_alternating_us(fns, reps, warmup=3)
        visits = 2 * 32 * (2 * r + 1) ** 2 * P * H * W
        for name, t in zip(("plain", "tiled"), times):
            out[f"flowmedian_P{P}_r{r}_{name}_us"] = t
            out[f"flowmedian_P{P}_r{r}_{name}_visits_per_ns"] = visits / (t * 1e3)
        out[f"flowmedian_P{P}_r{r}_plain_over_tiled"] = times[0] / times[1]
    return out


DISPARITY_SPARSE_BYTES_PER_PIXEL = 8 + 8 + 2 + 1 + 4 + 4     # both flows, valid of both directions, the mask in; n and c out
DISPARITY_RELAX_BYTES_PER_PIXEL = (4 + 1) * 4                # one launch of the relaxation: d, n, c, grey in, d out


def bench_disparity(dev, g, W, H, reps, F, iters=30):
    from nsff_pl_amd import depth
    px = F * H * W
    K = np.array([[400.0, 0, W / 2], [0, 400.0, H / 2], [0, 0, 1]])
    poses = np.tile(np.eye(4)[:3], (F + 1, 1, 1))                # one pose more than frames, so that F = 1 has a neighbour's row
    poses[:, 0, 3] = 0.1 * np.arange(F + 1)
    Pm = depth.parallax_matrices(K, poses)[:F].contiguous().to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    delta = 0.3 + 0.1 * torch.sin(0.02 * xs + 0.03 * ys)         # a smooth disparity map: the flow is its parallax, 40 delta px, and noise
    fw = torch.stack([-40.0 * delta, torch.zeros_like(delta)], -1).expand(F, H, W, 2) + 0.05 * torch.randn(F, H, W, 2, device=dev, generator=g)
    bw = -fw + 0.05 * torch.randn(F, H, W, 2, device=dev, generator=g)
    valid = (torch.rand(F, 2, H, W, device=dev, generator=g) < 0.9).to(torch.uint8)
    masks = torch.where((xs - W / 2) ** 2 + (ys - H / 2) ** 2 < (0.2 * H) ** 2, 0, 255).to(torch.uint8).expand(F, H, W).contiguous()
    grey = (127.5 + 38 * (torch.sin(0.31 * xs + 0.12 * ys) + 0.8 * torch.sin(1.1 - 0.22 * xs + 0.41 * ys))).expand(F, H, W).contiguous()
    rgb = grey.clamp(0, 255).to(torch.uint8)[..., None].expand(F, H, W, 3).contiguous()
    counts = torch.empty(F, dtype=torch.int64, device=dev)
    small = torch.zeros(_lib.disparity_sparse_scratch_bytes(F, H, W), dtype=torch.uint8, device=dev)
    sparse = lambda: _lib.disparity_sparse(fw, bw, Pm, valid=valid, masks=masks, counts=counts, scratch=small)
    n, c = sparse()
    tag = f"disparity_F{F}"
    out = {f"{tag}_known_fraction": float(counts.sum()) / px,
           f"{tag}_sparse_us": time_us(sparse, reps),
           f"{tag}_sparse_bound_us": px * DISPARITY_SPARSE_BYTES_PER_PIXEL / HBM_PEAK * 1e6}
    d, other = torch.full((F, H, W), 0.3, device=dev), torch.empty(F, H, W, device=dev)
    routes = [("plain", dict(fused=False))] + [(f"fused_T{t}_K{k}", dict(fused=True, tile=t, k=k)) for t, k in _lib.DISPARITY_PAIRS]
    times = time_alternating_us([lambda kw=kw: _lib.disparity_relax(d, n, c, grey, iters, other=other, **kw) for _, kw in routes], reps)
    for (name, kw), t in zip(routes, times):
        launches = -(-iters // kw.get("k", 1))
        out[f"{tag}_relax{iters}_{name}_us"] = t
        out[f"{tag}_relax{iters}_{name}_bound_us"] = px * DISPARITY_RELAX_BYTES_PER_PIXEL * launches / HBM_PEAK * 1e6
        if kw["fused"]:
            out[f"{tag}_{name}_redundancy"] = ((kw["tile"] + 2 * kw["k"]) / kw["tile"]) ** 2
    scratch = torch.empty(depth.scratch_bytes(F, H, W), dtype=torch.uint8, device=dev)
    disps = torch.empty(F, H, W, device=dev)
    calls = time_alternating_us([lambda kw=kw: _lib.disparity_dense(n, c, grey, disps, iters=iters, scratch=scratch, **kw) for _, kw in routes], reps)
    for (name, _), t in zip(routes, calls):
        out[f"{tag}_dense_{name}_us"] = t
    if F > 1:
        out.update(bench_disparity_span(dev, fw, bw, K, poses, valid, masks, reps, tag))
    poses_F = poses[:F] if F > 1 else poses[:1]
    out[f"{tag}_maps_call_default_us"] = time_us(lambda: depth.disparity_maps(rgb, fw, bw, K, poses_F, masks=masks, valid=valid), reps)
    return out


DISPARITY_SPANS = (1, 2, 4, 8)


def disparity_span_bytes_per_pixel(span):
    """What nsff_disparity_span must move: per direction 10 B for the first vote (flow, valid, mask) and 10 B of unique taps per
    hop, n, c and votes written."""
    return 20 * span + 9


def bench_disparity_span(dev, fw, bw, K, poses, valid, masks, reps, tag):
    """nsff_disparity_span at every span of DISPARITY_SPANS and nsff_disparity_sparse on the same inputs, taken in turn."""
    from nsff_pl_amd import depth
    F, H, W = (int(v) for v in fw.shape[:3])
    px = F * H * W
    counts = torch.empty(F, dtype=torch.int64, device=dev)
    votes = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
    out2 = tuple(torch.empty(F, H, W, device=dev) for _ in range(2))
    scratch = torch.zeros(_lib.disparity_span_scratch_bytes(F, H, W), dtype=torch.uint8, device=dev)
    rows = {s: depth.parallax_matrices(K, poses, span=s)[:F].reshape(F, 2, s, 12).contiguous().to(dev) for s in DISPARITY_SPANS}
    fns = [lambda s=s: _lib.disparity_span(fw, bw, rows[s], s, valid=valid, masks=masks, counts=counts, votes=votes, scratch=scratch, out=out2)
           for s in DISPARITY_SPANS]
    Pm1 = rows[1].reshape(F, 2, 12)
    fns.append(lambda: _lib.disparity_sparse(fw, bw, Pm1, valid=valid, masks=masks, counts=counts, scratch=scratch))
    times = time_alternating_us(fns, reps)
    out = {}
    for s, t in zip(DISPARITY_SPANS, times):
        fns[DISPARITY_SPANS.index(s)]()
        bound = px * disparity_span_bytes_per_pixel(s) / HBM_PEAK * 1e6
        out[f"{tag}_span{s}_us"], out[f"{tag}_span{s}_bound_us"], out[f"{tag}_span{s}_bound_fraction"] = t, bound, bound / t
        out[f"{tag}_span{s}_known_fraction"] = float(counts.sum()) / px
        out[f"{tag}_span{s}_mean_votes"] = float(votes.sum(dtype=torch.int64)) / px
    out[f"{tag}_span1_sparse_us"] = times[-1]
    return out


MOTION_SPANS, MOTION_REACHES = (1, 2, 4, 8), (1, 2, 4)


def motion_span_bytes_per_pixel(span):
    """What nsff_motion_span must move: per direction 9 B for the first step (flow, valid) and 10 B of unique taps per hop; err,
    hops and raw written (8 + 2 + 1)."""
    return 20 * span + 9


def mask_propagate_bytes_per_pixel(reach):
    """What nsff_mask_propagate must move: per direction 9 B for the first step, one mask byte per step and 10 B of unique taps per
    hop; src read, dst and hits written."""
    return 22 * reach + 1


def bench_motionspan(dev, g, W, H, reps, F):
    """nsff_motion_span, nsff_disparity_span and nsff_mask_propagate at every span / reach, and nsff_motion_maps, on the inputs of
    bench_disparity, taken in turn; then the whole motion_masks(span=4, reach=2) call."""
    from nsff_pl_amd import depth, motion
    px = F * H * W
    K = np.array([[400.0, 0, W / 2], [0, 400.0, H / 2], [0, 0, 1]])
    poses = np.tile(np.eye(4)[:3], (F, 1, 1))
    poses[:, 0, 3] = 0.1 * np.arange(F)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    delta = 0.3 + 0.1 * torch.sin(0.02 * xs + 0.03 * ys)         # a smooth disparity map: the flow is its parallax, 40 delta px, and noise
    fw = torch.stack([-40.0 * delta, torch.zeros_like(delta)], -1).expand(F, H, W, 2) + 0.05 * torch.randn(F, H, W, 2, device=dev, generator=g)
    bw = -fw + 0.05 * torch.randn(F, H, W, 2, device=dev, generator=g)
    valid = (torch.rand(F, 2, H, W, device=dev, generator=g) < 0.9).to(torch.uint8)
    masks = torch.where((xs - W / 2) ** 2 + (ys - H / 2) ** 2 < (0.2 * H) ** 2, 0, 255).to(torch.uint8).expand(F, H, W).contiguous()
    scratch = torch.zeros(_lib.motion_maps_scratch_bytes(F, H, W), dtype=torch.uint8, device=dev)
    err, hops = torch.empty(F, 2, H, W, device=dev), torch.empty(F, 2, H, W, dtype=torch.uint8, device=dev)
    raw, dst, hits = (torch.empty(F, H, W, dtype=torch.uint8, device=dev) for _ in range(3))
    counts3, counts5, counts1 = (torch.empty(F, n, dtype=torch.int64, device=dev) for n in (3, 5, 1))
    sums, valid_out = torch.empty(F, 2, dtype=torch.float64, device=dev), torch.empty(F, 2, H, W, dtype=torch.uint8, device=dev)
    votes, out2 = torch.empty(F, H, W, dtype=torch.uint8, device=dev), tuple(torch.empty(F, H, W, device=dev) for _ in range(2))
    Fs = {s: motion.fundamental_matrices(K, poses, span=s).reshape(F, 2, s, 3, 3).contiguous().to(dev) for s in MOTION_SPANS}
    Ps = {s: depth.parallax_matrices(K, poses, span=s).reshape(F, 2, s, 12).contiguous().to(dev) for s in MOTION_SPANS}
    scales = {s: torch.from_numpy(motion.default_hop_scale(s)).to(dev) for s in MOTION_SPANS}
    names, fns = [], []
    for s in MOTION_SPANS:
        names.append(f"span{s}")
        fns.append(lambda s=s: _lib.motion_span(fw, bw, Fs[s], scales[s], s, valid=valid, err=err, hops=hops, raw=raw, counts=counts3, scratch=scratch))
        names.append(f"disparity_span{s}")
        fns.append(lambda s=s: _lib.disparity_span(fw, bw, Ps[s], s, valid=valid, masks=masks, counts=counts1, votes=votes, scratch=scratch, out=out2))
    for r in MOTION_REACHES:
        names.append(f"propagate{r}")
        fns.append(lambda r=r: _lib.mask_propagate(masks, fw, bw, r, valid=valid, dst=dst, hits=hits, zero_counts=counts1, scratch=scratch))
    names.append("motion_maps")
    fns.append(lambda: _lib.motion_maps(fw, bw, Fs[1].reshape(F, 2, 3, 3), err=err, valid=valid_out, raw=raw, counts=counts5, err_sums=sums, scratch=scratch))
    times = dict(zip(names, time_alternating_us(fns, reps)))
    tag = f"motionspan_F{F}"
    out = {}
    for s in MOTION_SPANS:
        fns[names.index(f"span{s}")]()
        bound = px * motion_span_bytes_per_pixel(s) / HBM_PEAK * 1e6
        out[f"{tag}_span{s}_us"], out[f"{tag}_span{s}_bound_us"], out[f"{tag}_span{s}_bound_fraction"] = times[f"span{s}"], bound, bound / times[f"span{s}"]
        out[f"{tag}_span{s}_disparity_span_us"] = times[f"disparity_span{s}"]
        out[f"{tag}_span{s}_mean_hops"] = float(hops.sum(dtype=torch.int64)) / px
    out[f"{tag}_motion_maps_us"] = times["motion_maps"]
    for r in MOTION_REACHES:
        bound = px * mask_propagate_bytes_per_pixel(r) / HBM_PEAK * 1e6
        out[f"{tag}_propagate{r}_us"], out[f"{tag}_propagate{r}_bound_us"], out[f"{tag}_propagate{r}_bound_fraction"] = times[f"propagate{r}"], bound, bound / times[f"propagate{r}"]
    out[f"{tag}_masks_span4_reach2_call_us"] = time_us(lambda: motion.motion_masks(fw, bw, K, poses, span=4, reach=2), reps)
    out[f"{tag}_masks_default_call_us"] = time_us(lambda: motion.motion_masks(fw, bw, K, poses), reps)
    return out


def disparity_resources(source="depth.hip"):
    """The compiler's resource report of every kernel of csrc/depth.hip (or of another source of csrc/ built the same way):
    {kernel: [VGPRs, scratch bytes, LDS bytes, waves per SIMD]}."""
    import re
    import subprocess
    import tempfile
    csrc = os.path.join(ROOT, "nsff_pl_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
               "-Rpass-analysis=kernel-resource-usage", "-c", source, "-o", os.path.join(tmp, "out.o")]
        text = subprocess.run(cmd, cwd=csrc, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", m.group(1))
            t = re.match(r"([a-z_]+?)(?:ILi(\d+)ELi(\d+)EE|E)", name)
            name = f"{t.group(1)}<{t.group(2)}, {t.group(3)}>" if t and t.group(2) else (t.group(1) if t else name)
            out[name] = [None] * 4
        for i, key in enumerate(("VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name and "Agpr" not in line:
                out[name][i] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="", help="comma-separated cases to run: finish, flow, panel, resize, lpips, scale, tracks, motion, optflow, flowmedian, disparity, motionspan (default: everything but lpips, optflow, flowmedian, disparity and motionspan); disparity_resources and motionspan_resources alone need no GPU")
    args = ap.parse_args()
    if args.only == "disparity_resources":
        print(json.dumps(disparity_resources()))
        return
    if args.only == "motionspan_resources":
        print(json.dumps(disparity_resources("motionspan.hip")))
        return
    dev = torch.device("cuda:0")
    W, H = 512, 288
    px = W * H
    g = torch.Generator(dev).manual_seed(0)
    out = {"frame": [W, H], "hbm_peak_TBps": HBM_PEAK / 1e12}
    only = [c for c in args.only.split(",") if c]
    if only:
        for F in (1, 100):
            if "finish" in only:
                out.update(bench_finish_frames(dev, g, W, H, args.reps, F))
            if "flow" in only:
                out.update(bench_flow_frames(dev, g, W, H, args.reps, F))
            torch.cuda.empty_cache()
        if "panel" in only:
            for F in (1, 30):
                out.update(bench_panels(dev, g, W, H, args.reps, F))
        if "resize" in only:
            for F in (1, 30):
                out.update(bench_resize(dev, g, W, H, args.reps, F))
                torch.cuda.empty_cache()
        if "lpips" in only:
            for F in (1, 30):
                out.update(bench_lpips(dev, g, W, H, args.reps, F))
                torch.cuda.empty_cache()
        if "scale" in only:
            for F in (1, 30, 100):
                out.update(bench_scale(dev, g, W, H, args.reps, F))
                torch.cuda.empty_cache()
        if "tracks" in only:
            out.update(bench_tracks(dev, g, W, H, args.reps))
        if "motion" in only:
            for F in (1, 30):
                out.update(bench_motion(dev, g, W, H, args.reps, F))
        if "optflow" in only:
            for P in (1, 58):
                out.update(bench_optflow(dev, g, W, H, args.reps, P))
                torch.cuda.empty_cache()
        if "flowmedian" in only:
            for P in (1, 58):
                out.update(bench_flowmedian(dev, g, W, H, P))
                torch.cuda.empty_cache()
        if "disparity" in only:
            for F in (1, 30):
                out.update(bench_disparity(dev, g, W, H, args.reps, F))
                torch.cuda.empty_cache()
        if "motionspan" in only:
            for F in (1, 30):
                out.update(bench_motionspan(dev, g, W, H, min(args.reps, 30), F))
                torch.cuda.empty_cache()
        print(json.dumps({k: (round(v, 2) if v >= 0.01 else float(f"{v:.3g}")) if isinstance(v, float) else v for k, v in out.items()}))
        return
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
        out.update(bench_flow_frames(dev, g, W, H, args.reps, F))
        torch.cuda.empty_cache()
    for F in (1, 30):
        out.update(bench_panels(dev, g, W, H, args.reps, F))
        out.update(bench_resize(dev, g, W, H, args.reps, F))
    print(json.dumps({k: round(v, 2) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
