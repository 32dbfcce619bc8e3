"""MI355X checks of what the frame wrappers of nsff_pl_amd/_lib.py refuse before they launch, and of their scratch policy.

The wrappers bind their tensors through one table-driven helper; these are the words it must keep.  For each wrapper one tensor
is spoiled in turn: (a) one element short, (b) of another dtype, (c) a non-contiguous view of the right size -- all three raise in
Python, nothing is launched.  (d) is an ordinary call on zero flows with the fewest tensors the library takes for its outputs (the
reduction outputs among them, every other optional tensor None) and ``scratch=None``: it returns, a second one returns the same
bytes, and so do two calls that share one zeroed scratch of the caller's -- the scratch is left as the next call needs it.

F, H, W = 2, 5, 7: H * W = 35 is odd, so the second frame starts unaligned.  Span and reach are 2.  lpips alone takes 31 x 33
frames, the smallest AlexNet's second pooling leaves a pixel of."""
import pytest
import torch

from nsff_pl_amd import _lib

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
F, H, W, SPAN = 2, 5, 7, 2
PX = F * H * W
LH, LW = _lib.LPIPS_MIN_SIZE, _lib.LPIPS_MIN_SIZE + 2
f32, f64, u8, i32, i64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64
OTHER = {f32: f64, f64: f32, u8: i32, i32: i64, i64: i32}
GH, GW = _lib.panel_grid_shape(H, W, 3 + 3 + 1 + 1)


def z(*shape, dtype=f32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def rnd(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))).to(DEV)


def flows():
    return dict(flows_fw=z(F, H, W, 2), flows_bw=z(F, H, W, 2))


# name -> (wrapper, every tensor it takes, the one to spoil (keyword[, index in a pair]), its name in the message)
FULL = {
    "motion_maps": (lambda: dict(flows(), Fm=rnd(F, 2, 3, 3), err=z(F, 2, H, W), valid=z(F, 2, H, W, dtype=u8), raw=z(F, H, W, dtype=u8),
                                 counts=z(F, 5, dtype=i64), err_sums=z(F, 2, dtype=f64)), ("counts",), "counts"),
    "flow_median": (lambda: dict(flow=z(F, H, W, 2), grey=rnd(F, H, W), out=z(F, H, W, 2), valid=z(F, H, W, dtype=u8)), ("grey",), "grey"),
    "disparity_sparse": (lambda: dict(flows(), Pm=rnd(F, 2, 12), valid=z(F, 2, H, W, dtype=u8), masks=z(F, H, W, dtype=u8),
                                      counts=z(F, dtype=i64)), ("Pm",), "Pm"),
    "disparity_span": (lambda: dict(flows(), Pm=rnd(F, 2, SPAN, 12), span=SPAN, valid=z(F, 2, H, W, dtype=u8), masks=z(F, H, W, dtype=u8),
                                    counts=z(F, dtype=i64), votes=z(F, H, W, dtype=u8), out=(z(F, H, W), z(F, H, W))), ("votes",), "votes"),
    "motion_span": (lambda: dict(flows(), Fm=rnd(F, 2, SPAN, 3, 3), hop_scale=z(SPAN) + 1, span=SPAN, valid=z(F, 2, H, W, dtype=u8),
                                 err=z(F, 2, H, W), hops=z(F, 2, H, W, dtype=u8), raw=z(F, H, W, dtype=u8), counts=z(F, 3, dtype=i64)),
                    ("hop_scale",), "hop_scale"),
    "mask_propagate": (lambda: dict(flows(), src=z(F, H, W, dtype=u8), reach=SPAN, valid=z(F, 2, H, W, dtype=u8), dst=z(F, H, W, dtype=u8),
                                    hits=z(F, H, W, dtype=u8), zero_counts=z(F, dtype=i64)), ("hits",), "hits"),
    "frame_finish": (lambda: dict(rgb=rnd(F, H, W, 3), gt=rnd(F, H, W, 3, seed=1), valid=z(F, H, W, dtype=u8) + 1, depth=rnd(F, H, W),
                                  lut=z(256, 3, dtype=u8), rgb_clipped=z(F, H, W, 3), rgb_u8=z(F, H, W, 3, dtype=u8), sums=z(F, 3, dtype=f64),
                                  depth_range=z(F, 2), depth_u8=z(F, H, W, dtype=u8), depth_rgb_u8=z(F, H, W, 3, dtype=u8)),
                     ("depth_range",), "depth_range"),
    "val_panels": (lambda: dict(F=F, H=H, W=W, pred=rnd(F, H, W, 3), gt=rnd(F, H, W, 3, seed=1), depth=rnd(F, H, W),
                                transient_alpha=rnd(F, H, W, seed=2), static_rgb=rnd(F, H, W, 3, seed=3), static_depth=rnd(F, H, W, seed=4),
                                mask=rnd(F, H, W, seed=5), disp=rnd(F, H, W, seed=6), ssim_loss=rnd(F, H, W, 3, seed=7),
                                lut_depth=z(256, 3, dtype=u8), lut_mask=z(256, 3, dtype=u8), ranges=z(F, 5, 2),
                                grid_u8=z(F, GH, GW, 3, dtype=u8), rmse_u8=z(F, H, W, dtype=u8), ssim_u8=z(F, H, W, dtype=u8),
                                rmse_blend_u8=z(F, H, W, 3, dtype=u8), ssim_blend_u8=z(F, H, W, 3, dtype=u8)), ("grid_u8",), "grid_u8"),
    "flow_maps": (lambda: dict(F=F, H=H, W=W, flow=(z(F, H, W, 2), z(F, H, W, 2)), gt=(rnd(F, H, W, 2), rnd(F, H, W, 2, seed=1)),
                               mask=z(F, H, W, dtype=u8), epe_sums=z(F, 2, 3, dtype=f64), epe_counts=z(F, 2, 3, dtype=i64), maxrad=z(F, 2, 2),
                               image=(z(F, H, W, 3, dtype=u8), z(F, H, W, 3, dtype=u8)),
                               gt_image=(z(F, H, W, 3, dtype=u8), z(F, H, W, 3, dtype=u8))), ("gt", 0), "gt_fw"),
    "ssim": (lambda: dict(gt=rnd(F, H, W, 3), pred=rnd(F, H, W, 3, seed=1), mask=z(F, H * W, dtype=u8), map=z(F, H, W, 3), mean_map=z(F, H * W),
                          sums=z(F, 3, dtype=f64)), ("map",), "map"),
    "lpips": (lambda: dict(packed=z(int(_lib.load().nsff_lpips_packed_bytes()) // 4), gt=rnd(F, LH, LW, 3), pred=rnd(F, LH, LW, 3, seed=1),
                           valid=z(F, LH * LW, dtype=u8), map=z(F, LH, LW), sums=z(F, 3, dtype=f64)), ("map",), "map"),
    "mask_erode": (lambda: dict(src=z(F, H, W, dtype=u8), dst=z(F, H, W, dtype=u8), k=3, zero_counts=z(F, dtype=i64)), ("dst",), "dst"),
}
# (ssim, lpips and mask_erode took the count message of the other nine with the binder; before it they had words of their own)
# name -> (the fewest tensors the library takes for these outputs, the outputs to compare besides what the call returns)
LEAN = {
    "motion_maps": (lambda: dict(flows(), err=z(F, 2, H, W), valid=z(F, 2, H, W, dtype=u8), raw=z(F, H, W, dtype=u8), counts=z(F, 5, dtype=i64),
                                 err_sums=z(F, 2, dtype=f64)), ("err", "valid", "raw", "counts", "err_sums")),
    "flow_median": (lambda: dict(flow=z(F, H, W, 2), grey=rnd(F, H, W), out=z(F, H, W, 2)), ()),
    "disparity_sparse": (lambda: dict(flows(), Pm=rnd(F, 2, 12), counts=z(F, dtype=i64)), ("counts",)),
    "disparity_span": (lambda: dict(flows(), Pm=rnd(F, 2, SPAN, 12), span=SPAN, counts=z(F, dtype=i64)), ("counts",)),
    "motion_span": (lambda: dict(flows(), Fm=rnd(F, 2, SPAN, 3, 3), hop_scale=z(SPAN) + 1, span=SPAN, err=z(F, 2, H, W),
                                 hops=z(F, 2, H, W, dtype=u8), counts=z(F, 3, dtype=i64)), ("err", "hops", "counts")),
    "mask_propagate": (lambda: dict(flows(), src=(rnd(F, H, W) > 0.5).to(u8) * 255, reach=SPAN, hits=z(F, H, W, dtype=u8),
                                    zero_counts=z(F, dtype=i64)), ("hits", "zero_counts")),
    "frame_finish": (lambda: dict(rgb=rnd(F, H, W, 3), gt=rnd(F, H, W, 3, seed=1), depth=rnd(F, H, W), rgb_clipped=z(F, H, W, 3),
                                  rgb_u8=z(F, H, W, 3, dtype=u8), sums=z(F, 3, dtype=f64), depth_range=z(F, 2), depth_u8=z(F, H, W, dtype=u8)),
                     ("rgb_clipped", "rgb_u8", "sums", "depth_range", "depth_u8")),
    "val_panels": (lambda: dict(F=F, H=H, W=W, pred=rnd(F, H, W, 3), gt=rnd(F, H, W, 3, seed=1), ranges=z(F, 5, 2), rmse_u8=z(F, H, W, dtype=u8)),
                   ("ranges", "rmse_u8")),
    "flow_maps": (lambda: dict(F=F, H=H, W=W, flow=(z(F, H, W, 2), None), gt=(rnd(F, H, W, 2), None), epe_sums=z(F, 2, 3, dtype=f64),
                               epe_counts=z(F, 2, 3, dtype=i64), maxrad=z(F, 2, 2), image=(z(F, H, W, 3, dtype=u8), None)),
                  ("epe_sums", "epe_counts", "maxrad", "image")),
}
SCRATCH_BYTES = dict(motion_maps=_lib.motion_maps_scratch_bytes, disparity_sparse=_lib.disparity_sparse_scratch_bytes,
                     disparity_span=_lib.disparity_span_scratch_bytes, motion_span=_lib.motion_span_scratch_bytes,
                     mask_propagate=_lib.motion_span_scratch_bytes, frame_finish=_lib.frame_finish_scratch_bytes,
                     val_panels=_lib.val_panels_scratch_bytes, flow_maps=_lib.flow_maps_scratch_bytes)


def spoiled(name, spoil):
    """The wrapper, its full keywords with the chosen tensor replaced by spoil(tensor), that tensor, and its name in the message."""
    make, where, label = FULL[name]
    kw = make()
    good = kw[where[0]] if len(where) == 1 else kw[where[0]][where[1]]
    bad = spoil(good)
    kw[where[0]] = bad if len(where) == 1 else tuple(bad if i == where[1] else t for i, t in enumerate(kw[where[0]]))
    return getattr(_lib, name), kw, good, f"{name}: {label}"


def refused(fn, kw, text):
    with pytest.raises(RuntimeError) as e:
        fn(**kw)
    print(f"{text!r} <- {str(e.value)!r}")
    assert text in str(e.value)


@pytest.mark.parametrize("name", list(FULL))
def test_one_element_short_is_refused_with_both_counts(hip_lib, name):
    fn, kw, good, who = spoiled(name, lambda t: torch.zeros(t.numel() - 1, dtype=t.dtype, device=DEV))
    refused(fn, kw, f"{who} has {good.numel() - 1} elements on {DEV}, expected {good.numel()} on {DEV}")


@pytest.mark.parametrize("name", list(FULL))
def test_another_dtype_is_refused_by_name(hip_lib, name):
    fn, kw, good, who = spoiled(name, lambda t: t.to(OTHER[t.dtype]))
    refused(fn, kw, f"{who}: need a contiguous {good.dtype} tensor, got {OTHER[good.dtype]}")
    with pytest.raises(RuntimeError) as e:
        fn(**kw)
    assert "(non-contiguous)" not in str(e.value)


@pytest.mark.parametrize("name", list(FULL))
def test_a_non_contiguous_view_is_refused_by_name(hip_lib, name):
    fn, kw, good, who = spoiled(name, lambda t: torch.zeros(2 * t.numel(), dtype=t.dtype, device=DEV)[::2])
    refused(fn, kw, f"{who}: need a contiguous {good.dtype} tensor, got {good.dtype} (non-contiguous)")


def raw_bytes(t):
    return t.contiguous().view(-1).view(u8)


@pytest.mark.parametrize("name", list(LEAN))
def test_lean_call_without_scratch_repeats_itself(hip_lib, name):
    make, outputs = LEAN[name]

    def run(**extra):
        kw = make()
        got = getattr(_lib, name)(**kw, **extra)
        got = () if got is None else got if isinstance(got, tuple) else (got,)
        for o in outputs:
            got += tuple(t for t in (kw[o] if isinstance(kw[o], tuple) else (kw[o],)) if t is not None)
        torch.cuda.synchronize()
        return [raw_bytes(t) for t in got]
    first, second = run(), run()
    assert len(first) == len(second) >= 1
    assert all(torch.equal(a, b) for a, b in zip(first, second)), name
    if name in SCRATCH_BYTES:                                       # one scratch of the caller's, zeroed once, serves call after call
        scratch = torch.zeros(max(SCRATCH_BYTES[name](F, H, W), 16), dtype=u8, device=DEV)
        for turn in range(2):
            again = run(scratch=scratch)
            assert all(torch.equal(a, b) for a, b in zip(first, again)), (name, turn)
