"""GPU checks of nsff_flow_median (csrc/flowmedian.hip) and of the layer over it, nsff_pl_amd.optflow.refine_flow and
sequence_flows(refine=...): both routes against the twin tests/flowmedian_numpy.py at EVERY pixel, as numbers (the weights are
integers, so every sum is exact and any selection gives the same value); the tiled route against the plain one bit for bit; and
the method condition on the GPU's own flow."""
import numpy as np
import pytest
import torch

import flowmedian_numpy as fnp
import optflow_numpy as onp
from nsff_pl_amd import _lib, motion, optflow

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
f32 = np.float32
# a 1-pixel frame, smaller than any window; odd sizes with a ragged last tile; several tiles a frame, both ways, ragged
SHAPES = [(1, 1, 1), (3, 19, 33), (2, 37, 71), (2, 129, 511)]
RADII = [1, 3, 7]
KINDS, GUIDES = ("smooth", "quarter"), ("random", "constant", "step")
VARIANTS = [(k, g) for k in KINDS for g in GUIDES]
SENTINEL = 12345.0

_CASES, _TWINS = {}, {}


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).to(DEV)


def case(shape, kind, guide):
    """Flows in the manner of test_parallax_gpu.py's case: mostly smooth plus noise, sprinkled with 1e10, NaN and infinite values (and
    both zeros); `quarter`: quantised to quarter pixels, so that many candidates tie.  Guides: random, constant (pure spatial
    weights) and a step edge with a little noise.  Shared, read-only."""
    key = (shape, kind, guide)
    if key in _CASES:
        return _CASES[key]
    P, H, W = shape
    rng = np.random.default_rng(100 * H + W + 1000 * KINDS.index(kind) + 10000 * GUIDES.index(guide))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flow = np.zeros((P, H, W, 2))
    for p in range(P):
        a, b, ph = rng.uniform(0.05, 0.3, 2), rng.uniform(0.05, 0.3, 2), rng.uniform(0, 6, 2)
        for c in range(2):
            flow[p, ..., c] = 3 * np.sin(a[c] * xs + b[c] * ys + ph[c]) + np.where(xs + ys > (H + W) / 2, 2.5, -1.0)
    flow += rng.normal(0, 0.3, flow.shape)
    if kind == "quarter":
        flow = np.round(flow * 4) / 4                                # (a small negative rounds to -0)
    flow = flow.astype(f32)
    sort = rng.random((P, H, W))
    flow[sort < 0.01] = 1e10                                         # unknown, the Middlebury way
    flow[(sort >= 0.01) & (sort < 0.015), 0] = np.nan
    flow[(sort >= 0.015) & (sort < 0.02), 1] = np.inf
    flow[(sort >= 0.02) & (sort < 0.025), 0] = -np.inf
    flow[(sort >= 0.025) & (sort < 0.03), 1] = 2e7                   # just beyond the threshold
    flow[(sort >= 0.03) & (sort < 0.04)] = 0.0
    flow[(sort >= 0.04) & (sort < 0.05)] = -0.0
    if guide == "random":
        grey = rng.uniform(0, 255, (P, H, W))
    elif guide == "constant":
        grey = np.full((P, H, W), 100.0)
    else:
        grey = np.where(xs + 0.5 * ys > 0.55 * W, 200.0, 40.0)[None] + rng.normal(0, 3, (P, H, W))
    valid = (rng.random((P, H, W)) < 0.85).astype(np.uint8)
    c = dict(flow=flow, grey=grey.astype(f32), valid=valid, known=fnp.motion_numpy.known(flow))
    for v in c.values():
        v.setflags(write=False)
    _CASES[key] = c
    return c


def twin(shape, kind, guide, radius, given):
    key = (shape, kind, guide, radius, given)
    if key not in _TWINS:
        c = case(shape, kind, guide)
        _TWINS[key] = fnp.weighted_median(c["flow"], c["grey"], c["valid"] if given == "with" else None, radius)
        _TWINS[key].setflags(write=False)
    return _TWINS[key]


def run(c, radius, given, tiled, pairs=slice(None), **kw):
    """One call of the C entry point with a sentinel in every output value."""
    flow, grey = dev(c["flow"][pairs]), dev(c["grey"][pairs])
    out = torch.full_like(flow, SENTINEL)
    _lib.flow_median(flow, grey, out, valid=dev(c["valid"][pairs]) if given == "with" else None, radius=radius, tiled=tiled, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_against_twin(got, c, want, what):
    kn = c["known"]
    assert not np.isnan(got[kn]).any(), what
    bad = kn[..., None] & ~(got == want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    # an unknown centre is copied, bits unchanged (which also shows that the sentinel is gone everywhere)
    assert (bits(got)[~kn] == bits(c["flow"])[~kn]).all(), what
    assert (bits(want)[~kn] == bits(c["flow"])[~kn]).all(), what


def variants_of(shape, radius, given):
    """Every (kind, guide) on the small shapes; on the large one a single variant per (radius, given), all six between them."""
    if shape != SHAPES[-1]:
        return VARIANTS
    return [VARIANTS[(2 * RADII.index(radius) + (given == "with")) % len(VARIANTS)]]


@pytest.mark.parametrize("given", ["with", "without"])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_both_routes_equal_the_twin_at_every_pixel(shape, radius, given):
    for kind, guide in variants_of(shape, radius, given):
        c, want = case(shape, kind, guide), twin(shape, kind, guide, radius, given)
        for tiled in (False, True):
            check_against_twin(run(c, radius, given, tiled), c, want, (kind, guide, "tiled" if tiled else "plain"))


def test_all_six_variants_reach_the_large_shape():
    seen = {variants_of(SHAPES[-1], r, g)[0] for r in RADII for g in ("with", "without")}
    assert seen == set(VARIANTS)


@pytest.mark.parametrize("radius", range(1, fnp.MAX_RADIUS + 1))
def test_tiled_route_gives_the_plain_routes_bits(radius):
    """Every radius is a build of its own of the tiled kernel."""
    for shape, kind, guide in (((3, 19, 33), "quarter", "step"), ((2, 37, 71), "smooth", "random")):
        c = case(shape, kind, guide)
        for given in ("with", "without"):
            plain, tiled = run(c, radius, given, False), run(c, radius, given, True)
            assert (bits(plain) == bits(tiled)).all(), (shape, given)
    # other weights than the defaults: a narrow guide and a narrow window
    c = case((2, 37, 71), "smooth", "step")
    kw = dict(sigma_i=2.5, sigma_s=1.75)
    plain, tiled = run(c, radius, "with", False, **kw), run(c, radius, "with", True, **kw)
    assert (bits(plain) == bits(tiled)).all()
    check_against_twin(tiled, c, fnp.weighted_median(c["flow"], c["grey"], c["valid"], radius, **kw), "narrow")


@pytest.mark.parametrize("tiled", [False, True])
def test_a_pair_alone_equals_the_pair_in_a_batch_and_a_second_call_repeats(tiled):
    shape = (3, 19, 33)
    c = case(shape, "smooth", "random")
    batch = run(c, 3, "with", tiled)
    assert (bits(run(c, 3, "with", tiled)) == bits(batch)).all()
    for p in range(shape[0]):
        assert (bits(run(c, 3, "with", tiled, pairs=slice(p, p + 1))) == bits(batch[p:p + 1])).all(), p


def test_refine_flow_on_uint8_images_equals_refine_flow_on_their_grey():
    shape = (2, 37, 71)
    c = case(shape, "smooth", "random")
    rng = np.random.default_rng(5)
    images = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    flow, valid = dev(c["flow"]), dev(c["valid"])
    a = optflow.refine_flow(flow, dev(images), valid, radius=3)
    b = optflow.refine_flow(flow, _lib.optflow_grey(dev(images)), valid, radius=3)
    d = optflow.refine_flow(flow, dev(images), valid, radius=3, tiled=not optflow.DEFAULT_MEDIAN_TILED)
    assert a.data_ptr() != flow.data_ptr() and a.shape == flow.shape and a.dtype == torch.float32
    assert (bits(a.cpu().numpy()) == bits(b.cpu().numpy())).all() and (bits(a.cpu().numpy()) == bits(d.cpu().numpy())).all()
    check_against_twin(a.cpu().numpy(), c, fnp.weighted_median(c["flow"], onp.grey(images), c["valid"], 3), "uint8")
    with pytest.raises(RuntimeError, match="refine_flow: images: need"):
        optflow.refine_flow(flow, dev(images)[:1], valid)
    with pytest.raises(RuntimeError, match="refine_flow: valid: need"):
        optflow.refine_flow(flow, dev(images), valid.float())
    with pytest.raises(RuntimeError, match="nsff_flow_median failed"):      # out on flow is refused by the C call
        _lib.flow_median(flow, _lib.optflow_grey(dev(images)), flow, radius=3)


def test_sequence_flows_refine_is_the_composition_written_out():
    pair = fnp.make_contrast_pair(64, 96, 0)
    images = dev(np.concatenate([pair["images0"], pair["images1"], pair["images0"]]))
    F, kw = 3, dict(levels=4, warps=3, iters=20)
    both = optflow.optical_flow(torch.cat([images[:-1], images[1:]]), torch.cat([images[1:], images[:-1]]), **kw)
    zero = torch.zeros_like(both[:1])
    fw, bw = torch.cat([both[:F - 1], zero]), torch.cat([zero, both[F - 1:]])
    valid = motion.flow_consistency(fw, bw)
    rfw = torch.cat([optflow.refine_flow(fw[:F - 1], images[:F - 1], valid[:F - 1, 0].contiguous()), zero])
    rbw = torch.cat([zero, optflow.refine_flow(bw[1:], images[1:], valid[1:, 1].contiguous())])
    same = lambda a, b: a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())

    plain = optflow.sequence_flows(images, **kw)                       # refine=False: today's output
    assert sorted(plain) == ["flows_bw", "flows_fw", "valid"]
    assert same(plain["flows_fw"], fw) and same(plain["flows_bw"], bw) and torch.equal(plain["valid"], valid)
    got = optflow.sequence_flows(images, refine=True, **kw)
    assert sorted(got) == ["flows_bw", "flows_fw", "valid"]
    assert same(got["flows_fw"], rfw) and same(got["flows_bw"], rbw)
    assert not same(rfw, fw)                                           # the refinement does something here
    assert (got["flows_fw"][-1] == 0).all() and (got["flows_bw"][0] == 0).all()
    assert torch.equal(got["valid"], motion.flow_consistency(rfw, rbw))
    unchecked = optflow.sequence_flows(images, refine=True, check=False, **kw)
    assert sorted(unchecked) == ["flows_bw", "flows_fw"] and same(unchecked["flows_fw"], rfw) and same(unchecked["flows_bw"], rbw)
    small = optflow.sequence_flows(images, refine=dict(radius=3, tiled=False), **kw)
    assert same(small["flows_fw"][:F - 1], optflow.refine_flow(fw[:F - 1], images[:F - 1], valid[:F - 1, 0].contiguous(), radius=3))


def test_the_gpu_chain_meets_the_rim_condition():
    """(1, 96, 160), seed 0, levels 4, warps 5, iters 30, radius 7: flow, check, refine, all on the GPU.  The twin's rim EPE goes from
    0.855 to 0.159 px, 0.19 of the unrefined one; the GPU's flow is the twin's bits, so the same figures are expected here."""
    pair = fnp.make_contrast_pair(96, 160, 0)
    images = dev(np.concatenate([pair["images0"], pair["images1"]]))
    kw = dict(levels=4, warps=5, iters=30)
    before = optflow.sequence_flows(images, **kw)["flows_fw"][:1].cpu().numpy()
    after = optflow.sequence_flows(images, refine=True, **kw)["flows_fw"][:1].cpu().numpy()
    rim0, interior0, whole0 = fnp.rim_epe(before, pair)
    rim1, interior1, whole1 = fnp.rim_epe(after, pair)
    print(f"\nrim / interior / whole EPE: unrefined {rim0:.4f} / {interior0:.4f} / {whole0:.4f}, refined {rim1:.4f} / {interior1:.4f} / "
          f"{whole1:.4f}: {rim1 / rim0:.3f} of the unrefined rim")
    assert rim1 <= 0.3 * rim0
