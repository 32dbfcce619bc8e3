"""MI355X checks of the optical-flow kernels (csrc/optflow.hip) against the numpy fp32 twin tests/optflow_numpy.py, and of
optflow.optical_flow / sequence_flows on top of them.  Nothing is read from outside the repository.

Every stage is a chain of single fp32 operations that numpy rounds the same way (add, subtract, multiply, divide, floor, square
root, comparisons), so every comparison is for EQUALITY OF BITS at every pixel: the threshold step of the iteration is discontinuous
and amplifies last-place differences to whole pixels near occlusions, so a tolerance would say nothing.  The accuracy of the method
itself is a condition on the result (and, by bit equality, on the twin): see test_accuracy_on_the_two_motion_pair."""
import numpy as np
import pytest
import torch

import optflow_numpy as onp
from nsff_pl_amd import _lib, frames, motion, optflow

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
T, K = _lib.OPTFLOW_TILE, _lib.OPTFLOW_K
STAGE_SHAPES = [(2, 37, 53), (1, 64, 96)]                       # odd sides on the way down the pyramid
ITER_SHAPES = [(3, 4, 4), (2, 19, 33), (1, 37, 71), (1, T + 3, 2 * T + 5)]     # the minimum; ...; several tiles both ways, ragged
SMALL = (1, 11, 23)                                             # smaller than a tile: one halo crosses two opposite borders
PARAMS = dict(lam=0.15, theta=0.3, tau=0.25)

_CASES = {}


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


def iter_case(shape):
    """A random non-zero state (u and p) and constants under which all four branches of the threshold step occur; shared, read-only."""
    if shape in _CASES:
        return _CASES[shape]
    P, H, W = shape
    rng = np.random.default_rng(100 * H + W)
    Ix, Iy = (rng.normal(0, 12, shape).astype(np.float32) for _ in range(2))
    flat = rng.random(shape) < 0.1                              # no gradient there: g = 0, the step factor is 0
    Ix[flat], Iy[flat] = 0, 0
    consts = np.stack([Ix, Iy, Ix * Ix + Iy * Iy, rng.normal(0, 25, shape).astype(np.float32), np.zeros(shape, np.float32)])
    state = np.concatenate([rng.normal(0, 1.5, (2,) + shape), rng.uniform(-0.7, 0.7, (4,) + shape)]).astype(np.float32)
    c = dict(consts=consts, state=state, twin={})
    consts.setflags(write=False), state.setflags(write=False)
    _CASES[shape] = c
    return c


def twin_iterations(shape, iters):
    c = iter_case(shape)
    if iters not in c["twin"]:
        done = max((n for n in c["twin"] if n < iters), default=0)          # continue from the longest run there is
        c["twin"][iters] = onp.iterate(c["consts"], c["twin"][done] if done else c["state"], iters - done, **PARAMS)
        c["twin"][iters].setflags(write=False)
    return c["twin"][iters]


def run_iterations(shape, iters, **route):
    c = iter_case(shape)
    return _lib.optflow_iterate(dev(c["consts"]), dev(c["state"]), iters, **PARAMS, **route)


# ---- grey and pyramid, upsampling, median ----
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_grey_pyramid_upsampling_and_median_equal_the_twin(hip_lib, shape):
    n, H, W = shape
    rng = np.random.default_rng(H + W)
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    level, got = onp.grey(rgb), _lib.optflow_grey(dev(rgb))
    assert same_bits(got, level) == 0
    assert torch.equal(_lib.optflow_grey(got), got)             # grey frames are copied
    sizes = [(H, W)]
    while min(level.shape[1:]) >= 2:                            # all the way down, past what the pipeline uses
        level, got = onp.down(level), _lib.optflow_down(got)
        sizes.append(level.shape[1:])
        assert tuple(got.shape) == level.shape and same_bits(got, level) == 0, sizes[-1]
    assert any(h % 2 or w % 2 for h, w in sizes[:-1]) and len(sizes) >= 6     # an odd side somewhere on the way
    for (h, w), (Hf, Wf) in zip(sizes[1:], sizes[:-1]):        # every level to the one above it
        if min(h, w) < 2:
            continue
        coarse = rng.normal(0, 3, (n, h, w)).astype(np.float32)
        assert same_bits(_lib.optflow_up(dev(coarse), (Hf, Wf)), onp.up(coarse, (Hf, Wf))) == 0, (h, w)
    planes = rng.normal(0, 3, shape).astype(np.float32)
    planes[:, ::5, ::3] = 0.0                                   # ties, zeros of both signs
    planes[:, 1::7, 2::4] = -0.0
    assert same_bits(_lib.optflow_median(dev(planes)), onp.median(planes)) == 0
    with pytest.raises(RuntimeError, match="is not the half of"):
        _lib.optflow_up(dev(planes), (2 * H + 1, 2 * W))


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_warp_equals_the_twin(hip_lib, shape):
    """Three flows: one whose targets leave the image across all four borders, one exactly integer-valued, zero."""
    P, H, W = shape
    rng = np.random.default_rng(3 * H + W)
    I0, I1 = (rng.uniform(0, 255, shape).astype(np.float32) for _ in range(2))
    ys, xs = np.mgrid[0:H, 0:W]
    away = np.stack([np.where(xs < W / 2, -1.0, 1.0) * rng.uniform(0, 0.7 * W, shape), np.where(ys < H / 2, -1.0, 1.0) * rng.uniform(0, 0.7 * H, shape)])
    whole = np.stack([rng.integers(-3, 4, shape), rng.integers(-3, 4, shape)])
    for name, u in (("away", away), ("integer", whole), ("zero", np.zeros((2,) + shape))):
        u = u.astype(np.float32)
        if name == "away":
            tx, ty = xs + u[0], ys + u[1]
            assert (tx < 0).any() and (tx > W - 1).any() and (ty < 0).any() and (ty > H - 1).any()
            assert ((tx > 0) & (tx < W - 1) & (ty > 0) & (ty < H - 1)).any()
        want = onp.warp(I0, I1, u)
        got = _lib.optflow_warp(dev(I0), dev(I1), dev(u))
        bad = [same_bits(got[i], want[i]) for i in range(5)]
        print(f"{shape} {name}: differing values per plane (Ix, Iy, g, rho_c, I1w) {bad}")
        assert bad == [0] * 5, name
        if name == "zero":
            assert np.array_equal(want[4], I1)                  # the sample at a pixel is the pixel


# ---- the iteration ----
@pytest.mark.parametrize("shape", ITER_SHAPES)
def test_one_iteration_equals_the_twin_on_both_routes(hip_lib, shape):
    c, want = iter_case(shape), twin_iterations(shape, 1)
    if shape[1] * shape[2] > 1000:                              # every branch of the threshold step, and the border rules, are in play
        rho = (c["consts"][3] + c["consts"][0] * c["state"][0]) + c["consts"][1] * c["state"][1]
        lg = np.float32(PARAMS["lam"]) * np.float32(PARAMS["theta"]) * c["consts"][2]
        assert (rho < -lg).any() and (rho > lg).any() and ((np.abs(rho) <= lg) & (lg > 0)).any() and (c["consts"][2] == 0).any()
    assert np.abs(want[:2] - c["state"][:2]).max() > 0.1 and np.abs(want[2:] - c["state"][2:]).max() > 0.01
    for route in (dict(fused=False), dict(fused=True)):
        got = run_iterations(shape, 1, **route)
        bad = [same_bits(got[i], want[i]) for i in range(6)]
        print(f"{shape} {route}: differing values per plane (u1, u2, p11, p12, p21, p22) {bad}")
        assert bad == [0] * 6, route


@pytest.mark.parametrize("iters", [1, K, K + 1, 2 * K + 3])
@pytest.mark.parametrize("shape", ITER_SHAPES + [SMALL])
def test_fused_equals_plain(hip_lib, shape, iters):
    """k iterations per launch on tiles with a halo of k against `iters` launches of the plain kernel: the same bits, also where
    iters is no multiple of k (a last launch runs the rest)."""
    plain, fused = run_iterations(shape, iters, fused=False), run_iterations(shape, iters, fused=True)
    assert same_bits(fused, plain.cpu().numpy()) == 0
    assert same_bits(run_iterations(shape, iters, fused=True, tile=T, k=K), plain.cpu().numpy()) == 0      # the same route, by name
    if iters == 2 * K + 3:
        assert same_bits(plain, twin_iterations(shape, iters)) == 0


@pytest.mark.parametrize("tile,k", _lib.OPTFLOW_PAIRS)
def test_every_built_tile_equals_plain(hip_lib, tile, k):
    for shape in ((1, tile + 3, 2 * tile + 5), SMALL):
        for iters in (k + 1, 2 * k + 3):
            plain, fused = run_iterations(shape, iters, fused=False), run_iterations(shape, iters, fused=True, tile=tile, k=k)
            assert same_bits(fused, plain.cpu().numpy()) == 0, (shape, iters)


def test_iterate_uses_the_callers_second_buffer(hip_lib):
    shape = ITER_SHAPES[1]
    c = iter_case(shape)
    state, other = dev(c["state"]), torch.full((6,) + shape, 7.0, device=DEV)
    out = _lib.optflow_iterate(dev(c["consts"]), state, 2 * K, fused=True, other=other, **PARAMS)      # two launches: back in `state`
    assert out is state and same_bits(out, twin_iterations(shape, 2 * K)) == 0
    out = _lib.optflow_iterate(dev(c["consts"]), dev(c["state"]), 3, fused=False, other=other, **PARAMS)
    assert out is other and same_bits(out, twin_iterations(shape, 3)) == 0
    with pytest.raises(RuntimeError, match="NSFF_ERR_INVALID"):
        _lib.optflow_iterate(dev(c["consts"]), state, 3, fused=True, tile=48, k=4, **PARAMS)


# ---- the whole pipeline ----
def colour_frames(grey):
    """(n, H, W) fp32 on 0..255 -> (n, H, W, 3) uint8, the channels differently weighted."""
    return np.stack([np.rint(grey), np.rint(0.8 * grey + 20), np.rint(255 - 0.9 * grey)], -1).astype(np.uint8)


def pipeline_case():
    if "pipeline" not in _CASES:
        pairs = [onp.make_pair(72, 96, seed=s) for s in (1, 2)]
        grey0, grey1 = (np.concatenate([p[k] for p in pairs]) for k in ("images0", "images1"))
        c = dict(grey0=grey0, grey1=grey1, rgb0=colour_frames(grey0), rgb1=colour_frames(grey1))
        kw = dict(levels=3, warps=2, iters=10)
        c["twin_rgb"] = onp.optical_flow(c["rgb0"], c["rgb1"], median_filter=True, **kw)
        c["twin_grey"] = onp.optical_flow(grey0, grey1, median_filter=False, **kw)
        for v in c.values():
            v.setflags(write=False)
        _CASES["pipeline"] = c
    return _CASES["pipeline"]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("median", [True, False])
def test_whole_pipeline_equals_the_twin(hip_lib, median, fused):
    """2 pairs of 72 x 96, 3 levels, 2 warps, 10 iterations: colour bytes with the median, grey floats without."""
    c = pipeline_case()
    a, b, want = (c["rgb0"], c["rgb1"], c["twin_rgb"]) if median else (c["grey0"], c["grey1"], c["twin_grey"])
    got = optflow.optical_flow(dev(a), dev(b), levels=3, warps=2, iters=10, median=median, fused=fused)
    assert tuple(got.shape) == (2, 72, 96, 2) and got.is_cuda and got.dtype == torch.float32
    bad = same_bits(got, want)
    print(f"median {median} fused {fused}: {bad} of {want.size} values differ; mean |flow| {np.abs(want).mean():.3f} px")
    assert bad == 0 and np.abs(want).mean() > 0.5
    if fused:                                                   # a pair alone is the pair inside the batch; None is a built route
        alone = optflow.optical_flow(dev(a[1:]), dev(b[1:]), levels=3, warps=2, iters=10, median=median, fused=fused)
        assert torch.equal(alone[0], got[1])
        assert torch.equal(optflow.optical_flow(dev(a), dev(b), levels=3, warps=2, iters=10, median=median), got)
        assert optflow.default_route(2, 72, 96) == (16, 2)      # (a small batch: None took the small tile)


def test_accuracy_on_the_two_motion_pair(hip_lib):
    """The 144 x 256 two-motion pair (background (-2, 0.7) px, a disc (3, -1.5) px), 4 levels, 5 warps, 30 iterations, median on.
    Condition: the mean end-point error over the pixels more than 6 px from the disc's rim and more than 8 px from the image
    border is at most one tenth of the zero flow's error over the same pixels.

    The fp32 twin alone (tests/test_optflow_host.py checks it on the CPU): 0.01259 px against 2.501 px; the same code in float64:
    0.01260 px.  The GPU result has the twin's bits, so it has the twin's value."""
    pair = onp.make_pair(144, 256)
    kw = dict(levels=4, warps=5, iters=30)
    want = onp.optical_flow(pair["images0"], pair["images1"], **kw)
    got = optflow.optical_flow(dev(pair["images0"]), dev(pair["images1"]), **kw)
    epe, zero = onp.interior_epe(got.cpu().numpy(), pair)
    twin_epe, _ = onp.interior_epe(want, pair)
    print(f"interior end-point error {epe:.5f} px (twin {twin_epe:.5f}), zero flow {zero:.4f} px; {same_bits(got, want)} values differ")
    assert epe <= 0.1 * zero
    assert same_bits(got, want) == 0 and epe == twin_epe
    assert torch.equal(optflow.optical_flow(dev(pair["images0"]), dev(pair["images1"]), fused=not optflow.DEFAULT_FUSED, **kw), got)


# ---- conventions ----
def test_sequence_flows_follow_the_reference_convention(hip_lib):
    c = pipeline_case()
    images = dev(np.concatenate([c["rgb0"][:1], c["rgb1"][:1], c["rgb0"][1:]]))       # three frames
    kw = dict(levels=3, warps=2, iters=10)
    out = optflow.sequence_flows(images, **kw)
    assert sorted(out) == ["flows_bw", "flows_fw", "valid"]
    fw, bw = out["flows_fw"], out["flows_bw"]
    assert tuple(fw.shape) == tuple(bw.shape) == (3, 72, 96, 2) and fw.dtype == bw.dtype == torch.float32
    assert not fw[2].any() and not bw[0].any() and fw[:2].abs().mean() > 0.5 and bw[1:].abs().mean() > 0.5     # zero ends
    assert torch.equal(fw[:2], optflow.optical_flow(images[:2], images[1:], **kw))
    assert torch.equal(bw[1:], optflow.optical_flow(images[1:], images[:2], **kw))
    assert same_bits(fw[0], c["twin_rgb"][0]) == 0             # frame 0 -> 1 is the pipeline case's first pair
    valid = motion.flow_consistency(fw, bw)
    assert torch.equal(out["valid"], valid) and valid.dtype == torch.uint8 and 0.5 < valid[0, 0].float().mean() <= 1
    assert not valid[2, 0].any() and not valid[0, 1].any()
    assert sorted(optflow.sequence_flows(images, check=False, **kw)) == ["flows_bw", "flows_fw"]
    # ... and into the ray records without conversion: columns 12..15 are pixel + flow
    g = torch.Generator(DEV).manual_seed(0)
    disps = torch.rand(3, 72, 96, device=DEV, generator=g)
    masks = torch.full((3, 72, 96), 255, dtype=torch.uint8, device=DEV)
    K = np.array([[100.0, 0, 48], [0, 100.0, 36], [0, 0, 1]])
    poses = np.tile(np.eye(4)[:3], (3, 1, 1))
    with_flow = frames.build_records(K, poses, images, disps, masks, fw, bw)
    without = frames.build_records(K, poses, images, disps, masks, torch.zeros_like(fw), torch.zeros_like(bw))
    assert tuple(with_flow.shape) == (3, 72 * 96, _lib.RAY_RECORD) and torch.isfinite(with_flow).all()
    moved = (with_flow != without).any(1)
    assert moved[0, 12:16].tolist() == [True, True, False, False] and moved[2, 12:16].tolist() == [False, False, True, True]
    assert not moved[:, :12].any()


# ---- capture ----
@pytest.mark.parametrize("fused", [False, True])
def test_a_call_is_capturable(hip_lib, fused):
    """No synchronisation and no allocation inside nsff_optflow: one call recorded into a graph on a single stream and replayed on
    new frames equals the eager result."""
    c = pipeline_case()
    kw = dict(levels=3, warps=2, iters=10, median=True, fused=fused)
    a, b = dev(c["grey0"]), dev(c["grey1"])
    flow = torch.zeros(2, 72, 96, 2, device=DEV)
    scratch = torch.empty(optflow.scratch_bytes(2, 72, 96, 3), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.optflow(a, b, flow, scratch=scratch, **kw)         # warm-up outside the graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = flow.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.optflow(a, b, flow, scratch=scratch, **kw)
    a.copy_(dev(c["grey1"])), b.copy_(dev(c["grey0"]))         # new data: the pairs the other way round
    flow.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = optflow.optical_flow(dev(c["grey1"]), dev(c["grey0"]), **kw)
    assert torch.equal(flow, eager) and not torch.equal(flow, first) and flow.abs().mean() > 0.5
