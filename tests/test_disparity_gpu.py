"""MI355X checks of the disparity kernels (csrc/depth.hip) against the numpy fp32 twin tests/disparity_numpy.py, and of
depth.triangulate / densify / disparity_maps / sequence_geometry on top of them.  Nothing is read from outside the repository.

Every stage is a chain of single fp32 operations that numpy rounds the same way (add, subtract, multiply, divide, comparisons), so
every comparison is for EQUALITY OF BITS at every pixel, and the known-pixel counts are equal integers.  The accuracy of the method
itself is a condition on the twin (tests/test_disparity_host.py) and, by bit equality, on the GPU result."""
import numpy as np
import pytest
import torch

import disparity_numpy as dnp
import optflow_numpy as onp
from nsff_pl_amd import _lib, depth, frames
from nsff_pl_amd.sampling import RayBank

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
f32 = np.float32
SHAPES = [(1, 1, 1), (3, 19, 33), (2, 37, 71), (2, 129, 511)]     # a 1-pixel image; odd sizes all the way up the pyramid; ragged tiles
PARAMS = dict(lam=8.0, sigma=12.75)
MIN_PARALLAX = 0.5

_CASES = {}


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


def case(shape):
    """Flows that mostly follow the parallax of a random disparity map, sprinkled with unknown, NaN and infinite values, flows that
    leave the image and flows that put the point behind the cameras; where the sequence allows, one pair of coincident camera
    centres (frames 1 and 2 of three) and one frame without a static pixel (frame 1).  With the twin's results; shared, read-only."""
    if shape in _CASES:
        return _CASES[shape]
    F, H, W = shape
    rng = np.random.default_rng(1000 * F + 10 * H + W)
    K = np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1.0]])
    poses = np.zeros((F, 3, 4))
    for t in range(F):
        poses[t, :, :3] = dnp.mnp.rotation(*rng.uniform(-0.01, 0.01, 3))
        poses[t, :, 3] = [0.12 * t, rng.uniform(-0.01, 0.01), rng.uniform(-0.02, 0.02)]
    if F >= 3:
        poses[2, :, 3] = poses[1, :, 3]
    rows = depth.parallax_matrices(K, poses, rounded=False)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x = np.stack([xs, ys, np.ones_like(xs)], -1)
    flows = np.zeros((2, F, H, W, 2))
    for f in range(F):
        delta = rng.uniform(0.1, 0.5, (H, W))
        for d in range(2):
            if rows[f, d].any():
                q = delta[..., None] * rows[f, d, 9:] + x @ rows[f, d, :9].reshape(3, 3).T
                flows[d, f] = q[..., :2] / q[..., 2:] - x[..., :2] + rng.normal(0, 0.05, (H, W, 2))
            else:
                flows[d, f] = rng.normal(0, 2.0, (H, W, 2))
    flows = flows.astype(f32)
    kind = rng.random((2, F, H, W))
    flows[kind < 0.03] = 1e10                                     # unknown, the Middlebury way
    flows[(kind >= 0.03) & (kind < 0.04), 0] = np.nan
    flows[(kind >= 0.04) & (kind < 0.05), 1] = np.inf
    flows[(kind >= 0.05) & (kind < 0.06), 0] = -np.inf
    away = (kind >= 0.06) & (kind < 0.09)                         # far out of the image, all four ways
    flows[away] = rng.choice([-1.0, 1.0], (int(away.sum()), 2)).astype(f32) * rng.uniform(W + H, 4 * (W + H), (int(away.sum()), 2)).astype(f32)
    back = (kind >= 0.09) & (kind < 0.12)                         # against the parallax: behind the cameras
    flows[back] = -flows[back]
    flows[(kind >= 0.12) & (kind < 0.14)] = 0.0                   # no parallax at all
    valid = (rng.random((F, 2, H, W)) < 0.8).astype(np.uint8)
    masks = np.where(rng.random((F, H, W)) < 0.7, 255, 0).astype(np.uint8)
    if F >= 2:
        masks[1] = 0
    grey = (rng.uniform(0, 255, shape) * (rng.random(shape) < 0.5) + 40 * np.sin(0.3 * xs + 0.2 * ys) + 100).astype(f32)
    grey[:, : H // 2, : W // 3] = 77.0                            # a flat patch: weights of exactly 1
    c = dict(K=K, poses=poses, Pm=rows.astype(f32), fw=flows[0], bw=flows[1], valid=valid, masks=masks, grey=grey)
    c["with"] = dnp.sparse(c["fw"], c["bw"], c["Pm"], valid=valid, masks=masks, min_parallax=MIN_PARALLAX)
    c["without"] = dnp.sparse(c["fw"], c["bw"], c["Pm"], min_parallax=MIN_PARALLAX)
    n, cc, _ = c["without"]
    pyr = [(cc, n, grey)]
    while pyr[-1][0].shape[1:] != (1, 1):
        pyr.append(dnp.push(*pyr[-1]))
    c["pyramid"] = pyr
    c["state"] = (rng.normal(0.3, 0.3, shape)).astype(f32)        # a random state for the relaxation: both signs
    c["relaxed"] = {}
    for v in (c["fw"], c["bw"], valid, masks, grey, c["state"]):
        v.setflags(write=False)
    _CASES[shape] = c
    return c


def twin_relaxed(shape, iters):
    c = case(shape)
    if iters not in c["relaxed"]:
        done = max((k for k in c["relaxed"] if k < iters), default=0)
        n, cc, _ = c["without"]
        c["relaxed"][iters] = dnp.relax(c["relaxed"][done] if done else c["state"], n, cc, c["grey"], iters=iters - done, **PARAMS)
    return c["relaxed"][iters]


def run_relax(shape, iters, **route):
    c = case(shape)
    n, cc, _ = c["without"]
    return _lib.disparity_relax(dev(c["state"]), dev(n), dev(cc), dev(c["grey"]), iters, **PARAMS, **route)


# ---- the triangulation ----
@pytest.mark.parametrize("given", ["with", "without"])
@pytest.mark.parametrize("shape", SHAPES)
def test_sparse_equals_the_twin(hip_lib, shape, given):
    c = case(shape)
    F, H, W = shape
    want_n, want_c, want_counts = c[given]
    kw = dict(valid=dev(c["valid"]), masks=dev(c["masks"])) if given == "with" else {}
    counts = torch.full((F,), -1, dtype=torch.int64, device=DEV)
    n, cc = _lib.disparity_sparse(dev(c["fw"]), dev(c["bw"]), dev(c["Pm"]), min_parallax=MIN_PARALLAX, counts=counts, **kw)
    bad = (same_bits(n, want_n), same_bits(cc, want_c))
    print(f"{shape} {given} valid / masks: differing values (n, c) {bad}; known per frame {want_counts.tolist()} of {H * W}")
    assert bad == (0, 0) and counts.cpu().numpy().tolist() == want_counts.tolist()
    assert np.array_equal(want_counts, (want_c > 0).reshape(F, -1).sum(1))
    if F == 1:
        assert not want_counts.any()                              # a single frame has no neighbour: nothing is known
    if F >= 2 and given == "with":
        assert want_counts[0] > 0 and want_counts[1] == 0         # frame 1 has no static pixel
    if H * W > 500 and given == "without":
        assert 0.3 * H * W < want_counts[0] < H * W               # most pixels are measured, the sprinkled ones are not
    if F == 3 and given == "without":
        assert want_counts[1] > 0 and want_counts[2] == 0         # frame 2 has only the coincident neighbour
    # a frame alone is the frame in the batch: the rows carry everything about its neighbours
    if F >= 2:
        one = torch.zeros(1, dtype=torch.int64, device=DEV)
        kw1 = dict(valid=dev(c["valid"][:1]), masks=dev(c["masks"][:1])) if given == "with" else {}
        n1, c1 = _lib.disparity_sparse(dev(c["fw"][:1]), dev(c["bw"][:1]), dev(c["Pm"][:1]), min_parallax=MIN_PARALLAX, counts=one, **kw1)
        assert torch.equal(n1[0], n[0]) and torch.equal(c1[0], cc[0]) and int(one[0]) == want_counts[0]


# ---- the pyramid ----
@pytest.mark.parametrize("shape", SHAPES)
def test_push_and_pull_equal_the_twin(hip_lib, shape):
    pyr = case(shape)["pyramid"]
    level = tuple(dev(a) for a in pyr[0])
    gpu = [level]
    for want in pyr[1:]:
        level = _lib.disparity_push(*level)
        gpu.append(level)
        bad = [same_bits(g, w) for g, w in zip(level, want)]
        assert bad == [0, 0, 0], (want[0].shape, bad)
    assert tuple(gpu[-1][0].shape[1:]) == (1, 1) and len(gpu) == _lib.disparity_levels(*shape[1:])
    want, got = None, None
    for l in range(len(pyr) - 1, -1, -1):                         # down from the top: the top has no parent
        want = dnp.pull(pyr[l][0], pyr[l][1], want)
        got = _lib.disparity_pull(gpu[l][0], gpu[l][1], got)
        assert same_bits(got, want) == 0, pyr[l][0].shape
        if l > 0:
            hw = pyr[l - 1][0].shape[1:]
            assert same_bits(_lib.disparity_pull(None, None, got, hw), dnp.pull(None, None, want, hw)) == 0, hw
    if shape[1] * shape[2] > 500:
        empty = pyr[0][0] == 0
        assert empty.any() and (want[0][empty[0]] > 0).all()      # holes at the finest level were filled from above


# ---- the relaxation ----
@pytest.mark.parametrize("shape", SHAPES)
def test_one_relax_iteration_equals_the_twin_on_both_routes(hip_lib, shape):
    c, want = case(shape), twin_relaxed(shape, 1)
    if shape[1] * shape[2] > 500:
        assert np.abs(want - c["state"]).max() > 0.1
    for route in (dict(fused=False), dict(fused=True), dict(fused=True, tile=16, k=2)):
        bad = same_bits(run_relax(shape, 1, **route), want)
        print(f"{shape} {route}: {bad} of {want.size} values differ")
        assert bad == 0, route


@pytest.mark.parametrize("tile,k", _lib.DISPARITY_PAIRS)
def test_fused_equals_plain_for_every_built_tile(hip_lib, tile, k):
    """k iterations per launch on tiles with a halo of k against `iters` launches of the plain kernel: the same bits, also where
    iters is no multiple of k (a last launch runs the rest) and where it is 0 (no launch: the state itself)."""
    big = (2, 2 * tile + 3, 2 * tile + 5)                         # two tiles and a remainder in each axis
    for shape in ((2, 37, 71), big):
        for iters in (0, 1, k - 1, k, 2 * k + 3):
            plain = run_relax(shape, iters, fused=False)
            fused = run_relax(shape, iters, fused=True, tile=tile, k=k)
            assert same_bits(fused, plain.cpu().numpy()) == 0, (shape, iters)
            if iters == 0:
                assert same_bits(plain, case(shape)["state"]) == 0
            if iters == 2 * k + 3:
                assert same_bits(plain, twin_relaxed(shape, iters)) == 0, shape


def test_relax_uses_the_callers_second_buffer(hip_lib):
    shape = SHAPES[2]
    c = case(shape)
    n, cc, _ = c["without"]
    d, other = dev(c["state"]), torch.full(shape, 7.0, device=DEV)
    out = _lib.disparity_relax(d, dev(n), dev(cc), dev(c["grey"]), 3, fused=False, other=other, **PARAMS)
    assert out is other and same_bits(out, twin_relaxed(shape, 3)) == 0
    out = _lib.disparity_relax(dev(c["state"]), dev(n), dev(cc), dev(c["grey"]), 4, fused=True, tile=32, k=2, other=other, **PARAMS)
    assert out is not other and same_bits(out, twin_relaxed(shape, 4)) == 0
    with pytest.raises(RuntimeError, match="NSFF_ERR_INVALID"):
        _lib.disparity_relax(d, dev(n), dev(cc), dev(c["grey"]), 3, fused=True, tile=48, k=4, **PARAMS)


# ---- the whole densification ----
def twin_dense(shape, levels, iters):
    c = case(shape)
    key = ("dense", levels, iters)
    if key not in c:
        n, cc, _ = c["without"]
        c[key] = dnp.dense(n, cc, c["grey"], levels=levels, iters=iters, **PARAMS)
    return c[key]


@pytest.mark.parametrize("shape", SHAPES)
def test_dense_equals_the_twin_on_both_routes(hip_lib, shape):
    c = case(shape)
    F, H, W = shape
    n, cc, counts = c["without"]
    top = _lib.disparity_levels(H, W)
    runs = [(min(3, top), 7), (1, 0)] + ([(top, 2), (top - 1, 3)] if top > 3 and H * W < 5000 else [])
    for levels, iters in runs:
        want = twin_dense(shape, levels, iters)
        for route in (dict(fused=False), dict(fused=True), dict(fused=True, tile=16, k=2), dict(fused=True, tile=32, k=6)):
            out = torch.full(shape, -3.0, device=DEV)
            got = _lib.disparity_dense(dev(n), dev(cc), dev(c["grey"]), out, levels=levels, iters=iters, **PARAMS, **route)
            bad = same_bits(got, want)
            print(f"{shape} levels {levels} iters {iters} {route}: {bad} of {want.size} values differ")
            assert got is out and bad == 0, (levels, iters, route)
        for f in range(F):                                        # a frame without a known pixel is zero, every other one positive
            assert (want[f] > 0).all() if counts[f] else not want[f].any()
    with pytest.raises(RuntimeError, match="NSFF_ERR_INVALID"):
        _lib.disparity_dense(dev(n), dev(cc), dev(c["grey"]), torch.empty(shape, device=DEV), levels=top + 1, iters=1)
    if F >= 2:                                                    # a frame alone is the frame in the batch
        levels, iters = min(3, top), 7
        alone = _lib.disparity_dense(dev(n[:1]), dev(cc[:1]), dev(c["grey"][:1]), torch.empty((1, H, W), device=DEV), levels=levels,
                                     iters=iters, **PARAMS)
        assert same_bits(alone[0], twin_dense(shape, levels, iters)[0]) == 0


# ---- the Python layer ----
def scene_case():
    if "scene" not in _CASES:
        sc = dnp.make_scene(3, 64, 96, noise=0.05, seed=0)
        _CASES["scene"] = dict(scene=sc, twin=dnp.scene_disparity(sc))
    return _CASES["scene"]


def test_disparity_maps_equal_the_twin_and_repeat_their_bits(hip_lib):
    """The synthetic scene at (3, 64, 96) through depth.disparity_maps with the twin's masks and validity: the twin's bits, so the
    twin's accuracy (tests/test_disparity_host.py: ratio 0.1674 against the bound of one half), and the same bits from a second
    call that reuses the first one's scratch."""
    s = scene_case()
    sc, twin = s["scene"], s["twin"]
    args = (dev(sc["guide"]), dev(sc["flows_fw"]), dev(sc["flows_bw"]), sc["K"], sc["poses"])
    kw = dict(masks=dev(twin["masks"]), valid=dev(twin["valid"]), sigma=0.05)
    scratch = torch.empty(depth.scratch_bytes(3, 64, 96), dtype=torch.uint8, device=DEV)
    first = depth.disparity_maps(*args, scratch=scratch, **kw)
    assert sorted(first) == ["conf", "disps", "known", "sparse", "stats"]
    d = first["disps"]
    assert tuple(d.shape) == (3, 64, 96) and d.dtype == torch.float32 and d.is_cuda
    assert same_bits(d, twin["disps"]) == 0 and same_bits(first["conf"], twin["c"]) == 0
    ratio, method, const = dnp.static_error(d.cpu().numpy(), sc)
    print(f"ratio {ratio:.4f} (method {method:.5f}, constant {const:.5f})")
    assert ratio <= 0.5 and bool((d > 0).all()) and bool(torch.isfinite(d).all())
    stats = first["stats"]
    assert stats.counts.tolist() == twin["counts"].tolist() and np.array_equal(stats.known_fraction, twin["counts"] / (64 * 96))
    assert stats.empty_frames.size == 0 and torch.equal(first["known"], first["conf"] > 0)
    known = first["known"].cpu().numpy()
    assert same_bits(first["sparse"].cpu().numpy()[known], (twin["n"][known] / twin["c"][known]).astype(f32)) == 0
    second = depth.disparity_maps(*args, scratch=scratch, **kw)
    for key in ("disps", "sparse", "conf", "known"):
        assert torch.equal(first[key], second[key]), key
    for fused in (True, False, None):                             # every route, and a fresh scratch
        assert torch.equal(depth.disparity_maps(*args, fused=fused, **kw)["disps"], d), fused
    # the two halves by themselves
    tri = depth.triangulate(*args[1:], masks=kw["masks"], valid=kw["valid"])
    assert sorted(tri) == ["conf", "counts", "known", "sparse"] and torch.equal(tri["sparse"], first["sparse"]) and torch.equal(tri["conf"], first["conf"])
    filled = depth.densify(tri["sparse"], tri["conf"], args[0], sigma=0.05)
    assert bool((filled > 0).all()) and float((filled - d).abs().max()) < 1e-5      # (n = conf * sparse is rounded once more)
    # without a single static pixel a frame is all zero, and stats say so
    masks = kw["masks"].clone()
    masks[1] = 0
    out = depth.disparity_maps(*args, masks=masks, valid=kw["valid"], sigma=0.05)
    assert not out["disps"][1].any() and out["stats"].empty_frames.tolist() == [1] and torch.equal(out["disps"][0], d[0])


def test_a_dense_call_is_capturable(hip_lib):
    """No synchronisation and no allocation inside nsff_disparity_dense: one call recorded into a graph on a single stream and
    replayed on new data equals the eager result."""
    shape = SHAPES[2]
    c = case(shape)
    n, cc, _ = c["without"]
    gn, gc, gg = dev(n), dev(cc), dev(c["grey"])
    out = torch.zeros(shape, device=DEV)
    scratch = torch.empty(depth.scratch_bytes(*shape), dtype=torch.uint8, device=DEV)
    kw = dict(levels=3, iters=7, fused=True, scratch=scratch, **PARAMS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.disparity_dense(gn, gc, gg, out, **kw)               # warm-up outside the graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert same_bits(out, twin_dense(shape, 3, 7)) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.disparity_dense(gn, gc, gg, out, **kw)
    gg.copy_(dev(c["grey"][::-1].copy()))                         # new data: the guides of the two frames exchanged
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = _lib.disparity_dense(gn, gc, dev(c["grey"][::-1].copy()), torch.empty(shape, device=DEV), levels=3, iters=7, fused=False, **PARAMS)
    assert torch.equal(out, eager) and same_bits(out, twin_dense(shape, 3, 7)) != 0


def test_frames_to_ray_bank_in_one_session(hip_lib):
    """images + K + poses -> flows, masks and disparities -> RayBank.from_frames, with no file and no network: three frames of the
    optical-flow tests' textured pair, a camera that moves sideways."""
    pairs = onp.make_pair(72, 96, seed=1)
    grey = np.concatenate([pairs["images0"], pairs["images1"], pairs["images0"]])
    images = dev(np.stack([np.rint(grey), np.rint(0.8 * grey + 20), np.rint(255 - 0.9 * grey)], -1).astype(np.uint8))
    K = np.array([[100.0, 0, 48], [0, 100.0, 36], [0, 0, 1]])
    poses = np.tile(np.eye(4)[:3], (3, 1, 1))
    poses[:, 0, 3] = [0.0, 0.1, 0.0]
    out = depth.sequence_geometry(images, K, poses, flow_kw=dict(levels=3, warps=2, iters=10), mask_kw=dict(threshold=2.0))
    assert sorted(out) == ["conf", "disps", "flows_bw", "flows_fw", "known", "masks", "motion_stats", "stats", "valid"]
    d = out["disps"]
    assert tuple(d.shape) == (3, 72, 96) and d.dtype == torch.float32 and bool(torch.isfinite(d).all()) and bool((d >= 0).all())
    frac = out["stats"].known_fraction
    print(f"known fraction per frame {frac.tolist()}")
    assert frac.shape == (3,) and (frac > 0.05).all() and bool((d > 0).all())
    assert tuple(frames.resize_disps(d, (48, 36)).shape) == (3, 36, 48)
    records = frames.build_records(K, poses, images, d, out["masks"], out["flows_fw"], out["flows_bw"])
    assert tuple(records.shape) == (3, 72 * 96, _lib.RAY_RECORD) and bool(torch.isfinite(records).all())
    bank = RayBank.from_frames(K, poses, images, d, out["masks"], out["flows_fw"], out["flows_bw"], (96, 72), seed=0)
    assert bank is not None
