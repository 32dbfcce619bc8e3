"""MI355X checks of nsff_disparity_span (csrc/parallax.hip) against the numpy fp32 twin tests/parallax_numpy.py, against
nsff_disparity_sparse at span 1, and of depth.triangulate / disparity_maps with a span on top of it.  Nothing is read from outside
the repository.

Every step is a single fp32 operation that numpy rounds the same way, so every comparison is for EQUALITY OF BITS at every pixel,
and the votes and the known-pixel counts are equal integers.  The method's coverage and accuracy are conditions on the twin
(tests/test_parallax_host.py) and, by bit equality, on the GPU result."""
import numpy as np
import pytest
import torch

import disparity_numpy as dnp
import parallax_numpy as pnp
from nsff_pl_amd import _lib, depth

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
f32 = np.float32
# a 1-pixel frame alone; odd sizes, odd H * W (no frame but the first starts on a quad); several workgroups a frame with a ragged last one
SHAPES = [(1, 1, 1), (4, 19, 33), (6, 37, 71), (5, 129, 511)]
SPANS = [1, 2, 3, 8]                                              # 8 is longer than any sequence here
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
    """In the manner of test_disparity_gpu.py's case: flows that mostly follow the parallax of a random disparity map, sprinkled with
    unknown, NaN and infinite values, flows that leave the image and flows that put the point behind the cameras; where the sequence
    allows, one pair of coincident camera centres (frames 1 and 2) and one frame without a static pixel (frame 1); random valid and
    masks, dense enough that chains survive several hops.  Shared, read-only."""
    if shape in _CASES:
        return _CASES[shape]
    F, H, W = shape
    rng = np.random.default_rng(1000 * F + 10 * H + W + 7)
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
    flows[kind < 0.01] = 1e10                                     # unknown, the Middlebury way
    flows[(kind >= 0.01) & (kind < 0.015), 0] = np.nan
    flows[(kind >= 0.015) & (kind < 0.02), 1] = np.inf
    flows[(kind >= 0.02) & (kind < 0.025), 0] = -np.inf
    away = (kind >= 0.025) & (kind < 0.045)                       # far out of the image, all four ways
    flows[away] = rng.choice([-1.0, 1.0], (int(away.sum()), 2)).astype(f32) * rng.uniform(W + H, 4 * (W + H), (int(away.sum()), 2)).astype(f32)
    back = (kind >= 0.045) & (kind < 0.065)                       # against the parallax: behind the cameras
    flows[back] = -flows[back]
    flows[(kind >= 0.065) & (kind < 0.08)] = 0.0                  # no parallax at all
    valid = (rng.random((F, 2, H, W)) < 0.9).astype(np.uint8)
    masks = np.where(rng.random((F, H, W)) < 0.85, 255, 0).astype(np.uint8)
    if F >= 2:
        masks[1] = 0
    c = dict(K=K, poses=poses, fw=flows[0], bw=flows[1], valid=valid, masks=masks, Pm={}, twin={})
    for v in (c["fw"], c["bw"], valid, masks):
        v.setflags(write=False)
    _CASES[shape] = c
    return c


def rows_of(shape, span):
    c = case(shape)
    if span not in c["Pm"]:
        Pm = depth.parallax_matrices(c["K"], c["poses"], span=span).numpy()
        c["Pm"][span] = Pm[:, :, None] if span == 1 else Pm
    return c["Pm"][span]


def twin(shape, span, given):
    c = case(shape)
    if (span, given) not in c["twin"]:
        kw = dict(valid=c["valid"], masks=c["masks"]) if given == "with" else {}
        c["twin"][span, given] = pnp.sparse_span(c["fw"], c["bw"], rows_of(shape, span), span, min_parallax=MIN_PARALLAX, **kw)
    return c["twin"][span, given]


def run(shape, span, given, scratch=None):
    """One call with sentinels in every output."""
    c = case(shape)
    F, H, W = shape
    kw = dict(valid=dev(c["valid"]), masks=dev(c["masks"])) if given == "with" else {}
    counts = torch.full((F,), -1, dtype=torch.int64, device=DEV)
    votes = torch.full(shape, 201, dtype=torch.uint8, device=DEV)
    out = (torch.full(shape, -7.0, device=DEV), torch.full(shape, float("nan"), device=DEV))
    n, cc, v = _lib.disparity_span(dev(c["fw"]), dev(c["bw"]), dev(rows_of(shape, span)), span, min_parallax=MIN_PARALLAX, counts=counts,
                                   votes=votes, scratch=scratch, out=out, **kw)
    assert v is votes and n is out[0] and cc is out[1]
    return n, cc, votes, counts


@pytest.mark.parametrize("given", ["with", "without"])
@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("shape", SHAPES)
def test_span_equals_the_twin(hip_lib, shape, span, given):
    F, H, W = shape
    want_n, want_c, want_votes, want_counts = twin(shape, span, given)
    scratch = torch.zeros(_lib.disparity_span_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    for turn in range(2):                                         # the scratch is used twice and left zero
        n, cc, votes, counts = run(shape, span, given, scratch)
        bad = (same_bits(n, want_n), same_bits(cc, want_c), int((votes.cpu().numpy() != want_votes).sum()))
        if turn == 0:
            print(f"{shape} span {span} {given} valid / masks: differing values (n, c, votes) {bad}; known per frame "
                  f"{want_counts.tolist()} of {H * W}; pixels by votes {np.bincount(want_votes.ravel()).tolist()}")
        assert bad == (0, 0, 0) and counts.cpu().numpy().tolist() == want_counts.tolist(), turn
        assert not scratch.any(), turn
    # what the twin's result says about the case
    assert want_votes.max() <= 2 * span and np.array_equal(want_counts, (want_c > 0).reshape(F, -1).sum(1))
    assert not (want_c > 0)[want_votes == 0].any()
    if F == 1:
        assert not want_counts.any() and not want_votes.any()     # a single frame has no neighbour: nothing is known
    if F >= 2 and given == "with":
        assert want_counts[0] > 0 and want_counts[1] == 0         # frame 1 has no static pixel
    if H * W > 500:
        if span > 1:                                              # more votes than span 1 casts: chains that outlived a hop
            assert want_votes.astype(np.int64).sum() > twin(shape, 1, given)[2].astype(np.int64).sum()
        if given == "without":
            assert 0.3 * H * W < want_counts[0] < H * W           # most pixels are measured, the sprinkled ones are not


@pytest.mark.parametrize("given", ["with", "without"])
@pytest.mark.parametrize("shape", SHAPES)
def test_span_1_gives_the_bits_of_the_one_frame_kernel(hip_lib, shape, given):
    c = case(shape)
    F, H, W = shape
    kw = dict(valid=dev(c["valid"]), masks=dev(c["masks"])) if given == "with" else {}
    counts = torch.full((F,), -1, dtype=torch.int64, device=DEV)
    Pm1 = depth.parallax_matrices(c["K"], c["poses"])
    want_n, want_c = _lib.disparity_sparse(dev(c["fw"]), dev(c["bw"]), Pm1.to(DEV), min_parallax=MIN_PARALLAX, counts=counts, **kw)
    n, cc, votes, got_counts = run(shape, 1, given)
    assert same_bits(n, want_n.cpu().numpy()) == 0 and same_bits(cc, want_c.cpu().numpy()) == 0 and torch.equal(got_counts, counts)
    assert int(votes.max()) <= 2 and not bool((cc > 0)[votes == 0].any())
    # without votes, counts and scratch the call computes the same n and c
    n2, c2, _ = _lib.disparity_span(dev(c["fw"]), dev(c["bw"]), dev(rows_of(shape, 1)), 1, min_parallax=MIN_PARALLAX, **kw)
    assert torch.equal(n2, n) and torch.equal(c2, cc)


@pytest.mark.parametrize("shape", [(4, 9, 1), (4, 7, 2), (4, 1, 6)])
def test_narrow_frames_hop_along_their_only_columns(hip_lib, shape):
    """One and two columns (the right tap is the left one again, or always the last column) and one row: flows of whole and half
    pixels, so that chains land inside such a frame at all, and min_parallax 0, so that they vote."""
    F, H, W = shape
    rng = np.random.default_rng(10 * H + W)
    K = np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1.0]])
    poses = np.tile(np.eye(4)[:3], (F, 1, 1))
    poses[:, :, 3] = np.stack([0.12 * np.arange(F), rng.uniform(-0.01, 0.01, F), rng.uniform(-0.02, 0.02, F)], -1)
    Pm = depth.parallax_matrices(K, poses, span=3).numpy()
    steps = np.array([-1.0, -0.5, 0.0, 0.0, 0.5, 1.0], f32)
    fw, bw = (rng.choice(steps, (F, H, W, 2)) for _ in range(2))
    fw[rng.random((F, H, W)) < 0.05] = 1e10
    valid = (rng.random((F, 2, H, W)) < 0.9).astype(np.uint8)
    masks = np.where(rng.random((F, H, W)) < 0.9, 255, 0).astype(np.uint8)
    for kw in (dict(valid=valid, masks=masks), {}):
        want_n, want_c, want_votes, want_counts = pnp.sparse_span(fw, bw, Pm, 3, min_parallax=0.0, **kw)
        assert want_votes.max() >= 3                              # chains that outlived a hop
        counts = torch.full((F,), -1, dtype=torch.int64, device=DEV)
        n, c, votes = _lib.disparity_span(dev(fw), dev(bw), dev(Pm), 3, min_parallax=0.0, counts=counts, **{k: dev(v) for k, v in kw.items()})
        assert same_bits(n, want_n) == 0 and same_bits(c, want_c) == 0 and np.array_equal(votes.cpu().numpy(), want_votes)
        assert counts.cpu().numpy().tolist() == want_counts.tolist()


def test_the_longer_chains_change_the_result(hip_lib):
    """The spans are different measurements, not one: on the largest case more pixels vote more often as the span grows."""
    shape = SHAPES[3]
    votes = [twin(shape, span, "without")[2].astype(np.int64).sum() for span in (1, 2, 3)]
    assert votes[0] < votes[1] < votes[2]
    assert same_bits(run(shape, 3, "without")[0], twin(shape, 1, "without")[0]) != 0


# ---- the Python layer ----
def test_triangulate_and_disparity_maps_with_a_span(hip_lib):
    sc = dnp.make_scene(4, 64, 96, noise=0.05, seed=0)
    inp = pnp.scene_inputs(sc)
    fw, bw, masks, valid = dev(sc["flows_fw"]), dev(sc["flows_bw"]), dev(inp["masks"]), dev(inp["valid"])
    K, poses = sc["K"], sc["poses"]
    # triangulate(span=3) is the _lib call on parallax_matrices(span=3)
    tri = depth.triangulate(fw, bw, K, poses, valid=valid, masks=masks, span=3)
    assert sorted(tri) == ["conf", "counts", "known", "sparse", "votes"]
    counts = torch.empty(4, dtype=torch.int64, device=DEV)
    n, c, votes = _lib.disparity_span(fw, bw, depth.parallax_matrices(K, poses, span=3).to(DEV), 3, valid=valid, masks=masks, counts=counts)
    assert torch.equal(tri["conf"], c) and torch.equal(tri["votes"], votes) and torch.equal(tri["counts"], counts)
    assert torch.equal(tri["known"], c > 0) and torch.equal(tri["sparse"], torch.where(c > 0, n / c, torch.zeros_like(n)))
    assert int(votes.max()) == 3 and tri["votes"].dtype == torch.uint8          # four frames: three neighbours, 3 + 0 or 2 + 1
    # span = 1 is the route it always was
    one = depth.triangulate(fw, bw, K, poses, valid=valid, masks=masks)
    n1, c1 = _lib.disparity_sparse(fw, bw, depth.parallax_matrices(K, poses).to(DEV), valid=valid, masks=masks)
    assert sorted(one) == ["conf", "counts", "known", "sparse"] and torch.equal(one["conf"], c1)
    # disparity_maps(span=2): a finite dense map whose sparse part is the twin's
    Pm = pnp.rows(K, poses, 2).astype(f32)
    want_n, want_c, want_votes, want_counts = pnp.sparse_span(sc["flows_fw"], sc["flows_bw"], Pm, 2, **inp)
    out = depth.disparity_maps(dev(sc["guide"]), fw, bw, K, poses, masks=masks, valid=valid, sigma=0.05, span=2)
    assert sorted(out) == ["conf", "disps", "known", "sparse", "stats", "votes"]
    d = out["disps"]
    assert tuple(d.shape) == (4, 64, 96) and d.dtype == torch.float32 and bool(torch.isfinite(d).all()) and bool((d > 0).all())
    known = want_c > 0
    assert same_bits(out["conf"], want_c) == 0 and np.array_equal(out["known"].cpu().numpy(), known)
    with np.errstate(all="ignore"):
        want_sparse = np.where(known, want_n / want_c, f32(0)).astype(f32)
    assert same_bits(out["sparse"], want_sparse) == 0 and np.array_equal(out["votes"].cpu().numpy(), want_votes)
    assert out["stats"].counts.tolist() == want_counts.tolist() and (want_counts > 0).all()
    ratio, method, const = dnp.static_error(d.cpu().numpy(), sc)
    print(f"span 2 on the scene: ratio {ratio:.4f} (method {method:.5f}, constant {const:.5f})")
    # the same map from the twin's sparse part through the dense twin, so the fill is the one that is tested elsewhere
    assert same_bits(d, dnp.dense(want_n, want_c, sc["guide"], levels=3, iters=30, lam=8.0, sigma=0.05)) == 0
