"""MI355X checks of nsff_motion_span and nsff_mask_propagate (csrc/motionspan.hip) against the numpy fp32 twin
tests/motionspan_numpy.py, against nsff_motion_maps at span 1, and of motion.motion_masks / propagate / depth.sequence_geometry on
top of them.  Nothing is read from outside the repository.

Every step is a single fp32 operation that numpy rounds the same way, so every comparison is for EQUALITY OF BITS AND BYTES at every
pixel, and all counts are equal integers.  What the method finds is a condition on the twin (tests/test_motionspan_host.py) and,
by bit equality, on the GPU result."""
import numpy as np
import pytest
import torch

import motion_numpy as mnp
import motionspan_numpy as msn
import test_motionspan_host as host
from nsff_pl_amd import _lib, depth, motion

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
f32 = np.float32
# a 1-pixel frame alone; odd sizes, odd H * W (no frame but the first starts on a quad); several workgroups a frame with a ragged last one
SHAPES = [(1, 1, 1), (4, 19, 33), (6, 37, 71), (5, 129, 511)]
SPANS = [1, 2, 3, 8]                                              # spans and reaches; 8 is longer than any sequence here
THRESHOLD = 1.0

_CASES = {}


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


def same_bytes(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (got.shape, want.shape, got.dtype, want.dtype)
    return int((got != want).sum())


def case(shape):
    """Flows that mostly follow the parallax of a random disparity map (so that they lie on their epipolar lines, with 0.05 px of
    noise), a tenth of them pushed off the line by a few pixels, sprinkled with unknown, NaN and infinite values, flows that leave
    the image and flows that land exactly on the image's rim; where the sequence allows, one pair of coincident camera centres
    (frames 1 and 2); a random valid, dense enough that chains survive several hops; a random mask to propagate.  Shared, read-only."""
    if shape in _CASES:
        return _CASES[shape]
    F, H, W = shape
    rng = np.random.default_rng(1000 * F + 10 * H + W + 11)
    K = np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1.0]])
    poses = np.zeros((F, 3, 4))
    for t in range(F):
        poses[t, :, :3] = mnp.rotation(*rng.uniform(-0.01, 0.01, 3))
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
    away = (kind >= 0.025) & (kind < 0.04)                        # far out of the image, all four ways
    flows[away] = rng.choice([-1.0, 1.0], (int(away.sum()), 2)).astype(f32) * rng.uniform(W + H, 4 * (W + H), (int(away.sum()), 2)).astype(f32)
    off = (kind >= 0.04) & (kind < 0.14)                          # off the line: moving
    flows[off] += rng.normal(0, 2.5, (int(off.sum()), 2)).astype(f32)
    grid = np.broadcast_to(np.stack([xs, ys], -1).astype(f32), (2, F, H, W, 2))
    for lo, corner in ((0.14, (W - 1, H - 1)), (0.15, (0, 0)), (0.16, (W - 1, 0))):      # exactly onto the rim: q is a corner of the image
        rim = (kind >= lo) & (kind < lo + 0.01)
        flows[rim] = np.array(corner, f32) - grid[rim]
    valid = (rng.random((F, 2, H, W)) < 0.9).astype(np.uint8)
    src = rng.choice(np.array([0, 1, 7, 255], np.uint8), (F, H, W), p=[0.1, 0.05, 0.05, 0.8])
    c = dict(K=K, poses=poses, fw=flows[0], bw=flows[1], valid=valid, src=src, Fm={}, span={}, prop={})
    for v in (c["fw"], c["bw"], valid, src):
        v.setflags(write=False)
    _CASES[shape] = c
    return c


def matrices(shape, span):
    c = case(shape)
    if span not in c["Fm"]:
        Fm = motion.fundamental_matrices(c["K"], c["poses"], span=span).numpy()
        c["Fm"][span] = Fm[:, :, None] if span == 1 else Fm
    return c["Fm"][span]


def twin_span(shape, span, given):
    c = case(shape)
    if (span, given) not in c["span"]:
        c["span"][span, given] = msn.motion_span(c["fw"], c["bw"], matrices(shape, span), msn.hop_scale(span), span,
                                                 valid=c["valid"] if given == "with" else None, threshold=THRESHOLD)
    return c["span"][span, given]


def twin_prop(shape, reach, given):
    c = case(shape)
    if (reach, given) not in c["prop"]:
        c["prop"][reach, given] = msn.propagate(c["src"], c["fw"], c["bw"], reach, valid=c["valid"] if given == "with" else None)
    return c["prop"][reach, given]


def run_span(fw, bw, Fm, span, valid, scratch=None, scale=None):
    """One call with sentinels in every output."""
    F, H, W = fw.shape[:3]
    err = torch.full((F, 2, H, W), -7.0, device=DEV)
    hops = torch.full((F, 2, H, W), 201, dtype=torch.uint8, device=DEV)
    raw = torch.full((F, H, W), 77, dtype=torch.uint8, device=DEV)
    counts = torch.full((F, 3), -1, dtype=torch.int64, device=DEV)
    got = _lib.motion_span(dev(fw), dev(bw), dev(Fm), dev(msn.hop_scale(span) if scale is None else scale), span, valid=dev(valid),
                           threshold=THRESHOLD, err=err, hops=hops, raw=raw, counts=counts, scratch=scratch)
    assert got is raw
    return err, hops, raw, counts


def run_prop(src, fw, bw, reach, valid, scratch=None):
    F, H, W = src.shape
    dst = torch.full((F, H, W), 99, dtype=torch.uint8, device=DEV)
    hits = torch.full((F, H, W), 201, dtype=torch.uint8, device=DEV)
    zeros = torch.full((F,), -1, dtype=torch.int64, device=DEV)
    got = _lib.mask_propagate(dev(src), dev(fw), dev(bw), reach, valid=dev(valid), dst=dst, hits=hits, zero_counts=zeros, scratch=scratch)
    assert got is dst
    return dst, hits, zeros


def differing_span(got, want):
    err, hops, raw, counts = got
    return (same_bits(err, want["err"]), same_bytes(hops, want["hops"]), same_bytes(raw, want["raw"]),
            int((counts.cpu().numpy() != want["counts"]).sum()))


@pytest.mark.parametrize("given", ["with", "without"])
@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("shape", SHAPES)
def test_span_equals_the_twin(hip_lib, shape, span, given):
    F, H, W = shape
    c = case(shape)
    want = twin_span(shape, span, given)
    scratch = torch.zeros(_lib.motion_span_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    for turn in range(2):                                         # the scratch is used twice and left zero
        got = run_span(c["fw"], c["bw"], matrices(shape, span), span, c["valid"] if given == "with" else None, scratch)
        bad = differing_span(got, want)
        if turn == 0:
            print(f"{shape} span {span} {given} valid: differing values (err, hops, raw, counts) {bad}; counts per frame "
                  f"{want['counts'].tolist()} of {H * W}; pixels by hops {np.bincount(want['hops'].ravel()).tolist()}")
        assert bad == (0, 0, 0, 0), turn
        assert not scratch.any(), turn
    # what the twin's result says about the case
    assert want["hops"].max() <= span and np.array_equal(want["err"] == msn.UNKNOWN, want["hops"] == 0)
    assert np.array_equal(want["counts"][:, 2], (want["raw"] == 0).reshape(F, -1).sum(1))
    if F == 1:
        assert not want["hops"].any() and (want["raw"] == 255).all()     # a single frame has no neighbour: nothing is measured
    if F >= 3:
        assert (want["hops"][1, 0] <= span - 1).all()             # frames 1 and 2 share a centre: no line between them
    if H * W > 500:
        assert want["hops"].max() == min(span, F - 1)             # chains that outlived every hop
        assert 0 < want["counts"][0, 2] < H * W                   # moving and static pixels both


@pytest.mark.parametrize("given", ["with", "without"])
@pytest.mark.parametrize("reach", SPANS)
@pytest.mark.parametrize("shape", SHAPES)
def test_propagate_equals_the_twin(hip_lib, shape, reach, given):
    F, H, W = shape
    c = case(shape)
    want_dst, want_hits, want_zeros = twin_prop(shape, reach, given)
    scratch = torch.zeros(_lib.motion_span_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    for turn in range(2):                                         # the scratch is used twice and left zero
        dst, hits, zeros = run_prop(c["src"], c["fw"], c["bw"], reach, c["valid"] if given == "with" else None, scratch)
        bad = (same_bytes(dst, want_dst), same_bytes(hits, want_hits), int((zeros.cpu().numpy() != want_zeros).sum()))
        if turn == 0:
            print(f"{shape} reach {reach} {given} valid: differing values (dst, hits, zero counts) {bad}; zeros per frame "
                  f"{want_zeros.tolist()} of {H * W}; pixels by hits {np.bincount(want_hits.ravel()).tolist()}")
        assert bad == (0, 0, 0), turn
        assert not scratch.any(), turn
    assert want_hits.max() <= 2 * reach and np.array_equal(want_dst == 0, (c["src"] == 0) | (want_hits > 0))
    assert np.array_equal(want_dst[want_dst != 0], c["src"][want_dst != 0])      # every other pixel keeps its value
    if F == 1:
        assert not want_hits.any()
    if H * W > 500:
        assert want_hits.max() >= min(2, reach, F - 1) and (want_zeros > (c["src"] == 0).reshape(F, -1).sum(1)).all()
        if reach > 1:                                             # chains that outlived a hop met more
            assert want_hits.astype(np.int64).sum() > twin_prop(shape, 1, given)[1].astype(np.int64).sum()


@pytest.mark.parametrize("shape", [(4, 9, 1), (4, 7, 2), (4, 1, 6)])
def test_narrow_frames_hop_along_their_only_columns(hip_lib, shape):
    """One and two columns (the right tap is the left one again, or always the last column) and one row, at span and reach 3: flows
    of whole and half pixels, so that chains land inside such a frame at all."""
    F, H, W = shape
    rng = np.random.default_rng(10 * H + W)
    K = np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1.0]])
    poses = np.tile(np.eye(4)[:3], (F, 1, 1))
    poses[:, :, 3] = np.stack([0.12 * np.arange(F), rng.uniform(-0.01, 0.01, F), rng.uniform(-0.02, 0.02, F)], -1)
    Fm = motion.fundamental_matrices(K, poses, span=3).numpy()
    steps = np.array([-1.0, -0.5, 0.0, 0.0, 0.5, 1.0], f32)
    fw, bw = (rng.choice(steps, (F, H, W, 2)) for _ in range(2))
    for flow in (fw, bw):                                         # across a frame one pixel wide or high only a zero component stays inside
        if W == 1:
            flow[..., 0] = 0
        if H == 1:
            flow[..., 1] = 0
    fw[rng.random((F, H, W)) < 0.05] = 1e10
    valid = (rng.random((F, 2, H, W)) < 0.9).astype(np.uint8)
    src = rng.choice(np.array([0, 255], np.uint8), (F, H, W), p=[0.5, 0.5])
    for v in (valid, None):
        want = msn.motion_span(fw, bw, Fm, msn.hop_scale(3), 3, valid=v, threshold=THRESHOLD)
        assert want["hops"].max() == 3                            # chains that outlived both hops
        assert differing_span(run_span(fw, bw, Fm, 3, v), want) == (0, 0, 0, 0)
        want_dst, want_hits, want_zeros = msn.propagate(src, fw, bw, 3, valid=v)
        assert want_hits.astype(int).sum() > msn.propagate(src, fw, bw, 1, valid=v)[1].astype(int).sum()      # ... that met a zero after a hop
        dst, hits, zeros = run_prop(src, fw, bw, 3, v)
        assert same_bytes(dst, want_dst) == 0 and same_bytes(hits, want_hits) == 0 and zeros.cpu().numpy().tolist() == want_zeros.tolist()


def test_a_frame_with_its_neighbours_alone_gives_the_bits_it_has_in_the_batch(hip_lib):
    """Frame 3 of six with span / reach 2 sees frames 1 .. 5.  Those five frames alone (the frame's own matrices; the frames now
    start at other flat offsets, so the lanes' vector and scalar routes change) give frame 3 the same bits and counts, for both
    kernels -- and the outputs that the call may leave out change nothing."""
    shape, span = SHAPES[2], 2
    c = case(shape)
    full = run_span(c["fw"], c["bw"], matrices(shape, span), span, c["valid"])
    part = run_span(c["fw"][1:], c["bw"][1:], matrices(shape, span)[1:], span, c["valid"][1:])
    for a, b in zip(full, part):
        assert torch.equal(a[3], b[2])
    assert not torch.equal(full[2][1], part[2][0])                # (frame 1 lost its backward neighbour: the window matters)
    full = run_prop(c["src"], c["fw"], c["bw"], span, c["valid"])
    part = run_prop(c["src"][1:], c["fw"][1:], c["bw"][1:], span, c["valid"][1:])
    for a, b in zip(full, part):
        assert torch.equal(a[3], b[2])
    # without err, hops, counts and scratch the call computes the same raw; without hits and counts the same dst
    raw = _lib.motion_span(dev(c["fw"]), dev(c["bw"]), dev(matrices(shape, span)), dev(msn.hop_scale(span)), span, valid=dev(c["valid"]),
                           threshold=THRESHOLD)
    assert same_bytes(raw, twin_span(shape, span, "with")["raw"]) == 0
    assert same_bytes(_lib.mask_propagate(dev(c["src"]), dev(c["fw"]), dev(c["bw"]), span, valid=dev(c["valid"])), twin_prop(shape, span, "with")[0]) == 0


@pytest.mark.parametrize("shape", SHAPES + ["scene"])
def test_span_1_is_the_one_frame_kernel(hip_lib, shape):
    """With span 1, hop_scale = {1} and nsff_motion_maps' own valid: that kernel's raw map and over-counts, and its err where valid.
    On the sprinkled cases, whose two flows are drawn independently, so that few pixels pass the forward-backward check, and on the
    synthetic scene, where most do."""
    if shape == "scene":
        sc = scene()
        K, poses, fw, bw = sc["K"], sc["poses"], sc["flows_fw"], sc["flows_bw"]
    else:
        c = case(shape)
        K, poses, fw, bw = c["K"], c["poses"], c["fw"], c["bw"]
    F, H, W = fw.shape[:3]
    Fm = motion.fundamental_matrices(K, poses)
    err = torch.empty(F, 2, H, W, device=DEV)
    valid = torch.empty(F, 2, H, W, dtype=torch.uint8, device=DEV)
    raw = torch.empty(F, H, W, dtype=torch.uint8, device=DEV)
    counts, sums = torch.empty(F, 5, dtype=torch.int64, device=DEV), torch.empty(F, 2, dtype=torch.float64, device=DEV)
    _lib.motion_maps(dev(fw), dev(bw), Fm.to(DEV), threshold=THRESHOLD, err=err, valid=valid, raw=raw, counts=counts, err_sums=sums)
    got_err, got_hops, got_raw, got_counts = run_span(fw, bw, Fm[:, :, None].numpy(), 1, valid.cpu().numpy(), scale=np.ones(1, f32))
    assert torch.equal(got_raw, raw) and torch.equal(got_counts, counts[:, 2:5]) and torch.equal(got_hops, valid)
    v = valid != 0
    assert torch.equal(got_err[v], err[v]) and bool((got_err[~v] == motion.UNKNOWN).all())
    print(f"{shape}: valid {int(v.sum())} of {v.numel()}, dynamic per frame {counts[:, 4].tolist()}")
    if shape == "scene":                                          # the disc is found and most pixels have a vote
        assert int(counts[:, 4].min()) > 50 and int(v[1:-1].sum()) > 0.8 * v[1:-1].numel()
    elif H * W > 500:
        assert int(v.sum()) > 0


# ---- the Python layer ----
def scene():
    if "scene" not in _CASES:
        sc = mnp.make_scene(4, 37, 71, noise=0.05, seed=0)
        for v in sc.values():
            v.setflags(write=False)
        _CASES["scene"] = sc
    return _CASES["scene"]


def twin_chain(fw, bw, K, poses, span, reach, erode=15):
    """What motion_masks(span, reach) states: the one-frame twin for err and valid, the chained test for raw, the propagation, the
    erosion."""
    Fs = motion.fundamental_matrices(K, poses, span=span).numpy()
    maps = mnp.motion_maps(fw, bw, Fs[:, :, 0] if span > 1 else Fs)
    out = dict(err=maps["err"], valid=maps["valid"], counts=maps["counts"], raw=maps["raw"])
    if span > 1:
        sp = msn.motion_span(fw, bw, Fs, msn.hop_scale(span), span, valid=maps["valid"])
        out.update(err_span=sp["err"], hops=sp["hops"], span_counts=sp["counts"], raw=sp["raw"])
    if reach > 0:
        out["raw"], out["hits"], out["propagated"] = msn.propagate(out["raw"], fw, bw, reach, valid=maps["valid"])
    out["mask"] = mnp.erode(out["raw"], erode)
    return out


def check_chain(got, want, stats):
    for key in ("err", "err_span"):
        assert same_bits(got[key], want[key]) == 0, key
    for key in ("valid", "hops", "hits", "raw", "mask"):
        assert same_bytes(got[key], want[key]) == 0, key
    F = len(want["raw"])
    assert stats.counts.tolist() == want["counts"].tolist() and stats.span_counts.tolist() == want["span_counts"].tolist()
    assert stats.propagated.tolist() == want["propagated"].tolist() == (want["raw"] == 0).reshape(F, -1).sum(1).tolist()
    assert stats.dynamic.tolist() == (want["mask"] == 0).reshape(F, -1).sum(1).tolist()


def test_motion_masks_with_default_arguments_is_what_it_was(hip_lib):
    """The call, its two launches and every returned bit: nsff_motion_maps and nsff_mask_erode called directly."""
    sc = scene()
    fw, bw = dev(sc["flows_fw"]), dev(sc["flows_bw"])
    F, H, W = fw.shape[:3]
    got = motion.motion_masks(fw, bw, sc["K"], sc["poses"])
    assert sorted(got) == ["err", "mask", "raw", "stats", "valid"]
    err = torch.empty(F, 2, H, W, device=DEV)
    valid = torch.empty(F, 2, H, W, dtype=torch.uint8, device=DEV)
    raw, mask = torch.empty(F, H, W, dtype=torch.uint8, device=DEV), torch.empty(F, H, W, dtype=torch.uint8, device=DEV)
    counts, sums = torch.empty(F, 5, dtype=torch.int64, device=DEV), torch.empty(F, 2, dtype=torch.float64, device=DEV)
    dynamic = torch.empty(F, dtype=torch.int64, device=DEV)
    _lib.motion_maps(fw, bw, motion.fundamental_matrices(sc["K"], sc["poses"]).to(DEV), alpha=0.01, beta=0.5, threshold=1.0, err=err,
                     valid=valid, raw=raw, counts=counts, err_sums=sums)
    _lib.mask_erode(raw, mask, 15, zero_counts=dynamic)
    assert torch.equal(got["err"].view(torch.int32), err.view(torch.int32)) and torch.equal(got["valid"], valid)
    assert torch.equal(got["raw"], raw) and torch.equal(got["mask"], mask) and int((raw == 0).sum()) > 0
    st = got["stats"]
    assert torch.equal(st.gpu_counts, counts) and torch.equal(st.gpu_err_sums, sums) and torch.equal(st.gpu_dynamic, dynamic)
    assert st.span_counts is None and st.propagated is None
    again = motion.motion_masks(fw, bw, sc["K"], sc["poses"], span=1, reach=0, hop_scale=None)
    assert torch.equal(again["raw"], raw) and torch.equal(again["mask"], mask) and sorted(again) == sorted(got)


def test_motion_masks_with_a_span_and_a_reach(hip_lib):
    sc = scene()
    fw, bw = dev(sc["flows_fw"]), dev(sc["flows_bw"])
    got = motion.motion_masks(fw, bw, sc["K"], sc["poses"], span=3, reach=2)
    assert sorted(got) == ["err", "err_span", "hits", "hops", "mask", "raw", "stats", "valid"]
    want = twin_chain(sc["flows_fw"], sc["flows_bw"], sc["K"], sc["poses"], 3, 2)
    check_chain(got, want, got["stats"])
    assert want["hops"].max() == 3 and want["hits"].max() >= 2 and 0 < (want["raw"] == 0).sum() < want["raw"].size
    # each keyword alone, and a hop_scale of one's own
    one = motion.motion_masks(fw, bw, sc["K"], sc["poses"], span=3, hop_scale=[1.0, 0.5, 0.25])
    assert sorted(one) == ["err", "err_span", "hops", "mask", "raw", "stats", "valid"] and one["stats"].propagated is None
    sp = msn.motion_span(sc["flows_fw"], sc["flows_bw"], motion.fundamental_matrices(sc["K"], sc["poses"], span=3).numpy(),
                         np.array([1.0, 0.5, 0.25], f32), 3, valid=want["valid"])
    assert same_bytes(one["raw"], sp["raw"]) == 0 and same_bits(one["err_span"], sp["err"]) == 0
    two = motion.motion_masks(fw, bw, sc["K"], sc["poses"], reach=2)
    assert sorted(two) == ["err", "hits", "mask", "raw", "stats", "valid"] and two["stats"].span_counts is None
    assert same_bytes(two["raw"], twin_chain(sc["flows_fw"], sc["flows_bw"], sc["K"], sc["poses"], 1, 2)["raw"]) == 0
    # propagate() on masks from any source
    src = np.where(np.random.default_rng(0).random((4, 37, 71)) < 0.05, 0, 200).astype(np.uint8)
    dst, hits = motion.propagate(dev(src), fw, bw, valid=dev(want["valid"]), reach=2, return_hits=True)
    want_dst, want_hits, _ = msn.propagate(src, sc["flows_fw"], sc["flows_bw"], 2, valid=want["valid"])
    assert same_bytes(dst, want_dst) == 0 and same_bytes(hits, want_hits) == 0
    assert same_bytes(motion.propagate(dev(src), fw, bw), msn.propagate(src, sc["flows_fw"], sc["flows_bw"], 2)[0]) == 0


def test_sequence_geometry_passes_the_keywords_on(hip_lib):
    """images -> flows -> masks with span 3 and reach 2 -> disparities: the masks are the twin chain's on the flows the call returns."""
    ys, xs = np.meshgrid(np.arange(37.0), np.arange(71.0), indexing="ij")
    grey = [127.5 + 38 * (np.sin(0.31 * (xs - 1.5 * t) + 0.12 * ys) + 0.8 * np.sin(1.1 - 0.22 * (xs - 1.5 * t) + 0.41 * ys)) for t in range(4)]
    images = dev(np.repeat(np.rint(np.stack(grey))[..., None], 3, -1).astype(np.uint8))
    sc = scene()
    out = depth.sequence_geometry(images, sc["K"], sc["poses"], flow_kw=dict(levels=2, warps=2, iters=10), mask_kw=dict(span=3, reach=2))
    fw, bw = out["flows_fw"].cpu().numpy(), out["flows_bw"].cpu().numpy()
    want = twin_chain(fw, bw, sc["K"], sc["poses"], 3, 2)
    assert same_bytes(out["masks"], want["mask"]) == 0 and same_bytes(out["valid"], want["valid"]) == 0
    st = out["motion_stats"]
    assert st.span_counts.tolist() == want["span_counts"].tolist() and st.propagated.tolist() == want["propagated"].tolist()
    assert tuple(out["disps"].shape) == (4, 37, 71) and bool(torch.isfinite(out["disps"]).all())


def test_the_calls_reject_bad_arguments_without_a_launch(hip_lib):
    host.check_refusals()
    torch.cuda.synchronize()
