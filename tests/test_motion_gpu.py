"""MI355X checks of nsff_motion_maps and nsff_mask_erode (csrc/motion.hip) against the numpy fp32 twin tests/motion_numpy.py, and of
motion.motion_masks on top of them.  Nothing is read from outside the repository.

Map pass, shapes (F, H, W): (1, 1, 1) no neighbours -- everything static, every error unknown; (3, 19, 33) both end rules fire,
627 pixels a frame, so frames 1 and 2 start off 16-byte alignment (the element path of the pixel quads), and frames 1 and 2 share a
camera centre (a zero matrix: no vote between them); (2, 37, 71) 2627 pixels -- three partials for the frame's last workgroup to
fold; (2, 129, 511) 65 919 pixels -- 65 workgroups, the last ragged, lane 0 of the folding wave takes two partials.  The inputs are
the synthetic scene's flows (noise 0.05 px) sprinkled with unknown, NaN and infinite flows, flows that leave the image and flows
that land exactly on column 0 / W-1 and row 0 / H-1.

Every step of the pass is one fp32 operation that numpy rounds the same way (add, multiply, divide, floor, square root -- the
operations nsff_flow_maps is already compared on), so err, valid and raw are compared for EQUALITY at every pixel and no pixel
near the threshold is left out.  The fp64 sums: both sides add the same fp32 terms in float64, the twin with math.fsum; the bound
is the one tests/test_flow_gpu.py derives for the same reduction, 1e-12 relative."""
import numpy as np
import pytest
import torch

import motion_numpy as mnp
from nsff_pl_amd import _lib, frames, motion

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 19, 33), (2, 37, 71), (2, 129, 511)]
SUM_TOL = 1e-12

_CASES = {}


def case(shape, seed=0):
    """Inputs and the twin's results of one shape, computed once and shared (read-only)."""
    key = shape + (seed,)
    if key in _CASES:
        return _CASES[key]
    F, H, W = shape
    rng = np.random.default_rng(3100 + 10 * H + W + seed)
    sc = mnp.make_scene(F, H, W, noise=0.05, seed=7 + seed)
    poses = sc["poses"].copy()
    if shape == (3, 19, 33) and seed == 0:
        poses[2, :, 3] = poses[1, :, 3]                         # frames 1 and 2: coincident camera centres
    fw, bw = sc["flows_fw"].copy(), sc["flows_bw"].copy()
    if H * W > 1:
        ys, xs = np.mgrid[0:H, 0:W]
        for a in (fw, bw):
            flat = a.reshape(-1, 2)
            some = rng.permutation(len(flat))
            k = max(len(flat) // 150, 1)
            flat[some[:k]] = mnp.UNKNOWN                        # unknown
            flat[some[k:2 * k], 0] = np.nan                     # NaN in one component
            flat[some[2 * k:3 * k], 1] = np.inf
            flat[some[3 * k:4 * k], 0] = np.float32(1.0000001e7)   # just past the threshold
            flat[some[4 * k:5 * k]] = [2.0 * W, -3.0 * H]       # leaving the image
            for j, (u, v) in enumerate(((W - 1, None), (None, H - 1), (0, None), (None, 0), (W - 1, H - 1))):
                for p in some[(5 + j) * k:(6 + j) * k]:         # landing exactly on the last / first column or row
                    f, rest = divmod(int(p), H * W)
                    y, x = divmod(rest, W)
                    if u is not None:
                        a[f, y, x, 0] = u - x
                    if v is not None:
                        a[f, y, x, 1] = v - y
    Fm = motion.fundamental_matrices(sc["K"], poses).numpy()
    c = dict(K=sc["K"], poses=poses, fw=fw, bw=bw, Fm=Fm, disc=sc["disc"])
    c["twin"] = mnp.motion_maps(fw, bw, Fm, alpha=0.01, beta=0.5, threshold=1.0)
    c["twin_check"] = mnp.motion_maps(fw, bw, None, alpha=0.01, beta=0.5)
    for v in list(c.values()) + list(c["twin"].values()) + list(c["twin_check"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = c
    return c


def dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)                 # (a copy: the shared cases are read-only)


def outputs(F, H, W):
    return dict(err=torch.zeros(F, 2, H, W, device=DEV), valid=torch.full((F, 2, H, W), 9, dtype=torch.uint8, device=DEV),
                raw=torch.full((F, H, W), 9, dtype=torch.uint8, device=DEV), counts=torch.full((F, 5), -1, dtype=torch.int64, device=DEV),
                err_sums=torch.full((F, 2), -1.0, dtype=torch.float64, device=DEV))


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def against_twin(out, twin, what):
    got_err, want_err = out["err"].cpu().numpy(), twin["err"]
    print(f"{what}: {int((got_err.view(np.uint32) != want_err.view(np.uint32)).sum())} of {want_err.size} errors differ in their bits; "
          f"counts {twin['counts'].tolist()}")
    assert same_bits(got_err, want_err), what
    assert np.array_equal(out["valid"].cpu().numpy(), twin["valid"]), what
    assert np.array_equal(out["raw"].cpu().numpy(), twin["raw"]), what
    assert np.array_equal(out["counts"].cpu().numpy(), twin["counts"]), what
    got, want = out["err_sums"].cpu().numpy(), twin["err_sums"]
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"{what}: sums {want.tolist()}, max relative error {rel.max():.2e}")
    assert rel.max() <= SUM_TOL and ((want == 0) <= (got == 0)).all(), what


@pytest.mark.parametrize("shape", SHAPES)
def test_map_pass_equals_the_twin(hip_lib, shape):
    c = case(shape)
    F, H, W = shape
    fw, bw, Fm = dev(c["fw"]), dev(c["bw"]), dev(c["Fm"])
    scratch = torch.zeros(_lib.motion_maps_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    twin = c["twin"]
    for turn in range(2):                                       # the scratch buffer is used twice
        out = outputs(F, H, W)
        _lib.motion_maps(fw, bw, Fm, alpha=0.01, beta=0.5, threshold=1.0, scratch=scratch, **out)
        torch.cuda.synchronize()
        against_twin(out, twin, f"{shape} turn {turn}")
        assert not scratch.any(), turn                          # left zero
    assert (twin["counts"][:, 4] == (twin["raw"] == 0).reshape(F, -1).sum(1)).all()
    if shape == (1, 1, 1):
        assert (twin["err"] == mnp.UNKNOWN).all() and (twin["raw"] == 255).all() and not twin["valid"].any() and not twin["counts"].any()
        return
    assert (twin["err"][0, 1] == mnp.UNKNOWN).all() and (twin["err"][F - 1, 0] == mnp.UNKNOWN).all()     # the end rules
    assert twin["counts"][0, 0] > 0.5 * H * W and twin["counts"][0, 2] > 0
    assert (twin["valid"] < (twin["err"] != mnp.UNKNOWN)).any()                                          # an error without a vote
    if shape == (3, 19, 33):                                    # no vote across the coincident pair: frame 2 has none at all
        assert not c["Fm"][1, 0].any() and not c["Fm"][2, 1].any()
        assert (twin["err"][1, 0] == mnp.UNKNOWN).all() and not twin["valid"][2].any() and (twin["raw"][2] == 255).all()
    else:
        assert twin["counts"][F - 1, 1] > 0.5 * H * W and twin["counts"][F - 1, 3] > 0
    # the sprinkled pixels: an unknown or NaN flow has no error; one that leaves the image or lands on the rim has one
    unknown = ~mnp.known(c["fw"][0])
    assert unknown.sum() >= 3 and (twin["err"][0, 0][unknown] == mnp.UNKNOWN).all()
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore"):
        rim = (xs + c["fw"][0, ..., 0] == W - 1) | (ys + c["fw"][0, ..., 1] == H - 1)
        gone = xs + c["fw"][0, ..., 0] > W - 1
    assert rim.sum() >= 2 and (twin["err"][0, 0][rim & ~unknown] != mnp.UNKNOWN).all() and gone.any()
    assert not twin["valid"][0, 0][gone].any() and (twin["err"][0, 0][gone & ~unknown] != mnp.UNKNOWN).all()


@pytest.mark.parametrize("shape", [(3, 19, 33), (2, 37, 71)])
def test_consistency_check_alone_and_single_outputs(hip_lib, shape):
    c = case(shape)
    F, H, W = shape
    fw, bw = dev(c["fw"]), dev(c["bw"])
    valid = motion.flow_consistency(fw, bw)
    assert valid.dtype == torch.uint8 and np.array_equal(valid.cpu().numpy(), c["twin_check"]["valid"])
    out = outputs(F, H, W)
    _lib.motion_maps(fw, bw, None, **out)                      # every output with the flag off
    against_twin(out, c["twin_check"], f"{shape} consistency alone")
    assert (out["raw"] == 255).all() and (out["err"] == motion.UNKNOWN).all()
    loose = motion.flow_consistency(fw, bw, alpha=0.5, beta=4.0).cpu().numpy()
    assert np.array_equal(loose, mnp.motion_maps(c["fw"], c["bw"], None, alpha=0.5, beta=4.0)["valid"]) and loose.sum() > c["twin_check"]["valid"].sum()
    for name in ("err", "valid", "raw"):                       # each output alone (no scratch needed)
        one = {name: outputs(F, H, W)[name]}
        _lib.motion_maps(fw, bw, dev(c["Fm"]), **one)
        got, want = one[name].cpu().numpy(), c["twin"][name]
        assert same_bits(got, want) if name == "err" else np.array_equal(got, want), name
    tight = outputs(F, H, W)                                   # another threshold
    _lib.motion_maps(fw, bw, dev(c["Fm"]), threshold=0.125, **tight)
    against_twin(tight, mnp.motion_maps(c["fw"], c["bw"], c["Fm"], threshold=0.125), f"{shape} threshold 0.125")


@pytest.mark.parametrize("shape", [(3, 19, 33), (2, 37, 71), (2, 129, 511)])
def test_a_sequence_is_bit_identical_alone_and_inside_a_batch(hip_lib, shape):
    """The sequence twice in one batch, with zero matrices across the seam (no vote there, as at a sequence end): both copies --
    the second starts at another alignment where H * W is odd -- equal the sequence alone, outputs and statistics."""
    c = case(shape)
    F, H, W = shape
    alone = outputs(F, H, W)
    _lib.motion_maps(dev(c["fw"]), dev(c["bw"]), dev(c["Fm"]), **alone)
    Fm2 = np.concatenate([c["Fm"], c["Fm"]])
    assert not Fm2[F - 1, 0].any() and not Fm2[F, 1].any()     # the seam: the sequence's own end matrices are zero
    both = outputs(2 * F, H, W)
    _lib.motion_maps(dev(np.concatenate([c["fw"], c["fw"]])), dev(np.concatenate([c["bw"], c["bw"]])), dev(Fm2), **both)
    for name in alone:
        for half in range(2):
            assert torch.equal(both[name][half * F:(half + 1) * F], alone[name]), (name, half)
    again = outputs(F, H, W)
    _lib.motion_maps(dev(c["fw"]), dev(c["bw"]), dev(c["Fm"]), **again)
    for name in alone:
        assert torch.equal(again[name], alone[name]), name    # and run to run
    against_twin(alone, c["twin"], f"{shape} alone")


ERODE_CASES = [((1, 5, 9), 15), ((2, 37, 150), 15), ((2, 37, 150), 3), ((2, 37, 150), 1), ((1, 40, 70), 31), ((3, 19, 33), 7)]


@pytest.mark.parametrize("shape,k", ERODE_CASES)
def test_erosion_equals_the_twin(hip_lib, shape, k):
    rng = np.random.default_rng(40 + k + shape[2])
    binary = rng.choice(np.array([0, 255], np.uint8), shape, p=[0.004, 0.996])
    grey = rng.integers(1, 256, shape, dtype=np.uint8)          # not binary: any values, a few zeros
    grey[rng.random(shape) < 0.002] = 0
    edge = np.full(shape, 255, np.uint8)                        # zeros in the corners and on the rim only
    edge[:, 0, 0] = edge[:, -1, -1] = edge[:, shape[1] // 2, -1] = 0
    scratch = torch.zeros(_lib.motion_maps_scratch_bytes(*shape), dtype=torch.uint8, device=DEV)
    for name, img in (("binary", binary), ("grey", grey), ("edge", edge)):
        want = mnp.erode(img, k)
        got, counts = motion.erode(dev(img), k, return_counts=True)
        zeros = (want == 0).reshape(shape[0], -1).sum(1)
        print(f"{shape} k = {k} {name}: zero pixels {(img == 0).reshape(shape[0], -1).sum(1).tolist()} -> {zeros.tolist()}")
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), name
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), zeros), name
        assert torch.equal(motion.erode(dev(img), k), got)     # without the counts
        dst, n = torch.full(shape, 9, dtype=torch.uint8, device=DEV), torch.full((shape[0],), -1, dtype=torch.int64, device=DEV)
        _lib.mask_erode(dev(img), dst, k, zero_counts=n, scratch=scratch)     # a caller's scratch, reused
        assert torch.equal(dst, got) and torch.equal(n, counts) and not scratch.any(), name
        if k == 1:
            assert np.array_equal(want, img)
    one = motion.erode(dev(grey[0]), k)                         # a single (H, W) image
    assert tuple(one.shape) == shape[1:] and np.array_equal(one.cpu().numpy(), mnp.erode(grey[0], k))


def test_motion_masks_is_the_composition_of_its_parts_and_feeds_the_records(hip_lib):
    shape = (3, 19, 33)
    F, H, W = shape
    c = case(shape, seed=1)                                     # (seed 1: the scene's own poses, no coincident pair)
    fw, bw = dev(c["fw"]), dev(c["bw"])
    scratch = torch.zeros(_lib.motion_maps_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)
    for kwargs in (dict(), dict(threshold=0.5, erode=5, alpha=0.02, beta=1.0, scratch=scratch)):
        res = motion.motion_masks(fw, bw, c["K"], c["poses"], **kwargs)
        assert sorted(res) == ["err", "mask", "raw", "stats", "valid"] and all(res[k].is_cuda for k in ("err", "mask", "raw", "valid"))
        kw = {k: v for k, v in kwargs.items() if k in ("threshold", "alpha", "beta")}
        twin = mnp.motion_maps(c["fw"], c["bw"], c["Fm"], **kw)
        part = outputs(F, H, W)
        _lib.motion_maps(fw, bw, dev(c["Fm"]), **kw, **part)
        for name in ("err", "valid", "raw"):
            assert torch.equal(res[name], part[name]), name
        k = kwargs.get("erode", 15)
        eroded, zeros = motion.erode(part["raw"], k, return_counts=True)
        assert torch.equal(res["mask"], eroded) and np.array_equal(res["mask"].cpu().numpy(), mnp.erode(twin["raw"], k))
        stats = res["stats"]
        assert torch.equal(stats.gpu_counts, part["counts"]) and torch.equal(stats.gpu_err_sums, part["err_sums"])
        assert torch.equal(stats.gpu_dynamic, zeros) and np.array_equal(stats.counts, twin["counts"])
        assert np.array_equal(stats.dynamic_fraction, (res["mask"] == 0).reshape(F, -1).sum(1).cpu().numpy() / (H * W))
        assert np.array_equal(stats.valid_fraction, twin["counts"][:, :2] / (H * W)) and np.isnan(stats.mean_err[0, 1])
        assert abs(stats.mean_err[1, 0] - twin["err_sums"][1, 0] / twin["counts"][1, 0]) <= 1e-12 * stats.mean_err[1, 0]
        assert (res["mask"] <= res["raw"]).all() and (res["mask"] == 0).sum() > (res["raw"] == 0).sum() > 0
        assert not scratch.any()
    # 'mask' goes unchanged into the ray records: column 11 is mask / 255
    res = motion.motion_masks(fw, bw, c["K"], c["poses"], erode=3)
    g = torch.Generator(DEV).manual_seed(0)
    images = torch.randint(0, 256, (F, H, W, 3), device=DEV, generator=g, dtype=torch.uint8)
    disps = torch.rand(F, H, W, device=DEV, generator=g)
    rec = frames.build_records(np.array(c["K"]), np.array(c["poses"]), images, disps, res["mask"], fw, bw)
    want = res["mask"].reshape(F, H * W).float() / 255.0
    assert torch.equal(rec[:, :, 11], want) and 0 < int((want == 0).sum()) < want.numel() and set(want.unique().tolist()) == {0.0, 1.0}


def test_the_two_calls_are_capturable(hip_lib):
    """No synchronisation and no allocation inside nsff_motion_maps and nsff_mask_erode: both recorded into a graph and replayed on
    new data."""
    shape = (2, 37, 71)
    F, H, W = shape
    first, second = case(shape), case(shape, seed=1)
    fw, bw, Fm = dev(first["fw"]), dev(first["bw"]), dev(first["Fm"])
    out = outputs(F, H, W)
    mask, dynamic = torch.zeros(F, H, W, dtype=torch.uint8, device=DEV), torch.zeros(F, dtype=torch.int64, device=DEV)
    scratch = torch.zeros(_lib.motion_maps_scratch_bytes(F, H, W), dtype=torch.uint8, device=DEV)

    def call():
        _lib.motion_maps(fw, bw, Fm, scratch=scratch, **out)
        _lib.mask_erode(out["raw"], mask, 5, zero_counts=dynamic, scratch=scratch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                  # warm-up outside the graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    against_twin(out, first["twin"], "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    fw.copy_(dev(second["fw"])), bw.copy_(dev(second["bw"])), Fm.copy_(dev(second["Fm"]))
    for t in list(out.values()) + [mask, dynamic]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(first["twin"]["raw"], second["twin"]["raw"])
    against_twin(out, second["twin"], "replayed")
    want = mnp.erode(second["twin"]["raw"], 5)
    assert np.array_equal(mask.cpu().numpy(), want) and dynamic.tolist() == (want == 0).reshape(F, -1).sum(1).tolist()
    assert not scratch.any()
