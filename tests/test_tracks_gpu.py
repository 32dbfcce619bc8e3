"""MI355X checks of the track layer (nsff_pl_amd/tracks.py, csrc/tracks.hip), in the default arithmetic and in "f32":

* one step of ``advect`` against the reference's own render (golden g5: ``xyzs_fine`` -> ``transient_flows_fw/bw``, all 4608 samples);
* golden g30 (the reference's forward chained in float64, tests/golden/make_golden_tracks.py): teacher-forced steps at the
  project's 1e-4 max-norm bar, the free-running chain within the golden's own ``bound[j]``, times and liveness exact;
* ``nsff_track_step`` alone on synthetic records, bit for bit against the numpy twin tests/tracks_numpy.py, uv and depth included, in
  both camera modes.  R * S: 1; 255, 256, 257 (a wave's 64 lanes x 4 points); 1023, 1024, 1025 (a workgroup's 256 lanes x 4 points);
  (130, 3) and (37, 3): slab 1 of the path starts 8 and 12 bytes off a 16-byte boundary, so every lane takes the dword path, and row
  starts fall inside a lane's four points; (5, 64): rows that are a multiple of a wave;
* both ``pts_per_ray`` routes of the field dispatcher (S = 1 and S = 64) through ``advect`` against the twin driven by the oracle's
  numpy field; ``nsff_track_draw`` bit for bit against the twin; ``evaluate.track_panel`` against the composition of its parts."""
import os

import numpy as np
import pytest
import torch

import common
import scenes
import tracks_numpy as tnp
import nsff_pl_amd as A
from nsff_pl_amd import _lib, evaluate, metrics, tracks
from oracle import nsff_oracle as orc

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(n_rays=37, N_samples=3, N_importance=0, transient=True, viewdir=False, appearance=False, test_time=True,
           flow=['fw', 'bw'], gain=1.5, seed=30)                # make_golden_tracks.CFG
N, MAX_T = 4, 5
TOL = 1e-4                                                      # the project's relative bar (max-norm)
DIRS = [("fw", 1), ("bw", -1)]


@pytest.fixture(params=["default", "f32"])
def precision(request, hip_lib):
    if request.param == "f32":
        A.set_precision("f32")
    yield request.param
    A.set_precision(A.config.DEFAULT_PRECISION)


@pytest.fixture(scope="module")
def g30():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g30_tracks.npz")))
    for v in g.values():
        v.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def scene():
    """The g30 model on the GPU and its fp32 oracle field (shared, read-only)."""
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, CFG)
    field = tnp.oracle_field(orc, orc.field_from_module(models["fine"]), emb["xyz"].freqs.numpy(), emb["t"].weight.detach().numpy())
    models["fine"].to(DEV), emb["t"].to(DEV)
    return models["fine"], emb, field


@pytest.fixture(scope="module")
def g5():
    cfg, meta, rays, ts, models, emb, dataset, want = common.build_case("g5_nsff_test_vis", A.NeRF, A.PosEmbedding)
    models["fine"].to(DEV), emb["t"].to(DEV)
    return models["fine"], emb, ts, want


def dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)                  # (a copy: the shared cases are read-only)


def host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def k4(K):
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


# ---- one step against the reference's own render ----
@pytest.mark.parametrize("tag,sign", DIRS)
def test_one_step_equals_the_reference_render(g5, precision, tag, sign):
    model, emb, ts, want = g5
    xyz, ref = want["xyzs_fine"], want["transient_flows_" + tag]
    assert xyz.shape == (24, 192, 3) and ts.tolist() == [7] * 24
    zeroed = want["zs_fine"] > np.float32(0.95)
    assert np.array_equal(tnp.zero_rule(xyz), zeroed) and zeroed.sum() == 234             # the rule on the point = the rule on the depth
    out = host(tracks.advect(model, emb, dev(xyz), ts.to(DEV), sign, scenes.N_FRAMES - 1))
    assert sorted(out) == ["alive", "t", "xyz"] and out["xyz"].shape == (2, 24, 192, 3) and out["xyz"].dtype == np.float32
    assert same_bits(out["xyz"][0], xyz) and out["alive"].dtype == np.bool_ and out["alive"].all()
    assert out["t"].dtype == np.int32 and (out["t"][0] == 7).all() and (out["t"][1] == 7 + sign).all()
    moved = out["xyz"][1].astype(np.float64) - xyz
    err = np.abs(moved - ref).max() / np.abs(ref).max()
    print(f"[{precision}] {tag}: one step over all {ref[..., 0].size} samples, max-norm relative error {err:.2e}")
    assert err <= TOL
    assert same_bits(out["xyz"][1][zeroed], xyz[zeroed])                                      # zeroed samples: exactly 0


# ---- golden g30 ----
@pytest.mark.parametrize("tag,sign", DIRS)
def test_teacher_forced_steps(g30, scene, precision, tag, sign):
    model, emb, _ = scene
    x = g30["xyz_" + tag][:N].astype(np.float32).reshape(-1, 3, 3)                           # every float64 position, rounded; no compounding
    ts = g30["t_" + tag][:N].reshape(-1)
    out = host(tracks.advect(model, emb, dev(x), dev(ts), sign, MAX_T))
    moved = (out["xyz"][1].astype(np.float64) - x).reshape(N, -1, 3, 3)
    for j in range(N):
        ref = g30["flow_" + tag][j]
        err = np.abs(moved[j] - ref).max() / np.abs(ref).max()
        print(f"[{precision}] {tag} step {j}: max-norm relative error {err:.2e}")
        assert err <= TOL
    can = (ts < MAX_T) if sign > 0 else (ts > 0)
    assert np.array_equal(out["alive"][1], can) and np.array_equal(out["t"][1], ts + sign * can)
    assert same_bits(out["xyz"][1][~can], x[~can])


@pytest.mark.parametrize("tag,sign", DIRS)
@pytest.mark.parametrize("view", ["time", "fixed"])
def test_free_running_chain(g30, scene, precision, tag, sign, view):
    model, emb, _ = scene
    Ps = g30["Ps"] if view == "time" else g30["Ps"][int(g30["fixed_view"])]
    out = host(tracks.advect(model, emb, dev(g30["xyz"]), dev(g30["ts"]), sign * N, MAX_T, Ps=dev(Ps), K=g30["K"]))
    assert sorted(out) == ["alive", "depth", "t", "uv", "xyz"]
    assert np.array_equal(out["t"], g30["t_" + tag]) and np.array_equal(out["alive"], g30["alive_" + tag])
    err = np.abs(out["xyz"] - g30["xyz_" + tag]).max((1, 2, 3))
    print(f"[{precision}] {tag} ({view}): free-running error per step {err}, bound {g30['bound_' + tag]}")
    assert not np.isnan(out["xyz"]).any() and (err <= g30["bound_" + tag]).all()
    dead = ~out["alive"][1:]
    assert dead.any() and same_bits(out["xyz"][1:][dead], out["xyz"][:-1][dead])             # a dead row: its last live position
    uv, depth = tnp.project_path(out["xyz"], out["t"], k4(g30["K"]), Ps, view == "fixed")     # the projection of the path it made
    assert same_bits(out["uv"], uv) and same_bits(out["depth"], depth)
    assert (out["depth"] > 0).all() and (out["uv"] != tnp.UNKNOWN).all()                      # (as in the golden: nothing behind a camera)


# ---- the step kernel alone ----
STEP_SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (1023, 1), (1024, 1), (1025, 1), (130, 3), (37, 3), (5, 64)]


@pytest.mark.parametrize("shape", STEP_SHAPES)
@pytest.mark.parametrize("fixed", [False, True])
def test_step_kernel_equals_the_twin_bit_for_bit(hip_lib, shape, fixed):
    R, S = shape
    rng = np.random.default_rng(3100 + 7 * R + S + fixed)
    max_t, n_poses = 4, 5
    K, Ps_all, _ = scenes.camera_buffers()
    K, Ps = K[0].numpy().astype(np.float64), Ps_all[0, :n_poses].numpy()
    if fixed:
        Ps = Ps[3:4]
    xyz = np.concatenate([rng.uniform(-1.2, 1.2, (R, S, 2)), rng.uniform(-1, 0.89, (R, S, 1))], -1).astype(np.float32)
    some = rng.random((R, S))
    xyz[..., 2][some < 0.15] = rng.uniform(0.9, 0.999, int((some < 0.15).sum()))               # the zero rule
    xyz[..., 2][some > 0.93] = rng.uniform(1.0, 1.6, int((some > 0.93).sum()))                 # behind every camera
    if R * S > 1:
        xyz.reshape(-1, 3)[rng.integers(R * S), 2] = np.float32(0.9)                          # (0.9f + 1) * 0.5f, at the threshold
    raw = rng.standard_normal((R * S, _lib.RAW_STRIDE)).astype(np.float32)
    raw[:, 8:14] *= np.float32(0.2)
    t = rng.integers(0, max_t + 1, R).astype(np.int32)
    alive = rng.random(R) < 0.8
    bufs = lambda *shape_, dtype=torch.float32: torch.full((2,) + shape_, 77, dtype=dtype, device=DEV)
    for sign in (1, -1):
        flow = raw[:, 8:11] if sign > 0 else raw[:, 11:14]
        want_x, want_t, want_alive, _ = tnp.step(xyz, t, alive, flow.reshape(R, S, 3), sign, max_t)
        # slab 1 of every array is the one the kernel sees: off a 16-byte boundary whenever R * S * 12 is no multiple of 16
        x_in, x_out, uv, depth = bufs(R, S, 3), bufs(R, S, 3), bufs(R, S, 2), bufs(R, S)
        t_in, t_out = bufs(R, dtype=torch.int32), bufs(R, dtype=torch.int32)
        a_in, a_out = bufs(R, dtype=torch.uint8), bufs(R, dtype=torch.uint8)
        x_in[1], t_in[1], a_in[1] = dev(xyz), dev(t), dev(alive.astype(np.uint8))
        cams = dict(K4=k4(K), Ps=dev(Ps), fixed_view=fixed)
        _lib.track_step(R, S, sign, max_t, x_in[1], t_in[1], a_in[1], raw=dev(raw), xyz_out=x_out[1], t_out=t_out[1], alive_out=a_out[1],
                        uv=uv[1], depth=depth[1], **cams)
        got = host(dict(x=x_out, t=t_out, a=a_out, uv=uv, depth=depth))
        want_uv, want_depth = tnp.project(want_x, want_t, k4(K), Ps, fixed)
        assert same_bits(got["x"][1], want_x) and np.array_equal(got["t"][1], want_t) and np.array_equal(got["a"][1], want_alive)
        assert same_bits(got["uv"][1], want_uv) and same_bits(got["depth"][1], want_depth)
        assert (want_uv == tnp.UNKNOWN).any() or R * S < 8
        for k in got:                                                                         # slab 0 is nobody's: untouched
            assert (got[k][0] == 77).all(), k
        # the projection of a first slab: no records, nothing moves, no state is written
        uv0, depth0 = bufs(R, S, 2), bufs(R, S)
        _lib.track_step(R, S, sign, max_t, x_in[1], t_in[1], a_in[1], uv=uv0[1], depth=depth0[1], **cams)
        got = host(dict(uv=uv0, depth=depth0))
        want_uv, want_depth = tnp.project(xyz, t, k4(K), Ps, fixed)
        assert same_bits(got["uv"][1], want_uv) and same_bits(got["depth"][1], want_depth) and (got["uv"][0] == 77).all()
        # without cameras only the state moves
        x_only = bufs(R, S, 3)
        _lib.track_step(R, S, sign, max_t, x_in[1], t_in[1], a_in[1], raw=dev(raw), xyz_out=x_only[1], t_out=t_out[0], alive_out=a_out[0])
        got = host(dict(x=x_only, t=t_out, a=a_out))
        assert same_bits(got["x"][1], want_x) and np.array_equal(got["t"][0], want_t) and np.array_equal(got["a"][0], want_alive)


# ---- both routes of the field dispatcher ----
@pytest.mark.parametrize("shape,chunk", [((300, 1), None), ((300, 1), 128), ((5, 64), None), ((5, 64), 2)])
def test_field_routes_through_advect(scene, precision, shape, chunk):
    model, emb, field = scene
    R, S = shape
    rng = np.random.default_rng(3200 + R)
    xyz = np.concatenate([rng.uniform(-1, 1, (R, S, 2)), rng.uniform(-1, 0.85, (R, S, 1))], -1).astype(np.float32)
    ts = rng.integers(0, MAX_T + 1, R).astype(np.int32)
    for sign in (1, -1):
        want = tnp.advect(field, xyz, ts, sign, MAX_T)
        out = host(tracks.advect(model, emb, dev(xyz), dev(ts), sign, MAX_T, chunk=chunk))
        assert np.array_equal(out["t"], want["t"]) and np.array_equal(out["alive"], want["alive"])
        moved = out["xyz"][1].astype(np.float64) - xyz
        err = np.abs(moved - want["flow"][0]).max() / np.abs(want["flow"][0]).max()
        print(f"[{precision}] {shape} chunk {chunk} direction {sign}: one step against the twin, max-norm relative error {err:.2e}")
        assert err <= TOL
        three = host(tracks.advect(model, emb, dev(xyz), dev(ts), 3 * sign, MAX_T, chunk=chunk))
        assert same_bits(three["xyz"][:2], out["xyz"])                                        # a longer chain starts with the shorter one
        want = tnp.advect(field, xyz, ts, 3 * sign, MAX_T)
        assert np.array_equal(three["t"], want["t"]) and np.array_equal(three["alive"], want["alive"])
        err = np.abs(three["xyz"] - want["xyz"]).max() / np.abs(want["xyz"]).max()
        print(f"[{precision}] {shape} chunk {chunk} direction {sign}: three free steps against the fp32 twin, paths {err:.2e}")
        assert err <= TOL


# ---- trails ----
def draw_case(name):
    rng = np.random.default_rng(33)
    U = float(tnp.UNKNOWN)
    if name == "one pixel":
        return np.full((1, 1, 3), 5, np.uint8), np.array([[[0.2, -0.3]], [[0.4, 0.1]]], np.float32), np.ones((2, 1), bool)
    img = rng.integers(0, 256, (19, 33, 3)).astype(np.uint8)
    if name == "kinds":
        #      horizontal  vertical   diagonal  steep     reversed   partly off  wholly off  too long   dead      unknown    NaN
        uv = [[[2, 3],    [5, 2],    [8, 1],   [20, 1],  [30, 17],  [28, 10],   [-9, -9],   [-30, 5],  [1, 15],  [4, 15],   [7, 15]],
              [[12, 3],   [5, 14],   [16, 9],  [23, 17], [22, 9],   [45, 14],   [-2, -20],  [30, 5],   [3, 17],  [U, U],    [np.nan, 16]],
              [[12.4, 3], [5.6, 14], [8, 17],  [20, 1],  [30, 17],  [28, 25],   [60, 30],   [30, 70],  [1, 15],  [4, 15],   [7, 15]]]
        ok = np.ones((3, 11), bool)
        ok[1, 8] = False
        return img, np.array(uv, np.float32), ok
    if name == "crossing":
        uv = [[[2, 2], [2, 16], [30, 2]], [[30, 16], [30, 2], [2, 16]], [[2, 2], [2, 16], [30, 2]]]
        return img, np.array(uv, np.float32), np.ones((3, 3), bool)
    Q = int(name)
    n = 5
    uv = np.cumsum(np.concatenate([rng.uniform(2, 17, (1, Q, 2)), rng.normal(0, 4, (n, Q, 2))]), 0).astype(np.float32)
    ok = (rng.random((n + 1, Q)) < 0.9) | (Q == 1)
    if Q > 1:
        uv[rng.random((n + 1, Q)) < 0.03] = U
    return img, uv, ok


@pytest.mark.parametrize("name", ["one pixel", "kinds", "crossing", "1", "257"])
def test_draw_equals_the_twin_bit_for_bit(hip_lib, name):
    img, uv, ok = draw_case(name)
    lut = tracks.default_lut()
    want = tnp.draw(img, uv, ok, lut)
    keys = tnp.canvas(img.shape[0], img.shape[1], uv, ok)
    got = tracks.draw(dev(img), dev(uv), dev(ok), dev(lut))
    again = tracks.draw(dev(img), dev(uv), dev(ok.astype(np.uint8)), dev(lut))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and same_bits(got.cpu().numpy(), want) and torch.equal(got, again)        # two runs: the same bits
    print(f"{name}: {int((keys != 0).sum())} of {keys.size} pixels drawn, {len(set(np.unique(keys).tolist()) - {0})} segments visible")
    assert (keys != 0).any()
    if name == "one pixel":
        assert (want[0, 0] == lut[255]).all()
    if name == "kinds":
        seg = lambda j, q: ((j + 1) << 20) | q
        drawn = set(np.unique(keys).tolist()) - {0}
        assert {seg(0, q) for q in (0, 1, 2, 5)} | {seg(1, q) for q in range(5)} <= drawn       # (a reversed second segment may cover its first)
        assert not drawn & {seg(j, q) for j in (0, 1) for q in (6, 7, 8, 9, 10)}               # off the image, too long, dead, unknown, NaN
    if name == "crossing":
        assert keys[9, 16] == ((2 << 20) | 2)                                                  # all six diagonals meet here: the last step's highest track


def test_track_panel_is_the_composition_of_its_parts(scene, precision):
    model, emb, _ = scene
    models = {"fine": model}
    w, h, n, t0, steps, stride = 33, 19, MAX_T + 1, 2, 2, 4
    stub = scenes.DatasetStub(30)
    poses = stub.poses[:n]
    K = np.array([[40.0, 0, w / 2], [0, 40.0, h / 2], [0, 0, 1]])
    ys, xs = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    pixels = (ys * w + xs).reshape(-1)
    # by hand; min_alpha = the median over the strided pixels, so that some pass and some do not
    rays = evaluate.frame_rays(torch.tensor(K, dtype=torch.float32), torch.tensor(poses[t0]), h, w, device=DEV)
    ts = torch.full((h * w,), t0, dtype=torch.long, device=DEV)
    res = evaluate.render_frame(models, emb, rays, ts, n - 1, 8, 0, output_transient=True, output_transient_flow=['fw', 'bw'])
    min_alpha = float(res["transient_alpha_fine"][pixels].median())
    image, trk = evaluate.track_panel(models, emb, K, poses, t0, (w, h), 8, 0, steps, stride=stride, min_alpha=min_alpha)
    assert image.shape == (h, w, 3) and image.dtype == torch.uint8 and sorted(trk) == ["bw", "fw", "pixels", "selected"]
    assert np.array_equal(trk["pixels"].cpu().numpy(), pixels)
    base = metrics.finish_frames(res["rgb_fine"].view(1, h, w, 3))["rgb_u8"][0]
    selected = res["transient_alpha_fine"][pixels] >= min_alpha
    assert torch.equal(trk["selected"], selected)
    view = A.projection_matrices(K, poses)[1][0][t0]
    want = base
    for key, k in (("fw", steps), ("bw", -steps)):
        part = tracks.advect(model, emb, res["xyz_fine"][pixels].contiguous(), ts[pixels], k, n - 1, Ps=view, K=K)
        for name in ("xyz", "t", "alive", "uv", "depth"):
            assert torch.equal(part[name], trk[key][name]), (key, name)
        assert part["uv"].shape == (steps + 1, len(pixels), 1, 2)
        want = tracks.draw(want, part["uv"], part["alive"] & selected)
    assert torch.equal(image, want)
    # ... and against the twin: trails change only the pixels the twin draws, all inside the image
    twin = base.cpu().numpy()
    sel = selected.cpu().numpy()
    drawn = np.zeros((h, w), bool)
    for key in ("fw", "bw"):
        uv, ok = trk[key]["uv"].cpu().numpy().reshape(steps + 1, -1, 2), trk[key]["alive"].cpu().numpy() & sel
        drawn |= tnp.canvas(h, w, uv, ok) != 0
        twin = tnp.draw(twin, uv, ok, tracks.default_lut())
    got = image.cpu().numpy()
    print(f"[{precision}] track_panel: {int(sel.sum())} of {len(pixels)} pixels selected, {int(drawn.sum())} trail pixels")
    assert same_bits(got, twin) and sel.any() and not sel.all() and drawn.any()
    assert same_bits(got[~drawn], base.cpu().numpy()[~drawn])
