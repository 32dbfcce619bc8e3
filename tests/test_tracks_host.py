"""CPU checks of the track layer: the numpy twin tests/tracks_numpy.py against golden g30 (the reference's own forward chained in
float64, tests/golden/make_golden_tracks.py), the C ABI of nsff_track_step / nsff_track_draw (declared, exported, bound; argument
validation without a launch), every refusal of the Python layer, and the twin's line rule against properties that do not depend on
how it is written."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import scenes
import tracks_numpy as tnp
import nsff_pl_amd as A
from nsff_pl_amd import _lib, evaluate, tracks
from oracle import nsff_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CFG = dict(n_rays=37, N_samples=3, N_importance=0, transient=True, viewdir=False, appearance=False, test_time=True,
           flow=['fw', 'bw'], gain=1.5, seed=30)                # make_golden_tracks.CFG
R, S, N, MAX_T = 37, 3, 4, 5
# The twin's float64 chain against the reference's: the same float64 operations up to the summation order of the dense layers.  One
# 256-term dot product differs by at most 256 * 2^-53 = 3e-14 of its terms' sum; eight layers deep with |weights| summing to a few
# units a row this stays below 1e-11 on a flow, and the chain's measured growth (g30 `growth_*`: at most 23) carries it to < 1e-9.
F64_TOL = 1e-9


@pytest.fixture(scope="module")
def g30():
    return dict(np.load(os.path.join(GOLDEN, "g30_tracks.npz")))


@pytest.fixture(scope="module")
def scene():
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, CFG)
    return models["fine"], emb, scenes.weight_checksum(models, emb)


def k4(g):
    K = g["K"]
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def test_golden_is_the_one_described(g30, scene):
    assert g30["xyz"].shape == (R, S, 3) and g30["xyz"].dtype == np.float32
    assert g30["ts"].dtype == np.int32 and sorted(set(g30["ts"].tolist())) == list(range(MAX_T + 1)) and int(g30["max_t"]) == MAX_T
    assert abs(scene[2] - float(g30["weight_checksum"])) <= 1e-9 * abs(scene[2])              # the seeded weights are the golden's
    assert (g30["xyz"][..., 2] > 0.9).sum() == 14                                              # the zero rule fires
    for tag in ("fw", "bw"):
        assert g30["xyz_" + tag].shape == (N + 1, R, S, 3) and g30["xyz_" + tag].dtype == np.float64
        assert g30["flow_" + tag].shape == (N, R, S, 3) and g30["uv_time_" + tag].shape == g30["uv_fixed_" + tag].shape == (N + 1, R, S, 2)
        alive = g30["alive_" + tag]
        assert alive[0].all() and sorted(set(alive.sum(0).tolist())) == [1, 2, 3, 4, 5]       # rows die after 0, 1, 2, ... steps
        assert g30["bound_" + tag][0] == 0 and (np.diff(g30["bound_" + tag]) > 0).all() and g30["bound_" + tag][-1] < 1e-4
        assert np.array_equal(g30["xyz_" + tag][0], g30["xyz"].astype(np.float64))
    assert os.path.getsize(os.path.join(GOLDEN, "g30_tracks.npz")) < os.path.getsize(os.path.join(GOLDEN, "g26_flow.npz"))


@pytest.mark.parametrize("tag,steps", [("fw", N), ("bw", -N)])
def test_twin_with_the_oracle_field_reproduces_the_reference_chain(g30, scene, tag, steps):
    model, emb, _ = scene
    field = tnp.oracle_field(orc, orc.field_from_module(model), emb["xyz"].freqs.numpy(), emb["t"].weight.detach().numpy(), np.float64)
    got = tnp.advect(field, g30["xyz"].astype(np.float64), g30["ts"], steps, MAX_T)
    assert got["xyz"].dtype == np.float64 and orc.F is np.float32                             # (the oracle's format is restored)
    assert np.array_equal(got["t"], g30["t_" + tag]) and np.array_equal(got["alive"], g30["alive_" + tag])
    e_flow = np.abs(got["flow"] - g30["flow_" + tag]).max()
    e_path = np.abs(got["xyz"] - g30["xyz_" + tag]).max()
    print(f"{tag}: float64 twin against the reference chain: flows {e_flow:.2e}, paths {e_path:.2e}")
    assert e_flow <= F64_TOL and e_path <= F64_TOL
    dead = ~got["alive"][1:]
    assert (got["flow"][dead] == 0).all() and np.array_equal(got["xyz"][1:][dead], got["xyz"][:-1][dead])   # a stopped row stays
    zeroed = tnp.zero_rule(got["xyz"][:-1])
    assert zeroed.any() and (got["flow"][zeroed] == 0).all()
    for key, Ps, fixed in (("uv_time_", g30["Ps"], False), ("uv_fixed_", g30["Ps"][int(g30["fixed_view"])], True)):
        uv, depth = tnp.project_path(got["xyz"], got["t"], k4(g30), Ps, fixed)
        want = g30[key + tag]
        assert np.array_equal(uv == 1e10, want == 1e10) and (depth > 0).all()
        assert np.abs(uv - want).max() <= 1e-6                                                  # pixels of a 512 x 288 view
    # the fp32 twin stays within the golden's bound
    field32 = tnp.oracle_field(orc, orc.field_from_module(model), emb["xyz"].freqs.numpy(), emb["t"].weight.detach().numpy())
    got32 = tnp.advect(field32, g30["xyz"], g30["ts"], steps, MAX_T)
    assert got32["xyz"].dtype == np.float32 and np.array_equal(got32["alive"], g30["alive_" + tag])
    err = np.abs(got32["xyz"] - g30["xyz_" + tag]).max((1, 2, 3))
    print(f"{tag}: fp32 twin, free-running error per step {err}, bound {g30['bound_' + tag]}")
    assert (err <= g30["bound_" + tag] + np.finfo(np.float32).eps).all()                        # (+ the rounding of the start points' sums)


# ---- C ABI ----
_BUF = (C.c_double * 64)()                                    # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15


def _step_args(**kw):
    a = _lib.TrackStepArgs(n_rows=5, pts_per_row=3, direction=1, max_t=2, n_poses=3, fixed_view=0, fx=10.0, fy=10.0, cx=2.5, cy=2.0,
                           raw=_P, xyz_in=_P, t_in=_P, alive_in=_P, xyz_out=_P + 64, t_out=_P + 128, alive_out=_P + 192,
                           Ps=_P, uv=_P, depth=_P)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _draw_args(**kw):
    a = _lib.TrackDrawArgs(H=4, W=5, n_steps=3, n_tracks=7, uv=_P, ok=_P, image=_P, lut=_P, out=_P, scratch=_P, scratch_bytes=80)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_abi_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    step = lambda **kw: lib.nsff_track_step(C.byref(_step_args(**kw)), None)
    assert lib.nsff_track_step(None, None) == -2
    no_cam = dict(Ps=None, uv=None, depth=None)
    no_move = dict(raw=None, xyz_out=None, t_out=None, alive_out=None)
    for bad in (dict(n_rows=-1), dict(pts_per_row=0), dict(direction=0), dict(direction=2), dict(max_t=-1),
                dict(n_rows=1 << 30, pts_per_row=4),                                          # more points than an int32 index holds
                dict(max_t=3), dict(n_poses=0), dict(fx=0.0), dict(fy=float("nan")),          # cameras: a time without a matrix
                dict(t_out=_P), dict(alive_out=_P),                                           # a row's state stepped in place
                dict(raw=None), dict(raw=None, xyz_out=None, t_out=None),                     # a next slab without records
                dict(**no_cam, **no_move)):                                                   # nothing to compute
        assert step(**bad) == -1, bad
    assert step(fixed_view=1, n_poses=1, max_t=7, n_rows=0) == 0                              # one fixed view serves any time
    for missing in ("xyz_in", "t_in", "alive_in", "xyz_out", "t_out", "alive_out", "Ps", "uv", "depth"):
        assert step(**{missing: None}) == -2, missing
    assert step(raw=_P + 4) == -3 and step(xyz_in=_P + 2) == -3 and step(t_out=_P + 129) == -3 and step(uv=_P + 1) == -3
    assert step(n_rows=0) == 0 and step(n_rows=0, **no_cam) == 0                              # no rows: nothing launched
    draw = lambda **kw: lib.nsff_track_draw(C.byref(_draw_args(**kw)), None)
    assert lib.nsff_track_draw(None, None) == -2
    for bad in (dict(H=0), dict(W=-1), dict(H=65536, W=32768), dict(n_steps=0), dict(n_steps=1 << 11), dict(n_tracks=-1),
                dict(n_tracks=1 << 20), dict(scratch_bytes=79)):
        assert draw(**bad) == -1, bad
    for missing in ("uv", "ok", "image", "lut", "out", "scratch"):
        assert draw(**{missing: None}) == -2, missing
    assert draw(scratch=_P + 2) == -3 and draw(uv=_P + 4) == -3
    need = lib.nsff_track_draw_scratch_bytes
    assert need(4, 5) == 80 and need(288, 512) == 4 * 288 * 512 and need(0, 5) == 0 and need(65536, 32768) == 0
    assert C.sizeof(_lib.TrackStepArgs) == 8 + 6 * 4 + 4 * 4 + 10 * 8 and C.sizeof(_lib.TrackDrawArgs) == 4 * 4 + 6 * 8 + 8


def test_header_declares_the_symbols_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint nsff_track_step\(const NsffTrackStepArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint nsff_track_draw\(const NsffTrackDrawArgs\* args, void\* stream\);", header)
    assert re.search(r"\bint64_t nsff_track_draw_scratch_bytes\(int32_t H, int32_t W\);", header)
    for sym in ("nsff_track_step", "nsff_track_draw", "nsff_track_draw_scratch_bytes"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym)
    assert callable(_lib.track_step) and callable(_lib.track_draw) and callable(_lib.track_draw_scratch_bytes)
    assert re.search(r"#define NSFF_TRACK_MAX_TRACKS \(1 << 20\)", header) and _lib.TRACK_MAX_TRACKS == 1 << 20
    assert re.search(r"#define NSFF_TRACK_MAX_STEPS  \(1 << 11\)", header) and _lib.TRACK_MAX_STEPS == 1 << 11
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header)
    assert _lib.load().nsff_abi_version() == _lib.ABI_VERSION == 32
    assert A.advect is tracks.advect and A.draw is tracks.draw and A.tracks is tracks and callable(evaluate.track_panel)
    assert {"tracks", "advect", "draw"} <= set(A.__all__) and tracks.UNKNOWN == 1e10 == float(tnp.UNKNOWN)
    makefile = open(os.path.join(ROOT, "nsff_pl_amd", "csrc", "Makefile")).read()
    assert re.search(r"-ffp-contract=off -c tracks\.hip", makefile)
    assert all("tracks.o" in line for line in makefile.splitlines() if "-shared" in line)     # every library links it


def test_python_layer_refuses_by_name(scene):
    model, emb, _ = scene
    xyz, ts = torch.zeros(4, 3, 3), torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="advect: xyz must be a GPU tensor"):
        tracks.advect(model, emb, xyz, ts, 2, 5)
    with pytest.raises(RuntimeError, match="advect: xyz must be a tensor"):
        tracks.advect(model, emb, xyz.numpy(), ts, 2, 5)
    with pytest.raises(RuntimeError, match="advect: xyz must be float32"):
        tracks.advect(model, emb, xyz.double(), ts, 2, 5)
    with pytest.raises(RuntimeError, match=r"advect: xyz must be \(R, S, 3\) or \(R, 3\)"):
        tracks.advect(model, emb, torch.zeros(4, 3, 2), ts, 2, 5)
    no_flow = A.NeRF("fine", use_viewdir=False, encode_transient=True, in_channels_t=scenes.N_TAU)
    with pytest.raises(RuntimeError, match="advect: the model has no scene-flow heads"):
        tracks.advect(no_flow, emb, xyz, ts, 2, 5)
    for steps in (0, 1.5, True, None):
        with pytest.raises(ValueError, match="advect: steps must be a non-zero integer"):
            tracks.advect(model, emb, xyz, ts, steps, 5)
    for bad in (torch.tensor([0, 1, 6, 2]), torch.tensor([0, -1, 2, 2]), [0, 1, 2, 6], np.array([-1, 0, 0, 0])):
        with pytest.raises(ValueError, match=r"advect: ts outside 0 \.\. max_t = 5"):
            tracks.advect(model, emb, xyz, bad, 2, 5)
    for bad in (torch.zeros(5, dtype=torch.long), torch.zeros(4), torch.zeros(4, 1, dtype=torch.long), [0, 1, 2], [0.0, 1.0, 2.0, 3.0]):
        with pytest.raises(RuntimeError, match=r"advect: ts must be \(4,\) integer start times"):
            tracks.advect(model, emb, xyz, bad, 2, 5)
    with pytest.raises(ValueError, match="advect: max_t = -1 is negative"):
        tracks.advect(model, emb, xyz, ts, 2, -1)
    K, Ps = np.eye(3), np.zeros((1, 6, 3, 4), np.float32)
    with pytest.raises(ValueError, match="advect: Ps is given without K"):
        tracks.advect(model, emb, xyz, ts, 2, 5, Ps=Ps)
    with pytest.raises(ValueError, match="advect: K is given without Ps"):
        tracks.advect(model, emb, xyz, ts, 2, 5, K=K)
    with pytest.raises(RuntimeError, match=r"advect: Ps must be \(N,3,4\), \(1,N,3,4\) or one \(3,4\) view"):
        tracks.advect(model, emb, xyz, ts, 2, 5, Ps=np.zeros((6, 4, 4), np.float32), K=K)
    with pytest.raises(RuntimeError, match=r"advect: K must be \(3,3\) or \(1,3,3\)"):
        tracks.advect(model, emb, xyz, ts, 2, 5, Ps=Ps, K=np.eye(4))
    with pytest.raises(ValueError, match="advect: max_t = 6 is outside the 6 projection matrices"):
        tracks.advect(model, emb, xyz, ts, 2, 6, Ps=Ps, K=K)
    with pytest.raises(ValueError, match="advect: chunk must be at least one row"):
        tracks.advect(model, emb, xyz, ts, 2, 5, chunk=0)
    with pytest.raises(RuntimeError, match="advect: xyz must be a GPU tensor"):                # every shape is fine: the device is not
        tracks.advect(model, emb, xyz, ts, -2, 5, Ps=Ps[0, 0], K=K, chunk=3)

    img, uv, ok, lut = torch.zeros(4, 5, 3, dtype=torch.uint8), torch.zeros(3, 7, 2), torch.ones(3, 7, dtype=torch.bool), tracks.default_lut()
    with pytest.raises(RuntimeError, match="draw: image_u8 must be a GPU tensor"):
        tracks.draw(img, uv, ok, lut)
    with pytest.raises(RuntimeError, match=r"draw: image_u8 must be an \(H, W, 3\) uint8 image"):
        tracks.draw(img.float(), uv, ok, lut)
    with pytest.raises(RuntimeError, match=r"draw: uv must be \(n\+1, Q, 2\) or \(n\+1, R, S, 2\) float32 with n >= 1"):
        tracks.draw(img, uv[:1], ok[:1], lut)
    with pytest.raises(RuntimeError, match="draw: ok must be bool or uint8"):
        tracks.draw(img, uv, ok.float(), lut)
    with pytest.raises(RuntimeError, match=r"draw: ok must be \(3, 7\)"):
        tracks.draw(img, uv, ok[:, :6], lut)
    with pytest.raises(RuntimeError, match=r"draw: ok must be \(3, 7, 2\) like uv or \(3, 7\)"):
        tracks.draw(img, torch.zeros(3, 7, 2, 2), torch.ones(3, 2, dtype=torch.bool), lut)
    with pytest.raises(ValueError, match=r"draw: 1048576 tracks, the pixel key holds fewer than 2\*\*20"):
        tracks.draw(img, torch.zeros(2, 1 << 20, 2), torch.ones(2, 1 << 20, dtype=torch.bool), lut)
    with pytest.raises(ValueError, match=r"draw: 2048 steps, the pixel key holds fewer than 2\*\*11"):
        tracks.draw(img, torch.zeros(2049, 1, 2), torch.ones(2049, 1, dtype=torch.bool), lut)
    assert tracks.default_lut().shape == (256, 3) and tracks.default_lut().dtype == np.uint8
    with pytest.raises(RuntimeError, match="track_panel: models\\['fine'\\] has no scene-flow heads"):
        evaluate.track_panel({"fine": no_flow}, emb, K, np.zeros((3, 3, 4)), 0, (5, 4), 8, 0, 2)
    with pytest.raises(ValueError, match="track_panel: t0 = 3 is outside the sequence of 3 poses"):
        evaluate.track_panel({"fine": model}, emb, K, np.zeros((3, 3, 4)), 3, (5, 4), 8, 0, 2)
    with pytest.raises(ValueError, match="track_panel: steps and stride must be positive"):
        evaluate.track_panel({"fine": model}, emb, K, np.zeros((3, 3, 4)), 0, (5, 4), 8, 0, 0)


# ---- the line rule ----
def test_line_rule_properties():
    rng = np.random.default_rng(31)
    ends = [(0, 0, 0, 0), (3, 4, 3, 4), (0, 0, 7, 0), (0, 0, 0, 7), (0, 0, 7, 7), (0, 0, -7, 7), (0, 0, 2, 9), (0, 0, 9, 2), (5, 5, -4, 1),
            (0, 0, 1, 2), (0, 0, 2, 1), (-3, 8, 4, -9), (0, 0, 65535, 1), (0, 0, 3, -65535)]
    ends += [tuple(int(v) for v in rng.integers(-40, 40, 4)) for _ in range(300)]
    for x0, y0, x1, y1 in ends:
        px = tnp.line_pixels(x0, y0, x1, y1)
        N = max(abs(x1 - x0), abs(y1 - y0))
        assert len(px) == N + 1 and len(set(px)) == N + 1                                     # max(|dx|, |dy|) + 1 distinct pixels
        assert px[0] == (x0, y0) and px[-1] == (x1, y1)                                       # both ends coloured
        steps = np.abs(np.diff(np.array(px), axis=0)) if N else np.zeros((0, 2), int)
        assert (steps.max(1) == 1).all()                                                      # 8-connected, never standing still
        assert len(tnp.line_pixels(x1, y1, x0, y0)) == len(px)                                # reversed ends cover the same count
        if N:                                                                                 # no pixel further than half a pixel from the line
            a = np.array(px) - (x0, y0)
            off = np.abs(a[:, 0] * (y1 - y0) - a[:, 1] * (x1 - x0)) / N
            assert off.max() <= 0.5
    assert tnp.line_pixels(0, 0, 4, 2) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]            # halves round up: 0.5 -> 1, 1.5 -> 2
    assert tnp.round_end(2.5) == 3 and tnp.round_end(-2.5) == -2 and tnp.round_end(-0.4) == 0 and tnp.round_end(7.49) == 7


def test_twin_trail_image_by_hand():
    img = np.full((5, 6, 3), 9, np.uint8)
    lut = np.stack([np.arange(256)] * 3, -1).astype(np.uint8)
    U = tnp.UNKNOWN
    #              track 0: right along row 1, then down   track 1: crosses it   track 2: dead end   track 3: unknown   track 4: too long
    uv = np.array([[[0, 1], [2, 0], [0, 4], [1, 1], [0, 0]],
                   [[3, 1], [2, 3], [5, 4], [U, U], [20, 0]],
                   [[3, 3], [2, 3], [5, 0], [1, 1], [0, 0]]], np.float32)
    ok = np.ones((3, 5), bool)
    ok[1, 2] = False
    keys = tnp.canvas(5, 6, uv, ok)
    k = lambda j, q: ((j + 1) << 20) | q
    want = np.zeros((5, 6), np.uint32)
    want[1, 0:4] = k(0, 0)
    want[0:4, 2] = k(0, 1)                                       # same step, higher track: wins the crossing at (2, 1)
    want[1:4, 3] = k(1, 0)                                       # the later step wins (3, 1)
    want[3, 2] = k(1, 1)                                         # a zero-length segment: its one pixel
    assert np.array_equal(keys, want)
    out = tnp.draw(img, uv, ok, lut)
    assert (out[keys == 0] == 9).all() and (out[1, 0] == 127).all() and (out[2, 3] == 255).all()      # lut[(255 * (j + 1)) // 2]
