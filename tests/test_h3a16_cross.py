"""The hand-scheduled inference kernel on v_mfma_f32_16x16x32_f16 (nsff_field_kernel_h3a16, NSFF_H3A_SHAPE=16, tile_points 130): the
schedule, phase programs and arguments of nsff_field_kernel_h3a, another MFMA shape and a repacked weight buffer.  Checked here:
records against the oracle (1e-4, tests/parity.py); persistent launches against one workgroup per tile, bit for bit; its error
against the exact-fp32 kernel beside the 32-shape body's (the two differ in fp32 summation order only); the repacked buffer against
a numpy restatement of its layout; which shape a launch reports, and that NSFF_H3A_SHAPE=32 restores the 32-shape body's records bit for bit.

What is compared with what: the oracle comparison runs for the both-trunk launches of the small cases; static-only, dynamic-only and
the 32 896-point launches are held to the exact-fp32 kernel (2e-5) and, persistent against per-tile, bit for bit.  "NSFF_H3A_SHAPE=32
restores the parent's records" compares two 32-shape paths of this tree (the switch, and a caller without the second buffer): the
only comparison one tree allows; bench.py's A/B against the parent's own tree is in EXPERIMENTS.md section R11.

Models: the C2 architecture (D = 8, skip at 4), D = 2 without a skip, D = 4 with a skip at 2 (the input tile's rebuild); static-only,
dynamic-only and both-trunk launches with the flow heads; the time code as per-ray bias rows and through the matrix pipe (A8F / B8).
Points: 256 (two tiles), 300 (ragged last tile), 32 768 + 128 of one trunk (one tile more than the part has compute units: a persistent
workgroup walks two tiles)."""
import os

import numpy as np
import pytest
import torch

import parity
import nsff_pl_amd as A
from nsff_pl_amd import _lib, config
from oracle import nsff_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ARCHS = [(8, [4], 10, 48), (2, [], 6, 16), (4, [2], 10, 48)]          # D, skips, n_freqs, n_tau
MODES = [(2, 2, 2), (2, 0, 0), (0, 2, 1)]                            # (static_mode, transient_mode, flow heads)
GROUPS = ((0, 4), (4, 8), (8, 14))                                   # record floats: static, dynamic, flows
# Assertion 3: the largest error of the 16-shape records against the exact-fp32 kernel over the cases of this file may exceed the
# 32-shape body's by this factor = 2 x the ratio measured on these cases on the MI355X (EXPERIMENTS.md, section R11), 4 at most.
ERR_FACTOR = 2 * 1.035


def _model(arch, seed):
    D, skips, n_freqs, n_tau = arch
    torch.manual_seed(seed)
    m = A.NeRF("fine", D=D, skips=skips, in_channels_xyz=3 + 6 * n_freqs, use_viewdir=False, encode_transient=True,
               in_channels_t=n_tau, output_flow=True)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(".weight"):
                p.mul_(2.5)
    return m.to(DEV), [float(f) for f in A.PosEmbedding(n_freqs - 1, n_freqs).freqs]


def _launch(m, P, S, mode, xyz, freqs, t_rows, shape=None, precision="f16x3", t_bias=None, no_persist=False):
    """one field launch -> (records, kernel name, workgroups, MFMA shape reported); shape None: NSFF_H3A_SHAPE unset"""
    sm, tm, fh = mode
    keep = {k: os.environ.get(k) for k in ("NSFF_H3A_SHAPE", "NSFF_NO_PERSIST")}
    for k, v in (("NSFF_H3A_SHAPE", None if shape is None else str(shape)), ("NSFF_NO_PERSIST", "1" if no_persist else None)):
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    config.set_precision("f16x3")
    config.set_tile_points(130)
    raw = torch.full((P, _lib.RAW_STRIDE), float("nan"), device=DEV)
    try:
        _lib.field_query(m, raw, P, S, sm, tm, fh, xyz=xyz, freqs=freqs, t_emb=t_rows if tm else None, t_bias=t_bias,
                         precision=config.PRECISIONS[precision])
        torch.cuda.synchronize()
        return raw.cpu().numpy(), _lib.last_field_kernel(), _lib.last_field_grid(), _lib.last_field_mfma_shape()
    finally:
        config.set_tile_points(0)
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _err(got, ref, mode):
    """largest difference over the launch's record groups, relative to the group's largest reference value"""
    sm, tm, fh = mode
    worst = 0.0
    for (lo, hi), on in zip(GROUPS, (sm, tm, tm and fh)):
        if on:
            hi = min(hi, 8 + 3 * fh) if lo == 8 else hi
            worst = max(worst, float(np.abs(got[:, lo:hi] - ref[:, lo:hi]).max() / max(np.abs(ref[:, lo:hi]).max(), 1e-30)))
    return worst


@pytest.fixture(scope="module")
def runs(hip_lib):
    """every small case once: the 16-shape, the 32-shape and the exact-fp32 records of the same inputs"""
    out = []
    for ai, arch in enumerate(ARCHS):
        m, freqs = _model(arch, 700 + ai)
        g = torch.Generator().manual_seed(40 + ai)
        for P, S in ((256, 64), (300, 60)):
            n_rays = P // S
            xyz = (torch.rand(P, 3, generator=g) * 2.4 - 1.2).to(DEV)
            t_rows = torch.randn(n_rays, arch[3], generator=g).to(DEV)
            for mode in MODES:
                for rows in ((False, True) if (mode[1] and S % 64 == 0) else (False,)):
                    tb = _lib.time_bias([(m, t_rows)])[0] if rows else None
                    r16, k16, _, s16 = _launch(m, P, S, mode, xyz, freqs, t_rows, 16, t_bias=tb)
                    r32, k32, _, s32 = _launch(m, P, S, mode, xyz, freqs, t_rows, 32, t_bias=tb)
                    rf, kf, _, _ = _launch(m, P, S, mode, xyz, freqs, t_rows, 16, precision="f32")
                    out.append(dict(ai=ai, arch=arch, P=P, S=S, mode=mode, rows=rows, m=m, freqs=freqs, xyz=xyz, t_rows=t_rows,
                                    r16=r16, r32=r32, rf=rf, k16=k16, k32=k32, kf=kf, s16=s16, s32=s32))
    return out


def test_covered_launches_run_the_16_shape_kernel(runs):
    for r in runs:
        want = "h3a_tb" if r["rows"] else "h3a"
        assert r["k16"] == want and r["k32"] == want and r["kf"] == "f32", (r["arch"], r["P"], r["mode"], r["k16"], r["k32"], r["kf"])
        assert r["s16"] == 16 and r["s32"] == 32, (r["arch"], r["P"], r["mode"], r["s16"], r["s32"])
        sm, tm, fh = r["mode"]
        used = slice(0, 4) if tm == 0 else (slice(4, 8 + 3 * fh) if sm == 0 else slice(0, 8 + 3 * fh))
        assert np.isfinite(r["r16"][:, used]).all()
        assert not np.array_equal(r["r16"][:, used], r["r32"][:, used]), "the two shapes add in different orders: equal records mean one kernel ran twice"


@pytest.mark.parametrize("ai", range(len(ARCHS)))
@pytest.mark.parametrize("P", [256, 300])
def test_records_match_the_oracle(runs, ai, P):
    """both trunks with the flow heads, time code through the matrix pipe and (P = 256) as per-ray rows: 1e-4 of the key's largest value"""
    cases = [r for r in runs if r["ai"] == ai and r["P"] == P and r["mode"] == (2, 2, 2)]
    assert len(cases) == (2 if P == 256 else 1)
    r = cases[0]
    f = orc.field_from_module(r["m"])
    x_emb = np.concatenate([orc.pos_embedding(r["xyz"].cpu().numpy(), np.asarray(r["freqs"], np.float32)),
                            np.repeat(r["t_rows"].cpu().numpy(), r["S"], 0)], 1)
    want = orc.nerf_forward(f["params"], dict(f["cfg"], in_dir=0, in_a=0), x_emb, output_transient=True, output_transient_flow=("fw", "bw"))
    for r in cases:
        worst = parity.assert_close(f"arch {r['arch']} P={P} rows={r['rows']} (16-shape) vs oracle", r["r16"][:, 0:14], want, parity.RTOL)
        print(f"16-shape vs oracle: arch {r['arch']} P={P} rows={r['rows']}: {worst:.2e}")


@pytest.fixture(scope="module")
def big(hip_lib):
    """32 768 + 128 points of ONE trunk of the C2 model: static-only, and dynamic-only with per-ray time rows"""
    m, freqs = _model(ARCHS[0], 900)
    g = torch.Generator().manual_seed(77)
    S, P = 64, 32768 + 128
    xyz = (torch.rand(P, 3, generator=g) * 2.4 - 1.2).to(DEV)
    t_rows = torch.randn(P // S, ARCHS[0][3], generator=g).to(DEV)
    out = []
    for mode, rows in (((2, 0, 0), False), ((0, 2, 1), True)):
        tb = _lib.time_bias([(m, t_rows)])[0] if rows else None
        out.append(dict(mode=mode, rows=rows, P=P,
                        pers=_launch(m, P, S, mode, xyz, freqs, t_rows, 16, t_bias=tb),
                        tile=_launch(m, P, S, mode, xyz, freqs, t_rows, 16, t_bias=tb, no_persist=True),
                        r32=_launch(m, P, S, mode, xyz, freqs, t_rows, 32, t_bias=tb)[0],
                        rf=_launch(m, P, S, mode, xyz, freqs, t_rows, 16, precision="f32")[0]))
    return out


def test_persistent_16_shape_launch_is_bit_identical_to_one_workgroup_per_tile(big):
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    for b in big:
        (a, ka, ga, sa), (t, kt, gt, st) = b["pers"], b["tile"]
        tiles = (b["P"] + 127) // 128
        assert ka == kt == ("h3a_tb" if b["rows"] else "h3a") and sa == st == 16, (ka, kt, sa, st)
        assert gt == tiles and ga == (n_cus if tiles >= n_cus and n_cus % 8 == 0 else tiles), (ga, gt, tiles, n_cus)
        used = slice(0, 4) if b["mode"][1] == 0 else slice(4, 8 + 3 * b["mode"][2])
        assert np.isfinite(a[:, used]).all()
        assert np.array_equal(a.view(np.uint32), t.view(np.uint32)), b["mode"]


def test_16_shape_error_against_exact_fp32_beside_the_32_shape_bodys(runs, big):
    """the yardstick is the exact-fp32 kernel; the largest error over every case of this file, per shape"""
    e16 = e32 = 0.0
    for r in runs:
        e16, e32 = max(e16, _err(r["r16"], r["rf"], r["mode"])), max(e32, _err(r["r32"], r["rf"], r["mode"]))
    for b in big:
        e16, e32 = max(e16, _err(b["pers"][0], b["rf"], b["mode"])), max(e32, _err(b["r32"], b["rf"], b["mode"]))
    print(f"largest error against the exact-fp32 kernel: 16-shape {e16:.3e}, 32-shape {e32:.3e}, ratio {e16 / e32:.3f}")
    assert 0.0 < e32 < 2e-5 and e16 < 2e-5, (e16, e32)
    assert ERR_FACTOR <= 4 and e16 <= ERR_FACTOR * e32, (e16, e32, e16 / e32)


def test_repacked_buffer_is_the_permutation_of_the_trunk_segments(hip_lib):
    """the second buffer of the C2 model against the layout's definition: chunk [wave][slot j][mt'][part][lane = 16 g + c] holds
    part(W[64 wave + 16 (2 (j & 1) + mt') + c][32 (j >> 1) + 8 g + t]), t = 0..7; every word outside the trunk segments (biases, head tiles,
    folded rows, the *_final layers) is the first pack's"""
    m, _ = _model(ARCHS[0], 31)
    config.set_precision("f16x3")
    src = m.packed(config.PRECISIONS["f16x3"]).view(torch.int32).cpu().numpy().view(np.uint32).copy()
    dst = m.packed(_lib.REPACKED).view(torch.int32).cpu().numpy().view(np.uint32).copy()
    torch.cuda.synchronize()
    assert src.shape == dst.shape
    steps, n_static, _, _ = _lib.h3a_program(m, 2, 2)
    assert len(steps) == 2 * (ARCHS[0][0] + len(ARCHS[0][1])) and n_static == len(steps) // 2
    trunk = np.zeros(src.size, bool)
    lane = np.arange(64)
    for (w, _b, nks, _pre, _post, _head) in steps:
        n_words = nks * 4096                            # 256 rows x 16 nks columns x (hi + lo) halfs
        assert not trunk[w:w + n_words].any()
        trunk[w:w + n_words] = True
        old = src[w:w + n_words].view(np.uint16).reshape(4, nks, 2, 2, 64, 8)      # [wave][ks][mt][part][lane][t]
        W = np.zeros((2, 256, 16 * nks), np.uint16)                                # [part][neuron][column]
        for wv in range(4):
            for ks in range(nks):
                for mt in range(2):
                    for t in range(8):
                        W[:, 64 * wv + 32 * mt + (lane & 31), 16 * ks + 8 * (lane >> 5) + t] = old[wv, ks, mt, :, :, t]
        want = np.zeros((4, nks, 2, 2, 64, 8), np.uint16)
        for wv in range(4):
            for j in range(nks):
                for mt in range(2):
                    for t in range(8):
                        want[wv, j, mt, :, :, t] = W[:, 64 * wv + 16 * (2 * (j & 1) + mt) + (lane & 15), 32 * (j >> 1) + 8 * (lane >> 4) + t]
        assert np.array_equal(dst[w:w + n_words].view(np.uint16), want.reshape(-1)), f"segment at word {w}"
        assert not np.array_equal(dst[w:w + n_words], src[w:w + n_words])
    assert trunk.any() and not trunk.all()
    assert np.array_equal(dst[~trunk], src[~trunk])


def test_shape_switch_and_view_direction_models(hip_lib, runs, monkeypatch):
    """unset, covered launches run the 16 shape; NSFF_H3A_SHAPE=32 gives what a caller without the second buffer gets (plain
    nsff_field_query: the kernel of before), bit for bit; a view-direction model reports 32 whatever the switch says"""
    r = next(r for r in runs if r["ai"] == 0 and r["P"] == 300 and r["mode"] == (2, 2, 2))
    d, kd, _, sd = _launch(r["m"], r["P"], r["S"], r["mode"], r["xyz"], r["freqs"], r["t_rows"], None)
    assert kd == "h3a" and sd == 16
    assert np.array_equal(d.view(np.uint32), r["r16"].view(np.uint32))
    # the same launch through nsff_field_query itself: no second buffer, the 32-shape kernel
    monkeypatch.setattr(_lib.load(), "nsff_field_mfma_shape", lambda *a: 32)       # (field_query then never builds or passes the buffer)
    p, kp, _, sp = _launch(r["m"], r["P"], r["S"], r["mode"], r["xyz"], r["freqs"], r["t_rows"], None)
    monkeypatch.undo()
    assert kp == "h3a" and sp == 32 and np.array_equal(p.view(np.uint32), r["r32"].view(np.uint32))
    torch.manual_seed(11)
    emb_d = A.PosEmbedding(3, 4)
    v = A.NeRF("fine", use_viewdir=True, encode_transient=True, in_channels_t=48, output_flow=True).to(DEV)
    g = torch.Generator().manual_seed(2)
    S, n_rays = 64, 4
    P = S * n_rays
    xyz = (torch.rand(P, 3, generator=g) * 2 - 1).to(DEV)
    t_rows = torch.randn(n_rays, 48, generator=g).to(DEV)
    dirs = emb_d(torch.randn(n_rays, 3, generator=g).to(DEV)).contiguous()
    freqs = [float(f) for f in A.PosEmbedding(9, 10).freqs]
    got = {}
    for shape in (16, 32):
        os.environ["NSFF_H3A_SHAPE"] = str(shape)
        config.set_precision("f16x3"); config.set_tile_points(130)
        try:
            for rows in (False, True):
                raw = torch.full((P, _lib.RAW_STRIDE), float("nan"), device=DEV)
                _lib.field_query(v, raw, P, S, 2, 2, 2, xyz=xyz, freqs=freqs, t_emb=t_rows, dir_emb=dirs,
                                 s_bias=_lib.side_bias(v, dirs, None) if rows else None)
                torch.cuda.synchronize()
                assert _lib.last_field_kernel() == ("h3a_side" if rows else "h3a") and _lib.last_field_mfma_shape() == 32
                got[shape, rows] = raw.cpu().numpy()
        finally:
            config.set_tile_points(0)
            os.environ.pop("NSFF_H3A_SHAPE", None)
    for rows in (False, True):
        assert np.array_equal(got[16, rows].view(np.uint32), got[32, rows].view(np.uint32))
