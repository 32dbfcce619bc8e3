"""The f16x3 value-domain flag: NSFF_RANGE_* / nsff_range_flags, ``nsff_pl_amd.range_flags`` and the modes of
``config.set_range_check`` (value domain).  The CPU part checks the configuration, the decoding and the binding;
the GPU part drives every f16x3 kernel form on both sides of the fp16 range and checks that the flag -- and nothing else --
tells them apart."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import nsff_pl_amd as A
from nsff_pl_amd import _lib, config, range_check
from nsff_pl_amd.range_check import RangeFlags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


# ---------------------------------------------------------------- CPU ----------------------------------------------------
def test_set_range_check_validates():
    assert config.get_range_check() == "off"
    try:
        for mode in ("warn", "raise", "fallback", "off"):
            A.set_range_check(mode)
            assert A.get_range_check() == mode
        with pytest.raises(ValueError):
            A.set_range_check("loud")
        assert A.get_range_check() == "off"
    finally:
        A.set_range_check("off")


@pytest.mark.parametrize("value,ok", [("warn", True), ("fallback", True), ("bogus", False)])
def test_range_check_environment_variable(value, ok):
    env = dict(os.environ, NSFF_RANGE_CHECK=value)
    code = "import nsff_pl_amd.config as c; print(c.get_range_check())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    if ok:
        assert r.returncode == 0 and r.stdout.strip() == value, r.stderr
    else:
        assert r.returncode != 0 and "NSFF_RANGE_CHECK" in r.stderr


def test_range_flags_decoding():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    bits = {}
    for name in ("ACT", "SAVED", "PARAMS", "CODES"):
        line = next(l for l in header.splitlines() if l.startswith(f"#define NSFF_RANGE_{name} "))
        bits[name] = int(line.split()[2].rstrip("u"), 16)
    assert bits == {"ACT": RangeFlags.ACTIVATIONS, "SAVED": RangeFlags.SAVED_ACTIVATIONS, "PARAMS": RangeFlags.PARAMETERS,
                    "CODES": RangeFlags.CODES}
    f = RangeFlags(0x5)
    assert RangeFlags.ACTIVATIONS in f and RangeFlags.PARAMETERS in f and RangeFlags.CODES not in f
    assert range_check.describe(f) == "activations, parameters"
    assert range_check.describe(RangeFlags(0)) == "none" and not RangeFlags(0)
    assert int(RangeFlags(0x10 | 0x2)) == 0x12                  # unknown bits survive the decoding


def test_range_flags_symbol_is_bound():
    assert "nsff_range_flags" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    fn = lib.nsff_range_flags
    assert fn.restype is C.c_int and len(fn.argtypes) == 3
    assert fn(None, 1, None) == -2                              # NSFF_ERR_NULL before any GPU work
    assert lib.nsff_abi_version() == 32


def test_modes_off_calls_run_unchecked(monkeypatch):
    calls = []
    monkeypatch.setattr(range_check, "range_flags", lambda *a, **k: calls.append(a) or RangeFlags(0))
    assert range_check.checked("x", "cpu", lambda: 7, True) == 7 and calls == []


def test_modes_warn_raise_fallback(monkeypatch):
    """The policy around one call, with the device word replaced by a stub that reports ACTIVATIONS after the first run."""
    state = {"word": 0, "runs": []}

    def flags(device=None, clear=True):
        w = state["word"]
        if clear:
            state["word"] = 0
        return RangeFlags(w)

    def run():
        state["runs"].append(config.get_precision())
        if config.get_precision() == "f16x3":
            state["word"] |= 1
        return len(state["runs"])
    monkeypatch.setattr(range_check, "range_flags", flags)
    monkeypatch.setattr(range_check.torch.cuda, "is_current_stream_capturing", lambda: False)
    try:
        A.set_range_check("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert range_check.checked("render_rays", "cuda:0", run, True) == 1
        assert len(w) == 1 and issubclass(w[0].category, RuntimeWarning) and "activations" in str(w[0].message)
        assert "set_precision('f32')" in str(w[0].message)
        A.set_range_check("raise")
        with pytest.raises(RuntimeError, match="activations"):
            range_check.checked("render_rays", "cuda:0", run, True)
        A.set_range_check("fallback")
        state["runs"].clear()
        assert range_check.checked("render_rays", "cuda:0", run, True) == 2 and state["runs"] == ["f16x3", "f32"]
        assert config.get_precision() == "f16x3"
        with pytest.raises(RuntimeError):
            range_check.checked("render_rays", "cuda:0", run, False)
        with range_check.suppressed():
            assert range_check.active() == "off"
    finally:
        A.set_range_check("off")


# ---------------------------------------------------------------- GPU ----------------------------------------------------
FORMS = [  # (tile_points, persistent, points, expected kernel)
    (0, True, 4096, "h3_64"), (0, True, 40960, "h3a"), (0, False, 40960, "h3a"), (64, True, 40960, "h3_64"),
    (130, True, 4096, "h3a"), (130, False, 40960, "h3a"), (131, True, 4096, "h3_8wave"), (131, True, 40960, "h3_8wave"),
]


def _domain_model():
    """test_f16x3_value_domain's construction: a D = 3 model whose layer-0 gain sets the size of the hidden activations"""
    A.range_flags()                                             # (the word is sticky: start every test from zero)
    torch.manual_seed(5)
    m = A.NeRF("coarse", D=3, skips=[], use_viewdir=False).to(DEV)
    emb = A.PosEmbedding(9, 10)
    w0 = m.static_xyz_encoding_1[0].weight.detach().clone()
    b0 = m.static_xyz_encoding_1[0].bias.detach()
    xyz = (torch.rand(40960, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    x = emb(xyz)
    act = lambda gain: float(torch.relu(x @ (w0 * gain).T + b0).abs().max())
    gains = {"in": 3.0e4 / act(1.0), "out": 1.0e6 / act(1.0)}
    assert 2.0e4 < act(gains["in"]) < 6.5e4 and act(gains["out"]) > 5e5

    def set_gain(g):
        with torch.no_grad():
            m.static_xyz_encoding_1[0].weight.copy_(w0 * g)
    return m, emb, xyz, gains, set_gain


def _query(m, emb, xyz, n, tile, persistent, precision="f16x3"):
    config.set_precision(precision)
    config.set_tile_points(tile)
    try:
        with config.launch_form(persistent=persistent):
            raw = torch.empty(n, _lib.RAW_STRIDE, device=DEV)
            _lib.field_query(m, raw, n, 1, 2, 0, 0, xyz=xyz[:n].contiguous(), freqs=[float(f) for f in emb.freqs])
            torch.cuda.synchronize()
            return raw, _lib.last_field_kernel()
    finally:
        config.set_tile_points(0)
        config.set_precision(config.DEFAULT_PRECISION)


@pytest.mark.gpu
def test_every_f16x3_form_flags_out_of_range_activations(hip_lib):
    m, emb, xyz, gains, set_gain = _domain_model()
    for tile, persistent, n, kernel in FORMS:
        for side, gain in gains.items():
            set_gain(gain)
            _query(m, emb, xyz, 128, 0, True)                   # (packs the weights at this gain, outside the check below)
            A.range_flags()
            _, got = _query(m, emb, xyz, n, tile, persistent)
            assert got == kernel, (tile, persistent, n, got)
            f = A.range_flags(clear=False)
            want = RangeFlags.ACTIVATIONS if side == "out" else RangeFlags(0)
            assert f == want, (tile, persistent, n, side, f)
            assert A.range_flags() == want                       # clear=False kept it; this read clears it
            assert A.range_flags() == RangeFlags(0)
            _query(m, emb, xyz, n, tile, persistent, precision="f32")
            assert A.range_flags() == RangeFlags(0), "f32 arithmetic never sets a bit"


@pytest.mark.gpu
def test_flag_is_asynchronous_and_capturable(hip_lib):
    m, emb, xyz, gains, set_gain = _domain_model()
    set_gain(gains["out"])
    _query(m, emb, xyz, 40960, 0, True)
    out = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.range_flags(out, False)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.range_flags(out, True)
    A.range_flags(clear=False)
    g.replay()
    torch.cuda.synchronize()
    assert int(out.item()) == int(RangeFlags.ACTIVATIONS) and A.range_flags() == RangeFlags(0)


@pytest.mark.gpu
def test_outputs_are_bit_identical_in_every_mode(hip_lib):
    import scenes
    m, emb, xyz, gains, set_gain = _domain_model()
    set_gain(gains["in"])
    x_in = torch.cat([emb(xyz[:4096]), torch.zeros(4096, m.in_channels_dir, device=DEV)], 1)
    cfg = dict(scenes.CASES["g3_nsff_train"], n_rays=64)
    rays, ts = scenes.synthetic_rays(cfg["n_rays"], cfg["seed"])
    models, sembs = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
    _to_dev(models, sembs)
    kw = scenes.render_kwargs(cfg)
    outs = {}
    try:
        for mode in ("off", "warn", "raise", "fallback"):
            A.set_range_check(mode)
            with torch.no_grad():
                a = m(x_in, sigma_only=False, output_transient=False)
                r = A.render_rays(models, sembs, rays.to(DEV), ts.to(DEV), scenes.N_FRAMES - 1, cfg["N_samples"], 0, 0,
                                  cfg["N_importance"], 32768, test_time=True, **kw)
            outs[mode] = [a.cpu().numpy()] + [v.cpu().numpy() for _, v in sorted(r.items())]
    finally:
        A.set_range_check("off")
    for mode in ("warn", "raise", "fallback"):
        assert all(np.array_equal(x, y) for x, y in zip(outs["off"], outs[mode])), mode


def _to_dev(models, emb):
    for m in models.values():
        m.to(DEV)
    for k in ("t", "a"):
        if k in emb:
            emb[k].to(DEV)


def _scene(name="g3_nsff_train", n_rays=64):
    import scenes
    A.range_flags()
    cfg = dict(scenes.CASES[name] if isinstance(name, str) else name, n_rays=n_rays)
    rays, ts = scenes.synthetic_rays(cfg["n_rays"], cfg["seed"])
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
    _to_dev(models, emb)
    return cfg, rays.to(DEV), ts.to(DEV), models, emb, scenes.render_kwargs(cfg)


def _blow_up(models, gain):
    with torch.no_grad():
        for m in models.values():
            m.static_xyz_encoding_1[0].weight.mul_(gain)
            m._pack_cache.invalidate()


@pytest.mark.gpu
@pytest.mark.parametrize("grad_precision", ["f16", "f16x3"])
def test_training_forward_flags_saved_activations(hip_lib, grad_precision):
    import scenes
    cfg, rays, ts, models, emb, kw = _scene(n_rays=256)
    _blow_up(models, 1e5)
    config.set_grad_precision(grad_precision)
    try:
        A.range_flags()
        res = A.render_rays(models, emb, rays, ts, scenes.N_FRAMES - 1, cfg["N_samples"], 0, 0, cfg["N_importance"], 32768,
                            test_time=False, **kw)
        scenes.cotangent_loss(res).backward()
        torch.cuda.synchronize()
        assert _lib.last_field_kernel() in ("h3a_save", "h3_save")
        assert RangeFlags.SAVED_ACTIVATIONS in A.range_flags()
    finally:
        config.set_grad_precision("f16")


def _trainer(graph, case="g3_nsff_train", n_rays=128):
    import scenes
    from nsff_pl_amd.training import NSFFTrainer
    cfg, rays, ts, models, emb, kw = _scene(case, n_rays=n_rays)
    Ks, Ps, _ = scenes.camera_buffers()
    hp = dict(N_samples=cfg["N_samples"], N_importance=cfg["N_importance"], perturb=0, noise_std=0)
    tr = NSFFTrainer(models, emb, scenes.N_FRAMES, hp, Ks, Ps, output_transient_flow=cfg["flow"], graph=graph).to(DEV)
    tr.on_train_epoch_start(scenes.LOSS_EPOCH)
    batch = {k: v.to(DEV) for k, v in scenes.synthetic_targets(cfg["n_rays"], ts.cpu(), cfg["seed"]).items()}
    batch["rays"] = rays
    A.range_flags()                                             # (the word is sticky: what earlier work left is not this trainer's)
    return tr, models, batch


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_trainer_raise_leaves_weights_and_adam_untouched(hip_lib, graph):
    tr, models, batch = _trainer(graph)
    tr.step(batch)                                              # (graph: captured here, in range)
    assert A.range_flags() == RangeFlags(0)
    _blow_up(models, 1e5)
    before = [p.detach().clone() for p in tr.params]
    opt_before = [t.detach().clone() for t in _optimizer_tensors(tr.optimizer)]
    try:
        A.set_range_check("raise")
        with pytest.raises(RuntimeError, match="NSFFTrainer.step"):
            tr.step(batch)
    finally:
        A.set_range_check("off")
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, tr.params))
    opt_after = _optimizer_tensors(tr.optimizer)
    assert len(opt_after) == len(opt_before) and all(torch.equal(a, b) for a, b in zip(opt_before, opt_after))


def _optimizer_tensors(opt):
    out = []

    def walk(x):
        if torch.is_tensor(x):
            out.append(x)
        elif isinstance(x, dict):
            for k in sorted(x, key=str):
                walk(x[k])
        elif isinstance(x, (list, tuple)):
            for v in x:
                walk(v)
    walk(opt.state_dict())
    return out


@pytest.mark.gpu
def test_packing_flags_out_of_range_parameters(hip_lib):
    m, emb, xyz, gains, set_gain = _domain_model()
    _query(m, emb, xyz, 128, 0, True)
    assert A.range_flags() == RangeFlags(0)
    with torch.no_grad():
        m.static_xyz_encoding_2[0].weight[3, 7] = 1e5
    m._pack_cache.invalidate()
    m.packed(config.PRECISIONS["f16x3"])
    torch.cuda.synchronize()
    assert A.range_flags() == RangeFlags.PARAMETERS
    m.packed(config.PRECISIONS["f32"])
    m._pack_cache.invalidate()
    m.packed(config.PRECISIONS["f32"])
    torch.cuda.synchronize()
    assert A.range_flags() == RangeFlags(0)


@pytest.mark.gpu
def test_modes_on_the_device(hip_lib):
    import scenes
    m, emb, xyz, gains, set_gain = _domain_model()
    set_gain(gains["out"])
    x_in = torch.cat([emb(xyz[:4096]), torch.zeros(4096, m.in_channels_dir, device=DEV)], 1)
    cfg, rays, ts, models, sembs, kw = _scene()
    _blow_up(models, 1e5)
    args = (models, sembs, rays, ts, scenes.N_FRAMES - 1, cfg["N_samples"])
    try:
        A.set_range_check("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            with torch.no_grad():
                A.render_rays(*args, 0, 0, cfg["N_importance"], 32768, test_time=True, **kw)
        assert len([x for x in w if issubclass(x.category, RuntimeWarning)]) == 1
        A.set_range_check("raise")
        with pytest.raises(RuntimeError, match="render_rays"):
            with torch.no_grad():
                A.render_rays(*args, 0, 0, cfg["N_importance"], 32768, test_time=True, **kw)
        with pytest.raises(RuntimeError, match="NeRF.forward"):
            with torch.no_grad():
                m(x_in, sigma_only=False, output_transient=False)
        A.set_range_check("fallback")
        with torch.no_grad():
            got_r = A.render_rays(*args, 0, 0, cfg["N_importance"], 32768, test_time=True, **kw)
            got_m = m(x_in, sigma_only=False, output_transient=False)
        with pytest.raises(RuntimeError, match="render_rays"):
            with torch.no_grad():
                A.render_rays(*args, 1, 0, cfg["N_importance"], 32768, test_time=True, **kw)
        A.set_range_check("off")
        A.set_precision("f32")
        with torch.no_grad():
            want_r = A.render_rays(*args, 0, 0, cfg["N_importance"], 32768, test_time=True, **kw)
            want_m = m(x_in, sigma_only=False, output_transient=False)
    finally:
        A.set_range_check("off")
        A.set_precision(config.DEFAULT_PRECISION)
    assert torch.equal(got_m, want_m)
    assert sorted(got_r) == sorted(want_r) and all(torch.equal(got_r[k], want_r[k]) for k in want_r)


@pytest.mark.gpu
def test_no_false_positives(hip_lib):
    import scenes
    A.range_flags()
    for name in scenes.CASES:
        for tile in (0, 64, 130, 131):
            cfg, rays, ts, models, emb, kw = _scene(name, n_rays=scenes.CASES[name].get("n_rays", 64))
            config.set_tile_points(tile)
            try:
                with torch.no_grad():
                    A.render_rays(models, emb, rays, ts, scenes.N_FRAMES - 1, cfg["N_samples"], 0, 0, cfg["N_importance"], 32768,
                                  test_time=True, **kw)
                torch.cuda.synchronize()
            finally:
                config.set_tile_points(0)
            assert A.range_flags() == RangeFlags(0), (name, tile)
    for graph in (False, True):
        tr, models, batch = _trainer(graph)
        for _ in range(2):
            tr.step(batch)
        torch.cuda.synchronize()
        assert A.range_flags() == RangeFlags(0), graph


@pytest.mark.gpu
def test_no_false_positives_at_the_golden_training_sizes_and_a_full_frame(hip_lib):
    """the golden training configurations (g20: the README's, g21: C2's, 512 rays each) and one 512 x 288 frame leave the word at 0"""
    import scenes
    from nsff_pl_amd import evaluate
    for case in (scenes.README_TRAIN_CASE, scenes.C2_TRAIN_CASE):
        for graph in (False, True):
            tr, models, batch = _trainer(graph, case, n_rays=case["n_rays"])
            for _ in range(2):
                tr.step(batch)
            torch.cuda.synchronize()
            assert A.range_flags() == RangeFlags(0), (case["seed"], graph)
    cfg, _, _, models, emb, kw = _scene("g4_nsff_test")
    H, W = 288, 512
    K = np.array([[400., 0, W / 2], [0, 400., H / 2], [0, 0, 1]], np.float32)
    c2w = np.array([[1, 0, 0, 0.05], [0, 1, 0, -0.02], [0, 0, 1, 0.1]], np.float32)
    rays = evaluate.frame_rays(K, c2w, H, W, device=DEV)
    ts = torch.full((H * W,), 7, dtype=torch.long, device=DEV)
    out = evaluate.render_frame(models, emb, rays, ts, scenes.N_FRAMES - 1, 64, 64, chunk=32768, keys=("rgb_fine",), **kw)
    torch.cuda.synchronize()
    assert out["rgb_fine"].shape == (H * W, 3)
    assert _lib.last_field_kernel().startswith("h3a")
    assert A.range_flags() == RangeFlags(0)
