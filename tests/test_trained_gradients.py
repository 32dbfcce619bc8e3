"""Training gradients against float64 on TRAINED weights.

Every other gradient test (test_gradients.py, test_losses.py's g20 / g21, test_grad_x3.py, test_field_grad.py) runs at seeded
initial weights, where a weight gradient's per-point terms dpre_p (x) h_p mostly add up.  On a batch a network has been trained on
they mostly cancel: the total is small, the terms are as large as before -- the regime in which a reduced-precision backward goes
wrong.  Here the student of test_trained_scene.py is trained on one fixed 512-ray batch (the README batch size) and the native
backward of the training loss is compared with float64 autograd of the torch expression of the same step (tests/torch_path.py at
the native forward's depths) at steps 0, 100 and 300, on the training batch and on a fresh batch of the same teacher, in both
backward arithmetics.

How much a gradient cancels is measured by tests/grad_condition.py: kappa = ||A||_1 / ||g||_1 with A the float64 sum of the
absolute per-point products (A_W = |dpre|^T |h|, A_b = sum_p |dpre_p|; embedding tables: |g|).  Bounds, per tensor, on
scenes.grad_stats and on the full gradients of scenes.FULL_GRAD_PARAMS -- the suite's own, unchanged:

* f16x3 (three products): 2e-4 ||g64||_1 + 3 x scatter (test_grad_x3.py),
* f16 (one product, the default): 2e-3 ||g64||_1 + 3 x scatter (test_gradients.py),

where the scatter is the largest deviation from float64 of the torch expression in fp32 and of ULP_RUNS fp32 runs with every
parameter and every ray perturbed by one ulp -- measured at the SNAPSHOT's weights, since it grows with the cancellation.

CPU part: the tolerance itself, at golden scene g3's seeded weights.  A one-product fp16 backward emulated in float64 (fp16
operands with a power of two per point, float64 accumulation) passes the f16 bound; planted defects -- one tensor's gradient x 1.01,
the smallest-|dpre| points carrying 1 % of ||A||_1 left out of the weight gradients (what an underflowing per-trunk scale does),
one head row zeroed -- fail it.
"""
import contextlib
import os
import time

import numpy as np
import pytest
import torch

import common
import grad_condition as GC
import parity
import scenes
import test_gradients as TG
import torch_path
import nsff_pl_amd as A

F16_RTOL = TG.GRAD_RTOL                  # 2e-3
X3_RTOL = 2e-4                           # test_grad_x3.X3_RTOL


def failures(stats, full, s64, full64, scatter, rtol, fp32_A=None):
    """Every statistic / full gradient outside  rtol ||g64||_1 + 3 x scatter  (test_gradients._check_grads' bound) as a list of
    (tensor, statistic, error, tolerance); empty = pass.  fp32_A (only at the student's initialisation, see INIT_FP32_TERM):
    {tensor: A} -- the statistics' bound gains 4 x 2^-24 ||A||_1, the rounding of one fp32 evaluation at that conditioning."""
    bad = []
    scale = max(abs(v[1]) for v in s64.values())
    for pname, want in s64.items():
        mag = max(want[1], 1e-6 * scale)
        for i in range(3):
            tol = rtol * mag + 3 * scatter[pname][i] + (0.0 if fp32_A is None else 4 * 2.0 ** -24 * float(fp32_A[pname].sum()))
            err = abs(stats[pname][i] - want[i])
            if not err <= tol:
                bad.append((pname, i, err, tol))
    for pname, want in full64.items():
        rel = max(scatter[pname]) / max(s64[pname][1], 1e-30) * want.size ** 0.5
        ok = np.isfinite(full[pname]).all()
        err = parity.max_rel_err(full[pname], want) if ok else float("inf")
        if not err <= rtol + 3 * rel:
            bad.append(("full " + pname, None, err, rtol + 3 * rel))
    return bad


def needed_rtol(stats, s64, scatter):
    """the smallest rtol with which the statistics pass, and the tensor that needs it"""
    scale = max(abs(v[1]) for v in s64.values())
    worst = (-float("inf"), "")
    for pname, want in s64.items():
        mag = max(want[1], 1e-6 * scale)
        for i in range(3):
            worst = max(worst, ((abs(stats[pname][i] - want[i]) - 3 * scatter[pname][i]) / mag, pname))
    return worst


# ------------------------------------------------------------------------------------------------------------------ CPU part

G3 = "g3_nsff_train"


def _g3_grads(hook=None, dt=torch.float64):
    """golden scene g3 at its seeded weights through the torch expression at the golden depths, objective = the NSFF loss
    (test_gradients.objective_fn, G10); returns (models, embeddings) with .grad set."""
    cfg, meta, rays, ts, models, emb, _, want = common.build_case(G3, A.NeRF, A.PosEmbedding)
    draws = scenes.replay_draws(cfg, meta["draw_seed"])
    for m in list(models.values()) + [emb["t"]]:
        m.to(dt)
    rec = TG._record(cfg, want, draws, rays.to(dt))
    rec = {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in rec.items()}
    with hook if hook is not None else contextlib.nullcontext():
        res = torch_path.recompute(models, emb, rays.to(dt), ts, scenes.N_FRAMES - 1, rec)
        TG.objective_fn(G3, "nsff_loss", dt)(res).backward()
    return models, emb


@pytest.fixture(scope="module")
def g3_emulated():
    models, emb = _g3_grads(GC.LinHook(emulate=True))
    return models, emb, TG.grad_truth(G3, "nsff_loss")


def test_hook_sums_equal_per_point_sums_and_leave_the_gradient_alone():
    """A_W / A_b of the hook against an explicit loop over points (pre-activation gradients from retain_grad), on a scene of two
    rays; every linear layer of both models is seen -- *_xyz_encoding_final too; the hook's gradients are autograd's."""
    import torch.nn.functional as F
    cfg = dict(scenes.CASES[G3], n_rays=2, N_samples=12, N_importance=6)
    rays, ts = scenes.synthetic_rays(2, 5)
    rays = rays.double()
    g = torch.Generator().manual_seed(3)
    zs_c = torch.linspace(0, 1, 12, dtype=torch.float64).expand(2, 12).contiguous()
    zs_f = torch.sort(torch.rand(2, 12 + 2 * 6, generator=g, dtype=torch.float64), 1)[0]
    rec = dict(N_importance=6, noise_std=0.0, output_transient=True, flows=list(cfg["flow"]), zs_coarse=zs_c, zs_fine=zs_f,
               view_dir=rays[:, 3:6], t_embedded_override=None, a_embedded_override=None)

    def run(hook, lin=None):
        models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
        for m in list(models.values()) + [emb["t"]]:
            m.double()
        old = torch_path._lin
        if lin is not None:
            torch_path._lin = lin
        try:
            with hook if hook is not None else contextlib.nullcontext():
                res = torch_path.recompute(models, emb, rays, ts, scenes.N_FRAMES - 1, rec)
                scenes.cotangent_loss(res).backward()
        finally:
            torch_path._lin = old
        return models, emb

    calls = []

    def recording_lin(mod, x):
        layer = mod[0] if isinstance(mod, torch.nn.Sequential) else mod
        pre = F.linear(x, layer.weight, layer.bias)
        pre.retain_grad()
        calls.append((layer, x.detach(), pre))
        return pre

    models_r, emb_r = run(None, recording_lin)
    hook = GC.LinHook()
    models_h, emb_h = run(hook)
    named_r, named_h = scenes.named_grad_params(models_r, emb_r), scenes.named_grad_params(models_h, emb_h)
    for (n, p), (_, q) in zip(named_r, named_h):
        assert torch.allclose(q.grad, p.grad, rtol=1e-12, atol=1e-14 * float(p.grad.abs().max())), n
    brute = {}
    for layer, x, pre in calls:
        aw, ab = brute.get(layer, (torch.zeros_like(layer.weight), torch.zeros_like(layer.bias)))
        for p in range(x.shape[0]):
            aw = aw + torch.outer(pre.grad[p].abs(), x[p].abs())
            ab = ab + pre.grad[p].abs()
        brute[layer] = (aw, ab)
    linears = {n: m for key in sorted(models_r) for n, m in
               ((f"{key}.{n}", m) for n, m in models_r[key].named_modules()) if isinstance(m, torch.nn.Linear)}
    assert len(linears) == 46 and set(brute) == set(linears.values())
    assert sum(1 for n in linears if n.endswith("xyz_encoding_final")) == 4
    A_h = hook.named_A(named_h)
    for n, layer in linears.items():
        aw, ab = brute[layer]
        assert float(aw.sum()) > 0, n
        assert torch.allclose(A_h[n + ".weight"], aw, rtol=1e-12, atol=0), n
        assert torch.allclose(A_h[n + ".bias"], ab, rtol=1e-12, atol=0), n
        # |g| <= A elementwise: A bounds the gradient it is the absolute sum of
        w = dict(named_h)[n + ".weight"]
        assert (w.grad.abs() <= A_h[n + ".weight"] * (1 + 1e-12) + 1e-300).all(), n
    assert torch.equal(A_h["t.weight"], dict(named_h)["t.weight"].grad.abs())


def test_emulated_one_product_backward_passes_the_f16_bound(g3_emulated):
    """fp16 operands (a power of two per point), float64 accumulation: the arithmetic of the default backward, which the f16
    bound must admit -- and which is measurably not float64 (the check is not vacuous)."""
    models, emb, (s64, full64, scatter) = g3_emulated
    stats, full = scenes.grad_stats(models, emb)
    assert failures(stats, full, s64, full64, scatter, F16_RTOL) == []
    need, where = needed_rtol(stats, s64, scatter)
    print(f"\nemulated one-product backward on g3: rtol needed {need:.2e} ({where})")
    assert max(abs(stats[n][1] - s64[n][1]) / s64[n][1] for n in s64 if s64[n][1] > 0) > 1e-6


@pytest.mark.parametrize("defect", ["scale 1.01", "drop 1 % of A", "zero head row"])
def test_planted_defects_fail_the_f16_bound(defect, g3_emulated):
    """The same emulated backward with one defect planted must FAIL the f16 bound: a one-per-cent systematic error of one weight
    tensor, an underflow that loses the smallest-|dpre| points carrying 1 % of ||A_W||_1 of every layer call (data gradients kept),
    one row of a head's weight gradient zeroed."""
    _, _, (s64, full64, scatter) = g3_emulated
    if defect.startswith("drop"):
        hook = GC.LinHook(emulate=True, drop=0.01)
        models, emb = _g3_grads(hook)
        assert hook.dropped > 0
    else:
        models, emb = _g3_grads(GC.LinHook(emulate=True))
        named = dict(scenes.named_grad_params(models, emb))
        with torch.no_grad():
            if defect.startswith("scale"):
                named["fine.transient_xyz_encoding_4.0.weight"].grad.mul_(1.01)
            else:
                named["fine.transient_rgb.0.weight"].grad[1].zero_()
                named["fine.transient_rgb.0.bias"].grad[1].zero_()
    stats, full = scenes.grad_stats(models, emb)
    bad = failures(stats, full, s64, full64, scatter, F16_RTOL)
    print(f"\n{defect}: {len(bad)} statistics outside the f16 bound, e.g. {bad[:2]}")
    assert bad


# ------------------------------------------------------------------------------------------------------------------ GPU part

N_RAYS, STEPS, SNAPSHOTS = 512, 300, (0, 100, 300)
CFG = dict(scenes.CASES[G3], n_rays=N_RAYS)
BATCHES = {"train": (77, 9), "fresh": (78, 10)}           # (ray seed, synthetic-target seed); rgbs = the teacher's colours
# At the student's initialisation (plain torch init, gain 1) the sigma heads' gradients cancel by up to 2e5 (kappa of
# fine.transient_sigma.bias 1.9e5, coarse.static_sigma.bias 3.4e5): there the fp32 torch expression itself is 4.1e-3 (L1) from
# float64, further than either native arithmetic (3.2e-3), and fine.static_sigma's statistics missed rtol + 3 x scatter by up to
# 14 % -- in BOTH arithmetics alike, and with the exact-fp32 forward as well (measured on the MI355X): fp32 rounding upstream of
# the field backward at that conditioning, not the backward's arithmetic.  Only there the statistics' bound gains the rounding of
# one fp32 evaluation, 4 x 2^-24 ||A||_1, and the native L1 error must stay within 1.5 x the fp32 torch expression's.
INIT_FP32_TERM = (0,)
ULP_RUNS = 8                # one-ulp-perturbed fp32 runs of the scatter (test_gradients.grad_truth: 3)


@contextlib.contextmanager
def _env(key, value):
    old = os.environ.get(key)
    os.environ[key] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[key]
        else:
            os.environ[key] = old


def _student(snap):
    models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, dict(CFG, seed=202, gain=1.0))
    with torch.no_grad():
        for n, p in scenes.named_grad_params(models, emb):
            p.copy_(snap[n])
    return models, emb


def _loss(dt, targets, dev):
    from nsff_pl_amd.losses import NeRFWLoss
    loss_fn = NeRFWLoss(lambda_geo=0.04, thickness=1, topk=1.0)
    Ks, Ps, max_t = scenes.camera_buffers()
    loss_fn.register_buffer("Ks", Ks.to(dt))
    loss_fn.register_buffer("Ps", Ps.to(dt))
    loss_fn.max_t = max_t
    loss_fn.to(dev)
    tg = {k: (v.to(dt) if v.is_floating_point() else v).to(dev) for k, v in targets.items()}
    kw = scenes.render_kwargs(CFG)
    return lambda res: sum(loss_fn(res, tg, epoch=scenes.LOSS_EPOCH, **kw).values())


def _flat(models, emb):
    return torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad).detach().double().flatten()
                      for _, p in scenes.named_grad_params(models, emb)])


@pytest.fixture(scope="module")
def trained(hip_lib):
    """The teacher-student setup of test_trained_scene.py on one fixed 512-ray batch, trained in the default arithmetic; the
    parameters at SNAPSHOTS (CPU clones) and the two evaluation batches (CPU)."""
    from test_gpu_parity import _to_dev, DEV
    from test_trained_scene import _render
    from nsff_pl_amd.training import NSFFTrainer
    t0 = time.time()
    teacher, emb_t = scenes.build_scene(A.NeRF, A.PosEmbedding, dict(CFG, seed=101))
    _to_dev(teacher, emb_t)
    batches = {}
    for tag, (ray_seed, tgt_seed) in BATCHES.items():
        rays, ts = scenes.synthetic_rays(N_RAYS, ray_seed)
        targets = scenes.synthetic_targets(N_RAYS, ts, tgt_seed)
        targets["rgbs"] = _render(teacher, emb_t, rays.to(DEV), ts.to(DEV), CFG, "f32")["rgb_fine"].cpu()
        assert float(targets["rgbs"].std()) > 0.05
        batches[tag] = (rays, ts, targets)
    assert A.config.get_grad_precision() == "f16"
    student, emb_s = scenes.build_scene(A.NeRF, A.PosEmbedding, dict(CFG, seed=202, gain=1.0))
    Ks, Ps, _ = scenes.camera_buffers()
    hp = dict(N_samples=CFG["N_samples"], N_importance=CFG["N_importance"], perturb=1.0, noise_std=0.0, lambda_geo_init=0.0)
    tr = NSFFTrainer(student, emb_s, scenes.N_FRAMES, hp, Ks, Ps, output_transient_flow=CFG["flow"]).to(DEV)
    tr.on_train_epoch_start(0)
    rays, ts, targets = batches["train"]
    batch = {k: v.to(DEV) for k, v in targets.items()}
    batch["rays"], batch["ts"] = rays.to(DEV), ts.to(DEV)
    torch.manual_seed(1234)
    snaps, psnr = {}, {}
    for i in range(STEPS + 1):
        if i in SNAPSHOTS:
            snaps[i] = {n: p.detach().cpu().clone() for n, p in scenes.named_grad_params(student, emb_s)}
        if i < STEPS:
            log = tr.step(batch)
            if i + 1 in SNAPSHOTS:
                psnr[i + 1] = float(log["train/psnr"])
    print(f"\ntrained {STEPS} steps of {N_RAYS} rays in {time.time() - t0:.1f} s; training-batch PSNR {psnr}")
    return snaps, batches


def _native(snap, batch, mode, zs_fine=None):
    """render_rays (f16x3 forward, perturb 0, noise 0, train mode) + NSFF loss + backward through the native kernels in the given
    backward arithmetic; zs_fine: evaluate the fine pass at these depths."""
    from test_gpu_parity import _to_dev, DEV
    from nsff_pl_amd import _lib
    models, emb = _student(snap)
    _to_dev(models, emb)
    rays, ts, targets = batch
    A.config.set_grad_precision(mode)
    try:
        res = common.render_rays_at(zs_fine)(models, emb, rays.to(DEV), ts.to(DEV), scenes.N_FRAMES - 1, CFG["N_samples"], 0, 0,
                                             CFG["N_importance"], 1024 * 32, test_time=False, **scenes.render_kwargs(CFG))
        _loss(torch.float32, targets, DEV)(res).backward()
        torch.cuda.synchronize()
        assert (_lib.last_bwd_kernel() == "x3") == (mode == "f16x3")
    finally:
        A.config.set_grad_precision("f16")
    stats, full = scenes.grad_stats(models, emb)
    return stats, full, _flat(models, emb), (res["zs_coarse"].detach(), res["zs_fine"].detach())


def _torch(snap, batch, zs, dt, hook=None, ulp_seed=0):
    """tests/torch_path.py at the depths zs, the same loss, in dt on the GPU (torch expression of the loss, not the fused kernels);
    ulp_seed > 0: every parameter times (1 + 6e-8 N(0,1)) first, as test_gradients.grad_truth does -- and the rays as well: the
    points o + d z carry one rounding in any fp32 evaluation, and where a gradient cancels by 1e5 (the student's initialisation)
    that rounding, amplified by sin(2^9 x), is the largest part of the fp32 error, common to every run at the same fp32 points."""
    from test_gpu_parity import DEV
    models, emb = _student(snap)
    rays, ts, targets = batch
    if ulp_seed:
        g = torch.Generator().manual_seed(ulp_seed)
        with torch.no_grad():
            for _, p in scenes.named_grad_params(models, emb):
                p.mul_(1 + 6e-8 * torch.randn(p.shape, generator=g))
            rays = rays * (1 + 6e-8 * torch.randn(rays.shape, generator=g))
    for m in list(models.values()) + [emb["t"]]:
        m.to(DEV).to(dt)
    r = rays.to(DEV, dt)
    rec = dict(N_importance=CFG["N_importance"], noise_std=0.0, output_transient=True, flows=list(CFG["flow"]),
               zs_coarse=zs[0].to(dt), zs_fine=zs[1].to(dt), view_dir=r[:, 3:6], t_embedded_override=None, a_embedded_override=None)
    with _env("NSFF_FUSED_LOSS", "0"), (hook if hook is not None else contextlib.nullcontext()):
        res = torch_path.recompute(models, emb, r, ts.to(DEV), scenes.N_FRAMES - 1, rec)
        _loss(dt, targets, DEV)(res).backward()
    torch.cuda.synchronize()
    stats, full = scenes.grad_stats(models, emb)
    named = scenes.named_grad_params(models, emb)
    return stats, full, _flat(models, emb), (hook.named_A(named) if hook is not None and not hook.emulate else None)


def _summary(flat, flat64):
    d = float((flat - flat64).abs().sum() / flat64.abs().sum())
    cos = float(torch.dot(flat, flat64) / (flat.norm() * flat64.norm()))
    return d, cos


@pytest.mark.gpu
def test_trained_weight_gradients_against_float64(trained, hip_lib):
    """Both backward arithmetics at steps 0 / 100 / 300 of training, on the training batch and on a fresh batch, against float64
    autograd of the same step at the same depths -- per tensor at the suite's bounds (module text)."""
    snaps, batches = trained
    t0 = time.time()
    old_tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    A.set_precision("f16x3")
    rows, problems = [], []
    try:
        for step in SNAPSHOTS:
            for tag, batch in batches.items():
                snap = snaps[step]
                n16 = _native(snap, batch, "f16")
                zs = n16[3]
                n3 = _native(snap, batch, "f16x3", zs_fine=zs[1])
                s64, full64, flat64, Amap = _torch(snap, batch, zs, torch.float64, hook=GC.LinHook())
                emu = _torch(snap, batch, zs, torch.float64, hook=GC.LinHook(emulate=True))
                runs32 = [_torch(snap, batch, zs, torch.float32, ulp_seed=u) for u in range(ULP_RUNS + 1)]
                samples = [r[0] for r in runs32]
                scatter = {k: [max(abs(s[k][i] - s64[k][i]) for s in samples) for i in range(3)] for k in s64}
                d32 = _summary(runs32[0][2], flat64)[0]
                kap = {n: float(Amap[n].sum()) / s64[n][1] for n in s64 if s64[n][1] > 0}
                kmax = max(kap, key=kap.get)
                for arith, (stats, full, flat) in (("f16", n16[:3]), ("f16x3", n3[:3]), ("emul f16", emu[:3])):
                    d, cos = _summary(flat, flat64)
                    need, where = needed_rtol(stats, s64, scatter)
                    # error beyond the scatter in units of 2^-11 ||A||_1, worst tensor
                    inA = max(((abs(stats[n][i] - s64[n][i]) - 3 * scatter[n][i]) / (GC.U16 * float(Amap[n].sum())), n)
                              for n in s64 if float(Amap[n].sum()) > 0 for i in range(3))
                    rows.append((step, tag, arith, d, cos, kap[kmax], kmax, need, where, inA))
                    rtol = {"f16": F16_RTOL, "f16x3": X3_RTOL}.get(arith)
                    if rtol is not None:
                        bad = failures(stats, full, s64, full64, scatter, rtol, Amap if step in INIT_FP32_TERM else None)
                        if step in INIT_FP32_TERM and not d < 1.5 * d32:       # (no further from float64 than fp32 torch is)
                            bad.append(("rel L1", None, d, 1.5 * d32))
                        if bad:
                            problems.append((step, tag, arith, bad))
                rows.append((step, tag, "fp32 torch", d32, _summary(runs32[0][2], flat64)[1], kap[kmax], kmax,
                             *needed_rtol(samples[0], s64, scatter), (0.0, "")))
                print(f"step {step:3d} {tag:5s}: kappa per tensor (largest six): "
                      + ", ".join(f"{n} {kap[n]:.1f}" for n in sorted(kap, key=kap.get, reverse=True)[:6]), flush=True)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old_tf32
        A.set_precision(A.config.DEFAULT_PRECISION)
        A.config.set_grad_precision("f16")
    print(f"\nstep  batch  arithmetic   rel L1 err   cosine        max kappa   rtol needed (tensor)        err / 2^-11 ||A||_1")
    for step, tag, arith, d, cos, k, kn, need, where, inA in rows:
        print(f"{step:4d}  {tag:5s}  {arith:9s}  {d:10.3e}  {cos:.9f}  {k:9.1f}   {need:9.2e} {where:34s} {inA[0]:7.3f} {inA[1]}")
    print(f"(gradient evaluations: {time.time() - t0:.1f} s)")
    for p in problems:
        print("OUTSIDE:", p[:3], p[3][:6])
    assert not problems
