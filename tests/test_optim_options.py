"""The reference's optimizer and learning-rate options in the trainer (utils/__init__.py:24-76 get_optimizer / get_scheduler,
opt.py:75-103): the native SGD and RAdam steps (nsff_pl_amd/optim.py, csrc/optim.hip) against torch.optim.SGD /
torch.optim.RAdam(decoupled_weight_decay=True), and the schedules against sequences recorded from the reference's own
schedulers (tests/golden/make_golden_lr.py -> g23_lr_schedules.npz)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import common
import optim_twins
from nsff_pl_amd.optim import FlatAdam, FlatRAdam, FlatSGD

SHAPES = [(256, 63), (256,), (3, 256), (1,), (5, 7, 3), (48, 30)]          # total not a multiple of 4 (tests/test_optim.py)
LR = 5e-4
STEPS = 9                       # RAdam's rho_t crosses 5 at step 6 (beta2 = 0.999): both of its branches run
# The bound of the native steps against torch (the device tests below).  The project's Adam bound is rtol 2e-6, atol 1e-9
# (tests/test_optim.py:155).  Measured on the CPU, on the inputs of _run below (9 steps, the rate change, with and without unused
# tensors): torch's own fp32 optimizers against a float64 run of themselves, worst element of |fp32 - fp64| / (2e-6 |fp64| + 1e-9):
#     SGD    momentum 0.9: 1.41 (wd 0), 2.11 (wd 0.01);   momentum 0: 0.28 (wd 0), 0.40 (wd 0.01)
#     RAdam  1.97 (wd 0), 3.04 (wd 0.01)
# That is more than half of the Adam bound, so the bound here is 2 x the measured deviation per optimizer: the Adam bound scaled by
# 2 x 2.11 for SGD and by 2 x 3.04 for RAdam.  (Nothing in it comes from the kernels under test.)
RTOL, ATOL = 2e-6, 1e-9
BOUND = {"sgd": dict(rtol=2 * 2.11 * RTOL, atol=2 * 2.11 * ATOL), "radam": dict(rtol=2 * 3.04 * RTOL, atol=2 * 3.04 * ATOL)}


def _params(dev, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.3).to(dev, dtype)) for s in SHAPES]


def _run(opt_factory, dev, wd, steps=STEPS, lr_drop_at=5, unused=(), dtype=torch.float32):
    """The gradient generator of tests/test_optim.py.  `unused`: indices of parameters that never receive a gradient (torch:
    .grad stays None; flat: the slice stays zero).  The rate drops x 0.1 after step `lr_drop_at`."""
    params = _params(dev, dtype=dtype)
    opt = opt_factory(params, wd)
    g = torch.Generator().manual_seed(7)
    for i in range(steps):
        opt.zero_grad()
        for k, p in enumerate(params):
            grad = (torch.randn(*p.shape, generator=g) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=g))).to(dev, dtype)
            if k in unused:
                continue
            if p.grad is None:
                p.grad = grad
            else:
                p.grad.copy_(grad)
        opt.step()
        if i + 1 == lr_drop_at:
            if isinstance(opt, (FlatSGD, FlatRAdam)):
                opt.set_lr(float(opt.lr) * 0.1)
            else:
                opt.param_groups[0]["lr"] *= 0.1
    return [p.detach().cpu().numpy().copy() for p in params]


def _torch_sgd(momentum):
    return lambda params, wd: torch.optim.SGD(params, lr=LR, momentum=momentum, weight_decay=wd)


def _torch_radam(params, wd):
    return torch.optim.RAdam(params, lr=LR, eps=1e-8, weight_decay=wd, decoupled_weight_decay=True)


def _flat_sgd(cls, momentum, **kw):
    return lambda params, wd: cls(params, lr=LR, momentum=momentum, weight_decay=wd, **kw)


def _flat_radam(cls, **kw):
    return lambda params, wd: cls(params, lr=LR, eps=1e-8, weight_decay=wd, **kw)


def _assert_close(got, want, rtol, atol=ATOL):
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


# ---- schedules ---------------------------------------------------------------------------------------------------------------

def _lr_golden():
    z = np.load(os.path.join(common.GOLDEN_DIR, "g23_lr_schedules.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k[3:]: z[k] for k in z.files if k.startswith("lr/")}


def _cpu_trainer(hparams, twin=None):
    """A trainer over one small model on the CPU with the torch-op twin of its optimizer (no step is taken: schedules only)."""
    import nsff_pl_amd as A
    from nsff_pl_amd.training import NSFFTrainer
    if twin is None:
        kind = (hparams or {}).get("optimizer", "adam")
        twin = {"adam": common.cpu_flat_adam, "sgd": optim_twins.cpu_flat_sgd, "radam": optim_twins.cpu_flat_radam}[kind]()
    models = {"fine": A.NeRF("fine", use_viewdir=False)}
    emb = {"xyz": A.PosEmbedding(9, 10), "dir": A.PosEmbedding(3, 4)}
    tr = NSFFTrainer(models, emb, 30, hparams, output_transient=False, optimizer_cls=twin)
    return tr.to("cpu")


def _drive(tr, epochs, start=0):
    """on_train_epoch_start(e) / on_train_epoch_end() as the training loop calls them; the rate in force during each epoch."""
    seen = []
    for e in range(start, epochs):
        tr.on_train_epoch_start(e)
        seen.append(float(tr.optimizer.lr))
        tr.on_train_epoch_end()
    return np.asarray(seen, dtype=np.float64)


LR_CASES = [f"{kind}_w{w}_m{m}" for kind in ("steplr", "cosine", "poly") for w, m in ((0, 1), (3, 1), (3, 4))]


@pytest.mark.parametrize("case", [c for c in LR_CASES if not (c.startswith("cosine") and "_w3" in c)])
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_schedules_follow_the_reference_schedulers(case, optimizer):
    """rtol 1e-6: the rate is held as an fp32 device scalar (rounding 6e-8), torch's recursive forms carry a few double ulps."""
    meta, golden = _lr_golden()
    hp = dict(meta["cases"][case], optimizer=optimizer)
    got = _drive(_cpu_trainer(hp), hp["num_epochs"])
    np.testing.assert_allclose(got, golden[case], rtol=1e-6, atol=0)


def test_default_schedule_is_the_in_place_multiplication():
    """steplr without warm-up (the default): bit-identical to multiplying the device scalar by gamma at each milestone."""
    tr = _cpu_trainer(None)
    assert type(tr.optimizer).__mro__[1] is FlatAdam and tr.hp["lr_scheduler"] == "steplr" and tr.hp["optimizer"] == "adam"
    want = torch.tensor(5e-4)
    for e in range(45):
        tr.on_train_epoch_start(e)
        assert torch.equal(tr.optimizer.lr, want), e
        tr.on_train_epoch_end()
        if e + 1 in (20,):
            want = want.mul(0.1)
    meta, golden = _lr_golden()
    hp = meta["cases"]["steplr_w0_m1"]
    tr = _cpu_trainer(hp)
    want = torch.tensor(hp["lr"])
    for e in range(hp["num_epochs"]):
        tr.on_train_epoch_start(e)
        assert torch.equal(tr.optimizer.lr, want), e
        tr.on_train_epoch_end()
        if e + 1 in hp["decay_step"]:
            want = want.mul(hp["decay_gamma"])


@pytest.mark.parametrize("m", [1, 4])
def test_cosine_with_warmup_is_the_clean_rule_not_the_reference_artefact(m):
    """Cosine + warm-up: m * cosine(e - W - 1) after the ramp (training.lr_at).  The reference's own sequence under current
    torch overshoots its peak m * lr at e = W + 1 (CosineAnnealingLR's recursion on a base rate changed under it); it is on
    file in the golden and NOT what the trainer does."""
    meta, golden = _lr_golden()
    case = f"cosine_w3_m{m}"
    hp = meta["cases"][case]
    W, T, lr = hp["warmup_epochs"], hp["num_epochs"], hp["lr"]
    want = [lr * ((m - 1) * e / W + 1) if e <= W else
            1e-8 + (m * lr - 1e-8) * (1 + math.cos(math.pi * (e - W - 1) / T)) / 2 for e in range(T)]
    got = _drive(_cpu_trainer(dict(hp, optimizer="adam")), T)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    assert got.max() <= m * lr * (1 + 1e-6)
    assert golden[case][W + 1] > m * lr * 1.01                  # the documented artefact is really what is recorded
    np.testing.assert_allclose(got[:W + 1], golden[case][:W + 1], rtol=1e-6, atol=0)   # (the ramp itself agrees)


def test_readme_configuration_follows_its_cosine_schedule():
    """README.md:227-233 of the reference: --optimizer adam --lr 5e-4 --lr_scheduler cosine --num_epochs 50."""
    _, golden = _lr_golden()
    tr = _cpu_trainer(dict(optimizer="adam", lr=5e-4, lr_scheduler="cosine", num_epochs=50))
    assert type(tr.optimizer).__mro__[1] is FlatAdam
    got = _drive(tr, 50)
    assert len(golden["readme_cosine"]) == 50 and got[-1] < 0.01 * got[0]
    np.testing.assert_allclose(got, golden["readme_cosine"], rtol=1e-6, atol=0)


# ---- option handling ---------------------------------------------------------------------------------------------------------

def test_unknown_options_are_refused_at_construction():
    with pytest.raises(ValueError, match="torch_optimizer"):
        _cpu_trainer(dict(optimizer="ranger"), twin=common.cpu_flat_adam())
    with pytest.raises(ValueError, match="optimizer not recognized"):
        _cpu_trainer(dict(optimizer="lion"), twin=common.cpu_flat_adam())
    with pytest.raises(ValueError, match="scheduler not recognized"):
        _cpu_trainer(dict(lr_scheduler="exponential"))


def test_hparams_pick_the_optimizer_class():
    from nsff_pl_amd.training import NSFFTrainer
    import nsff_pl_amd as A
    models = {"fine": A.NeRF("fine", use_viewdir=False)}
    emb = {"xyz": A.PosEmbedding(9, 10), "dir": A.PosEmbedding(3, 4)}
    for name, cls in (("adam", FlatAdam), ("sgd", FlatSGD), ("radam", FlatRAdam), (None, FlatAdam)):
        tr = NSFFTrainer(models, emb, 30, None if name is None else dict(optimizer=name), output_transient=False)
        assert tr.optimizer_cls is cls
    tr = _cpu_trainer(dict(optimizer="sgd", momentum=0.5, weight_decay=0.01))
    assert isinstance(tr.optimizer, FlatSGD) and tr.optimizer.momentum == 0.5 and tr.optimizer.weight_decay == 0.01
    assert tr.checkpoint()["optimizer"]["param_groups"][0]["momentum"] == 0.5


def test_radam_ignores_warmup_and_const_never_changes_the_rate():
    meta, golden = _lr_golden()
    hp = dict(meta["cases"]["poly_w3_m4"], optimizer="radam")
    np.testing.assert_allclose(_drive(_cpu_trainer(hp), hp["num_epochs"]), golden["poly_w0_m1"], rtol=1e-6, atol=0)
    tr = _cpu_trainer(dict(lr_scheduler="const", lr=3e-4, num_epochs=12, decay_step=[2]))
    first = tr.optimizer.lr.clone()
    for e in range(12):
        tr.on_train_epoch_start(e)
        tr.on_train_epoch_end()
        assert torch.equal(tr.optimizer.lr, first)


def test_resumed_run_continues_the_schedule_from_the_restored_epoch():
    _, golden = _lr_golden()
    hp = dict(optimizer="adam", lr=5e-4, lr_scheduler="cosine", num_epochs=50)
    tr = _cpu_trainer(hp)
    _drive(tr, 5)
    tr.on_train_epoch_start(5)
    ck = tr.checkpoint()
    assert ck["epoch"] == 5
    fresh = _cpu_trainer(hp)
    fresh.load_checkpoint(ck)
    assert fresh.current_epoch == 5
    got = _drive(fresh, 12, start=5)
    np.testing.assert_allclose(got, golden["readme_cosine"][5:12], rtol=1e-6, atol=0)


# ---- the torch-op twins against torch, CPU -----------------------------------------------------------------------------------

@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_sgd_twin_equals_torch_sgd_on_cpu(wd, momentum):
    cpu = torch.device("cpu")
    got = _run(_flat_sgd(optim_twins.cpu_flat_sgd(), momentum, decay_unused=True), cpu, wd)
    _assert_close(got, _run(_torch_sgd(momentum), cpu, wd), rtol=1e-6)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_radam_twin_equals_torch_radam_on_cpu(wd):
    cpu = torch.device("cpu")
    got = _run(_flat_radam(optim_twins.cpu_flat_radam(), decay_unused=True), cpu, wd)
    _assert_close(got, _run(_torch_radam, cpu, wd), rtol=1e-6)


@pytest.mark.parametrize("which", ["sgd", "radam"])
def test_twins_skip_parameters_without_gradient_like_torch(which):
    cpu, unused = torch.device("cpu"), (2, 3)
    if which == "sgd":
        flat, ref = (lambda **kw: _flat_sgd(optim_twins.cpu_flat_sgd(), 0.9, **kw)), _torch_sgd(0.9)
    else:
        flat, ref = (lambda **kw: _flat_radam(optim_twins.cpu_flat_radam(), **kw)), _torch_radam
    got = _run(flat(), cpu, 0.01, unused=unused)
    _assert_close(got, _run(ref, cpu, 0.01, unused=unused), rtol=1e-6)
    start = [p.detach().numpy() for p in _params(cpu)]
    for k in unused:
        np.testing.assert_array_equal(got[k], start[k])
    decayed = _run(flat(decay_unused=True), cpu, 0.01, unused=unused)
    assert not np.array_equal(decayed[2], start[2])        # the every-element step does decay them


def test_sgd_without_momentum_keeps_no_buffer_and_new_classes_refuse_cpu():
    Twin = optim_twins.cpu_flat_sgd()
    assert Twin(_params(torch.device("cpu")), momentum=0.0).momentum_buffer is None
    assert Twin(_params(torch.device("cpu")), momentum=0.9).momentum_buffer is not None
    for cls in (FlatSGD, FlatRAdam):
        with pytest.raises(RuntimeError, match="HIP device only"):
            cls(_params(torch.device("cpu")))


def test_torch_state_loaders_refuse_other_parameter_lists_and_step_counts():
    cpu = torch.device("cpu")
    pt = _params(cpu)
    for p in pt:
        p.grad = torch.ones_like(p)
    for make, Twin in ((_torch_sgd(0.9), optim_twins.cpu_flat_sgd()), (lambda ps, wd: _torch_radam(ps, wd), optim_twins.cpu_flat_radam())):
        ot = make(pt, 0.0)
        ot.step()
        sd = ot.state_dict()
        with pytest.raises(ValueError, match="parameters"):
            Twin(_params(cpu)[:-1]).load_torch_state_dict(sd)
        Twin(_params(cpu)).load_torch_state_dict(sd)                        # the matching list loads
    o = _torch_radam(pt, 0.0)
    o.step()
    sd = o.state_dict()
    sd["state"][2]["step"] = sd["state"][2]["step"] + 1
    with pytest.raises(ValueError, match="different step counts"):
        optim_twins.cpu_flat_radam()(_params(cpu)).load_torch_state_dict(sd)


# ---- the native steps, on the device -----------------------------------------------------------------------------------------

DEV = torch.device("cuda:0")
UNUSED = (1, 3, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_native_sgd_equals_torch_sgd(wd, momentum, hip_lib):
    """Bound: torch's fp32 SGD against a float64 run of itself on these inputs (CPU) deviates by up to 2.11 x the project's Adam
    bound (rtol 2e-6, atol 1e-9) -- more than half of it -- so the bound is 2 x that measurement: rtol 8.44e-6, atol 4.22e-9."""
    _assert_close(_run(_flat_sgd(FlatSGD, momentum, decay_unused=True), DEV, wd), _run(_torch_sgd(momentum), DEV, wd), **BOUND["sgd"])


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_native_radam_equals_torch_radam(wd, hip_lib):
    """Bound: torch's fp32 RAdam against a float64 run of itself on these inputs (CPU) deviates by up to 3.04 x the project's Adam
    bound (rtol 2e-6, atol 1e-9) -- more than half of it -- so the bound is 2 x that measurement: rtol 1.216e-5, atol 6.08e-9."""
    _assert_close(_run(_flat_radam(FlatRAdam, decay_unused=True), DEV, wd), _run(_torch_radam, DEV, wd), **BOUND["radam"])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["sgd", "sgd0", "radam"])
def test_native_steps_skip_parameters_without_gradient_like_torch(which, hip_lib):
    """The segment form (weight_decay > 0): tensors 1, 3, 4 never receive a gradient and stay bit-equal to their start values;
    tensor boundaries are not float4-aligned in SHAPES, so straddling float4s are exercised."""
    flat, ref = {"sgd": (_flat_sgd(FlatSGD, 0.9), _torch_sgd(0.9)), "sgd0": (_flat_sgd(FlatSGD, 0.0), _torch_sgd(0.0)),
                 "radam": (_flat_radam(FlatRAdam), _torch_radam)}[which]
    got, want = _run(flat, DEV, 0.01, unused=UNUSED), _run(ref, DEV, 0.01, unused=UNUSED)
    start = [p.detach().cpu().numpy() for p in _params(DEV)]
    _assert_close(got, want, **BOUND[which.rstrip("0")])
    for k in UNUSED:
        np.testing.assert_array_equal(got[k], start[k])


WRAP_N = 2048 * 256 * 4 + 1024 + 3          # one pass of the capped launch + a ragged tail: the grid-stride loop wraps


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["sgd", "radam"])
def test_native_steps_wrap_the_stride_loop(which, hip_lib):
    g = torch.Generator().manual_seed(5)
    start = torch.randn(WRAP_N, generator=g) * 0.3
    grads = [torch.randn(WRAP_N, generator=g).to(DEV) for _ in range(2)]
    pf, pt = torch.nn.Parameter(start.to(DEV)), torch.nn.Parameter(start.to(DEV))
    if which == "sgd":
        of, ot = FlatSGD([pf], lr=LR, momentum=0.9, weight_decay=0.01), torch.optim.SGD([pt], lr=LR, momentum=0.9, weight_decay=0.01)
    else:
        of, ot = FlatRAdam([pf], lr=LR, weight_decay=0.01), _torch_radam([pt], 0.01)
    assert of.flat_param.numel() == WRAP_N + 1
    for gr in grads:
        pf.grad.copy_(gr)
        pt.grad = gr.clone()
        of.step(); ot.step()
    got, want = pf.detach().cpu().numpy(), pt.detach().cpu().numpy()
    assert not np.array_equal(got[-1027:], start.numpy()[-1027:])           # the tail was stepped
    np.testing.assert_allclose(got, want, **BOUND[which])
    assert float(of.flat_param[WRAP_N]) == 0.0                              # the padding element: zero gradient, zero value


def _radam_at_step_4(params):
    """A FlatRAdam whose state was loaded at step 4 (flat layout), so that steps 5, 6, 7 cross the rho_t > 5 switch."""
    opt = FlatRAdam(params, lr=1e-3, weight_decay=0.01)
    g = torch.Generator().manual_seed(11)
    sd = opt.state_dict()
    sd["step"] = torch.full_like(sd["step"], 4.0)
    sd["exp_avg"] = (torch.randn(opt.numel, generator=g) * 0.05).to(DEV)
    sd["exp_avg_sq"] = (torch.rand(opt.numel, generator=g) * 0.01).to(DEV)
    opt.load_state_dict(sd)
    return opt


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["sgd", "radam"])
def test_native_steps_replay_from_a_captured_graph(which, hip_lib):
    """One warm-up step on a side stream, step() captured, two replays with set_lr between them == three eager steps with the
    same rate change, bit for bit; the device step count reads 3 (RAdam: 4 + 3, across the switch of its two branches)."""
    make = (lambda ps: FlatSGD(ps, lr=1e-3, momentum=0.9, weight_decay=0.01)) if which == "sgd" else _radam_at_step_4
    opt, ref = make(_params(DEV)), make(_params(DEV))
    first = 0.0 if which == "sgd" else 4.0
    assert float(opt.state[0]) == first
    opt.flat_grad[:opt.numel].fill_(0.5)
    opt.flat_grad[1::3] *= -2.0
    ref.flat_grad.copy_(opt.flat_grad)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                          # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    graph.replay()
    opt.set_lr(2.5e-4)
    graph.replay()                                          # warm-up + two replays = three steps
    ref.step(); ref.step()
    ref.set_lr(2.5e-4)
    ref.step()
    torch.cuda.synchronize()
    assert float(opt.state[0]) == float(ref.state[0]) == first + 3.0
    assert torch.equal(opt.flat_param, ref.flat_param)
    if which == "radam":
        assert float(ref.state[4]) == 1.0                   # ended on the rectified branch ...
        probe = _radam_at_step_4(_params(DEV))
        probe.flat_grad.copy_(ref.flat_grad)
        probe.step()
        assert float(probe.state[4]) == 0.0                 # ... and started on the other one (step 5)
    else:
        assert torch.equal(opt.momentum_buffer, ref.momentum_buffer)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["sgd", "radam"])
def test_optimizer_state_round_trips_through_torch(which, hip_lib):
    """Three steps in torch, load_torch_state_dict, two steps here == five steps in torch; and back into a fresh torch optimizer."""
    g = torch.Generator().manual_seed(21)
    grads = [[(torch.randn(*s, generator=g) * 0.1).to(DEV) for s in SHAPES] for _ in range(5)]
    make_t = _torch_sgd(0.9) if which == "sgd" else _torch_radam

    def run(opt, params, steps):
        for i in steps:
            for p, gr in zip(params, grads[i]):
                if p.grad is None:
                    p.grad = gr.clone()
                else:
                    p.grad.copy_(gr)
            opt.step()
    pt = _params(DEV)
    ot = make_t(pt, 0.01)
    run(ot, pt, range(3))
    pf = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    of = FlatSGD(pf, lr=1.0, momentum=0.5) if which == "sgd" else FlatRAdam(pf, lr=1.0)   # (hyper-parameters come from the state)
    of.load_torch_state_dict(ot.state_dict())
    assert abs(float(of.lr) - LR) < 1e-9 and of.weight_decay == 0.01
    assert of.momentum == 0.9 if which == "sgd" else float(of.state[0]) == 3.0
    run(of, pf, range(3, 5))
    run(ot, pt, range(3, 5))
    _assert_close([p.detach().cpu().numpy() for p in pf], [p.detach().cpu().numpy() for p in pt], **BOUND[which])
    back = of.torch_state_dict()
    p2 = [torch.nn.Parameter(p.detach().clone()) for p in pf]
    o2 = make_t(p2, 0.01)
    o2.load_state_dict(back)
    name = "momentum_buffer" if which == "sgd" else "exp_avg"
    assert torch.equal(o2.state[p2[1]][name], back["state"][1][name])
    if which == "radam":
        assert int(o2.state[p2[0]]["step"]) == 5
    # clones, not views of the flat buffers
    flat = of.momentum_buffer if which == "sgd" else of.exp_avg
    keep = back["state"][0][name].clone()
    flat.add_(1.0)
    assert torch.equal(back["state"][0][name], keep)
    assert not (flat.data_ptr() <= back["state"][0][name].data_ptr() < flat.data_ptr() + 4 * flat.numel())


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer,graph", [("sgd", False), ("radam", False), ("sgd", True)])
def test_trainer_steps_checkpoints_and_restores_with_the_new_optimizers(optimizer, graph, hip_lib):
    import scenes
    import nsff_pl_amd as A
    from nsff_pl_amd.training import NSFFTrainer
    cfg, meta, rays, ts, models, emb, _, _ = common.build_case("g3_nsff_train", A.NeRF, A.PosEmbedding)
    Ks, Ps, _ = scenes.camera_buffers()
    hp = dict(N_samples=cfg["N_samples"], N_importance=cfg["N_importance"], perturb=0, noise_std=0, optimizer=optimizer)
    tr = NSFFTrainer(models, emb, scenes.N_FRAMES, hp, Ks, Ps, output_transient_flow=cfg["flow"], graph=graph).to(DEV)
    assert type(tr.optimizer) is {"sgd": FlatSGD, "radam": FlatRAdam}[optimizer]
    tr.on_train_epoch_start(0)
    batch = {k: v.to(DEV) for k, v in scenes.synthetic_targets(cfg["n_rays"], ts, cfg["seed"]).items()}
    batch["rays"] = rays.to(DEV)
    start = tr.checkpoint()["state_dict"]
    log = tr.step(batch)
    assert torch.isfinite(log["train/loss"]) and float(tr.optimizer.state[0]) == 1.0
    if graph:                                   # one captured step: the warm-up steps were undone, one step of the schedule remains
        assert any(not torch.equal(v, start[k]) for k, v in tr.checkpoint()["state_dict"].items())
        return
    tr.step(batch)
    ck = tr.checkpoint()
    at_ckpt = {k: v.clone() for k, v in ck["state_dict"].items()}
    assert any(not torch.equal(at_ckpt[k], start[k]) for k in at_ckpt)
    tr.step(batch)
    assert any(not torch.equal(tr.checkpoint()["state_dict"][k], at_ckpt[k]) for k in at_ckpt)
    tr.load_checkpoint(ck)
    back = tr.checkpoint()
    assert all(torch.equal(back["state_dict"][k], at_ckpt[k]) for k in at_ckpt) and tr.optimizer.in_place()
    name = "momentum_buffer" if optimizer == "sgd" else "exp_avg"
    assert len(back["optimizer"]["state"]) == len(tr.params)
    assert all(torch.equal(back["optimizer"]["state"][i][name], ck["optimizer"]["state"][i][name]) for i in range(len(tr.params)))
    if optimizer == "radam":
        assert int(back["optimizer"]["state"][0]["step"]) == 2
    torch_cls = torch.optim.SGD if optimizer == "sgd" else torch.optim.RAdam
    fresh = torch_cls([torch.nn.Parameter(p.detach().clone()) for p in tr.params], lr=1.0)
    fresh.load_state_dict(back["optimizer"])                                # the restored state converts to torch's format
    assert abs(fresh.param_groups[0]["lr"] - 5e-4) < 1e-9
