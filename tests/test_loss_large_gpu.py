"""The fused loss above 4096 rays (csrc/loss.hip: nsff_nerfw_loss_ex, radix select over many workgroups) on the MI355X: against
the torch expression it replaces there, bit for bit against the rank-counting kernels where both run, against the numpy
restatement of the selection rule (tests/select_rule.py) on tied data, captured in a graph, through NSFFTrainer.step and against
the reference's own numbers (golden g22).  Render dicts are seeded random leaves of the right shapes: no render is needed."""
import functools
import json

import numpy as np
import pytest
import torch

import common
import parity
import scenes
import select_rule
import nsff_pl_amd as A
from nsff_pl_amd import _lib, fused_loss
from nsff_pl_amd.losses import NeRFWLoss

pytestmark = pytest.mark.gpu
FLOW = ["fw", "bw", "disocc"]
TERM_RTOL, GRAD_RTOL = 2e-5, 2e-4          # the bounds of test_fused_loss_kernels_equal_the_torch_expression


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=2)
def _render(n, s, seed, coarse=True):
    return select_rule.synthetic_render(n, s, seed, coarse)


def _targets(n, seed):
    return scenes.synthetic_targets(n, select_rule.synthetic_ts(n, scenes.N_FRAMES, seed), seed)


def _loss_module(topk, thickness, dtype=torch.float32):
    loss_fn = NeRFWLoss(lambda_geo=0.04, thickness=thickness, topk=topk)
    Ks, Ps, max_t = scenes.camera_buffers()
    loss_fn.register_buffer("Ks", Ks.to(dtype)); loss_fn.register_buffer("Ps", Ps.to(dtype)); loss_fn.max_t = max_t
    return loss_fn.to(_dev())


def _evaluate(render, targets, topk, thickness, weights, upstream, dtype=torch.float32):
    """terms {name: float} and gradients {key: fp64 numpy} of sum_k upstream[k] * term_k"""
    loss_fn = _loss_module(topk, thickness, dtype)
    leaves = select_rule.leaves_of(render, _dev(), dtype)
    tg = {k: (v.to(_dev(), dtype) if v.is_floating_point() else v.to(_dev())) for k, v in targets.items()}
    kw = dict(output_transient_flow=FLOW, epoch=3)
    if weights is not None:
        kw["weights"] = weights.to(_dev(), dtype)
    terms = loss_fn(leaves, tg, **kw)
    sum(upstream[k] * v for k, v in terms.items()).backward()
    torch.cuda.synchronize()
    return terms, {k: float(v.detach()) for k, v in terms.items()}, \
        {k: v.grad.detach().double().cpu().numpy() for k, v in leaves.items() if v.grad is not None}


def _upstream(seed=11):
    g = torch.Generator().manual_seed(seed)
    return {k: float(torch.rand(1, generator=g)) + 0.5 for k in fused_loss.TERMS}, g


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("n_rays", [4097, 8192, 65536])
def test_batches_above_4096_rays_take_the_radix_select_kernels(n_rays, monkeypatch):
    """Fails without nsff_nerfw_loss_ex: applicable() refused more than 4096 rays and the torch expression ran, silently."""
    monkeypatch.delenv("NSFF_FUSED_LOSS", raising=False)
    monkeypatch.delenv("NSFF_LOSS_SELECT", raising=False)
    s = 64 if n_rays > 8192 else 16
    loss_fn = _loss_module(1.0, 1)
    leaves = select_rule.leaves_of(_render(n_rays, s, 1), _dev())
    tg = {k: v.to(_dev()) for k, v in _targets(n_rays, 1).items()}
    assert fused_loss.applicable(loss_fn, leaves, tg, dict(output_transient_flow=FLOW, epoch=3)) is True
    terms = loss_fn(leaves, tg, output_transient_flow=FLOW, epoch=3)
    assert isinstance(terms, fused_loss.LossTerms) and sorted(terms) == sorted(fused_loss.TERMS)
    assert _lib.last_loss_path() == 2
    terms.total().backward()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in terms.values())
    # ... and NSFF_LOSS_SELECT=rank is the behaviour before: not applicable above 4096 rays
    monkeypatch.setenv("NSFF_LOSS_SELECT", "rank")
    assert fused_loss.applicable(loss_fn, leaves, tg, dict(output_transient_flow=FLOW, epoch=3)) is False


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("coarse", [True, False])
@pytest.mark.parametrize("topk,thickness,weighted", [(1.0, 1, False), (0.3, 1, False), (0.7, 5, True)])
@pytest.mark.parametrize("n_rays", [4097, 8192, 65536])
def test_radix_select_loss_equals_the_torch_expression(n_rays, topk, thickness, weighted, coarse, monkeypatch):
    """Terms (2e-5 relative) and gradients w.r.t. every consumed leaf (max-norm 2e-4) against NSFF_FUSED_LOSS=0 -- the torch
    expression on the same leaves, which is what ran above 4096 rays before.  Where the fp32 torch expression is itself further
    than the bound from its own float64 evaluation (long fp32 sums), the kernels are held to the SAME bound against float64
    instead: they sum the selected values in float64 partials."""
    monkeypatch.delenv("NSFF_LOSS_SELECT", raising=False)
    render, targets = _render(n_rays, 64, 2, coarse), _targets(n_rays, 2)
    upstream, g = _upstream()
    weights = (torch.rand(n_rays, generator=g) + 0.25) if weighted else None
    monkeypatch.setenv("NSFF_FUSED_LOSS", "1")
    obj, t1, g1 = _evaluate(render, targets, topk, thickness, weights, upstream)
    assert isinstance(obj, fused_loss.LossTerms) and _lib.last_loss_path() == 2
    monkeypatch.setenv("NSFF_FUSED_LOSS", "0")
    obj, t0, g0 = _evaluate(render, targets, topk, thickness, weights, upstream)
    assert not isinstance(obj, fused_loss.LossTerms)
    assert sorted(t1) == sorted(t0) == sorted(fused_loss.TERMS) and sorted(g1) == sorted(g0)
    ref64 = []

    def float64():
        if not ref64:
            ref64.append(_evaluate(render, targets, topk, thickness, weights, upstream, torch.float64)[1:])
        return ref64[0]

    def rel(a, b):
        return abs(a - b) / max(abs(b), 1e-6)
    for k in t0:
        d = rel(t1[k], t0[k])
        print(f"{k}: fused {t1[k]:.9g} torch {t0[k]:.9g} rel {d:.2e}")
        if d > TERM_RTOL:
            t64 = float64()[0]
            assert rel(t0[k], t64[k]) > TERM_RTOL, (k, t1[k], t0[k], t64[k])          # the fp32 torch expression is what is off
            assert rel(t1[k], t64[k]) <= TERM_RTOL, (k, t1[k], t0[k], t64[k])
    for k in g0:
        d = parity.max_rel_err(g1[k], g0[k])
        print(f"d/d {k}: max-norm rel {d:.2e}")
        assert np.isfinite(g1[k]).all(), k
        if d > GRAD_RTOL:
            g64 = float64()[1]
            assert parity.max_rel_err(g0[k], g64[k]) > GRAD_RTOL, (k, d)
            parity.assert_close("d loss / d " + k + " (against float64)", g1[k], g64[k], GRAD_RTOL)


# ---------------------------------------------------------------- direct calls of the entry points
def _direct(render, targets, topk=1.0, weights=None, radix=True, thickness=1, backward=False):
    """mode 1 (and 2) of nsff_nerfw_loss / nsff_nerfw_loss_ex on device copies of a render dict; returns numpy arrays"""
    dev = _dev()
    n, s = render["xyzs_fine"].shape[:2]
    Ks, Ps, max_t = scenes.camera_buffers()
    args = {arg: render[key].to(dev).contiguous() for key, arg, _ in fused_loss._INPUTS if key in render}
    tg = dict(rgbs=targets["rgbs"], disps=targets["disps"], uv_fw=targets["uv_fw"], uv_bw=targets["uv_bw"], Ks=Ks.reshape(-1, 3, 3), Ps=Ps)
    tg = {k: v.float().contiguous().to(dev) for k, v in tg.items()}
    tg.update(ts=targets["ts"].long().to(dev), cam_ids=targets["cam_ids"].long().to(dev))
    hyper = torch.tensor([0.04, 0.04, 0.3 * 1e-3 / 5, 0.1, 1e-3], device=dev)
    out = dict(stats=torch.empty(24, device=dev), terms=torch.empty(11, device=dev), per_ray=torch.empty(11, n, device=dev),
               coef=torch.empty(11, n, device=dev))
    work = torch.empty(_lib.nerfw_loss_work_bytes(n), dtype=torch.uint8, device=dev).fill_(0xA5) if radix else None
    common_ = dict(hyper=hyper, weights=None if weights is None else weights.float().to(dev), topk=topk, thickness=thickness, work=work)
    dims = (n, s, int(s * 0.95), int(Ps.shape[1]), max_t)
    _lib.nerfw_loss(1, *dims, **args, **tg, **out, **common_)
    assert _lib.last_loss_path() == (2 if radix else 1)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if backward:
        grads = {garg: torch.empty_like(args[arg]) for _, arg, garg in fused_loss._INPUTS if garg is not None and arg in args}
        term_w = torch.linspace(0.5, 1.5, 11, device=dev)
        _lib.nerfw_loss(2, *dims, **args, **tg, **{k: v for k, v in out.items() if k != "terms"}, term_w=term_w, **grads, **common_)
        res.update({k: v.cpu().numpy() for k, v in grads.items()})
    torch.cuda.synchronize()
    return res


def _check_against_the_rule(res, render, targets, topk, weights=None):
    """coef != 0, K, the terms and the medians of one direct call against select_rule on that call's own per-ray values"""
    stats = res["stats"]
    vectors = [render["depth_fine"].numpy(), render["depth_coarse"].numpy() if "depth_coarse" in render else None, -targets["disps"].numpy()]
    for v, x in enumerate(vectors):
        if x is None:
            continue
        val, idx = select_rule.median(x)
        assert int(stats[select_rule.ST_IDX + v:select_rule.ST_IDX + v + 1].view(np.int32)[0]) == idx, (v, idx)
        assert stats[select_rule.ST_MED + v] == val
    w = None if weights is None else weights.numpy()
    for k, name in enumerate(select_rule.TERMS):
        if not np.isfinite(res["per_ray"][k]).all():      # (NaN has no order: see test_radix_select_equals_rank_counting_bit_for_bit)
            assert name == "disp_l" and float(render["depth_fine"].std()) == 0
            continue
        coef, term = select_rule.reduce_term(res["per_ray"][k], topk, w, masked=k in select_rule.MASKED)
        assert np.array_equal(res["coef"][k] != 0, coef != 0), (name, int((res["coef"][k] != 0).sum()), int((coef != 0).sum()))
        assert np.allclose(res["coef"][k], coef, rtol=1e-6, atol=0), name
        assert abs(float(res["terms"][k]) - term) <= 2e-6 * max(abs(term), 1e-12), (name, float(res["terms"][k]), term)


def _tied(render, targets, n, seed):
    """depth_fine constant, disps on an 8-bit grid, 60 % of the rays exact copies of ONE ray (every per-ray term then has a run of
    equal values that covers the cut K = M / 2 wherever that ray is in the term's population), scattered over the whole batch"""
    g = torch.Generator().manual_seed(seed)
    src = int(torch.nonzero((targets["ts"] > 0) & (targets["ts"] < scenes.N_FRAMES - 1))[0])
    copies = torch.randperm(n, generator=g)[:int(0.6 * n)]
    render = {k: v.clone() for k, v in render.items()}
    targets = {k: v.clone() for k, v in targets.items()}
    targets["disps"] = torch.round(targets["disps"] * 100) / 128          # <= 256 distinct values
    for d in (render, targets):
        for k in d:
            d[k][copies] = d[k][src].clone()
    render["depth_fine"] = torch.full((n,), 0.75)
    return render, targets


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("n_rays", [333, 1024, 4096])
def test_radix_select_equals_rank_counting_bit_for_bit(n_rays, tied):
    """Where both paths run: coef and the medians (value and index) bit-identical, terms within 1e-6 (the rank-counting path adds
    its workgroups' sums with float atomics).  On tied data the truth is the numpy rule; both paths must equal it exactly.
    A constant depth_fine ties the median completely (checked: ST_IDX of both paths is the rule's) and has a zero mean absolute
    deviation, so disp_l's per-ray values are NaN in every implementation, the torch expression included; NaN has no order, so
    that one term's selection is left out of the tied comparison -- ten terms carry the duplicated-row ties."""
    render, targets = _render(n_rays, 16, 3), _targets(n_rays, 3)
    cases = [(0.5, None)]
    if tied:
        render, targets = _tied(render, targets, n_rays, 3)
        assert len(np.unique(targets["disps"].numpy())) <= 256
    else:
        g = torch.Generator().manual_seed(5)
        cases += [(1.0, None), (0.3, torch.rand(n_rays, generator=g) + 0.25)]
    for topk, weights in cases:
        rank = _direct(render, targets, topk, weights, radix=False)
        radix = _direct(render, targets, topk, weights, radix=True)
        for res in (rank, radix):
            _check_against_the_rule(res, render, targets, topk, weights)
        rows = [k for k in range(11) if not (tied and k == 1)]
        assert np.array_equal(rank["coef"][rows].view(np.int32), radix["coef"][rows].view(np.int32))
        for lo in (select_rule.ST_MED, select_rule.ST_IDX):
            assert np.array_equal(rank["stats"][lo:lo + 3].view(np.int32), radix["stats"][lo:lo + 3].view(np.int32))
        assert np.allclose(radix["terms"][rows], rank["terms"][rows], rtol=1e-6, atol=0), (radix["terms"], rank["terms"])
        if tied:        # the run of equal values really straddles the cut
            k = 0
            v = rank["per_ray"][k]
            cut = np.sort(v)[::-1][int(0.5 * n_rays) - 1]
            assert (v == cut).sum() >= 0.3 * n_rays and 0 < ((v == cut) & (rank["coef"][k] != 0)).sum() < (v == cut).sum()


# ---------------------------------------------------------------- 4
@pytest.mark.parametrize("n_rays,s", [(4097, 8), (5000, 8), (_lib.LOSS_MAX_RAYS, 2)])
def test_radix_select_edge_populations(n_rays, s):
    """Flow populations of 0, 1 and all rays, K = 0; the first size of the new path, a size that is no multiple of 256, the bound."""
    free = torch.cuda.mem_get_info()[0]
    if free < 64 * n_rays * s * 4 + (2 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free")
    render, base = _render(n_rays, s, 4), _targets(n_rays, 4)
    max_t = scenes.N_FRAMES - 1
    last = torch.full((n_rays,), max_t)
    one = last.clone(); one[n_rays // 2] = 7
    for ts, topk, m_fw in ((last, 0.5, 0), (last, 1.0, 0), (one, 0.5, None), (one, 1.0, None),
                           (torch.full((n_rays,), 7), 0.5, None), (torch.full((n_rays,), 7), 1.0, None), (base["ts"], 1e-7, None)):
        targets = dict(base, ts=ts)
        res = _direct(render, targets, topk, radix=True, backward=n_rays <= 5000)
        _check_against_the_rule(res, render, targets, topk)
        pop_fw = int((res["per_ray"][4] >= 0).sum())
        if m_fw is not None:
            assert pop_fw == m_fw and res["terms"][4] == 0 and not res["coef"][4].any()
        if ts is one:
            assert pop_fw <= 1
            if pop_fw == 1 and topk >= 1:
                assert res["coef"][4][n_rays // 2] == 1.0 and res["terms"][4] == res["per_ray"][4][n_rays // 2]
        if topk == 1e-7:
            assert not res["coef"].any() and not res["terms"].any()          # K = int(topk * M) = 0 for every term
        assert all(np.isfinite(v).all() for v in res.values())


# ---------------------------------------------------------------- 5
def test_radix_select_loss_is_capturable():
    """mode 1 + mode 2 at 8192 rays in one captured graph, replayed twice with the leaves changed in place between the replays"""
    dev, n, s = _dev(), 8192, 16
    Ks, Ps, max_t = scenes.camera_buffers()
    renders = [select_rule.synthetic_render(n, s, 20 + i) for i in range(2)]
    targets = _targets(n, 6)
    topk = 0.5
    args = {arg: renders[0][key].to(dev).contiguous() for key, arg, _ in fused_loss._INPUTS}
    tg = {k: targets[k].float().to(dev) for k in ("rgbs", "disps", "uv_fw", "uv_bw")}
    tg.update(ts=targets["ts"].to(dev), cam_ids=targets["cam_ids"].to(dev), Ks=Ks.reshape(-1, 3, 3).contiguous().to(dev), Ps=Ps.contiguous().to(dev))
    out = dict(stats=torch.empty(24, device=dev), per_ray=torch.empty(11, n, device=dev), coef=torch.empty(11, n, device=dev))
    terms = torch.empty(11, device=dev)
    grads = {garg: torch.empty_like(args[arg]) for _, arg, garg in fused_loss._INPUTS if garg is not None}
    common_ = dict(hyper=torch.tensor([0.04, 0.04, 6e-5, 0.1, 1e-3], device=dev), topk=topk,
                   work=torch.empty(_lib.nerfw_loss_work_bytes(n), dtype=torch.uint8, device=dev))
    term_w = torch.linspace(0.5, 1.5, 11, device=dev)
    dims = (n, s, int(s * 0.95), int(Ps.shape[1]), max_t)

    def both():
        _lib.nerfw_loss(1, *dims, **args, **tg, **out, terms=terms, **common_)
        _lib.nerfw_loss(2, *dims, **args, **tg, **out, term_w=term_w, **grads, **common_)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for render in (renders[1], renders[0]):
        for key, arg, _ in fused_loss._INPUTS:
            args[arg].copy_(render[key].to(dev).reshape(args[arg].shape))
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in dict(out, terms=terms, **grads).items()}
        common_["work"].fill_(0x5A)                                  # nothing of a call survives in the workspace
        both()
        torch.cuda.synchronize()
        assert torch.equal(got["stats"][:9], out["stats"][:9]), (got["stats"], out["stats"])
        assert torch.equal(got["coef"], out["coef"]), ((got["coef"] != 0).sum(1), (out["coef"] != 0).sum(1), got["terms"], terms)
        assert torch.allclose(got["terms"], terms, rtol=1e-6, atol=0)
        for k in grads:
            assert torch.allclose(got[k], grads[k], rtol=1e-5, atol=1e-12), k
        _check_against_the_rule({k: v.cpu().numpy() for k, v in dict(out, terms=terms).items()}, render, targets, topk)


# ---------------------------------------------------------------- 6
def test_trainer_step_at_8192_rays_with_topk_and_ray_weights(monkeypatch):
    """One eager NSFFTrainer.step of the C2 training configuration at 8192 rays with topk = 0.5 and per-ray weights -- a
    combination static_shapes cannot express -- on the kernels and on the torch expression."""
    from nsff_pl_amd.training import NSFFTrainer
    free = torch.cuda.mem_get_info()[0]
    if free < 48 << 30:
        pytest.skip(f"{free >> 30} GiB of device memory free")
    monkeypatch.delenv("NSFF_LOSS_SELECT", raising=False)
    n = 8192
    cfg = dict(scenes.C2_TRAIN_CASE, n_rays=n)
    Ks, Ps, _ = scenes.camera_buffers()
    hp = dict(N_samples=cfg["N_samples"], N_importance=cfg["N_importance"], perturb=0, noise_std=0, topk=0.5)
    rays, ts = scenes.synthetic_rays(n, cfg["seed"])
    batch = {k: v.to(_dev()) for k, v in scenes.synthetic_targets(n, ts, cfg["seed"]).items()}
    batch["rays"] = rays.to(_dev())
    batch["weights"] = (torch.rand(n, generator=torch.Generator().manual_seed(8)) + 0.25).to(_dev())
    runs = {}
    A.set_precision("f16x3")
    try:
        for fused in ("1", "0"):
            monkeypatch.setenv("NSFF_FUSED_LOSS", fused)
            models, emb = scenes.build_scene(A.NeRF, A.PosEmbedding, cfg)
            tr = NSFFTrainer(models, emb, scenes.N_FRAMES, hp, Ks, Ps, output_transient_flow=cfg["flow"]).to(_dev())
            tr.on_train_epoch_start(scenes.LOSS_EPOCH)
            log = tr.step(batch)
            torch.cuda.synchronize()
            if fused == "1":
                assert _lib.last_loss_path() == 2
            runs[fused] = ({k: float(v) for k, v in log.items() if k.startswith("train/")}, tr._flat_grad.detach().double().cpu().numpy().copy())
            del tr, models, emb
    finally:
        A.set_precision(A.config.DEFAULT_PRECISION)
    (t1, g1), (t0, g0) = runs["1"], runs["0"]
    for k in fused_loss.TERMS:
        print(f"train/{k}: fused {t1['train/' + k]:.9g} torch {t0['train/' + k]:.9g}")
        assert abs(t1["train/" + k] - t0["train/" + k]) <= TERM_RTOL * max(abs(t0["train/" + k]), 1e-6), k
    l1 = np.abs(g1 - g0).sum() / np.abs(g0).sum()
    print(f"flat gradient: relative L1 distance {l1:.3e}")
    assert np.isfinite(g1).all() and l1 <= GRAD_RTOL


# ---------------------------------------------------------------- golden g22
@pytest.mark.parametrize("topk", [1.0, 0.5])
def test_radix_select_loss_matches_reference_statistics(topk, monkeypatch):
    """golden g22 (tests/golden/make_golden_loss_large.py): the REFERENCE's NeRFWLoss on the seeded synthetic render dict at
    8192 rays x 32 samples -- its eleven terms and, per consumed tensor, (sum g, sum |g|, <g, r>) in fp32 and fp64.  g20's bounds:
    terms 1e-4, statistics 2e-3 sum |g|, each plus 3 x the reference's own fp32 - fp64 distance."""
    monkeypatch.setenv("NSFF_FUSED_LOSS", "1")
    monkeypatch.delenv("NSFF_LOSS_SELECT", raising=False)
    z = np.load(common.GOLDEN_DIR + "/g22_loss_large.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    tag = f"topk{topk:g}"
    t32, t64, s32, s64 = (json.loads(bytes(z[f"{name}_{tag}"]).decode()) for name in ("terms32", "terms64", "stats32", "stats64"))
    n, s, seed = meta["n_rays"], meta["n_samples"], meta["seed"]
    assert (n, s) == (8192, 32)
    obj, terms, grads = _evaluate(select_rule.synthetic_render(n, s, seed), _targets(n, seed), topk, 1, None,
                                  {k: 1.0 for k in fused_loss.TERMS})
    assert isinstance(obj, fused_loss.LossTerms) and _lib.last_loss_path() == 2
    assert sorted(terms) == sorted(t64)
    for k, v in t64.items():
        print(f"{k}: fused {terms[k]:.9g} reference fp64 {v:.9g} fp32 {t32[k]:.9g}")
        assert abs(terms[k] - v) <= 1e-4 * max(abs(v), 1e-6) + 3 * abs(t32[k] - v), (k, terms[k], v, t32[k])
    stats = select_rule.grad_statistics({k: torch.from_numpy(v) for k, v in grads.items()})
    assert sorted(stats) == sorted(s64)
    scale = max(abs(v[1]) for v in s64.values())
    for k, want in s64.items():
        mag = max(want[1], 1e-6 * scale)
        for i in range(3):
            tol = 2e-3 * mag + 3 * abs(s32[k][i] - want[i])
            assert abs(stats[k][i] - want[i]) <= tol, (k, i, stats[k], want, s32[k], tol)
