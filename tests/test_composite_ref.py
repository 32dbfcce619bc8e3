"""CPU tests of tests/composite_ref.py: the float64 expression the compositing kernels are held to IS the project's compositing
(it agrees with tests/torch_path.py::render_pass, values and gradients, through a field stub that hands out the case's raw
records -- the goldens hold softplus'd sigmas and no re-query records, so they cannot feed it), the planted cells are where the
case generator says, the yardstick d32 is finite and small, and the comparison rule notices six planted defects on every case
that has the route each one breaks."""
import pytest
import torch

import composite_ref as R
import torch_path


def _render_pass(case, dtype=torch.float64):
    """torch_path.render_pass on the case: rays (o, d) with xyz = o + d z, the field replaced by the case's records"""
    c = case
    n, S = c.n, c.S
    rays = torch.randn(n, 6, generator=torch.Generator().manual_seed(5), dtype=dtype)
    zs = c.zs.to(dtype)
    raws = [t.to(dtype).reshape(n * S, 16).requires_grad_(True) for t in (c.raw, c.raw_fw, c.raw_bw)]
    calls = []

    def field_fn(model, xyz, freqs, t_rows, s, static, transient, dir_e, a_e):
        calls.append((static, transient))
        return raws[len(calls) - 1]
    noise = {}
    if c.noise_given:
        noise = dict(static=c.noise["static"].to(dtype), transient=c.noise["transient"].to(dtype),
                     warp_fw=c.noise["fw"].to(dtype), warp_bw=c.noise["bw"].to(dtype))
    results = {}
    torch_path.render_pass(results, None, "fine", [1.0], rays, zs, None, None, None, None, None, bool(c.has_transient),
                           ["fw", "bw"] if c.flow_mode >= 1 else [], c.noise_std, noise, c.flow_mode == 1, field_fn)
    assert calls == [(True, bool(c.has_transient))] + ([(False, True)] * 2 if c.flow_mode == 2 else [])
    names = {"static_sigmas": "static_sigmas_fine", "transient_sigmas": "transient_sigmas_fine", "static_weights": "static_weights_fine",
             "transient_weights": "transient_weights_fine", "weights": "weights_fine", "depth": "depth_fine", "rgb": "rgb_fine",
             "transient_alpha": "transient_alpha_fine", "transient_rgb": "transient_rgb_fine", "so_rgb": "_static_rgb_fine",
             "so_depth": "_static_depth_fine", "xyz_exp": "xyz_fine", "flow_fw_exp": "transient_flow_fw",
             "flow_bw_exp": "transient_flow_bw", "rgb_fw": "rgb_fw", "rgb_bw": "rgb_bw"}
    if not c.has_transient:
        names["weights"] = "static_weights_fine"                 # one tensor under both names (rendering.py:248)
    return results, names, raws, rays


@pytest.mark.parametrize("form", R.FORM_NAMES)
def test_the_float64_expression_is_the_project_s_compositing(form):
    """values and gradients agree with render_pass in float64 (its own exclusive-product backward, its far mask, its warps) to
    1e-11 of each tensor's largest value on every S of the sweep from 2 up (render_pass builds its last-sample deltas from a
    column of the others, so it has no S = 1), plants included"""
    worst = 0.0
    for S in R.S_BOTH[1:] + R.S_FORWARD_ONLY:
        for mode in R.NOISE_MODES:
            c = R.make_case(R.N_SWEEP, S, form, mode)
            results, names, raws, rays = _render_pass(c)
            xyz = rays[:, None, 0:3] + rays[:, None, 3:6] * c.zs.double()[..., None]
            leaf = lambda t: t.double().requires_grad_(True)
            ins = [leaf(t) for t in (c.raw, c.raw_fw, c.raw_bw, c.f_fw, c.f_bw)]
            noise = {k: (v.double() if c.noise_given else None) for k, v in c.noise.items()}
            out = R.composite(ins[0], ins[1], ins[2], c.zs.double(), xyz, ins[3], ins[4], noise, c.noise_std, c.has_transient,
                              c.flow_mode)
            close = lambda a, b: float(((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).detach())
            for k in c.names:
                worst = max(worst, close(out[k], results[names[k]].reshape(out[k].shape)))
            want = torch.autograd.grad(sum((results[names[k]].reshape(out[k].shape) * c.cot[k].double()).sum() for k in c.names),
                                       raws, allow_unused=True)
            got = torch.autograd.grad(sum((out[k] * c.cot[k].double()).sum() for k in c.names), ins, allow_unused=True)
            zero = lambda g, like: torch.zeros_like(like) if g is None else g
            d_raw, d_fw, d_bw = [zero(g, r).view(c.n, S, 16) for g, r in zip(want, raws)]
            worst = max(worst, close(zero(got[0], ins[0])[..., :8], d_raw[..., :8]))
            if c.flow_mode >= 1:                                 # render_pass reads the flows out of the record and masks them
                near = (c.zs <= R.Z_FAR)[..., None].double()
                assert float((d_raw[..., 8:14] * (1 - near)).abs().max()) == 0
                worst = max(worst, close(got[3] * near, d_raw[..., 8:11]), close(got[4] * near, d_raw[..., 11:14]))
            if c.flow_mode >= 2:
                worst = max(worst, close(got[1][..., 4:8], d_fw[..., 4:8]), close(got[2][..., 4:8], d_bw[..., 4:8]))
    assert worst < 1e-11, worst


def test_the_planted_cells_are_there():
    seen = set()
    one = torch.ones((), dtype=torch.float32)
    for key in R.forward_keys():
        c = R.make_case(*key)
        d = torch.cat([c.zs[:, 1:] - c.zs[:, :-1], torch.full((c.n, 1), 100.0)], 1)
        d_t = torch.cat([d[:, :-1], torch.full((c.n, 1), 1e-3)], 1)
        assert (d >= 0).all() and c.zs.dtype == torch.float32 and c.raw.dtype == torch.float32
        nz = lambda k: (c.noise[k] * c.noise_std) if c.noise_given else 0.0
        al_s = one - torch.exp(-d * torch.nn.functional.softplus(c.raw[..., 3] + nz("static")))
        al_t = one - torch.exp(-d_t * torch.nn.functional.softplus(c.raw[..., 7] + nz("transient")))
        assert sum(kind == "empty" for items in c.planted.values() for kind, _ in items) <= 1
        assert (c.empty_ray is not None) == (c.n > R.EMPTY_RAY)
        for r, items in c.planted.items():
            for kind, at in items:
                seen.add((kind, "last-but-one" if kind == "static_4000" and at == c.S - 2 else at))
                if kind == "static_4000":
                    assert c.raw[r, at, 3] == 4000 and one - al_s[r, at] == 0, (key, r, at)
                elif kind == "transient_40000":
                    assert c.raw[r, at, 7] == 40000 and one - al_t[r, at] == 0, (key, r, at)
                elif kind == "linear_branch":
                    assert c.raw[r, at, 3] == 25 and c.raw[r, at, 7] == 30 and c.raw_fw[r, at, 7] == 25 and c.raw_bw[r, at, 7] == 30
                    assert c.noise_std == 0 or not c.noise_given or (c.raw[r, at, 3] + c.noise["static"][r, at] > 20)
                elif kind == "equal_depths":
                    assert c.zs[r, at + 1] == c.zs[r, at]
                elif kind == "empty":
                    assert r == c.empty_ray == R.EMPTY_RAY
                    assert all((rec[r, :, 3] == -30).all() and (rec[r, :, 7] == -30).all() for rec in (c.raw, c.raw_fw, c.raw_bw))
        tail = [r for r in range(c.n) if r % 4 != 2]
        assert (c.zs[tail, -1] > R.Z_FAR).all() and (c.f_fw[c.zs > R.Z_FAR] == 0).all() and (c.f_bw[c.zs > R.Z_FAR] == 0).all()
        assert c.S == 1 or (c.zs[:, 0] < R.Z_FAR).all()
    for need in (("static_4000", 63), ("static_4000", 64), ("static_4000", 0), ("static_4000", "last-but-one"),
                 ("transient_40000", 64), ("equal_depths", 63), ("empty", None)):
        assert need in seen, need
    assert any(k == "linear_branch" for k, _ in seen)


def test_the_sweep_is_the_issue_s():
    keys = R.backward_keys()
    assert len(keys) == len(set(keys)) == 4 * (9 * 3 + 2 * 3)
    assert {k[1] for k in keys} == {1, 2, 63, 64, 65, 128, 129, 192, 200} and {k[0] for k in keys} == {1, 5, 9}
    assert {k[1] for k in R.forward_keys()} - {k[1] for k in keys} == {257, 260}


def test_the_yardstick_is_finite_and_small():
    """d32 < 1e-3 on every case, group and output: 8 x d32 stays far below a wrong gradient"""
    worst = {}
    for key in R.forward_keys():
        ref = R.reference(key)
        figures = dict(ref.d32_out)
        if key in set(R.backward_keys()):
            figures.update(ref.d32_grads)
        for name, v in figures.items():
            assert v == v and v < 1e-3, (key, name, v)
            worst[key[2]] = max(worst.get(key[2], 0.0), v)
    print("worst d32 per form:", {k: f"{v:.3g}" for k, v in worst.items()})


# defect -> (the cases that have the route it breaks, the gradient group that must leave its bound)
DEFECT_ROUTES = {
    "carry": (lambda c: c.S >= 65, ("d_raw", "static_sigma")),                       # a second chunk
    "last_delta": (lambda c: True, ("d_raw", "static_sigma")),                       # every case has a ray lit to its last sample
    "background": (lambda c: c.has_transient, ("d_raw", "transient_sigma")),         # g_transient_rgb reaches the transient weights
    "so_blend": (lambda c: c.has_transient and c.S >= 2, ("d_raw", "static_sigma")),   # a static-only chain of more than one factor
    "fbw_weight": (lambda c: c.flow_mode >= 1, ("d_f_bw", "flow")),                  # the flow expectations
    "suffix_stop": (lambda c: c.S >= 2, ("d_raw", "static_sigma")),                  # a sample in front of the last one
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_the_rule_notices_a_planted_defect(defect):
    """the defective float64 expression against the SOUND float32 evaluation: outside the bound on every case with the route"""
    route, (t, group) = DEFECT_ROUTES[defect]
    sl = dict(R.GROUPS[t])[group]
    n_cases, least = 0, float("inf")
    for key in R.backward_keys():
        ref = R.reference(key)
        c = ref.case
        if not route(c):
            continue
        _, g = R.evaluate(c, torch.float64, defect=defect)
        ratio = float(R.ray_errors(ref.grads32[t][..., sl], g[t][..., sl], c.empty_ray).max()) / R.bound(ref.d32_grads[(t, group)])
        assert ratio > 1, (defect, key, ratio)
        n_cases, least = n_cases + 1, min(least, ratio)
    assert n_cases >= 30
    print(f"{defect}: {n_cases} cases, least error / bound {least:.3g}")


def test_the_sound_evaluations_pass_their_own_rule():
    """(the other half of the previous test: float32 against float64 is inside the bound by construction, and a non-finite or
    non-zero value where the reference is identically zero is an infinite error)"""
    ref = R.reference((5, 65, "transient_warp", "given"))
    assert all(e <= b for e, b, _ in R.gradient_errors(ref, ref.grads32).values())
    assert all(e <= b for e, b, _ in R.output_errors(ref, ref.out32).values())
    bad = {k: v.clone() for k, v in ref.grads32.items()}
    bad["d_raw"][4, 64, 3] = float("nan")
    assert R.gradient_errors(ref, bad)[("d_raw", "static_sigma")][0] == float("inf")
    want = torch.zeros(2, 3, 1, dtype=torch.float64)
    assert R.ray_errors(torch.zeros(2, 3, 1), want, None).tolist() == [0.0, 0.0]
    assert R.ray_errors(torch.full((2, 3, 1), 1e-30), want, None).tolist() == [float("inf")] * 2
