"""TEST INFRASTRUCTURE: the sigma->alpha compositing of one render pass as a plain torch expression of the inputs of
``nsff_composite`` / ``nsff_composite_backward`` (csrc/rays.hip, csrc/rays_bwd.hip), the cases the two kernels are held to
and the comparison rule.

The expression is the mathematics of tests/torch_path.py::render_pass (reference models/rendering.py:122-140,200-298) with the
field taken out: the raw records, the depths, the points and the already far-masked per-sample flows come in, every output that
``NsffCompositeBwdArgs`` has a ``g_*`` for goes out.  Evaluated with autograd in float64 it is the reference; evaluated in
float32 on the CPU it measures what fp32 arithmetic costs this expression -- the yardstick ``d32`` of the rule below.  The
transmittances are ``torch.cumprod``, whose CPU backward is exact where a factor is zero.

The rule (``errors`` / ``bound``).  Every gradient tensor and column group is judged on its own.  The error of a ray is the
largest ``|got - want64|`` of the group in that ray over the largest ``|want64|`` of the group in that ray; the ONE designated
empty ray of a case (raw sigmas -30 throughout: its fp32 gradients are 100 % off their 1e-13-sized float64 values) is divided
by the largest value of the group in the whole case instead.  The bound of a (case, group) is ``max(8 d32, 16 * 2^-24)`` with
``d32`` the same figure for the CPU float32 evaluation.  The forward outputs are judged the same way, per ray and output.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

Z_FAR = 0.95
FACTOR = 8.0
FLOOR = 16 * 2.0 ** -24

# form = (name, has_transient, flow_mode)
FORMS = (("static", 0, 0), ("transient", 1, 0), ("transient_flow", 1, 1), ("transient_warp", 1, 2))
FORM_NAMES = tuple(f[0] for f in FORMS)
NOISE_MODES = ("given", "null", "std0")        # noise_std 1 + arrays, noise_std 1 + NULL pointers, noise_std 0 + arrays
S_BOTH = (1, 2, 63, 64, 65, 128, 129, 192, 200)
S_FORWARD_ONLY = (257, 260)                    # the forward's serial form over five chunks
N_SWEEP = 5
N_EDGE = (1, 9)
S_EDGE = (1, 65, 200)
EMPTY_RAY = 3                                  # the designated empty ray (cases of more than three rays)
MIN_GAP = 0.006                                # depth step behind a planted saturated sample: 0.006 * (4000 - 5) > 17.4 = -log(2^-25)

INPUT_GRADS = ("raw", "raw_fw", "raw_bw", "f_fw", "f_bw")
GROUPS = {"d_raw": (("static_rgb", slice(0, 3)), ("static_sigma", slice(3, 4)), ("transient_rgb", slice(4, 7)),
                    ("transient_sigma", slice(7, 8))),
          "d_raw_fw": (("transient_rgb", slice(4, 7)), ("transient_sigma", slice(7, 8))),
          "d_raw_bw": (("transient_rgb", slice(4, 7)), ("transient_sigma", slice(7, 8))),
          "d_f_fw": (("flow", slice(0, 3)),), "d_f_bw": (("flow", slice(0, 3)),)}
DEFECTS = ("carry", "last_delta", "background", "so_blend", "fbw_weight", "suffix_stop")


def output_names(has_transient, flow_mode):
    """the outputs of a form, named like the g_* of NsffCompositeBwdArgs without the prefix"""
    if not has_transient:
        return ["static_sigmas", "static_weights", "weights", "depth", "rgb"]
    names = ["static_sigmas", "transient_sigmas", "static_weights", "transient_weights", "weights", "depth", "rgb",
             "transient_alpha", "transient_rgb", "so_rgb", "so_depth"]
    if flow_mode >= 1:
        names += ["xyz_exp", "flow_fw_exp", "flow_bw_exp"]
    if flow_mode >= 2:
        names += ["rgb_fw", "rgb_bw"]
    return names


def group_list(has_transient, flow_mode):
    """(tensor, group, columns) of every gradient a form produces"""
    out = [("d_raw", g, sl) for g, sl in GROUPS["d_raw"] if has_transient or g.startswith("static")]
    if flow_mode >= 1:
        out += [(t, g, sl) for t in ("d_f_fw", "d_f_bw") for g, sl in GROUPS[t]]
    if flow_mode >= 2:
        out += [(t, g, sl) for t in ("d_raw_fw", "d_raw_bw") for g, sl in GROUPS[t]]
    return out


def _excl_cumprod(om, restart_at=None):
    """T_i = prod_{j<i} om_j along dim 1.  restart_at (a planted defect): the product starts again at 1 at that sample."""
    one = torch.ones_like(om[:, :1])
    if restart_at is None or om.shape[1] <= restart_at:
        return torch.cat([one, torch.cumprod(om, 1)[:, :-1]], 1)
    return torch.cat([_excl_cumprod(om[:, :restart_at]), _excl_cumprod(om[:, restart_at:])], 1)


def composite(raw, raw_fw, raw_bw, zs, xyz, f_fw, f_bw, noise, noise_std, has_transient, flow_mode, defect=None):
    """One pass.  raw* (n, S, 16), zs (n, S), xyz / f_fw / f_bw (n, S, 3) with the flows already zeroed beyond z = 0.95,
    noise: dict static / transient / fw / bw -> (n, S) or None.  Any dtype; returns a dict (see output_names).
    defect: one of DEFECTS, planted to show that the comparison rule notices it (never used for a reference)."""
    assert defect is None or defect in DEFECTS
    nz = lambda k: 0.0 if noise.get(k) is None else noise[k] * noise_std
    deltas = zs[:, 1:] - zs[:, :-1]
    d_trans = torch.cat([deltas, torch.full_like(zs[:, :1], 1e-3)], 1)
    d_static = d_trans if defect == "last_delta" else torch.cat([deltas, torch.full_like(zs[:, :1], 100.0)], 1)
    restart = 64 if defect == "carry" else None

    def blend_T(om):
        T = _excl_cumprod(om, restart)
        if defect == "suffix_stop" and T.shape[1] >= 2:           # the last sample's transmittance sends nothing back
            T = torch.cat([T[:, :-1], T[:, -1:].detach()], 1)
        return T

    out = {}
    s_rgb = raw[..., 0:3]
    s_sig = out["static_sigmas"] = F.softplus(raw[..., 3] + nz("static"))
    s_alpha = 1 - torch.exp(-d_static * s_sig)
    if not has_transient:
        w = s_alpha * blend_T(1 - s_alpha)
        out["static_weights"] = w
        out["weights"] = w
        out["depth"] = (w * zs).sum(1)
        out["rgb"] = (w[..., None] * s_rgb).sum(1)
        return out
    t_rgb = raw[..., 4:7]
    t_sig = out["transient_sigmas"] = F.softplus(raw[..., 7] + nz("transient"))
    t_alpha = 1 - torch.exp(-d_trans * t_sig)
    alphas = 1 - (1 - s_alpha) * (1 - t_alpha)
    T = blend_T(1 - alphas)
    w = out["weights"] = alphas * T
    s_w = out["static_weights"] = s_alpha * T
    t_w = out["transient_weights"] = t_alpha * T
    out["depth"] = (w * zs).sum(1)
    t_map = (t_w[..., None] * t_rgb).sum(1)
    out["rgb"] = (s_w[..., None] * s_rgb).sum(1) + t_map
    ta = out["transient_alpha"] = t_w.sum(1)
    out["transient_rgb"] = t_map if defect == "background" else t_map + 0.8 * (1 - ta[:, None])
    so_w = s_alpha * _excl_cumprod(1 - (alphas if defect == "so_blend" else s_alpha))
    out["so_rgb"] = (so_w[..., None] * s_rgb).sum(1)
    out["so_depth"] = (so_w * zs).sum(1)
    if flow_mode >= 1:
        w3 = w[..., None]
        out["xyz_exp"] = (w3 * xyz).sum(1)
        out["flow_fw_exp"] = (w3 * f_fw).sum(1)
        out["flow_bw_exp"] = ((t_w[..., None] if defect == "fbw_weight" else w3) * f_bw).sum(1)
    if flow_mode >= 2:
        for key, rec, nk in (("rgb_fw", raw_fw, "fw"), ("rgb_bw", raw_bw, "bw")):
            al_w = 1 - torch.exp(-d_trans * F.softplus(rec[..., 7] + nz(nk)))
            Tw = _excl_cumprod(1 - (1 - (1 - s_alpha) * (1 - al_w)))
            out[key] = ((s_alpha * Tw)[..., None] * s_rgb).sum(1) + ((al_w * Tw)[..., None] * rec[..., 4:7]).sum(1)
    return out


# ---- the cases ----
def plants(n, S, ray):
    """what is planted into `ray` of an (n, S) case: list of (kind, sample)"""
    slot, out = ray, []
    if slot == 0 and S >= 64 and n > 1:                           # (a single ray keeps its last chunk lit)
        out.append(("static_4000", 63))
    if slot == 1 and S >= 65:
        out.append(("static_4000", 64))
    if slot == 2:                                                 # the blend goes dark at 64, the static-only and warped chains at S - 2
        if S >= 65:
            out.append(("transient_40000", 64))
        if S >= 2 and S != 65:                                    # (S = 65: sample 63 is ray 0's)
            out.append(("static_4000", S - 2))
    if slot == EMPTY_RAY and n > EMPTY_RAY:
        out.append(("empty", None))
    if slot == 4:                                                 # lit to its last sample
        out.append(("linear_branch", min(S // 3, 40)))            # raw sigma 25 (static, fw re-query) / 30 (transient, bw re-query)
        if S >= 4:
            out.append(("equal_depths", S // 2 - 1))              # zs[p + 1] == zs[p]
    if slot == 5:
        out.append(("static_4000", 0))
    if slot == 8 and S >= 65:                                     # the ray alone in the last workgroup: both fields saturate at 64
        out += [("static_4000", 64), ("transient_40000", 64)]
    return out


def _case_seed(n, S, form, noise_mode):
    return 7919 * S + 101 * n + 13 * FORM_NAMES.index(form) + NOISE_MODES.index(noise_mode)


@functools.lru_cache(maxsize=None)
def make_case(n, S, form, noise_mode):
    """Seeded float32 inputs and standard normal cotangents of one case (CPU tensors; both evaluations and the kernels
    share them)."""
    _, tr, fm = FORMS[FORM_NAMES.index(form)]
    g = torch.Generator().manual_seed(_case_seed(n, S, form, noise_mode))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    un = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g)

    def records():
        r = rn(n, S, 16)                                          # slots 14, 15 (and 0-3 of a re-query) are never read
        r[..., 0:3], r[..., 4:7] = un(0.05, 0.95, n, S, 3), un(0.05, 0.95, n, S, 3)
        r[..., 3], r[..., 7] = 1.0 + 2.0 * rn(n, S), 1.0 + 2.0 * rn(n, S)
        return r
    raw, raw_fw, raw_bw = records(), records(), records()
    flow = 0.1 * rn(n, S, 6)
    raw[..., 8:14] = flow                                         # the forward kernel masks these itself
    gaps = un(0.2, 1.8, n, S) * (0.9 / S)
    planted = {r: plants(n, S, r) for r in range(n)}
    empty_ray = None
    for r, items in planted.items():
        for kind, at in items:
            if kind == "static_4000":
                raw[r, at, 3] = 4000.0
                gaps[r, at] = max(float(gaps[r, at]), MIN_GAP)
            elif kind == "transient_40000":
                raw[r, at, 7] = 40000.0
                gaps[r, at] = max(float(gaps[r, at]), MIN_GAP)
            elif kind == "linear_branch":
                raw[r, at, 3], raw[r, at, 7], raw_fw[r, at, 7], raw_bw[r, at, 7] = 25.0, 30.0, 25.0, 30.0
            elif kind == "equal_depths":
                gaps[r, at] = 0.0
            elif kind == "empty":
                empty_ray = r
                for rec in (raw, raw_fw, raw_bw):
                    rec[r, :, 3] = rec[r, :, 7] = -30.0
    zs = 0.02 + torch.cumsum(torch.cat([torch.zeros(n, 1), gaps[:, :-1]], 1), 1)      # (a running sum: never decreasing)
    k = max(1, S // 10)                                           # depths above 0.95 at the tail (not on every fourth ray)
    for r in range(n):
        if r % 4 != 2:
            zs[r, S - k:] += max(0.0, 0.956 - float(zs[r, S - k]))
    far = (zs > Z_FAR)[..., None]
    f_fw = torch.where(far, torch.zeros(()), flow[..., 0:3]).contiguous()
    f_bw = torch.where(far, torch.zeros(()), flow[..., 3:6]).contiguous()
    noise = dict(static=rn(n, S), transient=rn(n, S), fw=rn(n, S), bw=rn(n, S))
    names = output_names(tr, fm)
    per_sample = ("static_sigmas", "transient_sigmas", "static_weights", "transient_weights", "weights")
    cot = {k_: rn(n, S) if k_ in per_sample else (rn(n) if k_ in ("depth", "transient_alpha", "so_depth") else rn(n, 3))
           for k_ in names}
    return SimpleNamespace(n=n, S=S, form=form, noise_mode=noise_mode, has_transient=tr, flow_mode=fm,
                           noise_std=0.0 if noise_mode == "std0" else 1.0, noise_given=noise_mode != "null",
                           raw=raw, raw_fw=raw_fw, raw_bw=raw_bw, zs=zs, xyz=0.5 * rn(n, S, 3), f_fw=f_fw, f_bw=f_bw,
                           noise=noise, cot=cot, names=names, planted=planted, empty_ray=empty_ray,
                           key=(n, S, form, noise_mode))


def backward_keys(form=None):
    """(n, S, form, noise mode) of the gradient sweep: every S with every form and noise mode at n = 5; n = 1 and 9 at S in
    {1, 65, 200} with the noise arrays given"""
    forms = FORM_NAMES if form is None else (form,)
    keys = [(N_SWEEP, S, f, m) for f in forms for S in S_BOTH for m in NOISE_MODES]
    keys += [(n, S, f, "given") for f in forms for n in N_EDGE for S in S_EDGE]
    return keys


def forward_keys(form=None):
    forms = FORM_NAMES if form is None else (form,)
    return backward_keys(form) + [(N_SWEEP, S, f, m) for f in forms for S in S_FORWARD_ONLY for m in NOISE_MODES]


# ---- the two evaluations ----
def evaluate(case, dtype, defect=None, grads=True):
    """(outputs, gradients) of the expression in `dtype`: gradients of sum_k <cot_k, out_k> w.r.t. raw, raw_fw, raw_bw, f_fw,
    f_bw as d_raw (n, S, 16), ..., d_f_bw (n, S, 3); those a form does not produce are absent."""
    c = case
    leaf = lambda t: t.to(dtype).requires_grad_(True)
    ins = dict(raw=leaf(c.raw), raw_fw=leaf(c.raw_fw), raw_bw=leaf(c.raw_bw), f_fw=leaf(c.f_fw), f_bw=leaf(c.f_bw))
    noise = {k: (v.to(dtype) if c.noise_given else None) for k, v in c.noise.items()}
    out = composite(ins["raw"], ins["raw_fw"], ins["raw_bw"], c.zs.to(dtype), c.xyz.to(dtype), ins["f_fw"], ins["f_bw"], noise,
                    c.noise_std, c.has_transient, c.flow_mode, defect)
    assert sorted(out) == sorted(c.names)
    values = {k: v.detach() for k, v in out.items()}
    if not grads:
        return values, None
    total = sum((out[k] * c.cot[k].to(dtype)).sum() for k in c.names)
    wanted = ["raw"] + (["f_fw", "f_bw"] if c.flow_mode >= 1 else []) + (["raw_fw", "raw_bw"] if c.flow_mode >= 2 else [])
    got = torch.autograd.grad(total, [ins[k] for k in wanted], allow_unused=True)
    return values, {"d_" + k: (torch.zeros_like(ins[k]) if v is None else v) for k, v in zip(wanted, got)}


@functools.lru_cache(maxsize=None)
def reference(key):
    """The shared, read-only reference of a case: float64 outputs / gradients, and d32 per output and per gradient group."""
    c = make_case(*key)
    out64, g64 = evaluate(c, torch.float64)
    out32, g32 = evaluate(c, torch.float32)
    d32_g = {(t, g): float(ray_errors(g32[t][..., sl], g64[t][..., sl], c.empty_ray).max())
             for t, g, sl in group_list(c.has_transient, c.flow_mode)}
    d32_o = {k: float(ray_errors(out32[k], out64[k], c.empty_ray).max()) for k in c.names}
    return SimpleNamespace(case=c, out=out64, grads=g64, out32=out32, grads32=g32, d32_grads=d32_g, d32_out=d32_o)


# ---- the rule ----
def ray_errors(got, want, empty_ray):
    """per ray: largest |got - want| over the largest |want| of that ray (of the whole case for the designated empty ray);
    a ray whose reference is identically zero must be reproduced exactly.  Non-finite values give inf."""
    n = want.shape[0]
    got, want = got.detach().double().reshape(n, -1), want.detach().double().reshape(n, -1)
    diff = (got - want).abs().amax(1)
    scale = want.abs().amax(1)
    if empty_ray is not None:
        scale = scale.clone()
        scale[empty_ray] = want.abs().max()
    err = torch.where(scale > 0, diff / scale.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")),
                                                                             torch.zeros_like(diff)))
    return torch.where(torch.isfinite(got).all(1), err, torch.full_like(err, float("inf")))


def bound(d32, factor=FACTOR):
    return max(factor * d32, FLOOR)


def gradient_errors(ref, grads):
    """{(tensor, group): (largest ray error, bound, d32)} of a set of gradients (n, S, C) against the reference of a case"""
    c = ref.case
    return {(t, g): (float(ray_errors(grads[t][..., sl], ref.grads[t][..., sl], c.empty_ray).max()),
                     bound(ref.d32_grads[(t, g)]), ref.d32_grads[(t, g)])
            for t, g, sl in group_list(c.has_transient, c.flow_mode)}


def output_errors(ref, outs):
    c = ref.case
    return {k: (float(ray_errors(outs[k], ref.out[k], c.empty_ray).max()), bound(ref.d32_out[k]), ref.d32_out[k]) for k in c.names}
