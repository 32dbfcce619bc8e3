"""The selection rule of the fused loss kernels (csrc/loss.hip), restated in numpy, and seeded render-dict leaves of any size.

Both device paths -- rank counting inside one workgroup (<= 4096 rays) and the radix select over many -- are defined by it:

* median: the element of rank (N - 1) // 2 in ascending order, ties to the lower index (torch.median's lower median);
* term: population = every ray, for the two flow terms the rays whose per-ray entry is not negative; M its size,
  K = int(topk * M) (M for topk >= 1); selected = the K largest values, ties to the lower index;
  coef[n] = weight[n] / K on the selected rays, else 0; term = sum of the selected values / K.

A stable argsort IS "ties to the lower index".
"""
import numpy as np
import torch

TERMS = ("col_l", "disp_l", "entropy_l", "cross_entropy_l", "flow_fw_l", "flow_bw_l", "pho_l", "cyc_l",
         "reg_temp_sm_l", "reg_min_l", "reg_sp_sm_l")
MASKED = (4, 5)
ST_MED, ST_IDX = 0, 6


def median(x):
    """(value, index) of the lower median of a 1-d array"""
    x = np.asarray(x)
    i = int(np.argsort(x, kind="stable")[(len(x) - 1) // 2])
    return x[i], i


def select(values, topk, masked=False):
    """(selected (N) bool, K, M) for one term's per-ray values"""
    v = np.asarray(values)
    pop = np.flatnonzero(~(v < 0)) if masked else np.arange(len(v))
    M = len(pop)
    K = M if topk >= 1 else int(topk * M)
    order = pop[np.argsort(-v[pop].astype(np.float64), kind="stable")]      # descending, ties to the lower index
    sel = np.zeros(len(v), bool)
    sel[order[:K]] = True
    return sel, K, M


def reduce_term(values, topk, weights=None, masked=False):
    """(coef (N) fp32, term fp64) of one term"""
    v = np.asarray(values)
    sel, K, _ = select(v, topk, masked)
    w = np.ones(len(v), np.float32) if weights is None else np.asarray(weights, np.float32)
    coef = np.where(sel, w / np.float32(max(K, 1)), np.float32(0)).astype(np.float32)
    return coef, (float(v[sel].astype(np.float64).sum()) / K if K else 0.0)


# ---- seeded render-dict leaves of the NSFF train configuration (no render needed) ----
NO_GRAD = ("disocc_fw", "disocc_bw", "disoccs_fw", "disoccs_bw", "xyzs_fine")


def synthetic_render(n, s, seed, coarse=True):
    """The keys NeRFWLoss consumes, as CPU fp32 tensors of the shapes render_rays gives them: NDC points with z < 0.85 (ndc2world has
    its pole at z = 1), weights and disocclusion weights in (0, 1]."""
    g = torch.Generator().manual_seed(9000 + seed)

    def r(*shape):
        return torch.rand(*shape, generator=g)

    def points(*lead):
        return torch.cat([r(*lead, 2) * 2 - 1, r(*lead, 1) * 1.7 - 0.9], -1)
    xyzs = points(n, s)
    d = dict(rgb_fine=r(n, 3), depth_fine=r(n) * 1.5 + 0.1,
             transient_weights_fine=r(n, s) * 0.1 + 1e-3, static_weights_fine=r(n, s) * 0.1 + 1e-3,
             xyz_fw=points(n), xyz_bw=points(n), rgb_fw=r(n, 3), rgb_bw=r(n, 3),
             disocc_fw=r(n, 1) * 0.9 + 0.1, disocc_bw=r(n, 1) * 0.9 + 0.1,
             disoccs_fw=r(n, s, 1) * 0.9 + 0.1, disoccs_bw=r(n, s, 1) * 0.9 + 0.1,
             xyzs_fine=xyzs, xyzs_fw=xyzs + (r(n, s, 3) - 0.5) * 0.05, xyzs_bw=xyzs + (r(n, s, 3) - 0.5) * 0.05,
             xyzs_fw_bw=xyzs + (r(n, s, 3) - 0.5) * 0.02, xyzs_bw_fw=xyzs + (r(n, s, 3) - 0.5) * 0.02)
    if coarse:
        d.update(rgb_coarse=r(n, 3), depth_coarse=r(n) * 1.5 + 0.1)
    return d


def synthetic_ts(n, n_frames, seed):
    """frame indices over the whole range: the rays of the first / last frame have no backward / forward neighbour"""
    return torch.randint(0, n_frames, (n,), generator=torch.Generator().manual_seed(9500 + seed))


def leaves_of(render, device=None, dtype=None):
    """fresh leaves (requires_grad where the loss is differentiated) of a synthetic render dict"""
    return {k: v.detach().clone().to(device=device, dtype=dtype).requires_grad_(k not in NO_GRAD) for k, v in render.items()}


def grad_statistics(grads, seed=778):
    """{key: [sum g, sum |g|, <g, r>]} over the sorted keys, r ~ N(0, 1) from a fixed generator (as scenes.grad_stats)"""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k in sorted(grads):
        g = grads[k].detach().cpu().double()
        rr = torch.randn(g.shape, generator=gen).double()
        out[k] = [float(g.sum()), float(g.abs().sum()), float((g * rr).sum())]
    return out
