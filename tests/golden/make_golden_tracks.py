"""Generate tests/golden/g30_tracks.npz by CHAINING THE REFERENCE's own forward in float64: scene-flow tracks over four steps.

Build-container only, like make_golden.py (whose reference import it uses): the reference (kwea123/nsff_pl, read-only, absent on
the GPU box) supplies ``NeRF`` / ``PosEmbedding``, this file the inputs and the loop:

* the model is a seeded tests/scenes.py scene (``CFG``: fine model with flow heads) moved to float64; ``max_t = 5`` (six frames of its
  30-row time table), cameras ``tests/scenes.camera_buffers()``'s first six.  Its gain is 1.5, not the 2.5 of the render goldens: at
  2.5 the chained map is chaotic -- a 1e-6 perturbation of the start grows 2e4-fold (forward) and 8e4-fold (backward) in three steps,
  and the bound below becomes 0.5 .. 1.8, which pins nothing -- while at 1.5 flows reach 0.025 NDC units a step and a perturbation
  grows 2 .. 5-fold a step: a field that varies in space, and a bound below 1e-4 at every step;
* ``xyz`` (R, S, 3) = (37, 3, 3) fp32 NDC start points, x, y in [-1, 1], z in [-1, 0.85] except ``N_FAR`` points with z in
  [0.91, 0.99] -- beyond z = 0.9, i.e. (z + 1) / 2 > 0.95, the reference zeroes a flow (rendering.py:126,187-188 on NDC rays);
  ``ts`` = r mod 6, so going forward rows die after 5, 4, ... 0 steps and going backward after 0, 1, ... 5;
* per direction d in fw / bw (n = 4 steps): the query of render_transient_warping (rendering.py:112-126) -- ``model(cat[embedding_xyz(x),
  dir, t], output_static=False, output_transient=True, output_transient_flow=[d])`` columns 4:7 -- at ``(x_j, E_t[t_j])``, zeroed where
  (z + 1) / 2 > 0.95, added where the row can still step: ``xyz_d`` (5, R, S, 3) float64 paths, ``flow_d`` (4, R, S, 3) what moved the
  points (0 for a row that could not step), ``t_d`` / ``alive_d`` (5, R); ``uv_time_d`` / ``uv_fixed_d`` (5, R, S, 2) float64 pixels seen by
  the camera of each step's own time and by the fixed camera ``FIXED_VIEW`` (tests/tracks_numpy.project, the formulas of
  losses.py:99-111 in float64; 1e10 behind the camera);
* ``bound_d`` (5,): the tolerance of a free-running fp32 chain at step j, from the reference alone.  Each query i may be off by the
  project's standing max-norm bar, ``1e-4 max|flow_i|``; an error made at query i sits in ``x_{i+1}`` and is carried through the
  remaining j - i - 1 steps, growing by ``G[i+1 -> j]``, the measured max-norm growth of a 1e-6 perturbation of ``x_{i+1}`` (the largest
  of ``N_PROBES`` random sign patterns, never below 1: a stopped row keeps its error): ``bound[j] = sum_{i<j} 1e-4 max|flow_i| G[i+1 -> j]``.
  No sample may lie within ``MARGIN`` of the zero rule's threshold at any step, perturbed or not (asserted), so the rule is decided
  alike by any fp32 chain that stays within the bound.

Only inputs and results are written; no reference source travels.

    python tests/golden/make_golden_tracks.py               # rewrites tests/golden/g30_tracks.npz
"""
import os
import sys

import numpy as np
import torch

import make_golden

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import scenes  # noqa: E402
import tracks_numpy as tnp  # noqa: E402

CFG = dict(n_rays=37, N_samples=3, N_importance=0, transient=True, viewdir=False, appearance=False, test_time=True,
           flow=['fw', 'bw'], gain=1.5, seed=30)
R, S, N, MAX_T = 37, 3, 4, 5
N_FAR, FIXED_VIEW = 14, 2
QUERY_TOL, PERTURB, N_PROBES, MARGIN = 1e-4, 1e-6, 8, 2e-4


def reference_field(model, embeddings):
    """(xyz (R, S, 3) float64, t (R,), direction) -> the reference's flow head at (xyz, E_t[t]), float64."""
    def run(xyz, t, direction):
        n_rows, s = xyz.shape[:2]
        x = torch.from_numpy(np.ascontiguousarray(xyz.reshape(-1, 3)))
        rows = embeddings["t"](torch.from_numpy(np.asarray(t, np.int64))).repeat_interleave(s, 0)
        pad = torch.zeros(n_rows * s, model.in_channels_dir + model.in_channels_a, dtype=torch.float64)
        with torch.no_grad():
            out = model(torch.cat([embeddings["xyz"](x), pad, rows], 1), output_static=False, output_transient=True,
                        output_transient_flow=["fw" if direction > 0 else "bw"])
        return out[:, 4:7].numpy().reshape(n_rows, s, 3)
    return run


def margin(path):
    return np.abs((path[..., 2] + 1) * 0.5 - tnp.Z_FAR).min()


def growth(field, chain, direction, rng):
    """G[m][j], m <= j: growth of a 1e-6 max-norm perturbation of slab m by slab j."""
    G = np.ones((N + 1, N + 1))
    for m in range(1, N):
        for _ in range(N_PROBES):
            x = chain["xyz"][m] + PERTURB * rng.choice([-1.0, 1.0], chain["xyz"][m].shape)
            t, alive = chain["t"][m], chain["alive"][m]
            for j in range(m, N):
                x, t, alive, _ = tnp.step(x, t, alive, field(x, t, direction), direction, MAX_T)
                assert margin(x) > MARGIN
                G[m][j + 1] = max(G[m][j + 1], np.abs(x - chain["xyz"][j + 1]).max() / PERTURB)
    return G


def main():
    NeRF, PosEmbedding, _, _ = make_golden.import_reference()
    models, embeddings = scenes.build_scene(NeRF, PosEmbedding, CFG)
    checksum = scenes.weight_checksum(models, embeddings)
    model = models["fine"].double()
    embeddings["t"].double()
    field = reference_field(model, embeddings)
    rng = np.random.default_rng(30)
    xyz = np.concatenate([rng.uniform(-1, 1, (R, S, 2)), rng.uniform(-1, 0.85, (R, S, 1))], -1)
    far = rng.choice(R * S, N_FAR, replace=False)
    xyz.reshape(-1, 3)[far, 2] = rng.uniform(0.91, 0.99, N_FAR)
    xyz = xyz.astype(np.float32)
    ts = (np.arange(R) % (MAX_T + 1)).astype(np.int32)
    K, Ps, _ = scenes.camera_buffers()
    K, Ps = K[0].numpy().astype(np.float64), Ps[0, :MAX_T + 1].numpy().astype(np.float32)
    K4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    out = dict(xyz=xyz, ts=ts, max_t=np.int32(MAX_T), K=K, Ps=Ps, fixed_view=np.int32(FIXED_VIEW), weight_checksum=np.float64(checksum),
               query_tol=np.float64(QUERY_TOL))
    for tag, steps in (("fw", N), ("bw", -N)):
        chain = tnp.advect(field, xyz.astype(np.float64), ts, steps, MAX_T)
        assert chain["xyz"].dtype == np.float64 and margin(chain["xyz"]) > MARGIN, margin(chain["xyz"])
        zeroed = tnp.zero_rule(chain["xyz"][:-1]) & chain["alive"][1:, :, None]
        G = growth(field, chain, steps, rng)
        fmax = np.abs(chain["flow"]).max((1, 2, 3))
        bound = np.array([sum(QUERY_TOL * fmax[i] * G[i + 1][j] for i in range(j)) for j in range(N + 1)])
        uv_time, _ = tnp.project_path(chain["xyz"], chain["t"], K4, Ps)
        uv_fixed, _ = tnp.project_path(chain["xyz"], chain["t"], K4, Ps[FIXED_VIEW], fixed_view=True)
        out.update({"xyz_" + tag: chain["xyz"], "flow_" + tag: chain["flow"], "t_" + tag: chain["t"], "alive_" + tag: chain["alive"],
                    "uv_time_" + tag: uv_time, "uv_fixed_" + tag: uv_fixed, "bound_" + tag: bound, "growth_" + tag: G})
        print(f"{tag}: alive rows per slab {chain['alive'].sum(1).tolist()}; zeroed samples per step {zeroed.sum((1, 2)).tolist()}; "
              f"margin to the zero rule {margin(chain['xyz']):.2e}; behind a camera: {int((uv_time[..., 0] == 1e10).sum())} (own time), "
              f"{int((uv_fixed[..., 0] == 1e10).sum())} (fixed)")
        print("  step j | max|flow_j| | growth G[j+1 -> 4] | bound[j]")
        for j in range(N + 1):
            print(f"  {j}      | {fmax[j] if j < N else float('nan'):.4e}  | {G[min(j + 1, N)][N]:8.3f}           | {bound[j]:.3e}")
    path = os.path.join(HERE, "g30_tracks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
