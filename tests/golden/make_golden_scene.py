"""Generate tests/golden/g29_scene_scale.npz by RUNNING THE REFERENCE's scene-scale and pose statements.

Build-container only, like make_golden_resize.py: the reference (kwea123/nsff_pl, read-only, absent on the GPU box) supplies the
statements, this file only the inputs and stand-ins.  The statements of datasets/monocular.py from ``pts_w = np.zeros(...)``
to ``self.Ps = self.K @ rt`` (:85-132) and the three pose functions of datasets/colmap_utils.py (``normalize``, ``average_poses``,
``center_poses``) are read when this tool runs and executed on seeded synthetic scenes with the installed numpy and scipy.  What is
not installed gets a stand-in: a ``cv2`` namespace whose ``imread`` returns the prepared float array and whose ``resize`` is the
identity at ``img_wh``; ``self`` is a SimpleNamespace; ``pts3d`` a dict of tuples with ``.xyz`` and ``.image_ids``.  ``linregress``
is scipy's, wrapped to record its result and the loop's arrays per frame.  Only inputs, results and versions are written.

    python tests/golden/make_golden_scene.py               # rewrites tests/golden/g29_scene_scale.npz

Keys: ``cases``, ``numpy``, ``scipy``; per case ``<c>/K`` (3,3) fp32, ``<c>/w2c`` (F,4,4), ``<c>/points`` (N,3), ``<c>/point_index``,
``<c>/image_id`` (the flat visibility pairs, with ids outside the frame range), ``<c>/start_end``, ``<c>/vis`` (F,N) uint8,
``<c>/disps`` (F,H,W) fp32; per frame ``<c>/slope``, ``intercept``, ``rvalue``, ``p95_disp`` fp32, ``p5_depth``, ``disp_os`` (F,2),
``depth_os`` (F,2), ``candidate``, ``pix`` (F,N) int32 (-1 not visible); ``<c>/nearest_depth``, ``<c>/poses`` (F,3,4), ``<c>/Ps`` (F,3,4) float64 (before the reference's cast to fp32).

Cases (F, W x H, N) -- the smallest at which each mechanism can go wrong: H*W = 960 fits one 1024-pixel block, 2077 is odd, spans
three and ends in a ragged quad; N = 300 spans two 256-point blocks, 700 three:
  c0  3  40 x 24  300  clean disp = a/d + b at distinct pixels (r^2 ~ 1), different visibility per frame
  c1  3  67 x 31  700  frame 1 noisy (r^2 low: the depth-percentile branch) with a few points behind the camera; frame 2 with ~10 %
                       of its points projecting outside the image on every side (the clip)
  c2  2  40 x 24  300  integer-valued disparities (a 16-bit PNG's) with heavy ties straddling rank lo, negative values and -0.0;
                       frame 1 constant
  c3  1  21 x 20   64  n - 1 = 419: 0.95 (n - 1) is no integer (g != 0)
  c4  1  41 x 1    64  n - 1 = 40: g = 0;   c4b the same with n_vis = 2
Conditions asserted here, so that the reference itself stays clear of its discontinuities: every visible in-image point's u and v
have a fractional part in [0.1, 0.9]; every frame's r^2 is outside [0.85, 0.95]; p95 - intercept > 0.05 where the regression is
used.  Two points on one pixel overwrite each other's planted disparity, so clean frames see distinct pixels only.
"""
import os
import textwrap
import types

import numpy as np
import scipy
from scipy.stats import linregress

import make_golden

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 2900
CASES = dict(c0=(3, 40, 24, 300), c1=(3, 67, 31, 700), c2=(2, 40, 24, 300), c3=(1, 21, 20, 64), c4=(1, 41, 1, 64),
             c4b=(1, 41, 1, 64))
START = 2                                                         # start_frame: rows are image id - 1 - START


def reference_block(rel, first_mark, last_mark, keep_last=True):
    """The dedented lines of a reference file from the one holding first_mark to the one holding last_mark, compiled."""
    path = os.path.join(make_golden.REF, rel)
    lines = open(path).read().split("\n")
    a = next(i for i, l in enumerate(lines) if first_mark in l)
    b = next(i for i, l in enumerate(lines) if last_mark in l and i >= a)
    return compile(textwrap.dedent("\n".join(lines[a:b + (1 if keep_last else 0)])), path, "exec")


def rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def scene(rng, name):
    """Inputs of a case: K, w2c (F,4,4), points, vis (F,N), disps (F,H,W) fp32."""
    F, W, H, N = CASES[name]
    f = 0.9 * max(W, 24)
    K = np.array([[f, 0, W / 2], [0, f * 1.013, H / 2], [0, 0, 1]], dtype=np.float32)
    w2c = np.tile(np.eye(4), (F, 1, 1))
    for i in range(F):
        w2c[i, :3, :3] = rotation(rng, 0.04 * (i + 1) if H > 1 else 0.003)
        w2c[i, :3, 3] = rng.normal(size=3) * 0.15
        if H == 1:                                                # one row: keep v inside it
            w2c[i, 1, 3] *= 0.05
    clip_frame = 2 if name == "c1" else None
    noisy_frame = 1 if name == "c1" else None
    if clip_frame is not None:
        w2c[clip_frame, 2, 3] -= 1.4                              # closer: the points spread past every border
    depth = rng.uniform(2.5, 9.0, N)
    spread = 0.46 if H > 1 else 0.5
    points = np.stack([rng.uniform(-spread, spread, N) * depth * W / f, rng.uniform(-spread, spread, N) * depth * (H if H > 1 else 0.5) / f, depth], 1)
    if noisy_frame is not None:
        points[:4, 2] = -rng.uniform(1.0, 3.0, 4)                 # behind every camera
    vis = np.zeros((F, N), np.uint8)
    disps = np.empty((F, H, W), np.float32)
    Kd = K.astype(np.float64)
    for i in range(F):
        c = w2c[i, :3, :3] @ points.T + w2c[i, :3, 3:]
        uvd = Kd @ c
        uv = uvd[:2] / uvd[2:]
        inside = (uv[0] >= 0) & (uv[0] < W) & (uv[1] >= 0) & (uv[1] < H)
        frac = uv - np.floor(uv)
        clear = ((frac > 0.12) & (frac < 0.88)).all(0)
        px = np.clip(uv[1].astype(int), 0, H - 1) * W + np.clip(uv[0].astype(int), 0, W - 1)
        want = rng.random(N) < (0.75 if name != "c4b" else 1.0)
        want &= clear | ~inside
        if i == noisy_frame:
            want[:4] = True                                       # the points behind the camera
        else:
            want &= uvd[2] > 0
        want &= inside | (uvd[2] < 0) | ((rng.random(N) < 0.12) if i == clip_frame else False)
        if i == clip_frame:                                       # ... with some past each of the four borders
            for side in (uv[0] < 0, uv[0] >= W, uv[1] < 0, uv[1] >= H):
                some = np.flatnonzero(side & (uvd[2] > 0))[:3]
                assert len(some) == 3
                want[some] = True
        if i not in (noisy_frame, clip_frame):                    # clean frames: one point per pixel
            seen = set()
            for j in np.flatnonzero(want):
                if px[j] in seen:
                    want[j] = False
                seen.add(px[j])
        if name == "c4b":
            keep = np.flatnonzero(want)[[0, -1]]
            want[:] = False
            want[keep] = True
        vis[i] = want
        a, b = 1.3 + 0.2 * i, 0.11 + 0.01 * i
        disp = rng.uniform(0.12, 0.7, H * W)
        planted = a / uvd[2] + b
        if i == noisy_frame:
            planted = planted + rng.normal(size=N) * 0.25
        order = np.flatnonzero(want & inside) if i != clip_frame else np.flatnonzero(want)
        disp[px[order]] = planted[order]
        if name == "c2":
            if i == 1:
                disp[:] = 7.0
            else:                                                 # a 16-bit PNG's integers; the top tenth tied; negatives and -0.0
                disp = np.round(disp * 2000.0)
                top = rng.permutation(np.setdiff1d(np.arange(H * W), px[order]))[:H * W // 10]
                disp[top] = 1500.0
                low = np.setdiff1d(np.arange(H * W), np.concatenate([px[order], top]))
                disp[low[:6]] = -5.0
                disp[low[6:12]] = -0.0
        disps[i] = disp.reshape(H, W).astype(np.float32)
    return K, w2c, points, vis, disps


def run_reference(block, poses_fns, K, w2c, points, vis, disps, point_index, image_id):
    """Execute the reference's statements on one scene; returns (namespace `self`, per-frame records)."""
    F, H, W = disps.shape
    ids = {}
    for p, j in zip(point_index, image_id):
        ids.setdefault(int(p), []).append(int(j))
    P3 = types.SimpleNamespace
    pts3d = {1000 + i: P3(xyz=points[i], image_ids=np.array(ids.get(i, []), np.int64)) for i in range(len(points))}
    me = types.SimpleNamespace(N_frames=F, start_frame=START, end_frame=START + F, img_wh=(W, H), K=K,
                               disp_paths=list(range(F)))
    cv2 = types.SimpleNamespace(IMREAD_ANYDEPTH=0, INTER_NEAREST=0, imread=lambda path, flag: disps[path].copy(),
                                resize=lambda img, wh, interpolation: img)
    records = []
    scope = {"np": np, "cv2": cv2, "self": me, "pts3d": pts3d, "w2c_mats": w2c, "poses": np.linalg.inv(w2c)[:, :3],
             "colmap_utils": types.SimpleNamespace(center_poses=poses_fns["center_poses"])}

    def recording_linregress(x, y):
        reg = linregress(x, y)
        records.append(dict(reg=reg, depth=scope["pts_d_v"].copy(), uvd=scope["pts_uvd_v"].copy(), uv=scope["pts_uv_v"].copy(),
                            disp=scope["disp"].copy()))
        return reg
    scope["linregress"] = recording_linregress
    exec(block, scope)
    me.visibilities = scope["visibilities"]
    return me, records


def main():
    block = reference_block("datasets/monocular.py", "pts_w = np.zeros((1, 3, len(pts3d)))", "self.Ps = self.K @ rt")
    fns = {"np": np}
    exec(reference_block("datasets/colmap_utils.py", "def normalize(v):", "def create_spiral_poses", keep_last=False), fns)
    rng = np.random.default_rng(SEED)
    out = {"cases": np.array(list(CASES)), "numpy": np.array(np.__version__), "scipy": np.array(scipy.__version__)}
    for name, (F, W, H, N) in CASES.items():
        K, w2c, points, vis, disps = scene(rng, name)
        pi, fi = np.nonzero(vis.T)
        point_index, image_id = pi.astype(np.int64), (fi + 1 + START).astype(np.int64)
        # pairs the rule must drop: image ids before and after the frame range
        extra = rng.integers(0, N, 8)
        point_index = np.concatenate([point_index, extra])
        image_id = np.concatenate([image_id, np.array([1, 2, START, START, START + F + 1, START + F + 2, 1, START + F + 1])])
        me, records = run_reference(block, fns, K, w2c, points, vis, disps, point_index, image_id)
        assert np.array_equal(me.visibilities, vis) and len(records) == F
        res = {k: [] for k in ("slope", "intercept", "rvalue", "p95_disp", "p5_depth", "disp_os", "depth_os", "candidate", "pix")}
        for i, rec in enumerate(records):
            reg, d = rec["reg"], rec["depth"]
            uv = (rec["uvd"][:2] / rec["uvd"][2:]).T
            inside = (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)
            frac = (uv - np.floor(uv))[inside]
            assert ((frac >= 0.1) & (frac <= 0.9)).all(), (name, i)
            r2 = reg.rvalue ** 2
            assert not 0.85 <= r2 <= 0.95, (name, i, r2)
            p95, p5 = np.percentile(rec["disp"], 95), np.percentile(d, 5)
            assert p95.dtype == np.float32 and p5.dtype == np.float64
            if r2 > 0.9:
                assert p95 - reg.intercept > 0.05, (name, i)
            n, nv = H * W, len(d)
            lo, lo_d = int(np.floor(np.float32(n - 1) * (np.float32(95) / np.float32(100)))), int(np.floor((nv - 1) * 0.05))
            ds, zs = np.sort(rec["disp"].ravel()) + np.float32(0), np.sort(d)
            pix = np.full(N, -1, np.int32)
            pix[vis[i] == 1] = rec["uv"][:, 1] * W + rec["uv"][:, 0]
            for k, v in (("slope", reg.slope), ("intercept", reg.intercept), ("rvalue", reg.rvalue), ("p95_disp", p95), ("p5_depth", p5),
                         ("disp_os", ds[[lo, min(lo + 1, n - 1)]]), ("depth_os", zs[[lo_d, min(lo_d + 1, nv - 1)]]),
                         ("candidate", reg.slope / (p95 - reg.intercept) if r2 > 0.9 else p5), ("pix", pix)):
                res[k].append(v)
            print(f"{name} frame {i}: n_vis {nv:3d} (outside {int((~inside).sum())}, behind {int((d < 0).sum())})  r2 {r2:.4f}  "
                  f"p95 {p95:.4f}  p5 {p5:.4f}  candidate {res['candidate'][-1]:.5f}")
        assert min(1e8, min(res["candidate"])) * 0.75 == me.nearest_depth
        out.update({f"{name}/{k}": np.asarray(v) for k, v in res.items()})
        out.update({f"{name}/K": K, f"{name}/w2c": w2c, f"{name}/points": points, f"{name}/vis": vis, f"{name}/disps": disps,
                    f"{name}/point_index": point_index, f"{name}/image_id": image_id, f"{name}/start_end": np.array([START, START + F]),
                    f"{name}/nearest_depth": np.float64(me.nearest_depth), f"{name}/poses": me.poses,
                    f"{name}/Ps": me.Ps})
        print(f"{name}: nearest_depth {me.nearest_depth:.6f}")
    path = os.path.join(HERE, "g29_scene_scale.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, numpy", np.__version__, "scipy", scipy.__version__)
    assert os.path.getsize(path) < 500_000


if __name__ == "__main__":
    main()
