"""Camera paths and time indices of the reference's test splits (datasets/monocular.py:190-209, 256-266 and
datasets/colmap_utils.py:373-429), host numpy in float64.

* :func:`spiral_poses` -- ``colmap_utils.create_spiral_poses``: rotations slerped between the key poses, positions interpolated
  linearly, and a ``radii * [cos t, -sin t, 0]`` offset that runs over four turns.  The slerp is written here in numpy
  (``R_i exp(alpha log(R_i^T R_{i+1}))``, Rodrigues both ways); the package does not depend on scipy.
* :func:`wander_path`  -- ``colmap_utils.create_wander_path``; returns the (n, 3, 4) top rows of the reference's 4 x 4 matrices
  (its ray generation reads only those).
* :func:`split_path`   -- the poses, the time index of every pose and the interpolation count of ``test``, ``test_spiral``,
  ``test_spiral{X}`` and ``test_fixview{X}_interp{Y}``.
"""
import re

import numpy as np

SPLIT_FORMS = "'test', 'test_spiral', 'test_spiral{X}' or 'test_fixview{X}_interp{Y}'"


def _hat(v):
    x, y, z = v
    return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])


def rotation_log(R):
    """Rotation vector of a rotation matrix (angle below pi): axis * angle."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])      # axis * sin(angle)
    s = np.linalg.norm(v)
    angle = np.arctan2(s, 0.5 * (np.trace(R) - 1.0))
    return v if s < 1e-12 else v * (angle / s)


def rotation_exp(w):
    """Rodrigues' formula: the rotation matrix of a rotation vector."""
    angle = np.linalg.norm(w)
    K = _hat(w)
    if angle < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(angle) / angle) * K + ((1.0 - np.cos(angle)) / angle ** 2) * (K @ K)


def slerp_rotations(rotations, times):
    """Rotations (N, 3, 3) at the integer key times 0 .. N-1, interpolated at ``times`` (each in [0, N-1]): (len(times), 3, 3)."""
    rotations = np.asarray(rotations, dtype=np.float64)
    n = len(rotations)
    logs = [rotation_log(rotations[i].T @ rotations[i + 1]) for i in range(n - 1)]
    out = np.empty((len(times), 3, 3))
    for k, t in enumerate(times):
        i = min(max(int(np.searchsorted(np.arange(n), t, side="left")) - 1, 0), n - 2)     # the interval (i, i + 1] holding t
        out[k] = rotations[i] @ rotation_exp((t - i) * logs[i])
    return out


def spiral_poses(poses, radii, n_poses=120):
    """colmap_utils.create_spiral_poses: poses (N, 3, 4), radii (3,) -> (n_poses, 3, 4)."""
    poses = np.asarray(poses, dtype=np.float64)
    radii = np.asarray(radii, dtype=np.float64)
    n = len(poses)
    if poses.ndim != 3 or poses.shape[1:] != (3, 4) or n < 2:
        raise ValueError(f"spiral_poses: need at least two (3, 4) poses, got {poses.shape}")
    times = np.linspace(0, n - 1, n_poses + 1)[:-1]
    out = np.zeros((n_poses, 3, 4))
    out[:, :, :3] = slerp_rotations(poses[:, :, :3], times)
    xyz = np.stack([np.interp(times, np.arange(n), poses[:, i, 3]) for i in range(3)], -1)
    turn = np.linspace(0, 8 * np.pi, n_poses + 1)[:-1]                                     # 8 pi: four rounds
    out[:, :, 3] = xyz + radii * np.stack([np.cos(turn), -np.sin(turn), np.zeros_like(turn)], -1)
    return out


def wander_path(c2w, max_trans, n_poses=60):
    """colmap_utils.create_wander_path: c2w (3, 4) or (4, 4) -> (n_poses, 3, 4), the top rows of ``c2w @ inv([I | t_i])``."""
    c2w = np.asarray(c2w, dtype=np.float64)[:3, :4]
    phase = 2.0 * np.pi * np.arange(n_poses, dtype=np.float64) / float(n_poses)
    trans = np.stack([max_trans * np.sin(phase), max_trans * np.cos(phase) / 2.0, max_trans * np.cos(phase)], -1)
    out = np.empty((n_poses, 3, 4))
    out[:, :, :3] = c2w[:, :3]
    out[:, :, 3] = c2w[:, 3] - trans @ c2w[:, :3].T                                        # inv([I | t]) = [I | -t]
    return out


def parse_split(split, n_frames=None):
    """('test' | 'spiral' | 'wander' | 'fixview', X or None, Y or 0) of a split name; ValueError names the forms."""
    kind, target, interp = None, None, 0
    if split == "test":
        kind = "test"
    elif split == "test_spiral":
        kind = "spiral"
    else:
        m = re.fullmatch(r"test_spiral(\d+)", str(split))
        if m:
            kind, target = "wander", int(m.group(1))
        m = re.fullmatch(r"test_fixview(\d+)_interp(\d+)", str(split))
        if m:
            kind, target, interp = "fixview", int(m.group(1)), int(m.group(2))
    if kind is None:
        raise ValueError(f"split {split!r} is not one of {SPLIT_FORMS}")
    if target is not None and n_frames is not None and target >= n_frames:
        raise ValueError(f"split {split!r}: target frame {target} is outside the sequence of {n_frames} frames ({SPLIT_FORMS})")
    return kind, target, interp


def split_path(poses, split):
    """``(poses_test (n, 3, 4) float64, ts (n,) int64, interp)`` of a test split over the dataset poses (N, 3, 4).

    test: the poses themselves at times 0 .. N-1.  test_fixview{X}_interp{Y}: pose X repeated N times at times 0 .. N-1, interp = Y.
    test_spiral: a 6 N pose spiral with radii [m, m, 0], m the 10th percentile of the x steps between frames, at times
    int(i / (6 N) * N).  test_spiral{X}: the 60-pose wander path about pose X with max_trans |x_0 - x_{N-1}| / 5, all at time X."""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (3, 4):
        raise ValueError(f"split_path: poses must be (N, 3, 4), got {poses.shape}")
    n = len(poses)
    kind, target, interp = parse_split(split, n)
    if kind == "test":
        return poses.copy(), np.arange(n, dtype=np.int64), 0
    if kind == "fixview":
        return np.tile(poses[target], (n, 1, 1)), np.arange(n, dtype=np.int64), interp
    if kind == "spiral":
        max_trans = np.percentile(np.abs(np.diff(poses[:, 0, 3])), 10)
        out = spiral_poses(poses, np.array([max_trans, max_trans, 0]), n_poses=6 * n)
        return out, np.array([int(i / len(out) * n) for i in range(len(out))], dtype=np.int64), 0
    max_trans = np.abs(poses[0, 0, 3] - poses[-1, 0, 3]) / 5
    out = wander_path(poses[target], max_trans=max_trans, n_poses=60)
    return out, np.full(len(out), target, dtype=np.int64), 0


def frame_names(n_poses, interp=0):
    """The frame names of eval.py:186, 216, 225 in order: '{i:03d}', or '{i:03d}_{int(dt*100):03d}' with interp images per pose and
    the last pose closing the sequence at '_000' ((n_poses - 1) * interp + 1 names)."""
    if interp <= 0:
        return [f"{i:03d}" for i in range(n_poses)]
    names = [f"{i:03d}_{int(dt * 100):03d}" for i in range(n_poses - 1) for dt in np.linspace(0, 1, interp + 1)[:-1]]
    return names + [f"{n_poses - 1:03d}_000"]
