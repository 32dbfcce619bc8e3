"""Numpy restatement of the training split's ray records (reference datasets/monocular.py:136-184 with
datasets/ray_utils.py:7-106), the role tests/splat_ref.py has for the splat kernels: fp32 step by step, in the reference's order
of operations, with no reference code.  Used by the CPU tests of tests/test_ray_records_host.py against golden g24."""
import numpy as np

f32 = np.float32


def uv_grid(H, W):
    """(H*W, 2) fp32 pixel coordinates (column, row), row-major, no half-pixel offset (ray_utils.py:23-32)."""
    j, i = np.mgrid[:H, :W]
    return np.stack([i, j], -1).reshape(-1, 2).astype(f32)


def ndc_rays(K, c2w, H, W, near=1.0):
    """(H*W, 6) fp32: get_ray_directions -> get_rays -> get_ndc_rays with shift_near = -min(-1, c2w[2,3])."""
    K, c2w = np.asarray(K, f32), np.asarray(c2w, f32)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    uv = uv_grid(H, W)
    dirs = np.stack([(uv[:, 0] - cx) / fx, -(uv[:, 1] - cy) / fy, -np.ones(H * W, f32)], -1)
    d = (dirs @ c2w[:, :3].T).astype(f32)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True, dtype=f32))
    o = np.broadcast_to(c2w[:, 3], d.shape)
    shift_near = f32(-min(-1.0, float(c2w[2, 3])))
    t = -(shift_near + o[:, 2]) / d[:, 2]
    o = o + t[:, None] * d
    ox_oz, oy_oz = o[:, 0] / o[:, 2], o[:, 1] / o[:, 2]
    sx, sy = f32(-1.0) / (cx / fx), f32(-1.0) / (cy / fy)
    o2 = f32(1.0) + f32(2.0) * f32(near) / o[:, 2]
    out = np.stack([sx * ox_oz, sy * oy_oz, o2, sx * (d[:, 0] / d[:, 2] - ox_oz), sy * (d[:, 1] / d[:, 2] - oy_oz),
                    f32(1.0) - o2], -1)
    assert out.dtype == f32
    return out


def to_float(x):
    """uint8 -> fp32 by a true division by 255 (torchvision's ToTensor); fp32 passes through."""
    x = np.asarray(x)
    return x.astype(f32) / f32(255) if x.dtype == np.uint8 else x.astype(f32)


def records(K, poses, images, disps, masks, flows_fw=None, flows_bw=None, near=1.0):
    """(F, H*W, 16) fp32 in the column layout of monocular.py:181-184."""
    F, H, W = np.asarray(images).shape[:3]
    uv = uv_grid(H, W)
    out = np.zeros((F, H * W, 16), f32)
    for t in range(F):
        zero = np.zeros((H * W, 2), f32)
        fw = zero if flows_fw is None or t == F - 1 else np.asarray(flows_fw[t], f32).reshape(-1, 2)
        bw = zero if flows_bw is None or t == 0 else np.asarray(flows_bw[t], f32).reshape(-1, 2)
        out[t, :, :6] = ndc_rays(K, poses[t], H, W, near)
        out[t, :, 6:9] = to_float(images[t]).reshape(-1, 3)
        out[t, :, 9] = t
        out[t, :, 10] = np.asarray(disps[t], f32).reshape(-1)
        out[t, :, 11] = to_float(masks[t]).reshape(-1)
        out[t, :, 12:14] = uv + fw
        out[t, :, 14:16] = uv + bw
    return out


def projection_matrices(K, poses):
    """(F, 3, 4) float64: K @ flip(inverse([pose; 0 0 0 1])[:3]), rows 1 and 2 negated (monocular.py:127-132)."""
    K, poses = np.asarray(K, np.float64), np.asarray(poses, np.float64)
    out = []
    for p in poses:
        rt = np.linalg.inv(np.vstack([p, [0, 0, 0, 1]]))[:3]
        out.append(K @ (np.diag([1.0, -1.0, -1.0]) @ rt))
    return np.stack(out)
