"""TEST INFRASTRUCTURE: the three small fp32 kernels around a field launch -- ``nsff_time_bias`` and ``nsff_side_bias``
(csrc/field_h3.hip), ``nsff_field_input_backward`` (csrc/field_bwd.hip) -- as plain numpy expressions of their inputs, the cases
the kernels are held to and the comparison rule.  Nothing here touches the GPU; every case is seeded, built once and read-only.

Each operation exists twice: in float64 (the reference) and as a float32 "twin" that does the same arithmetic in numpy float32,
one rounding per operation, in the order the header documents.  The twin is not the kernel: it measures what fp32 costs the
expression -- the yardstick ``d32`` of the rule.

The rule is the project's (composite_ref.FACTOR / FLOOR): a figure is inside when it is at most ``max(8 d32, 16 * 2^-24)``, with
``d32`` the twin's own distance from float64 in the same measure.

    time / side bias, d_t   per (ray, row): largest error over the row's columns over the largest |reference| among them
    d_xyz                   per element, over M = |d[c]| + sum_f f (|d_cos| + |d_sin|), the sum of the absolute terms

Time bias (include/nsff_render.h): out[ray][i] = b_l + W_l[:, in_xyz : in_xyz + in_t] t, l = 0 and then the skip layers in
ascending order, W_l / b_l the parameters of ``transient_xyz_encoding_{l+1}[0]``.  The twin adds the columns one by one in
ascending order.  The two weight columns on either side of the window (in_xyz - 1 and in_xyz + in_t, for a skip layer the first
fed-back column) are 100 times their initial size, so that a window off by one misses by far more than any bound.

Side bias: out[ray] = b_dir + W_dir[:, :256] b_final + W_dir[:, 256:] [dir | a] with W_dir / b_dir of ``static_dir_encoding[0]``
and b_final the bias of ``static_xyz_encoding_final`` (nerf.py: static_dir_encoding reads [static_xyz_encoding_final(h) | dir | a];
nsff_pack_weights folds the activation-free *_final layer into it, so its bias arrives through W_dir[:, :256]).

Input backward: d_xyz[p, c] = d[c] + sum_f f (cos(a) d[3 + 6 f + c] - sin(a) d[3 + 6 f + 3 + c]) with a the FLOAT32 product
float32(f) * float32(x) widened to float64 -- the argument PosEmbedding's forward takes the sine of, which is the definition of the
operation (with the linear frequency list an exact-product reference lies up to 138 x 2^-24 of M away; for powers of two the two
coincide); d_t[ray] = the sum of the ray's S rows of columns [t0, t0 + in_t), its twin the sequential fp32 sum in point order,
which the kernel must reproduce bit for bit (plain adds in that order, nothing to contract).
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import nsff_pl_amd as A
from composite_ref import FACTOR, FLOOR, bound  # noqa: F401  (the project's rule; re-exported for the tests)

W = 256
ULP = 2.0 ** -24
RAY_COUNTS = (1, 15, 16, 17, 37)               # both sides of the sixteen-ray workgroup
N_RAYS_MAX = max(RAY_COUNTS)

# (D, skips, n_freqs, in_t)
TIME_MODELS = ((8, (4,), 10, 48),              # the default
               (2, (), 6, 16),                 # no skip layer
               (5, (3,), 8, 20),               # in_t not a multiple of 16
               (3, (2,), 10, 4),               # the narrowest time code
               (6, (1, 2, 3, 4, 5), 4, 36),    # six rows, in_t not a multiple of 16
               (8, (1, 2, 3, 4, 5, 6, 7), 10, 64))   # eight rows = NSFF_MAX_LAYERS, the widest time code
TIME_DEFECTS = ("window_right", "window_left", "partial_tile")
SIDE_MODELS = ((27, 0), (27, 48), (27, 6))     # (in_dir, in_a); 33 columns: no multiple of 4 or 16
SIDE_DEFECTS = ("no_final_bias",)

# index mode: a 12-row table of which frames 0..8 are in use (a cropped sequence); frame indices at both clamps, at the
# table's end and outside the table
N_TABLE, MAX_T = 12, 8
TS_EDGE = (0, 1, 7, 8, 11, -3, 40)
N_INDEX_RAYS = 21                              # two workgroups, the second ragged
INDEX_DEFECTS = ("clamp_at_table_end",)

# (xin_rows, t_row0, in_t, n_freqs, logscale)
GEOMETRIES = ((128, 64, 48, 10, True),
              (128, 64, 48, 10, False),
              (128, 32, 4, 4, True),
              (256, 128, 64, 12, True),
              (256, 192, 64, 24, True),        # NSFF_MAX_FREQS
              (128, 8, 16, 0, True))           # no frequencies: d_xyz = d[0:3]
S_LIST = (1, 2, 63, 64, 65, 128, 130, 200)     # both sides of every 64-point chunk
RAYS_BWD = (1, 5)
XYZ_DEFECTS = ("sine_sign", "top_frequency")
DT_DEFECTS = ("last_point",)


def _frozen(a):
    a.setflags(write=False)
    return a


def _f32(x):
    return np.asarray(x, dtype=np.float32)


# ---- the rule ----
def row_errors(got, want):
    """got, want (..., C): per leading index, largest |got - want| over the largest |want| of that row; a row whose reference is
    identically zero must be reproduced exactly; anything non-finite gives inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    diff, scale = np.abs(got - want).max(-1), np.abs(want).max(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff > 0, np.inf, 0.0))
    return np.where(np.isfinite(got).all(-1), err, np.inf)


def element_errors(got, want, scale):
    """per element |got - want| / scale (scale > 0 wherever want != 0); anything non-finite gives inf"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    diff = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff > 0, np.inf, 0.0))
    return np.where(np.isfinite(got), err, np.inf)


# ---- time bias ----
def time_layers(model_index):
    """the layers (0-based) of a time-bias model that read the time code: 0 and the skip layers, ascending"""
    _, skips, _, _ = TIME_MODELS[model_index]
    return [0] + sorted(skips)


def make_time_model(model_index):
    """A fresh CPU module of TIME_MODELS[model_index] with seeded weights and the two columns beside the time-code window of
    every layer that has the window scaled by 100.  (Not cached: the caller may move it to a device.)"""
    D, skips, n_freqs, in_t = TIME_MODELS[model_index]
    torch.manual_seed(1800 + model_index)
    in_xyz = 3 + 6 * n_freqs
    m = A.NeRF("fine", D=D, skips=list(skips), in_channels_xyz=in_xyz, use_viewdir=False, encode_transient=True,
               in_channels_t=in_t, output_flow=True)
    with torch.no_grad():
        for l in time_layers(model_index):
            w = getattr(m, f"transient_xyz_encoding_{l + 1}")[0].weight
            w[:, in_xyz - 1] *= 100.0
            if w.shape[1] > in_xyz + in_t:
                w[:, in_xyz + in_t] *= 100.0
    return m


def time_bias(ws, bs, in_xyz, t_rows, dtype, defect=None):
    """(n, rows, 256) of the layers' (weight, bias) pairs.  float64: one matrix product; float32: column by column in ascending
    order, a rounding after every product and every sum.  defect: one of TIME_DEFECTS (never used for a reference)."""
    assert defect is None or defect in TIME_DEFECTS
    in_t = t_rows.shape[1]
    shift = {"window_right": 1, "window_left": -1}.get(defect, 0)
    cols = [j for j in range(in_t) if not (defect == "partial_tile" and j >= 16 * (in_t // 16))]
    t = np.asarray(t_rows, dtype)
    out = np.empty((t.shape[0], len(ws), W), dtype)
    for i, (w, b) in enumerate(zip(ws, bs)):
        w, b = np.asarray(w, dtype), np.asarray(b, dtype)
        flat, at = w.reshape(-1), np.arange(W) * w.shape[1] + in_xyz + shift
        col = lambda j: flat[np.minimum(at + j, flat.size - 1)]      # (a shifted window runs into the next row, as a kernel's would)
        if dtype == np.float64:
            out[:, i] = b + t[:, cols] @ np.stack([col(j) for j in cols], 0)
            continue
        acc = np.broadcast_to(b, (t.shape[0], W)).copy()
        for j in cols:
            acc = acc + t[:, j:j + 1] * col(j)[None, :]
        out[:, i] = acc
    return out


@functools.lru_cache(maxsize=None)
def time_case(model_index):
    """weights, the 37 seeded time-code rows, the float64 reference, the twin and d32 per ray count of one model.  A launch of
    n rays takes the first n rows."""
    D, skips, n_freqs, in_t = TIME_MODELS[model_index]
    m = make_time_model(model_index)
    lins = [getattr(m, f"transient_xyz_encoding_{l + 1}")[0] for l in time_layers(model_index)]
    ws = [_frozen(p.weight.detach().numpy().copy()) for p in lins]
    bs = [_frozen(p.bias.detach().numpy().copy()) for p in lins]
    in_xyz = 3 + 6 * n_freqs
    assert all(w.shape == (W, in_xyz + in_t + (W if l else 0)) for w, l in zip(ws, time_layers(model_index)))
    g = torch.Generator().manual_seed(1900 + model_index)
    t_rows = _frozen(torch.randn(N_RAYS_MAX, in_t, generator=g).numpy())
    want = _frozen(time_bias(ws, bs, in_xyz, t_rows, np.float64))
    twin = _frozen(time_bias(ws, bs, in_xyz, t_rows, np.float32))
    err = row_errors(twin, want)
    return SimpleNamespace(index=model_index, in_xyz=in_xyz, in_t=in_t, rows=len(ws), ws=ws, bs=bs, t_rows=t_rows, want=want,
                           twin=twin, d32={n: float(err[:n].max()) for n in RAY_COUNTS})


# ---- index mode ----
def gather_index(ts, delta, n_table=N_TABLE, max_t=MAX_T, defect=None):
    """the table row of every ray: the reference's clamp(ts + 1, max=max_t) / clamp(ts - 1, min=0) / ts (rendering.py:153,218,224),
    then kept inside the table"""
    assert defect is None or defect in INDEX_DEFECTS
    t = np.asarray(ts, np.int64) + delta
    if delta > 0:
        t = np.minimum(t, n_table - 1 if defect == "clamp_at_table_end" else max_t)
    if delta < 0:
        t = np.maximum(t, 0)
    return np.clip(t, 0, n_table - 1)


@functools.lru_cache(maxsize=None)
def index_case():
    """the frame indices and the table (in_t = 48) of the index-mode launch"""
    g = torch.Generator().manual_seed(2000)
    ts = list(TS_EDGE) + [int(v) for v in torch.randint(0, N_TABLE, (N_INDEX_RAYS - len(TS_EDGE),), generator=g)]
    table = torch.randn(N_TABLE, 48, generator=g).numpy()
    return SimpleNamespace(ts=_frozen(np.asarray(ts, np.int64)), table=_frozen(table))


def make_coarse_model():
    """the coarse partner of TIME_MODELS[0] in the index-mode launch: two skip layers, so three rows against the fine model's two"""
    torch.manual_seed(2001)
    return A.NeRF("coarse", D=8, skips=[2, 5], in_channels_xyz=63, use_viewdir=False, encode_transient=True, in_channels_t=48)


# ---- side bias ----
def make_side_model(model_index):
    in_dir, in_a = SIDE_MODELS[model_index]
    torch.manual_seed(2100 + model_index)
    return A.NeRF("fine", use_viewdir=True, in_channels_dir=in_dir, encode_appearance=in_a > 0, in_channels_a=max(in_a, 1),
                  encode_transient=False)


def side_bias(w_dir, b_dir, b_final, side, dtype, defect=None):
    """(n, 256).  float32: the folded bias b_dir + sum_j W_dir[:, j] b_final[j] and then the [dir | a] columns, every sum
    sequential in ascending order."""
    assert defect is None or defect in SIDE_DEFECTS
    w, bd, bf, x = (np.asarray(v, dtype) for v in (w_dir, b_dir, b_final, side))
    if dtype == np.float64:
        fold = bd + (0.0 if defect == "no_final_bias" else w[:, :W] @ bf)
        return fold + x @ w[:, W:].T
    fold = bd.copy()
    if defect != "no_final_bias":
        for j in range(W):
            fold = fold + w[:, j] * bf[j]
    acc = np.broadcast_to(fold, (x.shape[0], W)).copy()
    for j in range(x.shape[1]):
        acc = acc + x[:, j:j + 1] * w[None, :, W + j]
    return acc


@functools.lru_cache(maxsize=None)
def side_case(model_index):
    in_dir, in_a = SIDE_MODELS[model_index]
    m = make_side_model(model_index)
    assert m.in_channels_a == in_a
    lin = m.static_dir_encoding[0]
    w_dir, b_dir = _frozen(lin.weight.detach().numpy().copy()), _frozen(lin.bias.detach().numpy().copy())
    b_final = _frozen(m.static_xyz_encoding_final.bias.detach().numpy().copy())
    assert w_dir.shape == (W, W + in_dir + in_a) and in_dir == 27
    g = torch.Generator().manual_seed(2200 + model_index)
    d = torch.randn(N_RAYS_MAX, 3, generator=g).numpy()
    d = _f32(d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float64)
    cols = [d]
    for f in (1.0, 2.0, 4.0, 8.0):                           # PosEmbedding(3, 4) of a unit direction (float64, then rounded:
        cols += [np.sin(f * d), np.cos(f * d)]               #  numpy's float32 sine differs in the last bit between CPUs)
    dirs = _frozen(_f32(np.concatenate(cols, 1)))
    a_rows = _frozen(torch.randn(N_RAYS_MAX, in_a, generator=g).numpy()) if in_a else None
    side = dirs if a_rows is None else np.concatenate([dirs, a_rows], 1)
    want = _frozen(side_bias(w_dir, b_dir, b_final, side, np.float64))
    twin = _frozen(side_bias(w_dir, b_dir, b_final, side, np.float32))
    err = row_errors(twin, want)
    return SimpleNamespace(index=model_index, in_dir=in_dir, in_a=in_a, w_dir=w_dir, b_dir=b_dir, b_final=b_final, dirs=dirs,
                           a_rows=a_rows, side=_frozen(side), want=want, twin=twin,
                           d32={n: float(err[:n].max()) for n in RAY_COUNTS})


# ---- input backward ----
def frequencies(n_freqs, logscale):
    """PosEmbedding(n_freqs - 1, n_freqs, logscale).freqs as float32 (nerf.py:41-44)"""
    if n_freqs == 0:
        return np.zeros(0, np.float32)
    if logscale:
        return (2 ** torch.linspace(0, n_freqs - 1, n_freqs)).numpy()
    return torch.linspace(1, 2 ** (n_freqs - 1), n_freqs).numpy()


def d_xyz(d_xin, xyz, freqs, dtype, defect=None, exact_product=False):
    """(P, 3) and, in float64, the scale M of every element.  The argument is the float32 product f x in both precisions
    (exact_product: the float64 product, to show how far that other definition lies)."""
    assert defect is None or defect in XYZ_DEFECTS
    d, x, f32 = np.asarray(d_xin), _f32(xyz), _f32(freqs)
    g = d[:, 0:3].astype(dtype)
    M = np.abs(d[:, 0:3]).astype(np.float64)
    top = len(f32) - 1
    for k, f in enumerate(f32):
        arg = np.float64(f) * x.astype(np.float64) if exact_product else f * x
        dc, ds = d[:, 3 + 6 * k:6 + 6 * k].astype(dtype), d[:, 6 + 6 * k:9 + 6 * k].astype(dtype)
        M = M + np.float64(f) * (np.abs(dc).astype(np.float64) + np.abs(ds).astype(np.float64))
        if defect == "top_frequency" and k == top:
            continue
        a = arg.astype(dtype)
        sign = -1 if defect == "sine_sign" and k == max(top - 1, 0) else 1
        g = g + dtype(f) * (np.cos(a) * dc - dtype(sign) * np.sin(a) * ds)
    return g, M


def d_t(d_xin, n_rays, S, t0, in_t, dtype, defect=None):
    """(n_rays, in_t): the sum over a ray's points, in float32 sequentially in ascending point order"""
    assert defect is None or defect in DT_DEFECTS
    rows = np.asarray(d_xin)[:, t0:t0 + in_t].reshape(n_rays, S, in_t).astype(dtype)
    last = S - 1 if defect == "last_point" else S
    if dtype == np.float64:
        return rows[:, :last].sum(1)
    acc = np.zeros((n_rays, in_t), np.float32)
    for s in range(last):
        acc = acc + rows[:, s]
    return acc


def _geometry_seed(geometry, n_rays, S):
    xr, t0, in_t, n_freqs, log = geometry
    return 2300 + 7919 * S + 101 * n_rays + 13 * xr + 7 * t0 + 5 * in_t + 3 * n_freqs + int(log)


@functools.lru_cache(maxsize=None)
def input_case(geometry, n_rays, S):
    """d_xin (P, xin_rows): cotangent rows over six decades, NaN in every column outside [0, 3 + 6 n_freqs) and [t0, t0 + in_t)
    (the kernel stages those columns and must not use them); points in [-1.2, 1.2]; references, twins, d32."""
    xr, t0, in_t, n_freqs, log = geometry
    P, in_xyz = n_rays * S, 3 + 6 * n_freqs
    assert in_xyz <= t0 <= xr - in_t
    g = torch.Generator().manual_seed(_geometry_seed(geometry, n_rays, S))
    d = torch.randn(P, xr, generator=g) * 10.0 ** (6.0 * torch.rand(P, 1, generator=g) - 3.0)
    d = d.numpy()
    d[:, in_xyz:t0] = np.nan
    d[:, t0 + in_t:] = np.nan
    xyz = (2.4 * torch.rand(P, 3, generator=g) - 1.2).numpy()
    freqs = frequencies(n_freqs, log)
    want_xyz, M = d_xyz(d, xyz, freqs, np.float64)
    twin_xyz, _ = d_xyz(d, xyz, freqs, np.float32)
    assert np.isfinite(want_xyz).all() and (M > 0).all()
    want_t, twin_t = d_t(d, n_rays, S, t0, in_t, np.float64), d_t(d, n_rays, S, t0, in_t, np.float32)
    return SimpleNamespace(geometry=geometry, n_rays=n_rays, S=S, P=P, xin_rows=xr, t0=t0, in_t=in_t, freqs=_frozen(freqs),
                           d_xin=_frozen(d), xyz=_frozen(xyz), want_xyz=_frozen(want_xyz), M=_frozen(M),
                           twin_xyz=_frozen(twin_xyz), want_t=_frozen(want_t), twin_t=_frozen(twin_t),
                           d32_xyz=float(element_errors(twin_xyz, want_xyz, M).max()),
                           d32_t=float(row_errors(twin_t, want_t).max()))


def input_keys(geometries=GEOMETRIES):
    return [(g, n, S) for g in geometries for n in RAYS_BWD for S in S_LIST]
