"""The launch plans of the two field dispatchers (csrc/field_h3.hip::h3_plan_launch, csrc/field_bwd.hip::bwd_plan_launch) through
their host-only views nsff_field_launch_plan / nsff_field_bwd_launch_plan: no GPU involved.

tests/golden/launch_plan_trace.npz is the trace of the dispatchers as they were BEFORE they were split into fill / plan / issue:
the same sweep run through the old nsff_h3_field_query / nsff_field_backward compiled for the host with recording stubs in place
of the launches, the compute-unit query and the environment -- per case the return code (kernel code or error) and, per launch,
kernel, grid, block, the persistent-grid words and a hash of the kernel's argument bytes.  The plan must reproduce it case for case.
"""
import itertools
import os
import re

import numpy as np

from nsff_pl_amd import _lib
from nsff_pl_amd.config import PRECISIONS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan_trace.npz")
W = _lib.PLAN_WORDS
KERNEL_CODES = {name: code for code, name in _lib.KERNEL_NAMES.items() if name}
ERR_INVALID, ERR_NULL, ERR_ALIGN = -1, -2, -3


def P(i):
    """a distinct, 16-byte aligned fake device address (the plan calls never read through a pointer)"""
    return 0x10000 * (i + 1)


def desc(D=8, skips=(4,), viewdir=0, in_a=0, in_t=48, n_freqs=10, transient=1):
    skips = sorted(skips)
    return _lib.ModelDesc(D=D, W=256, skip=skips[0] if len(skips) == 1 else 0, skip_mask=sum(1 << s for s in skips) if len(skips) != 1 else 0,
                          in_xyz=3 + 6 * n_freqs, in_dir=27, in_a=in_a if viewdir else 0, in_t=in_t, use_viewdir=viewdir,
                          has_transient=transient, has_flow=transient, flow_scale=0.25)


def models():
    out = []
    for D, skips in ((2, ()), (2, (1,)), (4, ()), (4, (3,)), (8, ()), (8, (4,)), (8, (7,))):
        for viewdir, in_a in ((0, 0), (1, 0), (1, 32)):
            for in_t in (48, 34):
                for n_freqs in (10, 12):            # 63 columns: one 64-column segment; 75: two
                    out.append(dict(D=D, skips=skips, viewdir=viewdir, in_a=in_a, in_t=in_t, n_freqs=n_freqs))
    return out


THRESHOLD_MODELS = [dict(D=8, skips=(4,)), dict(D=8, skips=(4,), viewdir=1, in_a=32), dict(D=2, skips=()), dict(D=8, skips=(7,)),
                    dict(D=4, skips=(3,), viewdir=1), dict(D=8, skips=(4,), in_t=34), dict(D=8, skips=(2, 5), viewdir=1, in_a=8)]


def fwd_args(m, n_points, modes, tile=130, ppr=64, save=0, rows=(0, 0), launch_form=0, raw_xyz=True, n_freqs=None, lo=(0, 0, 0),
             t_emb_off=0):
    """save: 0 inference, 1 training forward (every buffer the model has), 2 acts + masks only, 3 masks only"""
    d = desc(**m)
    a = _lib.FieldArgs(n_points=n_points, precision=PRECISIONS["f16x3"], tile_points=tile, pts_per_ray=ppr, static_mode=modes[0],
                       transient_mode=modes[1], flow_heads=0, raw=P(0), launch_form=launch_form)
    if raw_xyz:
        a.xyz = P(1)
        a.n_freqs = m.get("n_freqs", 10) if n_freqs is None else n_freqs
        for i in range(a.n_freqs):
            a.freqs[i] = float(2 ** i)
        a.dir_emb, a.a_emb, a.t_emb = P(2), (P(3) if d.in_a else None), P(4) + t_emb_off
    else:
        a.x_emb, a.ld_emb, a.off_xyz, a.off_dir, a.off_a, a.off_t = P(5), 512, 0, 128, 192, 256
    side_model = bool(d.use_viewdir and modes[0] == 2)
    if save:
        a.save_masks = P(8)
        if save in (1, 2):
            a.save_acts = P(6)
        if save == 1:
            a.save_xin = P(7)
            a.save_side = P(9) if side_model else None
    for i in range(3):
        a.save_lo_delta[i] = lo[i]
    if rows[0]:
        a.s_bias, a.s_bias_rows = P(10), 1
    if rows[1]:
        a.t_bias, a.t_bias_rows = P(11), 1 + len(m.get("skips", (4,)))
    return d, a


def forward_cases():
    """(label, desc, args, n_cus, no_persist) in a fixed order"""
    MODES = ((2, 0), (0, 2), (2, 2))
    # 1. structure: every model x modes x tiling x inference / training forward (+ remainder planes) x rows x samples per ray
    for m in models():
        for modes, tile, (save, lo), rows, ppr, n in itertools.product(
                MODES, (64, 130, 131), ((0, (0, 0, 0)), (1, (0, 0, 0)), (1, (1 << 30, 0, 0))), ((0, 0), (1, 1)), (64, 96, 0),
                (128 * 300, 128 * 300 - 64)):
            yield ("structure", *fwd_args(m, n, modes, tile, ppr, save, rows, lo=lo), 256, 0)
    # 2. persistent-grid thresholds of the inference launches
    tiles = sorted({1, 2, 3, 4, 5, 6, 64, 127, 128, 129, 130, 135, 140, 150, 151, 152, 153, 160, 200, 255, 256, 257, 303, 304, 305, 400, 1000})
    points = [128 * t for t in tiles] + [128 * t - o for t in (128, 256, 304) for o in (64, 37)]
    for m in THRESHOLD_MODELS:
        for modes, rows, (n_cus, form, nop), n in itertools.product(
                MODES, ((0, 0), (1, 0), (0, 1), (1, 1)), ((256, 0, 0), (256, 1, 0), (256, 0, 1), (304, 0, 0), (6, 0, 0), (0, 0, 0), (260, 0, 0)), points):
            yield ("persist", *fwd_args(m, n, modes, 130, 128 if n % 128 == 0 else 64, 0, rows, form), n_cus, nop)
    # 3. the training forward's own rules: even tiles, 4 GiB per slot, which buffers are given, sigma-only modes, aligned time codes
    for m in THRESHOLD_MODELS:
        for modes, save, rows, n in itertools.product(MODES + ((1, 1), (1, 0)), (1, 2, 3), ((0, 0), (1, 0)),
                                                      (128, 64, 192, 200, 64 * 131070, 64 * 131072, 64 * 131072 - 64, 0x7fffffc0, 0x80000000)):
            yield ("save", *fwd_args(m, n, modes, 130, 64, save, rows), 256, 0)
        for modes, save, off in itertools.product(MODES, (0, 1), (4, 8)):
            yield ("t_emb", *fwd_args(m, 128 * 300, modes, 130, 64, save, (1, 1), t_emb_off=off), 256, 0)
        for modes, save in itertools.product(MODES, (0, 1)):       # codes of the side tile not given; rows of another count
            d, a = fwd_args(m, 128 * 300, modes, 130, 64, save, (1, 1))
            a.dir_emb = None
            yield ("no_dir", d, a, 256, 0)
            d, a = fwd_args(m, 128 * 300, modes, 130, 64, save, (1, 1))
            a.s_bias_rows, a.t_bias_rows = 2, 7
            yield ("rows", d, a, 256, 0)
            d, a = fwd_args(m, 128 * 300, modes, 0, 64, save, (1, 1))     # more points than an int32 holds
            a.n_points = 0x80000000 + 128
            yield ("int32", d, a, 256, 0)
        for modes, tile in itertools.product(MODES + ((1, 1),), (64, 130)):   # rows the caller embedded
            yield ("x_emb", *fwd_args(m, 128 * 300, modes, tile, 64, 0, (1, 1), raw_xyz=False), 256, 0)
    # 4. every early NSFF_ERR_INVALID of the dispatcher
    m = THRESHOLD_MODELS[1]
    yield ("err_freqs", *fwd_args(m, 4096, (2, 2), n_freqs=9), 256, 0)
    yield ("err_save_no_xyz", *fwd_args(m, 4096, (2, 2), save=3, raw_xyz=False), 256, 0)
    for lo in ((-8, 0, 0), (0, 12, 0), (0, 0, 64)):          # negative; not a multiple of 8; no buffer behind it (save 2: no save_side)
        yield ("err_lo", *fwd_args(m, 4096, (2, 2), save=2, lo=lo), 256, 0)
    yield ("err_steps", *fwd_args(dict(D=8, skips=(1, 2, 3, 4, 5, 6, 7), viewdir=1), 4096, (2, 2)), 256, 0)
    for tile, save, n in itertools.product((64, 130, 131), (0, 1), (64 << 30, (128 << 30) + 1)):     # 2 x tiles beyond int32
        yield ("err_grid", *fwd_args(m, n, (2, 2), tile, 64, save), 256, 0)
        yield ("err_grid", *fwd_args(THRESHOLD_MODELS[0], n, (0, 2), tile, 64, save), 256, 0)


def bwd_args(m, n_points, modes, lo=0, want_xin=True, **over):
    d = desc(**m)
    a = _lib.FieldBwdArgs(n_points=n_points, static_mode=modes[0], transient_mode=modes[1], d_raw=P(0), raw=P(1), gmax=P(2), masks=P(3),
                          dpre=P(4), dhead=P(5), d_xin=P(6) if want_xin else None, d_side=P(7) if d.use_viewdir else None, dpre_lo_delta=lo)
    for k, v in over.items():
        setattr(a, k, v)
    return d, a


def backward_cases():
    """(label, desc, args, n_cus, kernel_override, persist)"""
    MODES = ((2, 0), (0, 2), (2, 2))
    for m in models():
        for modes, n, lo, d_xin, (ko, persist) in itertools.product(MODES, (128 * 2000, 128 * 2000 - 64, 64), (0, 1 << 20), (True, False),
                                                                     ((None, 1), ("c", 1), (None, 0))):
            yield ("structure", *bwd_args(m, n, modes, lo, d_xin), 256, ko, persist)
    # the 2 x compute-units item rule: one trunk's items are the 128-point tiles, both trunks' twice that
    for m in THRESHOLD_MODELS:
        for modes, (n_cus, t128) in itertools.product(MODES, [(c, t) for c in (256, 304, 6, 0) for t in
                                                              (1, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 4 * c) if t > 0]):
            for ko, persist in ((None, 1), (None, 0), ("c", 1), ("h", 1)):
                yield ("items", *bwd_args(m, 128 * t128, modes), n_cus, ko, persist)
    m = THRESHOLD_MODELS[1]
    yield ("empty", *bwd_args(m, 0, (2, 2)), 256, None, 1)
    for modes in ((1, 0), (0, 1), (0, 0), (3, 2), (2, -1)):
        yield ("err_modes", *bwd_args(m, 4096, modes), 256, None, 1)
    yield ("err_transient", *bwd_args(dict(D=8, skips=(4,), transient=0), 4096, (2, 2)), 256, None, 1)
    yield ("err_negative", *bwd_args(m, -1, (2, 2)), 256, None, 1)
    for lo in (-8, 12):
        yield ("err_lo", *bwd_args(m, 4096, (2, 2), lo), 256, None, 1)
    yield ("err_tiles", *bwd_args(m, 64 << 31, (2, 2)), 256, None, 1)
    yield ("max_tiles", *bwd_args(m, (64 << 31) - 64, (0, 2)), 256, None, 1)
    # (the densest model make_layout_b accepts has 26 backward steps: the dispatcher's "more than 40 steps" return cannot be reached)
    yield ("max_steps", *bwd_args(dict(D=8, skips=(1, 2, 3, 4, 5, 6, 7), viewdir=1), 4096, (2, 2)), 256, None, 1)
    for name in ("d_raw", "raw", "gmax", "masks", "dpre", "dhead"):
        yield ("err_null", *bwd_args(m, 4096, (2, 2), **{name: None}), 256, None, 1)
    for name in ("d_raw", "raw", "masks", "dpre", "dhead", "d_xin", "d_side"):
        yield ("err_align", *bwd_args(m, 4096, (2, 2), **{name: P(9) + 4}), 256, None, 1)


def trace(cases, call):
    rows = []
    for case in cases:
        code, recs = call(*case[1:])
        rows.append([code] + [w for r in recs for w in r] + [0] * (W * (3 - len(recs))))
    return np.asarray(rows, dtype=np.int64).astype(np.int32)


def forward_trace():
    return trace(forward_cases(), _lib.field_launch_plan)


def backward_trace():
    return trace(backward_cases(), _lib.field_bwd_launch_plan)


def first_difference(got, want, cases):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad) == 0:
        return None
    i = int(bad[0])
    label = next(itertools.islice(cases, i, None))[0]
    return f"{len(bad)} of {len(got)} cases differ; first: case {i} ({label}): plan {got[i].tolist()} != recorded {want[i].tolist()}"


def test_forward_plan_reproduces_the_recorded_dispatcher():
    got, want = forward_trace(), np.load(GOLDEN)["forward"]
    assert first_difference(got, want, forward_cases()) is None, first_difference(got, want, forward_cases())


def test_backward_plan_reproduces_the_recorded_dispatcher():
    got, want = backward_trace(), np.load(GOLDEN)["backward"]
    assert first_difference(got, want, backward_cases()) is None, first_difference(got, want, backward_cases())


def test_the_sweep_reaches_every_kernel_form_and_error():
    g = np.load(GOLDEN)
    f, b = g["forward"], g["backward"]
    codes = set(f[:, 0].tolist())
    assert {KERNEL_CODES[n] for n in KERNEL_CODES if n.startswith("h3")} <= codes, sorted(codes)
    assert ERR_INVALID in codes
    h3a = f[:, 1:].reshape(len(f), 3, W)
    p_modes = {int(r[3]) for rec in h3a for r in rec if r[0] == 6}
    assert p_modes == {0, 1, 2, 3, 4}, p_modes
    assert {int(r[0]) for rec in h3a for r in rec} == {0, 1, 2, 3, 4, 5, 6, 7}           # every kernel, and unused records
    assert {0, 1, 2, 3, ERR_NULL, ERR_INVALID, ERR_ALIGN} <= set(b[:, 0].tolist())
    labels = [c[0] for c in forward_cases()]
    for lab in ("err_freqs", "err_save_no_xyz", "err_lo", "err_steps", "err_grid"):
        got = {int(f[i, 0]) for i, l in enumerate(labels) if l == lab}
        assert ERR_INVALID in got and (lab == "err_grid" or got == {ERR_INVALID}), (lab, got)
    labels = [c[0] for c in backward_cases()]
    for lab, err in (("err_modes", ERR_INVALID), ("err_transient", ERR_INVALID), ("err_negative", ERR_INVALID), ("err_lo", ERR_INVALID),
                     ("err_tiles", ERR_INVALID), ("err_null", ERR_NULL), ("err_align", ERR_ALIGN)):
        assert {int(b[i, 0]) for i, l in enumerate(labels) if l == lab} == {err}, lab


# ---- the Python callers restate two consequences of the plan (a ctypes call per launch would sit on the timed path) ----
def python_supplies_side_rows(n_points, samples_per_ray, tile_points, training):
    """rendering.py (inference of a view-direction model, f16x3): when it computes NsffFieldArgs::s_bias for the launch"""
    big_enough = training or tile_points == 130 or (tile_points == 0 and n_points >= 32768)
    return bool(n_points and samples_per_ray % 64 == 0 and tile_points in (0, 130) and big_enough)


def python_forward_can_save(static_mode, transient_mode):
    """field_grad.forward_can_save: the mode clause"""
    return static_mode in (0, 2) and transient_mode in (0, 2) and bool(static_mode or transient_mode)


def test_the_restatements_are_the_callers_own_text():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rendering = re.sub(r"\s+", " ", open(os.path.join(root, "nsff_pl_amd", "rendering.py")).read())
    assert "big_enough = ctx.rec is not None or config.get_tile_points() == 130 or (config.get_tile_points() == 0 and P >= 32768)" in rendering
    assert ("P and S % 64 == 0 and config.get_precision() == \"f16x3\" and config.get_tile_points() in (0, 130) and big_enough"
            in rendering)
    grad = re.sub(r"\s+", " ", open(os.path.join(root, "nsff_pl_amd", "field_grad.py")).read())
    assert "static_mode in (0, 2) and transient_mode in (0, 2) and (static_mode or transient_mode))" in grad


def test_python_side_row_predicate_agrees_with_the_plan():
    """Side rows are supplied exactly when the plan uses them (samples per ray a multiple of 64) -- for the (model, modes) the
    hand-scheduled body executes at all, i.e. whose large 128-point-tile launch uses them.  For the others (a position embedding of
    more than 64 columns; time codes not in float4 rows next to a dynamic trunk; a skip layer last) rendering.py still computes
    rows that the plan ignores: one small wasted launch, as before this test."""
    checked = ignored = 0
    for m in models():
        if not m["viewdir"]:
            continue
        for modes in ((2, 0), (2, 2)):
            executes = _lib.field_launch_plan(*fwd_args(m, 128 * 300, modes, 130, 64, 0, (1, 0)), 256)[0] == KERNEL_CODES["h3a_side"]
            for tile, ppr, n in itertools.product((0, 64, 130, 131), (64, 128, 192), (64, 4096, 32768 - 64, 32768, 32768 + 64, 128 * 300)):
                code, recs = _lib.field_launch_plan(*fwd_args(m, n, modes, tile, ppr, 0, (1, 0)), 256)
                assert code > 0
                used = any(r[0] == 6 and r[10] == 1 for r in recs)
                assert used == (code == KERNEL_CODES["h3a_side"])
                supplied = python_supplies_side_rows(n, ppr, tile, training=False)
                assert used == (supplied and executes), (m, modes, tile, ppr, n)
                checked += executes
                ignored += supplied and not executes
    assert checked > 1000 and ignored > 0


def test_python_forward_can_save_agrees_with_the_backward():
    """render_rays' own launch is made the training forward exactly for the modes nsff_field_backward accepts"""
    for m in THRESHOLD_MODELS:
        for sm, tm in itertools.product((0, 1, 2), (0, 1, 2)):
            code, _ = _lib.field_bwd_launch_plan(*bwd_args(m, 128 * 40, (sm, tm)), 256)
            assert (code >= 0) == python_forward_can_save(sm, tm), (m, sm, tm, code)
