"""The three small fp32 kernels around a field launch, called directly: `nsff_time_bias` in row and in index mode and
`nsff_side_bias` (csrc/field_h3.hip), `nsff_field_input_backward` (field_input_bwd_kernel<128 / 256>, csrc/field_bwd.hip), against
the float64 expressions of tests/field_inputs_ref.py on that module's cases: ray counts on both sides of the sixteen-ray
workgroup, time codes of 4 .. 64 columns with and without a partial 16-column tile, one to eight rows per ray, one to four jobs
per launch, frame indices at both clamps and outside the table; samples per ray on both sides of every 64-point chunk, both row
geometries of the trunk-input gradient, 0 .. 24 frequencies.

The rule and where its tolerance comes from are in field_inputs_ref.py: bound max(8 x d32, 16 x 2^-24) with d32 the CPU float32
twin's own distance from float64 -- never a figure of the kernel under test.  The CPU tests pin the twins' figures and show that
the rule notices each planted defect; the figures measured on the MI355X are in EXPERIMENTS.md R18.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import field_inputs_ref as R
import nsff_pl_amd as A
from nsff_pl_amd import _lib, config

DEV = "cuda:0"
TAIL = 64                                     # records behind every output buffer that must stay untouched
NAN = float("nan")
OK, INVALID, NULL, ALIGN = 0, -1, -2, -3      # NSFF_* of include/nsff_render.h
FAKE = 4096                                   # a 16-byte aligned non-null "pointer" for calls that are refused before any launch
gpu = pytest.mark.gpu


# =====================================================================================================================
# CPU: the twins' own figures, the planted defects, the refusals
# =====================================================================================================================
def _ulps(x):
    return round(x / R.ULP, 1)


def test_the_twins_reproduce_their_recorded_figures():
    """d32 of the fp32 twins on this module's seeded cases, in units of 2^-24 to the printed digit (EXPERIMENTS.md R18).  The
    time-bias sums cost 2.5 (in_t = 4) to 6.8 (in_t = 64), growing with the number of columns; d_xyz 1.5 to 1.6 with any
    frequency list, so its bound is the floor; the exact-product definition of d_xyz lies two orders of magnitude further away
    with the linear list and coincides for powers of two."""
    time_d32 = {R.TIME_MODELS[i][3]: _ulps(R.time_case(i).d32[R.N_RAYS_MAX]) for i in range(len(R.TIME_MODELS))}
    assert time_d32 == {48: 6.0, 16: 2.9, 20: 5.3, 4: 2.5, 36: 5.6, 64: 6.8}, time_d32
    side_d32 = {R.SIDE_MODELS[i]: _ulps(R.side_case(i).d32[R.N_RAYS_MAX]) for i in range(len(R.SIDE_MODELS))}
    assert side_d32 == {(27, 0): 5.5, (27, 48): 7.0, (27, 6): 4.1}, side_d32
    xyz_d32, off = {}, {}
    for geo in R.GEOMETRIES:
        cases = [R.input_case(*key) for key in R.input_keys((geo,))]
        xyz_d32[geo] = _ulps(max(c.d32_xyz for c in cases))
        exact = [R.d_xyz(c.d_xin, c.xyz, c.freqs, np.float64, exact_product=True)[0] for c in cases]
        off[geo] = _ulps(max(R.element_errors(e, c.want_xyz, c.M).max() for e, c in zip(exact, cases)))
        assert all(R.bound(c.d32_xyz) == R.FLOOR for c in cases)                # the floor is the bound of d_xyz
    # (numpy's float32 sine and cosine differ in the last bit between CPUs: a range for what goes through them)
    assert all(1.2 <= v <= 1.7 for v in list(xyz_d32.values())[:5]) and xyz_d32[R.GEOMETRIES[5]] == 0.0, xyz_d32
    assert all((100 < v < 200) if not geo[4] else v == 0.0 for geo, v in off.items()), off
    for i in range(len(R.TIME_MODELS)):                                        # d32 never shrinks with more rays of the same list
        d = R.time_case(i).d32
        assert all(d[a] <= d[b] for a, b in zip(R.RAY_COUNTS, R.RAY_COUNTS[1:]))


def test_the_columns_beside_the_window_are_large():
    """a hundred times the initial size, on every layer that has them"""
    for i in range(len(R.TIME_MODELS)):
        c = R.time_case(i)
        for w in c.ws:
            inside = np.abs(w[:, c.in_xyz:c.in_xyz + c.in_t]).max()
            assert np.abs(w[:, c.in_xyz - 1]).mean() > 20 * inside
            if w.shape[1] > c.in_xyz + c.in_t:
                assert np.abs(w[:, c.in_xyz + c.in_t]).mean() > 20 * inside


def _flagged(err, d32):
    """least error / bound of a defective result: above 1 the GPU test would fail on a kernel with that defect"""
    return float(np.min(err)) / R.bound(d32), float(np.max(err)) / R.bound(d32)


def test_the_rule_flags_the_planted_defects():
    """Each defect is planted in the fp32 twin and judged as a kernel's output would be.  `worst / bound` must exceed 1 for the GPU
    test to fail; where the defect touches every row, `least / bound` must."""
    report = {}
    # a window shifted by one column, either way: every row of every model is far outside
    for i in range(len(R.TIME_MODELS)):
        c = R.time_case(i)
        for defect in ("window_right", "window_left"):
            bad = R.time_bias(c.ws, c.bs, c.in_xyz, c.t_rows, np.float32, defect)
            least, _ = _flagged(R.row_errors(bad, c.want), c.d32[R.N_RAYS_MAX])
            report[(defect, i)] = least
            assert least > 100, (defect, i, least)
    # columns 16..19 dropped at in_t = 20: every row
    i = [m[3] for m in R.TIME_MODELS].index(20)
    c = R.time_case(i)
    err = R.row_errors(R.time_bias(c.ws, c.bs, c.in_xyz, c.t_rows, np.float32, "partial_tile"), c.want)
    report["partial_tile"] = _flagged(err, c.d32[R.N_RAYS_MAX])[0]
    assert report["partial_tile"] > 100
    # the +1 clamp at n_table - 1 instead of max_t: the rays at max_t and beyond take another row
    ic, c = R.index_case(), R.time_case(0)
    good, bad = R.gather_index(ic.ts, 1), R.gather_index(ic.ts, 1, defect="clamp_at_table_end")
    hit = good != bad
    assert hit[R.TS_EDGE.index(8)] and hit[R.TS_EDGE.index(11)] and hit[R.TS_EDGE.index(40)] and not hit[R.TS_EDGE.index(7)]
    assert not np.array_equal(ic.table[good[hit]], ic.table[bad[hit]])          # (the GPU test compares the rows bit for bit)
    want = R.time_bias(c.ws, c.bs, c.in_xyz, ic.table[good], np.float64)
    twin = R.time_bias(c.ws, c.bs, c.in_xyz, ic.table[good], np.float32)
    err = R.row_errors(R.time_bias(c.ws, c.bs, c.in_xyz, ic.table[bad], np.float32), want)
    report["clamp_at_table_end"] = _flagged(err[hit], float(R.row_errors(twin, want).max()))[0]
    assert report["clamp_at_table_end"] > 100
    # d_xyz: one frequency's sine term with the wrong sign, the highest frequency left out -- on every case that has frequencies
    for defect in R.XYZ_DEFECTS:
        worst = []
        for key in R.input_keys():
            c = R.input_case(*key)
            if len(c.freqs) == 0:
                continue
            bad, _ = R.d_xyz(c.d_xin, c.xyz, c.freqs, np.float32, defect)
            worst.append(_flagged(R.element_errors(bad, c.want_xyz, c.M), c.d32_xyz)[1])
        report[defect] = min(worst)
        assert len(worst) == 5 * len(R.RAYS_BWD) * len(R.S_LIST) and report[defect] > 100, (defect, report[defect])
    # d_t without the last point of a 65-point ray: other bits, and outside the rule as well
    for geo in R.GEOMETRIES:
        c = R.input_case(geo, 5, 65)
        bad = R.d_t(c.d_xin, c.n_rays, c.S, c.t0, c.in_t, np.float32, "last_point")
        assert not np.array_equal(bad.view(np.int32), c.twin_t.view(np.int32))
        report[("last_point", geo)] = _flagged(R.row_errors(bad, c.want_t), c.d32_t)[1]
        assert report[("last_point", geo)] > 100
    # the folded bias without W_dir[:, :256] b_final: every ray
    for i in range(len(R.SIDE_MODELS)):
        c = R.side_case(i)
        bad = R.side_bias(c.w_dir, c.b_dir, c.b_final, c.side, np.float32, "no_final_bias")
        report[("no_final_bias", i)] = _flagged(R.row_errors(bad, c.want), c.d32[R.N_RAYS_MAX])[0]
        assert report[("no_final_bias", i)] > 100
    print("R18 planted defects, least error / bound:", {k: f"{v:.3g}" for k, v in report.items()})


def test_the_sound_twins_pass_the_rule():
    """... and the rule does not flag the twin itself (d32 <= max(8 d32, floor)), nor a float32 rounding of the reference"""
    for i in range(len(R.TIME_MODELS)):
        c = R.time_case(i)
        assert R.row_errors(c.want.astype(np.float32), c.want).max() <= R.FLOOR
        assert R.row_errors(c.twin, c.want).max() <= R.bound(c.d32[R.N_RAYS_MAX])
    c = R.input_case(R.GEOMETRIES[1], 5, 200)
    assert R.element_errors(c.want_xyz.astype(np.float32), c.want_xyz, c.M).max() <= R.FLOOR


def test_refusals_that_need_no_launch(hip_lib):
    lib = hip_lib
    freqs = (C.c_float * 32)(*[float(2 ** (k % 8)) for k in range(32)])

    def fib(d_xin=FAKE, xin_rows=128, t_row0=64, xyz=FAKE, n_rays=4, pts=8, n_freqs=10, in_t=48, d_xyz=FAKE, d_t=FAKE):
        return lib.nsff_field_input_backward(d_xin, xin_rows, t_row0, xyz, n_rays, pts, freqs, n_freqs, in_t, d_xyz, d_t, None)
    assert fib(xin_rows=64, t_row0=32, n_freqs=4, in_t=4) == INVALID           # the row geometry is 128 or 256
    assert fib(t_row0=81) == INVALID                                           # t_row0 + in_t > xin_rows
    assert fib(n_freqs=21) == INVALID                                          # 3 + 6 x 21 = 129 rows
    assert fib(xin_rows=256, t_row0=192, n_freqs=25) == INVALID                # more than NSFF_MAX_FREQS
    assert fib(pts=0) == INVALID
    assert fib(d_xyz=None, d_t=None) == OK                                     # nothing wanted: nothing launched
    assert fib(d_xin=FAKE + 4, d_xyz=None) == ALIGN
    assert fib(d_xin=FAKE + 4) == ALIGN
    assert fib(d_xin=None) == NULL

    def tb(in_t, with_weights=False):
        m = A.NeRF("fine", use_viewdir=False, encode_transient=True, in_channels_t=in_t, output_flow=True)
        d = _lib.model_desc(m)
        jobs = (_lib.TimeBiasJob * 1)()
        jobs[0].desc, jobs[0].t_rows, jobs[0].out = C.pointer(d), FAKE, FAKE
        if with_weights:
            for i in range(2):
                jobs[0].w[i] = jobs[0].b[i] = FAKE
        return lib.nsff_time_bias(jobs, 1, 4, None)
    assert tb(68, True) == INVALID and tb(6, True) == INVALID                  # wider than 64 columns; no multiple of 4
    assert tb(48) == NULL                                                      # (a width it takes: on to the weight pointers)
    novd = _lib.model_desc(A.NeRF("fine", use_viewdir=False))
    assert lib.nsff_side_bias(C.byref(novd), FAKE, FAKE, FAKE, None, 4, FAKE, None) == INVALID
    vd = _lib.model_desc(A.NeRF("fine", use_viewdir=True, encode_appearance=True, in_channels_a=48))
    assert lib.nsff_side_bias(C.byref(vd), FAKE, FAKE, FAKE, None, 4, FAKE, None) == NULL      # in_a > 0 without a_rows


# =====================================================================================================================
# GPU
# =====================================================================================================================
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.tensor(np.asarray(a)).to(DEV).contiguous()


def _nan(records, width):
    return torch.full((records + TAIL, width), NAN, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


NAN_BITS = int(bits(torch.full((1,), NAN))[0])


def owned(buf, records, what):
    """the records of a NaN-filled buffer that the call owns, on the CPU as numpy: all finite, and the TAIL records behind them
    bit for bit what they were"""
    assert buf.shape[0] == records + TAIL
    assert bool((bits(buf[records:]) == NAN_BITS).all()), (what, "the records behind the call's were written")
    assert bool(torch.isfinite(buf[:records]).all()), (what, "non-finite values")
    return buf[:records].cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _report(tag, rows):
    """rows: (what, error, bound, d32).  Fails on the figures outside their bound; prints what R18 records."""
    bad = [(w, f"err {e / R.ULP:.3g} bound {b / R.ULP:.3g} d32 {d / R.ULP:.3g} (x 2^-24)") for w, e, b, d in rows if not e <= b]
    used = max(rows, key=lambda r: r[1] / r[2])
    line = f"R18 {tag}: {len(rows)} figures, worst error / bound {used[1] / used[2]:.3g} at {used[0]}"
    live = [r for r in rows if r[3] > 0]
    if live:
        top = max(live, key=lambda r: r[1] / r[3])
        line += (f"; worst error / d32 {top[1] / top[3]:.3g} at {top[0]}; worst error {max(r[1] for r in rows) / R.ULP:.3g}, "
                 f"d32 {min(r[3] for r in live) / R.ULP:.3g} .. {max(r[3] for r in live) / R.ULP:.3g} (x 2^-24)")
    print(line)
    assert not bad, f"{len(bad)} of {len(rows)} outside the bound: {bad[:12]}"


# ---- nsff_time_bias ----
@functools.lru_cache(maxsize=None)
def gpu_time_model(model_index):
    return R.make_time_model(model_index).to(DEV)


@functools.lru_cache(maxsize=None)
def gpu_coarse_model():
    return R.make_coarse_model().to(DEV)


def time_layers(m):
    return [getattr(m, f"transient_xyz_encoding_{l + 1}")[0] for l in [0] + sorted(set(int(s) for s in m.skips))]


def launch_time_bias(specs, n_rays):
    """One nsff_time_bias launch through the ctypes structures.  specs: (model, t_rows (n_rays, in_t) device tensor) for a row-mode
    job, (model, (table, ts, max_t, delta, want_rows)) for an index-mode one.  -> [(out (n_rays, rows, 256), rows_out or None)]
    as numpy, after the hygiene checks of owned()."""
    arr = (_lib.TimeBiasJob * len(specs))()
    keep, bufs = [], []
    for j, (m, src) in enumerate(specs):
        desc = _lib.model_desc(m)
        lins = time_layers(m)
        arr[j].desc = C.pointer(desc)
        for i, lin in enumerate(lins):
            arr[j].w[i], arr[j].b[i] = _lib._ptr(lin.weight.detach()), _lib._ptr(lin.bias.detach())
        out, rows_out = _nan(n_rays * len(lins), R.W), None
        arr[j].out = out.data_ptr()
        if isinstance(src, tuple):
            table, ts, max_t, delta, want_rows = src
            assert ts.dtype == torch.int64 and ts.shape == (n_rays,) and table.shape[1] == desc.in_t
            arr[j].table, arr[j].ts, arr[j].n_table, arr[j].max_t, arr[j].delta = _lib._ptr(table), ts.data_ptr(), table.shape[0], max_t, delta
            if want_rows:
                rows_out = _nan(n_rays, desc.in_t)
                arr[j].rows_out = rows_out.data_ptr()
        else:
            assert src.shape == (n_rays, desc.in_t)
            arr[j].t_rows = _lib._ptr(src)
        keep.append((desc, src))
        bufs.append((out, rows_out, len(lins)))
    assert _lib.load().nsff_time_bias(arr, len(specs), n_rays, _stream()) == OK
    torch.cuda.synchronize()
    return [(owned(out, n_rays * rows, f"job {j} out").reshape(n_rays, rows, R.W),
             None if rows_out is None else owned(rows_out, n_rays, f"job {j} rows_out"))
            for j, (out, rows_out, rows) in enumerate(bufs)]


@gpu
@pytest.mark.parametrize("model_index", range(len(R.TIME_MODELS)))
def test_time_bias_rows_against_float64(hip_lib, model_index):
    """row mode: every row of every ray inside the bound at 1, 15, 16, 17 and 37 rays (the NaN tail behind each launch's rows
    untouched), and a ray launched alone has the bits it has in the batch"""
    c, m = R.time_case(model_index), gpu_time_model(model_index)
    assert _lib.time_bias_rows(m) == c.rows
    t_all = _dev(c.t_rows)
    rows, batch = [], None
    for n in R.RAY_COUNTS:
        (got, _), = launch_time_bias([(m, t_all[:n].contiguous())], n)
        err = R.row_errors(got, c.want[:n])
        for i in range(c.rows):
            rows.append((f"{n} rays, row {i}", float(err[:, i].max()), R.bound(c.d32[n]), c.d32[n]))
        if n == 17:
            batch = got
    _report(f"time_bias row mode {R.TIME_MODELS[model_index]}", rows)
    for r in range(17):
        (one, _), = launch_time_bias([(m, t_all[r:r + 1].contiguous())], 1)
        assert same_bits(one[0], batch[r]), f"ray {r} alone differs from the batch"


@gpu
@pytest.mark.parametrize("models", [(0, 2, 4, 5), (1, 3, 0, 2)])
def test_time_bias_job_alone_equals_job_among_four(hip_lib, models):
    """four models in one launch: the grid has the largest model's rows, the others' surplus workgroups write nothing (NaN tails)
    and every job has the bits of its own single-job launch"""
    n = 17
    specs = [(gpu_time_model(i), _dev(R.time_case(i).t_rows[:n])) for i in models]
    four = launch_time_bias(specs, n)
    assert len({R.time_case(i).rows for i in models}) > 1
    for i, spec, (got, _) in zip(models, specs, four):
        (alone, _), = launch_time_bias([spec], n)
        assert same_bits(got, alone), f"model {i}"
        assert R.row_errors(got, R.time_case(i).want[:n]).max() <= R.bound(R.time_case(i).d32[n])


@gpu
def test_time_bias_index_mode(hip_lib):
    """The launch rendering._time_codes issues -- (fine, +1), (fine, -1), (fine, 0), (coarse, 0), the coarse model with one row
    more than the fine one -- on a 12-row table with max_t = 8 and frame indices at the clamps, at the table's end and outside
    it: the gathered rows are the torch expressions bit for bit, the bias rows those of a row-mode call on them, +1 / -1 rows and
    the outputs of the fine model's first two jobs are halves of one buffer; the same launch through the ctypes structures leaves
    every NaN tail alone."""
    ic = R.index_case()
    fine, coarse = gpu_time_model(0), gpu_coarse_model()
    assert _lib.time_bias_rows(fine) == 2 and _lib.time_bias_rows(coarse) == 3
    E, ts = _dev(ic.table), torch.tensor(ic.ts).to(DEV)
    n, width = ts.shape[0], E.shape[1]
    assert E.shape[0] == R.N_TABLE and n == R.N_INDEX_RAYS
    want_rows = {0: E[ts.clamp(0, R.N_TABLE - 1)],
                 1: E[torch.clamp(ts + 1, max=R.MAX_T).clamp(0, R.N_TABLE - 1)],
                 -1: E[torch.clamp(ts - 1, min=0).clamp(0, R.N_TABLE - 1)]}
    for d in (0, 1, -1):                                                        # (the numpy index of the CPU tests is that expression)
        assert same_bits(want_rows[d].cpu().numpy(), ic.table[R.gather_index(ic.ts, d)])
    plan = [(fine, 1), (fine, -1), (fine, 0), (coarse, 0)]
    outs, rows = _lib.time_bias(plan, index=(E, ts, R.MAX_T))
    torch.cuda.synchronize()
    assert sorted(rows) == [-1, 0, 1]
    for d in (0, 1, -1):
        assert rows[d].shape == (n, width) and torch.equal(bits(rows[d]), bits(want_rows[d])), f"rows of delta {d}"
    by_rows = _lib.time_bias([(mod, rows[d]) for mod, d in plan])
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(outs, by_rows)):
        assert a.shape == (n, 2 if j < 3 else 3, R.W) and torch.equal(bits(a), bits(b)), f"job {j}"
    assert rows[-1].data_ptr() == rows[1].data_ptr() + 4 * n * width
    assert rows[-1].untyped_storage().data_ptr() == rows[1].untyped_storage().data_ptr()
    assert outs[1].data_ptr() == outs[0].data_ptr() + 4 * n * 2 * R.W
    assert outs[1].untyped_storage().data_ptr() == outs[0].untyped_storage().data_ptr()
    # ... and against float64 on the gathered rows, under the rule
    c = R.time_case(0)
    figures = []
    for j, (_, d) in enumerate(plan[:3]):
        t_np = ic.table[R.gather_index(ic.ts, d)]
        want = R.time_bias(c.ws, c.bs, c.in_xyz, t_np, np.float64)
        d32 = float(R.row_errors(R.time_bias(c.ws, c.bs, c.in_xyz, t_np, np.float32), want).max())
        figures.append((f"delta {d}", float(R.row_errors(outs[j].cpu().numpy(), want).max()), R.bound(d32), d32))
    _report("time_bias index mode", figures)
    # the same launch through the structures: every output with a NaN tail; the coarse job leaves no rows behind
    direct = launch_time_bias([(mod, (E, ts, R.MAX_T, d, j < 3)) for j, (mod, d) in enumerate(plan)], n)
    for j, ((got, got_rows), (_, d)) in enumerate(zip(direct, plan)):
        assert same_bits(got, outs[j].cpu().numpy()), f"job {j}"
        assert (got_rows is None) == (j == 3)
        if got_rows is not None:
            assert same_bits(got_rows, want_rows[d].cpu().numpy()), f"rows of job {j}"


# ---- nsff_side_bias ----
@gpu
@pytest.mark.parametrize("model_index", range(len(R.SIDE_MODELS)))
def test_side_bias_against_float64(hip_lib, model_index):
    c = R.side_case(model_index)
    m = R.make_side_model(model_index).to(DEV)
    desc = _lib.model_desc(m)
    assert (desc.in_dir, desc.in_a, desc.use_viewdir) == (c.in_dir, c.in_a, 1)
    packed = m.packed(config.PRECISIONS["f16x3"])                               # (the folded bias row lives in the inference pack)
    w = m.static_dir_encoding[0].weight.detach()
    dirs, a_rows = _dev(c.dirs), None if c.a_rows is None else _dev(c.a_rows)

    def launch(lo, hi):
        n = hi - lo
        out = _nan(n, R.W)
        rc = _lib.load().nsff_side_bias(C.byref(desc), _lib._ptr(packed), _lib._ptr(w), _lib._ptr(dirs[lo:hi].contiguous()),
                                        None if a_rows is None else _lib._ptr(a_rows[lo:hi].contiguous()), n, _lib._ptr(out), _stream())
        assert rc == OK
        torch.cuda.synchronize()
        return owned(out, n, f"{n} rays")
    rows, batch = [], None
    for n in R.RAY_COUNTS:
        got = launch(0, n)
        rows.append((f"{n} rays", float(R.row_errors(got, c.want[:n]).max()), R.bound(c.d32[n]), c.d32[n]))
        if n == 17:
            batch = got
    _report(f"side_bias (in_dir, in_a) = {R.SIDE_MODELS[model_index]}", rows)
    for r in range(17):
        assert same_bits(launch(r, r + 1)[0], batch[r]), f"ray {r} alone differs from the batch"


# ---- nsff_field_input_backward ----
def default_geometry():
    """what nsff_train_dims reports for the default NSFF model (8 layers, skip 4, 10 frequencies, 48 time-code columns)"""
    xr, t0, _ = _lib.train_dims(A.NeRF("fine", use_viewdir=False, encode_transient=True, in_channels_t=48, output_flow=True))
    return (xr, t0, 48, 10, True)


def launch_input_backward(c, d_xin, xyz, want_xyz, want_t):
    d_xyz = _nan(c.P, 3) if want_xyz else None
    d_t = _nan(c.n_rays, c.in_t) if want_t else None
    f = (C.c_float * max(len(c.freqs), 1))(*[float(v) for v in c.freqs])
    rc = _lib.load().nsff_field_input_backward(_lib._ptr(d_xin), c.xin_rows, c.t0, _lib._ptr(xyz), c.n_rays, c.S, f, len(c.freqs),
                                               c.in_t, _lib._ptr(d_xyz), _lib._ptr(d_t), _stream())
    assert rc == OK
    torch.cuda.synchronize()
    return (owned(d_xyz, c.P, f"d_xyz {c.n_rays} x {c.S}") if want_xyz else None,
            owned(d_t, c.n_rays, f"d_t {c.n_rays} x {c.S}") if want_t else None)


@gpu
@pytest.mark.parametrize("geometry", list(range(len(R.GEOMETRIES))) + ["default"])
def test_field_input_backward_against_float64(hip_lib, geometry):
    """d_xyz inside the bound relative to the sum of the absolute terms, d_t with the sequential fp32 sum's bits, NaN in every
    column the operation does not read, NaN tails behind both outputs, the same bits whichever outputs are asked for"""
    geo = default_geometry() if geometry == "default" else R.GEOMETRIES[geometry]
    assert geometry != "default" or geo[:2] == (128, 64)
    rows = []
    for key in R.input_keys((geo,)):
        c = R.input_case(*key)
        d_xin, xyz = _dev(c.d_xin), _dev(c.xyz)
        assert bool(torch.isnan(d_xin).any()) and d_xin.shape == (c.P, c.xin_rows)
        got_xyz, got_t = launch_input_backward(c, d_xin, xyz, True, True)
        what = f"{c.n_rays} rays x {c.S}"
        rows.append((what, float(R.element_errors(got_xyz, c.want_xyz, c.M).max()), R.bound(c.d32_xyz), c.d32_xyz))
        assert same_bits(got_t, c.twin_t), f"{what}: d_t is not the sequential fp32 sum"
        only_xyz, none_t = launch_input_backward(c, d_xin, xyz, True, False)
        none_xyz, only_t = launch_input_backward(c, d_xin, xyz, False, True)
        assert none_t is None and none_xyz is None
        assert same_bits(only_xyz, got_xyz) and same_bits(only_t, got_t), what
    _report(f"field_input_backward {geo}", rows)
