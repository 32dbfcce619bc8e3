"""The small fp32 kernels between the pieces of the training step, called directly through the C ABI: `nsff_time_rows` and
`nsff_time_rows_backward` (csrc/rays.hip), `nsff_flow_grad` (csrc/rays_bwd.hip), `nsff_fold_grads`, `nsff_fold_grads_dense` and
`nsff_absmax` (csrc/field_bwd.hip), against the float64 expressions of tests/grad_glue_ref.py on that module's cases.

The cases are integer-valued and small enough that fp32 arithmetic is exact in any order (grad_glue_ref.py), so every comparison
is EQUALITY with the float64 reference -- no tolerance -- at the shapes where these kernels change route: ray counts on both sides
of the 2048-ray compaction pass, lists of exactly 2048 entries, list lengths on both sides of the sixteen-row step, widths on both
sides of the 64-column register and the 256-column group, one to 256 folded rows on both sides of the four-row workgroup, row
strides that differ between input and output, every 4-byte alignment of W_final, point counts on both sides of a 256-thread block.
The one real-valued case (time rows, 4097 rays x 300 columns) is held to the project's rule max(8 d32, 16 x 2^-24) with d32 the
distance of a sequential CPU fp32 sum from float64.  The CPU tests show that every planted defect changes the reference of a
named case, that every case reaches the route it is named for, and the refusals that need no launch.  Figures: EXPERIMENTS.md R19.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_glue_ref as R
import nsff_pl_amd as A
from nsff_pl_amd import _lib, field_grad

DEV = "cuda:0"
TAIL = 64                                     # floats behind every output buffer that must stay untouched
NAN = float("nan")
OK, INVALID, NULL, ALIGN = 0, -1, -2, -3      # NSFF_* of include/nsff_render.h
FAKE = 4096                                   # a 16-byte aligned non-null "pointer" for calls that are refused before any launch
ULP = 2.0 ** -24
gpu = pytest.mark.gpu


# =====================================================================================================================
# CPU: exactness, routes, planted defects, refusals
# =====================================================================================================================
def test_every_case_is_exact_in_fp32():
    """the sum of the absolute terms of every output element of every case is below 2^24, and the reference is an fp32 array"""
    worst = {}
    for name in R.TIME_CASES:
        c = R.time_case(name)
        worst["time " + name] = c.abs_terms
        R.to_f32(c.want)
    for P in R.FLOW_P:
        for form in range(len(R.FLOW_FORMS)):
            c = R.flow_case(P, form)
            worst[f"flow {P} {form}"] = c.abs_terms
            R.to_f32(c.want)
    for Rr in sorted(set(R.HEADS_R + R.DENSE_R)):
        c = R.fold_case(Rr)
        worst[f"fold {Rr}"] = c.abs_terms
        for part in R.fold_dense(c, 256, 256, True, True):
            R.to_f32(part)
    assert max(worst.values()) < R.EXACT, {k: v for k, v in worst.items() if v >= R.EXACT}
    print("R19 largest sum of absolute terms:", max(worst, key=worst.get), max(worst.values()), "of", R.EXACT)


def test_the_reference_is_the_plain_loop():
    """the one-hot product of the reference against a ray-by-ray loop (exact on integers, so the fp32 loop must agree)"""
    for name in ("n64_w63_cropped", "n65_w257", "list_tails", "one_row_table", "sparse_frames"):
        c = R.time_case(name)
        loop = R.time_rows_backward_f32(c.gs, c.ts, c.n_table, c.max_t, c.width)
        assert np.array_equal(loop.astype(np.float64), c.want), name


def test_the_time_row_cases_reach_their_routes():
    rt = {name: R.time_case(name).routes for name in R.TIME_CASES}
    case = R.time_case
    assert 18 <= len(R.TIME_CASES) <= 24
    # every value of every axis
    assert {case(n).n for n in rt} == {0, 1, 63, 64, 65, 2047, 2048, 2049, 4097}
    assert {case(n).width for n in rt} == {1, 3, 48, 63, 64, 65, 128, 256, 257, 300}
    assert {case(n).n_table for n in rt} == {1, 2, 12, 30}
    kinds = set()
    for n in rt:
        c = case(n)
        kinds |= {k for k, v in (("zero", 0), ("cropped", c.n_table - 4), ("last", c.n_table - 1), ("past", c.n_table + 5)) if c.max_t == v}
    assert kinds == {"zero", "cropped", "last", "past"}
    # each of the seven non-empty subsets of (cur, next, prev)
    assert {case(n).present for n in rt} == {tuple(bool(b >> k & 1) for k in range(3)) for b in range(1, 8)}
    # passes, lists, column groups
    assert rt["no_rays"].passes == 0 and rt["no_rays"].lists == 0 and len(rt["no_rays"].unhit) == 12
    assert rt["n2047_w48"].passes == 1 and rt["full_list"].passes == 1
    assert rt["full_list"].fullest == R.CHUNK and rt["full_list"].lists == 3 and rt["full_list"].unhit == [0, 1, 2, 3, 7, 8, 9, 10, 11]
    assert rt["n2049_w128_cur"].passes == 2 and rt["n2049_w256"].passes == 2 and rt["one_row_table"].passes == 2
    lp = R.hit_lists(case("last_pass_one_ray").ts, 12, 11, (1, 1, 1))
    assert rt["last_pass_one_ray"].passes == 3 and rt["last_pass_one_ray"].fullest == R.CHUNK
    assert sorted(len(v) for k, v in lp.items() if k[1] == 2) == [1, 1, 1] and sorted(k[2] for k in lp if k[1] == 2) == [10, 11, 11]
    assert lp[(0, 2, 11)][0] == 4096 and len(lp[(1, 2, 11)]) == 1 and (2, 2, 10) in lp        # cur and next on 11, prev on 10
    assert rt["n4097_w300"].passes == 3 and rt["n4097_w300"].groups == 2 and rt["n4097_w300"].registers == 4
    assert rt["n65_w257"].groups == 2 and rt["n2049_w256"].groups == 1 and rt["n2049_w256"].registers == 4 and rt["n1_w300"].groups == 2
    assert rt["n65_w65_past_end"].registers == 2 and rt["n65_w64_max_t_0"].registers == 1 and rt["n2049_w128_cur"].registers == 2
    assert {1, 5, 15, 0} <= rt["list_tails"].mods and rt["list_tails"].lists == 4 and rt["list_tails"].fullest == 31
    assert rt["sparse_frames"].unhit == [0, 1] + list(range(5, 30)) and rt["n65_w64_max_t_0"].unhit == list(range(1, 12))
    # frame indices outside the table, on both sides
    for n in ("n64_w63_cropped", "n2049_w128_cur", "n4097_w300", "list_tails", "one_row_table", "n65_w65_past_end"):
        c = case(n)
        assert -3 in c.ts and c.n_table + 10 in c.ts, n


def test_every_planted_defect_is_noticed_by_a_named_case():
    """the float64 reference of each named case changes under its defect: a kernel with that defect cannot equal it"""
    assert set(R.TIME_DEFECT_CASES) == set(R.TIME_DEFECTS)
    for defect, names in R.TIME_DEFECT_CASES.items():
        for name in names:
            c = R.time_case(name)
            bad = R.time_rows_backward(c.gs, c.ts, c.n_table, c.max_t, c.width, defect)
            assert not np.array_equal(bad, c.want), (defect, name)
    # a defect off its route changes nothing: the cases above are not noticed by accident
    c = R.time_case("n2047_w48")
    for defect in ("chunk_carry", "drop_entry_2047", "col_group", "col_register", "clamp_table_end"):
        assert np.array_equal(R.time_rows_backward(c.gs, c.ts, c.n_table, c.max_t, c.width, defect), c.want), defect
    # flow glue: on every point count of the form that has four cotangents in group a and both groups
    assert set(R.FLOW_DEFECT_FORMS) == set(R.FLOW_DEFECTS)
    for defect, form in R.FLOW_DEFECT_FORMS.items():
        for P in R.FLOW_P:
            c = R.flow_case(P, form)
            bad = R.flow_grad(c.zs, R.Z_FAR, c.prior, c.accumulate, c.col_a, c.g_a, c.col_b, c.g_b, defect)
            changed = not np.array_equal(bad, c.want)
            if defect == "mask_ge":                      # (shows at the point whose depth is exactly z_far)
                assert changed == bool(np.abs(c.want[c.at_far]).max() > 0), (defect, P)
                assert c.zs[c.at_far] == np.float32(R.Z_FAR)
            else:
                assert changed, (defect, P)
    assert any(np.abs(R.flow_case(P, 0).want[R.flow_case(P, 0).at_far]).max() > 0 for P in R.FLOW_P)
    for P in R.FLOW_P[1:]:                               # exactly at z_far and NaN: kept; one fp32 step above: dropped
        c = R.flow_case(P, 6)
        assert np.abs(c.want[c.at_far]).max() > 0 and np.abs(c.want[c.nan]).max() > 0 and np.abs(c.want[c.above]).max() == 0
    # fold
    for Rr in R.DENSE_R:
        c = R.fold_case(Rr)
        good = R.fold_dense(c, 331, 256, True, True)
        for defect in ("no_remainder_rows", "no_bias_term"):
            bad = R.fold_dense(c, 331, 256, True, True, defect)
            assert not np.array_equal(bad[0], good[0]), (defect, Rr)
        tail = R.fold_dense(c, 331, 256, True, True, "row_tail")
        assert (not np.array_equal(tail[0], good[0])) == (Rr % R.FOLD_ROWS != 0), Rr
        mix = R.fold_dense(c, 331, 256, True, True, "ld_mixup")
        assert (not np.array_equal(mix[0], good[0])) == (Rr > 1), Rr
        assert np.array_equal(R.fold_dense(c, 283, 283, True, True, "ld_mixup")[0], R.fold_dense(c, 283, 283, True, True)[0])
    assert {Rr % R.FOLD_ROWS for Rr in R.DENSE_R} == {0, 1, 2, 3}


def test_the_real_valued_case_and_its_twin():
    """d32 of the sequential fp32 sum on the real-valued time-row case, in units of 2^-24 (EXPERIMENTS.md R19): about 340 terms per
    table row and gather"""
    c = R.real_time_case()
    rt = R.time_routes(c.ts, c.width, c.n_table, c.max_t, (1, 1, 1))
    assert rt.passes == 3 and rt.groups == 2 and not rt.unhit
    print("R19 real-valued case: d32 =", c.d32 / ULP, "x 2^-24, bound", R.bound(c.d32) / ULP)
    assert round(c.d32 / ULP, 1) == 21.2 and R.bound(c.d32) == R.FACTOR * c.d32
    assert R.row_errors(c.want.astype(np.float32), c.want).max() <= R.FLOOR


def test_refusals_that_need_no_launch(hip_lib):
    lib = hip_lib

    def trb(g=FAKE, ts=FAKE, n=4, max_t=11, n_table=12, width=48, d=FAKE):
        return lib.nsff_time_rows_backward(g, g, g, ts, n, max_t, n_table, width, d, None)
    assert trb(n=-1) == INVALID and trb(n_table=0) == INVALID and trb(width=0) == INVALID
    assert trb(d=None) == NULL and trb(ts=None) == NULL

    def tr(table=FAKE, n_table=12, width=48, ts=FAKE, n=4, nxt=FAKE, prv=FAKE):
        return lib.nsff_time_rows(table, n_table, width, ts, n, 11, nxt, prv, None)
    assert tr(n=-1) == INVALID and tr(n_table=0) == INVALID and tr(width=0) == INVALID
    assert tr(n=0, ts=None, table=None) == OK                                  # no rays: nothing launched, nothing read
    assert tr(nxt=None, prv=None) == OK                                        # nothing wanted
    assert tr(table=None) == NULL and tr(ts=None) == NULL

    def fg(n_points=4, col_a=8, col_b=11, zs=FAKE, out=FAKE):
        a = _lib.FlowGradArgs(n_points=n_points, zs=zs, z_far=0.95, accumulate=0, col_a=col_a, col_b=col_b, out=out)
        return lib.nsff_flow_grad(C.byref(a), None)
    assert fg(col_a=14) == INVALID and fg(col_b=14) == INVALID and fg(col_a=-1, col_b=-1) == INVALID
    assert fg(col_a=8, col_b=10) == INVALID and fg(col_a=8, col_b=6) == INVALID and fg(col_a=8, col_b=8) == INVALID   # overlapping
    assert fg(n_points=-1) == INVALID
    assert fg(out=FAKE + 4) == ALIGN and fg(out=FAKE + 8) == ALIGN
    assert fg(n_points=0, zs=None, out=None) == OK                             # (checked before the null checks)
    assert fg(zs=None) == NULL and fg(out=None) == NULL
    assert lib.nsff_flow_grad(None, None) == NULL

    def heads(n_rows, missing=None):
        a = _lib.FoldGradArgs(n_rows=n_rows, g=FAKE, gb=FAKE, w_final=FAKE, b_final=FAKE, d_w_final=FAKE, d_b_final=FAKE)
        for r in range(16):
            a.w_head[r] = a.d_w_head[r] = a.d_b_head[r] = FAKE
        if missing is not None:
            getattr(a, missing[0])[missing[1]] = None
        return lib.nsff_fold_grads(C.byref(a), None)
    assert heads(0) == INVALID and heads(17) == INVALID and heads(-1) == INVALID
    assert heads(10, ("w_head", 9)) == NULL and heads(10, ("d_w_head", 0)) == NULL and heads(16, ("d_b_head", 15)) == NULL
    assert lib.nsff_fold_grads(None, None) == NULL

    def dense(n_rows=10, ld_head=283, ld_dhead=283, **null):
        ptrs = {k: FAKE for k in ("g", "gb", "w_head", "w_final", "b_final", "d_w_head", "d_b_head", "d_w_final", "d_b_final")}
        ptrs.update(null)
        a = _lib.FoldDenseArgs(n_rows=n_rows, accumulate=0, ld_head=ld_head, ld_dhead=ld_dhead, **ptrs)
        return lib.nsff_fold_grads_dense(C.byref(a), None)
    assert dense(n_rows=0) == INVALID and dense(n_rows=257) == INVALID
    assert dense(ld_head=255) == INVALID and dense(ld_dhead=255) == INVALID
    assert dense(w_final=None) == NULL and dense(d_b_head=None) == NULL
    assert lib.nsff_fold_grads_dense(None, None) == NULL

    assert lib.nsff_absmax(FAKE, -1, FAKE, None) == INVALID
    assert lib.nsff_absmax(FAKE + 4, 8, FAKE, None) == ALIGN and lib.nsff_absmax(FAKE + 8, 8, FAKE, None) == ALIGN
    assert lib.nsff_absmax(FAKE, 8, None, None) == NULL and lib.nsff_absmax(None, 8, FAKE, None) == NULL


# =====================================================================================================================
# GPU
# =====================================================================================================================
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.tensor(np.asarray(a)).to(DEV).contiguous()


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class Buf:
    """A device buffer a kernel writes: `init` (any shape, fp32) laid out flat `off` floats behind a 16-byte boundary, NaN before
    it and TAIL NaN floats behind it that must come back untouched."""

    def __init__(self, init, off=0):
        init = np.ascontiguousarray(init, np.float32)
        self.shape, self.n, self.off = init.shape, init.size, off
        self.t = torch.full((off + self.n + TAIL,), NAN, device=DEV)
        assert self.t.data_ptr() % 16 == 0
        if self.n:
            self.t[off:off + self.n] = _dev(init.reshape(-1))
        self.ptr = self.t.data_ptr() + 4 * off

    def read(self, what):
        host = self.t.cpu().numpy()
        guard = np.concatenate([host[:self.off], host[self.off + self.n:]])
        assert np.isnan(guard).all() and guard.size == self.off + TAIL, (what, "floats outside the call's were written")
        return host[self.off:self.off + self.n].reshape(self.shape)


def nans(*shape):
    return np.full(shape, np.nan, np.float32)


def same(got, want64, what):
    """EQUALITY with the float64 reference (cast to fp32, which is exact for these cases), NaN where the reference keeps NaN"""
    want = R.to_f32(want64)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want, equal_nan=True):
        diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {got.size} elements differ, the first at {at}: {got[at]} for {want[at]}")


# ---- 1. nsff_time_rows_backward, exactly ----
def launch_time_rows_backward(gs, ts, n, max_t, n_table, width, what):
    out = Buf(nans(n_table, width))
    rc = _lib.load().nsff_time_rows_backward(_ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(ts), n, max_t, n_table, width, out.ptr, _stream())
    assert rc == OK, what
    torch.cuda.synchronize()
    return out.read(what)


@gpu
@pytest.mark.parametrize("name", list(R.TIME_CASES))
def test_time_rows_backward_equals_float64(hip_lib, name):
    """every row of d_table -- the rows no ray hits as zeros -- equal to the float64 sum, the NaN tail behind the table untouched,
    and a second call on the same inputs with the same bits"""
    c = R.time_case(name)
    gs = [None if g is None else _dev(g) for g in c.gs]
    ts = _dev(c.ts) if c.n else None                                           # (no rays: a null ts is taken)
    got = launch_time_rows_backward(gs, ts, c.n, c.max_t, c.n_table, c.width, name)
    same(got, c.want, name)
    for r in c.routes.unhit:
        assert not got[r].any(), (name, r)
    again = launch_time_rows_backward(gs, ts, c.n, c.max_t, c.n_table, c.width, name)
    assert np.array_equal(bits(got), bits(again)), name


# ---- 2. nsff_time_rows_backward on real values ----
@gpu
def test_time_rows_backward_real_values_against_float64(hip_lib):
    """standard-normal cotangents, 4097 rays x 300 columns x 12 frames: per table row, the largest error over the row's columns over
    the row's largest |reference| is at most max(8 d32, 16 x 2^-24), d32 the same figure of a sequential CPU fp32 sum in ray order"""
    c = R.real_time_case()
    gs = [_dev(g) for g in c.gs]
    got = launch_time_rows_backward(gs, _dev(c.ts), c.n, c.max_t, c.n_table, c.width, "real")
    err = R.row_errors(got, c.want)
    print(f"R19 real-valued time rows: kernel error {err.max() / ULP:.3g}, twin d32 {c.d32 / ULP:.3g}, bound {R.bound(c.d32) / ULP:.3g} "
          f"(x 2^-24); per row {[round(float(e) / ULP, 2) for e in err]}")
    assert err.max() <= R.bound(c.d32), (err.max() / ULP, R.bound(c.d32) / ULP)


# ---- 3. nsff_time_rows ----
@gpu
@pytest.mark.parametrize("width", R.ROWS_WIDTHS)
def test_time_rows_gathers_are_table_rows(hip_lib, width):
    """next / prev equal to table[index] bit for bit with the table and either output at 0 and at 4 bytes past a 16-byte boundary
    (the vector route needs width % 4 == 0 AND all three aligned), only next, only prev and both"""
    lib = _lib.load()
    for n in R.ROWS_N:
        c = R.rows_case(n, width)
        ts = _dev(c.ts) if n else None
        for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            table = Buf(c.table, offs[0])
            for want_next, want_prev in ((1, 1), (1, 0), (0, 1)):
                what = (n, width, offs, want_next, want_prev)
                nxt, prv = Buf(nans(n, width), offs[1]), Buf(nans(n, width), offs[2])
                rc = lib.nsff_time_rows(table.ptr, c.n_table, width, _ptr(ts), n, c.max_t, nxt.ptr if want_next else None,
                                        prv.ptr if want_prev else None, _stream())
                assert rc == OK, what
                torch.cuda.synchronize()
                for buf, wanted, ref in ((nxt, want_next, c.next), (prv, want_prev, c.prev)):
                    got = buf.read(what)
                    if wanted:
                        assert np.array_equal(bits(got), bits(ref)), what
                    else:
                        assert np.isnan(got).all(), what
            assert np.array_equal(bits(table.read("table")), bits(c.table))


@gpu
def test_time_rows_wrapper_with_prev_off_alignment(hip_lib):
    """_lib.time_rows puts prev n x width floats behind next in one buffer: at (3, 50) that is 8 bytes past a 16-byte boundary"""
    c = R.rows_case(257, 50)
    table, ts = _dev(c.table), _dev(c.ts[:3])
    nxt, prv = _lib.time_rows(table, ts, c.max_t)
    torch.cuda.synchronize()
    assert prv.data_ptr() == nxt.data_ptr() + 4 * 3 * 50 and prv.data_ptr() % 16 != 0
    assert np.array_equal(bits(nxt.cpu().numpy()), bits(c.next[:3])) and np.array_equal(bits(prv.cpu().numpy()), bits(c.prev[:3]))


# ---- 4. nsff_flow_grad ----
@gpu
@pytest.mark.parametrize("P", R.FLOW_P)
def test_flow_grad_equals_float64(hip_lib, P):
    """every form: store onto a NaN-filled record (all 16 columns defined afterwards), accumulate onto integer records (every
    column outside the named groups keeps its bits); depths exactly at z_far and NaN keep the point, one fp32 step above drops it"""
    for form in range(len(R.FLOW_FORMS)):
        c = R.flow_case(P, form)
        what = (P, R.FLOW_FORMS[form])
        out = Buf(c.prior if c.accumulate else nans(P, 16))
        keep = [_dev(g) for g in c.g_a + c.g_b]
        zs = _dev(c.zs)
        a = _lib.FlowGradArgs(n_points=P, zs=zs.data_ptr(), z_far=R.Z_FAR, accumulate=int(c.accumulate), col_a=c.col_a,
                              col_b=c.col_b, out=out.ptr)
        for k in range(len(c.g_a)):
            a.g_a[k] = keep[k].data_ptr()
        for k in range(len(c.g_b)):
            a.g_b[k] = keep[len(c.g_a) + k].data_ptr()
        assert _lib.load().nsff_flow_grad(C.byref(a), _stream()) == OK, what
        torch.cuda.synchronize()
        got = out.read(what)
        same(got, c.want, what)
        if c.accumulate:
            named = [col + k for col in (c.col_a, c.col_b) if col >= 0 for k in range(3)]
            others = [k for k in range(16) if k not in named]
            assert np.array_equal(bits(got[:, others]), bits(c.prior[:, others])), what


# ---- 5. nsff_fold_grads ----
@gpu
@pytest.mark.parametrize("Rr", R.HEADS_R)
def test_fold_grads_equals_float64(hip_lib, Rr):
    """the heads' rows in separate tensors as field_grad._fold_in_place passes them, non-zero integer gradients already in every
    d_*, non-zero remainder rows 16 + r, NaN in rows R..15 and 16 + R..31 of the job"""
    c = R.fold_case(Rr)
    g32, gb32, want = R.fold_heads(c)
    assert np.isnan(g32).any() == (Rr < 16)
    g, gb, w_final, b_final = _dev(g32), _dev(gb32), _dev(c.w_final), _dev(c.b_final)
    a = _lib.FoldGradArgs(n_rows=Rr, g=g.data_ptr(), gb=gb.data_ptr(), w_final=w_final.data_ptr(), b_final=b_final.data_ptr())
    d_w_final, d_b_final = Buf(c.prior_w_final), Buf(c.prior_b_final)
    a.d_w_final, a.d_b_final = d_w_final.ptr, d_b_final.ptr
    heads, r0 = [], 0
    for k in R.head_split(Rr):
        w = _dev(c.w_head[r0:r0 + k, :256])
        dw, db = Buf(c.prior_w_head[r0:r0 + k, :256]), Buf(c.prior_b_head[r0:r0 + k])
        for j in range(k):
            a.w_head[r0 + j], a.d_w_head[r0 + j], a.d_b_head[r0 + j] = w.data_ptr() + 1024 * j, dw.ptr + 1024 * j, db.ptr + 4 * j
        heads.append((r0, k, w, dw, db))
        r0 += k
    assert _lib.load().nsff_fold_grads(C.byref(a), _stream()) == OK
    torch.cuda.synchronize()
    for r0, k, _, dw, db in heads:
        same(dw.read("d_w_head"), want[0][r0:r0 + k], (Rr, "d_w_head", r0))
        same(db.read("d_b_head"), want[1][r0:r0 + k], (Rr, "d_b_head", r0))
    same(d_w_final.read("d_w_final"), want[2], (Rr, "d_w_final"))
    same(d_b_final.read("d_b_final"), want[3], (Rr, "d_b_final"))


# ---- 6. nsff_fold_grads_dense ----
@gpu
@pytest.mark.parametrize("Rr", R.DENSE_R)
def test_fold_grads_dense_equals_float64(hip_lib, Rr):
    """row strides (ld_head, ld_dhead) equal and different, with and without the remainder summands, storing onto NaN and adding
    onto integers, W_final at 0, 4, 8 and 12 bytes past a 16-byte boundary: equal to float64 -- so the same bits at all four --,
    the floats between the rows of d_w_head and behind every output untouched"""
    c = R.fold_case(Rr)
    g, g2, gb, gb2, b_final = (_dev(v) for v in (c.g, c.g2, c.gb, c.gb2, c.b_final))
    w_finals = [Buf(c.w_final, off) for off in range(4)]
    assert [w.ptr % 16 for w in w_finals] == [0, 4, 8, 12]
    for ld_head, ld_dhead in R.DENSE_LDS:
        w_head = _dev(np.ascontiguousarray(c.w_head[:, :ld_head]))
        size = (Rr - 1) * ld_dhead + 256
        for with_g2 in (True, False):
            for accumulate in (0, 1):
                want = R.fold_dense(c, ld_head, ld_dhead, with_g2, bool(accumulate))
                first = None
                for w_final in w_finals:
                    what = (Rr, ld_head, ld_dhead, with_g2, accumulate, w_final.off)
                    if accumulate:
                        outs = [Buf(np.ascontiguousarray(c.prior_w_head[:, :ld_dhead]).reshape(-1)[:size]), Buf(c.prior_b_head),
                                Buf(c.prior_w_final), Buf(c.prior_b_final)]
                    else:
                        outs = [Buf(nans(size)), Buf(nans(Rr)), Buf(nans(256, 256)), Buf(nans(256))]
                    a = _lib.FoldDenseArgs(n_rows=Rr, accumulate=accumulate, ld_head=ld_head, ld_dhead=ld_dhead, g=g.data_ptr(),
                                           g2=g2.data_ptr() if with_g2 else None, gb=gb.data_ptr(), gb2=gb2.data_ptr() if with_g2 else None,
                                           w_head=w_head.data_ptr(), w_final=w_final.ptr, b_final=b_final.data_ptr(),
                                           d_w_head=outs[0].ptr, d_b_head=outs[1].ptr, d_w_final=outs[2].ptr, d_b_final=outs[3].ptr)
                    assert _lib.load().nsff_fold_grads_dense(C.byref(a), _stream()) == OK, what
                    torch.cuda.synchronize()
                    got = [o.read(what) for o in outs]
                    for part, w, n in zip(got, want, ("d_w_head", "d_b_head", "d_w_final", "d_b_final")):
                        same(part, w, what + (n,))
                    if first is None:
                        first = got
                    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(got, first)), what
    for w in w_finals:
        assert np.array_equal(bits(w.read("w_final")), bits(c.w_final))


# ---- 7. nsff_absmax ----
@gpu
@pytest.mark.parametrize("n", R.ABSMAX_N)
def test_absmax_equals_numpy(hip_lib, n):
    for plant in R.ABSMAX_PLANTS:
        c = R.absmax_case(n, plant)
        x = _dev(c.x) if n else None
        out = Buf(nans(1))
        assert _lib.load().nsff_absmax(_ptr(x), n, out.ptr, _stream()) == OK, (n, plant)
        torch.cuda.synchronize()
        got = out.read((n, plant))
        assert np.array_equal(bits(got), bits(np.asarray([c.want]))), (n, plant, got, c.want)
        assert c.want == (np.float32(5.5) if n else np.float32(0.0))


# ---- 8. parameters off alignment, through the real node ----
def _packed_model(viewdir, offset, with_grads):
    """the model with every parameter (and, with_grads, its zeroed .grad) a view of ONE flat buffer packed without padding from
    `offset` floats behind the buffer's start"""
    torch.manual_seed(4100)
    m = A.NeRF("fine", use_viewdir=viewdir, encode_appearance=viewdir, in_channels_a=48 if viewdir else 0, encode_transient=True,
               in_channels_t=48, output_flow=True).to(DEV)
    params = list(m.parameters())
    total = sum(p.numel() for p in params)
    flat = torch.zeros(total + offset + TAIL, device=DEV)
    gflat = torch.zeros(total + offset + TAIL, device=DEV)
    assert flat.data_ptr() % 16 == 0 and gflat.data_ptr() % 16 == 0
    at = offset
    with torch.no_grad():
        for p in params:
            k = p.numel()
            flat[at:at + k] = p.data.reshape(-1)
            p.data = flat[at:at + k].view(p.shape)
            p.grad = gflat[at:at + k].view(p.shape) if with_grads else None
            at += k
    return m, (flat, gflat)


@gpu
@pytest.mark.parametrize("deferred", [True, False], ids=["in_place", "returned"])
@pytest.mark.parametrize("viewdir", [False, True], ids=["default", "viewdir"])
def test_field_node_with_parameters_at_any_alignment(hip_lib, viewdir, deferred):
    """One forward + backward of field_grad.field at 128 rays x 3 points, both trunks and the dynamic trunk alone (the only form with
    d_xyz), with the parameters packed from offset 0 and from offset 1 float -- every tensor 4 bytes further on, so W_final of both
    trunks leaves its 16-byte alignment: every parameter gradient, d_xyz and d_t have the same bits in the two packings."""
    g = torch.Generator().manual_seed(4101)
    n_rays, s = 128, 3
    xyz = (torch.rand(n_rays * s, 3, generator=g) * 2 - 1).to(DEV)
    t_rows = torch.randn(n_rays, 48, generator=g).to(DEV)
    dir_rows, a_rows = torch.randn(n_rays, 27, generator=g).to(DEV), torch.randn(n_rays, 48, generator=g).to(DEV)
    cot = torch.randn(n_rays * s, 16, generator=g).to(DEV)
    freqs = [float(f) for f in A.PosEmbedding(9, 10).freqs]

    def run(offset, static):
        field_grad._GRAD_MAPS.clear()
        m, keep = _packed_model(viewdir, offset, deferred)
        x = xyz.clone().requires_grad_(not static)
        t = t_rows.clone().requires_grad_(True)
        side = dict(dir_rows=dir_rows, a_rows=a_rows) if (viewdir and static) else {}
        if deferred:
            with field_grad.deferred_weight_grads():
                field_grad.field(m, x, freqs, t, s, static, True, **side).backward(cot)
        else:
            field_grad.field(m, x, freqs, t, s, static, True, **side).backward(cot)
        torch.cuda.synchronize()
        assert not field_grad._PENDING and bool(field_grad._GRAD_MAPS) == deferred
        grads = {n: None if p.grad is None else p.grad.detach().clone() for n, p in m.named_parameters()}
        offsets = {n: p.data_ptr() % 16 for n, p in m.named_parameters()}
        return grads, x.grad, t.grad, offsets

    for static in (True, False):
        g0, dx0, dt0, at0 = run(0, static)
        g1, dx1, dt1, at1 = run(1, static)
        for n in ("static_xyz_encoding_final.weight", "transient_xyz_encoding_final.weight"):
            assert at0[n] == 0 and at1[n] == 4, (n, at0[n], at1[n])
        used = 0
        for n in g0:
            if g0[n] is None or g1[n] is None:
                assert g0[n] is None and g1[n] is None and n.startswith("static") and not static, n
                continue
            assert bool(g0[n].isfinite().all()), n
            assert torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32)), (static, n)
            used += int(float(g0[n].abs().max()) > 0)
        assert used >= (40 if static else 22), used
        assert torch.equal(dt0.view(torch.int32), dt1.view(torch.int32)) and float(dt0.abs().max()) > 0
        if static:
            assert dx0 is None and dx1 is None
        else:
            assert torch.equal(dx0.view(torch.int32), dx1.view(torch.int32)) and float(dx0.abs().max()) > 0
