"""The split-K weight-gradient path of csrc/field_bwd.hip called directly -- nsff_wgrad_kernel (one product and X3, 256 x 256 and
256 x 128), nsff_wgrad_head_kernel, nsff_wgrad_reduce_kernel, nsff_wgrad_accumulate_kernel, the host-side wgrad_plan -- and
nsff_absmax_raw, on inputs for which fp32 arithmetic is exact (tests/wgrad_numpy.py): the result must be EQUAL to a float64
`A.T @ B`, divided by the power-of-two scales.  No tolerance anywhere in this file.

The CPU tests prove that the inputs can tell: the reference with a planted defect (a k-step dropped or doubled, a split boundary
moved, two jobs mixed up, a head row on the trunk's scale, a job_b term omitted) differs from the true one in every case, and every
case reaches the kernel route it is named for."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_numpy as W
from wgrad_numpy import Case, Job

# ---- the cases -----------------------------------------------------------------------------------------------------------
ONE_EACH_A = (Job(256, 256, 0), Job(256, 128, 1), Job(32, 256, 0))
ONE_EACH_B = (Job(32, 256, 1), Job(256, 256, 1), Job(256, 128, 0))
# 18 jobs 256 x 256, 4 jobs 256 x 128, 2 head jobs (24 of MAX_WJOBS = 48), the classes interleaved so that a job's index in the
# call is not its index in its class's launch
MULTI = ((Job(32, 256, 0),) + tuple(Job(256, 256, j & 1) for j in range(9)) + (Job(256, 128, 0), Job(256, 128, 0))
         + tuple(Job(256, 256, j & 1) for j in range(9, 18)) + (Job(32, 256, 1), Job(256, 128, 1), Job(256, 128, 1)))
MAX_TILES = 30

GEMM_CASES = {
    "tiny": Case(ONE_EACH_A, 1, 1),
    "one_tile_splits": Case(ONE_EACH_B, 3, 16),
    "multi_13_of_16": Case(MULTI, 13, 16),
    "multi_15_of_16": Case(MULTI, 15, 16),
    "multi_29_of_16": Case(MULTI, 29, 16),
    "multi_30_of_16": Case(MULTI, 30, 16),
    "multi_30_of_32": Case(MULTI, 30, 32),
    "multi_29_of_1": Case(MULTI, 29, 1),
    # two cases more than the list of the issue: none of its tile counts gives a head split of 12 steps or a split count of 16
    "multi_23_of_1": Case(MULTI, 23, 1),
    "multi_16_of_16": Case(MULTI, 16, 16),
}
# the split counts [256 x 256, 256 x 128, heads] each case must produce (wgrad_plan) ...
SPLITS = {
    "tiny": [1, 1, 1], "one_tile_splits": [3, 3, 3], "multi_13_of_16": [13, 13, 13], "multi_15_of_16": [14, 15, 15],
    "multi_29_of_16": [14, 29, 29], "multi_30_of_16": [14, 30, 30], "multi_30_of_32": [28, 30, 30], "multi_29_of_1": [14, 29, 8],
    "multi_23_of_1": [14, 23, 8], "multi_16_of_16": [14, 16, 16],
}
# ... and the routes it is there for
ROUTES = {
    "tiny": {"one-tile split", "head split of 4 steps", "split count < 8"},
    "one_tile_splits": {"one-tile split", "head split of 4 steps", "split count < 8"},
    "multi_13_of_16": {"one-tile split", "split count >= 8 with remainder"},              # 13 splits of one tile, every class
    "multi_15_of_16": {"empty split", "short last split", "split count >= 8 with remainder"},   # 14 splits, per = 2: 7 + a tile + 6 empty
    "multi_29_of_16": {"empty split", "short last split"},                                # per = 3: 9 full, one of 2 tiles, 4 empty
    "multi_30_of_16": {"empty split", "split count >= 8 with remainder"},                 # per = 3: 10 full, 4 empty, no short one
    "multi_30_of_32": {"empty split", "split count >= 8 with remainder"},                 # 28 splits, per = 2: 15 full, 13 empty
    "multi_29_of_1": {"head split of 16 steps", "head split of 4 steps", "short last split", "split count multiple of 8"},
    "multi_23_of_1": {"head split of 12 steps", "head split of 8 steps", "short last split"},
    "multi_16_of_16": {"split count 16", "empty split"},
}
ACC_CASE = Case(MULTI, 29, 16)
FORMS = [pytest.param(False, id="one_product"), pytest.param(True, id="x3")]

_OPS = {}


def _ops(jobs, x3):
    """the operands of a job list (every job its own data), made once for MAX_TILES tiles: a case reads its first n_tiles"""
    key = (jobs, x3)
    if key not in _OPS:
        _OPS[key] = W.make_operands(jobs, MAX_TILES if jobs is MULTI else 3, x3, seed=len(jobs) + (100 if x3 else 0))
    return _OPS[key]


# ---- CPU: the helper itself ----------------------------------------------------------------------------------------------
def test_fragment_round_trips_with_unfragment():
    from test_grad_x3 import _unfragment
    rng = np.random.default_rng(0)
    for tiles, rows in ((1, 32), (3, 128), (2, 256)):
        mat = rng.integers(-15, 16, (tiles * 64, rows)).astype(np.float64)
        frag = W.fragment(mat, rows)
        assert frag.dtype == np.float16 and frag.shape == (tiles, 4, rows // 32, 2, 32, 8)
        assert np.array_equal(_unfragment(torch.from_numpy(frag).reshape(tiles, 64 * rows), tiles, rows), mat)
        assert np.array_equal(W.unfragment(frag, tiles, rows), mat)
        # point 16 ks + 8 half + t of tile T, row 32 rb + r
        assert frag[tiles - 1, 2, rows // 32 - 1, 1, 5, 3] == mat[(tiles - 1) * 64 + 16 * 2 + 8 + 3, rows - 32 + 5]


def test_pow2_scale_twin():
    assert W.pow2_scale(0.0) == 1.0 and W.pow2_scale(float("inf")) == 1.0 and W.pow2_scale(float("nan")) == 1.0
    assert W.pow2_scale(3.5e38) == 1.0
    for amax in (1.0, 0.75, 5.0, 1000.0, 2.0 ** -20, 1023.99, 1024.0):
        s = W.pow2_scale(amax)
        assert 1024.0 <= amax * s < 2048.0 and np.log2(s) == int(np.log2(s))
    assert len(set(W.GMAX.tolist())) == 16 and W.GMAX[1] == 0
    assert len({W.pow2_scale(g) for g in W.GMAX}) >= 8             # several powers of two


def test_plan_reproduces_the_numbers_of_the_source_comment():
    """csrc/field_bwd.hip above wgrad_plan: 18 jobs at 16 requested run 14 splits each (one round of the 256 CUs), at 32
    requested 28 (two rounds)"""
    big = tuple(Job(256, 256, 0) for _ in range(18))
    assert set(W.plan_splits(big, 1000, 16)) == {14}
    assert set(W.plan_splits(big, 1000, 32)) == {28}
    assert W.plan_splits(big + (Job(32, 256, 1),), 1000, 16)[-1] == 128         # heads: 8 x
    assert W.plan_splits(big, 5, 16) == [5] * 18 and W.plan_splits(big, 0, 16) == [1] * 18
    assert W.split_ranges(29, 14) == [(3 * s, min(3 * s + 3, 29)) for s in range(14)]


@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_case_reaches_its_routes(name):
    case = GEMM_CASES[name]
    assert len(case.jobs) <= W.MAX_WJOBS and case.n_tiles <= MAX_TILES
    per_class = {W.job_class(j): s for j, s in zip(case.jobs, W.plan_splits(*case))}
    assert [per_class[c] for c in range(3)] == SPLITS[name]
    assert ROUTES[name] <= W.routes(case), (ROUTES[name] - W.routes(case))


def test_the_cases_cover_every_route():
    """a split of one tile, an empty split, a short last split, head splits of 4 and of 12 steps, a split count >= 8 with a
    remainder, one below 8, one of exactly 16"""
    reached = set().union(*(W.routes(c) for c in GEMM_CASES.values()))
    assert {"one-tile split", "empty split", "short last split", "head split of 4 steps", "head split of 12 steps",
            "split count >= 8 with remainder", "split count < 8", "split count 16"} <= reached


def _differs(a, b):
    return any(not np.array_equal(x, y) for pa, pb in zip(a, b) for x, y in zip(pa, pb))


@pytest.mark.parametrize("x3", FORMS)
@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_planted_defects_change_the_reference(name, x3):
    """What a wrong kernel would return differs from the true reference, for every job the defect touches (the unaffected jobs are
    not recomputed): the GPU tests' equality can see each of these defects in each case."""
    case = GEMM_CASES[name]
    jobs, n_tiles = case.jobs, case.n_tiles
    ops = _ops(jobs, x3)
    splits = W.plan_splits(*case)
    by_shape = {}
    for j, job in enumerate(jobs):
        by_shape.setdefault(job[:2], []).append(j)
    for j, job in enumerate(jobs):
        one = lambda **kw: W.expected_out([job], [ops[j]], n_tiles, W.GMAX, **kw)
        true = one()
        step = (7 * j + 3) % (4 * n_tiles)
        for factor in (0.0, 2.0):                                   # one k-step dropped / counted twice
            w = W.step_weights(n_tiles)
            w[step] = factor
            assert _differs(true, one(weights={0: w})), (j, "k-step", factor)
        # a split boundary moved by one tile: the first split ends a tile early and its neighbour does not start earlier
        t0, t1 = W.split_ranges(n_tiles, splits[j])[0]
        w = W.step_weights(n_tiles)
        w[4 * (t1 - 1):4 * t1] = 0.0
        assert _differs(true, one(weights={0: w})), (j, "boundary")
        # two jobs mixed up: the outputs of two equally shaped jobs swapped, or (a lone job of its shape) B read from another job
        # with as many B rows (the lone 256 x 128 job of the two small cases has no such partner)
        same = [k for k in by_shape[job[:2]] if k != j]
        if same:
            other = W.expected_out([jobs[same[0]]], [ops[same[0]]], n_tiles, W.GMAX)
            assert _differs(true, other), (j, "swapped outputs")
        else:
            k = next(k for k, o in enumerate(jobs) if k != j and o.b_rows == job.b_rows) if job.b_rows == 256 else None
            if k is not None:
                assert _differs(true, W.expected_out([job, jobs[k]], [ops[j], ops[k]], n_tiles, W.GMAX, b_from={0: 1})[:1]), (j, "B of another job")
        if job.a_rows == 32:                                        # a head row on the trunk's scale
            assert _differs(true, one(head_rows_on_trunk_scale=True)), (j, "head scale")


def _acc_reference(x3, **kw):
    f, n_grad, n_aux = W.build_map(ACC_CASE.jobs, seed=3)
    grad0 = W.grad_prefill(n_grad, seed=4)
    return f, grad0, n_aux, W.expected_accumulate(ACC_CASE.jobs, _ops(MULTI, x3), ACC_CASE.n_tiles, W.GMAX, f, grad0, n_aux, **kw)


@pytest.mark.parametrize("x3", FORMS)
def test_accumulate_map_has_every_entry_form_and_sees_an_omitted_job_b(x3):
    f, grad0, n_aux, (grad, aux) = _acc_reference(x3)
    size = np.array([j.a_rows * j.b_rows for j in ACC_CASE.jobs])
    assert len(f["dst"]) > W.ACC_GRID_CAP                            # the grid-stride loop (2048 blocks at most) runs more than once
    assert len(np.unique(f["dst"])) == len(f["dst"])                 # one owner per destination
    two, bias, to_aux = f["job_b"] >= 0, f["e_a"] >= size[f["job_a"]], f["dst"] < 0
    for form in (two, bias, to_aux, two & bias, ~two & ~bias & ~to_aux):
        # every form of entry, in the first pass of the loop and in a later one
        assert form[:W.ACC_GRID_CAP].any() and form[W.ACC_GRID_CAP:].any()
    owned = np.zeros(len(grad), bool)
    owned[f["dst"][~to_aux]] = True
    # (a sum may be zero -- the head rows past a trunk's heads are -- so not every owned element moves; no other one does)
    assert (grad0 != 0).all() and n_aux > 0 and (grad != grad0)[owned].mean() > 0.95 and np.array_equal(grad[~owned], grad0[~owned])
    assert 0 < (~owned).sum() < 2000
    _, _, _, (grad_b, aux_b) = _acc_reference(x3, omit_job_b=True)
    touched = np.zeros(len(grad), bool)
    touched[f["dst"][two]] = True
    assert (grad_b != grad)[touched].mean() > 0.9 and np.array_equal(grad_b[~touched], grad[~touched])


# ---- GPU -----------------------------------------------------------------------------------------------------------------
_DEV_OPS = {}


def _device_jobs(jobs, x3, out_offs):
    """job tuples of _lib.weight_grad* over device copies of _ops(jobs, x3): a value plane with its remainder plane behind it"""
    key = (jobs, x3)
    if key not in _DEV_OPS:
        held = []
        for job, op in zip(jobs, _ops(jobs, x3)):
            tiles = op["a"].shape[0] // 64
            t = {}
            for side, rows in (("a", job.a_rows), ("b", job.b_rows)):
                planes = [W.fragment(op[side], rows)] + ([W.fragment(op[side + "_lo"], rows)] if side + "_lo" in op else [])
                t[side] = torch.from_numpy(np.stack(planes)).cuda()
                assert t[side].shape[1] == tiles
            held.append(t)
        _DEV_OPS[key] = held
    res = []
    for job, t, off in zip(jobs, _DEV_OPS[key], out_offs):
        lo = lambda x: x[0].numel() if x.shape[0] == 2 else 0
        res.append((t["a"].data_ptr(), t["b"].data_ptr(), job.a_rows, job.b_rows, off, job.trunk, lo(t["a"]), lo(t["b"])))
        assert (res[-1][7] != 0) == x3 and (res[-1][6] != 0) == (x3 and job.a_rows == 256)
    return res


def _out_layout(jobs):
    """out_off of every job: the jobs in reverse order with a 64-float gap in front of each (nothing may be written there)"""
    offs, off = [0] * len(jobs), 0
    for j in reversed(range(len(jobs))):
        off += 64
        offs[j] = off
        off += jobs[j].a_rows * jobs[j].b_rows
    return offs, off + 64


@pytest.mark.gpu
@pytest.mark.parametrize("x3", FORMS)
@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_weight_grad_equals_the_float64_product(name, x3, hip_lib):
    from nsff_pl_amd import _lib
    case = GEMM_CASES[name]
    jobs = case.jobs
    offs, total = _out_layout(jobs)
    want = W.expected_out(jobs, _ops(jobs, x3), case.n_tiles, W.GMAX)
    out = torch.full((total,), -77.0, device="cuda")
    bias = torch.full((len(jobs), 256), -77.0, device="cuda")
    _lib.weight_grad(_device_jobs(jobs, x3, offs), case.n_tiles, case.n_splits, out, bias, torch.from_numpy(W.GMAX).cuda())
    torch.cuda.synchronize()
    out, bias = out.cpu().numpy().astype(np.float64), bias.cpu().numpy().astype(np.float64)
    written = np.zeros(total, bool)
    for j, (job, (mat, rows)) in enumerate(zip(jobs, want)):
        got = out[offs[j]:offs[j] + mat.size].reshape(mat.shape)
        written[offs[j]:offs[j] + mat.size] = True
        assert np.abs(mat).max() > 0
        assert np.array_equal(got, mat), (name, j, job, int((got != mat).sum()), np.argwhere(got != mat)[:4].tolist())
        assert np.array_equal(bias[j, :job.a_rows], rows), (name, j, job, np.flatnonzero(bias[j, :job.a_rows] != rows)[:8].tolist())
        if job.a_rows == 32:                    # rows past the trunk's heads (and past their +16 twins): exact zeros
            dead = np.ones(32, bool)
            dead[:W.HEAD_ROWS[job.trunk]] = dead[16:16 + W.HEAD_ROWS[job.trunk]] = False
            assert not mat[dead].any() and not got[dead].any() and not bias[j, :32][dead].any()
    assert (out[~written] == -77.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("x3", FORMS)
def test_weight_grad_accumulate_equals_the_float64_sums(x3, hip_lib):
    """nsff_wgrad_accumulate_kernel through _lib.weight_grad_accumulate: 1.3 M entries (the 2048-block grid strides three times),
    one- and two-source entries, bias entries, stores to aux, onto a grad full of non-zero integers."""
    from nsff_pl_amd import _lib
    f, grad0, n_aux, (want_grad, want_aux) = _acc_reference(x3)
    jobs = ACC_CASE.jobs
    grad = torch.from_numpy(grad0.astype(np.float32)).cuda()
    aux = torch.full((n_aux,), -77.0, device="cuda")
    table = torch.from_numpy(W.pack_map(f)).cuda()
    _lib.weight_grad_accumulate(_device_jobs(jobs, x3, [0] * len(jobs)), ACC_CASE.n_tiles, ACC_CASE.n_splits, table, grad.data_ptr(),
                                torch.from_numpy(W.GMAX).cuda(), aux=aux)
    torch.cuda.synchronize()
    got_grad, got_aux = grad.cpu().numpy().astype(np.float64), aux.cpu().numpy().astype(np.float64)
    assert np.array_equal(got_grad, want_grad), (int((got_grad != want_grad).sum()), np.flatnonzero(got_grad != want_grad)[:8].tolist())
    assert np.array_equal(got_aux, want_aux), (int((got_aux != want_aux).sum()), np.flatnonzero(got_aux != want_aux)[:8].tolist())


@pytest.mark.gpu
def test_degenerate_calls_launch_nothing(hip_lib):
    from nsff_pl_amd import _lib
    lib = hip_lib
    dev_jobs = _device_jobs(ONE_EACH_A, False, [0, 65536, 98304])
    x3_jobs = _device_jobs(ONE_EACH_A, True, [0, 65536, 98304])
    out = torch.full((98304 + 8192,), -77.0, device="cuda")
    bias = torch.full((3, 256), -77.0, device="cuda")
    scratch = torch.empty(1 << 20, device="cuda")
    gmax = torch.from_numpy(W.GMAX).cuda()

    def call(jobs, n_tiles, n_splits=1):
        arr = _lib._wgrad_jobs(jobs, True)
        return lib.nsff_weight_grad(arr, len(jobs), n_tiles, n_splits, scratch.data_ptr(), out.data_ptr(), bias.data_ptr(), gmax.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert call(dev_jobs, 0) == 0                                           # no tiles: OK, nothing written
    a, b = dev_jobs[2][0], dev_jobs[1][1]
    assert call([(a, b, 32, 128, 0, 0)], 1) == -1                           # a 32 x 128 job: NSFF_ERR_INVALID
    assert call([dev_jobs[0], x3_jobs[1], dev_jobs[2]], 1) == -1            # X3 and one-product jobs in one call
    assert call([x3_jobs[0], dev_jobs[1], x3_jobs[2]], 1) == -1
    assert call(dev_jobs, 1, 0) == -1                                       # n_splits = 0
    arr = _lib._wgrad_jobs(dev_jobs, True)
    assert lib.nsff_weight_grad_scratch(arr, 3, 1, 0) == -1
    assert lib.nsff_weight_grad_scratch(arr, 3, 1, 1) == 256 * 256 + 256 * 128 + 32 * 256 + 3 * 256
    torch.cuda.synchronize()
    assert bool((out == -77.0).all()) and bool((bias == -77.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 255, 256, 257, 4099, 32771])          # (32771 points: more float4s than 512 blocks cover at once)
def test_absmax_of_records_equals_numpy(P, hip_lib):
    from nsff_pl_amd import _lib
    rng = np.random.default_rng(P)
    x = (rng.standard_normal((P, 16)) * np.exp2(rng.integers(-20, 20, (P, 16)))).astype(np.float32)
    x[:, 5] = 0.0                                     # a column of zeros
    x[:, 9] = -0.0                                    # ... and one of negative zeros
    x[rng.integers(0, P), 2] = -0.0
    x[-1, 3] = -3.0e30                                # the maximum in the last row, negative
    x[-1, 15] = 2.5e31
    got = _lib.absmax(torch.from_numpy(x).cuda()).cpu().numpy()
    want = np.abs(x).max(0)
    assert np.array_equal(got, want) and not np.signbit(got).any(), (got, want)
    assert got[3] == np.float32(3.0e30) and got[5] == 0 and got[9] == 0
