"""Plain numpy twin of the split-K weight-gradient path of csrc/field_bwd.hip (nsff_wgrad_kernel, nsff_wgrad_head_kernel,
nsff_wgrad_reduce_kernel, nsff_wgrad_accumulate_kernel and the host-side wgrad_plan), for inputs on which fp32 arithmetic is EXACT.

Both GEMM operands are fp16 and the accumulators fp32.  The operands made here are small integers (|v| <= 15) times a power of two
per operand row, so every product is an integer in the quantum 2^(ka[i] + kb[j]) of its output element (i, j) and every partial sum
stays below 2^24 of that quantum (asserted on the generated data): the MFMA accumulators, the fdot2 row sums, the sums over the
splits and the division by the power-of-two scales are all exact.  The reference is therefore a float64 `A.T @ B` and the GPU result
must be EQUAL to it -- no tolerance; a dropped or doubled 16-point step, a wrong split range, job offset or scale changes it.

Layout (include/nsff_render.h above NsffWgradJob; tests/test_grad_x3.py::_unfragment): an operand of `rows` rows over T 64-point
tiles is fp16 (T, 4, rows / 32, 2, 32, 8) = tile, k-step, row block, point half, row, 8 points; point 16 ks + 8 half + t of the tile.
"""
import math
from collections import namedtuple

import numpy as np

Job = namedtuple("Job", "a_rows b_rows trunk")
Case = namedtuple("Case", "jobs n_tiles n_splits")

MAX_WJOBS = 48
WGRAD_CUS = 256
ACC_GRID_CAP = 2048 * 256          # entries one pass of nsff_wgrad_accumulate_kernel's grid-stride loop covers
HEAD_ROWS = {0: 4, 1: 10}          # head rows a trunk writes (static: rgb + sigma, dynamic: rgb, sigma, two flows); + their +16 twins

# the 16 column maxima of |d_raw|: distinct, spanning 2^-3 .. 2^9, an exact power of two (1.0), a zero column (1: head row 1 of the
# static trunk is then on the scale 1) and the two unused columns 14, 15 (the scale of the head rows past a trunk's heads)
GMAX = np.array([0.75, 0.0, 5.0, 1.0, 96.0, 0.125, 1000.0, 0.3125, 12.0, 2.5, 320.0, 0.625, 40.0, 6.0, 0.25, 7.0], np.float32)


# ---- the plan ------------------------------------------------------------------------------------------------------------
def job_class(job):
    """0: 256 x 256, 1: 256 x 128 (nsff_wgrad_kernel's two builds), 2: the 32 x 256 head jobs (nsff_wgrad_head_kernel)"""
    return 2 if job.a_rows == 32 else (1 if job.b_rows == 128 else 0)


def plan_splits(jobs, n_tiles, n_splits):
    """wgrad_plan: the split-K factor of every job.  A class of m GEMM jobs gets floor(256 r / m) splits each with the smallest r
    that reaches 3/4 of the request, the heads 8 x the request; nothing above n_tiles, nothing below 1."""
    m = [sum(1 for j in jobs if job_class(j) == c) for c in range(3)]
    per_class = [1, 1, 8 * n_splits]
    for c in range(2):
        r = 1
        while m[c] > 0 and 4 * (WGRAD_CUS * r // m[c]) < 3 * n_splits:
            r += 1
        per_class[c] = WGRAD_CUS * r // m[c] if m[c] > 0 else 1
    return [max(1, min(per_class[job_class(j)], n_tiles)) for j in jobs]


def split_ranges(n_tiles, splits):
    """[(t0, t1)] of the kernels' `per = ceil(n_tiles / n_splits)` arithmetic: t1 <= t0 is an empty split (it writes zeros)"""
    per = (n_tiles + splits - 1) // splits
    return [(s * per, min(s * per + per, n_tiles)) for s in range(splits)]


def routes(case):
    """Names of the code routes a case drives the kernels through (what tests/test_wgrad_kernels.py states per case)."""
    out = set()
    for job, sp in zip(case.jobs, plan_splits(case.jobs, case.n_tiles, case.n_splits)):
        head = job_class(job) == 2
        sizes = [max(t1 - t0, 0) for t0, t1 in split_ranges(case.n_tiles, sp)]
        full = max(sizes)
        for n in sizes:
            if n == 0:
                out.add("empty split")
            if n == 1 and not head:
                out.add("one-tile split")            # 4 k-steps against 7 (X3: 3) prefetched stages of the LDS ring
            if 0 < n < full:
                out.add("short last split")
            if head and n > 0:
                out.add(f"head split of {4 * n} steps")
        out.add("split count < 8" if sp < 8 else ("split count 16" if sp == 16 else
                ("split count >= 8 with remainder" if sp % 8 else "split count multiple of 8")))
    return out


# ---- scales --------------------------------------------------------------------------------------------------------------
def pow2_scale(amax):
    """2^(11 - e) with amax = m 2^e, m in [0.5, 1); 1 for amax == 0 or a non-finite amax"""
    amax = float(amax)
    if not (amax > 0.0) or not (amax < 3.0e38):
        return 1.0
    return math.ldexp(1.0, 11 - math.frexp(amax)[1])


def trunk_scale(gmax, trunk):
    return pow2_scale(max(gmax[0:4]) if trunk == 0 else max(gmax[4:14]))


def head_row_scale(gmax, trunk, row):
    return pow2_scale(gmax[min((4 if trunk else 0) + (row & 15), 15)])


def row_scales(job, gmax, head_rows_on_trunk_scale=False):
    """the divisor of every output row (and bias row sum) of a job"""
    if job.a_rows == 32 and not head_rows_on_trunk_scale:
        return np.array([head_row_scale(gmax, job.trunk, r) for r in range(32)])
    return np.full(job.a_rows, trunk_scale(gmax, job.trunk))


# ---- layout --------------------------------------------------------------------------------------------------------------
def fragment(mat, rows):
    """(T * 64 points, rows) -> fp16 (T, 4, rows / 32, 2, 32, 8): the inverse of tests/test_grad_x3.py::_unfragment"""
    mat = np.asarray(mat)
    tiles = mat.shape[0] // 64
    assert mat.shape == (tiles * 64, rows) and rows % 32 == 0
    a = mat.reshape(tiles, 4, 2, 8, rows // 32, 32)               # tile, ks, point half, t, row block, row
    return np.ascontiguousarray(a.transpose(0, 1, 4, 2, 5, 3)).astype(np.float16)


def unfragment(frag, tiles, rows):
    a = np.asarray(frag).reshape(tiles, 4, rows // 32, 2, 32, 8)
    return a.transpose(0, 1, 3, 5, 2, 4).reshape(tiles * 64, rows).astype(np.float64)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def make_operands(jobs, n_tiles, x3, seed):
    """Per job {a, b[, a_lo, b_lo]}: fp16 (n_tiles * 64 points, rows) matrices of integers |v| <= 15 times 2^k per row (k in -2..2
    for A, -1..1 for B; a remainder plane shares its value plane's k), every job its own data.  A head job's A is non-zero only on
    its trunk's head rows and their +16 twins (the remainder rows: it has no a_lo).  Asserts the exactness bound."""
    rng = np.random.default_rng(seed)
    K = n_tiles * 64
    ops = []
    for job in jobs:
        ka = rng.integers(-2, 3, job.a_rows)
        kb = rng.integers(-1, 2, job.b_rows)
        ints = lambda rows: rng.integers(-15, 16, (K, rows)).astype(np.float64)
        planes = {"a": ints(job.a_rows), "b": ints(job.b_rows)}
        if x3:
            planes["b_lo"] = ints(job.b_rows)
            if job.a_rows == 256:
                planes["a_lo"] = ints(job.a_rows)
        if job.a_rows == 32:
            live = np.zeros(32, bool)
            live[:HEAD_ROWS[job.trunk]] = live[16:16 + HEAD_ROWS[job.trunk]] = True
            planes["a"][:, ~live] = 0.0
        # every accumulator holds sum_k a_k b_k over at most all K points, an integer in its own quantum: exact below 2^24
        bound = np.abs(planes["a"]).T @ np.abs(planes["b"])
        if "b_lo" in planes:
            bound += np.abs(planes["a"]).T @ np.abs(planes["b_lo"])
        if "a_lo" in planes:
            bound += np.abs(planes["a_lo"]).T @ np.abs(planes["b"])
        assert bound.max() < 2 ** 24, bound.max()
        assert np.abs(planes["a"]).sum(0).max() + (np.abs(planes["a_lo"]).sum(0).max() if "a_lo" in planes else 0) < 2 ** 24
        op = {}
        for name, v in planes.items():
            v = v * np.exp2(ka if name[0] == "a" else kb)
            op[name] = v.astype(np.float16)
            assert (op[name].astype(np.float64) == v).all()
        ops.append(op)
    return ops


def step_weights(n_tiles):
    """one weight per 16-point k-step: all ones is the true sum (the planted defects edit it)"""
    return np.ones(4 * n_tiles)


def job_sums(op, n_tiles, weights=None, b_from=None):
    """The unscaled sums of one job over its first n_tiles tiles: (a_rows, b_rows) matrix, (a_rows,) row sums.  One product, or
    (with remainder planes) A B + A_lo B + A B_lo; a head job has no A_lo.  weights: per k-step; b_from: another job's B planes."""
    K = 64 * n_tiles
    w = np.repeat(step_weights(n_tiles) if weights is None else weights, 16)[:, None]
    a = op["a"][:K].astype(np.float64) * w
    src = op if b_from is None else b_from
    b = src["b"][:K].astype(np.float64)
    mat, rows = a.T @ b, a.sum(0)
    if "b_lo" in src:
        mat += a.T @ src["b_lo"][:K].astype(np.float64)
    if "a_lo" in op:
        a_lo = op["a_lo"][:K].astype(np.float64) * w
        mat += a_lo.T @ b
        rows = rows + a_lo.sum(0)
    return mat, rows


def _exact32(x):
    assert (x.astype(np.float32).astype(np.float64) == x).all(), "the expected value is not an fp32 number"
    return x


def expected_out(jobs, ops, n_tiles, gmax, weights=None, head_rows_on_trunk_scale=False, b_from=None):
    """nsff_weight_grad: [(out_j (a_rows, b_rows), bias_j (a_rows,))], float64, every element an fp32 number.
    weights: {job index: per-k-step weights}; b_from: {job index: index of the job whose B it reads} (planted defects)."""
    res = []
    for j, (job, op) in enumerate(zip(jobs, ops)):
        mat, rows = job_sums(op, n_tiles, (weights or {}).get(j), ops[b_from[j]] if b_from and j in b_from else None)
        s = row_scales(job, gmax, head_rows_on_trunk_scale)
        res.append((_exact32(mat / s[:, None]), _exact32(rows / s)))
    return res


# ---- the gather form -----------------------------------------------------------------------------------------------------
def build_map(jobs, seed, n_spare=1000):
    """A gradient map (NsffGradMapEntry fields as int arrays: dst, e_a, e_b, job_a, job_b) over a job list, shuffled:
    * every element of every 256 x 256 job, one source;
    * the 256 x 128 jobs pairwise (same trunk): element e of the first + element e of the second (job_b >= 0);
    * every job's bias row sums (e >= size); the 256 x 128 pairs' again as two-source entries;
    * the head jobs: rows r + (16 + r), matrix and row sums (job_b = job_a);
    * dst < 0: the head jobs' dense matrices and their 32 row sums, stored to aux.
    Every dst >= 0 appears once; the destinations are a random subset of [0, n + n_spare).  -> (fields, n_grad, n_aux)"""
    rng = np.random.default_rng(seed)
    size = lambda j: jobs[j].a_rows * jobs[j].b_rows
    ja, ea, jb, eb, aux = [], [], [], [], []

    def add(j_a, e_a, j_b=None, e_b=None, to_aux=False):
        n = len(e_a)
        ja.append(np.full(n, j_a)); ea.append(np.asarray(e_a))
        jb.append(np.full(n, -1 if j_b is None else j_b)); eb.append(np.zeros(n, np.int64) if e_b is None else np.asarray(e_b))
        aux.append(np.full(n, to_aux))
    narrow = {0: [], 1: []}
    for j, job in enumerate(jobs):
        c = job_class(job)
        if c == 0:
            add(j, np.arange(size(j) + 256))
        elif c == 1:
            narrow[job.trunk].append(j)
            add(j, size(j) + np.arange(256))
        else:
            r = np.arange(16 * 256)
            add(j, r, j, r + 16 * 256)
            add(j, size(j) + np.arange(16), j, size(j) + 16 + np.arange(16))
            add(j, np.arange(size(j) + 32), to_aux=True)
    for t in (0, 1):
        for j0, j1 in zip(narrow[t][0::2], narrow[t][1::2]):
            e = np.arange(size(j0) + 256)
            add(j0, e, j1, e)
    f = {"job_a": np.concatenate(ja), "e_a": np.concatenate(ea), "job_b": np.concatenate(jb), "e_b": np.concatenate(eb)}
    to_aux = np.concatenate(aux)
    order = rng.permutation(len(to_aux))
    f = {k: v[order] for k, v in f.items()}
    to_aux = to_aux[order]
    n_grad, n_aux = int((~to_aux).sum()) + n_spare, int(to_aux.sum())
    dst = np.empty(len(to_aux), np.int64)
    dst[~to_aux] = rng.permutation(n_grad)[:n_grad - n_spare]
    dst[to_aux] = -(1 + rng.permutation(n_aux))
    f["dst"] = dst
    return f, n_grad, n_aux


def pack_map(f):
    """(n, 4) int32 rows of NsffGradMapEntry: dst, e_a, e_b, (job_a, job_b) as two little-endian int16"""
    ent = np.empty((len(f["dst"]), 4), np.int32)
    ent[:, 0], ent[:, 1], ent[:, 2] = f["dst"], f["e_a"], f["e_b"]
    pair = np.stack([f["job_a"].astype("<i2"), f["job_b"].astype("<i2")], 1)
    ent[:, 3] = np.ascontiguousarray(pair).view("<i4").reshape(-1)
    return ent


def grad_prefill(n_grad, seed):
    """non-zero integers: the kernel ADDS into grad"""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 9, n_grad) * rng.choice([-1.0, 1.0], n_grad)).astype(np.float64)


def expected_accumulate(jobs, ops, n_tiles, gmax, f, grad0, n_aux, omit_job_b=False):
    """nsff_weight_grad_accumulate_aux: grad[dst] += (S(job_a, e_a) + S(job_b, e_b)) / scale of job_a's row; dst < 0 stores to
    aux[-(dst + 1)].  -> (grad, aux) float64, every element an fp32 number."""
    sums = []
    for job, op in zip(jobs, ops):
        mat, rows = job_sums(op, n_tiles)
        tail = np.full(256, np.nan)                  # (a head job's row sums 32..255 are not defined: the map must not name them)
        tail[:job.a_rows] = rows
        sums.append(np.concatenate([mat.reshape(-1), tail]))
    val = np.empty(len(f["dst"]))
    for j, job in enumerate(jobs):
        size = job.a_rows * job.b_rows
        sel = f["job_a"] == j
        e = f["e_a"][sel]
        row = np.where(e < size, e // job.b_rows, e - size)
        v = sums[j][e]
        jb, ebs = f["job_b"][sel], f["e_b"][sel]
        if not omit_job_b:
            for k in np.unique(jb[jb >= 0]):
                assert jobs[k].trunk == job.trunk          # (the two sources of an element are on one scale)
                two = jb == k
                v[two] = v[two] + sums[k][ebs[two]]
        val[sel] = v / row_scales(job, gmax)[row]
    assert not np.isnan(val).any()
    grad, aux = grad0.copy(), np.zeros(n_aux)
    to_grad = f["dst"] >= 0
    assert len(np.unique(f["dst"])) == len(f["dst"])
    grad[f["dst"][to_grad]] += val[to_grad]
    aux[-(f["dst"][~to_grad] + 1)] = val[~to_grad]
    return _exact32(grad), _exact32(aux)
