"""TEST INFRASTRUCTURE: the small fp32 kernels between the pieces of the training step -- ``nsff_time_rows`` and
``nsff_time_rows_backward`` (csrc/rays.hip), ``nsff_flow_grad`` (csrc/rays_bwd.hip), ``nsff_fold_grads``, ``nsff_fold_grads_dense``
and ``nsff_absmax`` (csrc/field_bwd.hip) -- as plain numpy float64 expressions of their inputs (the header comments of
include/nsff_render.h), the cases the kernels are held to and the defects the cases must notice.  Nothing here touches the GPU;
every case is seeded, built once and read-only.

All of these are sums, or sums of products, of a few hundred to a few thousand fp32 terms.  The cases are INTEGER-VALUED fp32 arrays
(cotangents and G in [-7, 7], remainder rows in [-3, 3], weights and biases in [-7, 7], prior gradients in [-100, 100]) chosen so
that the sum of the ABSOLUTE terms of every output element stays below 2^24: every partial sum, in any order, is then an integer
below 2^24 in magnitude, fp32 arithmetic -- fmaf included -- is exact, and the kernel's result must EQUAL the float64 reference
cast to fp32.  No tolerance.  (``abs_terms`` of a case is that sum; the CPU tests assert it.)

Time rows (the index rule is the kernels' own, field_inputs_ref.gather_index): next = E[min(t + 1, max_t)] and prev =
E[max(t - 1, 0)], both kept inside the table; cur hits row t only for 0 <= t < n_table; d_table[r] = the sum of the rows of
g_cur / g_next / g_prev whose index is r, an absent cotangent contributes nothing, a row no ray hits is written as zeros.  The
kernel (one workgroup per table row) walks the rays in passes of CHUNK = 2048, compacts the hitting rays of a pass into one list
per gather, adds the listed rows sixteen at a time (four waves x four rows) and holds 64 x 4 = 256 columns in registers per
column group: ``hit_lists`` restates that bookkeeping so that a case can assert the route it was named for (passes, fullest
list, column groups, list lengths mod 16) and so that defects of exactly that bookkeeping can be planted.

Flow glue: out[p, col + c] = [not zs[p] > z_far] * sum_k g[k][p, c]; every other column zero (overwrite) or unchanged
(accumulate).  A NaN depth compares false: the point is kept, as torch.where(zs > z_far, 0, flow) keeps it.

Fold algebra (field_grad._folded_grads): with G = g + g2 and gb = gb + gb2
    dW_head = G W_final^T + gb (x) b_final      db_head = gb
    dW_final = W_head^T G                       db_final = W_head^T gb
for nsff_fold_grads g2 / gb2 are rows 16 + r of the same (32, 256) / (32) job.

A planted defect is a keyword of a reference function; a reference with a defect is never used as a reference.
"""
import functools
from types import SimpleNamespace

import numpy as np

from composite_ref import FACTOR, FLOOR, bound  # noqa: F401  (the project's rule, for the one real-valued case)
from field_inputs_ref import gather_index, row_errors  # noqa: F401  (the kernels' own index rule; the per-row measure)

EXACT = 2.0 ** 24
CHUNK = 2048               # TRB_CHUNK: rays per compaction pass
GROUP = 256                # 64 * TRB_COLS: columns per column group
LIST_STEP = 16             # four waves x four rows requested before the first add

TIME_DEFECTS = ("chunk_carry", "drop_list_tail", "drop_entry_2047", "col_group", "col_register", "clamp_table_end", "cur_clamped")
FLOW_DEFECTS = ("mask_ge", "fourth_cotangent", "group_b_over_a")
FOLD_DEFECTS = ("no_remainder_rows", "no_bias_term", "row_tail", "ld_mixup")
FOLD_ROWS = 4              # rows of the folded layer per workgroup of the dense head kernel


def _frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


def _ints(rng, lo, hi, *shape):
    """integer-valued fp32 in [lo, hi]"""
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def to_f32(x):
    """a float64 reference as the fp32 array the kernel must produce (exact for these cases: asserted)"""
    y = np.asarray(x, np.float64).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), np.asarray(x, np.float64), equal_nan=True), "the reference is no fp32 number"
    return y


# =====================================================================================================================
# time rows
# =====================================================================================================================
def time_indices(ts, n_table, max_t, defect=None):
    """[(row (n,), counted (n,))] for cur, next, prev"""
    t = np.asarray(ts, np.int64)
    inside = (t >= 0) & (t < n_table)
    if defect == "cur_clamped":
        inside = np.ones_like(inside)
    every = np.ones(t.shape, bool)
    return [(np.clip(t, 0, n_table - 1), inside),
            (gather_index(t, 1, n_table, max_t, "clamp_at_table_end" if defect == "clamp_table_end" else None), every),
            (gather_index(t, -1, n_table, max_t), every)]


def time_rows(table, ts, max_t, delta):
    """the forward gather: table[index], bit for bit"""
    return np.asarray(table)[gather_index(ts, delta, np.asarray(table).shape[0], max_t)]


def hit_lists(ts, n_table, max_t, present, defect=None):
    """{(gather, pass, row): ascending ray numbers}: the non-empty lists of the kernel's compaction"""
    out = {}
    n = len(ts)
    for l, (row, ok) in enumerate(time_indices(ts, n_table, max_t, defect)):
        if not present[l]:
            continue
        for p, base in enumerate(range(0, n, CHUNK)):
            seg = np.arange(base, min(base + CHUNK, n))
            seg = seg[ok[seg]]
            for r in np.unique(row[seg]):
                out[(l, p, int(r))] = seg[row[seg] == r]
    return out


def time_routes(ts, width, n_table, max_t, present):
    """what a launch takes: passes, the fullest list, column groups, 64-column registers in use, the list lengths mod 16 and the
    table rows that no list names"""
    lists = hit_lists(ts, n_table, max_t, present)
    lens = [len(v) for v in lists.values()]
    return SimpleNamespace(passes=-(-len(ts) // CHUNK), fullest=max(lens, default=0), groups=-(-width // GROUP),
                           registers=-(-min(width, GROUP) // 64), mods={v % LIST_STEP for v in lens},
                           unhit=sorted(set(range(n_table)) - {k[2] for k in lists}), lists=len(lists))


def time_rows_backward(gs, ts, n_table, max_t, width, defect=None, absolute=False):
    """(n_table, width) float64.  gs: (g_cur, g_next, g_prev), each (n, width) or None.  absolute: the sum of the absolute terms."""
    assert defect is None or defect in TIME_DEFECTS
    out = np.zeros((n_table, width), np.float64)
    n = len(ts)
    present = [g is not None for g in gs]
    by_list = defect in ("chunk_carry", "drop_list_tail", "drop_entry_2047")
    lists = hit_lists(ts, n_table, max_t, present, defect) if by_list else None
    for l, (row, ok) in enumerate(time_indices(ts, n_table, max_t, defect)):
        if gs[l] is None or n == 0:
            continue
        g = np.asarray(gs[l], np.float64).reshape(n, width)
        g = np.abs(g) if absolute else g
        if not by_list:
            onehot = np.zeros((n_table, n), np.float64)
            onehot[row[ok], np.nonzero(ok)[0]] = 1.0
            out += onehot @ g
            continue
        for (ll, p, r), rays in lists.items():
            if ll != l:
                continue
            use = rays
            if defect == "drop_list_tail":
                use = rays[:len(rays) - len(rays) % LIST_STEP]
            if defect == "drop_entry_2047":
                use = rays[rays % CHUNK != CHUNK - 1]
            out[r] += g[use].sum(0)
            if defect == "chunk_carry" and p >= 1 and (l, p - 1, r) in lists:
                out[r] += g[lists[(l, p - 1, r)]].sum(0)
    if defect == "col_group" and width > GROUP:
        out[:, GROUP:] = out[:, :width - GROUP]
    if defect == "col_register" and width > 64:
        hi = min(width, 128)
        out[:, 64:hi] = out[:, :hi - 64]
    return out


def time_rows_backward_f32(gs, ts, n_table, max_t, width):
    """the fp32 twin of the real-valued case: a sequential fp32 sum in ray order (cur, next, prev of ray 0, then ray 1, ...)"""
    acc = np.zeros((n_table, width), np.float32)
    idx = time_indices(ts, n_table, max_t)
    gs = [None if g is None else np.asarray(g, np.float32) for g in gs]
    for i in range(len(ts)):
        for l, (row, ok) in enumerate(idx):
            if gs[l] is not None and ok[i]:
                acc[row[i]] = acc[row[i]] + gs[l][i]
    return acc


def _ts_edges(rng, n, n_table, max_t):
    """uniform frames with the clamps, the table's end and two indices outside the table planted at seeded places"""
    ts = rng.integers(0, n_table, size=n).astype(np.int64)
    edge = [-3, n_table + 10, 0, n_table - 1, min(max(max_t, 0), n_table - 1), min(max(max_t - 1, 0), n_table - 1), 1 % n_table]
    where = rng.permutation(n)[:len(edge)]
    ts[where] = edge[:len(where)]
    return ts


def _ts_counts(rng, n, n_table, counts):
    """`counts[frame]` rays on each named frame, every other ray outside the table (-3 and n_table + 10 in turn), shuffled"""
    ts = [f for f, c in counts.items() for _ in range(c)]
    assert len(ts) <= n
    ts += [(-3, n_table + 10)[k % 2] for k in range(n - len(ts))]
    return rng.permutation(np.asarray(ts, np.int64))


CUR, NEXT, PREV = (1, 0, 0), (0, 1, 0), (0, 0, 1)
ALL3 = (1, 1, 1)
# name: (n, width, n_table, max_t, (cur, next, prev) present, frame indices)
#   frame indices: "edges" (see _ts_edges) | ("frame", f): every ray on frame f | ("frames", (f, ...)): uniform over those frames |
#   ("counts", {frame: rays}): see _ts_counts
TIME_CASES = {
    "no_rays":            (0, 48, 12, 11, ALL3, "edges"),                          # every row written as zeros
    "one_ray_one_row":    (1, 1, 1, 0, ALL3, ("frame", 0)),                        # all three gathers of the ray hit row 0
    "n63_w3":             (63, 3, 2, 1, (1, 1, 0), "edges"),
    "n64_w63_cropped":    (64, 63, 12, 8, ALL3, "edges"),                          # max_t = n_table - 4: a cropped sequence
    "n65_w64_max_t_0":    (65, 64, 12, 0, NEXT, "edges"),                          # next is row 0 for every ray
    "n65_w65_past_end":   (65, 65, 12, 17, PREV, "edges"),                         # max_t = n_table + 5
    "n2047_w48":          (2047, 48, 12, 11, ALL3, "edges"),                       # the trainer's shape, one ray short of a pass
    "full_list":          (2048, 48, 12, 11, ALL3, ("frame", 5)),                  # lists of exactly TRB_CHUNK entries (rows 5, 6, 4)
    "n2049_w128_cur":     (2049, 128, 30, 26, CUR, "edges"),                       # a second pass of one ray; two registers
    "last_pass_one_ray":  (4097, 64, 12, 11, ALL3, ("frame", 11)),                 # two full lists, then a pass of one ray
    "n4097_w300":         (4097, 300, 12, 11, ALL3, "edges"),                      # three passes x two column groups
    "n2049_w256":         (2049, 256, 30, 35, (0, 1, 1), "edges"),                 # exactly one column group, all four registers
    "n65_w257":           (65, 257, 2, 0, ALL3, "edges"),                          # a second column group of one column
    "sparse_frames":      (2047, 65, 30, 26, (1, 0, 1), ("frames", (3, 4))),       # rows 2..4 hit, 27 rows of zeros
    "list_tails":         (2047, 48, 12, 11, CUR, ("counts", {2: 17, 5: 21, 7: 31, 9: 16})),    # cnt % 16 = 1, 5, 15, 0
    "one_row_table":      (2049, 1, 1, 6, ALL3, "edges"),                          # n_table = 1: next / prev of every ray are row 0
    "n1_w300":            (1, 300, 30, 29, ALL3, ("frame", 29)),                   # cur and next on the last row, prev on 28
    "n2048_w3_cropped":   (2048, 3, 30, 26, (0, 1, 0), "edges"),
    "n4097_w1":           (4097, 1, 2, 7, (1, 0, 1), "edges"),
    "n64_w128_two_rows":  (64, 128, 2, 1, ALL3, "edges"),
}
# the named case on which each planted defect must show
TIME_DEFECT_CASES = {"chunk_carry": ("last_pass_one_ray", "n4097_w300", "n2049_w128_cur"),
                     "drop_list_tail": ("list_tails", "n2047_w48"),
                     "drop_entry_2047": ("full_list", "last_pass_one_ray"),
                     "col_group": ("n4097_w300", "n65_w257"),
                     "col_register": ("n65_w65_past_end", "n2049_w128_cur", "n4097_w300"),
                     "clamp_table_end": ("n64_w63_cropped", "n2048_w3_cropped"),
                     "cur_clamped": ("n64_w63_cropped", "list_tails", "n2049_w128_cur")}


@functools.lru_cache(maxsize=None)
def time_case(name):
    n, width, n_table, max_t, present, kind = TIME_CASES[name]
    rng = np.random.default_rng(3000 + list(TIME_CASES).index(name))
    if n == 0:
        ts = np.zeros(0, np.int64)
    elif kind == "edges":
        ts = _ts_edges(rng, n, n_table, max_t)
    elif kind[0] == "frame":
        ts = np.full(n, kind[1], np.int64)
    elif kind[0] == "frames":
        ts = rng.choice(np.asarray(kind[1], np.int64), size=n)
    else:
        ts = _ts_counts(rng, n, n_table, kind[1])
    gs = tuple(_frozen(_ints(rng, -7, 7, n, width)) if on else None for on in present)
    want = time_rows_backward(gs, ts, n_table, max_t, width)
    return SimpleNamespace(name=name, n=n, width=width, n_table=n_table, max_t=max_t, present=tuple(bool(v) for v in present),
                           ts=_frozen(ts), gs=gs, want=_frozen(want),
                           abs_terms=float(time_rows_backward(gs, ts, n_table, max_t, width, absolute=True).max(initial=0.0)),
                           routes=time_routes(ts, width, n_table, max_t, present))


@functools.lru_cache(maxsize=None)
def real_time_case():
    """the one real-valued case: standard-normal cotangents, 4097 rays x 300 columns on 12 frames (three passes, two column
    groups), float64 reference, the sequential fp32 twin and its d32 in the per-row measure"""
    n, width, n_table, max_t = 4097, 300, 12, 11
    rng = np.random.default_rng(3100)
    ts = _ts_edges(rng, n, n_table, max_t)
    gs = tuple(_frozen(rng.standard_normal((n, width)).astype(np.float32)) for _ in range(3))
    want = time_rows_backward(gs, ts, n_table, max_t, width)
    twin = time_rows_backward_f32(gs, ts, n_table, max_t, width)
    return SimpleNamespace(n=n, width=width, n_table=n_table, max_t=max_t, ts=_frozen(ts), gs=gs, want=_frozen(want),
                           twin=_frozen(twin), d32=float(row_errors(twin, want).max()))


# ---- the forward gathers ----
ROWS_WIDTHS = (3, 4, 48, 50)
ROWS_N = (0, 1, 255, 256, 257)
ROWS_N_TABLE, ROWS_MAX_T = 12, 8


@functools.lru_cache(maxsize=None)
def rows_case(n, width):
    """a 12-row table of which frames 0..8 are in use; frame indices at both clamps, at the table's end and outside the table"""
    rng = np.random.default_rng(3200 + 1000 * width + n)
    table = _frozen(rng.standard_normal((ROWS_N_TABLE, width)).astype(np.float32))
    ts = _ts_edges(rng, n, ROWS_N_TABLE, ROWS_MAX_T) if n else np.zeros(0, np.int64)
    return SimpleNamespace(n=n, width=width, table=table, ts=_frozen(ts), n_table=ROWS_N_TABLE, max_t=ROWS_MAX_T,
                           next=_frozen(time_rows(table, ts, ROWS_MAX_T, 1)), prev=_frozen(time_rows(table, ts, ROWS_MAX_T, -1)))


# =====================================================================================================================
# flow glue
# =====================================================================================================================
Z_FAR = float(np.float32(0.95))
FLOW_P = (1, 255, 256, 257, 1000)
# (col_a, cotangents of a, col_b, cotangents of b, accumulate)
FLOW_FORMS = ((8, 4, 11, 1, False), (11, 1, 8, 4, True), (0, 1, 13, 1, False), (5, 4, -1, 0, True), (-1, 0, 2, 4, False),
              (8, 0, 11, 1, True), (8, 4, 11, 4, False))
FLOW_DEFECT_FORMS = {"mask_ge": 0, "fourth_cotangent": 0, "group_b_over_a": 0}


def flow_grad(zs, z_far, prior, accumulate, col_a, g_a, col_b, g_b, defect=None, absolute=False):
    """(P, 16) float64.  prior: the record before the call (used in accumulate form only); g_a / g_b: lists of (P, 3)."""
    assert defect is None or defect in FLOW_DEFECTS
    zs = np.asarray(zs, np.float64)
    with np.errstate(invalid="ignore"):
        far = (zs >= z_far) if defect == "mask_ge" else (zs > z_far)
    keep = np.where(far, 0.0, 1.0)[:, None]
    P = zs.shape[0]
    prior = np.asarray(prior, np.float64)
    out = (np.abs(prior) if absolute else prior.copy()) if accumulate else np.zeros((P, 16), np.float64)

    def total(gs):
        gs = list(gs)[:3] if (defect == "fourth_cotangent" and len(gs) == 4) else list(gs)
        s = np.zeros((P, 3), np.float64)
        for g in gs:
            s += np.abs(np.asarray(g, np.float64)) if absolute else np.asarray(g, np.float64)
        return s
    sa, sb = total(g_a), total(g_b)
    if defect == "group_b_over_a" and col_a >= 0 and col_b >= 0:
        sa = sb
    if col_a >= 0:
        out[:, col_a:col_a + 3] += keep * sa
    if col_b >= 0:
        out[:, col_b:col_b + 3] += keep * sb
    return out


@functools.lru_cache(maxsize=None)
def flow_case(P, form):
    col_a, n_a, col_b, n_b, accumulate = FLOW_FORMS[form]
    rng = np.random.default_rng(3300 + 100 * form + P)
    zs = rng.uniform(0.0, 1.2, size=P).astype(np.float32)
    # depths exactly at z_far (kept), one fp32 step above (dropped) and NaN (kept), wherever there is room
    special = [np.float32(Z_FAR), np.nextafter(np.float32(Z_FAR), np.float32(2.0)), np.float32("nan"),
               np.nextafter(np.float32(Z_FAR), np.float32(0.0))]
    where = rng.permutation(P)[:len(special)]
    zs[where] = special[:len(where)]
    if P > 8:
        assert 0 < int((zs > Z_FAR).sum()) < P
    g_a = tuple(_frozen(_ints(rng, -7, 7, P, 3)) for _ in range(n_a))
    g_b = tuple(_frozen(_ints(rng, -7, 7, P, 3)) for _ in range(n_b))
    prior = _frozen(_ints(rng, -100, 100, P, 16))
    c = SimpleNamespace(P=P, form=form, col_a=col_a, col_b=col_b, accumulate=accumulate, zs=_frozen(zs), g_a=g_a, g_b=g_b,
                        prior=prior, at_far=int(where[0]), above=int(where[1]) if P > 1 else None, nan=int(where[2]) if P > 2 else None)
    c.want = _frozen(flow_grad(zs, Z_FAR, prior, accumulate, col_a, g_a, col_b, g_b))
    c.abs_terms = float(flow_grad(zs, Z_FAR, prior, accumulate, col_a, g_a, col_b, g_b, absolute=True).max())
    return c


# =====================================================================================================================
# fold
# =====================================================================================================================
HEADS_R = (1, 3, 4, 10, 16)
DENSE_R = (1, 3, 4, 5, 10, 128, 255, 256)
DENSE_LDS = ((256, 256), (283, 283), (331, 256))          # (ld_head, ld_dhead): 283 = 256 + 27, 331 = 256 + 27 + 48
LD_MAX = 331


def fold(g, gb, w_head, w_final, b_final, g2=None, gb2=None, defect=None, absolute=False):
    """(dW_head (R, 256), db_head (R), dW_final (256, 256), db_final (256)) in float64; w_head (R, 256).
    absolute: every term replaced by its absolute value, |g| + |g2| for G -- the bound of every partial sum."""
    assert defect is None or defect in FOLD_DEFECTS
    f = (lambda x: np.abs(np.asarray(x, np.float64))) if absolute else (lambda x: np.asarray(x, np.float64))
    G, GB = f(g), f(gb)
    if defect != "no_remainder_rows":
        G = G + (0.0 if g2 is None else f(g2))
        GB = GB + (0.0 if gb2 is None else f(gb2))
    wh, wf, bf = f(w_head), f(w_final), f(b_final)
    d_w_head = G @ wf.T + (0.0 if defect == "no_bias_term" else np.outer(GB, bf))
    return d_w_head, GB.copy(), wh.T @ G, wh.T @ GB


@functools.lru_cache(maxsize=None)
def fold_case(R):
    """the inputs of both fold kernels at R rows: g / gb with their remainder rows g2 / gb2, the folded layer's weights as an
    (R, LD_MAX) matrix (its first 256 columns are W_head; a launch with a smaller row stride takes a re-laid copy), *_final, and
    integer prior gradients for every output"""
    rng = np.random.default_rng(3400 + R)
    c = SimpleNamespace(R=R,
                        g=_frozen(_ints(rng, -7, 7, R, 256)), g2=_frozen(_ints(rng, -3, 3, R, 256)),
                        gb=_frozen(_ints(rng, -7, 7, R)), gb2=_frozen(_ints(rng, -3, 3, R)),
                        w_head=_frozen(_ints(rng, -7, 7, R, LD_MAX)),
                        w_final=_frozen(_ints(rng, -7, 7, 256, 256)), b_final=_frozen(_ints(rng, -7, 7, 256)),
                        prior_w_head=_frozen(_ints(rng, -100, 100, R, LD_MAX)), prior_b_head=_frozen(_ints(rng, -100, 100, R)),
                        prior_w_final=_frozen(_ints(rng, -100, 100, 256, 256)), prior_b_final=_frozen(_ints(rng, -100, 100, 256)))
    assert np.abs(c.g2).max() > 0 and np.abs(c.gb2).max() > 0 and min(np.abs(c.prior_b_head).max(), np.abs(c.prior_b_final).max()) > 0
    terms = fold(c.g, c.gb, c.w_head[:, :256], c.w_final, c.b_final, c.g2, c.gb2, absolute=True)
    c.abs_terms = 100.0 + max(float(t.max()) for t in terms)
    return c


def fold_dense(c, ld_head, ld_dhead, with_g2, accumulate, defect=None):
    """What nsff_fold_grads_dense leaves in its four output buffers, in float64: d_w_head as a FLAT buffer of (R - 1) ld_dhead +
    256 floats (the floats between the rows' 256 columns keep what they held), d_b_head (R), d_w_final (256, 256), d_b_final
    (256).  Before the call the buffers hold the case's prior gradients (accumulate) or NaN (store)."""
    R = c.R
    dwh, dbh, dwf, dbf = fold(c.g, c.gb, c.w_head[:, :256], c.w_final, c.b_final, c.g2 if with_g2 else None,
                              c.gb2 if with_g2 else None, defect)
    size = (R - 1) * ld_dhead + 256
    if accumulate:
        buf = np.zeros(R * LD_MAX, np.float64)
        buf[:R * ld_dhead] = c.prior_w_head[:, :ld_dhead].astype(np.float64).reshape(-1)
        buf = buf[:size].copy()
        out_b, out_wf, out_bf = (np.asarray(v, np.float64).copy() for v in (c.prior_b_head, c.prior_w_final, c.prior_b_final))
    else:
        buf = np.full(size, np.nan)
        out_b, out_wf, out_bf = np.full(R, np.nan), np.full((256, 256), np.nan), np.full(256, np.nan)
    rows = range(R - R % FOLD_ROWS) if defect == "row_tail" else range(R)
    ld = ld_head if defect == "ld_mixup" else ld_dhead
    for r in rows:
        at = r * ld
        if at + 256 > size:
            continue                                          # (a defective stride runs past the buffer: those rows are lost)
        buf[at:at + 256] = (buf[at:at + 256] if accumulate else 0.0) + dwh[r]
        out_b[r] = (out_b[r] if accumulate else 0.0) + dbh[r]
    out_wf = (out_wf if accumulate else 0.0) + dwf
    out_bf = (out_bf if accumulate else 0.0) + dbf
    return buf, out_b, out_wf, out_bf


def head_split(R):
    """how the R folded rows are spread over separate head tensors: 3 + 1 + 3 + 3 as the dynamic trunk's rgb / sigma / flow_fw /
    flow_bw heads, then threes"""
    sizes, left = [], R
    for k in (3, 1, 3, 3, 3, 3):
        if left <= 0:
            break
        sizes.append(min(k, left))
        left -= sizes[-1]
    assert sum(sizes) == R
    return sizes


def fold_heads(c):
    """What nsff_fold_grads adds: the priors plus the fold of rows r and 16 + r, as (d_w_head (R, 256), d_b_head (R), d_w_final,
    d_b_final) in float64; and the (32, 256) / (32) job with NaN in every row the kernel must not read."""
    R = c.R
    g32, gb32 = np.full((32, 256), np.nan, np.float32), np.full(32, np.nan, np.float32)
    g32[:R], g32[16:16 + R], gb32[:R], gb32[16:16 + R] = c.g, c.g2, c.gb, c.gb2
    dwh, dbh, dwf, dbf = fold(c.g, c.gb, c.w_head[:, :256], c.w_final, c.b_final, c.g2, c.gb2)
    want = (c.prior_w_head[:, :256].astype(np.float64) + dwh, c.prior_b_head.astype(np.float64) + dbh,
            c.prior_w_final.astype(np.float64) + dwf, c.prior_b_final.astype(np.float64) + dbf)
    return g32, gb32, want


# =====================================================================================================================
# absmax
# =====================================================================================================================
ABSMAX_N = (0, 1, 3, 4, 5, 1023, 1025, 2 ** 20 + 3, 2 ** 21 + 7)     # the last: a second trip of the grid-stride loop as well
ABSMAX_PLANTS = ("first", "last", "last_aligned")


@functools.lru_cache(maxsize=None)
def absmax_case(n, plant):
    """values in (-1, 1) with -0.0 among them and ONE element of larger magnitude, negative, at the first, the last or the last
    element of the float4 part"""
    rng = np.random.default_rng(3500 + n % 9973)
    x = rng.uniform(-1.0, 1.0, size=n).astype(np.float32)
    if n:
        x[n // 2] = -0.0
        at = {"first": 0, "last": n - 1, "last_aligned": max(4 * (n // 4) - 1, 0)}[plant]
        x[at] = -5.5
    return SimpleNamespace(n=n, x=_frozen(x), want=np.float32(np.abs(x).max()) if n else np.float32(0.0))
