"""`nsff_composite_backward` (csrc/rays_bwd.hip) and its forward twin `nsff_composite` (csrc/rays.hip) called directly, against
float64 autograd of the plain expression in tests/composite_ref.py, on the cases of that module: 1 / 5 / 9 rays (a last
workgroup of one wave), S = 1, 2 and both sides of every 64-sample chunk boundary up to 200 (260 for the forward), the four
forms (static; transient with flow_mode 0, 1, 2), noise given / NULL / scaled by 0, saturated samples on the chunk boundary, at
sample 0 and at S - 2, an empty ray, equal depths, softplus's linear branch.

The rule and where its tolerance comes from are in composite_ref.py: per gradient tensor, column group and ray, relative to
that ray's largest reference value, bound max(8 x d32, 16 x 2^-24) with d32 the CPU float32 evaluation's own distance from
float64 -- never a figure of the kernel under test.  Figures measured on the MI355X are in EXPERIMENTS.md R17.
"""
import ctypes as C
import functools

import pytest
import torch

import composite_ref as R
from nsff_pl_amd import _lib

pytestmark = pytest.mark.gpu

TAIL = 64                                     # records behind every output buffer that must stay untouched
NAN = float("nan")
INVALID, NULL, ALIGN = -1, -2, -3             # NSFF_ERR_* of include/nsff_render.h
BWD_FIELDS = {name for name, _ in _lib.CompositeBwdArgs._fields_}
FORWARD_NAMES = {"so_rgb": "static_only_rgb", "so_depth": "static_only_depth"}       # output of nsff_composite <- name here


def _dev(t):
    return t.cuda().contiguous()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def backward_tensors(c, cot, rays=slice(None)):
    """the pointer arguments of one nsff_composite_backward call on rays `rays` of case c (cot: name -> tensor or None) and the
    NaN-filled outputs, TAIL records longer than needed"""
    n = c.zs[rays].shape[0]
    P = n * c.S
    tens = dict(raw=_dev(c.raw[rays]), zs=_dev(c.zs[rays]))
    if c.noise_given:
        tens.update(noise_static=_dev(c.noise["static"][rays]), noise_transient=_dev(c.noise["transient"][rays]),
                    noise_fw=_dev(c.noise["fw"][rays]), noise_bw=_dev(c.noise["bw"][rays]))
    if c.flow_mode >= 1:
        tens.update(xyz=_dev(c.xyz[rays]), f_fw=_dev(c.f_fw[rays]), f_bw=_dev(c.f_bw[rays]))
    if c.flow_mode >= 2:
        tens.update(raw_fw=_dev(c.raw_fw[rays]), raw_bw=_dev(c.raw_bw[rays]))
    for k, g in cot.items():
        tens["g_" + k] = None if g is None else _dev(g[rays])
    outs = dict(d_raw=_nan(P + TAIL, 16))
    if c.flow_mode >= 1:
        outs.update(d_f_fw=_nan(P + TAIL, 3), d_f_bw=_nan(P + TAIL, 3))
    if c.flow_mode >= 2:
        outs.update(d_raw_fw=_nan(P + TAIL, 16), d_raw_bw=_nan(P + TAIL, 16))
    tens["scratch"] = _nan(P, 4)
    assert set(tens) | set(outs) <= BWD_FIELDS
    return n, tens, outs


def run_backward(c, cot=None, rays=slice(None)):
    """the full output buffers (tail included) of one launch, on the CPU"""
    n, tens, outs = backward_tensors(c, c.cot if cot is None else cot, rays)
    _lib.composite_backward(n, c.S, c.has_transient, c.flow_mode, c.noise_std, **tens, **outs)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in outs.items()}


@functools.lru_cache(maxsize=None)
def kernel_gradients(key):
    """one launch per case, shared by the gradient and the hygiene test"""
    return run_backward(R.make_case(*key))


def head(c, buf):
    """the (n, S, C) records of a buffer that the call owns"""
    return buf[:c.n * c.S].view(c.n, c.S, -1)


def bits(t):
    return t.contiguous().view(torch.int32)


def _report(tag, form, rows):
    """rows: (key, name, error, bound, d32).  Fails on the cases outside their bound; prints the figures R17 records."""
    bad = [(k, n, f"err {e:.3g} bound {b:.3g} d32 {d:.3g}") for k, n, e, b, d in rows if not e <= b]
    used = max(rows, key=lambda r: r[2] / r[3])
    live = [r for r in rows if R.FACTOR * r[4] > R.FLOOR]
    line = f"R17 {tag} {form}: {len(rows)} figures, worst error / bound {used[2] / used[3]:.3g} at {used[0]} {used[1]}"
    if live:
        top = max(live, key=lambda r: r[2] / r[4])
        line += f"; worst error / d32 (where 8 d32 is the bound) {top[2] / top[4]:.3g} at {top[0]} {top[1]} (d32 {top[4]:.3g})"
    print(line)
    assert not bad, f"{len(bad)} of {len(rows)} outside the bound: {bad[:12]}"


# ---- gradients ----
def backward_rows(form):
    rows = []
    for key in R.backward_keys(form):
        ref = R.reference(key)
        c = ref.case
        got = {k: head(c, v) for k, v in kernel_gradients(key).items()}
        rows += [(key, f"{t}.{g}", e, b, d) for (t, g), (e, b, d) in R.gradient_errors(ref, got).items()]
    return rows


@pytest.mark.parametrize("form", R.FORM_NAMES)
def test_gradients_against_float64(hip_lib, form):
    _report("backward", form, backward_rows(form))


@pytest.mark.parametrize("form", R.FORM_NAMES)
def test_record_hygiene(hip_lib, form):
    """slots the kernel owns but has nothing for are exactly 0, the records behind the call's are untouched, nothing is NaN / inf"""
    for key in R.backward_keys(form):
        c = R.make_case(*key)
        got = kernel_gradients(key)
        assert set(got) == {"d_raw"} | ({"d_f_fw", "d_f_bw"} if c.flow_mode >= 1 else set()) | \
            ({"d_raw_fw", "d_raw_bw"} if c.flow_mode >= 2 else set())
        for name, buf in got.items():
            assert torch.isnan(buf[c.n * c.S:]).all(), (key, name, "tail written")
            assert torch.isfinite(buf[:c.n * c.S]).all(), (key, name, "non-finite")
        zero = lambda t: bool((bits(t) == 0).all())                  # +0.0, not -0.0
        d_raw = head(c, got["d_raw"])
        assert zero(d_raw[..., 8:16]), key
        if not c.has_transient:
            assert zero(d_raw[..., 4:8]), key
        for name in ("d_raw_fw", "d_raw_bw"):
            if name in got:
                assert zero(head(c, got[name])[..., 0:4]) and zero(head(c, got[name])[..., 8:16]), (key, name)


# ---- absent cotangents ----
@pytest.mark.parametrize("form", R.FORM_NAMES)
def test_absent_cotangents_equal_zero_cotangents(hip_lib, form):
    """NULL for a g_* is bit for bit a zero tensor, for three random subsets per form (the others stay random)"""
    c = R.make_case(R.N_SWEEP, 129, form, "given")
    g = torch.Generator().manual_seed(1234 + R.FORM_NAMES.index(form))
    seen = set()
    for _ in range(3):
        while True:
            drop = frozenset(k for k in c.names if torch.rand((), generator=g) < 0.5)
            if 0 < len(drop) < len(c.names) and drop not in seen:
                break
        seen.add(drop)
        absent = run_backward(c, {k: (None if k in drop else v) for k, v in c.cot.items()})
        zeros = run_backward(c, {k: (torch.zeros_like(v) if k in drop else v) for k, v in c.cot.items()})
        for name in absent:
            assert torch.equal(bits(absent[name][:c.n * c.S]), bits(zeros[name][:c.n * c.S])), (sorted(drop), name)
        full = kernel_gradients(c.key)
        assert any(not torch.equal(bits(absent[k][:c.n * c.S]), bits(full[k][:c.n * c.S])) for k in absent), sorted(drop)


# ---- linearity over rays ----
@pytest.mark.parametrize("form", R.FORM_NAMES)
def test_a_ray_s_result_does_not_depend_on_its_wave(hip_lib, form):
    """9 rays in one launch (waves 0-3 of two workgroups, wave 0 of a third) = the same rays launched one at a time, bit for bit"""
    c = R.make_case(9, 129, form, "given")
    whole = run_backward(c)
    for r in range(c.n):
        one = run_backward(c, rays=slice(r, r + 1))
        for name, buf in one.items():
            assert torch.isnan(buf[c.S:]).all()
            assert torch.equal(bits(buf[:c.S]), bits(whole[name][r * c.S:(r + 1) * c.S])), (r, name)


# ---- the forward twin ----
def run_forward(c):
    n, S = c.n, c.S
    kw = dict(n_rays=n, n_samples=S, has_transient=c.has_transient, has_rgb=1, flow_mode=c.flow_mode, want_disocc=0,
              noise_std=c.noise_std, z_far=R.Z_FAR, raw=_dev(c.raw), zs=_dev(c.zs))
    if c.noise_given:
        kw.update(noise_static=_dev(c.noise["static"]), noise_transient=_dev(c.noise["transient"]),
                  noise_fw=_dev(c.noise["fw"]), noise_bw=_dev(c.noise["bw"]))
    if c.flow_mode >= 1:
        kw["xyz"] = _dev(c.xyz)
    if c.flow_mode >= 2:
        kw.update(raw_fw=_dev(c.raw_fw), raw_bw=_dev(c.raw_bw), xyz_fw=torch.zeros(n, S, 3, device="cuda"),
                  xyz_bw=torch.zeros(n, S, 3, device="cuda"))
    ref = R.reference(c.key)
    outs = {k: _nan(*ref.out[k].shape) for k in c.names}
    kw.update({FORWARD_NAMES.get(k, k): v for k, v in outs.items()})
    assert all(k in _lib._COMPOSITE_PTRS_OUT for k in (FORWARD_NAMES.get(k, k) for k in outs))
    _lib.composite(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in outs.items()}


def forward_rows(form, env):
    """env: setenv / delenv like pytest's monkeypatch.  (rows of the default form, rows of the serial form where the two differ)"""
    rows, serial_rows = [], []
    for key in R.forward_keys(form):
        ref = R.reference(key)
        c = ref.case
        got = run_forward(c)
        rows += [(key, k, e, b, d) for k, (e, b, d) in R.output_errors(ref, got).items()]
        if 65 <= c.S <= 256:
            env.setenv("NSFF_SERIAL_COMPOSITE", "1")
            try:
                serial = run_forward(c)
            finally:
                env.delenv("NSFF_SERIAL_COMPOSITE")
            serial_rows += [(key, k, e, b, d) for k, (e, b, d) in R.output_errors(ref, serial).items()]
            for k in ("static_sigmas", "transient_sigmas", "static_weights", "transient_weights", "weights"):
                if k in got:
                    assert torch.equal(bits(got[k]), bits(serial[k])), (key, k)
    return rows, serial_rows


@pytest.mark.parametrize("form", R.FORM_NAMES)
def test_forward_values_against_float64(hip_lib, form, monkeypatch):
    """the training-form outputs of nsff_composite under the same rule, in the default form (serial for S <= 64 and S > 256,
    one wave per chunk between) and, where the two differ, in the serial form too; the weights of the two forms are bit-identical"""
    rows, serial_rows = forward_rows(form, monkeypatch)
    _report("forward", form, rows)
    _report("forward-serial", form, serial_rows)


# ---- refusals ----
def test_refusals_touch_nothing(hip_lib):
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    c = R.make_case(R.N_SWEEP, 65, "transient_warp", "given")

    def call(n_rays=None, n_samples=None, has_transient=None, flow_mode=None, edit=None):
        n, tens, outs = backward_tensors(c, c.cot)
        a = _lib.CompositeBwdArgs(n_rays=n if n_rays is None else n_rays, n_samples=c.S if n_samples is None else n_samples,
                                  has_transient=c.has_transient if has_transient is None else has_transient,
                                  flow_mode=c.flow_mode if flow_mode is None else flow_mode, noise_std=c.noise_std)
        for k, v in {**tens, **outs}.items():
            setattr(a, k, _lib._ptr(v))
        if edit:
            edit(a)
        rc = lib.nsff_composite_backward(C.byref(a), stream)
        torch.cuda.synchronize()
        assert all(torch.isnan(v).all() for v in list(outs.values()) + [tens["scratch"]]), "a refused call wrote"
        return rc

    def drop(name):
        return lambda a: setattr(a, name, None)

    def shift_scratch(a):
        a.scratch = a.scratch + 4                      # (inside the buffer: never dereferenced anyway)
    assert call(n_samples=0) == INVALID
    assert call(flow_mode=3) == INVALID
    assert call(flow_mode=1, has_transient=0) == INVALID
    assert call(edit=drop("scratch")) == NULL
    assert call(flow_mode=1, edit=drop("f_fw")) == NULL
    assert call(edit=drop("d_raw_bw")) == NULL
    assert call(edit=shift_scratch) == ALIGN
    empty = _lib.CompositeBwdArgs(n_rays=0, n_samples=c.S, has_transient=1, flow_mode=2, noise_std=1.0)
    assert lib.nsff_composite_backward(C.byref(empty), stream) == 0
