"""CPU checks of the ray-bank builder (nsff_ray_records, nsff_pl_amd/frames.py): the numpy restatement of tests/records_ref.py
and ``projection_matrices`` against golden g24 (the reference's own ray generation, tests/golden/make_golden_records.py), the
C-ABI's argument validation (no launch), the Python layer's refusals, and the bank's full-frame sample."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import parity
import records_ref
from nsff_pl_amd import _lib, frames
from nsff_pl_amd.sampling import RayBank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_TOL = 1e-5          # the bar of test_frame_rays_match_reference, the same arithmetic
PS_TOL = 1e-6           # both sides compute in float64 and round once to fp32 (ulp 6e-8); the inverse may differ in a last place


@pytest.fixture(scope="module")
def g24():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g24_ray_records.npz")))


def test_golden_scene_is_the_one_described(g24):
    F, H, W = g24["images"].shape[:3]
    assert (F, H, W) == (3, 19, 33) and g24["records"].shape == (3, 627, 16) and g24["Ps"].shape == (1, 3, 3, 4)
    assert np.array_equal(g24["K"], [[37, 0, 16.5], [0, 41, 9.5], [0, 0, 1]])
    assert g24["poses"][:, 2, 3].tolist() == [0.3, -1.7, -1.0]
    assert g24["images"].dtype == np.uint8 and g24["masks"].dtype == np.uint8
    assert np.abs(g24["flows_fw"][F - 1]).min() > 0 and np.abs(g24["flows_bw"][0]).min() > 0   # the slots a builder ignores
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g24_ray_records.npz")) < 200_000


def test_restatement_reproduces_the_golden_records(g24):
    got = records_ref.records(g24["K"], g24["poses"], g24["images"], g24["disps"], g24["masks"], g24["flows_fw"],
                              g24["flows_bw"])
    want = g24["records"]
    for t in range(len(want)):
        err = parity.assert_close(f"frame {t} ndc rays", got[t, :, :6], want[t, :, :6], RAY_TOL)
        print(f"frame {t}: ray columns max-norm rel err {err:.2e}")
    assert np.array_equal(got[..., 6:], want[..., 6:])
    uv = records_ref.uv_grid(19, 33)
    assert np.array_equal(want[2, :, 12:14], uv) and np.array_equal(want[0, :, 14:16], uv)
    nofl = records_ref.records(g24["K"], g24["poses"], g24["images"], g24["disps"], g24["masks"])
    assert np.array_equal(nofl[..., 12:14], np.broadcast_to(uv, (3, 627, 2)))
    assert np.array_equal(nofl[..., 14:16], np.broadcast_to(uv, (3, 627, 2)))


def test_projection_matrices_match_the_golden(g24):
    Ks, Ps = frames.projection_matrices(g24["K"], g24["poses"])
    assert Ks.dtype == Ps.dtype == torch.float32 and tuple(Ks.shape) == (1, 3, 3) and tuple(Ps.shape) == (1, 3, 3, 4)
    assert np.array_equal(Ks[0].numpy(), g24["K"].astype(np.float32))
    err = parity.max_rel_err(Ps.numpy(), g24["Ps"])
    print(f"Ps max-norm rel err {err:.2e}")
    assert err <= PS_TOL
    assert parity.max_rel_err(records_ref.projection_matrices(g24["K"], g24["poses"])[None], g24["Ps"]) <= PS_TOL
    Kt, Pt = frames.projection_matrices(torch.tensor(g24["K"]), torch.tensor(g24["poses"]))       # tensors as well as arrays
    assert torch.equal(Kt, Ks) and torch.equal(Pt, Ps)
    with pytest.raises(ValueError, match="poses"):
        frames.projection_matrices(g24["K"], g24["poses"][0])


_BUF = (C.c_float * 80)()                                   # host memory: nothing is launched, nothing dereferenced
_P = (C.addressof(_BUF) + 15) & ~15


def _args(**kw):
    p = _P
    a = _lib.RayRecordArgs(n_frames=3, H=4, W=5, first_frame=0, frame_count=3, image_u8=1, mask_u8=1, fx=5, fy=5, cx=2.5,
                           cy=2, near=1, n_pixels=20, images=p, disps=p, masks=p, flow_fw=p, flow_bw=p, frame_table=p,
                           records=p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_abi_rejects_bad_arguments_without_a_launch():
    lib = _lib.load()
    call = lambda **kw: lib.nsff_ray_records(C.byref(_args(**kw)), None)
    assert lib.nsff_ray_records(None, None) == -2
    for name in ("images", "disps", "masks", "frame_table", "records"):
        assert call(**{name: None}) == -2, name
    for bad in (dict(n_pixels=21), dict(n_pixels=0), dict(H=0), dict(W=-1), dict(frame_count=-1), dict(first_frame=-1),
                dict(first_frame=1), dict(frame_count=4), dict(n_frames=-1), dict(n_frames=70000, frame_count=70000),
                dict(H=65536, W=32768, n_pixels=1 << 31)):
        assert call(**bad) == -1, bad
    # zero frames: OK without a launch, whatever the pointers are
    assert call(frame_count=0) == 0 and call(frame_count=0, first_frame=3) == 0
    assert call(frame_count=0, images=None, records=None) == 0 and call(n_frames=0, frame_count=0) == 0
    assert call(records=_P + 8) == -3 and call(flow_fw=_P + 4) == -3 and call(image_u8=0, images=_P + 1) == -3
    assert C.sizeof(_lib.RayRecordArgs) == 7 * 4 + 5 * 4 + 8 + 7 * 8


def test_header_declares_the_symbol_and_the_abi_is_unchanged():
    header = open(os.path.join(ROOT, "include", "nsff_render.h")).read()
    assert re.search(r"\bint nsff_ray_records\(const NsffRayRecordArgs\* args, void\* stream\);", header)
    assert "nsff_ray_records" in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), "nsff_ray_records")
    assert re.search(r"#define NSFF_ABI_VERSION\s+32\b", header)
    assert _lib.load().nsff_abi_version() == _lib.ABI_VERSION == 32
    assert int(re.search(r"#define NSFF_FRAME_TABLE\s+(\d+)", header).group(1)) == _lib.FRAME_TABLE


def _cpu_inputs(g24):
    return dict(images=torch.from_numpy(g24["images"]), disps=torch.from_numpy(g24["disps"]),
                masks=torch.from_numpy(g24["masks"]), flows_fw=torch.from_numpy(g24["flows_fw"]),
                flows_bw=torch.from_numpy(g24["flows_bw"]))


def test_build_records_refuses_cpu_tensors_and_other_layouts(g24):
    K, poses, x = g24["K"], g24["poses"], _cpu_inputs(g24)
    with pytest.raises(RuntimeError, match="GPU"):
        frames.build_records(K, poses, **x)
    with pytest.raises(RuntimeError, match="GPU"):
        frames.build_records(K, poses, **{k: list(v) for k, v in x.items()})                 # lists of per-frame tensors
    with pytest.raises(RuntimeError, match="GPU"):
        RayBank.from_frames(K, poses, x["images"], x["disps"], x["masks"], None, None, (33, 19))
    with pytest.raises(ValueError, match=r"channels-last \(F,H,W,3\).*\(F,3,H,W\)"):
        frames.build_records(K, poses, **dict(x, images=x["images"].permute(0, 3, 1, 2)))
    with pytest.raises(ValueError, match="images must be channels-last"):
        frames.build_records(K, poses, **dict(x, images=x["images"][0]))
    for name, bad in (("disps", x["disps"][:, :-1]), ("masks", x["masks"][:2]), ("flows_fw", x["flows_fw"][..., :1]),
                      ("flows_bw", x["flows_bw"].permute(0, 3, 1, 2))):
        with pytest.raises(ValueError, match=name):
            frames.build_records(K, poses, **dict(x, **{name: bad}))
    with pytest.raises(ValueError, match="poses"):
        frames.build_records(K, poses[:2], **x)
    with pytest.raises(TypeError, match="images"):
        frames.build_records(K, poses, **dict(x, images=g24["images"]))
    for name in ("images", "disps", "masks"):                    # a None entry is a missing flow, never a missing frame
        with pytest.raises(TypeError, match=f"{name} list"):
            frames.build_records(K, poses, **dict(x, **{name: [None] + list(x[name][1:])}))
    with pytest.raises(RuntimeError, match="GPU"):               # (a None flow entry passes the list check)
        frames.build_records(K, poses, **dict(x, flows_fw=list(x["flows_fw"][:2]) + [None]))


def test_frame_table_holds_poses_and_shift_near(g24):
    tab = frames.frame_table(g24["poses"], "cpu")
    assert tuple(tab.shape) == (3, _lib.FRAME_TABLE) and tab.dtype == torch.float32
    assert np.array_equal(tab[:, :12].numpy(), g24["poses"].astype(np.float32).reshape(3, 12))
    assert tab[:, 12].tolist() == [1.0, float(np.float32(1.7)), 1.0] and not tab[:, 13:].any()


def test_bank_full_frame_sample_and_moves(g24):
    """frame_sample reads the validation split's sample off the records; to() carries Ks / Ps when the bank has them."""
    bank = RayBank(g24["records"], (33, 19))
    assert bank.Ks is None and bank.Ps is None and bank.to("cpu").Ks is None
    s, r = bank.frame_sample(2), g24["records"][2]
    assert set(s) == {"rays", "ts", "rgbs", "disp", "mask"}
    assert s["ts"].dtype == torch.int64 and s["ts"].tolist() == [2] * 627
    for key, cols in (("rays", slice(0, 6)), ("rgbs", slice(6, 9)), ("disp", 10), ("mask", 11)):
        assert np.array_equal(s[key].numpy(), r[:, cols]), key
    assert np.array_equal(s["rgbs"].numpy(), g24["images"][2].reshape(-1, 3).astype(np.float32) / np.float32(255))
    bank.Ks, bank.Ps = frames.projection_matrices(g24["K"], g24["poses"])
    moved = bank.to(torch.device("cpu"))
    assert moved is bank and tuple(bank.Ps.shape) == (1, 3, 3, 4)
