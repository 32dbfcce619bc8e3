"""MI355X checks of the frame resize (nsff_frame_resize behind frames.resize_*): the Lanczos kernel against golden g28 (the
reference's own PIL statement, tests/golden/make_golden_resize.py) byte for byte; the gather and bilinear kernels bit-equal to
the numpy restatement tests/resize_numpy.py; batches, lists, per-kind source sizes, graph replay, the chain into build_records
and RayBank.from_frames(resize=True), and the refusals."""
import os

import numpy as np
import pytest
import torch

import resize_numpy as rn
from nsff_pl_amd import _lib, frames
from nsff_pl_amd.sampling import RayBank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
N_CASES = 7
SINGLE_PASS, IDENTITY = (2, 3), 4


@pytest.fixture(scope="module")
def g28():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g28_resize.npz")))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def wh(a):
    return int(a.shape[2]), int(a.shape[1])


def lanczos_into_prefilled(src, img_wh):
    """The kernel itself on an output prefilled with 0xAB (an unwritten byte shows), through the tables the library keeps."""
    W, H = img_wh
    F, h, w, ch = src.shape
    out = torch.full((F, H, W, ch), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.frame_resize(_lib.RESIZE_LANCZOS_U8, src, out, frames._table(DEV, _lib.RESIZE_LANCZOS_U8, w, W),
                      frames._table(DEV, _lib.RESIZE_LANCZOS_U8, h, H))
    return out


@pytest.mark.parametrize("i", range(N_CASES))
def test_lanczos_equals_the_reference_bytes(g28, hip_lib, i):
    src, want = dev(g28[f"c{i}/src"]), dev(g28[f"c{i}/dst"])
    got = lanczos_into_prefilled(src, wh(want))                    # (the identity too: both passes skipped, a copy through LDS)
    print(f"case {i}: {int((got != want).sum())} of {want.numel()} bytes differ")
    assert torch.equal(got, want)
    api = frames.resize_images(src, wh(want))
    assert api.dtype == torch.uint8 and api.is_contiguous() and torch.equal(api, want)
    if i == IDENTITY:
        assert api.data_ptr() != src.data_ptr() and torch.equal(api, src)
    if i in SINGLE_PASS:
        assert (src.shape[1] == want.shape[1]) != (src.shape[2] == want.shape[2])


@pytest.mark.parametrize("i", range(N_CASES))
def test_masks_equal_the_reference_bytes(g28, hip_lib, i):
    src, want = dev(g28[f"c{i}/mask_src"]), dev(g28[f"c{i}/mask_dst"])
    got = frames.resize_masks(src, wh(want))
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert got.data_ptr() != src.data_ptr()


def test_a_frame_is_the_same_alone_and_in_a_batch(g28, hip_lib):
    for i in (0, 5):
        src, want = dev(g28[f"c{i}/src"]), dev(g28[f"c{i}/dst"])
        batch = torch.cat([src, src.flip(0), src[:1]])
        got = frames.resize_images(batch, wh(want))
        assert torch.equal(got, torch.cat([want, want.flip(0), want[:1]]))
        for f in range(2):
            assert torch.equal(frames.resize_images(src[f:f + 1], wh(want)), want[f:f + 1])


def test_one_channel_is_each_channel_of_three(g28, hip_lib):
    for i in (0, 1, 6):
        src, want = dev(g28[f"c{i}/src"]), dev(g28[f"c{i}/dst"])
        for c in range(3):
            one = src[..., c:c + 1].contiguous()
            assert torch.equal(lanczos_into_prefilled(one, wh(want)), want[..., c:c + 1])
    assert frames.resize_images(dev(g28["c0/src"])[..., :1].contiguous(), (33, 19)).shape == (2, 19, 33, 1)


def _fields(rng, F, h, w):
    disp = rng.random((F, h, w), dtype=np.float32) * 40
    flow = (rng.standard_normal((F, h, w, 2)) * 7).astype(np.float32)
    return disp, flow


@pytest.mark.parametrize("h,w,H,W", [(45, 80, 19, 33), (23, 40, 31, 57), (40, 33, 19, 33), (19, 70, 19, 33), (37, 61, 150, 262),
                                     (150, 262, 70, 131), (5, 3, 1, 1), (1, 1, 4, 6)])
def test_disps_and_flows_equal_the_restatement_bit_for_bit(hip_lib, h, w, H, W):
    rng = np.random.default_rng(h * 1000 + W)
    disp, flow = _fields(rng, 3, h, w)
    got = frames.resize_disps(dev(disp), (W, H))
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), rn.resize_nearest_cv(disp, (W, H)).view(np.int32))
    got = frames.resize_flows(dev(flow), (W, H))
    want = rn.resize_flow(flow, (W, H))
    assert got.shape == (3, H, W, 2) and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def test_flow_and_nearest_properties(hip_lib):
    const = np.empty((1, 12, 20, 2), np.float32)
    const[..., 0], const[..., 1] = 3.0, -1.5
    # sizes whose lerp weights are dyadic (.25 / .75, .5 / .5, eighths): the lerp of a constant is then exact in fp32; at other
    # sizes (1 - fx) + fx need not be 1 in fp32 and the output is pinned by the restatement instead (the test above)
    for W, H in ((40, 24), (10, 6), (80, 48), (40, 6), (20, 24)):
        got = frames.resize_flows(dev(const), (W, H)).cpu().numpy()
        assert np.array_equal(got[..., 0], np.full((1, H, W), np.float32(3.0) * np.float32(W / 20)))       # constant x ratio
        assert np.array_equal(got[..., 1], np.full((1, H, W), np.float32(-1.5) * np.float32(H / 12)))
    rng = np.random.default_rng(5)
    flow = rng.standard_normal((1, 6, 9, 2)).astype(np.float32)
    got = frames.resize_flows(dev(flow), (27, 18)).cpu().numpy()                                           # 3x up: the border clamps
    ratio = np.float32(3.0)
    for (y, x), (sy, sx) in (((0, 0), (0, 0)), ((17, 26), (5, 8)), ((0, 26), (0, 8)), ((17, 0), (5, 0))):
        assert np.array_equal(got[0, y, x], flow[0, sy, sx] * ratio), (y, x)
    disp = rng.random((2, 10, 14), dtype=np.float32)
    got = frames.resize_disps(dev(disp), (7, 5)).cpu().numpy()                                             # 2x: pixels 0, 2, 4, ...
    assert np.array_equal(got, disp[:, ::2, ::2])
    same = frames.resize_disps(dev(disp), (14, 10))
    assert np.array_equal(same.cpu().numpy(), disp)
    same = frames.resize_flows(dev(flow), (9, 6))                                                          # resize_flow's early return
    assert np.array_equal(same.cpu().numpy(), flow)


def test_lists_and_per_kind_source_sizes(g28, hip_lib):
    rng = np.random.default_rng(11)
    img, mask = g28["c0/src"], g28["c1/mask_src"]                  # 45 x 80 images, 23 x 40 masks
    disp, _ = _fields(rng, 2, 37, 61)
    _, fw = _fields(rng, 2, 40, 33)
    _, bw = _fields(rng, 2, 19, 70)
    img_wh = (33, 19)
    d = frames.resize_frames(list(dev(img)), list(dev(disp)), dev(mask), [dev(fw)[0], None], list(dev(bw)), img_wh)
    assert sorted(d) == ["disps", "flows_bw", "flows_fw", "images", "masks"]
    assert torch.equal(d["images"], dev(g28["c0/dst"]))
    assert np.array_equal(d["masks"].cpu().numpy(), rn.resize_nearest_pil(mask, img_wh))
    assert np.array_equal(d["disps"].cpu().numpy(), rn.resize_nearest_cv(disp, img_wh))
    fw_holed = fw.copy()
    fw_holed[1] = 0
    assert np.array_equal(d["flows_fw"].cpu().numpy(), rn.resize_flow(fw_holed, img_wh))
    assert np.array_equal(d["flows_bw"].cpu().numpy(), rn.resize_flow(bw, img_wh))
    none = frames.resize_frames(dev(img), dev(disp), dev(mask), None, None, img_wh)
    assert none["flows_fw"] is None and none["flows_bw"] is None
    key = (str(DEV), _lib.RESIZE_LANCZOS_U8, 80, 33)
    table = frames._TABLES[key]
    frames.resize_images(dev(img), img_wh)
    assert frames._TABLES[key] is table and table[0].device == DEV                                       # built once, kept


def test_graph_capture_and_replay_on_new_data(g28, hip_lib):
    src, want = dev(g28["c0/src"]), dev(g28["c0/dst"])
    W, H = wh(want)
    xt, yt = frames._table(DEV, _lib.RESIZE_LANCZOS_U8, 80, W), frames._table(DEV, _lib.RESIZE_LANCZOS_U8, 45, H)
    out = torch.empty_like(want)
    call = lambda: _lib.frame_resize(_lib.RESIZE_LANCZOS_U8, src, out, xt, yt)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                     # warm-up outside the graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    src.copy_(src.flip(0))                                         # the frames change places
    out.fill_(0xAB)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want.flip(0))


def _scene(g28, rng):
    """Two frames: golden images (45 x 80), everything else synthetic at sizes of its own; target 33 x 19."""
    img, mask = g28["c0/src"], (g28["c0/mask_src"] > 127).astype(np.uint8) * 255
    disp, fw = _fields(rng, 2, 40, 70)
    _, bw = _fields(rng, 2, 23, 40)
    poses = np.tile(np.eye(3, 4, dtype=np.float32), (2, 1, 1))
    poses[:, :, 3] = rng.standard_normal((2, 3)).astype(np.float32) * 0.1
    K = frames.scaled_intrinsics(60.0, (80, 45), (33, 19))
    return K, poses, img, disp, mask, fw, bw


def test_resized_frames_build_the_restatements_records(g28, hip_lib):
    rng = np.random.default_rng(3)
    K, poses, img, disp, mask, fw, bw = _scene(g28, rng)
    img_wh = (33, 19)
    d = frames.resize_frames(dev(img), dev(disp), dev(mask), dev(fw), dev(bw), img_wh)
    got = frames.build_records(K, poses, **d)
    want = frames.build_records(K, poses, dev(rn.resize_lanczos(img, img_wh)), dev(rn.resize_nearest_cv(disp, img_wh)),
                                dev(rn.resize_nearest_pil(mask, img_wh)), dev(rn.resize_flow(fw, img_wh)),
                                dev(rn.resize_flow(bw, img_wh)))
    assert got.shape == (2, 19 * 33, 16) and torch.equal(got, want)
    rgb = (torch.from_numpy(g28["c0/dst"]).float() / 255).to(DEV)                                         # ToTensor, on the host
    assert torch.equal(got[..., 6:9].reshape(2, 19, 33, 3), rgb)                                         # the reference's rgb bits
    bank = RayBank.from_frames(K, poses, dev(img), dev(disp), dev(mask), dev(fw), dev(bw), img_wh, resize=True)
    assert torch.equal(bank.records, want)
    with pytest.raises(ValueError, match="build_records"):                                                # the default: today's errors
        RayBank.from_frames(K, poses, dev(img), dev(disp), dev(mask), dev(fw), dev(bw), img_wh)


def test_refusals(g28, hip_lib):
    src = dev(g28["c0/src"])
    with pytest.raises(RuntimeError, match="resize_images: images must be a GPU tensor"):
        frames.resize_images(src.cpu(), (33, 19))
    with pytest.raises(ValueError, match="channels-first"):
        frames.resize_images(src.permute(0, 3, 1, 2).contiguous(), (33, 19))
    with pytest.raises(TypeError, match="resize_images: images must be torch.uint8.*Lanczos"):
        frames.resize_images(src.float() / 255, (33, 19))
    with pytest.raises(RuntimeError, match="8x"):
        frames.resize_images(torch.zeros(1, 97, 40, 3, dtype=torch.uint8, device=DEV), (20, 12))
    with pytest.raises(TypeError, match="resize_disps: disps must be torch.float32"):
        frames.resize_disps(torch.zeros(1, 8, 8, dtype=torch.float64, device=DEV), (4, 4))
    with pytest.raises(ValueError, match="resize_flows: flows must be channels-last"):
        frames.resize_flows(torch.zeros(1, 8, 8, 3, device=DEV), (4, 4))
    with pytest.raises(ValueError, match="resize_masks: masks must be channels-last"):
        frames.resize_masks(torch.zeros(1, 8, 8, 1, dtype=torch.uint8, device=DEV), (4, 4))
    with pytest.raises(ValueError, match="differ in shape"):
        frames.resize_disps([torch.zeros(8, 8, device=DEV), torch.zeros(8, 9, device=DEV)], (4, 4))
    out = torch.empty(2, 19, 33, 3, dtype=torch.uint8, device=DEV)
    xt, yt = frames._table(DEV, _lib.RESIZE_LANCZOS_U8, 80, 33), frames._table(DEV, _lib.RESIZE_LANCZOS_U8, 45, 19)
    with pytest.raises(RuntimeError, match="NSFF_ERR_INVALID"):                                           # tables of another size pair
        _lib.frame_resize(_lib.RESIZE_LANCZOS_U8, src, out, frames._table(DEV, _lib.RESIZE_LANCZOS_U8, 160, 33), yt)
    with pytest.raises(RuntimeError, match="table has"):
        _lib.frame_resize(_lib.RESIZE_LANCZOS_U8, src, out[:, :, :30].contiguous(), xt, yt)
