"""The LPIPS 0.1 graph (net='alex', lpips=True, spatial=True, eval mode) restated with torch.nn.functional on the CPU, in any
dtype -- the float64 form is what the GPU tests compare against -- and seeded random weights of AlexNet's shapes (no weight file
is committed; the published weights are about 10 MB and not available to the tests).

    x = 2 x - 1 (normalize);  (x - shift) / scale
    conv 3->64 k11 s4 p2 + ReLU = f1;  maxpool 3 s2, conv 64->192 k5 p2 + ReLU = f2;  maxpool 3 s2, conv 192->384 k3 p1 + ReLU = f3;
    conv 384->256 k3 p1 + ReLU = f4;  conv 256->256 k3 p1 + ReLU = f5
    n = f / (sqrt(sum_c f^2) + 1e-10);  m_l = sum_c w_l[c] (n0 - n1)^2;  bilinear upsample to (H, W), align_corners=False;  sum_l
"""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CONV = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))   # cin, cout, k, stride, pad
POOL_BEFORE = (False, True, True, False, False)
FEATURE_INDEX = (0, 3, 6, 8, 10)


def random_weights(seed):
    """{'conv_w': [5], 'conv_b': [5], 'lin': [5]} fp32 CPU tensors: conv weights ~ N(0, 2 / fan_in), biases uniform in
    [-0.05, 0.05], lin weights (1, C, 1, 1) uniform in [0, 1 / C]."""
    g = torch.Generator().manual_seed(seed)
    w = {"conv_w": [], "conv_b": [], "lin": []}
    for cin, cout, k, _, _ in CONV:
        fan_in = cin * k * k
        w["conv_w"].append(torch.randn(cout, cin, k, k, generator=g) * (2.0 / fan_in) ** 0.5)
        w["conv_b"].append(torch.rand(cout, generator=g) * 0.1 - 0.05)
        w["lin"].append(torch.rand(1, cout, 1, 1, generator=g) / cout)
    return w


def lpips_state_dict(w):
    """The weights under the keys of the public ``lpips`` package's LPIPS(net='alex') module."""
    sd = {}
    for l, i in enumerate(FEATURE_INDEX):
        sd[f"net.slice{l + 1}.{i}.weight"] = w["conv_w"][l]
        sd[f"net.slice{l + 1}.{i}.bias"] = w["conv_b"][l]
        sd[f"lin{l}.model.1.weight"] = w["lin"][l]
    return sd


def torchvision_state_dict(w):
    """The weights under torchvision AlexNet's keys, with the lin keys beside them."""
    sd = {}
    for l, i in enumerate(FEATURE_INDEX):
        sd[f"features.{i}.weight"] = w["conv_w"][l]
        sd[f"features.{i}.bias"] = w["conv_b"][l]
        sd[f"lin{l}.model.1.weight"] = w["lin"][l]
    return sd


def features(x, w, dtype):
    """The five ReLU outputs of (B, 3, H, W) images that are already scaled."""
    taps = []
    for l, (_, _, _, stride, pad) in enumerate(CONV):
        if POOL_BEFORE[l]:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w["conv_w"][l].to(dtype), w["conv_b"][l].to(dtype), stride=stride, padding=pad))
        taps.append(x)
    return taps


def lpips_map(in0, in1, w, dtype=torch.float64, normalize=True):
    """in0 / in1 (B, 3, H, W) -> (B, 1, H, W) in `dtype`, every step computed in `dtype`."""
    in0, in1 = in0.to(dtype), in1.to(dtype)
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    f0, f1 = features((in0 - shift) / scale, w, dtype), features((in1 - shift) / scale, w, dtype)
    H, W = in0.shape[2:]
    total = 0
    for l in range(5):
        n0 = f0[l] / (torch.sqrt(torch.sum(f0[l] ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = f1[l] / (torch.sqrt(torch.sum(f1[l] ** 2, dim=1, keepdim=True)) + 1e-10)
        m = F.conv2d((n0 - n1) ** 2, w["lin"][l].to(dtype))
        total = total + F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)
    return total


def image_pairs(seed, F_, H, W):
    """(gt, pred) (F, H, W, 3) fp32 in [0, 1]: smooth colour ramps with noise, and a prediction that differs by a blur-like
    perturbation -- the kind of pair the metric is for."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([xx, yy, 0.5 + 0.5 * torch.sin(6 * (xx + yy))], -1)
    gt = (base[None] * (0.6 + 0.4 * torch.rand(F_, 1, 1, 3, generator=g)) + 0.15 * torch.rand(F_, H, W, 3, generator=g)).clamp(0, 1)
    pred = (gt + 0.08 * torch.randn(F_, H, W, 3, generator=g)).clamp(0, 1)
    return gt.contiguous(), pred.contiguous()
