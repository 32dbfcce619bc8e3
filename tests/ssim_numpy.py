"""float64 numpy restatement of the reference's SSIM metric (metrics.py:19-33 over kornia 0.5.4's ssim_loss).

Restated from kornia 0.5.4 (kornia/losses/ssim.py, kornia/filters/filter.py::filter2d,
kornia/filters/kernels.py::get_gaussian_kernel2d), which is not vendored here:
  window  outer product of two normalised 1-D Gaussians, sigma 1.5, x = arange(11) - 5
  filter  11x11 correlation after F.pad(mode='reflect') by 5 (np.pad 'reflect': the edge pixel is not repeated)
  ssim    (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2) + 1e-12),  C1 = 0.01^2, C2 = 0.03^2
  loss    clamp((1 - ssim) / 2, 0, 1)          (LOSS_FORM; releases before 0.5.4: clamp(1 - ssim, 0, 1) / 2)
The reference's metric is 1 - loss.
"""
import numpy as np

WINDOW, SIGMA, HALF = 11, 1.5, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def gauss1d():
    x = np.arange(WINDOW, dtype=np.float64) - HALF
    g = np.exp(-x ** 2 / (2 * SIGMA ** 2))
    return g / g.sum()


def kernel2d():
    g = gauss1d()
    return np.outer(g, g)


def loss_form(ssim):
    """kornia 0.5.4's form -- the one place the choice between the two forms is made."""
    return np.clip((1 - ssim) / 2, 0, 1)


def loss_form_pre_054(ssim):
    return np.clip(1 - ssim, 0, 1) / 2


def filter2d(img):
    """(H, W) -> (H, W): kornia filter2d with border_type='reflect'."""
    H, W = img.shape
    p = np.pad(img, HALF, mode="reflect")
    k = kernel2d()
    out = np.zeros((H, W))
    for i in range(WINDOW):
        for j in range(WINDOW):
            out += k[i, j] * p[i:i + H, j:j + W]
    return out


def ssim_index(x, y):
    """Per-pixel SSIM (not the loss) of two (H, W) planes."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mu1, mu2 = filter2d(x), filter2d(y)
    s11 = filter2d(x * x) - mu1 ** 2
    s22 = filter2d(y * y) - mu2 ** 2
    s12 = filter2d(x * y) - mu1 * mu2
    return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s11 + s22 + C2) + 1e-12)


def ssim_loss(gt, pred):
    """(H, W, 3) pair -> (H, W, 3) kornia ssim_loss(reduction='none')."""
    return np.stack([loss_form(ssim_index(gt[..., c], pred[..., c])) for c in range(gt.shape[-1])], -1)


def ssim(gt, pred, valid_mask=None, reduction="mean"):
    """metrics.py:19-33 in float64."""
    value = ssim_loss(np.asarray(gt, np.float64), np.asarray(pred, np.float64))
    if valid_mask is not None:
        value = value[np.asarray(valid_mask, bool)]
    if reduction == "mean":
        return 1 - value.mean()
    return 1 - value


def reflect(i, n):
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def ssim_loss_direct(gt, pred, pixels=None):
    """The same by an explicit 11x11 double loop per pixel with explicit reflect indexing (slow: test reference only).
    pixels: iterable of (y, x) or None = all; returns {(y, x): (3,) loss}."""
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    H, W, _ = gt.shape
    k = kernel2d()
    pixels = [(y, x) for y in range(H) for x in range(W)] if pixels is None else pixels
    out = {}
    for (y, x) in pixels:
        loss = np.zeros(3)
        for c in range(3):
            m = np.zeros(5)
            for i in range(WINDOW):
                yy = reflect(y + i - HALF, H)
                for j in range(WINDOW):
                    xx = reflect(x + j - HALF, W)
                    a, b = gt[yy, xx, c], pred[yy, xx, c]
                    m += k[i, j] * np.array([a, b, a * a, b * b, a * b])
            s11, s22, s12 = m[2] - m[0] ** 2, m[3] - m[1] ** 2, m[4] - m[0] * m[1]
            s = (2 * m[0] * m[1] + C1) * (2 * s12 + C2) / ((m[0] ** 2 + m[1] ** 2 + C1) * (s11 + s22 + C2) + 1e-12)
            loss[c] = loss_form(s)
        out[(y, x)] = loss
    return out
