"""NumPy restatement of the device part of NIQE (edvr_amd/csrc/niqe.hip), shared by tests/test_niqe_cpu.py, tests/test_gpu_niqe.py and
scripts/make_niqe_golden.py.  It follows basicsr/metrics/niqe.py:67-205 step by step - to_y_channel on float32, the MSCN map in float32
with the 49 products of each convolution accumulated in double and rounded once (what scipy.ndimage.convolve does on a float32 array),
the second scale as the 2 x 2 float32 mean - and differs from the reference in one place only: the five sums per map are float64.  The
host finish is edvr_amd.metrics.niqe_from_moments itself; nothing here needs scipy, OpenCV or a GPU.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
F32 = np.float32
BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def window():
    from edvr_amd import metrics
    return metrics.niqe_window()


def y_plane(img):
    """The plane calculate_niqe scores, float32 in [0, 255]: to_y_channel of (h, w, 3) RGB bytes (metric_util.py:34-47 on the BGR image),
    or the bytes of an (h, w) image as they are ('HW' order)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return img.astype(F32)
    f = img.astype(F32) / 255.
    d = np.dot(f[..., ::-1], [24.966, 128.553, 65.481]) + 16.0  # float64
    return (d / 255.).astype(F32) * 255.


def kept(plane, crop_border=0):
    """crop_border off every side, then the top-left 96 nbh x 96 nbw pixels; (rectangle, nbh, nbw)"""
    if crop_border:
        plane = plane[crop_border:-crop_border, crop_border:-crop_border]
    nbh, nbw = plane.shape[0] // BLOCK, plane.shape[1] // BLOCK
    return plane[:nbh * BLOCK, :nbw * BLOCK], nbh, nbw


def mscn(x, win=None):
    """z = (x - mu) / (sigma + 1) in float32; mu and E[x^2]: 7 x 7 window, mode='nearest', products summed in double in row-major tap
    order and rounded once to float32"""
    win = window() if win is None else win
    assert x.dtype == F32
    h, w = x.shape
    xp = np.pad(x, 3, mode='edge')
    x2 = xp * xp
    s1, s2 = np.zeros((h, w), np.float64), np.zeros((h, w), np.float64)
    for ky in range(7):
        for kx in range(7):
            s1 = s1 + win[ky, kx] * xp[ky:ky + h, kx:kx + w].astype(np.float64)
            s2 = s2 + win[ky, kx] * x2[ky:ky + h, kx:kx + w].astype(np.float64)
    mu, m2 = s1.astype(F32), s2.astype(F32)
    sigma = np.sqrt(np.abs(m2 - mu * mu))
    z = (x - mu) / (sigma + F32(1))
    assert z.dtype == F32
    return z


def half(x):
    """cv2.resize(x / 255., (w // 2, h // 2), INTER_LINEAR) * 255. for even sides: at the exact factor 1/2 the 2 x 2 mean, in x's dtype"""
    assert x.shape[0] % 2 == 0 and x.shape[1] % 2 == 0
    t = x.dtype.type
    u = x / 255.
    return ((u[0::2, 0::2] + u[0::2, 1::2]) + (u[1::2, 0::2] + u[1::2, 1::2])) * t(0.25) * 255.


def block_moments(block):
    """(5, 5) float64: per map (z, z roll(z, s)) sum v^2 over v < 0, #(v < 0), sum v^2 over v > 0, #(v > 0), sum |v|; v and v^2 float32"""
    out = np.zeros((5, 5), np.float64)
    maps = [block] + [block * np.roll(block, s, axis=(0, 1)) for s in SHIFTS]
    for m, v in enumerate(maps):
        assert v.dtype == F32
        sq = (v * v).astype(np.float64)
        out[m] = [sq[v < 0].sum(), (v < 0).sum(), sq[v > 0].sum(), (v > 0).sum(), np.abs(v).astype(np.float64).sum()]
    return out


def moments_of_plane(plane, crop_border=0):
    """(2, nbh nbw, 5, 5) float64 for one float32 plane, blocks in the reference's order (idx_w outer); also nbh, nbw"""
    x, nbh, nbw = kept(np.ascontiguousarray(plane, dtype=F32), crop_border)
    assert nbh >= 1 and nbw >= 1
    out = np.zeros((2, nbh * nbw, 5, 5), np.float64)
    for s, scale in enumerate((1, 2)):
        z, b = mscn(x), BLOCK // scale
        for iw in range(nbw):
            for ih in range(nbh):
                out[s, iw * nbh + ih] = block_moments(z[ih * b:(ih + 1) * b, iw * b:(iw + 1) * b])
        if scale == 1:
            x = half(x)
    return out, nbh, nbw


def moments(img, crop_border=0):
    """uint8 (h, w, 3) RGB or (h, w) grey -> (2, blocks, 5, 5), nbh, nbw"""
    return moments_of_plane(y_plane(img), crop_border)


def niqe(img, params, crop_border=0):
    from edvr_amd import metrics
    m, nbh, nbw = moments(img, crop_border)
    return metrics.niqe_from_moments(m[None], nbh, nbw, params)[0]


def load_cases():
    """tests/golden/niqe.pt: {'tol': float, 'cases': [{'name', 'img' uint8 (n, h, w, 3) | (n, h, w), 'crop_border', 'ref' [n], 'ref64' [n],
    'feat' (n, blocks, 36) float64}]}"""
    import torch
    return torch.load(os.path.join(GOLDEN, 'niqe.pt'), weights_only=True)


def chw_float(img):
    """uint8 (n, h, w, 3) | (n, h, w) -> float32 (n, 3 | 1, h, w) tensor in [0, 1] whose tensor2img bytes are `img`"""
    import torch
    t = torch.as_tensor(np.asarray(img))
    t = t.permute(0, 3, 1, 2) if t.dim() == 4 else t[:, None]
    return (t.to(torch.float32) / 255.).contiguous()
