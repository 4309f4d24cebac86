"""References and case tables for the PSNR / SSIM kernels (edvr_amd/csrc/metrics.hip), shared by tests/test_metrics_refs_cpu.py,
tests/test_gpu_metrics_edges.py and oracle/make_golden.py::metrics_edges_case.  Nothing here needs a GPU or imports GPU code.

PSNR is compared as the per-image SUM of squared differences, the quantity the kernel returns: for RGB an integer (sse_rgb_ref, exact),
for the Y channel the float32 difference and float32 square of every pixel summed in float64 (sse_y_ref, the kernel's own definition -
the reference takes a float32 mean of the same squares, which is why PSNR on Y is only compared at 1e-4 dB).  SSIM's reference is
oracle.edvr_oracle.ssim_cropped (2-D window, float64); ssim_separable restates the kernel's algorithm (horizontal then vertical 11-tap
pass over five moments) in NumPy float64.

Every input is seeded from zlib.crc32(repr(case)): the same case gives the same tensors in every process and on every machine."""
import os
import zlib

import numpy as np
import torch

from oracle import edvr_oracle as EO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics_edges.pt')
F32 = np.float32

KINDS = ('rand', 'wide', 'ties', 'const', 'black_white', 'checker', 'checker_inv', 'ramp_noise', 'inf', 'identical')

# (h, w, crop): what it reaches in ssim_kernel (16 x 16 tiles of the valid region, 26 x 26 input window per tile)
SSIM_GEOMS = (
    (11, 11, 0),  # valid region 1 x 1: one live thread in one tile
    (13, 43, 1),  # valid 1 x 31: two tiles, the right one 15 wide
    (26, 26, 0),  # valid 16 x 16: exactly one full tile
    (27, 42, 0),  # valid 17 x 32: bottom tiles one row high, right tile exactly full
    (58, 75, 0),  # valid 48 x 65: 3 x 5 tiles, interior tiles with all eight neighbours, last column one pixel wide
    (40, 44, 7),  # cropped to 26 x 30, valid 16 x 20: crop offset plus clamped loads
)
# (h, w, crop): what it reaches in psnr_sse_kernel (256 threads, 4096 pixels of the UNCROPPED image per block, at most 256 blocks)
PSNR_GEOMS = (
    (1, 1, 0),        # smallest image
    (3, 3, 1),        # one pixel left after the crop
    (64, 64, 0),      # 4096 pixels: exactly one block
    (64, 65, 0),      # two blocks taking turns of 256 pixels, the last turn 64 pixels long
    (70, 70, 30),     # two blocks sized from 4900 pixels, 100 pixels after the crop: block 1 receives nothing
    (1032, 1024, 0),  # above 1,048,576 pixels: the 256-block cap and a block stride of 65,536
    (1032, 1024, 5),  # the same with a crop
)
PSNR_LARGE_KINDS = ('rand', 'black_white')
MODES = ((3, False), (3, True), (1, False), (1, True))  # (c, test_y_channel); the flag is ignored for c = 1, as the reference ignores it


def psnr_n(h, w):
    return 1 if h * w > 1 << 20 else 3


def psnr_kinds(h, w):
    return PSNR_LARGE_KINDS if h * w > 1 << 20 else KINDS


def seed_of(case):
    return zlib.crc32(repr(case).encode())


# ------------------------------------------------------------------------------------------------ geometry, as the wrappers compute it
def ssim_tiles(h, w, crop):
    """(vh, vw, tiles_y, tiles_x) of calculate_ssim: the valid region after the crop and the 11 x 11 window, in 16 x 16 tiles"""
    vh, vw = h - 2 * crop - 10, w - 2 * crop - 10
    return vh, vw, -(-vh // 16), -(-vw // 16)


def psnr_blocks(h, w):
    """gridDim.x of psnr_sse_kernel as sum_squared_error_uint8 sizes it: from h * w, not from the cropped area"""
    return max(1, min(256, (h * w + 4095) // 4096))


def psnr_block_pixels(h, w, crop):
    """pixels each block of psnr_sse_kernel receives: pixel i of the cropped area goes to block (i // 256) % blocks"""
    blocks, npx = psnr_blocks(h, w), (h - 2 * crop) * (w - 2 * crop)
    return np.bincount((np.arange(npx) // 256) % blocks, minlength=blocks)


# ------------------------------------------------------------------------------------------------ content
def _checker(h, w):
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2).astype(F32)


def make_pair(kind, n, c, h, w, salt=0):
    """(pred, gt): two (n, c, h, w) float32 tensors of content `kind`, seeded from the arguments."""
    assert kind in KINDS, kind
    rng = np.random.default_rng(seed_of((kind, n, c, h, w, salt)))
    shape = (n, c, h, w)
    if kind in ('rand', 'inf'):
        pred, gt = rng.random(shape, F32), rng.random(shape, F32)
        if kind == 'inf':  # one pixel per image to +inf, another to -inf (where the image has another): tensor2img clamps them to 255 and 0
            hot = (h // 2) * w + w // 2
            cold = (hot + 1) % (h * w)
            flat = pred.reshape(n, c, h * w)
            flat[:, 0, hot] = np.inf
            if (c - 1, cold) != (0, hot):
                flat[:, c - 1, cold] = -np.inf
    elif kind == 'wide':  # about half the pixels clamp, on both sides
        pred, gt = (2 * rng.standard_normal(shape)).astype(F32), (2 * rng.standard_normal(shape)).astype(F32)
    elif kind == 'ties':  # x 255 in float32 is exactly k + 0.5: np.round sends it to the even neighbour
        pred, gt = (ties_from_k(rng.integers(0, 255, shape)) for _ in range(2))
    elif kind == 'const':
        pred, gt = np.full(shape, 1.0, F32), np.full(shape, 128 / 255, F32)
    elif kind == 'black_white':
        pred, gt = np.zeros(shape, F32), np.ones(shape, F32)
    elif kind in ('checker', 'checker_inv'):
        ck = _checker(h, w)
        pred = np.broadcast_to(ck, shape).copy()
        if kind == 'checker_inv':
            gt = 1 - pred
        else:  # the checkerboard shifted by one pixel, edge replicated: right in channel 0, down in channel 1, both in channel 2
            gt = np.empty(shape, F32)
            for k in range(c):
                dy, dx = ((0, 1), (1, 0), (1, 1))[k]
                gt[:, k] = ck[np.maximum(np.arange(h) - dy, 0)][:, np.maximum(np.arange(w) - dx, 0)]
    elif kind == 'ramp_noise':
        ramp = (np.arange(h * w, dtype=np.float64) / (h * w)).reshape(h, w)
        pred, gt = ((ramp + 0.01 * rng.standard_normal(shape)).astype(F32) for _ in range(2))
    else:  # identical: every byte agrees (x 255 stays 0.25 away from k + 0.5, the perturbation moves it by 0.003), no float does
        pred = ((rng.integers(0, 256, shape) + rng.uniform(-0.25, 0.25, shape)) / 255).astype(F32)
        gt = pred + np.where(rng.random(shape) < 0.5, F32(-1e-5), F32(1e-5)).astype(F32)
    return torch.from_numpy(np.ascontiguousarray(pred)), torch.from_numpy(np.ascontiguousarray(gt))


def ties_from_k(k):
    """float32((k + 0.5) / 255) for integer k in 0..254 (any shape): the `ties` content, and how metrics_edges.pt stores it (as the bytes k)"""
    k = np.asarray(k)
    assert k.min() >= 0 and k.max() <= 254
    return ((k.astype(np.float64) + 0.5) / 255).astype(F32)


def take_channels(t, c):
    return t[:, :c].contiguous()


# ------------------------------------------------------------------------------------------------ references
def _crop(a, crop):
    return a[..., crop:a.shape[-2] - crop, crop:a.shape[-1] - crop]


def sse_rgb_ref(pred, gt, crop=0):
    """int64 (n,): sum over the crop of the squared differences of the tensor2img bytes.  Exact."""
    d = EO.tensor2img_uint8(pred).numpy().astype(np.int64) - EO.tensor2img_uint8(gt).numpy().astype(np.int64)
    d = _crop(d.reshape((-1,) + d.shape[-3:]), crop)
    return (d * d).sum(axis=(1, 2, 3))


def y_ref(img):
    """float32 (h, w): the Y plane of one (3, h, w) RGB tensor exactly as oracle.edvr_oracle.psnr_cropped builds it - bytes as float32 / 255,
    float64 dot with (24.966, 128.553, 65.481) in B, G, R order, + 16, / 255, cast to float32, x 255 in float32"""
    assert img.dim() == 3 and img.shape[0] == 3
    f = EO.tensor2img_uint8(img).numpy().astype(F32) / 255.
    y = np.dot(np.moveaxis(f[::-1], 0, -1), [24.966, 128.553, 65.481]) + 16.0
    out = (y / 255.).astype(F32) * 255.
    assert out.dtype == F32
    return out


def sse_y_ref(pred, gt, crop=0):
    """float64 (n,): float32 difference and float32 square per pixel of the two Y planes, summed in float64 (the kernel's definition)"""
    pred, gt = (t.reshape((-1,) + t.shape[-3:]) for t in (pred, gt))
    out = []
    for p, g in zip(pred, gt):
        d = _crop(y_ref(p), crop) - _crop(y_ref(g), crop)
        sq = d * d
        assert sq.dtype == F32
        out.append(sq.astype(np.float64).sum())
    return np.array(out, np.float64)


def sse_ref(pred, gt, crop=0, test_y_channel=False):
    """([SSE per image as float], element count) as metrics.sum_squared_error_uint8 returns them"""
    n, c, h, w = pred.shape
    y = test_y_channel and c == 3
    sse = sse_y_ref(pred, gt, crop) if y else sse_rgb_ref(pred, gt, crop)
    return [float(s) for s in sse], (h - 2 * crop) * (w - 2 * crop) * (1 if y else c)


def psnr_of(sse, count):
    import math
    mse = sse / count
    return float('inf') if mse == 0 else 20.0 * math.log10(255.0 / math.sqrt(mse))


def ssim_planes(img, crop=0, test_y_channel=False):
    """float64 (planes, h - 2 crop, w - 2 crop): what calculate_ssim filters - the bytes of every channel, or the one Y plane"""
    if test_y_channel and img.shape[0] == 3:
        return _crop(y_ref(img), crop)[None].astype(np.float64)
    return _crop(EO.tensor2img_uint8(img).numpy(), crop).astype(np.float64)


def ssim_window():
    k = np.exp(-0.5 / 1.5 ** 2 * (np.arange(11) - 5.0) ** 2)
    return k / k.sum()


def ssim_separable(pred, gt, crop=0, test_y_channel=False):
    """SSIM of ONE image pair (c, h, w) the way ssim_kernel computes it, in NumPy float64: per plane the five moments (a, b, a^2, b^2, ab)
    through a horizontal 11-tap pass and then a vertical one, the SSIM map over the valid region, its mean; mean over planes."""
    g = ssim_window()
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2

    def filt(m):
        hp = sum(g[k] * m[:, k:m.shape[1] - 10 + k] for k in range(11))
        return sum(g[k] * hp[k:hp.shape[0] - 10 + k] for k in range(11))
    vals = []
    for x, y in zip(ssim_planes(pred, crop, test_y_channel), ssim_planes(gt, crop, test_y_channel)):
        mu1, mu2, xx, yy, xy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
        s1, s2, s12 = xx - mu1 * mu1, yy - mu2 * mu2, xy - mu1 * mu2
        vals.append((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean())
    return float(np.mean(vals))


# ------------------------------------------------------------------------------------------------ the golden of the reference itself
GOLDEN_CASES = tuple((kind, h, w, crop) for (h, w, crop) in ((27, 42, 0), (40, 44, 7)) for kind in ('ties', 'wide', 'inf', 'const')
                     if not (kind == 'const' and crop))


def load_golden(path=GOLDEN):
    """[dict(kind, h, w, crop_border, pred, gt (1, 3, h, w) float32, psnr {flag: float}, ssim {flag: float})] of tests/golden/metrics_edges.pt.
    To stay small the file holds `ties` as the bytes k of float32((k + 0.5) / 255) and `const` as one value per tensor."""
    out = []
    for case in torch.load(path)['cases']:
        case = dict(case)
        if 'pred_k' in case:
            case['pred'], case['gt'] = (torch.from_numpy(ties_from_k(case.pop(key).numpy())) for key in ('pred_k', 'gt_k'))
        case['pred'], case['gt'] = (case[key].expand(1, 3, case['h'], case['w']).contiguous() for key in ('pred', 'gt'))
        out.append(case)
    return out
