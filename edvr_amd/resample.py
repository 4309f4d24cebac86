"""Host tables of ops.resample (csrc/resample.hip): the taps and weights of one axis by DESIGN 4.21, R1 - R5, in NumPy float64, and the
small cache that keeps one uploaded copy of each table per (I, O, kernel, device).  The project's own definition - no bit-compatibility
with swscale, zimg or PIL is claimed:

    R1  kernels K of radius a: 'lanczos3' (a = 3, K(0) = 1, K(x) = 3 sin(pi x) sin(pi x / 3) / (pi x)^2 for |x| < 3), 'bicubic' (Keys,
        -0.5, a = 2: the polynomial of csrc/resize.hip), 'bilinear' (a = 1); zero outside the radius
    R2  pixel centres aligned: u_j = ((2 j + 1) I - O) / (2 O), integer numerator, one float64 division; f = max(1, I / O) stretches
        the filter when reducing
    R3  T = ceil(2 a f) + 1 taps per output sample, the first at first_j = floor(u_j - a f) + 1, w_{j,t} = K((first_j + t - u_j) / f) in
        float64, divided by the row's sum (added in tap order), then rounded to float32
    R4  the tap index first_j + t is clamped into [0, I - 1] - by the kernel, so the tables stay rectangular
    R5  O == I is the identity: one tap of weight 1
"""
from collections import OrderedDict

import numpy as np

KERNELS = {'lanczos3': 3, 'bicubic': 2, 'bilinear': 1}  # name -> radius a (R1)
MAX_RATIO = 8   # 1 / 8 <= I / O <= 8 per axis
MAX_TAPS = 49   # T at I / O = 8 with 'lanczos3'


def _lanczos3(x):
    px = np.pi * x
    with np.errstate(divide='ignore', invalid='ignore'):
        k = 3.0 * np.sin(px) * np.sin(px / 3.0) / (px * px)
    return np.where(x == 0.0, 1.0, np.where(np.abs(x) < 3.0, k, 0.0))


def _bicubic(x):
    a = np.abs(x)
    a2 = a * a
    a3 = a2 * a
    return np.where(a <= 1.0, 1.5 * a3 - 2.5 * a2 + 1.0, np.where(a < 2.0, -0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0, 0.0))


def _bilinear(x):
    return np.maximum(1.0 - np.abs(x), 0.0)


_K = {'lanczos3': _lanczos3, 'bicubic': _bicubic, 'bilinear': _bilinear}


def check_axis(I, O, what='axis'):
    """ValueError unless I and O are positive and 1 / 8 <= I / O <= 8."""
    if I < 1 or O < 1:
        raise ValueError(f'resample: {what} of {I} samples cannot become {O}')
    if I > MAX_RATIO * O or O > MAX_RATIO * I:
        raise ValueError(f'resample: {what} ratio {I} / {O} is outside [1/{MAX_RATIO}, {MAX_RATIO}]')


def taps(I, O, kernel='lanczos3'):
    """T of R3 (1 for the identity axis of R5), in integers."""
    if kernel not in KERNELS:
        raise ValueError(f'kernel must be one of {sorted(KERNELS)}, got {kernel!r}')
    check_axis(I, O)
    a = KERNELS[kernel]
    if O == I:
        return 1
    return (-(-2 * a * I // O) if I > O else 2 * a) + 1


def axis_table(I, O, kernel='lanczos3'):
    """(first, weights) of an axis of I samples resampled to O: first int32 (O,), weights float32 (O, T), by R1 - R5."""
    I, O = int(I), int(O)
    T = taps(I, O, kernel)
    if O == I:
        return np.arange(O, dtype=np.int32), np.ones((O, 1), dtype=np.float32)
    a = float(KERNELS[kernel])
    f = max(1.0, I / O)
    j = np.arange(O, dtype=np.int64)
    u = ((2 * j + 1) * I - O).astype(np.float64) / np.float64(2 * O)
    first = np.floor(u - a * f).astype(np.int64) + 1
    w = np.empty((O, T), dtype=np.float64)
    total = np.zeros(O, dtype=np.float64)
    for t in range(T):
        w[:, t] = _K[kernel](((first + t).astype(np.float64) - u) / f)
        total = total + w[:, t]
    return first.astype(np.int32), (w / total[:, None]).astype(np.float32)


_CACHE = OrderedDict()  # (I, O, kernel, device) -> (first, weights, T) on the device
_CACHE_SIZE = 16        # two axes per stream: eight streams' worth


def device_table(I, O, kernel, device):
    """The axis table on `device`, uploaded once per (I, O, kernel, device): after a stream's first chunk a call finds both of its
    tables here, allocates nothing for them and waits for nothing."""
    import torch
    key = (int(I), int(O), kernel, str(device))
    hit = _CACHE.get(key)
    if hit is None:
        first, w = axis_table(I, O, kernel)
        hit = (torch.from_numpy(first).to(device), torch.from_numpy(w).to(device), w.shape[1])
        _CACHE[key] = hit
        while len(_CACHE) > _CACHE_SIZE:
            _CACHE.popitem(last=False)
    else:
        _CACHE.move_to_end(key)
    return hit
