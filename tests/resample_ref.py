"""The NumPy restatement of DESIGN 4.21, R1 - R7 - what ops.resample is compared with, bit for bit.  It shares no code with
edvr_amd/resample.py: the tables are formed here again, and the two passes are two loops over taps on whole arrays, every sum in float64
in tap order from 0 and rounded to float32 once per pass."""
import numpy as np

RADIUS = {'lanczos3': 3, 'bicubic': 2, 'bilinear': 1}


def kernel_value(name, x):
    """R1: K(x) for a float64 array x."""
    if name == 'lanczos3':
        px = np.pi * x
        with np.errstate(divide='ignore', invalid='ignore'):
            k = 3.0 * np.sin(px) * np.sin(px / 3.0) / (px * px)
        return np.where(x == 0.0, 1.0, np.where(np.abs(x) < 3.0, k, 0.0))
    if name == 'bicubic':
        a = np.abs(x)
        a2 = a * a
        a3 = a2 * a
        return np.where(a <= 1.0, 1.5 * a3 - 2.5 * a2 + 1.0, np.where(a < 2.0, -0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0, 0.0))
    if name == 'bilinear':
        return np.maximum(1.0 - np.abs(x), 0.0)
    raise ValueError(name)


def table(I, O, kernel):
    """R2, R3, R5: (first int64 (O,), weights float32 (O, T))."""
    if O == I:
        return np.arange(O, dtype=np.int64), np.ones((O, 1), dtype=np.float32)
    a = RADIUS[kernel]
    f = max(1.0, I / O)
    T = (-((-2 * a * I) // O) if I > O else 2 * a) + 1             # ceil(2 a f) + 1, in integers
    j = np.arange(O, dtype=np.int64)
    u = ((2 * j + 1) * I - O).astype(np.float64) / np.float64(2 * O)   # integer numerator, one division
    first = np.floor(u - a * f).astype(np.int64) + 1
    w = np.empty((O, T), dtype=np.float64)
    total = np.zeros(O, dtype=np.float64)
    for t in range(T):                                                # the row's sum, added in tap order
        w[:, t] = kernel_value(kernel, ((first + t).astype(np.float64) - u) / f)
        total = total + w[:, t]
    return first, (w / total[:, None]).astype(np.float32)


def _pass(x, first, w, I):
    """R4, R6 along the LAST axis of float32 x (..., I): float32 (..., O)."""
    acc = np.zeros(x.shape[:-1] + (first.shape[0],), dtype=np.float64)
    for t in range(w.shape[1]):
        idx = np.clip(first + t, 0, I - 1)
        acc = acc + w[:, t].astype(np.float64) * x[..., idx].astype(np.float64)
    return acc.astype(np.float32)


def resample(x, size, kernel='lanczos3'):
    """float32 (n, c, H, W) -> float32 (n, c, Ho, Wo): columns first, then rows (R6); every frame on its own (R7)."""
    x = np.asarray(x, dtype=np.float32)
    ho, wo = size
    H, W = x.shape[-2:]
    fx, wx = table(W, wo, kernel)
    fy, wy = table(H, ho, kernel)
    mid = _pass(x, fx, wx, W)                                 # (n, c, H, Wo)
    out = _pass(np.swapaxes(mid, -1, -2), fy, wy, H)          # (n, c, Wo, Ho)
    return np.ascontiguousarray(np.swapaxes(out, -1, -2))


def interior(I, O, kernel):
    """bool (O,): the output samples whose taps all lie inside [0, I - 1] - where R4 plays no part."""
    first, w = table(I, O, kernel)
    return (first >= 0) & (first + w.shape[1] - 1 <= I - 1)
