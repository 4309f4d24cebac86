"""Inputs shared by the bar tests (test_bars_cpu.py, test_gpu_bars.py): designed clips - a picture of random samples inside a box, bars at
limited-range black around it - random frames, and a Y4M stream around frames."""
import numpy as np

import deint_ref as D
from util_telecine import random_frames, y4m_bytes  # noqa: F401  (the same random frames and Y4M wrapper as the telecine tests)

FORMATS = ['420', '422', '444', '420p10', '444p16']


def designed_clip(boxes, H, W, fmt='420', seed=0):
    """uint8 (n, framesize): frame i shows random luma samples of 64 << sh ... 235 << sh (far above any limit: with a picture of more than
    a sixth of an axis every picture row and column is bright in the mean, bars included) inside boxes[i] = (top, bottom, left, right)
    and 16 << sh - limited-range black - outside it; a box of None is a blank frame.  Chroma is random everywhere: the crop must carry
    exactly the samples under the rect."""
    rng = np.random.default_rng(seed)
    sh = D.parse_format(fmt)[2] - 8
    (R, C), chroma = D.plane_shapes(H, W, fmt)[0], D.plane_shapes(H, W, fmt)[1]
    luma = np.full((len(boxes), R, C), 16 << sh, np.int64)
    for i, box in enumerate(boxes):
        if box is not None:
            t, b, l, r = box
            luma[i, t:b, l:r] = rng.integers(64 << sh, (235 << sh) + 1, size=(b - t, r - l))
    cb, cr = (rng.integers(16 << sh, (240 << sh) + 1, size=(len(boxes),) + chroma) for _ in range(2))
    return D.join([luma, cb, cr], fmt)


def letterbox(H, W, bar):
    return bar, H - bar, 0, W


def pillarbox(H, W, bar):
    return 0, H, bar, W - bar


def windowbox(H, W, bar_y, bar_x):
    return bar_y, H - bar_y, bar_x, W - bar_x


def compositions(n):
    """Every way to cut n frames into consecutive pieces: lists of piece lengths (2^(n - 1) of them)."""
    out = []
    for mask in range(1 << (n - 1)):
        sizes, run = [], 1
        for k in range(n - 1):
            if mask >> k & 1:
                sizes.append(run)
                run = 1
            else:
                run += 1
        out.append(sizes + [run])
    return out
