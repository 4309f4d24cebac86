"""A NumPy restatement of DESIGN 4.22, B1 - B7 (letterbox / pillarbox bars), written from the definition - not from edvr_amd/bars.py or
csrc/bars.hip.  Integers only.  Boxes are (top, bottom, left, right): rows [top, bottom), columns [left, right); rects (y0, x0, h, w)."""
import numpy as np

import deint_ref as D


def profile(frames, H, W, fmt):
    """B1: int64 (n, H + W) - per frame the H row sums of the luma plane, then its W column sums."""
    luma = D.split(frames, H, W, fmt)[0]
    return np.concatenate([luma.sum(axis=2), luma.sum(axis=1)], axis=1).astype(np.int64)


def frame_boxes(table, H, W, depth, limit=24):
    """B2, B3."""
    level = limit << (depth - 8)
    out = []
    for row in np.asarray(table, dtype=np.int64).reshape(-1, H + W):
        dark_rows, dark_cols = row[:H] <= level * W, row[H:] <= level * H
        t = H if dark_rows.all() else int(np.argmin(dark_rows))  # the first row that is not dark
        l = W if dark_cols.all() else int(np.argmin(dark_cols))
        if t == H or l == W:
            out.append(None)
            continue
        b, r = int(np.argmin(dark_rows[::-1])), int(np.argmin(dark_cols[::-1]))
        out.append((t, H - b, l, W - r))
    return out


def video_box(boxes):
    """B4."""
    have = np.array([b for b in boxes if b is not None], dtype=np.int64).reshape(-1, 4)
    if not len(have):
        return None
    return int(have[:, 0].min()), int(have[:, 1].max()), int(have[:, 2].min()), int(have[:, 3].max())


def axis(lo, hi, N, step, m, g=0):
    """B5 for one axis: (a, len0, o, len)."""
    if lo > 0:
        lo += g
    if hi < N:
        hi -= g
    a = (lo + step - 1) // step * step
    e = hi // step * step
    len0 = e - a
    length = (len0 // m) * m  # floor
    o = a + ((len0 - length) // (2 * step)) * step
    return a, len0, o, length


def aligned_rect(box, H, W, step, multiple, margin=0, min_bar=8):
    """B5, B6; step and multiple as (rows, columns)."""
    if box is None:
        return None
    t, b, l, r = box
    got = []
    for lo, hi, N, s, m in ((t, b, H, step[0], multiple[0]), (l, r, W, step[1], multiple[1])):
        _, _, o, length = axis(lo, hi, N, s, m, margin)
        if N - length < min_bar:
            o, length = 0, N
        got.append((o, length))
    (y0, h), (x0, w) = got
    if 2 * h < H or 2 * w < W:
        return None
    return y0, x0, h, w


def outside(boxes, rect, tolerance=2):
    y0, x0, h, w = rect
    return [i for i, b in enumerate(boxes) if b is not None and
            (y0 - b[0] > tolerance or b[1] - (y0 + h) > tolerance or x0 - b[2] > tolerance or b[3] - (x0 + w) > tolerance)]


def crop(frames, H, W, fmt, rect):
    """B7: uint8 (n, framesize of h x w) - NumPy slices of the three planes."""
    sx, sy, _ = D.parse_format(fmt)
    y0, x0, h, w = rect
    assert y0 % (1 << sy) == 0 and h % (1 << sy) == 0 and x0 % (1 << sx) == 0 and w % (1 << sx) == 0
    Y, Cb, Cr = D.split(frames, H, W, fmt)
    cy, cx, ch, cw = y0 >> sy, x0 >> sx, h >> sy, w >> sx
    return D.join([Y[:, y0:y0 + h, x0:x0 + w], Cb[:, cy:cy + ch, cx:cx + cw], Cr[:, cy:cy + ch, cx:cx + cw]], fmt)
