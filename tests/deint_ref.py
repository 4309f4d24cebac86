"""The NumPy restatement of the deinterlacer's definition: a literal per-sample loop and a vectorised form, on one
plane and on whole frames of a Y4M format.  Both take the context frames `prev` / `next`.  Integers only; nothing here is tuned to the
kernel - it is written from the definition.

A clip of n frames is the fields F_k, k = 0 ... 2 n - 1; field k lives in frame k // 2 on the rows of parity (k + b) % 2, b = 0 for top
field first, 1 for bottom field first.  S(k, r, x) = row fold(r, R), column clamp(x) of the frame `field_frame` names."""
import numpy as np

ORDER = (0, -1, 1, -2, 2)  # D4: the directions in the order that breaks ties
FIRST = {'top': 0, 'bottom': 1}


def fold(i, size):
    """i reflected into [0, size - 1], repeatedly: period 2 (size - 1); size >= 2.  Keeps the parity of i."""
    period = 2 * (size - 1)
    m = i % period
    return period - m if m > size - 1 else m


def field_frame(k, n, has_prev, has_next):
    """The frame that holds field k: 0 ... n - 1, -1 for `prev`, n for `next`.  On a side without a context frame k reflects about that
    end of the batch (about 0, about 2 n - 1) - repeatedly; with neither this is fold(k, 2 n) // 2.  Keeps the parity of k."""
    last = 2 * n - 1
    while True:
        if k < 0 and not has_prev:
            k = -k
        elif k > last and not has_next:
            k = 2 * last - k
        else:
            assert -2 <= k <= last + 2
            return k // 2


def field_indices(n, mode):
    return list(range(2 * n)) if mode == 'field' else list(range(0, 2 * n, 2))


def _source(plane, prev, nxt, k):
    n = plane.shape[0]
    f = field_frame(k, n, prev is not None, nxt is not None)
    return prev if f < 0 else nxt if f >= n else plane[f]


def plane_loop(plane, maxv, first='top', mode='field', prev=None, nxt=None):
    """D1 - D6 sample by sample.  plane: integer (n, R, C); prev / nxt: (R, C) or None.  Returns int64 (2 n | n, R, C)."""
    plane = np.asarray(plane).astype(np.int64)
    prev = None if prev is None else np.asarray(prev).astype(np.int64)
    nxt = None if nxt is None else np.asarray(nxt).astype(np.int64)
    n, R, C = plane.shape
    assert R >= 2 and C >= 1 and n >= 1
    b = FIRST[first]

    def S(k, r, x):
        return int(_source(plane, prev, nxt, k)[fold(r, R), min(max(x, 0), C - 1)])

    ks = field_indices(n, mode)
    out = np.empty((len(ks), R, C), np.int64)
    for o, k in enumerate(ks):
        q = (k + b) % 2
        for y in range(R):
            for x in range(C):
                if y % 2 == q:
                    out[o, y, x] = plane[k // 2, y, x]  # D1
                    continue
                c, e = S(k, y - 1, x), S(k, y + 1, x)  # D2
                p, nx = S(k - 1, y, x), S(k + 1, y, x)
                dmid = (p + nx) >> 1
                t0 = abs(p - nx)  # D3
                t1 = (abs(S(k - 2, y - 1, x) - c) + abs(S(k - 2, y + 1, x) - e)) >> 1
                t2 = (abs(S(k + 2, y - 1, x) - c) + abs(S(k + 2, y + 1, x) - e)) >> 1
                diff = max(t0 >> 1, t1, t2)
                best = pred = None  # D4
                for j in ORDER:
                    score = sum(abs(S(k, y - 1, x + j + u) - S(k, y + 1, x - j + u)) for u in (-1, 0, 1)) + (1 if j else 0)
                    if best is None or score < best:
                        best, pred = score, (S(k, y - 1, x + j) + S(k, y + 1, x - j)) >> 1
                bb = (S(k - 1, y - 2, x) + S(k + 1, y - 2, x)) >> 1  # D5
                ff = (S(k - 1, y + 2, x) + S(k + 1, y + 2, x)) >> 1
                hi = max(dmid - e, dmid - c, min(bb - c, ff - e))
                lo = min(dmid - e, dmid - c, max(bb - c, ff - e))
                diff = max(diff, lo, -hi)
                v = min(max(pred, dmid - diff), dmid + diff)  # D6
                assert 0 <= v <= maxv, (v, maxv)
                out[o, y, x] = v
    return out


def plane_vec(plane, maxv, first='top', mode='field', prev=None, nxt=None, info=None):
    """The same, whole rows at a time.  info: a dict that receives, per missing sample of every output frame in order, 'j' (the direction
    D4 chose) and 'clamp' (-1: D6 raised pred to dmid - diff, +1: lowered it to dmid + diff, 0: left it), as flat int arrays."""
    plane = np.asarray(plane).astype(np.int64)
    prev = None if prev is None else np.asarray(prev).astype(np.int64)
    nxt = None if nxt is None else np.asarray(nxt).astype(np.int64)
    n, R, C = plane.shape
    assert R >= 2 and C >= 1 and n >= 1
    b = FIRST[first]
    ks = field_indices(n, mode)
    out = np.empty((len(ks), R, C), np.int64)
    chosen, clamps = [], []
    for o, k in enumerate(ks):
        q = (k + b) % 2
        ys = np.arange(1 - q, R, 2)  # the missing rows
        out[o, q::2] = plane[k // 2, q::2]
        if ys.size == 0:
            continue

        def rows(dk, dy, dx=0):  # S(k + dk, ys + dy, x + dx) for every x
            src = _source(plane, prev, nxt, k + dk)[[fold(int(y) + dy, R) for y in ys]]
            return src[:, np.clip(np.arange(C) + dx, 0, C - 1)]

        c, e, p, nx = rows(0, -1), rows(0, 1), rows(-1, 0), rows(1, 0)
        dmid = (p + nx) >> 1
        t1 = (np.abs(rows(-2, -1) - c) + np.abs(rows(-2, 1) - e)) >> 1
        t2 = (np.abs(rows(2, -1) - c) + np.abs(rows(2, 1) - e)) >> 1
        diff = np.maximum(np.maximum(np.abs(p - nx) >> 1, t1), t2)
        best = pred = which = None
        for j in ORDER:
            score = sum(np.abs(rows(0, -1, j + u) - rows(0, 1, -j + u)) for u in (-1, 0, 1)) + (1 if j else 0)
            cand = (rows(0, -1, j) + rows(0, 1, -j)) >> 1
            if best is None:
                best, pred, which = score, cand, np.zeros_like(score)
            else:
                better = score < best
                best, pred, which = np.where(better, score, best), np.where(better, cand, pred), np.where(better, j, which)
        bb = (rows(-1, -2) + rows(1, -2)) >> 1
        ff = (rows(-1, 2) + rows(1, 2)) >> 1
        hi = np.maximum(np.maximum(dmid - e, dmid - c), np.minimum(bb - c, ff - e))
        lo = np.minimum(np.minimum(dmid - e, dmid - c), np.maximum(bb - c, ff - e))
        diff = np.maximum(np.maximum(diff, lo), -hi)
        v = np.minimum(np.maximum(pred, dmid - diff), dmid + diff)
        assert v.min() >= 0 and v.max() <= maxv, (v.min(), v.max(), maxv)
        out[o, ys] = v
        chosen.append(which.ravel())
        clamps.append((np.where(pred < dmid - diff, -1, 0) + np.where(pred > dmid + diff, 1, 0)).ravel())
    if info is not None:
        info['j'] = np.concatenate(chosen) if chosen else np.zeros(0, np.int64)
        info['clamp'] = np.concatenate(clamps) if clamps else np.zeros(0, np.int64)
    return out


def parse_format(fmt):
    """'420' | '422' | '444' with an optional p9 ... p16 -> (sx, sy, depth)."""
    base, _, bits = fmt.partition('p')
    sx, sy = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}[base]
    return sx, sy, int(bits) if bits else 8


def plane_shapes(H, W, fmt):
    sx, sy, _ = parse_format(fmt)
    return [(H, W), ((H + sy) >> sy, (W + sx) >> sx), ((H + sy) >> sy, (W + sx) >> sx)]


def frame_size(H, W, fmt):
    return sum(r * c for r, c in plane_shapes(H, W, fmt)) * (2 if parse_format(fmt)[2] > 8 else 1)


def split(frames, H, W, fmt):
    """uint8 (n, framesize) -> three integer planes (n, R, C): bytes, or little-endian 16-bit words above 8 bits."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    assert frames.ndim == 2 and frames.shape[1] == frame_size(H, W, fmt), (frames.shape, frame_size(H, W, fmt))
    samples = frames.view('<u2') if parse_format(fmt)[2] > 8 else frames
    planes, at = [], 0
    for r, c in plane_shapes(H, W, fmt):
        planes.append(samples[:, at:at + r * c].reshape(-1, r, c).astype(np.int64))
        at += r * c
    return planes


def join(planes, fmt):
    """The inverse of split."""
    wide = parse_format(fmt)[2] > 8
    flat = np.concatenate([p.reshape(p.shape[0], -1) for p in planes], 1)
    return np.ascontiguousarray(flat.astype('<u2')).view(np.uint8) if wide else flat.astype(np.uint8)


def deinterlace(frames, H, W, fmt='420', first='top', mode='field', prev=None, nxt=None, loop=False, info=None):
    """uint8 (n, framesize) interlaced frames -> uint8 (2 n | n, framesize): every plane through plane_vec (or plane_loop).  prev / nxt:
    uint8 (framesize,) or None.  info: a dict that receives plane_vec's 'j' and 'clamp' over all three planes."""
    assert H >= 4
    maxv = (1 << parse_format(fmt)[2]) - 1
    planes = split(frames, H, W, fmt)
    ctx_p = [None] * 3 if prev is None else [p[0] for p in split(np.asarray(prev).reshape(1, -1), H, W, fmt)]
    ctx_n = [None] * 3 if nxt is None else [p[0] for p in split(np.asarray(nxt).reshape(1, -1), H, W, fmt)]
    outs, infos = [], []
    for pl, pp, nn in zip(planes, ctx_p, ctx_n):
        if loop:
            outs.append(plane_loop(pl, maxv, first, mode, pp, nn))
        else:
            one = {}
            outs.append(plane_vec(pl, maxv, first, mode, pp, nn, one))
            infos.append(one)
    if info is not None and infos:
        info['j'] = np.concatenate([i['j'] for i in infos])
        info['clamp'] = np.concatenate([i['clamp'] for i in infos])
    return join(outs, fmt)
