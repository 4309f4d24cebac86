"""NumPy restatement of the MPEG-style round trip of DESIGN 4.18 (what ops.mpeg_roundtrip computes), steps M1 - M7, on top of the passes
of tests/jpeg_ref.py: 4:2:0 planes padded to 16, an intra frame quantised by the MPEG-2 default matrix, predicted frames by a full search
per 16 x 16 macroblock against the previous reconstruction, a half-sample chroma vector, a flat dead-zone quantiser on the residual.
Every value is an integer (int64 here; the kernels' 32 bits hold them all), `>>` is the arithmetic shift."""
import numpy as np

from jpeg_ref import _fdct_pass, _idct_pass

INTRA_W = np.array([8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
                    22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83],
                   np.int64).reshape(8, 8)


def intra_table(qscale):
    q = np.maximum(1, (INTRA_W * qscale + 8) >> 4)
    q[0, 0] = 8
    return q


def planes(img):
    """M1: uint8 (H, W, 3) -> [Y (Hp, Wp), Cb, Cr (Hp / 2, Wp / 2)], int64."""
    H, W = img.shape[:2]
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    full = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
            (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16]
    full = [np.pad(p, ((0, -H % 16), (0, -W % 16)), mode='edge') for p in full]
    ch = -(-H // 2)
    out = [full[0]]
    for p in full[1:]:
        bias = 1 + (np.arange(p.shape[1] // 2) & 1)
        c = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        c[ch:] = c[ch - 1]
        out.append(c)
    return out


def _blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    return b.transpose(0, 2, 1, 3).reshape(b.shape[0] * 8, b.shape[1] * 8)


def _fdct(p):
    c = _fdct_pass(_blocks(p), True)
    return _fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)


def _idct(c):
    c = _idct_pass(c.swapaxes(-1, -2), 11).swapaxes(-1, -2)
    return _unblocks(_idct_pass(c, 18))


def intra_plane(p, qscale, stats=None):
    """M3 on one plane."""
    Q = intra_table(qscale)
    c = _fdct(p - 128)
    k = np.sign(c) * ((np.abs(c) + 4 * Q) // (8 * Q))
    if stats is not None:
        stats['cmax_intra'] = max(stats.get('cmax_intra', 0), int(np.abs(c).max()))
        stats['nonzero'][-1] += int(np.count_nonzero(k))
    return np.clip(_idct(k * Q) + 128, 0, 255)


def inter_plane(p, pred, qscale, stats=None):
    """M6 on one plane."""
    c = _fdct(p - pred)
    k = np.sign(c) * (np.abs(c) // (8 * qscale))
    d = np.sign(k) * (((2 * np.abs(k) + 1) * qscale) >> 1)
    if stats is not None:
        stats['cmax_inter'] = max(stats.get('cmax_inter', 0), int(np.abs(c).max()))
        stats['nonzero'][-1] += int(np.count_nonzero(k))
    return np.clip(pred + _idct(d), 0, 255)


def search_vectors(cur, ref, qscale, R):
    """M4: source luma, reconstructed luma of the previous frame -> int64 (Hp / 16, Wp / 16, 2) of (dy, dx)."""
    Hp, Wp = cur.shape
    padded = np.pad(ref, R, mode='edge')
    best = np.full((Hp // 16, Wp // 16), np.iinfo(np.int64).max, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sad = np.abs(cur - padded[R + dy:R + dy + Hp, R + dx:R + dx + Wp]).reshape(Hp // 16, 16, Wp // 16, 16).sum((1, 3))
            cost = sad + qscale * (abs(dy) + abs(dx))
            best = np.minimum(best, (cost << 10) | ((dy + 15) << 5) | (dx + 15))
    return np.stack([((best >> 5) & 31) - 15, (best & 31) - 15], -1)


def predict(rec, mv):
    """M5: the previous reconstruction [Y, Cb, Cr] and the vectors -> the three predictions."""
    y, cb, cr = rec
    Hp, Wp = y.shape
    dy, dx = (np.repeat(np.repeat(mv[..., i], 16, 0), 16, 1) for i in range(2))
    yy, xx = np.mgrid[0:Hp, 0:Wp]
    out = [y[np.clip(yy + dy, 0, Hp - 1), np.clip(xx + dx, 0, Wp - 1)]]
    Hc, Wc = Hp // 2, Wp // 2
    dy, dx = dy[::2, ::2], dx[::2, ::2]
    iy, hy, ix, hx = dy >> 1, dy & 1, dx >> 1, dx & 1
    yy, xx = np.mgrid[0:Hc, 0:Wc]
    ya, yb = np.clip(yy + iy, 0, Hc - 1), np.clip(yy + iy + hy, 0, Hc - 1)
    xa, xb = np.clip(xx + ix, 0, Wc - 1), np.clip(xx + ix + hx, 0, Wc - 1)
    for c in (cb, cr):
        out.append((c[ya, xa] + c[ya, xb] + c[yb, xa] + c[yb, xb] + 2) >> 2)
    return out


def output(rec, H, W):
    """M7: reconstructed planes -> uint8 (H, W, 3)."""
    ch, cw = -(-H // 2), -(-W // 2)
    up = []
    for p in rec[1:]:
        c = p[:ch, :cw]
        rows = np.arange(ch)
        full = np.empty((2 * ch, 2 * cw), np.int64)
        for v, nb in ((0, np.maximum(rows - 1, 0)), (1, np.minimum(rows + 1, ch - 1))):
            if cw <= 2:
                full[v::2, 0::2] = full[v::2, 1::2] = c
                continue
            s = 3 * c + c[nb]
            left, right = s[:, np.maximum(np.arange(cw) - 1, 0)], s[:, np.minimum(np.arange(cw) + 1, cw - 1)]
            full[v::2, 0::2] = (3 * s + left + 8) >> 4
            full[v::2, 1::2] = (3 * s + right + 7) >> 4
        up.append(full[:H, :W])
    y, cb, cr = rec[0][:H, :W], up[0] - 128, up[1] - 128
    out = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(out, 0, 255).astype(np.uint8)


def is_intra(i, gop):
    return i == 0 or (gop > 0 and i % gop == 0)


def roundtrip_clip(frames, qscale, gop=12, search=7, details=False):
    """frames uint8 (t, H, W, 3) -> uint8 (t, H, W, 3); qscale 1 .. 31, 0: a copy.  details: also a dict with 'vectors' (per frame: None
    for an intra frame, else int64 (Hp / 16, Wp / 16, 2) of (dy, dx)), 'nonzero' (non-zero quantised coefficients per frame) and the
    largest |coefficient| seen before quantisation, 'cmax_intra' / 'cmax_inter'."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3, (frames.dtype, frames.shape)
    qscale, gop, search = int(qscale), int(gop), int(search)
    if not 0 <= qscale <= 31:
        raise ValueError(f'qscale {qscale} is outside 1 .. 31')
    if gop < 0 or not 0 <= search <= 15:
        raise ValueError(f'gop {gop} / search {search} out of range')
    stats = {'vectors': [], 'nonzero': []}
    if qscale == 0:
        return (frames.copy(), stats) if details else frames.copy()
    H, W = frames.shape[1:3]
    out, rec = [], None
    for i, img in enumerate(frames):
        src = planes(img)
        stats['nonzero'].append(0)
        if is_intra(i, gop):
            rec = [intra_plane(p, qscale, stats) for p in src]
            stats['vectors'].append(None)
        else:
            mv = search_vectors(src[0], rec[0], qscale, search)
            rec = [inter_plane(p, pr, qscale, stats) for p, pr in zip(src, predict(rec, mv))]
            stats['vectors'].append(mv)
        out.append(output(rec, H, W))
    out = np.stack(out)
    return (out, stats) if details else out


def roundtrip(frames, qscale, gop=12, search=7):
    """frames uint8 (b, t, H, W, 3) or (t, H, W, 3); qscale an int or b ints."""
    frames = np.asarray(frames)
    if frames.ndim == 4:
        return roundtrip_clip(frames, qscale, gop, search)
    q = [int(qscale)] * len(frames) if np.ndim(qscale) == 0 else [int(v) for v in qscale]
    return np.stack([roundtrip_clip(f, qi, gop, search) for f, qi in zip(frames, q)])
