"""NumPy restatement of the baseline JPEG round trip of DESIGN 4.16 (what ops.jpeg_roundtrip computes): integer colour conversion, edge
padding to the MCU, 4:2:0 chroma by the alternating-bias 2 x 2 mean, the 13-bit Loeffler forward DCT, Annex K tables scaled by the
quality, the 13-bit inverse DCT, triangle-filter chroma upsampling and the colour conversion back.  Every value is an integer (int64
here; the kernel's 32 bits hold them all), `>>` is the arithmetic shift.  Byte for byte what PIL's libjpeg writes and reads back
(Image.save(format='JPEG', quality=q, subsampling=0 | 2), Image.open(...).convert('RGB')): tests/test_jpeg_cpu.py."""
import numpy as np

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA = np.full((8, 8), 99, np.int64)
CHROMA[0, :4], CHROMA[1, :4], CHROMA[2, :3], CHROMA[3, :2] = (17, 18, 24, 47), (18, 21, 26, 66), (24, 26, 56), (47, 66)
SUBSAMPLINGS = ('420', '444')


def _d(x, k):
    return (x + (1 << (k - 1))) >> k


def quant_table(base, quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * s + 50) // 100, 1, 255)


def _odd(t4, t5, t6, t7):
    """The odd part both transforms share: (t4, t5, t6, t7) -> the four sums before the final descale."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def _fdct_pass(d, rows):
    """One 8-point pass along the last axis; rows: the first (row) pass, else the second (column) pass."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    k = 11 if rows else 15
    o = [None] * 8
    o[0], o[4] = ((t10 + t11) << 2, (t10 - t11) << 2) if rows else (_d(t10 + t11, 2), _d(t10 - t11, 2))
    z = (t12 + t13) * 4433
    o[2], o[6] = _d(z + t13 * 6270, k), _d(z - t12 * 15137, k)
    a, b, c, e = _odd(t4, t5, t6, t7)
    o[7], o[5], o[3], o[1] = _d(a, k), _d(b, k), _d(c, k), _d(e, k)
    return np.stack(o, -1)


def _idct_pass(c, k):
    c = [c[..., i] for i in range(8)]
    z = (c[2] + c[6]) * 4433
    t2, t3 = z - c[6] * 15137, z + c[2] * 6270
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = _odd(c[7], c[5], c[3], c[1])
    return np.stack([_d(v, k) for v in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)], -1)


def _codec_plane(plane, q):
    """Steps 4-6 on a plane whose sides are multiples of 8: samples 0 .. 255 in, samples 0 .. 255 out."""
    h, w = plane.shape
    b = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128  # [block row][block col][y][x]
    c = _fdct_pass(b, True)                                       # rows: along x
    c = _fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)    # columns: along y
    k = np.sign(c) * ((np.abs(c) + 4 * q) // (8 * q))
    c = k * q
    c = _idct_pass(c.swapaxes(-1, -2), 11).swapaxes(-1, -2)       # columns first
    c = _idct_pass(c, 18)
    return np.clip(c + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w)


def roundtrip(img, quality, subsampling='420'):
    """img uint8 (H, W, 3) RGB -> uint8 (H, W, 3): a baseline JPEG of `quality` 1 .. 100 written and read back; quality 0: a copy."""
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f'subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}')
    quality = int(quality)
    if not 0 <= quality <= 100:
        raise ValueError(f'quality {quality} is outside 1 .. 100')
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, (img.dtype, img.shape)
    if quality == 0:
        return img.copy()
    H, W = img.shape[:2]
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    planes = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
              (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
              (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16]
    mcu = 16 if subsampling == '420' else 8
    planes = [np.pad(p, ((0, -H % mcu), (0, -W % mcu)), mode='edge') for p in planes]
    ql, qc = quant_table(LUMA, quality), quant_table(CHROMA, quality)
    y = _codec_plane(planes[0], ql)
    if subsampling == '444':
        cb, cr = (_codec_plane(p, qc)[:H, :W] for p in planes[1:])
    else:
        ch, cw = -(-H // 2), -(-W // 2)
        up = []
        for p in planes[1:]:
            bias = 1 + (np.arange(p.shape[1] // 2) & 1)
            c = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            c[ch:] = c[ch - 1]  # below the frame the encoder repeats the last CHROMA row (an even H would otherwise average row H - 1 alone)
            c = _codec_plane(c, qc)[:ch, :cw]
            rows = np.arange(ch)
            full = np.empty((2 * ch, 2 * cw), np.int64)
            for v, nb in ((0, np.maximum(rows - 1, 0)), (1, np.minimum(rows + 1, ch - 1))):
                if cw <= 2:  # the decoder keeps the triangle filter for chroma planes wider than 2 samples and replicates narrower ones
                    full[v::2, 0::2] = full[v::2, 1::2] = c
                    continue
                s = 3 * c + c[nb]
                left, right = s[:, np.maximum(np.arange(cw) - 1, 0)], s[:, np.minimum(np.arange(cw) + 1, cw - 1)]
                full[v::2, 0::2] = (3 * s + left + 8) >> 4
                full[v::2, 1::2] = (3 * s + right + 7) >> 4
            up.append(full[:H, :W])
        cb, cr = up
    y, cb, cr = y[:H, :W], cb - 128, cr - 128
    out = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(out, 0, 255).astype(np.uint8)


def roundtrip_batch(frames, quality, subsampling='420'):
    """frames uint8 (n, H, W, 3); quality an int or n ints."""
    frames = np.asarray(frames)
    q = [int(quality)] * len(frames) if np.ndim(quality) == 0 else [int(v) for v in quality]
    return np.stack([roundtrip(f, qi, subsampling) for f, qi in zip(frames, q)])
