"""The definition of ops.yuv_to_rgb / ops.rgb_to_yuv in torch float32 on the CPU, one tensor operation per rounding: what
the kernels of csrc/yuv.hip are compared against bit for bit.  Written from the definition, not from the kernels, in the manner
of tests/util_yuv.py (whose 8-bit 4:2:0 definition this one must reproduce at '420')."""
import torch

from util_yuv import MATRICES

SUBSAMPLINGS = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}
ALIASES = ('420jpeg', '420mpeg2', '420paldv')


def parse(fmt):
    """name -> (sx, sy, depth)."""
    if fmt in ALIASES:
        return 1, 1, 8
    base, _, bits = fmt.partition('p')
    return SUBSAMPLINGS[base] + (int(bits) if bits else 8,)


def name(base, depth):
    return base + (f'p{depth}' if depth > 8 else '')


def plane_shapes(H, W, fmt):
    sx, sy, _ = parse(fmt)
    return (H, W), ((H + sy) >> sy, (W + sx) >> sx)


def frame_size(H, W, fmt):
    """Bytes of a frame."""
    (h, w), (hc, wc) = plane_shapes(H, W, fmt)
    return (h * w + 2 * hc * wc) * (2 if parse(fmt)[2] > 8 else 1)


def coeffs64(matrix, range, depth):
    """(M, Mi, off) as float64 tensors for samples of `depth` bits, k = 2^(depth - 8): limited scales luma to 219 k and chroma to 224 k
    with offsets (16 k, 128 k), full both to 2^depth - 1 with offsets (0, 2^(depth - 1)); the inverse by the adjugate, one float64
    operation per step."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    k = float(2 ** (depth - 8))
    if range == 'limited':
        ys, cs, yoff, coff = 219.0 * k, 224.0 * k, 16.0 * k, 128.0 * k
    else:
        ys, cs, yoff, coff = float(2 ** depth - 1), float(2 ** depth - 1), 0.0, float(2 ** (depth - 1))
    sy, scb, scr = ys / 255.0, cs / 255.0 / (2.0 * (1.0 - kb)), cs / 255.0 / (2.0 * (1.0 - kr))
    m = [[sy * kr, sy * kg, sy * kb], [scb * -kr, scb * -kg, scb * (1.0 - kb)], [scr * (1.0 - kr), scr * -kg, scr * -kb]]
    (a, b, c), (d, e, f), (g, h, i) = m
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * adj[0][0] + b * adj[1][0] + c * adj[2][0]
    mi = [[v / det for v in row] for row in adj]
    return torch.tensor(m, dtype=torch.float64), torch.tensor(mi, dtype=torch.float64), torch.tensor([yoff, coff, coff], dtype=torch.float64)


def coeffs(matrix, range, depth):
    return tuple(t.to(torch.float32) for t in coeffs64(matrix, range, depth))


def to_samples(yuv, depth):
    """(n, bytes) uint8 -> (n, samples) int32: the bytes themselves, or little-endian 16-bit words (all 16 bits: nothing is masked)."""
    if depth == 8:
        return yuv.to(torch.int32)
    pairs = yuv.reshape(yuv.shape[0], -1, 2).to(torch.int32)
    return pairs[..., 0] + 256 * pairs[..., 1]


def to_bytes(samples, depth):
    """(n, samples) integers -> (n, bytes) uint8."""
    samples = samples.to(torch.int32)
    if depth == 8:
        return samples.to(torch.uint8)
    return torch.stack([samples % 256, samples // 256], -1).to(torch.uint8).reshape(samples.shape[0], -1)


def split_planes(yuv, H, W, fmt):
    """(n, >= framesize) uint8 -> Y (n, H, W), Cb, Cr (n, Hc, Wc) as float32 (exact: a sample has at most 16 bits)."""
    depth = parse(fmt)[2]
    (_, _), (hc, wc) = plane_shapes(H, W, fmt)
    n = yuv.shape[0]
    s = to_samples(yuv[:, :frame_size(H, W, fmt)], depth).float()
    return s[:, :H * W].reshape(n, H, W), s[:, H * W:H * W + hc * wc].reshape(n, hc, wc), s[:, H * W + hc * wc:].reshape(n, hc, wc)


def _up_axis(c, dim, size):
    """Centre-sited x2 along `dim`, cropped to `size`: even 2k = 0.25 c[k - 1] + 0.75 c[k], odd 2k + 1 = 0.75 c[k] + 0.25 c[k + 1]."""
    n = c.shape[dim]
    idx = torch.arange(n)
    prev, nxt = c.index_select(dim, (idx - 1).clamp(min=0)), c.index_select(dim, (idx + 1).clamp(max=n - 1))
    out = torch.stack([prev * 0.25 + c * 0.75, c * 0.75 + nxt * 0.25], dim + 1)
    shape = list(c.shape)
    shape[dim] = 2 * n
    return out.reshape(shape).narrow(dim, 0, size)


def upsample_chroma(c, H, W, sx, sy, chroma):
    if chroma == 'nearest':
        if sy:
            c = c.repeat_interleave(2, 1)[:, :H]
        return c.repeat_interleave(2, 2)[:, :, :W] if sx else c
    if sy:
        c = _up_axis(c, 1, H)  # vertical first
    return _up_axis(c, 2, W) if sx else c


def decode_def(yuv, H, W, fmt='420', matrix='bt601', range='limited', chroma='bilinear'):
    sx, sy, depth = parse(fmt)
    _, mi, off = coeffs(matrix, range, depth)
    y, cb, cr = split_planes(yuv, H, W, fmt)
    d0 = y - off[0]
    d1 = upsample_chroma(cb, H, W, sx, sy, chroma) - off[1]
    d2 = upsample_chroma(cr, H, W, sx, sy, chroma) - off[2]
    v = torch.stack([(mi[k, 0] * d0 + mi[k, 1] * d1) + mi[k, 2] * d2 for k in (0, 1, 2)], 1).clamp(0.0, 255.0)
    return v / torch.full_like(v, 255.0)


def quantise(v, depth):
    return torch.round(v.clamp(0.0, float(2 ** depth - 1))).to(torch.int32)  # torch.round: half to even


def encode_def(rgb, fmt='420', matrix='bt601', range='limited'):
    """rgb float32 (n, 3, H, W) -> uint8 (n, framesize)."""
    sx, sy, depth = parse(fmt)
    m, _, off = coeffs(matrix, range, depth)
    x = torch.where(rgb != rgb, torch.zeros_like(rgb), rgb).clamp(0.0, 1.0) * 255.0  # NaN -> 0
    n, _, H, W = x.shape
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    p = [((m[k, 0] * r + m[k, 1] * g) + m[k, 2] * b) + off[k] for k in (0, 1, 2)]
    rows0, rows1 = torch.arange(0, H, 2), (torch.arange(0, H, 2) + 1).clamp(max=H - 1)
    cols0, cols1 = torch.arange(0, W, 2), (torch.arange(0, W, 2) + 1).clamp(max=W - 1)
    planes = [quantise(p[0], depth).reshape(n, -1)]
    for k in (1, 2):
        if sx and sy:
            top, bot = p[k][:, rows0], p[k][:, rows1]
            s = ((top[:, :, cols0] + top[:, :, cols1]) + (bot[:, :, cols0] + bot[:, :, cols1])) * 0.25
        elif sx:
            s = (p[k][:, :, cols0] + p[k][:, :, cols1]) * 0.5
        else:
            s = p[k]
        planes.append(quantise(s, depth).reshape(n, -1))
    return to_bytes(torch.cat(planes, 1), depth)


def encode_ref64(rgb, fmt, matrix, range):
    """The float64 formula: the same matrices in float64, x = clamp(f, 0, 1) * 255 of the float32 input taken exactly; samples as int32."""
    sx, sy, depth = parse(fmt)
    assert (sx, sy) == (0, 0)
    m, _, off = coeffs64(matrix, range, depth)
    x = rgb.double().clamp(0.0, 1.0) * 255.0
    p = torch.einsum('kc,nchw->nkhw', m, x) + off.view(1, 3, 1, 1)
    return torch.round(p.clamp(0.0, float(2 ** depth - 1))).to(torch.int32)


def random_frames(n, H, W, fmt, seed, above=0):
    """Frames with samples uniform in [0, 2^depth) as uint8 (n, framesize); `above` samples per frame are raised past 2^depth - 1 (the
    decode does not mask them; only where the word has room: depth < 16)."""
    depth = parse(fmt)[2]
    g = torch.Generator().manual_seed(seed)
    count = frame_size(H, W, fmt) // (2 if depth > 8 else 1)
    s = torch.randint(0, 2 ** depth, (n, count), generator=g, dtype=torch.int32)
    if 8 < depth < 16 and above:
        where = torch.randint(0, count, (n, above), generator=g)
        s.scatter_(1, where, torch.randint(2 ** depth, 2 ** 16, (n, above), generator=g, dtype=torch.int32))
    return to_bytes(s, depth)


def y4m_bytes(frames, H, W, header_tags, frame_params=b''):
    """A Y4M stream holding `frames` (n, framesize) uint8."""
    out = [f'YUV4MPEG2 W{W} H{H} {header_tags}'.rstrip().encode() + b'\n']
    for f in frames:
        out += [b'FRAME' + frame_params + b'\n', f.numpy().tobytes()]
    return b''.join(out)
