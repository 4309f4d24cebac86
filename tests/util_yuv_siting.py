"""The definition of chroma siting in ops.yuv_to_rgb / ops.rgb_to_yuv and the 8-bit 4:2:0 pair in torch float32 on the CPU,
one tensor operation per rounding: what the kernels of csrc/yuv.hip are compared against bit for bit.  Written from the definition, not
from the kernels, and on its own - the centre filters are spelled out here too, so that `siting='center'` reproducing
util_yuv_formats.decode_def / encode_def (tests/test_yuv_siting_cpu.py) compares two texts.  Formats, coefficients, plane splitting and
quantisation are util_yuv_formats'."""
import torch

import util_yuv_formats as F

# name -> (horizontal, vertical) co-sited?  Read along subsampled axes only.
SITINGS = {'center': (0, 0), 'left': (1, 0), 'topleft': (1, 1)}


def cosited_axes(fmt, siting):
    """(cx, cy): is the horizontal / vertical axis of `fmt` subsampled AND co-sited under `siting`?"""
    sx, sy, _ = F.parse(fmt)
    cx, cy = SITINGS[siting]
    return cx & sx, cy & sy


def up_axis(c, dim, size, cosited):
    """x2 along `dim`, cropped to `size`, indices clamped to the plane.
    centre:   even 2k = 0.25 c[k - 1] + 0.75 c[k], odd 2k + 1 = 0.75 c[k] + 0.25 c[k + 1]
    co-sited: even 2k = c[k],                     odd 2k + 1 = 0.5 c[k] + 0.5 c[k + 1]"""
    n = c.shape[dim]
    idx = torch.arange(n)
    prev, nxt = c.index_select(dim, (idx - 1).clamp(min=0)), c.index_select(dim, (idx + 1).clamp(max=n - 1))
    if cosited:
        even, odd = c, c * 0.5 + nxt * 0.5
    else:
        even, odd = prev * 0.25 + c * 0.75, c * 0.75 + nxt * 0.25
    shape = list(c.shape)
    shape[dim] = 2 * n
    return torch.stack([even, odd], dim + 1).reshape(shape).narrow(dim, 0, size)


def upsample_chroma(c, H, W, fmt, chroma, siting):
    sx, sy, _ = F.parse(fmt)
    if chroma == 'nearest':  # replication has no siting
        return F.upsample_chroma(c, H, W, sx, sy, chroma)
    cx, cy = cosited_axes(fmt, siting)
    if sy:
        c = up_axis(c, 1, H, cy)  # vertical first
    return up_axis(c, 2, W, cx) if sx else c


def decode_def(yuv, H, W, fmt='420', matrix='bt601', range='limited', chroma='bilinear', siting='center', out_dtype=torch.float32):
    """-> float32 (n, 3, H, W) in [0, 1], or (8-bit 4:2:0 only) uint8 (n, H, W, 3)."""
    depth = F.parse(fmt)[2]
    _, mi, off = F.coeffs(matrix, range, depth)
    y, cb, cr = F.split_planes(yuv, H, W, fmt)
    d0 = y - off[0]
    d1 = upsample_chroma(cb, H, W, fmt, chroma, siting) - off[1]
    d2 = upsample_chroma(cr, H, W, fmt, chroma, siting) - off[2]
    v = torch.stack([(mi[k, 0] * d0 + mi[k, 1] * d1) + mi[k, 2] * d2 for k in (0, 1, 2)], 1).clamp(0.0, 255.0)
    if out_dtype == torch.uint8:
        assert fmt == '420'
        return torch.round(v).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return v / torch.full_like(v, 255.0)


def _taps(p, dim, size, cosited):
    """The un-normalised decimation along `dim` (length `size`) and its scale, indices clamped to the frame.
    centre:   s[k] = p[2k] + p[2k + 1]                         scale 2
    co-sited: s[k] = (p[2k - 1] + p[2k + 1]) + (p[2k] + p[2k])  scale 4"""
    at = torch.arange(0, size, 2)
    mid, nxt = p.index_select(dim, at), p.index_select(dim, (at + 1).clamp(max=size - 1))
    if cosited:
        return (p.index_select(dim, (at - 1).clamp(min=0)) + nxt) + (mid + mid), 4.0
    return mid + nxt, 2.0


def encode_def(rgb, fmt='420', matrix='bt601', range='limited', siting='center'):
    """rgb float32 (n, 3, H, W) or (8-bit 4:2:0 only) uint8 (n, H, W, 3) -> uint8 (n, framesize)."""
    sx, sy, depth = F.parse(fmt)
    cx, cy = cosited_axes(fmt, siting)
    m, _, off = F.coeffs(matrix, range, depth)
    if rgb.dtype == torch.uint8:
        assert fmt == '420'
        x = rgb.permute(0, 3, 1, 2).float()
    else:
        x = torch.where(rgb != rgb, torch.zeros_like(rgb), rgb).clamp(0.0, 1.0) * 255.0  # NaN -> 0
    n, _, H, W = x.shape
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    p = [((m[k, 0] * r + m[k, 1] * g) + m[k, 2] * b) + off[k] for k in (0, 1, 2)]
    planes = [F.quantise(p[0], depth).reshape(n, -1)]
    for k in (1, 2):
        s, scale = p[k], 1.0
        if sx:  # horizontal first, left un-normalised
            s, f = _taps(s, 2, W, cx)
            scale *= f
        if sy:
            s, f = _taps(s, 1, H, cy)
            scale *= f
        if scale != 1.0:
            s = s * (1.0 / scale)  # ONE product with a power of two
        planes.append(F.quantise(s, depth).reshape(n, -1))
    return F.to_bytes(torch.cat(planes, 1), depth)


def hostile_rgb(n, H, W, seed):
    """float32 RGB for the encode's clamps: uniform in [-0.25, 1.25), with exact 0 and 1, a value far outside on either side and a NaN
    wherever the frame has room."""
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand((n, 3, H, W), generator=g) * 1.5 - 0.25
    flat = rgb.view(-1)
    for i, v in enumerate((0.0, 1.0, -7.0, 9.0, float('nan'))):
        flat[(i * 7) % flat.numel()] = v
    return rgb


def edge_frames(n, H, W, fmt, seed):
    """Random frames whose first samples of every plane are 0 and 2^depth - 1 (where the plane has two samples)."""
    depth = F.parse(fmt)[2]
    (_, _), (hc, wc) = F.plane_shapes(H, W, fmt)
    s = F.to_samples(F.random_frames(n, H, W, fmt, seed), depth)
    for start, size in ((0, H * W), (H * W, hc * wc), (H * W + hc * wc, hc * wc)):
        s[:, start] = 0
        if size > 1:
            s[:, start + 1] = 2 ** depth - 1
    return F.to_bytes(s, depth)
