"""The definition of ops.yuv420_to_rgb / ops.rgb_to_yuv420 in torch float32 on the CPU, one tensor operation per rounding:
what the 8-bit 4:2:0 instances of csrc/yuv.hip are compared against bit for bit, and what the golden fixture ties to the reference's rgb2ycbcr /
ycbcr2rgb.  Written from the definition, not from the kernels: the only shared piece is the order of operations the definition fixes."""
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ycbcr.pt')
MATRICES = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}
RANGES = {'limited': (219.0, 224.0, 16.0), 'full': (255.0, 255.0, 0.0)}


def frame_size(H, W):
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def coeffs64(matrix, range):
    """(M, Mi, off) as float64 tensors: the forward matrix for RGB in 0 ... 255, its inverse by the adjugate (each step one float64
    operation, so that every implementation of it gives the same bits), the offsets."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    ys, cs, yoff = RANGES[range]
    sy, scb, scr = ys / 255.0, cs / 255.0 / (2.0 * (1.0 - kb)), cs / 255.0 / (2.0 * (1.0 - kr))
    m = [[sy * kr, sy * kg, sy * kb], [scb * -kr, scb * -kg, scb * (1.0 - kb)], [scr * (1.0 - kr), scr * -kg, scr * -kb]]
    (a, b, c), (d, e, f), (g, h, i) = m
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * adj[0][0] + b * adj[1][0] + c * adj[2][0]
    mi = [[v / det for v in row] for row in adj]
    return torch.tensor(m, dtype=torch.float64), torch.tensor(mi, dtype=torch.float64), torch.tensor([yoff, 128.0, 128.0], dtype=torch.float64)


def coeffs(matrix='bt601', range='limited'):
    """(M, Mi, off) rounded to float32: what the kernels get as arguments."""
    return tuple(t.to(torch.float32) for t in coeffs64(matrix, range))


def split_planes(yuv, H, W):
    """(n, >= framesize) uint8 -> Y (n, H, W), Cb, Cr (n, Hc, Wc) as float32."""
    hc, wc = (H + 1) // 2, (W + 1) // 2
    n = yuv.shape[0]
    y = yuv[:, :H * W].reshape(n, H, W)
    cb = yuv[:, H * W:H * W + hc * wc].reshape(n, hc, wc)
    cr = yuv[:, H * W + hc * wc:H * W + 2 * hc * wc].reshape(n, hc, wc)
    return y.float(), cb.float(), cr.float()


def _up_axis(c, dim, size):
    """Centre-sited x2 along `dim`, cropped to `size`: even 2k = 0.25 c[k - 1] + 0.75 c[k], odd 2k + 1 = 0.75 c[k] + 0.25 c[k + 1]."""
    n = c.shape[dim]
    idx = torch.arange(n)
    prev, nxt = c.index_select(dim, (idx - 1).clamp(min=0)), c.index_select(dim, (idx + 1).clamp(max=n - 1))
    even = prev * 0.25 + c * 0.75
    odd = c * 0.75 + nxt * 0.25
    out = torch.stack([even, odd], dim + 1)
    shape = list(c.shape)
    shape[dim] = 2 * n
    return out.reshape(shape).narrow(dim, 0, size)


def upsample_chroma(c, H, W, chroma):
    if chroma == 'nearest':
        return c.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W]
    return _up_axis(_up_axis(c, 1, H), 2, W)  # vertical, then horizontal


def rne_byte(v):
    return torch.round(v.clamp(0.0, 255.0)).to(torch.uint8)  # torch.round: half to even


def decode_def(yuv, H, W, matrix='bt601', range='limited', chroma='bilinear', out_dtype=torch.float32):
    _, mi, off = coeffs(matrix, range)
    y, cb, cr = split_planes(yuv, H, W)
    d0 = y - off[0]
    d1 = upsample_chroma(cb, H, W, chroma) - off[1]
    d2 = upsample_chroma(cr, H, W, chroma) - off[2]
    v = torch.stack([(mi[k, 0] * d0 + mi[k, 1] * d1) + mi[k, 2] * d2 for k in (0, 1, 2)], 1).clamp(0.0, 255.0)  # (n, 3, H, W)
    if out_dtype == torch.uint8:
        return torch.round(v).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return v / torch.full_like(v, 255.0)  # a true float32 division, element by element


def encode_def(rgb, matrix='bt601', range='limited'):
    """rgb float32 (n, 3, H, W) or uint8 (n, H, W, 3) -> uint8 (n, framesize)."""
    m, _, off = coeffs(matrix, range)
    if rgb.dtype == torch.uint8:
        x = rgb.permute(0, 3, 1, 2).float()
    else:
        x = torch.where(rgb != rgb, torch.zeros_like(rgb), rgb).clamp(0.0, 1.0) * 255.0  # NaN -> 0, as the byte conversion of pixel.h
    n, _, H, W = x.shape
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    p = [((m[k, 0] * r + m[k, 1] * g) + m[k, 2] * b) + off[k] for k in (0, 1, 2)]
    rows0, rows1 = torch.arange(0, H, 2), (torch.arange(0, H, 2) + 1).clamp(max=H - 1)
    cols0, cols1 = torch.arange(0, W, 2), (torch.arange(0, W, 2) + 1).clamp(max=W - 1)
    planes = [rne_byte(p[0]).reshape(n, -1)]
    for k in (1, 2):
        top, bot = p[k][:, rows0], p[k][:, rows1]
        s = ((top[:, :, cols0] + top[:, :, cols1]) + (bot[:, :, cols0] + bot[:, :, cols1])) * 0.25
        planes.append(rne_byte(s).reshape(n, -1))
    return torch.cat(planes, 1)


def y4m_bytes(frames, H, W, header_tags='F25:1 Ip A1:1 C420jpeg', frame_params=b''):
    """A Y4M stream holding `frames` (n, framesize) uint8."""
    out = [f'YUV4MPEG2 W{W} H{H} {header_tags}'.rstrip().encode() + b'\n']
    for f in frames:
        out += [b'FRAME' + frame_params + b'\n', f.numpy().tobytes()]
    return b''.join(out)


# ---- the golden fixture of the reference (scripts/make_ycbcr_golden.py), shared by the CPU and the GPU test
def golden_conditions(got, want, what):
    """Every compared byte within 1 LSB of the reference (float64 with printed constants), at most 0.5 % of them different."""
    d = (got.to(torch.int32) - want.to(torch.int32)).abs()
    print(f'{what}: max {int(d.max())}, {float((d > 0).float().mean()) * 100:.4f} % of {d.numel()} bytes differ')
    assert int(d.max()) <= 1, what
    assert float((d > 0).float().mean()) <= 0.005, what


def golden_yuv(g):
    """The reference's 4:4:4 bytes of the 2 x 2-constant image as I420 frames (every block holds one chroma value)."""
    yc = g['ycbcr']
    n = yc.shape[0]
    return torch.cat([yc[..., 0].reshape(n, -1), yc[:, ::2, ::2, 1].reshape(n, -1), yc[:, ::2, ::2, 2].reshape(n, -1)], 1)
