"""The clips the MPEG round trip tests share (tests/test_mpeg_cpu.py, tests/test_gpu_mpeg.py, scripts/make_mpeg_golden.py): uint8 RGB
torch tensors, made the same way on every machine (integer arithmetic and torch's CPU generator only)."""
import torch


def _texture(h, w, seed):
    """uint8 (h, w, 3): grey blobs 6 pixels across plus fine grey grain, so that a block matches only where it came from, under a slow
    colour gradient (4:2:0 keeps all of it)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, 256, (-(-h // 6) + 1, -(-w // 6) + 1), generator=g)
    blobs = coarse.repeat_interleave(6, 0).repeat_interleave(6, 1)[:h, :w]
    grain = torch.randint(-24, 25, (h, w), generator=g)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    tint = torch.stack([xx // 3, torch.zeros_like(xx), yy // 3], -1)
    return ((blobs * 5 // 8 + 40 + grain)[..., None] + tint).clamp(0, 255).to(torch.uint8).contiguous()


def noise_clip(b, t, h, w, seed):
    """uint8 (b, t, h, w, 3) of independent noise."""
    return torch.randint(0, 256, (b, t, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def moving_clip(t, h, w, shift, seed, noise=2):
    """uint8 (t, h, w, 3): frame i is a window of one texture displaced by i * shift, so that the content of frame i at (y, x) is that
    of frame i - 1 at (y + sy, x + sx) - the vector M4 should find is `shift` - plus a little fresh noise per frame."""
    sy, sx = shift
    m = (t - 1) * max(abs(sy), abs(sx), 1)
    big = _texture(h + 2 * m, w + 2 * m, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    out = []
    for i in range(t):
        y0, x0 = m + i * sy, m + i * sx
        f = big[y0:y0 + h, x0:x0 + w].long()
        if noise:
            f = f + torch.randint(-noise, noise + 1, f.shape, generator=g)
        out.append(f.clamp(0, 255).to(torch.uint8))
    return torch.stack(out)


def inverted_stripes_clip(t, h, w):
    """Rows alternate 0 / 255 and every other frame is inverted: 7394 is the largest intra coefficient, and with search 0, where no
    vector can undo the inversion, 14788 the largest inter one."""
    rows = (torch.arange(h) & 1) * 255
    frame = rows[:, None, None].expand(h, w, 3)
    return torch.stack([(frame if i % 2 == 0 else 255 - frame) for i in range(t)]).to(torch.uint8).contiguous()


def tie_clip(h, w):
    """Two frames of vertical stripes of period 8 (4 dark, 4 bright columns), the second shifted by 4: dx = -4 and dx = +4 match equally
    well and cost the same, and M4's tie rule takes the first in raster order, -4."""
    def stripes(phase):
        cols = (((torch.arange(w) + phase) // 4) & 1) * 200 + 20
        return cols[None, :, None].expand(h, w, 3)
    return torch.stack([stripes(0), stripes(4)]).to(torch.uint8).contiguous()
