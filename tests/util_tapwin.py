"""The window geometry of the tap-window DCNv2 forward kernels (csrc/dcn_tapwin.hip, csrc/dcn_tapwin_s.hip) restated in NumPy, a census
of sampling positions by their place relative to the staged window, and offset fields that put lanes on every window edge.  CPU only.

Both kernels: a workgroup owns an 8 x 32 pixel tile and, per (deformable group, tap), stages a 12 x 40 window of the group's channels
around  tile + regular tap position + shift;  the shift is the rounded mid-range of the tap's offsets over eight sample pixels of the
tile, the window's column origin is rounded down to a multiple of 4.  A lane whose 2 x 2 bilinear cell lies in the window
(0 <= ry <= IH - 2 && 0 <= rx <= IW - 2) reads it from there, every other valid lane goes through the fix-up pass.  The arithmetic
below is float32 wherever the kernels' is (tests/test_tapwin_geom_cpu.py pins the constants to the two .hip files)."""
import numpy as np
import torch

TH, TW, RY, RX = 8, 32, 2, 2
IH = TH + 2 * RY
IW = (TW + 2 * RX + 3 + 3) // 4 * 4
SAMPLE_ROWS, SAMPLE_COLS = (1, 5), (4, 12, 20, 28)

EDGE_CLASSES = ('ry=0', 'ry=IH-2', 'rx=0', 'rx=IW-2', 'ry=-1', 'ry=IH-1', 'rx=-1', 'rx=IW-1')
RX_CLASSES = ('rx=0', 'rx=IW-2', 'rx=-1', 'rx=IW-1')
BORDERS = ('top', 'bottom', 'left', 'right')


def tile_shifts(plane):
    """plane (H, W) float32 -> (tiles_y, tiles_x) int64: the kernels' pre-pass,  fminf / fmaxf over the sample pixels (a NaN operand is
    dropped, as fminf does), mid = clamp(0.5f * (mn + mx), +-16384) through fmaxf then fminf, shift = floorf(mid + 0.5f)."""
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    ty0 = np.arange(0, H, TH)[:, None]
    tx0 = np.arange(0, W, TW)[None, :]
    mn = np.full((ty0.size, tx0.size), 3.0e38, np.float32)
    mx = -mn
    for r in SAMPLE_ROWS:
        for c in SAMPLE_COLS:
            f = plane[np.minimum(ty0 + r, H - 1), np.minimum(tx0 + c, W - 1)]
            mn, mx = np.fmin(mn, f), np.fmax(mx, f)
    with np.errstate(invalid='ignore', over='ignore'):
        mid = np.float32(0.5) * (mn + mx)
        mid = np.fmin(np.fmax(mid, np.float32(-16384.)), np.float32(16384.))
        return np.floor(mid + np.float32(0.5)).astype(np.int64)


def tap_geometry(off_img, g, t):
    """off_img (dg * 18, H, W) float32 of one image -> per pixel of tap (g, t): dict of (H, W) arrays  valid, inside, ry, rx, align,
    sy, sx, wy0, wx0  (the last five constant over a tile)."""
    off_img = np.asarray(off_img, np.float32)
    _, H, W = off_img.shape
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ty0, tx0 = (oy // TH) * TH, (ox // TW) * TW
    ti, tj = divmod(t, 3)
    dy, dx = off_img[g * 18 + 2 * t], off_img[g * 18 + 2 * t + 1]
    sy = tile_shifts(dy)[oy // TH, ox // TW]
    sx = tile_shifts(dx)[oy // TH, ox // TW]
    wy0 = ty0 - 1 + ti + sy - RY
    raw = tx0 - 1 + tj + sx - RX
    wx0 = raw & ~3
    h = (oy - 1 + ti).astype(np.float32) + dy
    w = (ox - 1 + tj).astype(np.float32) + dx
    valid = (h > np.float32(-1)) & (w > np.float32(-1)) & (h < np.float32(H)) & (w < np.float32(W))
    # (positions that are not valid never reach the window test; their ry / rx are clamped so that the int conversion stays defined)
    ry = np.floor(np.where(valid, h, 0)).astype(np.int64) - wy0
    rx = np.floor(np.where(valid, w, 0)).astype(np.int64) - wx0
    inside = valid & (ry >= 0) & (ry <= IH - 2) & (rx >= 0) & (rx <= IW - 2)
    return dict(valid=valid, inside=inside, ry=ry, rx=rx, align=raw & 3, sy=sy, sx=sx, wy0=wy0, wx0=wx0, h=h, w=w)


def new_census():
    c = dict(valid=0, inside=0, fixup=0, windows=0, outside=0)
    c.update({k: 0 for k in EDGE_CLASSES})
    c.update({(k, a): 0 for k in RX_CLASSES for a in range(4)})
    c.update({('align', a): 0 for a in range(4)})
    c.update({('clipped', b): 0 for b in BORDERS})
    return c


def add_census(a, b):
    return {k: a[k] + b[k] for k in a}


def census(off, dg):
    """off (B, dg * 18, H, W) -> counts over every (image, group, tap):
    valid / inside / fixup                 sampling positions that pass the reference's bounds rule; of those, in the window / not
    'ry=0' 'ry=IH-2' 'rx=0' 'rx=IW-2'      inside, on the window's first / last usable row / column
    'ry=-1' 'ry=IH-1' | 'rx=-1' 'rx=IW-1'  one row (column) outside with the other coordinate inside: the fix-up lanes next to the edge
    (rx class, a)                          the four rx classes by the column alignment  (tx0 - 1 + tj + sx - RX) & 3
    ('align', a)                           windows by that alignment
    ('clipped', border) / outside          windows that reach past that image border while holding image pixels / hold none
    windows                                (image, tile, group, tap) windows in all."""
    off = np.asarray(off.detach().cpu().numpy() if isinstance(off, torch.Tensor) else off, np.float32)
    B, planes, H, W = off.shape
    assert planes == dg * 18
    c = new_census()
    for b in range(B):
        for g in range(dg):
            for t in range(9):
                q = tap_geometry(off[b], g, t)
                valid, inside, ry, rx, al = q['valid'], q['inside'], q['ry'], q['rx'], q['align']
                in_y, in_x = valid & (ry >= 0) & (ry <= IH - 2), valid & (rx >= 0) & (rx <= IW - 2)
                sel = {'ry=0': inside & (ry == 0), 'ry=IH-2': inside & (ry == IH - 2), 'rx=0': inside & (rx == 0), 'rx=IW-2': inside & (rx == IW - 2),
                       'ry=-1': in_x & (ry == -1), 'ry=IH-1': in_x & (ry == IH - 1), 'rx=-1': in_y & (rx == -1), 'rx=IW-1': in_y & (rx == IW - 1)}
                c['valid'] += int(valid.sum())
                c['inside'] += int(inside.sum())
                c['fixup'] += int((valid & ~inside).sum())
                for k, s in sel.items():
                    c[k] += int(s.sum())
                for k in RX_CLASSES:
                    for a in range(4):
                        c[(k, a)] += int((sel[k] & (al == a)).sum())
                wy0, wx0, alt = q['wy0'][::TH, ::TW], q['wx0'][::TH, ::TW], al[::TH, ::TW]
                out = (wy0 + IH <= 0) | (wy0 >= H) | (wx0 + IW <= 0) | (wx0 >= W)
                c['windows'] += wy0.size
                c['outside'] += int(out.sum())
                for a in range(4):
                    c[('align', a)] += int((alt == a).sum())
                for name, m in (('top', wy0 < 0), ('bottom', wy0 + IH > H), ('left', wx0 < 0), ('right', wx0 + IW > W)):
                    c[('clipped', name)] += int((m & ~out).sum())
    return c


def census_table(c):
    """The census as printable lines."""
    lines = ['valid %d  inside %d  fixup %d  windows %d' % (c['valid'], c['inside'], c['fixup'], c['windows'])]
    lines.append('  '.join('%s %d' % (k, c[k]) for k in EDGE_CLASSES))
    for k in RX_CLASSES:
        lines.append('%-8s by alignment 0..3: %s' % (k, ' '.join(str(c[(k, a)]) for a in range(4))))
    lines.append('windows by alignment 0..3: %s' % ' '.join(str(c[('align', a)]) for a in range(4)))
    lines.append('windows clipped at ' + '  '.join('%s %d' % (b, c[('clipped', b)]) for b in BORDERS) + '  wholly outside %d' % c['outside'])
    return lines


# ------------------------------------------------------------------------------------------------ fields
def sample_pixel_mask(H, W):
    """(H, W) bool: the pixels the pre-pass reads (of every tile)."""
    samp = torch.zeros(H, W, dtype=torch.bool)
    for ty0 in range(0, H, TH):
        for tx0 in range(0, W, TW):
            for r in SAMPLE_ROWS:
                for c in SAMPLE_COLS:
                    samp[min(ty0 + r, H - 1), min(tx0 + c, W - 1)] = True
    return samp


def ladder_field(B, dg, H, W, seed, frac, span=6):
    """Every (group, tap, dy | dx) plane: an integer base in [-3, 3] (the dx bases moved up by 0..3 so that the window's column alignment
    is (g * 9 + t) % 4); the sample pixels carry base + frac - the shift is `base` for 0 <= frac < 0.5 -, every other pixel
    base + d + frac with d a uniform integer in [-span, span]: lanes at every distance up to `span` from the window's centre, in both
    directions, whatever the tile.  frac = 0 gives integer sampling positions (lh = lw = 0)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(-3, 4, (1, dg * 18, 1, 1), generator=g).float()
    for gg in range(dg):
        for t in range(9):
            tj, want = t % 3, (gg * 9 + t) % 4
            sx = int(base[0, gg * 18 + 2 * t + 1])
            while ((tj + sx - 1 - RX) & 3) != want:  # (tx0 is a multiple of 32: it does not enter the alignment)
                sx += 1
            base[0, gg * 18 + 2 * t + 1] = sx
    d = torch.randint(-span, span + 1, (B, dg * 18, H, W), generator=g).float()
    d[:, :, sample_pixel_mask(H, W)] = 0
    return (base + d + frac).contiguous()


def outward_field(B, dg, H, W, seed):
    """Per-plane constants of +-(3 .. 20) px (uniform magnitude, random sign): every lane is inside its window, and the windows of the
    tiles in the first / last tile row and column are clipped at, or lie wholly beyond, the image border they are pushed towards."""
    g = torch.Generator().manual_seed(seed)
    mag = 3.0 + 17.0 * torch.rand(1, dg * 18, 1, 1, generator=g)
    sign = torch.randint(0, 2, (1, dg * 18, 1, 1), generator=g).float() * 2 - 1
    return (mag * sign).expand(B, dg * 18, H, W).contiguous()


def noise_field(B, dg, H, W, seed, sigma):
    """White noise, clamped to the +-30 px the edge tests stay within."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, dg * 18, H, W, generator=g) * sigma).clamp_(-30., 30.).contiguous()


# The geometries of tests/test_gpu_dcn_tapwin_edges.py: label -> (B, C, dg, Co, H, W); C / dg is the kernels' CPG template argument.
EDGE_GEOMS = {
    'A': (1, 16, 2, 32, 8, 32),      # CPG 8, MT 1, exactly one tile
    'B': (2, 64, 8, 72, 9, 36),      # CPG 8, MT 3 with a ragged last channel tile, ragged tiles both ways
    'C': (1, 16, 1, 64, 1, 32),      # CPG 16, MT 2, one row: the second pixel row of every wave is dead
    'D': (1, 128, 8, 160, 17, 68),   # CPG 16, MT 4 + an MT 1 launch, three tile rows and columns, ragged
    'E': (3, 32, 2, 128, 8, 64),     # CPG 16, MT 4, strided offsets / masks, x at a storage offset, no bias
}
EDGE_FIELDS = ('ladder', 'ladder_int', 'outward', 'noise1', 'noise3')
LADDER_FIELDS = ('ladder', 'ladder_int')


def edge_field(label, field):
    """The offsets (B, dg * 18, H, W) of geometry `label` for one of EDGE_FIELDS."""
    B, C, dg, Co, H, W = EDGE_GEOMS[label]
    seed = H * W + dg
    if field == 'ladder':
        return ladder_field(B, dg, H, W, seed, 0.25)
    if field == 'ladder_int':
        return ladder_field(B, dg, H, W, seed, 0.0)
    if field == 'outward':
        return outward_field(B, dg, H, W, seed)
    return noise_field(B, dg, H, W, seed, {'noise1': 1.0, 'noise3': 3.0}[field])
