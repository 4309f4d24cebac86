"""The cell geometry of the five dX routes of the DCNv2 backward (csrc/dcn.hip, csrc/dcn_bwd_fused.hip) restated in NumPy, a census of
sampling positions by their place relative to each route's window, and offset fields that put taps on every window edge and on the
exact limits of the validity rule.  CPU only; what tests/util_tapwin.py is for the forward.

Every route resolves a tap the same way:  h = (oy - 1 + ti) + dy,  w = (ox - 1 + tj) + dx  in float32; the tap counts iff
-1 < h < H and -1 < w < W; its 2 x 2 bilinear cell starts at (h0, w0) = floor; corners outside the image carry no weight.  They differ
in where the cell's dX contributions go:
  dcn_bwd_fused_kernel           a workgroup owns an 8 x 32 tile; the x window is the tile + 3 on every side (IH x IW = 14 x 38); with
                                 (wr, wc) = (h0, w0) - (tile - 3):  xw = 0 <= wr <= IH - 2 && 0 <= wc <= IW - 2.  sub (floor of both
                                 offsets in {-1, 0}) -> wave-private LDS rows; mid = xw && !sub -> device atomics, x from the window;
                                 slow = valid && !xw -> global memory throughout
  dcn_bwd_coord_tile_kernel<R>   8 x 32 tile, LDS window (10 + 2R) x (34 + 2R) from tile - 1 - R; ly = r + ti + fy + R (r: row in the
                                 tile, fy: floor of the offset), inwin = 0 <= ly <= LH - 2 && 0 <= lx <= LW - 2, else device atomics
  dcn_bwd_dx_strip_kernel        lane = column of a 64-column strip; near = fy, fx in {-1, 0} -> 5 x 5 register patch, folded onto the
                                 owner lanes by wave shifts; lanes 0, 1, 62, 63 send the patch columns that belong to the neighbouring
                                 strip to their cells directly; far -> device atomics
  dcn_bwd_coord_kernel           device atomics, no window
tests/test_dcn_bwd_geom_cpu.py pins the constants and predicates to the .hip files."""
import numpy as np
import torch

TH, TW = 8, 32                        # the tile of the fused and the window kernels
BF_MARGIN = 3
BF_IH, BF_IW = TH + 2 * BF_MARGIN, TW + 2 * BF_MARGIN
STRIP_W = 64


def tile_window(R):
    """(LH, LW) of dcn_bwd_coord_tile_kernel<R>."""
    return TH + 2 + 2 * R, TW + 2 + 2 * R


GENERIC_CLASSES = ('h==-1', 'h==H', 'w==-1', 'w==W',                # exactly on a strict limit of the validity rule, other axis inside
                   'h0=-1', 'h0=H-1', 'w0=-1', 'w0=W-1',            # valid, one row / column of corners outside the image
                   'sub fy=-1 lh=0', 'sub fx=-1 lw=0')              # sub-pixel tap, an offset of exactly -1.0 on that axis
FUSED_EDGES = ('wr=0', 'wr=IH-2', 'wc=0', 'wc=IW-2', 'wr=-1', 'wr=IH-1', 'wc=-1', 'wc=IW-1')
TILE_EDGES = ('ly=0', 'ly=LH-2', 'lx=0', 'lx=LW-2', 'ly=-1', 'ly=LH-1', 'lx=-1', 'lx=LW-1')
STRIP_EDGES = ('fy=-2', 'fy=1', 'fx=-2', 'fx=1')
STRIP_CROSS = (('cross', 0), ('cross', 1), ('cross', 62), ('cross', 63))
ROUTE_CLASSES = {
    'fused': ('sub', 'mid', 'slow') + FUSED_EDGES,
    'tile3': ('inwin', 'outwin') + TILE_EDGES,
    'tile6': ('inwin', 'outwin') + TILE_EDGES,
    'strip': ('near', 'far') + STRIP_EDGES + STRIP_CROSS,
    'device': (),
}
KERNEL_NAMES = {'fused': 'dcn_bwd_fused_kernel', 'strip': 'dcn_bwd_dx_strip_kernel', 'tile3': 'dcn_bwd_coord_tile_kernel<3>',
                'tile6': 'dcn_bwd_coord_tile_kernel<6>', 'device': 'dcn_bwd_coord_kernel'}


def tap_geometry(off_img, g, t):
    """off_img (dg * 18, H, W) float32 of one image -> dict of (H, W) arrays for tap (g, t): h, w, valid, h0, w0, lh, lw, fy, fx."""
    off_img = np.asarray(off_img, np.float32)
    _, H, W = off_img.shape
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ti, tj = divmod(t, 3)
    h = (oy - 1 + ti).astype(np.float32) + off_img[g * 18 + 2 * t]
    w = (ox - 1 + tj).astype(np.float32) + off_img[g * 18 + 2 * t + 1]
    assert h.dtype == np.float32 and w.dtype == np.float32
    valid = (h > np.float32(-1)) & (w > np.float32(-1)) & (h < np.float32(H)) & (w < np.float32(W))
    fh, fw = np.floor(h), np.floor(w)
    h0, w0 = fh.astype(np.int64), fw.astype(np.int64)
    return dict(h=h, w=w, valid=valid, h0=h0, w0=w0, lh=h - fh, lw=w - fw, fy=h0 - (oy - 1 + ti), fx=w0 - (ox - 1 + tj), oy=oy, ox=ox, ti=ti, tj=tj, H=H, W=W)


def generic_classes(q):
    H, W, h, w, valid = q['H'], q['W'], q['h'], q['w'], q['valid']
    in_h = (h > np.float32(-1)) & (h < np.float32(H))
    in_w = (w > np.float32(-1)) & (w < np.float32(W))
    near = valid & (q['fy'] >= -1) & (q['fy'] <= 0) & (q['fx'] >= -1) & (q['fx'] <= 0)
    return {'h==-1': (h == np.float32(-1)) & in_w, 'h==H': (h == np.float32(H)) & in_w,
            'w==-1': (w == np.float32(-1)) & in_h, 'w==W': (w == np.float32(W)) & in_h,
            'h0=-1': valid & (q['h0'] == -1), 'h0=H-1': valid & (q['h0'] == H - 1),
            'w0=-1': valid & (q['w0'] == -1), 'w0=W-1': valid & (q['w0'] == W - 1),
            'sub fy=-1 lh=0': near & (q['fy'] == -1) & (q['lh'] == 0), 'sub fx=-1 lw=0': near & (q['fx'] == -1) & (q['lw'] == 0)}


def _window_edges(valid, r, c, last_r, last_c, names):
    """The eight edge classes of a window whose usable cell origins are 0 <= r <= last_r, 0 <= c <= last_c."""
    in_r, in_c = valid & (r >= 0) & (r <= last_r), valid & (c >= 0) & (c <= last_c)
    inside = in_r & in_c
    masks = (inside & (r == 0), inside & (r == last_r), inside & (c == 0), inside & (c == last_c),
             in_c & (r == -1), in_c & (r == last_r + 1), in_r & (c == -1), in_r & (c == last_c + 1))
    return inside, dict(zip(names, masks))


def route_classes(q, route):
    """-> {class: (H, W) bool} of ROUTE_CLASSES[route] for one tap's geometry."""
    valid, oy, ox = q['valid'], q['oy'], q['ox']
    ty0, tx0 = oy // TH * TH, ox // TW * TW
    near = (q['fy'] >= -1) & (q['fy'] <= 0) & (q['fx'] >= -1) & (q['fx'] <= 0)
    if route == 'fused':
        wr, wc = q['h0'] - (ty0 - BF_MARGIN), q['w0'] - (tx0 - BF_MARGIN)
        xw, out = _window_edges(valid, wr, wc, BF_IH - 2, BF_IW - 2, FUSED_EDGES)
        sub = valid & near
        assert not (sub & ~xw).any()  # "always inside the window"
        out.update(sub=sub, mid=xw & ~sub, slow=valid & ~xw)
        return out
    if route in ('tile3', 'tile6'):
        R = int(route[4:])
        LH, LW = tile_window(R)
        ly, lx = q['h0'] - (ty0 - 1 - R), q['w0'] - (tx0 - 1 - R)
        assert (ly == (oy - ty0) + q['ti'] + q['fy'] + R).all() and (lx == (ox - tx0) + q['tj'] + q['fx'] + R).all()
        inwin, out = _window_edges(valid, ly, lx, LH - 2, LW - 2, TILE_EDGES)
        out.update(inwin=inwin, outwin=valid & ~inwin)
        return out
    if route == 'strip':
        vn, W = valid & near, q['W']
        out = {'near': vn, 'far': valid & ~near,
               'fy=-2': valid & (q['fy'] == -2) & (q['fx'] >= -1) & (q['fx'] <= 0), 'fy=1': valid & (q['fy'] == 1) & (q['fx'] >= -1) & (q['fx'] <= 0),
               'fx=-2': valid & (q['fx'] == -2) & (q['fy'] >= -1) & (q['fy'] <= 0), 'fx=1': valid & (q['fx'] == 1) & (q['fy'] >= -1) & (q['fy'] <= 0)}
        lane, strip = ox % STRIP_W, ox // STRIP_W
        c0, c1 = q['w0'], q['w0'] + 1
        live0, live1 = c0 >= 0, (c1 <= W - 1) & (q['lw'] > 0)  # cells that carry a non-zero column weight
        left = (live0 & (c0 < strip * STRIP_W)) | (live1 & (c1 < strip * STRIP_W))
        right = (live0 & (c0 >= (strip + 1) * STRIP_W)) | (live1 & (c1 >= (strip + 1) * STRIP_W))
        for ln in (0, 1):
            out[('cross', ln)] = vn & (lane == ln) & left
        for ln in (62, 63):
            out[('cross', ln)] = vn & (lane == ln) & right
        return out
    assert route == 'device'
    return {}


def new_census(route):
    c = {k: 0 for k in ('taps', 'valid', 'lh=0', 'lw=0') + GENERIC_CLASSES + ROUTE_CLASSES[route]}
    return c


def add_census(a, b):
    return {k: a[k] + b[k] for k in a}


def census(off, dg, route):
    """off (B, dg * 18, H, W) -> counts over every (image, group, tap, pixel) of the classes above, for one route."""
    off = np.asarray(off.detach().cpu().numpy() if isinstance(off, torch.Tensor) else off, np.float32)
    B, planes, H, W = off.shape
    assert planes == dg * 18
    c = new_census(route)
    for b in range(B):
        for g in range(dg):
            for t in range(9):
                q = tap_geometry(off[b], g, t)
                c['taps'] += q['valid'].size
                c['valid'] += int(q['valid'].sum())
                c['lh=0'] += int((q['valid'] & (q['lh'] == 0)).sum())
                c['lw=0'] += int((q['valid'] & (q['lw'] == 0)).sum())
                for k, m in generic_classes(q).items():
                    c[k] += int(m.sum())
                for k, m in route_classes(q, route).items():
                    c[k] += int(m.sum())
    return c


def census_table(c, route):
    fmt = lambda keys: '  '.join('%s %d' % (k if isinstance(k, str) else 'cross@lane%d' % k[1], c[k]) for k in keys)
    lines = [fmt(('taps', 'valid', 'lh=0', 'lw=0')), fmt(GENERIC_CLASSES[:4]), fmt(GENERIC_CLASSES[4:8]), fmt(GENERIC_CLASSES[8:])]
    rc = ROUTE_CLASSES[route]
    for i in range(0, len(rc), 6):
        lines.append(fmt(rc[i:i + 6]))
    return lines


# ------------------------------------------------------------------------------------------------ fields
FIELDS = ('ladder', 'ladder_int', 'ladder_half', 'sub', 'border', 'noise16')
EXACT_FIELDS = FIELDS[:5]  # every sampling position is exact in float32: the oracle in float32 takes the same cells as in float64


def ladder_field(B, dg, H, W, seed, frac):
    """Uniform integers in [-9, 9] + frac: every window edge of every route and its neighbour, both ways."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-9, 10, (B, dg * 18, H, W), generator=g).float() + frac).contiguous()


def sub_field(B, dg, H, W, seed):
    """Offsets drawn from {-1, -0.75, ..., 0.75}: every tap sub-pixel, exact -1.0 and 0.0 included."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-4, 4, (B, dg * 18, H, W), generator=g).float() / 4).contiguous()


def border_field(B, dg, H, W, seed):
    """Per axis, half of the taps sit at an ABSOLUTE position drawn from {-1, -1 + 2^-8, -0.5, 0, n - 1, n - 0.5, n - 2^-8, n} (n = H or
    W: the limits of the validity rule, their inner neighbours, the clipped cells), the other half at near-regular positions (offsets
    from {-1, ..., 0.75}).  All exact in float32: position - regular position needs 7 integer and 8 fraction bits."""
    g = torch.Generator().manual_seed(seed)
    ch = torch.arange(dg * 18)
    t, axis = (ch % 18) // 2, ch % 2
    oy, ox = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    base = torch.where(axis.view(-1, 1, 1) == 0, oy[None] - 1 + (t // 3).view(-1, 1, 1), ox[None] - 1 + (t % 3).view(-1, 1, 1)).float()
    n = torch.where(axis == 0, H, W).float().view(1, -1, 1, 1)
    pick = torch.randint(0, 8, (B, dg * 18, H, W), generator=g)
    e = 2.0 ** -8
    rel = torch.tensor([-1., -1. + e, -0.5, 0., -1., -0.5, -e, 0.])[pick]          # position relative to 0 (first four) or to n (last four)
    pos = rel + torch.where(pick >= 4, n.expand_as(rel), torch.zeros_like(rel))
    near = torch.randint(-4, 4, (B, dg * 18, H, W), generator=g).float() / 4
    at_border = torch.rand(B, dg * 18, H, W, generator=g) < 0.5
    off = torch.where(at_border, pos - base[None], near)
    assert ((base[None] + off)[at_border] == pos[at_border]).all()  # float32 throughout: the kernels see exactly `pos`
    return off.contiguous()


def noise_field(B, dg, H, W, seed, sigma=16.0, clamp=60.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, dg * 18, H, W, generator=g) * sigma).clamp_(-clamp, clamp).contiguous()


# label -> (B, C, dg, Co, H, W)
GEOMS = {
    'F1': (2, 32, 2, 24, 17, 70),    # fused under STRIP, tile 3 / tile 6 / device atomics under LDS / LDS_WIDE / DEVICE; 3 x 3 tiles, two strips
    'F2': (1, 16, 1, 128, 8, 32),    # fused with dg = 1 (no next x window), Co = 128, exactly one tile
    'S1': (1, 32, 2, 160, 17, 70),   # Co > 128: STRIP runs the staged strip kernel, 16 channels per group
    'S2': (1, 16, 2, 16, 9, 65),     # 8 channels per group; the second strip has one live lane
}
HINTS = {'auto': 0, 'device': 1, 'lds': 2, 'strip': 3, 'lds_wide': 4}  # EDVR_DCN_SCATTER_*
# route -> (scatter hint, the geometries it is tested on)
ROUTES = {
    'fused': ('strip', ('F1', 'F2')),
    'strip': ('strip', ('S1', 'S2')),
    'tile3': ('lds', ('F1', 'S2')),
    'tile6': ('lds_wide', ('F1', 'S2')),
    'device': ('device', ('F1', 'S2')),
}


def edge_field(label, field):
    """The offsets (B, dg * 18, H, W) float32 of geometry `label` for one of FIELDS."""
    B, C, dg, Co, H, W = GEOMS[label]
    seed = 1000 * FIELDS.index(field) + H * W + dg
    if field.startswith('ladder'):
        return ladder_field(B, dg, H, W, seed, {'ladder': 0.25, 'ladder_int': 0.0, 'ladder_half': 0.5}[field])
    if field == 'sub':
        return sub_field(B, dg, H, W, seed)
    if field == 'border':
        return border_field(B, dg, H, W, seed)
    assert field == 'noise16'
    return noise_field(B, dg, H, W, seed)


def route_census(route):
    """All fields together over the route's geometries."""
    tot = new_census(route)
    for label in ROUTES[route][1]:
        for field in FIELDS:
            tot = add_census(tot, census(edge_field(label, field), GEOMS[label][2], route))
    return tot


def case_tensors(label, field):
    """CPU float32 tensors (x, off, m, w, dy) of a geometry / field; masks uniform in [0, 1)."""
    B, C, dg, Co, H, W = GEOMS[label]
    g = torch.Generator().manual_seed(9000 + 37 * sorted(GEOMS).index(label) + FIELDS.index(field))
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) * 0.1
    m = torch.rand(B, dg * 9, H, W, generator=g)
    dy = torch.randn(B, Co, H, W, generator=g)
    off = edge_field(label, field)
    assert off.abs().max().item() <= 80. and all(torch.isfinite(t).all() for t in (x, off, m, w, dy))
    return x, off, m, w, dy


def oracle_backward(label, field):
    """-> (fp64 gradients of the C oracle, flip): flip marks the dOffset elements where the oracle run in float32 leaves its own
    float64 result by more than 1e-3 of the largest - taps whose float32 position rounds across an integer."""
    from oracle import dcn_oracle as O
    x, off, m, w, dy = case_tensors(label, field)
    dg = GEOMS[label][2]
    ref = O.c_backward(x.double(), off.double(), m.double(), w.double(), dy.double(), True, 1, 1, 1, 1, dg)
    ref32 = O.c_backward(x, off, m, w, dy, True, 1, 1, 1, 1, dg)
    flip = (ref32[1].double() - ref[1]).abs() > 1e-3 * ref[1].abs().max()
    return ref, flip
