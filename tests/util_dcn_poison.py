"""Offset fields as a diverging conv_offset produces them: taps thrown thousands of pixels out, beyond the range of `int`, to FLT_MAX,
to +-inf and to NaN.  CPU only; the base fields and geometries are those of tests/util_tapwin.py (forward) and tests/util_dcn_bwd.py
(backward), of which a share of the taps is overwritten here.

The rule under test (include/edvr_amd.h, next to the DCN entry points): a sampling position outside (-1, H) x (-1, W) - +-inf and NaN
included - adds nothing to y, dX or dW and has dOffset = dMask = 0.  Every poison value is at least 1e4 in magnitude and every geometry
at most 70 pixels high and wide, so a poisoned tap is invalid in float32 and in float64 whichever component carries the value: the
oracle's result does not depend on the value at all, and one reference serves every kind (tests/test_dcn_poison_cpu.py proves both)."""
import functools

import numpy as np
import torch

import util_dcn_bwd
import util_tapwin

TH, TW = util_tapwin.TH, util_tapwin.TW   # the 8 x 32 pixel tile of the tile kernels, forward and backward alike
assert (TH, TW) == (util_dcn_bwd.TH, util_dcn_bwd.TW)
FLT_MAX = float(np.finfo(np.float32).max)
INF, NAN = float('inf'), float('nan')

# kind -> the magnitudes a poisoned offset component takes (the sign is drawn per entry).  2147483520 is the largest float32 below 2^31,
# 2147483648 = 2^31 the first value (int)floorf() cannot hold.
KINDS = {
    'far': (1.0e4,),
    'int_range': (2147483520., 2147483648., 3.0e9),
    'fltmax': (3.0e38, FLT_MAX),
    'inf': (INF,),
    'nan': (NAN,),
}
KINDS['mixed'] = tuple(v for k in ('far', 'int_range', 'fltmax', 'inf', 'nan') for v in KINDS[k])
# float16 holds none of the finite values above: +-6.0e4 (< 65504) stands for all of them
KINDS_F16 = {'far': (6.0e4,), 'int_range': (6.0e4,), 'fltmax': (6.0e4,), 'inf': (INF,), 'nan': (NAN,), 'mixed': (6.0e4, INF, NAN)}
DEAD_MOD, DEAD_REM = 7, 3   # the dead pixels:  (y * W + x) % 7 == 3
DEAD_TILE_SHARE = 0.2       # the dead tile holds at most this share of the batch's pixels


def dead_pixels(H, W):
    """(H, W) bool: the pixels all of whose taps are poisoned, in every image.  An image of fewer than 56 pixels (geometry C: 1 x 32)
    would hold fewer than eight of them: there the modulus is  H * W // 8  (C: every fourth pixel)."""
    return (torch.arange(H * W) % min(DEAD_MOD, H * W // 8) == DEAD_REM).view(H, W)


def dead_tile(B, H, W):
    """(ty0, tx0, rows, columns) of the tile of IMAGE 0 all of whose taps are poisoned, None where the image is one tile.  Of the tiles
    that hold at most DEAD_TILE_SHARE of the batch's pixels - with the random quarter and the dead pixels the poisoned share then stays
    below  1 - 3/4 x 6/7 x 4/5 = 48.6 % - it is the widest, then the tallest, then the first in raster order: in every tile kernel a
    wave's lanes run along a pixel row of the tile, so a dead tile of full width leaves whole half-waves (and, 8 rows high, the whole
    workgroup) without a valid tap, which is what the wave-uniform branches see.  A whole 8 x 32 tile in the geometries E (forward) and
    F1 (backward); where one such tile is a larger part of the batch (B, D, S1, S2) the 1 x 32 tile of the ragged last tile row."""
    tiles = [(ty0, tx0, min(TH, H - ty0), min(TW, W - tx0)) for ty0 in range(0, H, TH) for tx0 in range(0, W, TW)]
    if len(tiles) == 1:
        return None
    fit = [t for t in tiles if t[2] * t[3] <= DEAD_TILE_SHARE * B * H * W]
    return max(fit, key=lambda t: (t[3], t[2]))  # (max returns the first of equals)


def poison_mask(B, dg, H, W, seed):
    """(B, dg * 9, H, W) bool over (tap, pixel): the union of  (a) a seeded random quarter of all entries,  (b) every tap of every pixel
    of the dead tile (`dead_tile`),  (c) every tap of the dead pixels (`dead_pixels`)."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(B, dg * 9, H, W, generator=g) < 0.25
    tile = dead_tile(B, H, W)
    if tile is not None:
        ty0, tx0, th, tw = tile
        mask[0, :, ty0:ty0 + th, tx0:tx0 + tw] = True
    mask[:, :, dead_pixels(H, W)] = True
    return mask


def components(mask, seed):
    """(B, dg * 9, H, W) int64: which component of a poisoned entry carries the value - 0 dy, 1 dx, 2 both -, a third of the entries
    each (a seeded permutation dealt out in turn); -1 at the unpoisoned entries.  Depends on the mask and the seed alone: every kind
    poisons the same components."""
    g = torch.Generator().manual_seed(seed + 1)
    idx = mask.flatten().nonzero().flatten()
    comp = torch.full((mask.numel(),), -1, dtype=torch.int64)
    comp[idx[torch.randperm(idx.numel(), generator=g)]] = torch.arange(idx.numel()) % 3
    return comp.view(mask.shape)


def poison(off, mask, kind, seed, half=False):
    """off (B, dg * 18, H, W) with the entries of `mask` overwritten: the component(s) `components` names take a value of KINDS[kind]
    (KINDS_F16[kind] with half=True) drawn per entry and component, under a sign drawn per entry and component.  The OFFSET is
    overwritten, not the sampling position (position = integer + offset).  Returns a new tensor of off's dtype."""
    B, planes, H, W = off.shape
    assert mask.shape == (B, planes // 2, H, W) and mask.dtype == torch.bool
    vals = torch.tensor((KINDS_F16 if half else KINDS)[kind], dtype=torch.float64)
    comp = components(mask, seed)
    g = torch.Generator().manual_seed(seed + 2 + 7 * sorted(KINDS).index(kind))
    pick = vals[torch.randint(0, len(vals), (B, planes // 2, 2, H, W), generator=g)]
    sign = torch.randint(0, 2, (B, planes // 2, 2, H, W), generator=g).double() * 2 - 1
    hit = torch.stack([(comp == 0) | (comp == 2), (comp == 1) | (comp == 2)], 2)  # (B, dg * 9, 2: dy | dx, H, W)
    out = torch.where(hit, (pick * sign).to(off.dtype), off.view(B, planes // 2, 2, H, W))
    return out.view(B, planes, H, W).contiguous()


def mask_for(geom, label):
    """The poison mask of geometry `label` of util_tapwin.EDGE_GEOMS or util_dcn_bwd.GEOMS (geom = that dict)."""
    B, C, dg, Co, H, W = geom[label]
    return poison_mask(B, dg, H, W, 50000 + 97 * H * W + dg + B)


def poisoned(geom, label, off, kind, half=False):
    """off of geometry `label` poisoned with `kind` under the geometry's own mask -> (field, mask)."""
    mask = mask_for(geom, label)
    return poison(off, mask, kind, 60000 + geom[label][4] * geom[label][5], half), mask


def tap_to_offset_mask(mask):
    """(B, dg * 9, H, W) over taps -> (B, dg * 18, H, W) over offset planes (both components of a tap)."""
    return mask.repeat_interleave(2, dim=1)


def invalid_in_float32(off, dg):
    """(B, dg * 9, H, W) bool: the taps that fail the validity rule  -1 < h < H, -1 < w < W  in float32 NumPy arithmetic (EDVR
    signature: position = pixel - 1 + tap index + offset)."""
    off = np.asarray(off, np.float32)
    B, planes, H, W = off.shape
    oy, ox = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    out = np.zeros((B, dg * 9, H, W), bool)
    with np.errstate(all='ignore'):
        for g in range(dg):
            for t in range(9):
                h = (oy - 1 + t // 3).astype(np.float32) + off[:, g * 18 + 2 * t]
                w = (ox - 1 + t % 3).astype(np.float32) + off[:, g * 18 + 2 * t + 1]
                assert h.dtype == np.float32 and w.dtype == np.float32
                out[:, g * 9 + t] = ~((h > np.float32(-1)) & (w > np.float32(-1)) & (h < np.float32(H)) & (w < np.float32(W)))
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------ the cases of the two test files
FWD_GEOMS, BWD_GEOMS = util_tapwin.EDGE_GEOMS, util_dcn_bwd.GEOMS
FWD_CASES = [('ladder', kind) for kind in KINDS] + [('noise3', 'mixed')]                         # (base field, kind) per forward geometry
BWD_CASES = [('ladder', kind) for kind in KINDS] + [('border', 'mixed'), ('sub', 'mixed')]       # ... per backward route and geometry
FWD_FIELDS, BWD_FIELDS = ('ladder', 'noise3'), ('ladder', 'border', 'sub')


@functools.lru_cache(maxsize=None)
def fwd_tensors(label, field):
    """CPU float32 (x, base offsets, m, w, b) of a forward geometry / base field, shared and never written to; masks uniform in [0, 1);
    geometry E has no bias (as in tests/test_gpu_dcn_tapwin_edges.py)."""
    B, C, dg, Co, H, W = FWD_GEOMS[label]
    g = torch.Generator().manual_seed(81000 + 31 * ord(label) + util_tapwin.EDGE_FIELDS.index(field))
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) * 0.1
    b = torch.randn(Co, generator=g) if label != 'E' else None
    m = torch.rand(B, dg * 9, H, W, generator=g)
    return x, util_tapwin.edge_field(label, field), m, w, b


@functools.lru_cache(maxsize=None)
def fwd_offsets(label, field, kind):
    """(poisoned offsets, tap mask) of a forward case."""
    return poisoned(FWD_GEOMS, label, fwd_tensors(label, field)[1], kind)


@functools.lru_cache(maxsize=None)
def fwd_oracle(label, field, kind='far'):
    """y of the C oracle in fp64.  It is the same for every kind, bit for bit (tests/test_dcn_poison_cpu.py): the GPU tests use 'far'."""
    from oracle import dcn_oracle as O
    x, _, m, w, b = fwd_tensors(label, field)
    off = fwd_offsets(label, field, kind)[0]
    return O.c_forward(x.double(), off.double(), m.double(), w.double(), None if b is None else b.double(), 1, 1, 1, 1, FWD_GEOMS[label][2])


@functools.lru_cache(maxsize=None)
def bwd_offsets(label, field, kind):
    """(poisoned offsets, tap mask) of a backward case; x, m, w, dy are util_dcn_bwd.case_tensors(label, field)."""
    return poisoned(BWD_GEOMS, label, util_dcn_bwd.case_tensors(label, field)[1], kind)


@functools.lru_cache(maxsize=None)
def bwd_oracle(label, field, kind='far'):
    """(dx, doffset, dmask, dweight, dbias) of the C oracle in fp64; the same for every kind, bit for bit."""
    from oracle import dcn_oracle as O
    x, _, m, w, dy = util_dcn_bwd.case_tensors(label, field)
    off = bwd_offsets(label, field, kind)[0]
    return O.c_backward(x.double(), off.double(), m.double(), w.double(), dy.double(), True, 1, 1, 1, 1, BWD_GEOMS[label][2])
