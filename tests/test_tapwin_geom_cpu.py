"""The inputs of tests/test_gpu_dcn_tapwin_edges.py, judged without a GPU: tests/util_tapwin.py restates the window geometry of the
tap-window DCNv2 forward kernels; here its constants are pinned to the two .hip files, its arithmetic is checked on fields whose
answer is known, and the edge fields are PROVEN to put lanes on every window edge, at every column alignment, and windows over every
image border - a condition on the inputs, not a measurement of the kernels."""
import os
import re

import numpy as np
import torch

import util_tapwin as U

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'edvr_amd', 'csrc')


def _constants(fname, prefix):
    """TH, TW, RY, RX, IH, IW of a kernel file: the literal ones parsed, the derived ones evaluated from their own expressions."""
    src = open(os.path.join(CSRC, fname)).read()
    vals = {}
    lit = re.search(r'constexpr int %s_TH = (\d+), %s_TW = (\d+), %s_RY = (\d+), %s_RX = (\d+);' % ((prefix,) * 4), src)
    assert lit, fname
    vals.update(zip(('TH', 'TW', 'RY', 'RX'), map(int, lit.groups())))
    for name in ('IH', 'IW'):
        m = re.search(r'constexpr int %s_%s = ([^;]+);' % (prefix, name), src)
        assert m, (fname, name)
        expr = re.sub(r'%s_(\w+)' % prefix, lambda k: str(vals[k.group(1)]), m.group(1))
        assert re.fullmatch(r'[\d\s+\-*/()]+', expr), expr
        vals[name] = int(eval(expr.replace('/', '//')))  # (C integer division; every operand is positive)
    return vals


def test_window_constants_of_both_kernels_and_the_restatement_agree():
    fp32, split = _constants('dcn_tapwin.hip', 'TWN'), _constants('dcn_tapwin_s.hip', 'TWS')
    mine = dict(TH=U.TH, TW=U.TW, RY=U.RY, RX=U.RX, IH=U.IH, IW=U.IW)
    assert fp32 == split == mine, (fp32, split, mine)
    assert (U.IH, U.IW) == (12, 40)
    # the window predicate and the origin arithmetic, as text: both files carry the same lines
    for fname, p in (('dcn_tapwin.hip', 'TWN'), ('dcn_tapwin_s.hip', 'TWS')):
        src = open(os.path.join(CSRC, fname)).read()
        assert 'const bool inside = valid && ry >= 0 && ry <= IH - 2 && rx >= 0 && rx <= IW - 2;' in src, fname
        assert 'wy0 = ty0 - 1 + ti + sy - %s_RY;' % p in src and 'wx0 = (tx0 - 1 + tj + sx - %s_RX) & ~3;' % p in src, fname
        assert 'for (int r = 1; r < TH; r += 4)' in src and 'for (int c = 4; c < TW; c += 8)' in src, fname
    assert U.SAMPLE_ROWS == tuple(range(1, U.TH, 4)) and U.SAMPLE_COLS == tuple(range(4, U.TW, 8))


def test_zero_field_is_all_inside_with_zero_shifts():
    dg, H, W = 2, 17, 68
    off = np.zeros((dg * 18, H, W), np.float32)
    for g in range(dg):
        for t in range(9):
            q = U.tap_geometry(off, g, t)
            assert (q['sy'] == 0).all() and (q['sx'] == 0).all()
            assert (q['inside'] == q['valid']).all()
    c = U.census(off[None], dg)
    # the taps of a regular 3 x 3 convolution with zero padding: all but the border ring's outer taps are valid
    assert c['valid'] == c['inside'] == dg * sum((H - abs(i)) * (W - abs(j)) for i in (-1, 0, 1) for j in (-1, 0, 1)) and c['fixup'] == 0


def test_constant_field_shifts_by_the_constant_and_centres_every_lane():
    dg, H, W = 1, 16, 64
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    for k in (-7, -1, 3, 12):
        off = np.full((18, H, W), k, np.float32)
        for t in range(9):
            q = U.tap_geometry(off, 0, t)
            assert (q['sy'] == k).all() and (q['sx'] == k).all()
            assert (q['ry'][q['valid']] == (oy % U.TH + U.RY)[q['valid']]).all()      # row of the tile + RY
            col = (ox % U.TW + U.RX + q['align'])[q['valid']]                          # column of the tile + RX + what the alignment lost
            assert (q['rx'][q['valid']] == col).all() and col.max() <= U.IW - 2
            assert (q['inside'] == q['valid']).all()
    # a fraction below one half rounds to the same shift, one half rounds up (floorf(mid + 0.5f))
    assert (U.tile_shifts(np.full((8, 32), 2.25, np.float32)) == 2).all() and (U.tile_shifts(np.full((8, 32), 2.5, np.float32)) == 3).all()
    assert (U.tile_shifts(np.full((8, 32), -2.5, np.float32)) == -2).all() and (U.tile_shifts(np.full((8, 32), -2.75, np.float32)) == -3).all()


def test_shift_of_non_finite_sample_pixels_follows_the_fminf_fmaxf_clamp_chain():
    """Arithmetic only (the kernels take such input in tests/test_gpu_dcn_poison.py): fminf / fmaxf drop a NaN operand;
    0.5f * (-Inf + Inf) is NaN, which fmaxf(., -16384) turns into -16384."""
    nan, inf, flt_max = float('nan'), float('inf'), float(np.finfo(np.float32).max)
    def shift(vals):  # the eight sample pixels of one 8 x 32 tile, every other pixel 100 (never read)
        pl = np.full((8, 32), 100., np.float32)
        for v, (r, c) in zip(vals, [(r, c) for r in U.SAMPLE_ROWS for c in U.SAMPLE_COLS]):
            pl[r, c] = v
        return int(U.tile_shifts(pl)[0, 0])
    assert shift([2.] * 8) == 2
    assert shift([nan] * 8) == 0                           # mn = 3e38, mx = -3e38 survive: mid = 0
    assert shift([nan, 1., 5., nan, 1., 5., 3., 3.]) == 3  # NaNs dropped: mid-range of the rest
    assert shift([inf] + [0.] * 7) == 16384
    assert shift([-inf] + [0.] * 7) == -16384
    assert shift([inf, -inf] + [0.] * 6) == -16384
    assert shift([1e9] + [0.] * 7) == 16384 and shift([-1e9] + [0.] * 7) == -16384
    assert shift([3e38] * 8) == 16384                      # mn + mx overflows to +Inf: clamped
    # ... every sample non-finite, and the values of tests/util_dcn_poison.py next to ordinary ones
    assert shift([inf] * 8) == 16384 and shift([-inf] * 8) == -16384 and shift([-3e38] * 8) == -16384
    assert shift([-inf, inf] * 4) == -16384                # mn = -Inf, mx = +Inf: mid = NaN
    assert shift([nan] * 6 + [-inf, inf]) == -16384 and shift([nan] * 7 + [inf]) == 16384 and shift([nan] * 7 + [-inf]) == -16384
    assert shift([nan, inf, 2., 2., 2., 2., 2., 2.]) == 16384 and shift([nan, -inf, 2., 2., 2., 2., 2., 2.]) == -16384
    assert shift([flt_max, -flt_max] + [0.] * 6) == 0      # mn + mx = 0 exactly: no overflow on the way
    assert shift([flt_max] + [0.] * 7) == 16384 and shift([-flt_max] + [0.] * 7) == -16384
    assert shift([1e4] + [0.] * 7) == 5000 and shift([-1e4] + [2.] * 7) == -4999  # 'far' is inside the clamp: half way out
    assert shift([2147483520.] + [0.] * 7) == 16384 and shift([-2147483648.] + [0.] * 7) == -16384 and shift([3e9, -3e9] + [0.] * 6) == 0


def _ladder_census(cpg):
    tot = U.new_census()
    for label, (B, C, dg, Co, H, W) in U.EDGE_GEOMS.items():
        if C // dg != cpg:
            continue
        for field in U.LADDER_FIELDS:
            tot = U.add_census(tot, U.census(U.edge_field(label, field), dg))
    return tot


def test_ladder_fields_put_lanes_on_every_window_edge_at_every_alignment(capsys):
    """The coverage condition, per kernel instance family (8 / 16 channels per deformable group): over the GPU test's geometries and
    both ladder fields, at least half a wave of taps in each of the eight edge classes, at least one per (rx class, alignment)."""
    with capsys.disabled():
        for cpg in (8, 16):
            c = _ladder_census(cpg)
            print('\ntap-window census, ladder fields, CPG = %d:' % cpg)
            for line in U.census_table(c):
                print('  ' + line)
            for k in U.EDGE_CLASSES:
                assert c[k] >= 32, (cpg, k, c[k])
            for k in U.RX_CLASSES:
                for a in range(4):
                    assert c[(k, a)] >= 1, (cpg, k, a)
            for a in range(4):
                assert c[('align', a)] >= 1, (cpg, a)
            for b in U.BORDERS:
                assert c[('clipped', b)] >= 1, (cpg, b)
            assert c['outside'] >= 1 and c['fixup'] > 0 and c['inside'] > 0


def test_ladder_shifts_are_the_bases_and_offsets_stay_small():
    for label, (B, C, dg, Co, H, W) in U.EDGE_GEOMS.items():
        for field, frac in (('ladder', 0.25), ('ladder_int', 0.0)):
            off = U.edge_field(label, field)
            assert off.abs().max().item() <= 30.
            samp = U.sample_pixel_mask(H, W)
            for v in range(dg * 18):
                vals = off[:, v][:, samp]
                assert (vals == vals.flatten()[0]).all()  # every sample pixel of every tile and image carries base + frac
                assert (U.tile_shifts(off[0, v].numpy()) == round(vals.flatten()[0].item() - frac)).all()
            assert ((off - frac) == (off - frac).round()).all()
        for field in ('outward', 'noise1', 'noise3'):
            assert U.edge_field(label, field).abs().max().item() <= 30.


def test_outward_fields_clip_windows_at_every_border(capsys):
    with capsys.disabled():
        for cpg in (8, 16):
            tot = U.new_census()
            for label, (B, C, dg, Co, H, W) in U.EDGE_GEOMS.items():
                if C // dg == cpg:
                    c = U.census(U.edge_field(label, 'outward'), dg)
                    assert c['fixup'] == 0  # constant planes: no lane leaves its window; what is tested is the clipping of the window itself
                    tot = U.add_census(tot, c)
            print('\ntap-window census, outward fields, CPG = %d:' % cpg)
            for line in U.census_table(tot):
                print('  ' + line)
            for b in U.BORDERS:
                assert tot[('clipped', b)] >= 1, (cpg, b)
            assert tot['outside'] >= 1, cpg


def test_smooth_fields_of_the_older_cases_never_reach_four_of_the_edge_classes():
    """Why the edge file exists: over the smooth fields of TAPWIN_CASES (tests/test_gpu_dcn.py) no lane sits in the window's last column,
    one row below it, or one column to either side of it.  Whoever enriches those cases deletes this assertion."""
    import test_gpu_dcn as T
    tot = U.new_census()
    for i, (B, C, H, W, Co, dg, sigma, outliers, act) in enumerate(T.TAPWIN_CASES):
        if dg > 8:  # (falls back to the halo kernel)
            continue
        g = torch.Generator().manual_seed(1000 + i)
        torch.randn(B, C, H, W, generator=g), torch.randn(Co, C, 3, 3, generator=g), torch.randn(Co, generator=g)  # the draws the tests make first
        tot = U.add_census(tot, U.census(T._smooth_field(B, dg, H, W, sigma, g, outliers=outliers), dg))
    assert tot['inside'] > 100000
    assert tot['rx=IW-2'] == 0 and tot['ry=IH-1'] == 0 and tot['rx=-1'] == 0 and tot['rx=IW-1'] == 0, {k: tot[k] for k in U.EDGE_CLASSES}
