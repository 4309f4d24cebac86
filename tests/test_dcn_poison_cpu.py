"""The inputs of tests/test_gpu_dcn_poison.py, judged without a GPU: tests/util_dcn_poison.py overwrites a share of the taps of the edge
fields with offsets of 1e4 px, beyond the range of `int`, of FLT_MAX, +-inf and NaN.  Shown here, with NumPy and the C oracle alone:
every such tap fails the validity rule in float32; the poisoning leaves the base fields' edge classes populated; the oracle's answer is
finite, does not depend on the poison value at all (so one reference serves every kind), is exactly zero in dOffset / dMask at the
poisoned taps and exactly the bias at pixels without a valid tap; and the host-side statistics -> hint functions take non-finite input.
Conditions on the inputs and on the reference, not measurements of the kernels."""
import numpy as np
import pytest
import torch

import util_dcn_bwd as UB
import util_dcn_poison as P
import util_tapwin as UT

ALL_GEOMS = [(P.FWD_GEOMS, label) for label in sorted(P.FWD_GEOMS)] + [(P.BWD_GEOMS, label) for label in sorted(P.BWD_GEOMS)]
GEOM_IDS = ['fwd-' + l for l in sorted(P.FWD_GEOMS)] + ['bwd-' + l for l in sorted(P.BWD_GEOMS)]


def _base(geom, label):
    return (UT.edge_field if geom is P.FWD_GEOMS else UB.edge_field)(label, 'ladder')


def test_the_value_sets_are_the_ones_the_kernels_cannot_index_with():
    f32 = lambda v: float(np.float32(v))
    assert set(P.KINDS) == {'far', 'int_range', 'fltmax', 'inf', 'nan', 'mixed'} == set(P.KINDS_F16)
    assert P.KINDS['int_range'][0] == f32(np.nextafter(np.float32(2.0 ** 31), np.float32(0))) and P.KINDS['int_range'][1] == 2.0 ** 31
    assert P.KINDS['fltmax'][1] == f32(np.finfo(np.float32).max)
    for kind, vals in P.KINDS.items():
        for v in vals:
            assert np.isnan(v) or np.isinf(v) or (v >= 1.0e4 and np.isfinite(f32(v)) and abs(f32(v) - v) <= 1e-7 * v), (kind, v)  # finite stays finite in float32
    for kind, vals in P.KINDS_F16.items():
        for v in vals:
            assert np.isnan(v) or np.isinf(v) or (v == 6.0e4 and float(np.float16(v)) == v), (kind, v)
    assert len(P.KINDS['mixed']) == 8 and sum(np.isnan(v) for v in P.KINDS['mixed']) == 1
    assert max(max(g[4], g[5]) for geom in (P.FWD_GEOMS, P.BWD_GEOMS) for g in geom.values()) <= 70


@pytest.mark.parametrize('geom,label', ALL_GEOMS, ids=GEOM_IDS)
def test_every_poisoned_tap_is_invalid_in_float32_and_nothing_else_changes(geom, label):
    """Per geometry and kind, in float32 NumPy: every poisoned tap fails  -1 < h < H && -1 < w < W;  the unpoisoned entries keep their
    bits; every value of the kind occurs, under both signs; every kind poisons the same components."""
    B, C, dg, Co, H, W = geom[label]
    base = _base(geom, label)
    comp0 = None
    for kind in P.KINDS:
        off, mask = P.poisoned(geom, label, base, kind)
        assert off.dtype == torch.float32 and off.shape == base.shape and mask.shape == (B, dg * 9, H, W)
        assert P.invalid_in_float32(off.numpy(), dg)[mask].all(), kind
        changed = ~((off == base) | (torch.isnan(off) & torch.isnan(base)))
        assert not changed[~P.tap_to_offset_mask(mask)].any()
        comp = torch.where(changed[:, 0::2] & changed[:, 1::2], 2, torch.where(changed[:, 1::2], 1, torch.where(changed[:, 0::2], 0, -1)))
        assert ((comp >= 0) == mask).all()  # (|base| <= 30: a poisoned component never equals what it replaces)
        comp0 = comp if comp0 is None else comp0
        assert torch.equal(comp, comp0), kind
        hit = off[changed]
        for v in P.KINDS[kind]:
            if np.isnan(v):
                assert torch.isnan(hit).any()
            elif hit.numel() >= 64 * len(P.KINDS[kind]):  # (geometry C holds ~100 poisoned taps: not every value of `mixed` under both signs)
                assert (hit == v).any() and (hit == -v).any(), (kind, v)
    # float64 sees the same taps invalid: the oracle's rule on the same numbers
    off64 = P.poisoned(geom, label, base, 'mixed')[0].double().numpy()
    oy, ox = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    with np.errstate(all='ignore'):
        for g in range(dg):
            for t in range(9):
                h, w = oy - 1 + t // 3 + off64[:, g * 18 + 2 * t], ox - 1 + t % 3 + off64[:, g * 18 + 2 * t + 1]
                assert not ((h > -1) & (w > -1) & (h < H) & (w < W))[mask[:, g * 9 + t].numpy()].any()


@pytest.mark.parametrize('geom,label', ALL_GEOMS, ids=GEOM_IDS)
def test_mask_shares_components_dead_pixels_and_sample_pixels(geom, label):
    B, C, dg, Co, H, W = geom[label]
    mask = P.mask_for(geom, label)
    share = mask.float().mean().item()
    assert 0.25 <= share <= 0.50, share
    comp = P.components(mask, 60000 + H * W)
    counts = [int((comp == i).sum()) for i in range(3)]
    assert min(counts) >= 32 and max(counts) - min(counts) <= 1 and sum(counts) == int(mask.sum()), counts
    dead = P.dead_pixels(H, W)
    assert int(dead.sum()) >= 8 and mask[:, :, dead].all()
    assert (H * W >= 56) == (int(dead.sum()) == len([p for p in range(H * W) if p % 7 == 3]))  # the rule of the docstring, but for geometry C
    tile = P.dead_tile(B, H, W)
    tiles_y, tiles_x = -(-H // P.TH), -(-W // P.TW)
    assert (tile is None) == (tiles_y * tiles_x == 1)
    if tile is None:
        return
    ty0, tx0, th, tw = tile
    assert mask[0, :, ty0:ty0 + th, tx0:tx0 + tw].all() and tw == P.TW and th * tw <= P.DEAD_TILE_SHARE * B * H * W
    assert not mask[1:, :, ty0:ty0 + th, tx0:tx0 + tw].all() if B > 1 else True
    # the pre-pass of the tap-window kernels reads eight sample pixels per tile and plane: in at least one tile other than the dead one
    # a sample pixel is poisoned (in both planes of that tap for a third of them), so tile_shifts - and the kernels' pre-pass - see the value
    samp = UT.sample_pixel_mask(H, W)
    seen = 0
    for y0 in range(0, H, P.TH):
        for x0 in range(0, W, P.TW):
            if (y0, x0) != (ty0, tx0):
                sel = torch.zeros(H, W, dtype=torch.bool)
                sel[y0:y0 + P.TH, x0:x0 + P.TW] = True
                seen += int(mask[:, :, sel & samp & ~dead].any())
    assert seen >= 1


def test_whole_tiles_are_dead_where_the_batch_allows_it():
    assert P.dead_tile(*[P.FWD_GEOMS['E'][i] for i in (0, 4, 5)]) == (0, 0, 8, 32)
    assert P.dead_tile(*[P.BWD_GEOMS['F1'][i] for i in (0, 4, 5)]) == (0, 0, 8, 32)
    assert P.dead_tile(*[P.FWD_GEOMS['D'][i] for i in (0, 4, 5)]) == (16, 0, 1, 32)
    assert P.dead_tile(1, 8, 32) is None and P.dead_tile(1, 1, 32) is None


def test_tap_window_edge_classes_survive_the_poisoning(capsys):
    """The census of tests/util_tapwin.py over the UNPOISONED taps, per kernel instance family as tests/test_tapwin_geom_cpu.py takes it,
    on the `ladder` field the GPU file runs: at least half a wave of lanes in each of the eight edge classes.  The `nan` kind gives that
    census directly: a NaN tap is invalid, so it is in no class, and fminf / fmaxf drop NaN samples, so the windows stay where the base
    field puts them.  (Single geometries do not reach the floor unpoisoned either - A holds 1 lane in rx = IW - 2, C fewer than 10 in
    all -, which is why the floor is per family there and here.)
    Printed as well: the same census under `inf`.  There a plane with one poisoned sample pixel has its window sent 16384 px away and
    every valid lane of the tile goes through the fix-up pass - what a diverged field does to these kernels, and the reason the window
    classes are asserted on `nan` only."""
    with capsys.disabled():
        for cpg in (8, 16):
            tot = {kind: UT.new_census() for kind in ('nan', 'inf')}
            for label, (B, C, dg, Co, H, W) in P.FWD_GEOMS.items():
                if C // dg == cpg:
                    for kind in tot:
                        tot[kind] = UT.add_census(tot[kind], UT.census(P.fwd_offsets(label, 'ladder', kind)[0], dg))
            for kind, c in tot.items():
                print('\ntap-window census, ladder field poisoned with %s, CPG = %d:' % (kind, cpg))
                for line in UT.census_table(c):
                    print('  ' + line)
            for k in UT.EDGE_CLASSES:
                assert tot['nan'][k] >= 32, (cpg, k, tot['nan'][k])
            assert tot['nan']['inside'] > 0 and tot['nan']['fixup'] > 0
            assert tot['inf']['fixup'] > 4 * tot['inf']['inside']  # most windows have left
            assert tot['inf']['valid'] == tot['nan']['valid']      # the same taps count


def test_backward_edge_classes_survive_the_poisoning(capsys):
    """The census of tests/util_dcn_bwd.py over the unpoisoned taps, per route over its geometries and all fields as
    tests/test_dcn_bwd_geom_cpu.py takes it: at least 32 taps in every class that file asserts.  (No window moves in the backward: the
    census is the same under every kind; a poisoned tap is in no class, each of which needs a valid tap or an exact finite position.)"""
    with capsys.disabled(), np.errstate(all='ignore'):
        for route, (hint, labels) in UB.ROUTES.items():
            tot = UB.new_census(route)
            for label in labels:
                for field in UB.FIELDS:
                    off, mask = P.poisoned(P.BWD_GEOMS, label, UB.edge_field(label, field), 'mixed')
                    c = UB.census(off, P.BWD_GEOMS[label][2], route)
                    assert c['valid'] <= c['taps'] - int(mask.sum())
                    tot = UB.add_census(tot, c)
            print('\nDCN backward census over the unpoisoned taps, route %s, geometries %s, all fields:' % (route, ' '.join(labels)))
            for line in UB.census_table(tot, route):
                print('  ' + line)
            for k in UB.GENERIC_CLASSES + UB.ROUTE_CLASSES[route]:
                assert tot[k] >= 32, (route, k, tot[k])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize('field', P.FWD_FIELDS)
@pytest.mark.parametrize('label', sorted(P.FWD_GEOMS))
def test_oracle_forward_is_finite_and_blind_to_the_poison_value(label, field):
    x, base, m, w, b = P.fwd_tensors(label, field)
    assert base.abs().max().item() <= 30. and all(torch.isfinite(t).all() for t in (x, base, m, w) + (() if b is None else (b,)))
    ref = P.fwd_oracle(label, field)
    assert ref.dtype == torch.float64 and torch.isfinite(ref).all()
    for kind in P.KINDS:
        assert _same_bits(P.fwd_oracle(label, field, kind), ref), kind
    dead = P.dead_pixels(*P.FWD_GEOMS[label][4:])
    want = torch.zeros(ref.shape[1], dtype=torch.float64) if b is None else b.double()
    assert (b is None) == (label == 'E')
    assert torch.equal(ref[:, :, dead], want.view(1, -1, 1).expand(ref.shape[0], -1, int(dead.sum())))
    tile = P.dead_tile(*[P.FWD_GEOMS[label][i] for i in (0, 4, 5)])
    if tile is not None:
        ty0, tx0, th, tw = tile
        assert torch.equal(ref[0, :, ty0:ty0 + th, tx0:tx0 + tw], want.view(-1, 1, 1).expand(-1, th, tw))
    assert not torch.equal(ref, want.view(1, -1, 1, 1).expand_as(ref))  # (the live pixels do hold something)


@pytest.mark.parametrize('field', P.BWD_FIELDS)
@pytest.mark.parametrize('label', sorted(P.BWD_GEOMS))
def test_oracle_backward_is_finite_blind_to_the_poison_value_and_zero_at_poisoned_taps(label, field):
    from oracle import dcn_oracle as O
    x, base, m, w, dy = UB.case_tensors(label, field)
    ref = P.bwd_oracle(label, field)
    assert len(ref) == 5 and all(r.dtype == torch.float64 and torch.isfinite(r).all() for r in ref)
    for kind in P.KINDS:
        got = P.bwd_oracle(label, field, kind)
        for name, a, r in zip(('dx', 'doffset', 'dmask', 'dweight', 'dbias'), got, ref):
            assert _same_bits(a, r), (kind, name)
    mask = P.bwd_offsets(label, field, 'far')[1]
    assert (ref[1][P.tap_to_offset_mask(mask)] == 0).all() and (ref[2][mask] == 0).all()
    assert (ref[1] != 0).any() and (ref[2] != 0).any() and (ref[0] != 0).any()
    # the forward of the same case: finite, and 0 (no bias) at the dead pixels
    dg = P.BWD_GEOMS[label][2]
    y = O.c_forward(x.double(), P.bwd_offsets(label, field, 'mixed')[0].double(), m.double(), w.double(), None, 1, 1, 1, 1, dg)
    assert torch.isfinite(y).all() and (y[:, :, P.dead_pixels(*P.BWD_GEOMS[label][4:])] == 0).all()
    # the oracle run in float32 takes the same cells: the dOffset comparison of the GPU file excludes nothing
    off = P.bwd_offsets(label, field, 'far')[0]
    r32 = O.c_backward(x, off, m, w, dy, True, 1, 1, 1, 1, dg)
    assert not ((r32[1].double() - ref[1]).abs() > 1e-3 * ref[1].abs().max()).any()


def test_statistics_to_hint_functions_take_non_finite_input():
    """What a diverged clip leaves behind for the next call's kernel choice: absmean / rough of inf, NaN, 3e38.  Every answer is a legal
    hint, nothing raises."""
    from edvr_amd import functional as F_, ops
    halo_ok = {3, 7, -1, ops.DCN_HALO_TAPWIN}
    scatter_ok = {ops.DCN_SCATTER_DEVICE, ops.DCN_SCATTER_LDS, ops.DCN_SCATTER_STRIP, ops.DCN_SCATTER_LDS_WIDE}
    bad = (float('inf'), float('-inf'), float('nan'), 3.0e38)
    for a in bad + (None, 0.3, 8.0):
        for r in bad + (None, 0.2, 60.0):
            for ok in (True, False):
                assert F_.halo_hint_from_stats(a, r, ok) in halo_ok, (a, r, ok)
            assert F_.scatter_hint_from_stats(a, r) in scatter_ok, (a, r)
    assert F_.scatter_hint_from_stats(float('inf'), None) == ops.DCN_SCATTER_LDS_WIDE and F_.scatter_hint_from_stats(3.0e38, 0.1) == ops.DCN_SCATTER_LDS_WIDE
    assert F_.scatter_hint_from_stats(float('nan'), float('nan')) == ops.DCN_SCATTER_LDS  # (NaN fails every comparison: the window kernel, safe on any field)
    assert F_.halo_hint_from_stats(3.0e38, 3.0e38) == -1                                  # finite and huge: the column-buffer class
    for v in bad:
        st = torch.tensor([[v, 1.0], [v, 2.0]])  # (2, n) sums of abs_stats_per_image, one image non-finite
        a, r = ops.offset_stats(st, 16)
        assert isinstance(a, float) and (r is None or isinstance(r, float))
        assert F_.halo_hint_from_stats(a, r) in halo_ok and F_.scatter_hint_from_stats(a, r) in scatter_ok
        a, r = ops.offset_stats(torch.tensor([v, 1.0]), 16)  # the one-row form: no roughness
        assert isinstance(a, float) and r is None
    a, r = ops.offset_stats(torch.tensor([[3.0e38, 3.0e38], [-1.0, -1.0]]), 16)  # float32 sums that overflow only when added up: done in double
    assert np.isfinite(a) and r is None
