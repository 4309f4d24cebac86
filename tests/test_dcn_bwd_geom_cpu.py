"""The inputs of tests/test_gpu_dcn_bwd_edges.py and the backward's kernel choice, judged without a GPU: tests/util_dcn_bwd.py restates
the cell geometry of the five dX routes of the DCNv2 backward; here its constants and predicates are pinned to the .hip files, its
arithmetic is checked on fields whose answer is known, the edge fields are PROVEN to put at least half a wave of taps into every edge
class of every route and onto the exact limits of the validity rule - a condition on the inputs, not a measurement of the kernels -,
and edvr_dcnv2_bwd_kernel_name (the launch's own decision) is compared with a committed table."""
import os
import re

import numpy as np
import pytest
import torch

import util_dcn_bwd as U

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'edvr_amd', 'csrc')


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_constants_and_predicates_of_the_kernels_and_the_restatement_agree():
    fused, dcn, tap = _src('dcn_bwd_fused.hip'), _src('dcn.hip'), _src('dcn_tap.h')
    # ---- the fused kernel: tile, window = tile + 3 on every side, the three classes
    assert re.search(r'#define BF_TH_ROWS (\d+)', fused).group(1) == str(U.TH)
    m = re.search(r'constexpr int BF_TH = BF_TH_ROWS, BF_NT = 64 \* BF_TH, BF_TW = (\d+), BF_IH = BF_TH \+ (\d+), BF_IW = BF_TW \+ (\d+),', fused)
    assert m and (int(m.group(1)), U.TH + int(m.group(2)), int(m.group(1)) + int(m.group(3))) == (U.TW, U.BF_IH, U.BF_IW)
    assert (U.BF_IH, U.BF_IW) == (14, 38)
    for line in ('const int wy0 = ty0 - %d, wx0 = tx0 - %d;' % (U.BF_MARGIN, U.BF_MARGIN),
                 'const float h = (float)(oy - 1 + ti) + o_h, w = (float)(ox - 1 + tj) + o_w;',
                 'const bool valid = act && h > -1.f && w > -1.f && h < (float)a.H && w < (float)a.W;',
                 'const int fy = fhi - (oy - 1 + ti), fx = fwi - (ox - 1 + tj);',
                 'const int wr = fhi - wy0, wc = fwi - wx0;',
                 'const bool xw = valid && wr >= 0 && wr <= IH - 2 && wc >= 0 && wc <= IW - 2;',
                 'const bool sub = valid && (unsigned)(fy + 1) <= 1u && (unsigned)(fx + 1) <= 1u;',
                 'const bool mid = xw && !sub, slow = valid && !xw;',
                 'if (s.W < BF_TW) return false;'):
        assert line in fused, line
    # ---- the window kernels
    for line in ('constexpr int TH = %d, TW = %d, LH = TH + 2 + 2 * R, LW = TW + 2 + 2 * R,' % (U.TH, U.TW),
                 'const int wy0 = ty0 - 1 - R, wx0 = tx0 - 1 - R;',
                 'const int ly = t.h0 - wy0, lx = t.w0 - wx0;',
                 'const bool inwin = ly >= 0 && ly + 1 < LH && lx >= 0 && lx + 1 < LW;',
                 'dcn_bwd_coord_tile_kernel<6>', 'dcn_bwd_coord_tile_kernel<3>'):
        assert line in dcn, line
    assert U.tile_window(3) == (16, 40) and U.tile_window(6) == (22, 46)
    # ---- the strip kernel
    for line in ('const int x = strip * %d + lane;' % U.STRIP_W,
                 'const bool valid = (ph > -1.f) && (pw > -1.f) && (ph < (float)H) && (pw < (float)W);',
                 'const int fy = h0 - (y - 1 + i), fx = w0 - (x - 1 + j);',
                 'const bool near = (fy == -1 || fy == 0) && (fx == -1 || fx == 0);',
                 'if (strips > 1 && live && (lane < 2 || lane > 61)) {',
                 'if ((tl < 0 || tl > 63) && tx >= 0 && tx < W) {'):
        assert line in dcn, line
    # ---- the tap every other route resolves
    assert 'const bool valid = (h > -1.f) && (w > -1.f) && (h < (float)H) && (w < (float)W);' in tap
    assert 'const bool r0 = valid && h0 >= 0, r1 = valid && h1 <= H - 1;' in tap and 'const bool c0 = w0 >= 0, c1 = w1 <= W - 1;' in tap
    # ---- the names the query returns are the kernels' own
    for name in U.KERNEL_NAMES.values():
        assert '"%s"' % name in dcn and name.split('<')[0] in dcn + fused, name


def test_zero_field_is_a_regular_convolution_on_every_route():
    dg, H, W = 2, 17, 70
    off = np.zeros((1, dg * 18, H, W), np.float32)
    want = dg * sum((H - abs(i)) * (W - abs(j)) for i in (-1, 0, 1) for j in (-1, 0, 1))
    for route, inside in (('fused', 'sub'), ('tile3', 'inwin'), ('tile6', 'inwin'), ('strip', 'near')):
        c = U.census(off, dg, route)
        assert c['valid'] == c[inside] == c['lh=0'] == c['lw=0'] == want, (route, c)
    c = U.census(off, dg, 'strip')
    # regular taps one row / column outside the image sit exactly on the limits:  ti = 0 of row 0 -> h == -1, and so on
    assert c['h==-1'] == dg * sum(W - abs(j) for j in (-1, 0, 1)) and c['h==H'] == c['h==-1']
    assert c['w==-1'] == dg * sum(H - abs(i) for i in (-1, 0, 1)) and c['w==W'] == c['w==-1']
    # the strip crossings of a regular 3 x 3: lane 0 of strip 1 reaches column 63 with tj = 0, lane 63 of strip 0 column 64 with tj = 2
    assert c[('cross', 0)] == c[('cross', 63)] == dg * sum(H - abs(i) for i in (-1, 0, 1)) and c[('cross', 1)] == c[('cross', 62)] == 0


def test_constant_fields_sit_where_the_window_arithmetic_says():
    """wr = r + ti + fy + 2 in [0, 12] (fused), ly = r + ti + fy + R in [0, 8 + 2R] (windows), r = row in the tile, ti = tap row: an
    offset whose floor is fy keeps EVERY lane inside iff -2 <= fy <= 1 (fused), -R <= fy <= R - 1 (windows)."""
    H, W = 24, 96
    all_in = {-6.0: {'tile6': 'inwin'}, -3.0: {'tile3': 'inwin'}, -2.0: {'fused': 'mid'}, -1.0: {'fused': 'sub', 'tile3': 'inwin', 'tile6': 'inwin', 'strip': 'near'},
              0.5: {'fused': 'sub', 'strip': 'near'}, 1.0: {'fused': 'mid', 'strip': 'far'}, 2.0: {'tile3': 'inwin'}, 5.0: {'tile6': 'inwin'}}
    for k, cls in all_in.items():
        off = np.full((1, 18, H, W), k, np.float32)
        for route, inside in cls.items():
            c = U.census(off, 1, route)
            assert c[inside] == c['valid'] > 0, (k, route, c)
    # one step further and exactly the tile's last (first) row and column leave, for the tap furthest that way
    def classes(k, t, route):
        q = U.tap_geometry(np.full((18, H, W), k, np.float32), 0, t)
        return q, U.route_classes(q, route)
    q, r = classes(2.0, 8, 'fused')
    assert r['slow'].any() and (r['slow'] == (q['valid'] & ((q['oy'] % 8 == 7) | (q['ox'] % 32 == 31)))).all()
    q, r = classes(-3.0, 0, 'fused')
    assert r['slow'].any() and (r['slow'] == (q['valid'] & ((q['oy'] % 8 == 0) | (q['ox'] % 32 == 0)))).all()
    for route, R in (('tile3', 3), ('tile6', 6)):
        q, r = classes(float(R), 8, route)
        assert r['outwin'].any() and (r['outwin'] == (q['valid'] & ((q['oy'] % 8 == 7) | (q['ox'] % 32 == 31)))).all()
        q, r = classes(float(-R - 1), 0, route)
        assert r['outwin'].any() and (r['outwin'] == (q['valid'] & ((q['oy'] % 8 == 0) | (q['ox'] % 32 == 0)))).all()


def test_every_route_has_half_a_wave_of_taps_in_each_of_its_edge_classes(capsys):
    """The coverage condition: per route, over the geometries it is tested on and all fields together, at least 32 taps in each of the
    route's classes, on each exact invalid position, in each clipped-corner class and at an offset of exactly -1.0 on either axis."""
    with capsys.disabled():
        for route, (hint, labels) in U.ROUTES.items():
            c = U.route_census(route)
            print('\nDCN backward census, route %s (hint %s), geometries %s, all fields:' % (route, hint, ' '.join(labels)))
            for line in U.census_table(c, route):
                print('  ' + line)
            for k in U.GENERIC_CLASSES + U.ROUTE_CLASSES[route]:
                assert c[k] >= 32, (route, k, c[k])


def test_the_strip_crossings_come_from_the_sub_field():
    """The ladder, border and noise fields hold few sub-pixel taps; the crossing classes of the strip kernel need `sub`."""
    tot = U.new_census('strip')
    for label in U.ROUTES['strip'][1]:
        tot = U.add_census(tot, U.census(U.edge_field(label, 'sub'), U.GEOMS[label][2], 'strip'))
    assert tot['far'] == 0 and tot['near'] == tot['valid']
    for k in U.STRIP_CROSS:
        assert tot[k] >= 32, (k, tot[k])


def test_fields_are_what_their_names_say():
    for label, (B, C, dg, Co, H, W) in U.GEOMS.items():
        for field, frac in (('ladder', 0.25), ('ladder_int', 0.0), ('ladder_half', 0.5)):
            off = U.edge_field(label, field)
            assert ((off - frac) == (off - frac).round()).all() and off.min().item() == -9 + frac and off.max().item() == 9 + frac
        sub = U.edge_field(label, 'sub')
        assert set((sub * 4).unique().tolist()) == set(range(-4, 4))
        assert U.edge_field(label, 'noise16').abs().max().item() <= 60.
        for field in U.FIELDS:
            off = U.edge_field(label, field)
            assert off.shape == (B, dg * 18, H, W) and off.dtype == torch.float32 and off.abs().max().item() <= 80.
        # noise16 is mostly invalid
        c = U.census(U.edge_field(label, 'noise16'), dg, 'device')
        assert c['valid'] < 0.5 * c['taps'], (label, c['valid'], c['taps'])


def test_white_noise_cases_never_put_the_fused_kernel_on_an_exact_position():
    """Why the edge file exists: over the rows of test_gpu_dcn.CASES that the fused kernel takes, no tap sits exactly on a limit of
    the validity rule, and no sub-pixel tap has an offset of exactly -1.0.  Whoever enriches those cases deletes this assertion."""
    import test_gpu_dcn as T
    tot, rows = U.new_census('fused'), 0
    for case, sel in zip(T.CASES, CASES_TABLE):
        if sel[3] != 'F':
            continue
        *dims, kw = case
        off = T._mk(*dims, seed=len(str(case)), **kw)[1]
        tot = U.add_census(tot, U.census(off, dims[10], 'fused'))
        rows += 1
    assert rows == 5 and tot['valid'] > 400000
    assert [tot[k] for k in ('h==-1', 'h==H', 'w==-1', 'w==W', 'sub fy=-1 lh=0', 'sub fx=-1 lw=0')] == [0] * 6, tot


# ------------------------------------------------------------------------------------------------ which kernel runs
# One letter per hint, in the order AUTO, DEVICE, LDS, STRIP, LDS_WIDE:  F dcn_bwd_fused_kernel, S dcn_bwd_dx_strip_kernel (+
# dcn_bwd_coord_kernel<false>), 3 / 6 dcn_bwd_coord_tile_kernel<3> / <6>, D dcn_bwd_coord_kernel (device atomics).
LETTER = {'F': U.KERNEL_NAMES['fused'], 'S': U.KERNEL_NAMES['strip'], '3': U.KERNEL_NAMES['tile3'], '6': U.KERNEL_NAMES['tile6'], 'D': U.KERNEL_NAMES['device']}
HINT_ORDER = ('auto', 'device', 'lds', 'strip', 'lds_wide')
CASES_TABLE = [      # row of test_gpu_dcn.CASES: (B, C, H, W, Co, k, stride, pad, dil, groups, dg)
    '3D3S6',         # (2, 64, 16, 16, 64, 3, 1, 1, 1, 1, 8)       8 channels per group: never fused
    '3D3F6',         # (1, 128, 23, 37, 128, 3, 1, 1, 1, 1, 8)
    '3D3S6',         # (1, 64, 16, 20, 64, ...)
    '3D3S6',         # (1, 64, 12, 12, 64, ...) integer
    '3D3S6',         # (1, 64, 12, 12, 64, ...) half
    '3D3S6',         # (1, 64, 12, 16, 64, ...) sigma 16
    'DDDDD',         # stride 2, groups 2
    'DDDDD',         # dilation 2
    'DDDDD',         # 1x1
    '3D3F6',         # (1, 128, 64, 64, 128, ...) the training layer
    '3D3S6',         # (1, 48, 10, 13, 24, ...) 6 channels per group
    'DDDSD',         # (1, 64, 8, 64, 32, ..., dg 2) 32 channels per group: no LDS window
    '3D3S6',         # (1, 16, 1, 5, 16, ...)
    '3D3S6',         # (1, 32, 12, 150, 32, ...) 4 channels per group
    '3D3S6',         # (1, 16, 6, 128, 16, ...)
    '3D3F6',         # (2, 128, 17, 45, 128, ...)
    '3D3F6',         # (1, 128, 9, 33, 63, ...)
    '3D3S6',         # (1, 128, 12, 12, 64, ...) integer: 16 channels per group but W < 32 -> the staged strip pair
    '3D3S6',         # (1, 128, 12, 12, 64, ...) half: the same
    '3D3S6',         # (1, 128, 12, 16, 64, ...) sigma 16: the same
    '3D3F6',         # (3, 32, 16, 40, 32, ..., dg 2)
]
GEOMS_TABLE = {'F1': '3D3F6', 'F2': '3D3F6', 'S1': '3D3S6', 'S2': '3D3S6'}


def _names(B, C, H, W, Co, k, stride, pad, dil, groups, dg):
    from edvr_amd import ops
    x, w = torch.empty(B, C, H, W, device='meta'), torch.empty(Co, C // groups, k, k, device='meta')  # only the shapes are read
    return [ops.dcnv2_backward_kernel_name(x, w, stride, pad, dil, groups, dg, U.HINTS[h]) for h in HINT_ORDER]


def test_backward_kernel_selection_table(capsys):
    import test_gpu_dcn as T
    from edvr_amd import ops
    assert [U.HINTS[h] for h in HINT_ORDER] == [ops.DCN_SCATTER_AUTO, ops.DCN_SCATTER_DEVICE, ops.DCN_SCATTER_LDS, ops.DCN_SCATTER_STRIP, ops.DCN_SCATTER_LDS_WIDE]
    assert len(CASES_TABLE) == len(T.CASES)
    with capsys.disabled():
        print('\nDCN backward kernel per hint (%s):' % ' '.join(HINT_ORDER))
        for case, want in zip(T.CASES, CASES_TABLE):
            got = _names(*case[:11])
            print('  %-48s %s' % (case[:11], want))
            assert got == [LETTER[c] for c in want], (case, got, want)
        for label, want in GEOMS_TABLE.items():
            B, C, dg, Co, H, W = U.GEOMS[label]
            got = _names(B, C, H, W, Co, 3, 1, 1, 1, 1, dg)
            print('  %-48s %s' % ('%s %s' % (label, U.GEOMS[label]), want))
            assert got == [LETTER[c] for c in want], (label, got, want)
    # what the table states: every 12 x 12 and 12 x 16 row runs the staged pair under STRIP - the three with 16 channels per group that
    # were written for the fused kernel (integer, half, mostly out of bounds) included -, five rows do reach the fused kernel
    narrow = [i for i, c in enumerate(T.CASES) if (c[2], c[3]) in ((12, 12), (12, 16))]
    assert len(narrow) == 6 and all(CASES_TABLE[i][3] == 'S' for i in narrow)
    assert [i for i in narrow if T.CASES[i][1] == 128] == [17, 18, 19]
    assert sum(t[3] == 'F' for t in CASES_TABLE) >= 5
    # the routes of the edge file
    for route, (hint, labels) in U.ROUTES.items():
        for label in labels:
            assert LETTER[GEOMS_TABLE[label][HINT_ORDER.index(hint)]] == U.KERNEL_NAMES[route], (route, label)


def test_query_refuses_bad_shapes_and_needs_no_gpu():
    from edvr_amd import _lib, ops
    x, w = torch.empty(1, 15, 8, 32, device='meta'), torch.empty(16, 15, 3, 3, device='meta')
    with pytest.raises(Exception):
        ops.dcnv2_backward_kernel_name(x, w, 1, 1, 1, 1, 2)  # 15 channels, 2 deformable groups
    import ctypes
    buf = ctypes.create_string_buffer(4)  # a short buffer is filled up to its length, terminated
    assert _lib.lib().edvr_dcnv2_bwd_kernel_name(1, 16, 8, 32, 16, 3, 3, 1, 1, 1, 1, 1, 3, buf, 4) == 0 and buf.value == b'dcn'


# ------------------------------------------------------------------------------------------------ the oracle on these fields
@pytest.mark.parametrize('label', sorted(U.GEOMS))
def test_oracle_in_fp32_takes_the_same_cells_as_in_fp64_on_the_exact_fields(label):
    """The dOffset comparison of the GPU tests excludes NOTHING on the exact fields: every sampling position is exact in float32, so
    the oracle run in float32 never lands in another cell.  On the sigma-16 noise at most 2 elements (the existing cap)."""
    for field in U.FIELDS:
        _, flip = U.oracle_backward(label, field)
        n = int(flip.sum())
        assert n == 0 if field in U.EXACT_FIELDS else n <= 2, (label, field, n)
