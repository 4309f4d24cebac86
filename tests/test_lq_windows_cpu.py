"""CPU: the host side of training from GT frames alone - the window geometry (edvr_amd.data.lq_window) against the float64 restatements of
both degradations, the planners with and without an LQ tree, the refusals, and the argument matrix of scripts/train_reds.py."""
import importlib.util
import os
import random

import numpy as np
import pytest

import util_bd
import util_imresize
from util_data import SyntheticClient, base_opt

SCALES = (2, 3, 4)
SIZES = (8, 16, 64)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _axis_matrix(n, scale, degradation):
    m = util_imresize.axis_matrix(n, 1 / scale) if degradation == 'bi' else util_bd.axis_matrix(n, scale)
    return m.numpy()


def _lengths(size, scale, degradation):
    """LQ lengths of frames to try: the shortest the geometry admits, a few just above it, and larger ones, odd and even."""
    from edvr_amd import data as D
    lo = max(size, -(-D.lq_window_extent(size, scale, degradation) // scale))
    return [lo, lo + 1, lo + 2, lo + 5, 2 * lo + 3, 180]


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('size', SIZES)
def test_window_holds_every_tap_of_non_zero_weight(degradation, scale, size):
    """Every valid start of every frame length: the non-zero columns of rows [start, start + size) of the independent float64 axis
    matrix lie inside [lo, hi), [lo, hi) is no longer than the fixed extent, and the window placed by lq_window_origin holds it
    inside the frame."""
    from edvr_amd import data as D
    extent = D.lq_window_extent(size, scale, degradation)
    for n_lq in _lengths(size, scale, degradation):
        n = n_lq * scale
        m = _axis_matrix(n, scale, degradation)
        assert m.shape == (n_lq, n)
        nz = m != 0
        first, last = nz.argmax(1), n - 1 - nz[:, ::-1].argmax(1)
        for start in range(n_lq - size + 1):
            lo, hi, e = D.lq_window(start, size, n_lq, scale, degradation)
            assert e == extent and 0 <= lo < hi <= n and hi - lo <= extent
            assert lo <= first[start:start + size].min() and last[start:start + size].max() < hi, (n_lq, start)
            o = D.lq_window_origin(lo, n, extent)
            assert 0 <= o <= lo and hi <= o + extent <= n


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
@pytest.mark.parametrize('scale', SCALES)
def test_frame_length_need_not_be_a_multiple_of_the_scale(degradation, scale):
    """A GT length that is not a multiple of the scale is mod-cropped first: the geometry of n_lq = length // scale."""
    from edvr_amd import data as D
    for length in (97, 98, 99, 101):
        n_lq = length // scale
        m = _axis_matrix(n_lq * scale, scale, degradation)
        for start in (0, 1, n_lq // 2, n_lq - 8):
            lo, hi, _ = D.lq_window(start, 8, n_lq, scale, degradation)
            cols = np.flatnonzero((m[start:start + 8] != 0).any(0))
            assert lo <= cols.min() and cols.max() < hi


def test_extent_is_the_span_of_the_taps_and_inverts():
    from edvr_amd import data as D
    assert [D.lq_window_extent(1, s, 'bd') for s in SCALES] == [7, 11, 13]  # the kernel's non-zero taps
    assert [D.lq_window_extent(1, s, 'bi') for s in SCALES] == [8, 11, 16]  # 4 s samples strictly inside the support (one fewer when it ends on samples)
    for degradation in D.DEGRADATIONS:
        for s in SCALES:
            for size in (1, 2, 8, 64):
                e = D.lq_window_extent(size, s, degradation)
                assert e == D.lq_window_extent(1, s, degradation) + (size - 1) * s
                assert D.lq_window_size(e, s, degradation) == size
                assert D.lq_window_pitch(e) % 16 == 0 and 0 <= D.lq_window_pitch(e) - 3 * e < 16
            with pytest.raises(ValueError):
                D.lq_window_size(D.lq_window_extent(4, s, degradation) + 1, s, degradation)


def test_geometry_refusals():
    from edvr_amd import data as D
    with pytest.raises(ValueError, match='scale'):
        D.lq_window(0, 8, 64, 8, 'bd')
    with pytest.raises(ValueError, match='scale'):
        D.lq_window(0, 8, 64, 8, 'bi')
    with pytest.raises(ValueError, match='scale'):
        D.lq_window(0, 8, 64, 1, 'bi')
    with pytest.raises(ValueError, match='degradation'):
        D.lq_window(0, 8, 64, 4, 'blur')
    with pytest.raises(ValueError, match='empty'):
        D.lq_window(0, 0, 64, 4, 'bi')
    with pytest.raises(ValueError, match='leave'):
        D.lq_window(57, 8, 64, 4, 'bi')
    with pytest.raises(ValueError, match='leave'):
        D.lq_window(-1, 8, 64, 4, 'bd')
    for degradation in D.DEGRADATIONS:  # a frame shorter than the window: 8 LQ samples read 4 * 7 + 16 (13) GT samples
        short = (D.lq_window_extent(8, 4, degradation) - 1) // 4
        with pytest.raises(ValueError, match='fewer'):
            D.lq_window(0, 8, short, 4, degradation)
        D.lq_window(0, 8, short + 1, 4, degradation)


def _gt_only(opt, degradation='bi', **spec):
    return dict(opt, dataroot_lq=None, lq_from_gt=dict(scale=opt['scale'], degradation=degradation, **spec))


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_reds_planner_draws_the_same_plans_without_an_lq_tree(tmp_path, degradation):
    from edvr_amd import data as D
    meta = tmp_path / 'meta.txt'
    meta.write_text('000 100 (720,1280,3)\n001 100 (720,1280,3)\n002 100 (720,1280,3)\n')
    opt = base_opt(meta=str(meta), interval_list=[1, 2, 3], random_reverse=True)
    client = SyntheticClient((30, 41), 4)
    tree, gt_only = D.REDSClipPlanner(opt, client), D.REDSClipPlanner(_gt_only(opt, degradation), client)
    assert tree.lq_from_gt is None and gt_only.lq_from_gt == (4, degradation) and len(tree) == len(gt_only)
    ra, rb = random.Random(5), random.Random(5)
    for k in range(300):
        a, b = tree.plan(k % len(tree), ra), gt_only.plan(k % len(tree), rb)
        assert repr(a) == repr(b) and (a.key, a.clip, a.center, a.frames, a.top, a.left, a.flags) == (b.key, b.clip, b.center, b.frames, b.top, b.left, b.flags)
    assert ra.getstate() == rb.getstate()


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_vimeo_planner_draws_the_same_plans_without_an_lq_tree(tmp_path, degradation):
    from edvr_amd import data as D
    meta = tmp_path / 'meta.txt'
    meta.write_text(''.join(f'0000{c}/000{q} 7 (256,448,3)\n' for c in (1, 2) for q in (1, 2, 3)))
    opt = base_opt(meta=str(meta), type='Vimeo90KDataset', random_reverse=True)
    client = SyntheticClient((16, 28), 4)
    tree, gt_only = D.make_planner(opt, client), D.make_planner(_gt_only(opt, degradation), client)
    assert isinstance(gt_only, D.Vimeo90KClipPlanner) and gt_only.lq_from_gt == (4, degradation)
    ra, rb = random.Random(9), random.Random(9)
    for k in range(300):
        a, b = tree.plan(k % len(tree), ra), gt_only.plan(k % len(tree), rb)
        assert (a.key, a.clip, a.center, a.frames, a.top, a.left, a.flags) == (b.key, b.clip, b.center, b.frames, b.top, b.left, b.flags)
    assert ra.getstate() == rb.getstate()


def test_planner_mod_crops_the_gt_size(tmp_path):
    """A GT frame that is not a multiple of the scale: the LQ size is the mod-cropped size divided by the scale."""
    from edvr_amd import data as D

    class Odd(SyntheticClient):
        def size(self, kind, clip, frame):
            assert kind == 'gt', 'no LQ tree is read'
            return 123, 166

    meta = tmp_path / 'meta.txt'
    meta.write_text('001 100 (123,166,3)\n')
    planner = D.REDSClipPlanner(_gt_only(base_opt(meta=str(meta))), Odd((30, 41), 4))
    assert planner.clip_shapes('001', '00000000') == ((30, 41), (120, 164))


def test_load_stages_windows_a_table_and_the_centre_gt_crop(tmp_path):
    """load() without an LQ tree: per frame the window of the decoded GT frame at the origin the geometry gives, its table record, and
    the centre frame's GT crop as with an LQ tree."""
    from edvr_amd import data as D
    meta = tmp_path / 'meta.txt'
    meta.write_text('001 100 (120,164,3)\n')
    opt = base_opt(meta=str(meta))
    client = SyntheticClient((30, 41), 4)
    tree, gt_only = D.REDSClipPlanner(opt, client), D.REDSClipPlanner(_gt_only(opt, 'bd'), client)
    rng = random.Random(1)
    e = D.lq_window_extent(8, 4, 'bd')
    for k in range(6):
        plan = gt_only.plan(k, rng)
        (win, tab), gt = gt_only.load(plan)
        assert win.shape == (5, e, D.lq_window_pitch(e)) and win.dtype == np.uint8 and tab.shape == (5, D.LQ_WINDOW_RECORD_INTS) and tab.dtype == np.int32
        assert np.array_equal(gt, tree.load(plan)[1])
        for i, f in enumerate(plan.frames):
            frame = D.decode_image(client.get('gt', plan.clip, f'{f:08d}'))
            y0, x0, H, W, top, left = tab[i, :6]
            assert (H, W, top, left) == (120, 164, plan.top, plan.left)
            assert y0 == D.lq_window_origin(D.lq_window(plan.top, 8, 30, 4, 'bd')[0], 120, e)
            assert x0 == D.lq_window_origin(D.lq_window(plan.left, 8, 41, 4, 'bd')[0], 164, e)
            assert np.array_equal(win[i, :, :3 * e].reshape(e, e, 3), frame[y0:y0 + e, x0:x0 + e])


def test_option_refusals(tmp_path):
    from edvr_amd import data as D
    meta = tmp_path / 'meta.txt'
    meta.write_text('001 100 (120,164,3)\n')
    opt = base_opt(meta=str(meta))
    client = SyntheticClient((30, 41), 4)
    with pytest.raises(ValueError, match="dataset's scale"):  # scale mismatch
        D.REDSClipPlanner(dict(opt, dataroot_lq=None, lq_from_gt=dict(scale=2)), client)
    with pytest.raises(ValueError, match='degradation'):
        D.REDSClipPlanner(dict(opt, dataroot_lq=None, lq_from_gt=dict(scale=4, degradation='blur')), client)
    with pytest.raises(ValueError, match='scale 8'):  # BD has no x8
        D.REDSClipPlanner(dict(opt, scale=8, dataroot_lq=None, lq_from_gt=dict(scale=8, degradation='bd')), client)
    with pytest.raises(ValueError, match='scale 8'):
        D.Vimeo90KClipPlanner(dict(opt, scale=8, dataroot_lq=None, lq_from_gt=dict(scale=8, degradation='bi')), client)
    with pytest.raises(ValueError, match='quantised'):
        D.REDSClipPlanner(dict(opt, dataroot_lq=None, lq_from_gt=dict(scale=4, quantize=False)), client)
    with pytest.raises(ValueError, match='dataroot_lq is None'):
        D.REDSClipPlanner(dict(opt, dataroot_lq=None), client)
    with pytest.raises(ValueError, match='empty'):  # a gt_size below the scale: no LQ sample to make
        D.REDSClipPlanner(dict(opt, gt_size=2, dataroot_lq=None, lq_from_gt=dict(scale=4)), client)
    # a frame smaller than the window its crop reads: 8 LQ samples at x4 read 44 (BI) / 41 (BD) GT samples
    small = D.REDSClipPlanner(_gt_only(opt), SyntheticClient((10, 41), 4))
    with pytest.raises(ValueError, match='smaller than the window'):
        small.plan(0, random.Random(0))
    D.REDSClipPlanner(opt, SyntheticClient((10, 41), 4)).plan(0, random.Random(0))  # with an LQ tree that frame is fine
    # with an LQ tree the key is not looked at
    assert D.REDSClipPlanner(dict(opt, lq_from_gt=dict(scale=2, degradation='blur')), client).lq_from_gt is None


def test_ops_refuse_cpu_tensors():
    import torch
    from edvr_amd import data as D, ops
    e = D.lq_window_extent(8, 4, 'bi')
    with pytest.raises(NotImplementedError):
        ops.lq_crops_from_windows(torch.zeros(1, e, D.lq_window_pitch(e), dtype=torch.uint8), torch.zeros(1, 8, dtype=torch.int32), 4, 'bi')


BASE = ['--gt', 'gt', '--meta', 'meta.txt']


@pytest.mark.parametrize('argv,lq,lq_from_gt,degradation', [
    (['--lq', 'lq'], 'lq', None, 'bi'),
    (['--lq-from-gt', '4'], None, 4, 'bi'),
    (['--lq-from-gt', '4', '--degradation', 'bd'], None, 4, 'bd'),
    (['--lq-from-gt', '4', '--degradation', 'bi', '--val-gt', 'vgt'], None, 4, 'bi'),
    (['--lq', 'lq', '--val-gt', 'vgt', '--val-lq', 'vlq'], 'lq', None, 'bi'),
])
def test_train_reds_accepts(argv, lq, lq_from_gt, degradation):
    args = _load('train_reds').parse_args(BASE + argv)
    assert (args.lq, args.lq_from_gt, args.degradation) == (lq, lq_from_gt, degradation)


@pytest.mark.parametrize('argv', [
    [],                                           # neither --lq nor --lq-from-gt
    ['--lq', 'lq', '--lq-from-gt', '4'],          # both
    ['--lq', 'lq', '--degradation', 'bd'],        # bd without --lq-from-gt
    ['--lq-from-gt', '2'],                        # not the network's scale
    ['--lq-from-gt', '4', '--degradation', 'gaussian'],
    ['--lq', 'lq', '--val-gt', 'vgt'],            # --val-lq may be omitted only with --lq-from-gt
])
def test_train_reds_rejects(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _load('train_reds').parse_args(BASE + argv)
    assert e.value.code == 2
    capsys.readouterr()
