"""CPU: the definition of the MPEG-style round trip as tests/mpeg_ref.py restates it - its properties, its frozen fixture -
and the host side of the `lq_mpeg` / `mpeg_qscale` options: what the planners draw, and what is refused."""
import os
import random

import numpy as np
import pytest
import torch

import jpeg_ref
import mpeg_ref
from util_data import SyntheticClient, base_opt
from util_mpeg import inverted_stripes_clip, moving_clip, noise_clip, tie_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mpeg_roundtrip.pt')


def _intra_alone(img, qscale):
    """M1, M3, M7 on one frame, spelt out on jpeg_ref's passes."""
    planes = mpeg_ref.planes(img)
    Q = mpeg_ref.intra_table(qscale)
    rec = []
    for p in planes:
        h, w = p.shape
        b = p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128
        c = jpeg_ref._fdct_pass(b, True)
        c = jpeg_ref._fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)
        c = np.sign(c) * ((np.abs(c) + 4 * Q) // (8 * Q)) * Q
        c = jpeg_ref._idct_pass(jpeg_ref._idct_pass(c.swapaxes(-1, -2), 11).swapaxes(-1, -2), 18)
        rec.append(np.clip(c + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w))
    return mpeg_ref.output(rec, *img.shape[:2])


def test_intra_table():
    q = mpeg_ref.intra_table(1)
    assert q[0, 0] == 8 and q[0, 1] == 1 and q[7, 7] == (83 + 8) >> 4
    q = mpeg_ref.intra_table(31)
    assert q[0, 0] == 8 and q[7, 7] == (83 * 31 + 8) >> 4 == 161 and q.min() == 8
    assert (mpeg_ref.intra_table(16) == np.where(np.arange(64).reshape(8, 8) == 0, 8, mpeg_ref.INTRA_W)).all()


def test_planes_are_those_of_the_jpeg_definition():
    """M1 = J-steps 1 - 3 for '420': padded sizes, the edge repeat, and the chroma rows below the frame repeating chroma row ch - 1."""
    img = noise_clip(1, 1, 20, 4, 1)[0, 0].numpy()
    y, cb, cr = mpeg_ref.planes(img)
    assert y.shape == (32, 16) and cb.shape == cr.shape == (16, 8)
    assert (y[20:] == y[19]).all() and (y[:, 4:] == y[:, 3:4]).all()
    assert (cb[10:] == cb[9]).all() and (cr[10:] == cr[9]).all()
    img = noise_clip(1, 1, 8, 8, 2)[0, 0].numpy()
    cb = mpeg_ref.planes(img)[1]
    assert (cb[4:] == cb[3]).all()


@pytest.mark.parametrize('qscale', [1, 7, 31])
def test_intra_frames_equal_m3_alone(qscale):
    clip = moving_clip(3, 33, 47, (1, -2), 30).numpy()
    out = mpeg_ref.roundtrip_clip(clip, qscale, 12, 7)
    assert np.array_equal(out[0], _intra_alone(clip[0], qscale))
    every = mpeg_ref.roundtrip_clip(clip, qscale, 1, 7)
    for i in range(3):
        assert np.array_equal(every[i], _intra_alone(clip[i], qscale)), i
    assert not np.array_equal(out[1], every[1])


@pytest.mark.parametrize('g', [1, 2, 3])
def test_gop_restart(g):
    clip = moving_clip(7, 50, 70, (2, -3), 31).numpy()
    whole = mpeg_ref.roundtrip_clip(clip, 8, g, 7)
    assert np.array_equal(whole[g:], mpeg_ref.roundtrip_clip(clip[g:], 8, g, 7))
    assert np.array_equal(whole[2 * g:], mpeg_ref.roundtrip_clip(clip[2 * g:], 8, g, 7))
    assert not np.array_equal(whole[1:], mpeg_ref.roundtrip_clip(clip[1:], 8, 0, 7))


@pytest.mark.parametrize('shift', [(2, -3), (-7, 7), (0, 0), (5, 0)])
def test_planted_shift_is_found(shift):
    clip = moving_clip(3, 64, 96, shift, 32).numpy()
    for qscale in (1, 8, 16):
        _, stats = mpeg_ref.roundtrip_clip(clip, qscale, 12, 7, details=True)
        assert stats['vectors'][0] is None
        for mv in stats['vectors'][1:]:
            assert mv.shape == (4, 6, 2) and (mv[1:-1, 1:-1] == shift).all(), (shift, qscale, mv[1:-1, 1:-1])


def test_a_shift_past_the_range_is_not_found():
    clip = moving_clip(2, 64, 96, (0, 4), 33).numpy()
    _, stats = mpeg_ref.roundtrip_clip(clip, 4, 12, 4, details=True)
    assert (stats['vectors'][1][1:-1, 1:-1] == (0, 4)).all()
    _, stats = mpeg_ref.roundtrip_clip(clip, 4, 12, 3, details=True)  # |s| = R + 1
    mv = stats['vectors'][1]
    assert np.abs(mv).max() <= 3 and not (mv[1:-1, 1:-1] == (0, 4)).all(axis=-1).any()


def test_ties_go_to_the_first_candidate_in_raster_order():
    _, stats = mpeg_ref.roundtrip_clip(tie_clip(48, 64).numpy(), 1, 12, 7, details=True)
    mv = stats['vectors'][1]
    assert (mv[1:-1, 1:-1] == (0, -4)).all(), mv


def test_search_zero_is_frame_differencing():
    clip = moving_clip(3, 33, 47, (1, 2), 34).numpy()
    out, stats = mpeg_ref.roundtrip_clip(clip, 6, 0, 0, details=True)
    assert all((mv == 0).all() for mv in stats['vectors'][1:])
    src = [mpeg_ref.planes(f) for f in clip]
    rec = [mpeg_ref.intra_plane(p, 6) for p in src[0]]
    for i in (1, 2):
        rec = [mpeg_ref.inter_plane(p, r, 6) for p, r in zip(src[i], rec)]  # the prediction is the previous reconstruction itself
        assert np.array_equal(out[i], mpeg_ref.output(rec, 33, 47)), i


def test_qscale_zero_copies_and_bad_arguments_raise():
    clip = noise_clip(1, 3, 9, 11, 35)[0].numpy()
    assert np.array_equal(mpeg_ref.roundtrip_clip(clip, 0), clip)
    assert not np.array_equal(mpeg_ref.roundtrip_clip(clip, 1), clip)
    both = mpeg_ref.roundtrip(np.stack([clip, clip]), [0, 5])
    assert np.array_equal(both[0], clip) and np.array_equal(both[1], mpeg_ref.roundtrip_clip(clip, 5))
    for bad in ((32, 12, 7), (-1, 12, 7), (5, -1, 7), (5, 12, 16)):
        with pytest.raises(ValueError):
            mpeg_ref.roundtrip_clip(clip, *bad)


@pytest.mark.parametrize('qscale', [1, 31])
def test_coefficient_bounds(qscale):
    """|c| <= 16320 intra and <= 32640 inter, which is what lets 32 bits and the reciprocal-multiply quantiser hold everything.
    Measured here: the 0 / 255 rows clip, inverted every other frame, gives 7394 intra (|sample - 128| <= 128 caps an intra
    coefficient near 8192, so 16320 is out of an intra block's reach) and, at search 0 where no vector can undo the inversion,
    14788 inter; 16320 = 64 x 255 is the inter DC of a flat frame that inverts, and that is where it is reached."""
    clip = inverted_stripes_clip(4, 32, 32).numpy()
    for search in (0, 2):
        _, stats = mpeg_ref.roundtrip_clip(clip, qscale, 0, search, details=True)
        assert stats['cmax_intra'] <= 16320 and stats['cmax_inter'] <= 32640, stats
    _, stats = mpeg_ref.roundtrip_clip(clip, qscale, 0, 0, details=True)
    assert stats['cmax_intra'] == 7394 and stats['cmax_inter'] > 2 * 7000
    flat = np.stack([np.full((16, 16, 3), v, np.uint8) for v in (0, 255, 0)])
    _, stats = mpeg_ref.roundtrip_clip(flat, qscale, 0, 7, details=True)
    assert stats['cmax_inter'] == 16320 and stats['cmax_intra'] <= 16320


def test_quality_falls_with_the_quantiser_scale():
    """PSNR of every frame, intra and predicted, falls as the quantiser scale rises.  (How the P-frames compare with the I-frame depends
    on the content - the flat inter quantiser is finer than the intra matrix's high frequencies - and is not asserted.)"""
    clip = moving_clip(5, 50, 70, (2, -3), 36).numpy()

    def psnr(a, b):
        return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b) ** 2))
    curves = []
    for qscale in (2, 8, 31):
        out = mpeg_ref.roundtrip_clip(clip, qscale, 0, 7)
        curves.append([psnr(out[i], clip[i]) for i in range(5)])
    assert curves[0][0] > 40 and curves[2][0] < 30
    assert all(a > b + 3 > c + 6 for a, b, c in zip(*curves)), curves


def test_reference_equals_the_frozen_fixture():
    gold = torch.load(GOLDEN)
    assert len(gold['cases']) >= 5 and os.path.getsize(GOLDEN) < 300 * 1024
    assert {'moving_33x47', 'stripes_32x32', 'tie_48x64'} <= {c['name'] for c in gold['cases']}
    for case in gold['cases']:
        got, stats = mpeg_ref.roundtrip_clip(case['input'].numpy(), case['qscale'], case['gop'], case['search'], details=True)
        assert np.array_equal(got, case['output'].numpy()), case['name']
        for i, mv in enumerate(stats['vectors']):
            assert mpeg_ref.is_intra(i, case['gop']) == (mv is None)
            if mv is not None:
                assert np.array_equal(mv, case['vectors'][i].numpy()), (case['name'], i)
        assert stats['nonzero'] == case['nonzero'], case['name']


# ------------------------------------------------------------------------------------------------ planners
@pytest.fixture(scope='module')
def reds_meta(tmp_path_factory):
    p = tmp_path_factory.mktemp('mpeg_meta') / 'meta_info.txt'
    p.write_text(''.join(f'{c:03d} 100 (720,1280,3)\n' for c in (0, 1, 2, 11, 30)))
    return str(p)


@pytest.fixture(scope='module')
def vimeo_meta(tmp_path_factory):
    p = tmp_path_factory.mktemp('mpeg_vmeta') / 'meta_info_Vimeo90K_train_GT.txt'
    p.write_text(''.join(f'{c:05d}/{q:04d} 7 (256,448,3)\n' for c in (1, 2) for q in range(1, 9)))
    return str(p)


def _planner(kind, meta, **kw):
    from edvr_amd import data as D
    client = SyntheticClient((24, 40), 4)
    if kind == 'reds':
        return D.make_planner(base_opt(meta=meta, interval_list=[1, 2], random_reverse=True, **kw), client)
    return D.make_planner(dict(base_opt(meta=meta, random_reverse=True, num_frame=7, **kw), type='Vimeo90KDataset'), client)


def _plans(planner, seed, count=200):
    rng = random.Random(seed)
    if hasattr(planner, 'reset_epoch'):
        planner.reset_epoch()
    return [planner.plan(i % len(planner), rng) for i in range(count)]


@pytest.mark.parametrize('kind', ['reds', 'vimeo'])
def test_planner_invariance(kind, reds_meta, vimeo_meta):
    """200 plans from one stream: with and without lq_mpeg they differ in mpeg_qscale alone - the JPEG quality and the blur and noise
    drawn beside it included; the scales lie in [lo, hi], vary, and repeat under the same seed."""
    meta = reds_meta if kind == 'reds' else vimeo_meta
    others = dict(lq_jpeg={'quality': [20, 80]}, lq_degrade={'blur': {}, 'noise': {}})
    plain, mpeg = _planner(kind, meta, **others), _planner(kind, meta, lq_mpeg={'qscale': [2, 20]}, **others)
    assert plain.lq_mpeg is None and mpeg.lq_mpeg == (2, 20, 7, 1.0)
    a, b = _plans(plain, 3), _plans(mpeg, 3)
    for pa, pb in zip(a, b):
        assert (pa.key, pa.clip, pa.center, pa.frames, pa.top, pa.left, pa.flags, pa.jpeg_quality) == \
            (pb.key, pb.clip, pb.center, pb.frames, pb.top, pb.left, pb.flags, pb.jpeg_quality)
        assert repr(pa.degrade) == repr(pb.degrade) and pa.degrade is not None
        assert pa.mpeg_qscale == 0 and 2 <= pb.mpeg_qscale <= 20
    q = [p.mpeg_qscale for p in b]
    assert len(set(q)) > 10
    assert q == [p.mpeg_qscale for p in _plans(mpeg, 3)] and q != [p.mpeg_qscale for p in _plans(mpeg, 4)]
    assert q != [p.jpeg_quality % 19 + 2 for p in b]  # (a stream of its own, not the JPEG fork's)
    assert 'mpeg' in repr(b[0]) and 'mpeg' not in repr(a[0])
    alone = _plans(_planner(kind, meta, lq_mpeg={'qscale': [2, 20]}), 3)
    assert q == [p.mpeg_qscale for p in alone] and {p.jpeg_quality for p in alone} == {0}


def test_planner_prob(reds_meta):
    never = _planner('reds', reds_meta, lq_mpeg={'qscale': [2, 20], 'prob': 0})
    assert {p.mpeg_qscale for p in _plans(never, 1)} == {0}
    half = [p.mpeg_qscale for p in _plans(_planner('reds', reds_meta, lq_mpeg={'qscale': 9, 'search': 3, 'prob': 0.5}), 1)]
    assert set(half) == {0, 9} and 60 <= half.count(9) <= 140  # 200 fair coins: 100 +- 5.7 sigma


def test_qscale_draws_spelt_out():
    from edvr_amd.data import _draw_mpeg_qscale
    rng = random.Random(11)
    rng.random()
    state = rng.getstate()
    r = random.Random('lq_mpeg' + repr(state))
    assert _draw_mpeg_qscale((2, 20, 7, 1.0), rng) == r.randint(2, 20)
    r = random.Random('lq_mpeg' + repr(state))
    assert _draw_mpeg_qscale((1, 31, 7, 0.5), rng) == (r.randint(1, 31) if r.random() < 0.5 else 0)
    assert _draw_mpeg_qscale(None, rng) == 0 and rng.getstate() == state


def test_option_errors(reds_meta):
    from edvr_amd import data as D
    for bad in ({'qscale': 32}, {'qscale': 0}, {'qscale': [20, 2]}, {'qscale': [2, 9, 20]}, {'qscale': 5, 'search': 16}, {'qscale': 5, 'search': -1},
                {'qscale': 5, 'prob': 1.5}, {'qscale': 5.0}, {'qscale': True}, {'search': 7}, {'qscale': 5, 'gop': 12}, {'qscale': 5, 'search': 2.0}):
        with pytest.raises(ValueError):
            D.training_lq_mpeg({'lq_mpeg': bad})
        with pytest.raises(ValueError):
            _planner('reds', reds_meta, lq_mpeg=bad)
    assert D.training_lq_mpeg({}) is None and D.training_lq_mpeg({'lq_mpeg': None}) is None
    assert D.training_lq_mpeg({'lq_mpeg': {'qscale': 4, 'search': 0, 'prob': 0.25}}) == (4, 4, 0, 0.25)


def test_lq_from_gt_refusals_come_before_any_launch():
    from edvr_amd import data as D
    gt = torch.zeros(2, 3, 16, 16)
    for degradation in ('bi', 'bd'):
        with pytest.raises(ValueError, match='quantize'):
            D.lq_from_gt(gt, 4, False, degradation, mpeg_qscale=5)
    with pytest.raises(ValueError, match='32'):
        D.lq_from_gt(gt, 4, None, 'bi', mpeg_qscale=32)
    with pytest.raises(ValueError, match='mpeg_gop'):
        D.lq_from_gt(gt, 4, None, 'bi', mpeg_qscale=5, mpeg_gop=-2)
    with pytest.raises(ValueError, match='mpeg_search'):
        D.lq_from_gt(gt, 4, None, 'bi', mpeg_qscale=5, mpeg_search=16)
    with pytest.raises(NotImplementedError):  # nothing refused: the CPU tensor reaches the operator
        D.lq_from_gt(gt, 4, None, 'bi', mpeg_qscale=5)


def test_video_test_clips_options(tmp_path):
    from edvr_amd import data as D
    from util_data import video_test_opt, write_video_test_tree
    write_video_test_tree(str(tmp_path), dict(folders=['000'], frames=2, lq_hw=(8, 8), scale=4))
    opt = dict(video_test_opt(str(tmp_path), dict(cache_data=True, num_frame=5, padding='reflection')), dataroot_lq=None)
    ds = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'degradation': 'bd', 'mpeg_qscale': 6, 'mpeg_gop': 4}), device='cpu')
    assert ds.lq_from_gt['quantize'] is True and ds._lq_mpeg == {'mpeg_qscale': 6, 'mpeg_gop': 4, 'mpeg_search': 7}
    assert D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4}), device='cpu')._lq_mpeg == {}
    for bad in ({'scale': 4, 'quantize': False, 'mpeg_qscale': 6}, {'scale': 4, 'mpeg_qscale': 0}, {'scale': 4, 'mpeg_qscale': 6, 'mpeg_search': 16},
                {'scale': 4, 'mpeg_qscale': 6, 'mpeg_gop': -1}):
        with pytest.raises(ValueError):
            D.VideoTestClips(dict(opt, lq_from_gt=bad), device='cpu')
    with pytest.raises(ValueError, match='cache_data'):  # a window read on its own is not the clip in order
        D.VideoTestClips(dict(opt, cache_data=False, lq_from_gt={'scale': 4, 'mpeg_qscale': 6}), device='cpu')


def test_ops_refusals_without_a_gpu():
    from edvr_amd import ops
    frames = torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        ops.mpeg_roundtrip(frames, 5)
    assert ops.mpeg_qscale(np.int64(7)) == 7 and ops.mpeg_qscale(0, allow_zero=True) == 0 and ops.mpeg_gop(0) == 0 and ops.mpeg_search(15) == 15
    for bad in (0, 32, -1, 5.0, '5', True, None):
        with pytest.raises(ValueError):
            ops.mpeg_qscale(bad)


def test_gop_pieces():
    """Where scripts/make_lq.py cuts a clip: at multiples of the GOP, so that each piece starts on an intra frame."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_lq', os.path.join(ROOT, 'scripts', 'make_lq.py'))
    make_lq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make_lq)
    assert make_lq.gop_pieces(10, 4, 3) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert make_lq.gop_pieces(10, 4, 4) == [(0, 4), (4, 8), (8, 10)]
    assert make_lq.gop_pieces(10, 5, 3) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert make_lq.gop_pieces(10, 4, None) == [(0, 4), (4, 8), (8, 10)]
    assert make_lq.gop_pieces(10, 3, 0) == [(0, 10)] and make_lq.gop_pieces(10, 10, 0) == [(0, 10)]
