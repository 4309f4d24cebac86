"""CPU: the definition of the JPEG round trip as tests/jpeg_ref.py restates it, against PIL's libjpeg - the committed fixture
and a live round trip - and the host side of the `lq_jpeg` / `jpeg_quality` options: what the planners draw, and what is refused."""
import io
import os
import random

import numpy as np
import pytest
import torch

import jpeg_ref
from util_data import SyntheticClient, base_opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_roundtrip.pt')


def golden_cases():
    """[(name, input (H, W, 3) uint8 array, quality, subsampling, PIL's output array)] of the fixture."""
    gold = torch.load(GOLDEN)
    return [(c['name'], c['input'].numpy(), q, s, o.numpy()) for c in gold['cases'] for q, s, o in c['outputs']]


def test_fixture_holds_what_the_issue_lists():
    cases = golden_cases()
    shapes = {c[1].shape[:2] for c in cases}
    assert {(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (37, 53), (64, 64)} <= shapes
    assert any(h > 128 and w > 128 for h, w in shapes)  # a chroma ring crosses a seam of the kernel's 64 x 64 tiles on both axes
    assert {c[2] for c in cases} == {1, 10, 50, 75, 95, 100} and {c[3] for c in cases} == {'420', '444'}
    names = {c[0].split('_')[0] for c in cases}
    assert {'noise', 'grey', 'zeros', 'ones', 'magenta'} <= names
    assert os.path.getsize(GOLDEN) < 300 * 1024


def test_reference_equals_the_fixture_byte_for_byte():
    cases = golden_cases()
    assert len(cases) > 80
    for name, img, q, s, want in cases:
        got = jpeg_ref.roundtrip(img, q, s)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, q, s, int(np.abs(got.astype(int) - want).max()))


def test_reference_equals_a_live_pil_round_trip():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(5)
    for (h, w), q, s in (((45, 70), 35, '420'), ((26, 19), 85, '444')):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format='JPEG', quality=q, subsampling={'444': 0, '420': 2}[s])
        buf.seek(0)
        assert np.array_equal(jpeg_ref.roundtrip(img, q, s), np.asarray(Image.open(buf).convert('RGB'))), (h, w, q, s)


def test_reference_quality_zero_is_a_copy_and_bad_arguments_raise():
    img = np.random.default_rng(0).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    assert np.array_equal(jpeg_ref.roundtrip(img, 0), img)
    assert not np.array_equal(jpeg_ref.roundtrip(img, 100), img)
    with pytest.raises(ValueError):
        jpeg_ref.roundtrip(img, 101)
    with pytest.raises(ValueError):
        jpeg_ref.roundtrip(img, 50, '422')


# ------------------------------------------------------------------------------------------------ planners
@pytest.fixture(scope='module')
def reds_meta(tmp_path_factory):
    p = tmp_path_factory.mktemp('jpeg_meta') / 'meta_info.txt'
    p.write_text(''.join(f'{c:03d} 100 (720,1280,3)\n' for c in (0, 1, 2, 11, 30)))
    return str(p)


@pytest.fixture(scope='module')
def vimeo_meta(tmp_path_factory):
    p = tmp_path_factory.mktemp('jpeg_vmeta') / 'meta_info_Vimeo90K_train_GT.txt'
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
def test_planner_draws_the_quality_last(kind, reds_meta, vimeo_meta):
    """200 plans from one stream: with and without lq_jpeg they have identical key, frames, crop and flags - the quality is drawn after
    the reference's draws, from a fork that leaves the stream where they left it; the qualities lie in [lo, hi], vary, and repeat
    under the same seed."""
    meta = reds_meta if kind == 'reds' else vimeo_meta
    plain, jpeg = _planner(kind, meta), _planner(kind, meta, lq_jpeg={'quality': [20, 80]})
    assert plain.lq_jpeg is None and jpeg.lq_jpeg == (20, 80, '420', 1.0)
    a, b = _plans(plain, 3), _plans(jpeg, 3)
    assert len({(p.top, p.left, p.flags) for p in a}) > 20
    for pa, pb in zip(a, b):
        assert (pa.key, pa.clip, pa.center, pa.frames, pa.top, pa.left, pa.flags) == (pb.key, pb.clip, pb.center, pb.frames, pb.top, pb.left, pb.flags)
        assert pa.jpeg_quality == 0 and 20 <= pb.jpeg_quality <= 80
    q = [p.jpeg_quality for p in b]
    assert len(set(q)) > 10
    assert q == [p.jpeg_quality for p in _plans(jpeg, 3)]
    assert q != [p.jpeg_quality for p in _plans(jpeg, 4)]
    assert 'jpeg' in repr(b[0]) and 'jpeg' not in repr(a[0])


@pytest.mark.parametrize('kind', ['reds', 'vimeo'])
def test_planner_prob(kind, reds_meta, vimeo_meta):
    meta = reds_meta if kind == 'reds' else vimeo_meta
    never = _planner(kind, meta, lq_jpeg={'quality': [20, 80], 'prob': 0})
    assert {p.jpeg_quality for p in _plans(never, 1)} == {0}
    half = [p.jpeg_quality for p in _plans(_planner(kind, meta, lq_jpeg={'quality': 55, 'subsampling': '444', 'prob': 0.5}), 1)]
    assert set(half) == {0, 55} and 60 <= half.count(55) <= 140  # 200 fair coins: 100 +- 5.7 sigma


def test_quality_draws_spelt_out():
    """[r.random() < prob where prob < 1], then r.randint(lo, hi), on a fork r of the stream's state; the stream itself does not move."""
    from edvr_amd.data import _draw_jpeg_quality
    rng = random.Random(11)
    rng.random()
    state = rng.getstate()
    r = random.Random(repr(state))
    assert _draw_jpeg_quality((20, 80, '420', 1.0), rng) == r.randint(20, 80)
    r = random.Random(repr(state))
    assert _draw_jpeg_quality((1, 100, '420', 0.5), rng) == (r.randint(1, 100) if r.random() < 0.5 else 0)
    assert _draw_jpeg_quality(None, rng) == 0 and rng.getstate() == state
    assert _draw_jpeg_quality((30, 30, '444', 1.0), random) == 30  # the `random` module is a stream too


def test_option_errors(reds_meta):
    from edvr_amd import data as D
    for bad in ({'quality': 101}, {'quality': 0}, {'quality': [80, 20]}, {'quality': [20, 50, 80]}, {'quality': 50, 'subsampling': '422'},
                {'quality': 50, 'prob': 1.5}, {'quality': 50.0}, {'quality': True}, {'subsampling': '420'}, {'quality': 50, 'qualty': 3}):
        with pytest.raises(ValueError):
            D.training_lq_jpeg({'lq_jpeg': bad})
        with pytest.raises(ValueError):
            _planner('reds', reds_meta, lq_jpeg=bad)
    assert D.training_lq_jpeg({}) is None and D.training_lq_jpeg({'lq_jpeg': None}) is None
    assert D.training_lq_jpeg({'lq_jpeg': {'quality': 40, 'subsampling': '444', 'prob': 0.25}}) == (40, 40, '444', 0.25)


def test_lq_from_gt_refusals_come_before_any_launch():
    """Checked on the host, on a CPU tensor: the ValueError is raised before the operator is reached (which would refuse the CPU tensor)."""
    from edvr_amd import data as D
    gt = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match='quantize'):
        D.lq_from_gt(gt, 4, False, 'bi', jpeg_quality=40)
    with pytest.raises(ValueError, match='quantize'):
        D.lq_from_gt(gt, 4, False, 'bd', jpeg_quality=40)
    with pytest.raises(ValueError, match='101'):
        D.lq_from_gt(gt, 4, None, 'bi', jpeg_quality=101)
    with pytest.raises(ValueError, match='subsampling'):
        D.lq_from_gt(gt, 4, None, 'bi', jpeg_quality=40, jpeg_subsampling='422')
    with pytest.raises(NotImplementedError):  # nothing refused: the CPU tensor reaches the operator
        D.lq_from_gt(gt, 4, None, 'bi', jpeg_quality=40)


def test_video_test_clips_options(tmp_path):
    from edvr_amd import data as D
    from util_data import video_test_opt, write_video_test_tree
    write_video_test_tree(str(tmp_path), dict(folders=['000'], frames=2, lq_hw=(8, 8), scale=4))
    opt = dict(video_test_opt(str(tmp_path), dict(cache_data=False, num_frame=5, padding='reflection')), dataroot_lq=None)
    ds = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'degradation': 'bd', 'jpeg_quality': 40}), device='cpu')
    assert ds.lq_from_gt['quantize'] is True and ds._lq_jpeg == {'jpeg_quality': 40, 'jpeg_subsampling': '420'}
    assert D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4}), device='cpu')._lq_jpeg == {}
    for bad in ({'scale': 4, 'quantize': False, 'jpeg_quality': 40}, {'scale': 4, 'jpeg_quality': 0}, {'scale': 4, 'jpeg_quality': 40, 'jpeg_subsampling': '411'}):
        with pytest.raises(ValueError):
            D.VideoTestClips(dict(opt, lq_from_gt=bad), device='cpu')


def test_ops_refusals_without_a_gpu():
    from edvr_amd import ops
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        ops.jpeg_roundtrip(frames, 50)
    assert ops.jpeg_quality(np.int64(7)) == 7 and ops.jpeg_quality(0, allow_zero=True) == 0
    for bad in (0, 101, -1, 50.0, '50', True, None):
        with pytest.raises(ValueError):
            ops.jpeg_quality(bad)
