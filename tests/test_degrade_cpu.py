"""CPU: the definition of the blur and noise degradations as tests/degrade_ref.py restates it - Philox4x32-10 against
Random123's known answers, the Q20 kernels, the integer blur against a real-valued filter, the moments of the normals - and the host side
of the `lq_degrade` / `degrade` options: what the planners draw, and what is refused."""
import math
import random

import numpy as np
import pytest
import torch

import degrade_ref
from util_data import SyntheticClient, base_opt


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize('counter, key, words', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, words):
    assert tuple(int(w) for w in degrade_ref.philox4x32_10(counter, key)) == words


def test_philox_words_layout():
    w = degrade_ref.philox_words((7 << 32) | 5, 3, 4, 6)
    assert w.shape == (4, 6, 4) and w.dtype == np.uint32
    assert tuple(int(v) for v in w[2, 5]) == tuple(int(v) for v in degrade_ref.philox4x32_10((5, 2, 3, 0), (5, 7)))  # counter (x, y, ctr_t, 0)


def test_moments_of_z():
    """256 x 256 x 3 normals of key 0x0123456789abcdef, frame 0: mean and variance within 4 standard errors of 0 and 1 (1 / sqrt(N) and
    sqrt(2 / N), N = 196608).  The field is deterministic; its moments are recorded here."""
    z = degrade_ref.normals64(degrade_ref.philox_words(0x0123456789abcdef, 0, 256, 256))
    n = z.size
    mean, var = float(z.mean()), float(z.var())
    print('mean', repr(mean), 'var', repr(var))
    assert n == 196608 and abs(mean) < 4 / math.sqrt(n) and abs(var - 1) < 4 * math.sqrt(2 / n)
    assert abs(mean - MEAN_Z) < 1e-9 and abs(var - VAR_Z) < 1e-9
    g = degrade_ref.normals64(degrade_ref.philox_words(0x0123456789abcdef, 0, 8, 8), gray=True)
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 0], g[..., 2]) and np.array_equal(g[..., 0], z[:8, :8, 0])
    z32 = degrade_ref.normals32(degrade_ref.philox_words(0x0123456789abcdef, 0, 256, 256))
    assert z32.dtype == np.float32 and float(np.abs(z32 - z).max()) < 1e-4  # (u near 1 loses its last bit in float32: rho 2.4e-4 -> 0)


MEAN_Z, VAR_Z = 0.0007306069196191166, 0.9941541402701866  # recorded values of the field above (0.32 and 1.83 standard errors)


# ------------------------------------------------------------------------------------------------ kernels and the integer blur
def test_kernels_sum_to_one_and_are_symmetric():
    from edvr_amd.data import gaussian_blur_kernel
    for ksize, sx, sy, theta in ((3, 0.2, None, 0.0), (7, 1.3, None, 0.0), (21, 3.0, None, 0.0), (21, 0.2, None, 0.0), (11, 2.5, 0.7, 0.6), (21, 3.0, 0.4, -2.0),
                                 (5, 50.0, 50.0, 1.0)):
        k = gaussian_blur_kernel(ksize, sx, sy, theta)
        assert k.dtype == np.int32 and k.shape == (ksize, ksize) and int(k.sum(dtype=np.int64)) == 1 << 20 and k.min() >= 0
        assert k[ksize // 2, ksize // 2] == k.max()
        assert np.array_equal(k, k[::-1, ::-1])  # d -> -d
        if sy is None or sy == sx:
            assert np.array_equal(k, k.T) and np.array_equal(k, k[::-1]) and np.array_equal(k, k[:, ::-1])
            assert np.array_equal(k, gaussian_blur_kernel(ksize, sx, sx, 1.234))  # theta turns a circle into itself
        else:
            assert not np.array_equal(k, k.T)
            assert np.array_equal(k, gaussian_blur_kernel(ksize, sx, sy, theta + math.pi))
            assert np.array_equal(k.T, gaussian_blur_kernel(ksize, sy, sx, -theta))  # swapping the axes: x <-> y
    wide = gaussian_blur_kernel(9, 3.0, 0.5, 0.0)  # sigma_x lies along x: the row through the centre is the heavy one
    assert wide[4].sum() > 4 * wide[:, 4].sum() / 3
    for bad in ((4, 1.0), (1, 1.0), (23, 1.0), (7.0, 1.0), (True, 1.0), (7, 0.0), (7, -1.0), (7, float('nan')), (7, 1.0, float('inf')), (7, 1.0, 1.0, float('nan'))):
        with pytest.raises(ValueError):
            gaussian_blur_kernel(*bad)


def _real_kernel(ksize, sx, sy, theta):
    """The real-valued weights, written out independently of data.gaussian_blur_kernel: exp(-d' S^-1 d / 2), S = R diag(sx^2, sy^2) R'."""
    r = ksize // 2
    rot = np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])
    inv = np.linalg.inv(rot @ np.diag([sx * sx, sy * sy]) @ rot.T)
    w = np.empty((ksize, ksize))
    for a in range(ksize):
        for b in range(ksize):
            d = np.array([b - r, a - r], np.float64)  # (x, y)
            w[a, b] = math.exp(-0.5 * d @ inv @ d)
    return w / w.sum()


@pytest.mark.parametrize('ksize, sx, sy, theta, hw', [(21, 3.0, 3.0, 0.0, (30, 41)), (21, 2.9, 0.6, 0.8, (11, 13)), (7, 0.9, 2.0, -1.1, (9, 20)), (3, 0.2, 0.2, 0.0, (2, 2))])
def test_integer_blur_is_the_real_filter(ksize, sx, sy, theta, hw):
    """The Q20 blur and its rounding stay within ksize^2 255 2^-21 levels of float64 F.conv2d over the reflect-padded image: each weight
    is off by at most 2^-21 (the centre tap by the residue besides, which the others' errors bound), each sample is at most 255."""
    import torch.nn.functional as F
    from edvr_amd.data import gaussian_blur_kernel
    img = np.random.default_rng(ksize).integers(0, 256, hw + (3,), dtype=np.uint8)
    acc = degrade_ref.blur_acc(img, gaussian_blur_kernel(ksize, sx, sy, theta))
    x = torch.from_numpy(img).double().permute(2, 0, 1)[:, None]
    r = ksize // 2
    want = F.conv2d(F.pad(x, (r, r, r, r), mode='reflect'), torch.from_numpy(_real_kernel(ksize, sx, sy, theta))[None, None])[:, 0].permute(1, 2, 0).numpy()
    bound = ksize ** 2 * 255 * 2.0 ** -21
    err = float(np.abs(acc / 2.0 ** 20 - want).max())
    print('blur error', err, 'bound', bound)
    assert err <= bound
    out = degrade_ref.degrade(img, gaussian_blur_kernel(ksize, sx, sy, theta))
    assert out.dtype == np.uint8 and float(np.abs(out - want).max()) <= 0.5 + bound


def test_reference_pass_through_and_noise_bookkeeping():
    img = np.random.default_rng(1).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    assert np.array_equal(degrade_ref.degrade(img), img)
    assert np.array_equal(degrade_ref.degrade(img, None, (0.0, 0.0, True), key=5), img)
    a, b = degrade_ref.degrade(img, None, (10.0, 0.0, False), key=5, ctr_t=0), degrade_ref.degrade(img, None, (10.0, 0.0, False), key=5, ctr_t=1)
    assert not np.array_equal(a, b) and not np.array_equal(a, img)
    assert np.array_equal(a, degrade_ref.degrade(img, None, (10.0, 0.0, False), key=5, ctr_t=0))
    t64 = degrade_ref.noisy_t(degrade_ref.blur_acc(img, None), 10.0, 1.0, False, 5, 0)
    t32 = degrade_ref.noisy_t(degrade_ref.blur_acc(img, None), 10.0, 1.0, False, 5, 0, np.float32)
    assert t32.dtype == np.float32 and float(np.abs(t32 - t64).max()) < 1e-3


# ------------------------------------------------------------------------------------------------ planners
@pytest.fixture(scope='module')
def reds_meta(tmp_path_factory):
    p = tmp_path_factory.mktemp('degrade_meta') / 'meta_info.txt'
    p.write_text(''.join(f'{c:03d} 100 (720,1280,3)\n' for c in (0, 1, 2, 11, 30)))
    return str(p)


@pytest.fixture(scope='module')
def vimeo_meta(tmp_path_factory):
    p = tmp_path_factory.mktemp('degrade_vmeta') / 'meta_info_Vimeo90K_train_GT.txt'
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


def _fields(p):
    return p.key, p.clip, p.center, p.frames, p.top, p.left, p.flags, p.jpeg_quality


@pytest.mark.parametrize('kind', ['reds', 'vimeo'])
def test_planner_leaves_every_other_decision_alone(kind, reds_meta, vimeo_meta):
    """200 plans from one stream: with lq_degrade every other field of every plan - the JPEG quality included when both keys are set - is
    what it is without it; the draws lie in their ranges, vary, and repeat under the same seed."""
    from edvr_amd import data as D
    meta = reds_meta if kind == 'reds' else vimeo_meta
    block = {'blur': {}, 'noise': {}}
    plain, deg = _planner(kind, meta), _planner(kind, meta, lq_degrade=block)
    jpeg, both = _planner(kind, meta, lq_jpeg={'quality': [20, 80]}), _planner(kind, meta, lq_jpeg={'quality': [20, 80]}, lq_degrade=block)
    assert plain.lq_degrade is None and deg.lq_degrade == D.training_lq_degrade({'lq_degrade': D.LQ_DEGRADE_DEFAULTS})
    a, b, c, d = _plans(plain, 3), _plans(deg, 3), _plans(jpeg, 3), _plans(both, 3)
    assert len({(p.top, p.left, p.flags) for p in a}) > 20 and len({p.jpeg_quality for p in c}) > 10
    for pa, pb, pc, pd in zip(a, b, c, d):
        assert _fields(pa) == _fields(pb) and _fields(pc) == _fields(pd)
        assert pa.degrade is None and pc.degrade is None
        assert pb.degrade['blur'] == pd.degrade['blur'] and pb.degrade['noise'] == pd.degrade['noise'] and pb.degrade['key'] == pd.degrade['key']
        ksize, sx, sy, theta = pb.degrade['blur']
        assert ksize % 2 == 1 and 7 <= ksize <= 21 and 0.2 <= sx <= 3.0 and 0.2 <= sy <= 3.0 and -math.pi <= theta < math.pi
        assert (sx == sy and theta == 0.0) or sx != sy
        kernel = pb.degrade['kernel']  # ONE kernel per clip: all its frames share it
        assert kernel.shape == (ksize, ksize) and np.array_equal(kernel, D.gaussian_blur_kernel(ksize, sx, sy, theta))
        sigma, shot, gray = pb.degrade['noise']
        assert (shot == 0.0 and 1 <= sigma <= 30) or (sigma == 0.0 and 0.0025 <= shot <= 9.0)
        assert isinstance(gray, bool) and 0 <= pb.degrade['key'] < 1 << 64
    iso = sum(p.degrade['blur'][1] == p.degrade['blur'][2] for p in b)
    shots = sum(p.degrade['noise'][1] > 0 for p in b)
    grays = sum(p.degrade['noise'][2] for p in b)
    assert 110 <= iso <= 170 and 70 <= shots <= 130 and 50 <= grays <= 110  # 200 draws at 0.7, 0.5, 0.4: +- 4.6 sigma
    assert len({p.degrade['blur'][0] for p in b}) == 8 and len({p.degrade['key'] for p in b}) == 200
    again = _plans(deg, 3)
    assert [(p.degrade['blur'], p.degrade['noise'], p.degrade['key']) for p in again] == [(p.degrade['blur'], p.degrade['noise'], p.degrade['key']) for p in b]
    assert [p.degrade['key'] for p in _plans(deg, 4)] != [p.degrade['key'] for p in b]
    assert 'blur' in repr(b[0]) and 'noise' in repr(b[0]) and 'blur' not in repr(a[0])


@pytest.mark.parametrize('kind', ['reds', 'vimeo'])
def test_planner_prob(kind, reds_meta, vimeo_meta):
    meta = reds_meta if kind == 'reds' else vimeo_meta
    never = _planner(kind, meta, lq_degrade={'blur': {'prob': 0}, 'noise': {'prob': 0.0}})
    assert {p.degrade for p in _plans(never, 1)} == {None}
    assert {p.degrade for p in _plans(_planner(kind, meta, lq_degrade={'noise': {'prob': 0}}), 1)} == {None}
    half = _plans(_planner(kind, meta, lq_degrade={'blur': {'ksize': 9, 'sigma': 1.5, 'iso_prob': 1, 'prob': 0.5}}), 1)
    on = [p.degrade for p in half if p.degrade is not None]
    assert 60 <= len(on) <= 140 and all(d['blur'] == (9, 1.5, 1.5, 0.0) and d['noise'] is None for d in on)  # 200 fair coins: 100 +- 5.7 sigma
    only_noise = _plans(_planner(kind, meta, lq_degrade={'noise': {'shot_prob': 1, 'gray_prob': 1}}), 1)
    assert all(p.degrade['blur'] is None and p.degrade['kernel'] is None and p.degrade['noise'][0] == 0.0 and p.degrade['noise'][2] for p in only_noise)


def test_draws_spelt_out():
    """The fork: random.Random('lq_degrade' + repr(state)); the stream itself does not move."""
    from edvr_amd import data as D
    spec = D.training_lq_degrade({'lq_degrade': {'blur': {'iso_prob': 0.0}, 'noise': {'shot_prob': 0.0, 'prob': 0.5}}})
    rng = random.Random(11)
    rng.random()
    state = rng.getstate()
    got = D._draw_degrade(spec, rng)
    assert rng.getstate() == state and D._draw_degrade(None, rng) is None
    r = random.Random('lq_degrade' + repr(state))
    ksize = r.choice([7, 9, 11, 13, 15, 17, 19, 21])
    sx = r.uniform(0.2, 3.0)
    assert not r.random() < 0.0
    sy, theta = r.uniform(0.2, 3.0), r.uniform(-math.pi, math.pi)
    noise = None
    if r.random() < 0.5:
        assert not r.random() < 0.0
        noise = (r.uniform(1.0, 30.0), 0.0, r.random() < 0.4)
    assert got['blur'] == (ksize, sx, sy, theta) and got['noise'] == noise and got['key'] == r.getrandbits(64)
    assert D._draw_degrade(spec, random) is not None  # the `random` module is a stream too


def test_option_errors(reds_meta):
    from edvr_amd import data as D
    for bad in ({}, {'blurr': {}}, {'blur': {'size': 7}}, {'blur': {'ksize': [21, 7]}}, {'blur': {'ksize': [8, 8]}}, {'blur': {'ksize': [22, 30]}},
                {'blur': {'ksize': 7.5}}, {'blur': {'sigma': [3.0, 0.2]}}, {'blur': {'sigma': 0}}, {'blur': {'sigma': [0.2, float('inf')]}},
                {'blur': {'iso_prob': 1.5}}, {'blur': {'prob': -0.1}}, {'blur': {'prob': True}}, {'noise': {'sigma': [30, 1]}}, {'noise': {'sigma': -1}},
                {'noise': {'shot': [0.0, 9.0]}}, {'noise': {'shot': [9.0, 0.0025]}}, {'noise': {'shot': [1, 2, 3]}}, {'noise': {'shot_prob': 2}},
                {'noise': {'gray_prob': '0.4'}}, {'noise': {'gray': True}}, {'blur': {}, 'noise': {'prob': float('nan')}}):
        with pytest.raises(ValueError):
            D.training_lq_degrade({'lq_degrade': bad})
        with pytest.raises(ValueError):
            _planner('reds', reds_meta, lq_degrade=bad)
    assert D.training_lq_degrade({}) is None and D.training_lq_degrade({'lq_degrade': None}) is None
    one = D.training_lq_degrade({'lq_degrade': {'blur': {'ksize': [4, 10], 'sigma': 2}}})
    assert one['noise'] is None and one['blur']['ksize'] == [5, 7, 9] and one['blur']['sigma'] == (2.0, 2.0) and one['blur']['iso_prob'] == 0.7


def test_lq_from_gt_refusals_come_before_any_launch():
    """Checked on the host, on a CPU tensor: the ValueError is raised before the operator is reached (which would refuse the CPU tensor)."""
    from edvr_amd import data as D
    gt = torch.zeros(1, 3, 64, 64)
    noise = {'noise': {'sigma': 5}}
    for degradation in ('bi', 'bd'):
        with pytest.raises(ValueError, match='quantize'):
            D.lq_from_gt(gt, 4, False, degradation, degrade=noise)
    for bad in ({}, {'blur': {'ksize': 4, 'sigma_x': 1}}, {'blur': {'ksize': 5}}, {'blur': {'sigma_x': 0}}, {'noise': {'sigma': -1}}, {'noise': {'shot': float('nan')}},
                {'noise': {'sigma': 1e39}}, {'noise': {'sgima': 1}}, {'blurs': {}}):
        with pytest.raises(ValueError):
            D.lq_from_gt(gt, 4, None, 'bi', degrade=bad)
    with pytest.raises(NotImplementedError):  # nothing refused: the CPU tensor reaches the operator
        D.lq_from_gt(gt, 4, None, 'bi', degrade=noise)
    kernel, setting = D.degrade_spec({'blur': {'sigma_x': 1.2}, 'noise': {'shot': 0.5, 'gray': True}})
    assert kernel.shape == (9, 9) and setting == (0.0, 0.5, True)  # 3 sigma each side
    assert D.degrade_spec({'blur': {'sigma_x': 9, 'sigma_y': 1}})[0].shape == (21, 21) and D.degrade_spec({'blur': {'sigma_x': 0.2}})[0].shape == (3, 3)


def test_video_test_clips_options(tmp_path):
    from edvr_amd import data as D
    from util_data import video_test_opt, write_video_test_tree
    write_video_test_tree(str(tmp_path), dict(folders=['000'], frames=2, lq_hw=(8, 8), scale=4))
    opt = dict(video_test_opt(str(tmp_path), dict(cache_data=False, num_frame=5, padding='reflection')), dataroot_lq=None)
    spec = {'blur': {'sigma_x': 1.0}, 'noise': {'sigma': 5}}
    ds = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'degradation': 'bd', 'degrade': spec, 'degrade_seed': 9}), device='cpu')
    assert ds.lq_from_gt['quantize'] is True and ds._lq_degrade == {'degrade': spec, 'seed': 9}
    assert D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4}), device='cpu')._lq_degrade == {}
    for bad in ({'scale': 4, 'quantize': False, 'degrade': spec}, {'scale': 4, 'degrade': {}}, {'scale': 4, 'degrade': {'noise': {'sigma': -2}}}):
        with pytest.raises(ValueError):
            D.VideoTestClips(dict(opt, lq_from_gt=bad), device='cpu')


def test_ops_refusals_without_a_gpu():
    from edvr_amd import ops
    from edvr_amd.data import gaussian_blur_kernel
    frames = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        ops.degrade(frames, noise=(1.0, 0.0, False))
    k = gaussian_blur_kernel(7, 1.0)
    table, weights = ops.degrade_table(3, 16, 16, [k, None, k], [(2.0, 0.0, False), None, (0.0, 0.5, True)], seed=[1, 2, (1 << 64) - 1], frame_index=[5, 6, 7])
    assert table.dtype == np.int32 and table.shape == (3, 8) and weights.dtype == np.int32 and weights.shape == (49,)  # a shared kernel is stored once
    assert table[:, 0].tolist() == [7, 0, 7] and table[:, 1].tolist() == [0, 0, 0] and table[:, 4].tolist() == [0, 0, 1] and table[:, 7].tolist() == [5, 6, 7]
    assert table[:, 2].view(np.float32).tolist() == [2.0, 0.0, 0.0] and table[:, 3].view(np.float32).tolist() == [0.0, 0.0, 0.5]
    assert table[:, 5].tolist() == [1, 2, -1] and table[:, 6].tolist() == [0, 0, -1]
    assert ops.degrade_table(2, 4, 4)[1] is None and not ops.degrade_table(2, 4, 4)[0][:, :7].any()
    assert ops.degrade_table(1, 4, 4, noise=(-0.0, 0.0, False))[0][0, 2] == 0  # +0.0 as bits: no noise
    ops.check_degrade_table(table, 49, 16, 16, weights)
    even, short, neg = np.zeros((4, 4), np.int32), k.copy(), k.copy()
    even[0, 0] = short[0, 0] = 1 << 20
    neg[0, 0], neg[3, 3] = -1, neg[3, 3] + neg[0, 0] + 1
    assert int(neg.sum()) == 1 << 20
    big = np.zeros((23, 23), np.int32)
    big[11, 11] = 1 << 20
    for bad in (dict(blur=even), dict(blur=big), dict(blur=short), dict(blur=neg), dict(blur=k.astype(np.int64)), dict(blur=k.astype(np.float32)), dict(blur=k[:5]),
                dict(blur=[k, k]), dict(blur=gaussian_blur_kernel(21, 2.0)), dict(noise=(-1.0, 0.0, False)), dict(noise=(0.0, float('nan'), False)),
                dict(noise=(float('inf'), 0.0, False)), dict(noise=(1.0, 0.0)), dict(noise=[(1.0, 0.0, False)]), dict(seed=[1, 2]), dict(seed=1.5),
                dict(seed=1 << 64), dict(frame_index=[0, 1]), dict(frame_index=[0, 1, -1])):
        with pytest.raises(ValueError):
            ops.degrade_table(3, 10, 12, **bad)  # (10 rows are not more than the radius of a 21 x 21 kernel)
    for col, value in ((0, 4), (0, 23), (1, 1), (1, -1), (2, -1), (3, 0x7fc00000), (2, 0x7f800000)):
        t = table.copy()
        t[0, col] = value
        with pytest.raises(ValueError):
            ops.check_degrade_table(t, 49, 16, 16, weights)
    with pytest.raises(ValueError):
        ops.check_degrade_table(table, 49, 3, 16, weights)
    with pytest.raises(ValueError):
        ops.check_degrade_table(table, 49, 16, 16, weights + 1)
    for bad in ((1 << 64, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2)):
        with pytest.raises(ValueError):
            ops.philox_words(*bad)
