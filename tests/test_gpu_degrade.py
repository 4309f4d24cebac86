"""GPU: ops.degrade and ops.philox_words (csrc/degrade.hip) against the NumPy restatement tests/degrade_ref.py - the generator
and the blur with torch.equal, the noise byte for byte except where float32 cannot tell which side of a half-integer a sample lies on -
and everything that calls them: lq_from_gt, VideoTestClips, scripts/make_lq.py, the training loader's `lq_degrade` option and
scripts/train_reds.py --lq-degrade."""
import functools
import math
import os
import shutil

import numpy as np
import pytest
import torch

import degrade_ref
from test_gpu_jpeg import _batches, _frames, _load_script, _meta, _plans, _read_tree, _unaugment
from util_data import write_png_dataset, write_video_test_tree, write_vimeo_train_tree

pytestmark = pytest.mark.gpu

KEY = 0x9e3779b97f4a7c15


def _tile():
    from edvr_amd import _lib
    return _lib.DEGRADE_TILE


@functools.lru_cache(maxsize=None)
def _kernel(ksize, sx, sy=None, theta=0.0):
    from edvr_amd.data import gaussian_blur_kernel
    return gaussian_blur_kernel(ksize, sx, sy, theta)


def _ref(frames, kernels=None, noises=None, key=KEY, frame_index=None):
    """The float64 definition, image by image; kernels / noises: one for all or a list."""
    x = frames.cpu().numpy()
    n = x.shape[0]
    kernels = kernels if isinstance(kernels, list) else [kernels] * n
    noises = noises if isinstance(noises, list) else [noises] * n
    frame_index = range(n) if frame_index is None else frame_index
    return torch.from_numpy(np.stack([degrade_ref.degrade(x[i], kernels[i], noises[i], key, frame_index[i]) for i in range(n)]))


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize('h, w', [(1, 1), (5, 7), (65, 130)])
def test_philox_words(gpu, h, w):
    from edvr_amd import ops
    for key, t in ((0, 0), (KEY, 3), ((1 << 64) - 1, (1 << 32) - 1)):
        got = ops.philox_words(key, t, h, w, device=gpu)
        assert got.dtype == torch.int32 and got.shape == (h, w, 4)
        assert torch.equal(got.cpu(), torch.from_numpy(degrade_ref.philox_words(key, t, h, w).view(np.int32))), (key, t)


# ------------------------------------------------------------------------------------------------ blur alone: exact
def _blur_cases():
    T = _tile()
    aniso = _kernel(21, 3.0, 0.7, 0.6)
    return {'ring wider than half the image': ((3, 11, 13), _kernel(21, 2.5)),
            'one tile': ((2, T, T), _kernel(7, 1.2)),
            'a pixel and three past the tile': ((1, T + 1, T + 3), _kernel(13, 2.0, 1.0, -0.4)),
            'per-image kernels': ((3, T + 6, 2 * T + 2), [None, _kernel(3, 0.6), aniso])}


@pytest.mark.parametrize('case', ['ring wider than half the image', 'one tile', 'a pixel and three past the tile', 'per-image kernels'])
def test_blur_equals_the_reference(gpu, case):
    from edvr_amd import ops
    (n, h, w), kernels = _blur_cases()[case]
    x = _frames(n, h, w, 11)
    got = ops.degrade(x.to(gpu), blur=kernels)
    assert got.dtype == torch.uint8 and got.shape == x.shape
    want = _ref(x, kernels)
    assert torch.equal(got.cpu(), want), int((got.cpu().int() - want.int()).abs().max())
    assert not torch.equal(want, x)
    if isinstance(kernels, list):  # an image's result is its own: each equals its single-image call, and ksize 0 without noise is a copy
        assert torch.equal(got[0].cpu(), x[0])
        for i in range(n):
            assert torch.equal(got[i], ops.degrade(x[i:i + 1].to(gpu), blur=kernels[i])[0]), i


@pytest.mark.parametrize('gap, offset', [(18, 3), (16, 4)])  # image strides and bases that are not / are multiples of 4: byte and dword accesses
def test_image_strided_slices(gpu, gap, offset):
    from edvr_amd import ops
    n, h, w = 3, 40, 52
    x = _frames(n, h, w, 2)
    k = _kernel(9, 1.5, 0.8, 1.0)
    frame = 3 * h * w
    pitch, shape = frame + gap, (n, h, w, 3)
    src = torch.zeros((n + 1) * pitch, dtype=torch.uint8, device=gpu)
    view = src.as_strided(shape, (pitch, 3 * w, 3, 1), pitch - offset)
    view.copy_(x.to(gpu))
    assert view.stride(0) == pitch and torch.equal(view.cpu(), x)
    want = _ref(x, k)
    assert torch.equal(ops.degrade(view, blur=k).cpu(), want)
    dst = torch.full(((n + 1) * pitch,), 7, dtype=torch.uint8, device=gpu)
    out = dst.as_strided(shape, (pitch, 3 * w, 3, 1), offset)
    assert ops.degrade(view, blur=k, out=out) is out
    assert torch.equal(out.cpu(), want)
    written = torch.zeros_like(dst, dtype=torch.bool)
    written.as_strided(shape, (pitch, 3 * w, 3, 1), offset).fill_(True)
    assert bool((dst[~written] == 7).all()) and int((~written).sum()) == (n + 1) * pitch - n * frame  # bytes between the images are left alone
    longer = _frames(5, h, w, 3).to(gpu)
    assert torch.equal(ops.degrade(longer[1:4], blur=k), ops.degrade(longer, blur=k)[1:4])


def test_pass_through(gpu):
    from edvr_amd import ops
    x = _frames(2, 70, 67, 4).to(gpu)
    assert torch.equal(ops.degrade(x), x)
    assert torch.equal(ops.degrade(x, noise=(0.0, 0.0, True), seed=5), x)
    mixed = ops.degrade(x, noise=[None, (3.0, 0.0, False)])
    assert torch.equal(mixed[0], x[0]) and not torch.equal(mixed[1], x[1])
    # a device table nobody checked: the kernel reads any other ksize as 0
    table, _ = ops.degrade_table(2, 70, 67)
    table[:, 0] = (22, 4)
    assert torch.equal(ops.degrade(x, table=torch.from_numpy(table).to(gpu)), x)


# ------------------------------------------------------------------------------------------------ noise
NOISES = {'read': (10.0, 0.0, False), 'shot': (0.0, 1.0, False), 'gray': (6.0, 0.25, True)}


@pytest.mark.parametrize('blur', [False, True])
@pytest.mark.parametrize('setting', ['read', 'shot', 'gray'])
def test_noise_equals_the_float64_definition(gpu, setting, blur):
    """Every byte is clamp(floor(t64 + 0.5)) of the float64 restatement, except where t64 lies within delta of a half-integer: there
    either neighbour passes.  delta = 8 x the largest |t32 - t64| of the NumPy float32 restatement on these inputs - measured on the
    CPU: the largest |t32 - t64| is 3.3e-5 (read), 2.7e-5 (shot) and 1.9e-5 (gray) levels over the two images, without and with blur, so
    delta lies between 1.1e-4 and 2.6e-4 and at most 0.07 % of an image's samples are excused (the NumPy float32 restatement itself
    rounds 1 of the 156 780 samples to the other neighbour); the margin covers the device's logf, sinf and cosf differing from NumPy's by
    a few ulp.  The conditions delta <= 1e-2 and excused <= 2 % hold with room."""
    from edvr_amd import ops
    T = _tile()
    x = _frames(2, T + 1, T + 3, 21)
    kernel = _kernel(9, 2.0, 0.9, 0.5) if blur else None
    read, shot, gray = NOISES[setting]
    got = ops.degrade(x.to(gpu), blur=kernel, noise=NOISES[setting], seed=KEY).cpu().numpy()
    for i in range(2):
        acc = degrade_ref.blur_acc(x[i].numpy(), kernel)
        t64 = degrade_ref.noisy_t(acc, read, shot, gray, KEY, i)
        t32 = degrade_ref.noisy_t(acc, read, shot, gray, KEY, i, np.float32)
        delta = 8 * float(np.abs(t32.astype(np.float64) - t64).max())
        lo, hi = degrade_ref.round_levels(t64 - delta), degrade_ref.round_levels(t64 + delta)
        excused = float((lo != hi).mean())
        wrong = int(((got[i] < lo) | (got[i] > hi)).sum())
        differ = int((got[i] != degrade_ref.round_levels(t64)).sum())
        print(f'{setting} blur {blur} image {i}: delta {delta:.3g}, excused {excused:.3%}, differing from round(t64) {differ}, wrong {wrong}')
        assert delta <= 1e-2 and excused <= 0.02
        assert wrong == 0
        assert not np.array_equal(got[i], x[i].numpy())
    if not blur:  # (the unblurred inputs reach both ends: the clamp is exercised)
        assert int((got == 0).sum()) > 100 and int((got == 255).sum()) > 100


def test_gray_noise_is_one_draw_per_pixel(gpu):
    from edvr_amd import ops
    x = torch.full((1, 33, 70, 3), 150, dtype=torch.uint8)
    x[..., 1], x[..., 2] = 180, 220
    out = ops.degrade(x.to(gpu), noise=(3.0, 0.0, True), seed=KEY).cpu().int()
    d = out - x.int()
    assert int(out.min()) > 128 and int(out.max()) < 255 and int(d.abs().max()) > 6  # no channel clamps, and every t stays in [128, 256)
    # read noise alone: s is the same for the three channels, and v + s z is rounded on one float32 grid there, of which the three v are
    # even points - the channels differ by their offsets exactly
    assert torch.equal(d[..., 0], d[..., 1]) and torch.equal(d[..., 0], d[..., 2])
    colour = ops.degrade(x.to(gpu), noise=(3.0, 0.0, False), seed=KEY).cpu().int() - x.int()
    assert torch.equal(colour[..., 0], d[..., 0]) and not torch.equal(colour[..., 0], colour[..., 1]) and not torch.equal(colour[..., 0], colour[..., 2])


def test_noise_depends_on_the_record_not_on_the_batch_position(gpu):
    from edvr_amd import ops
    T = _tile()
    one = _frames(1, T + 5, T + 9, 31)
    x = torch.cat([one, _frames(1, T + 5, T + 9, 32), one]).to(gpu)
    k = _kernel(5, 1.0)
    out = ops.degrade(x, blur=[k, None, k], noise=(4.0, 0.5, False), seed=[KEY, 1, KEY], frame_index=[7, 7, 7])
    assert torch.equal(out[0], out[2]) and not torch.equal(out[0], out[1])
    other = ops.degrade(x, blur=[k, None, k], noise=(4.0, 0.5, False), seed=[KEY, 1, KEY], frame_index=[7, 7, 8])
    assert torch.equal(other[0], out[0]) and not torch.equal(other[2], out[2])  # another ctr_t: another field
    assert not torch.equal(ops.degrade(x[:1], blur=k, noise=(4.0, 0.5, False), seed=KEY + 1, frame_index=[7]), out[:1])
    assert torch.equal(ops.degrade(x[:1], blur=k, noise=(4.0, 0.5, False), seed=KEY, frame_index=[7]), out[:1])
    # the default frame indices are range(n)
    assert torch.equal(ops.degrade(x, noise=(4.0, 0.0, False), seed=3), ops.degrade(x, noise=(4.0, 0.0, False), seed=3, frame_index=[0, 1, 2]))


# ------------------------------------------------------------------------------------------------ the launch
def test_refusals(gpu):
    from edvr_amd import ops
    x = _frames(2, 16, 16, 4).to(gpu)
    k = _kernel(7, 1.0)
    with pytest.raises(NotImplementedError):
        ops.degrade(x.cpu(), blur=k)
    with pytest.raises(NotImplementedError):
        ops.degrade(x, blur=k, out=torch.empty(2, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='overlaps'):
        ops.degrade(x, blur=k, out=x)
    buf = torch.zeros(3, 16, 16, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match='overlaps'):
        ops.degrade(buf[:2], blur=k, out=buf[1:])
    table, weights = (torch.from_numpy(a).to(gpu) for a in ops.degrade_table(2, 16, 16, k))
    for bad in (dict(blur=_kernel(21, 2.0)[:, :20]), dict(blur=k.astype(np.int64)), dict(blur=[k]), dict(noise=(-1.0, 0.0, False)), dict(noise=(0.0, math.inf, False)),
                dict(table=table, blur=k), dict(table=table[:1], weights=weights), dict(table=table.long(), weights=weights), dict(weights=weights),
                dict(table=table, weights=weights.float()), dict(out=torch.empty(2, 16, 16, 3, dtype=torch.float32, device=gpu))):
        with pytest.raises(ValueError):
            ops.degrade(x, **bad)
    with pytest.raises(ValueError):
        ops.degrade(x.float())
    with pytest.raises(ValueError):
        ops.degrade(x[..., :2])
    with pytest.raises(ValueError, match='radius'):
        ops.degrade(x[:, :10], blur=_kernel(21, 2.0))  # 10 rows, radius 10: one reflection does not cover the ring
    host = table.cpu()
    host[1, 1] = 1  # 49 weights from offset 1 leave the buffer
    with pytest.raises(ValueError):
        ops.degrade(x, table=table, weights=weights, table_host=host)


def test_launch_is_booked_with_algorithmic_bytes(gpu):
    from edvr_amd import ops
    seen = []

    def hook(name, flops, launch, nbytes, executed):
        seen.append((name, flops, nbytes))
        launch()

    x = _frames(3, 33, 47, 5).to(gpu)
    k = _kernel(7, 1.0)
    prev, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, hook
    try:
        ops.degrade(x, blur=k, noise=(2.0, 0.0, False))
        ops.degrade(x, noise=(2.0, 0.0, False))
        ops.philox_words(1, 2, 5, 6, device=gpu)
    finally:
        ops.LAUNCH_HOOK = prev
    px = 3 * 33 * 47
    assert seen == [('degrade', 0.0, 6.0 * px + 32 * 3 + 4 * 49), ('degrade', 0.0, 6.0 * px + 32 * 3), ('philox_words', 0.0, 16.0 * 30)]


def test_graph_replay_equals_eager(gpu):
    """The table form captured once and replayed on new pixels, records and weights in the same buffers: the bytes of the eager call."""
    from edvr_amd import ops
    a, b = _frames(3, 70, 66, 6), _frames(3, 70, 66, 7)
    ka, kb = _kernel(7, 1.0), _kernel(7, 2.0, 0.5, 0.3)
    args_a = dict(blur=[ka, None, ka], noise=[(5.0, 0.0, False), (0.0, 0.5, True), None], seed=3)
    args_b = dict(blur=[kb, kb, None], noise=[None, (2.0, 0.1, False), (9.0, 0.0, True)], seed=4)
    (ta, wa), (tb, wb) = ops.degrade_table(3, 70, 66, **args_a), ops.degrade_table(3, 70, 66, **args_b)
    assert wa.shape == wb.shape == (49,)
    x, table, weights = a.to(gpu), torch.from_numpy(ta).to(gpu), torch.from_numpy(wa).to(gpu)
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(stream):
        ops.degrade(x, table=table, weights=weights)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = ops.degrade(x, table=table, weights=weights, table_host=ta, weights_host=wa)
    x.copy_(b), table.copy_(torch.from_numpy(tb)), weights.copy_(torch.from_numpy(wb))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.degrade(b.to(gpu), **args_b))
    assert not torch.equal(out, ops.degrade(a.to(gpu), **args_a))


# ------------------------------------------------------------------------------------------------ pipeline
SPEC = {'blur': {'ksize': 7, 'sigma_x': 1.4, 'sigma_y': 0.8, 'theta': 0.5}, 'noise': {'sigma': 4.0, 'shot': 0.2, 'gray': False}}


def _spec_args():
    return dict(blur=_kernel(7, 1.4, 0.8, 0.5), noise=(4.0, 0.2, False))


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_lq_from_gt(gpu, degradation):
    from edvr_amd import data as D, ops
    gt = ops.frames_u8_to_f32(_frames(3, 64, 96, 8).to(gpu)[None])[0]
    plain = D.lq_from_gt(gt, 4, True, degradation)
    lq_bytes = (plain * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(ops.frames_u8_to_f32(lq_bytes[None])[0], plain)  # (the bytes the quantised LQ frames are made of)
    degraded = ops.degrade(lq_bytes, seed=9, **_spec_args())  # frame i of the call: frame index i
    want = ops.frames_u8_to_f32(degraded[None])[0]
    assert torch.equal(D.lq_from_gt(gt, 4, None, degradation, degrade=SPEC, seed=9), want)  # 'bd': the key implies quantize
    assert torch.equal(D.lq_from_gt(gt, 4, True, degradation, degrade=SPEC, seed=9), want)
    assert not torch.equal(want, plain) and not torch.equal(D.lq_from_gt(gt, 4, None, degradation, degrade=SPEC, seed=10), want)
    then_jpeg = ops.frames_u8_to_f32(ops.jpeg_roundtrip(degraded, 40)[None])[0]  # blur, noise, then compression
    assert torch.equal(D.lq_from_gt(gt, 4, None, degradation, jpeg_quality=40, degrade=SPEC, seed=9), then_jpeg)
    only_blur = D.lq_from_gt(gt, 4, None, degradation, degrade={'blur': SPEC['blur']})
    assert torch.equal(only_blur, ops.frames_u8_to_f32(ops.degrade(lq_bytes, blur=_spec_args()['blur'])[None])[0])
    with pytest.raises(ValueError):
        D.lq_from_gt(gt, 4, False, degradation, degrade=SPEC)


def test_video_test_clips_with_degrade(gpu, tmp_path):
    from edvr_amd import data as D
    write_video_test_tree(str(tmp_path), dict(folders=['000'], frames=3, lq_hw=(16, 20), scale=4))
    opt = dict(name='REDS4', dataroot_gt=os.path.join(str(tmp_path), 'gt'), dataroot_lq=None, io_backend=dict(type='disk'), cache_data=True,
               num_frame=3, padding='reflection')
    lq, gt = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'degrade': SPEC, 'degrade_seed': 5, 'jpeg_quality': 60}), device=gpu).clip('000')
    assert torch.equal(lq, D.lq_from_gt(gt, 4, True, 'bi', jpeg_quality=60, degrade=SPEC, seed=5))
    lq, gt = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'degradation': 'bd', 'degrade': SPEC}), device=gpu).clip('000')
    assert torch.equal(lq, D.lq_from_gt(gt, 4, True, 'bd', degrade=SPEC, seed=0))
    assert not torch.equal(lq, D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'degradation': 'bd', 'quantize': True}), device=gpu).clip('000')[0])


def test_make_lq_with_blur_and_noise(gpu, tmp_path):
    """scripts/make_lq.py --scale 1 --blur-sigma ... --noise-sigma ... writes ops.degrade of the tree's frames, frame i of a clip at frame
    index i whatever the batch size; one frame is checked against the restatement's blur as well."""
    from edvr_amd import ops
    make_lq = _load_script('make_lq')
    root = str(tmp_path)
    write_video_test_tree(root, dict(folders=['000', '011'], frames=3, lq_hw=(9, 13), scale=4))  # GT 36 x 52
    gt = os.path.join(root, 'gt')
    args = make_lq.parse_args([gt, os.path.join(root, 'out'), '--scale', '1', '--blur-sigma', '1.4', '0.8', '0.5', '--blur-size', '7', '--noise-sigma', '4',
                               '--noise-shot', '0.2', '--degrade-seed', '3', '--batch', '2'])
    assert args.degrade == SPEC
    assert make_lq.make_lq(gt, args.lq_root, scale=1, batch=args.batch, degrade=args.degrade, degrade_seed=args.degrade_seed, device=gpu, log=lambda *a: None) == 6
    src, out = _read_tree(gt), _read_tree(args.lq_root)
    assert sorted(src) == sorted(out) and len(out) == 6
    for clip in ('000', '011'):
        names = sorted(k for k in src if k.startswith(clip))
        want = ops.degrade(torch.from_numpy(np.stack([src[k] for k in names])).to(gpu), seed=3, **_spec_args()).cpu().numpy()
        for i, k in enumerate(names):
            assert np.array_equal(out[k], want[i]), k
    blurred = os.path.join(root, 'blurred')
    make_lq.make_lq(gt, blurred, scale=1, degrade={'blur': SPEC['blur']}, device=gpu, log=lambda *a: None)
    name = sorted(src)[0]
    assert np.array_equal(_read_tree(blurred)[name], degrade_ref.degrade(src[name], _spec_args()['blur']))
    with pytest.raises(ValueError):
        make_lq.make_lq(gt, os.path.join(root, 'bad'), scale=1, degrade={'noise': {'sigma': -1}}, device=gpu, log=lambda *a: None)
    with pytest.raises(SystemExit):
        make_lq.parse_args([gt, 'x', '--blur-size', '7'])


# ------------------------------------------------------------------------------------------------ the training loader
BLOCK = {'blur': {'ksize': [3, 11], 'prob': 0.8}, 'noise': {'prob': 0.8}}


def _assert_loader_degrades(opt, gpu, jpeg=None):
    """For one rank and for the second of two, over two epochs: every lq of the loader with lq_degrade is frames_u8_to_f32(ops.degrade(crops,
    the plan's kernel, noise and key, frame index = place in the clip), flags) of the batch the loader yields WITHOUT the option under
    the same seed - then through the JPEG round trip where lq_jpeg is set too; gt and key are identical."""
    from edvr_amd import ops
    with_key = dict(opt, lq_degrade=BLOCK, **({'lq_jpeg': jpeg} if jpeg else {}))
    kinds, flags_seen = set(), set()
    for world, rank in ((1, 0), (2, 1)):
        plain, got, plans = _batches(opt, gpu, world, rank), _batches(with_key, gpu, world, rank), _plans(with_key, world, rank)
        assert len(plain) == len(got) == len(plans) > 0
        for (lq_a, gt_a, key_a), (lq_b, gt_b, key_b), batch in zip(plain, got, plans):
            assert key_a == key_b == [p.key for p in batch]
            assert torch.equal(gt_a, gt_b), key_a
            for i, plan in enumerate(batch):
                crops = _unaugment(lq_a[i], plan.flags)
                assert torch.equal(ops.frames_u8_to_f32(crops[None], bytes([plan.flags]))[0], lq_a[i])  # (the crop bytes, recovered)
                want, d = crops, plan.degrade
                if d is not None:
                    want = ops.degrade(crops, blur=d['kernel'], noise=d['noise'], seed=d['key'], frame_index=list(range(crops.shape[0])))
                if jpeg:
                    want = ops.jpeg_roundtrip(want, [plan.jpeg_quality] * crops.shape[0], '420')
                assert torch.equal(lq_b[i], ops.frames_u8_to_f32(want[None], bytes([plan.flags]))[0]), (plan, world, rank)
                kinds.add((d is None, d is not None and d['kernel'] is not None, d is not None and d['noise'] is not None))
                flags_seen.add(plan.flags)
    assert {(False, True, True), (False, True, False), (False, False, True)} <= kinds
    assert len(flags_seen) > 4


@pytest.mark.parametrize('source, jpeg', [('tree', None), ('gt', None), ('tree', {'quality': [20, 80]})])
def test_loader_degrades_the_lq_crops(gpu, tmp_path, source, jpeg):
    root = str(tmp_path)
    write_png_dataset(root, ['001', '002'], (16, 20), 4, frames=100)
    meta = _meta(tmp_path / 'meta_train.txt', ['001', '002'], 24)
    opt = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
               io_backend=dict(type='disk'), gt_size=32, scale=4, num_frame=5, interval_list=[1, 2], random_reverse=True, use_flip=True,
               use_rot=True, val_partition='REDS4')
    if source == 'gt':
        shutil.rmtree(os.path.join(root, 'lq'))
        opt = dict(opt, dataroot_lq=None, lq_from_gt=dict(scale=4, degradation='bi'))
    _assert_loader_degrades(opt, gpu, jpeg)


def test_vimeo_loader_degrades_the_lq_crops(gpu, tmp_path):
    root = str(tmp_path)
    keys = [f'{c:05d}/{q:04d}' for c in (1, 2) for q in range(1, 9)]
    meta = write_vimeo_train_tree(root, keys, (16, 28), 4)
    opt = dict(type='Vimeo90KDataset', dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), meta_info_file=meta,
               io_backend=dict(type='disk'), num_frame=7, gt_size=32, scale=4, random_reverse=True, use_flip=True, use_rot=True)
    _assert_loader_degrades(opt, gpu)


def test_loader_prob_zero_is_the_plain_loader(gpu, tmp_path):
    root = str(tmp_path)
    write_png_dataset(root, ['001'], (16, 20), 4, frames=100)
    meta = _meta(tmp_path / 'meta_train.txt', ['001'], 12)
    opt = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
               io_backend=dict(type='disk'), gt_size=32, scale=4, num_frame=5, interval_list=[1], random_reverse=False, use_flip=True,
               use_rot=True, val_partition='REDS4')
    plain = _batches(opt, gpu, 1, 0, 1)
    never = _batches(dict(opt, lq_degrade={'blur': {'prob': 0}, 'noise': {'prob': 0.0}}), gpu, 1, 0, 1)
    assert len(plain) == len(never) > 0
    for a, b in zip(plain, never):
        assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_training_loop_with_lq_degrade(gpu, tmp_path):
    """scripts/train_reds.py --lq-from-gt 4 --lq-degrade: training steps on blurred, noisy crops with finite losses."""
    tr = _load_script('train_reds')
    root = str(tmp_path)
    meta = write_png_dataset(root, ['001', '002'], (20, 24), 4, frames=100)
    shutil.rmtree(os.path.join(root, 'lq'))
    args = tr.parse_args(['--gt', os.path.join(root, 'gt'), '--meta', meta, '--lq-from-gt', '4', '--lq-degrade', '--num-feat', '64', '--num-reconstruct-block', '2',
                          '--gt-size', '64', '--batch', '2', '--threads', '4', '--enlarge-ratio', '1', '--iters', '2', '--dcn-lr-mul', '0.25', '--periods', '2', '2',
                          '--restart-weights', '1', '0.5', '--tsa-iter', '0', '--print-freq', '1', '--save-freq', '100'])
    assert args.lq_degrade is True
    losses = tr.train(args, log=lambda *a: None)
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses)
    assert tr.parse_args(['--gt', 'x', '--meta', 'y', '--lq-from-gt', '4']).lq_degrade is False
