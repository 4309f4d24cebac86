"""GPU: ops.jpeg_roundtrip (csrc/jpeg.hip) against PIL's libjpeg - torch.equal with the committed fixture - and against the
NumPy restatement tests/jpeg_ref.py, and everything that calls it: lq_from_gt, scripts/make_lq.py, the training loader's `lq_jpeg` option
and scripts/train_reds.py --lq-jpeg."""
import importlib.util
import io
import math
import os
import shutil

import numpy as np
import pytest
import torch

import jpeg_ref
from util_data import write_png_dataset, write_video_test_tree, write_vimeo_train_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_roundtrip.pt')


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _frames(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    base = 128 + 90 * torch.sin(xx / 3.0 + yy / 5.0)
    return (base[None, ..., None] + 40 * torch.randn(n, h, w, 3, generator=g)).clamp(0, 255).to(torch.uint8)


def _ref(frames, quality, subsampling='420'):
    return torch.from_numpy(jpeg_ref.roundtrip_batch(frames.cpu().numpy(), quality, subsampling))


def test_equals_pil_on_the_fixture(gpu):
    from edvr_amd import ops
    gold = torch.load(GOLDEN)
    count = 0
    for case in gold['cases']:
        x = case['input'][None].to(gpu)
        for q, s, want in case['outputs']:
            got = ops.jpeg_roundtrip(x, q, s)
            assert got.dtype == torch.uint8 and got.shape == x.shape
            assert torch.equal(got[0].cpu(), want), (case['name'], q, s, int((got[0].cpu().int() - want.int()).abs().max()))
            count += 1
    assert count > 80


def test_equals_the_reference_on_random_shapes(gpu):
    from edvr_amd import ops
    rng = np.random.default_rng(77)
    for i in range(10):
        h, w, n = int(rng.integers(1, 151)), int(rng.integers(1, 151)), int(rng.integers(1, 3))
        q, s = int(rng.integers(1, 101)), ('420', '444')[i & 1]
        x = _frames(n, h, w, 300 + i)
        assert torch.equal(ops.jpeg_roundtrip(x.to(gpu), q, s).cpu(), _ref(x, q, s)), (h, w, n, q, s)


@pytest.mark.parametrize('subsampling', ['420', '444'])
def test_batch_with_a_pass_through_image(gpu, subsampling):
    """Qualities (10, 0, 90): the middle image comes back untouched, each image equals its single-image call; and the scalar, list and
    device-table forms of `quality` agree."""
    from edvr_amd import ops
    x = _frames(3, 70, 90, 1).to(gpu)
    q = (10, 0, 90)
    out = ops.jpeg_roundtrip(x, list(q), subsampling)
    assert torch.equal(out[1], x[1])
    for i in range(3):
        assert torch.equal(out[i], ops.jpeg_roundtrip(x[i:i + 1], q[i], subsampling)[0]), i
    assert not torch.equal(out[0], x[0]) and not torch.equal(out[0], ops.jpeg_roundtrip(x[:1], 90, subsampling)[0])
    assert torch.equal(out, ops.jpeg_roundtrip(x, torch.tensor(q, dtype=torch.int32, device=gpu), subsampling))
    assert torch.equal(out, ops.jpeg_roundtrip(x, tuple(q), subsampling))
    same = ops.jpeg_roundtrip(x, 35, subsampling)
    assert torch.equal(same, ops.jpeg_roundtrip(x, [35, 35, 35], subsampling))
    assert torch.equal(same, ops.jpeg_roundtrip(x, torch.full((3,), 35, dtype=torch.int32, device=gpu), subsampling))
    assert torch.equal(same.cpu(), _ref(x, 35, subsampling))
    # a device table is clamped to 0 .. 100 by the kernel
    wild = ops.jpeg_roundtrip(x, torch.tensor([-5, 250, 100], dtype=torch.int32, device=gpu), subsampling)
    assert torch.equal(wild, ops.jpeg_roundtrip(x, [0, 100, 100], subsampling))


@pytest.mark.parametrize('gap, offset', [(18, 3), (16, 4)])  # image strides and bases that are not / are multiples of 4: byte and dword accesses
def test_image_strided_slices(gpu, gap, offset):
    from edvr_amd import ops
    n, h, w = 3, 40, 52
    x = _frames(n, h, w, 2)
    frame = 3 * h * w
    pitch, shape = frame + gap, (n, h, w, 3)
    src = torch.zeros((n + 1) * pitch, dtype=torch.uint8, device=gpu)
    view = src.as_strided(shape, (pitch, 3 * w, 3, 1), pitch - offset)
    view.copy_(x.to(gpu))
    assert view.stride(0) == pitch and torch.equal(view.cpu(), x)
    want = _ref(x, 60)
    assert torch.equal(ops.jpeg_roundtrip(view, 60).cpu(), want)
    dst = torch.full(((n + 1) * pitch,), 7, dtype=torch.uint8, device=gpu)
    out = dst.as_strided(shape, (pitch, 3 * w, 3, 1), offset)
    assert ops.jpeg_roundtrip(view, 60, out=out) is out
    assert torch.equal(out.cpu(), want)
    written = torch.zeros_like(dst, dtype=torch.bool)
    written.as_strided(shape, (pitch, 3 * w, 3, 1), offset).fill_(True)
    assert bool((dst[~written] == 7).all()) and int((~written).sum()) == (n + 1) * pitch - n * frame  # bytes between the images are left alone
    # a slice of a longer batch
    longer = _frames(5, h, w, 3).to(gpu)
    assert torch.equal(ops.jpeg_roundtrip(longer[1:4], 60), ops.jpeg_roundtrip(longer, 60)[1:4])


def test_refusals(gpu):
    from edvr_amd import ops
    x = _frames(2, 16, 16, 4).to(gpu)
    with pytest.raises(NotImplementedError):
        ops.jpeg_roundtrip(x.cpu(), 50)
    with pytest.raises(NotImplementedError):
        ops.jpeg_roundtrip(x, 50, out=torch.empty(2, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='overlaps'):
        ops.jpeg_roundtrip(x, 50, out=x)
    buf = torch.zeros(3, 16, 16, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match='overlaps'):
        ops.jpeg_roundtrip(buf[:2], 50, out=buf[1:])
    for bad in (101, -1, 50.5, [50], [50, 101], torch.tensor([50, 50], device=gpu), torch.tensor([50], dtype=torch.int32, device=gpu)):
        with pytest.raises(ValueError):
            ops.jpeg_roundtrip(x, bad)
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip(x, 50, '422')
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip(x.float(), 50)
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip(x, 50, out=torch.empty(2, 16, 16, 3, dtype=torch.float32, device=gpu))


def test_launch_is_booked_with_algorithmic_bytes(gpu):
    from edvr_amd import ops
    seen = []

    def hook(name, flops, launch, nbytes, executed):
        seen.append((name, flops, nbytes))
        launch()

    x = _frames(3, 33, 47, 5).to(gpu)
    prev, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, hook
    try:
        ops.jpeg_roundtrip(x, 50)
        ops.jpeg_roundtrip(x, torch.full((3,), 50, dtype=torch.int32, device=gpu), '444')
    finally:
        ops.LAUNCH_HOOK = prev
    px = 3 * 33 * 47
    assert seen == [('jpeg_roundtrip', 0.0, 3.0 * px + 3.0 * px), ('jpeg_roundtrip', 0.0, 3.0 * px + 3.0 * px + 4 * 3)]


def test_graph_replay_equals_eager(gpu):
    """Captured once and replayed on new pixels and a new table in the same buffers: the bytes of the eager call."""
    from edvr_amd import ops
    a, b = _frames(3, 70, 66, 6), _frames(3, 70, 66, 7)
    qa, qb = torch.tensor([10, 50, 90], dtype=torch.int32), torch.tensor([75, 0, 20], dtype=torch.int32)
    x, q = a.to(gpu), qa.to(gpu)
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(stream):
        ops.jpeg_roundtrip(x, q)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = ops.jpeg_roundtrip(x, q)
        out444 = ops.jpeg_roundtrip(x, 30, '444')
    x.copy_(b), q.copy_(qb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.jpeg_roundtrip(b.to(gpu), qb.to(gpu))) and torch.equal(out.cpu(), _ref(b, qb.tolist()))
    assert torch.equal(out444, ops.jpeg_roundtrip(b.to(gpu), 30, '444'))
    assert not torch.equal(out, ops.jpeg_roundtrip(a.to(gpu), qa.to(gpu)))


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_lq_from_gt(gpu, degradation):
    from edvr_amd import data as D, ops
    gt = ops.frames_u8_to_f32(_frames(3, 64, 96, 8).to(gpu)[None])[0]
    plain = D.lq_from_gt(gt, 4, True, degradation)
    lq_bytes = (plain * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(ops.frames_u8_to_f32(lq_bytes[None])[0], plain)  # (the bytes the quantised LQ frames are made of)
    for kw in ({}, {'jpeg_subsampling': '444'}):
        want = ops.frames_u8_to_f32(ops.jpeg_roundtrip(lq_bytes, 40, kw.get('jpeg_subsampling', '420'))[None])[0]
        assert torch.equal(D.lq_from_gt(gt, 4, None, degradation, jpeg_quality=40, **kw), want)  # 'bd': the quality implies quantize
        assert torch.equal(D.lq_from_gt(gt, 4, True, degradation, jpeg_quality=40, **kw), want)
    assert not torch.equal(want, plain)
    with pytest.raises(ValueError):
        D.lq_from_gt(gt, 4, False, degradation, jpeg_quality=40)


def test_video_test_clips_with_jpeg_quality(gpu, tmp_path):
    from edvr_amd import data as D
    write_video_test_tree(str(tmp_path), dict(folders=['000'], frames=3, lq_hw=(16, 20), scale=4))
    opt = dict(name='REDS4', dataroot_gt=os.path.join(str(tmp_path), 'gt'), dataroot_lq=None, io_backend=dict(type='disk'), cache_data=True,
               num_frame=3, padding='reflection')
    lq, gt = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'jpeg_quality': 30}), device=gpu).clip('000')
    assert torch.equal(lq, D.lq_from_gt(gt, 4, True, 'bi', jpeg_quality=30))
    assert not torch.equal(lq, D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4}), device=gpu).clip('000')[0])


def _pil_roundtrip(img, quality, subsampling):
    try:
        from PIL import Image
    except ImportError:
        return jpeg_ref.roundtrip(img, quality, subsampling)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=quality, subsampling={'444': 0, '420': 2}[subsampling])
    buf.seek(0)
    return np.asarray(Image.open(buf).convert('RGB'))


def _read_tree(root):
    from edvr_amd.data import decode_image
    out = {}
    for dp, _, fs in os.walk(root):
        for f in (f for f in fs if not f.startswith('.')):
            with open(os.path.join(dp, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(dp, f), root)] = decode_image(fh.read())
    return out


def test_make_lq_with_jpeg_quality(gpu, tmp_path):
    """The tree scripts/make_lq.py writes with jpeg_quality = PIL's round trip of the tree it writes without; --scale 1 compresses
    the tree at its own size, and imresize at scale 1 - which make_lq now skips - is the identity on bytes."""
    from edvr_amd import ops
    make_lq = _load_script('make_lq')
    root = str(tmp_path)
    write_video_test_tree(root, dict(folders=['000', '011'], frames=3, lq_hw=(9, 13), scale=4))  # GT 36 x 52
    gt = os.path.join(root, 'gt')
    quiet = dict(device=gpu, log=lambda *a: None)
    for scale, sub in ((4, '420'), (2, '444'), (1, '420')):
        plain, comp = os.path.join(root, f'plain{scale}'), os.path.join(root, f'jpeg{scale}')
        assert make_lq.make_lq(gt, plain, scale=scale, **quiet) == 6
        assert make_lq.make_lq(gt, comp, scale=scale, jpeg_quality=35, jpeg_subsampling=sub, **quiet) == 6
        a, b = _read_tree(plain), _read_tree(comp)
        assert sorted(a) == sorted(b) and len(a) == 6
        for name in a:
            assert a[name].shape == (36 // scale, 52 // scale, 3)
            assert np.array_equal(b[name], _pil_roundtrip(a[name], 35, sub)), (scale, name)
    ones = _read_tree(os.path.join(root, 'plain1'))
    gts = _read_tree(gt)
    assert all(np.array_equal(ones[k], gts[k]) for k in ones)
    x = _frames(2, 36, 52, 9).to(gpu)
    assert torch.equal(ops.imresize(x, 1, out_dtype=torch.uint8), x) and torch.equal(ops.imresize(x, 1, False, out_dtype=torch.uint8), x)
    with pytest.raises(ValueError):
        make_lq.make_lq(gt, os.path.join(root, 'bad'), scale=4, jpeg_quality=0, **quiet)
    with pytest.raises(ValueError):
        make_lq.make_lq(gt, os.path.join(root, 'bad'), scale=4, jpeg_quality=50, jpeg_subsampling='422', **quiet)


# ------------------------------------------------------------------------------------------------ the training loader
def _batches(opt, gpu, world, rank, epochs=2):
    from edvr_amd import data as D
    loader = D.REDSDeviceLoader(opt, 4, device=gpu, rank=rank, world_size=world, seed=7, num_threads=4, depth=2)
    out = []
    try:
        for epoch in range(epochs):
            if epoch:
                loader.reset(epoch)
            while True:
                b = loader.next()
                if b is None:
                    break
                out.append((b['lq'].clone(), b['gt'].clone(), list(b['key'])))
        torch.cuda.synchronize()
    finally:
        loader.close()
    return out


def _plans(opt, world, rank, epochs=2):
    """The plans of the same epochs in batches of 4, from the planner, sampler and random stream the loader uses."""
    from edvr_amd import data as D
    planner = D.make_planner(opt)
    sampler = D.EnlargedSampler(planner, world, rank)
    out = []
    for epoch in range(epochs):
        sampler.set_epoch(epoch)
        rng = D.epoch_rng(7 + rank, epoch)
        if hasattr(planner, 'reset_epoch'):
            planner.reset_epoch()
        order = list(sampler)
        for b0 in range(0, len(order) - 3, 4):
            out.append([planner.plan(i, rng) for i in order[b0:b0 + 4]])
    return out


def _unaugment(lq, flags):
    """(t, 3, p', p'') of one clip after hflip, vflip, transpose -> the crop bytes (t, p, p, 3) before them."""
    from edvr_amd.data import AUG_HFLIP, AUG_ROT90, AUG_VFLIP
    x = lq
    if flags & AUG_ROT90:
        x = x.transpose(-1, -2)
    if flags & AUG_VFLIP:
        x = x.flip(-2)
    if flags & AUG_HFLIP:
        x = x.flip(-1)
    return (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _assert_loader_compresses(opt, gpu, subsampling='420'):
    """Over two epochs, for one rank and for each of two: every lq of the loader with lq_jpeg is frames_u8_to_f32(jpeg_roundtrip(crops,
    the plans' qualities), flags) of the batch the loader yields WITHOUT the option under the same seed; gt and key are identical."""
    from edvr_amd import ops
    with_jpeg = dict(opt, lq_jpeg={'quality': [20, 80], 'subsampling': subsampling})
    qualities, flags_seen = set(), set()
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        plain, comp, plans = _batches(opt, gpu, world, rank), _batches(with_jpeg, gpu, world, rank), _plans(with_jpeg, world, rank)
        assert len(plain) == len(comp) == len(plans) > 0
        for (lq_a, gt_a, key_a), (lq_b, gt_b, key_b), batch in zip(plain, comp, plans):
            assert key_a == key_b == [p.key for p in batch]
            assert torch.equal(gt_a, gt_b), key_a
            assert lq_a.shape == lq_b.shape
            for i, plan in enumerate(batch):
                crops = _unaugment(lq_a[i], plan.flags)
                assert torch.equal(ops.frames_u8_to_f32(crops[None], bytes([plan.flags]))[0], lq_a[i])  # (the crop bytes, recovered)
                want = ops.frames_u8_to_f32(ops.jpeg_roundtrip(crops, [plan.jpeg_quality] * crops.shape[0], subsampling)[None], bytes([plan.flags]))[0]
                assert torch.equal(lq_b[i], want), (plan, world, rank)
                assert not torch.equal(lq_b[i], lq_a[i])
                qualities.add(plan.jpeg_quality)
                flags_seen.add(plan.flags)
    assert len(qualities) > 5 and all(20 <= q <= 80 for q in qualities)
    assert len(flags_seen) > 4


def _meta(path, clips, frames):
    with open(path, 'w') as fh:
        fh.writelines(f'{clip} {frames} (64,80,3)\n' for clip in clips)
    return str(path)


@pytest.mark.parametrize('source', ['tree', 'gt'])
def test_loader_compresses_the_lq_crops(gpu, tmp_path, source):
    root = str(tmp_path)
    write_png_dataset(root, ['001', '002'], (16, 20), 4, frames=100)
    meta = _meta(tmp_path / 'meta_train.txt', ['001', '002'], 24)
    opt = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
               io_backend=dict(type='disk'), gt_size=32, scale=4, num_frame=5, interval_list=[1, 2], random_reverse=True, use_flip=True,
               use_rot=True, val_partition='REDS4')
    if source == 'gt':
        shutil.rmtree(os.path.join(root, 'lq'))
        opt = dict(opt, dataroot_lq=None, lq_from_gt=dict(scale=4, degradation='bi'))
    _assert_loader_compresses(opt, gpu)


def test_vimeo_loader_compresses_the_lq_crops(gpu, tmp_path):
    root = str(tmp_path)
    keys = [f'{c:05d}/{q:04d}' for c in (1, 2) for q in range(1, 9)]
    meta = write_vimeo_train_tree(root, keys, (16, 28), 4)
    opt = dict(type='Vimeo90KDataset', dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), meta_info_file=meta,
               io_backend=dict(type='disk'), num_frame=7, gt_size=32, scale=4, random_reverse=True, use_flip=True, use_rot=True)
    _assert_loader_compresses(opt, gpu, '444')


def test_loader_prob_zero_is_the_plain_loader(gpu, tmp_path):
    root = str(tmp_path)
    write_png_dataset(root, ['001'], (16, 20), 4, frames=100)
    meta = _meta(tmp_path / 'meta_train.txt', ['001'], 12)
    opt = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
               io_backend=dict(type='disk'), gt_size=32, scale=4, num_frame=5, interval_list=[1], random_reverse=False, use_flip=True,
               use_rot=True, val_partition='REDS4')
    plain, never = _batches(opt, gpu, 1, 0, 1), _batches(dict(opt, lq_jpeg={'quality': 30, 'prob': 0.0}), gpu, 1, 0, 1)
    assert len(plain) == len(never) > 0
    for a, b in zip(plain, never):
        assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_training_loop_with_lq_jpeg(gpu, tmp_path):
    """scripts/train_reds.py --lq-from-gt 4 --lq-jpeg 30 90: training steps on compressed crops with finite losses, and a validation whose
    LQ frames are made from GT and compressed at the default (LO + HI) // 2."""
    tr = _load_script('train_reds')
    root = str(tmp_path)
    meta = write_png_dataset(root, ['001', '002'], (20, 24), 4, frames=100)
    write_video_test_tree(os.path.join(root, 'val'), dict(folders=['000'], frames=6, lq_hw=(16, 20), scale=4))  # (no fewer than --num-frame)
    shutil.rmtree(os.path.join(root, 'lq'))
    shutil.rmtree(os.path.join(root, 'val', 'lq'))
    args = tr.parse_args(['--gt', os.path.join(root, 'gt'), '--meta', meta, '--lq-from-gt', '4', '--lq-jpeg', '30', '90',
                          '--val-gt', os.path.join(root, 'val', 'gt'), '--num-feat', '64', '--num-reconstruct-block', '2', '--gt-size', '64',
                          '--batch', '2', '--threads', '4', '--enlarge-ratio', '1', '--iters', '2', '--dcn-lr-mul', '0.25', '--periods', '2', '2',
                          '--restart-weights', '1', '0.5', '--tsa-iter', '0', '--print-freq', '1', '--save-freq', '100', '--val-freq', '2',
                          '--val-batch', '3'])
    assert args.lq_jpeg == [30, 90] and args.lq_jpeg_prob == 1.0 and args.val_jpeg_quality is None
    lines = []
    losses = tr.train(args, log=lines.append)
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses)
    assert any('validation PSNR' in ln for ln in lines)
    for bad in (['--lq-jpeg', '90', '30'], ['--lq-jpeg', '0', '30'], ['--lq-jpeg-prob', '0.5'], ['--lq-jpeg', '30', '90', '--val-jpeg-quality', '0']):
        with pytest.raises(SystemExit):
            tr.parse_args(['--gt', 'x', '--meta', 'y', '--lq-from-gt', '4'] + bad)
