"""GPU: everything that calls ops.mpeg_roundtrip - the training loader's `lq_mpeg` option, alone and between `lq_degrade`
and `lq_jpeg`; data.lq_from_gt(mpeg_qscale=) and VideoTestClips; scripts/make_lq.py --mpeg-qscale, whose pieces equal the whole clip;
scripts/train_reds.py --lq-mpeg - against the NumPy restatement tests/mpeg_ref.py, byte for byte."""
import importlib.util
import math
import os
import shutil

import numpy as np
import pytest
import torch

import jpeg_ref
import mpeg_ref
from util_data import write_png_dataset, write_video_test_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _batches(opt, gpu, world, rank, epochs=1):
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


def _plans(opt, world, rank, epochs=1):
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


def _assert_loader_codes(base, extra, gpu, jpeg=False):
    """For one rank and for one of two: every lq of the loader with base + extra options is frames_u8_to_f32(the reference's round trip
    of the crop clip at the plan's qscale [then the JPEG reference at the plan's quality], flags) of the batch the loader yields with
    the base options under the same seed; gt and key are identical.  Frame 0 of the crop clip is the only intra frame."""
    from edvr_amd import ops
    full = dict(base, **extra)
    scales, flags_seen = set(), set()
    for world, rank in ((1, 0), (2, 1)):
        plain, coded, plans = _batches(base, gpu, world, rank), _batches(full, gpu, world, rank), _plans(full, world, rank)
        assert len(plain) == len(coded) == len(plans) > 0
        for (lq_a, gt_a, key_a), (lq_b, gt_b, key_b), batch in zip(plain, coded, plans):
            assert key_a == key_b == [p.key for p in batch]
            assert torch.equal(gt_a, gt_b), key_a
            for i, plan in enumerate(batch):
                crops = _unaugment(lq_a[i], plan.flags)
                assert torch.equal(ops.frames_u8_to_f32(crops[None].to(gpu), bytes([plan.flags]))[0], lq_a[i])  # (the crop bytes, recovered)
                want = mpeg_ref.roundtrip_clip(crops.cpu().numpy(), plan.mpeg_qscale, 0, full['lq_mpeg'].get('search', 7))
                if jpeg:
                    want = jpeg_ref.roundtrip_batch(want, plan.jpeg_quality)
                want = ops.frames_u8_to_f32(torch.from_numpy(want)[None].to(gpu), bytes([plan.flags]))[0]
                assert torch.equal(lq_b[i], want), (plan, world, rank)
                assert plan.mpeg_qscale == 0 or not torch.equal(lq_b[i], lq_a[i])
                scales.add(plan.mpeg_qscale)
                flags_seen.add(plan.flags)
    return scales, flags_seen


def _train_opt(tmp_path, source):
    root = str(tmp_path)
    write_png_dataset(root, ['001', '002'], (28, 40), 4, frames=100)  # (REDS clips have 100 frames, whatever the meta file's count)
    meta = tmp_path / 'meta_train.txt'
    meta.write_text(''.join(f'{clip} 24 (112,160,3)\n' for clip in ('001', '002')))
    opt = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=str(meta),
               io_backend=dict(type='disk'), gt_size=96, scale=4, num_frame=5, interval_list=[1, 2], random_reverse=True, use_flip=True,
               use_rot=True, val_partition='REDS4')  # LQ crops of 24 x 24: padded to 32, four macroblocks
    if source == 'gt':
        shutil.rmtree(os.path.join(root, 'lq'))
        opt = dict(opt, dataroot_lq=None, lq_from_gt=dict(scale=4, degradation='bi'))
    return opt


@pytest.mark.parametrize('source', ['tree', 'gt'])
def test_loader_codes_the_lq_crop_clips(gpu, tmp_path, source):
    scales, flags = _assert_loader_codes(_train_opt(tmp_path, source), {'lq_mpeg': {'qscale': [2, 20], 'search': 5, 'prob': 0.8}}, gpu)
    assert len(scales) > 4 and 0 in scales and all(q == 0 or 2 <= q <= 20 for q in scales) and len(flags) > 3


def test_loader_composes_degrade_mpeg_jpeg_in_that_order(gpu, tmp_path):
    base = dict(_train_opt(tmp_path, 'tree'), lq_degrade={'blur': {}, 'noise': {}})
    scales, _ = _assert_loader_codes(base, {'lq_mpeg': {'qscale': [2, 20]}, 'lq_jpeg': {'quality': [30, 90]}}, gpu, jpeg=True)
    assert 0 not in scales and len(scales) > 3


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_lq_from_gt(gpu, degradation):
    from edvr_amd import data as D, ops
    from util_mpeg import moving_clip
    gt = ops.frames_u8_to_f32(moving_clip(4, 64, 96, (4, -8), 50).to(gpu)[None])[0]
    plain = D.lq_from_gt(gt, 4, True, degradation)
    lq_bytes = (plain * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(ops.frames_u8_to_f32(lq_bytes[None])[0], plain)
    for kw in ({}, {'mpeg_gop': 2, 'mpeg_search': 3}, {'mpeg_gop': 0, 'mpeg_search': 0}):
        ref = mpeg_ref.roundtrip_clip(lq_bytes.cpu().numpy(), 6, kw.get('mpeg_gop', 12), kw.get('mpeg_search', 7))
        want = ops.frames_u8_to_f32(torch.from_numpy(ref).to(gpu)[None])[0]
        assert torch.equal(D.lq_from_gt(gt, 4, None, degradation, mpeg_qscale=6, **kw), want)  # 'bd': the scale implies quantize
        assert torch.equal(D.lq_from_gt(gt, 4, True, degradation, mpeg_qscale=6, **kw), want)
    assert not torch.equal(want, plain)
    # between degrade and the JPEG round trip
    blur = {'blur': {'ksize': 5, 'sigma_x': 1.0, 'sigma_y': 1.0, 'theta': 0.0}}
    blurred = D.lq_from_gt(gt, 4, True, degradation, degrade=blur)
    b_bytes = (blurred * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    ref = jpeg_ref.roundtrip_batch(mpeg_ref.roundtrip_clip(b_bytes, 6, 12, 7), 50)
    assert torch.equal(D.lq_from_gt(gt, 4, None, degradation, degrade=blur, mpeg_qscale=6, jpeg_quality=50),
                       ops.frames_u8_to_f32(torch.from_numpy(ref).to(gpu)[None])[0])
    with pytest.raises(ValueError):
        D.lq_from_gt(gt, 4, False, degradation, mpeg_qscale=6)


def test_video_test_clips_with_mpeg_qscale(gpu, tmp_path):
    from edvr_amd import data as D
    write_video_test_tree(str(tmp_path), dict(folders=['000'], frames=3, lq_hw=(16, 20), scale=4))
    opt = dict(name='REDS4', dataroot_gt=os.path.join(str(tmp_path), 'gt'), dataroot_lq=None, io_backend=dict(type='disk'), cache_data=True,
               num_frame=3, padding='reflection')
    plain, gt = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4}), device=gpu).clip('000')
    lq, gt2 = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'mpeg_qscale': 5, 'mpeg_search': 4}), device=gpu).clip('000')
    assert torch.equal(gt, gt2) and torch.equal(lq, D.lq_from_gt(gt, 4, True, 'bi', mpeg_qscale=5, mpeg_search=4))
    ref = mpeg_ref.roundtrip_clip((plain * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy(), 5, 12, 4)
    assert np.array_equal((lq * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy(), ref) and not torch.equal(lq, plain)


def _read_tree(root):
    from edvr_amd.data import decode_image
    out = {}
    for dp, _, fs in os.walk(root):
        for f in (f for f in fs if not f.startswith('.')):
            with open(os.path.join(dp, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(dp, f), root)] = decode_image(fh.read())
    return out


def test_make_lq_pieces_equal_the_whole_clip(gpu, tmp_path):
    """A 10-frame clip written in pieces of --batch 4: with gop 3 the pieces are cut at 3, 6, 9, with gop 0 the clip is one piece - and
    the tree is the reference's round trip of the whole clip of the tree written without the option, whatever the batch."""
    make_lq = _load_script('make_lq')
    root = str(tmp_path)
    write_video_test_tree(root, dict(folders=['000', '011'], frames=10, lq_hw=(9, 13), scale=4))  # GT 36 x 52
    gt = os.path.join(root, 'gt')
    quiet = dict(device=gpu, log=lambda *a: None)
    plain = os.path.join(root, 'plain')
    assert make_lq.make_lq(gt, plain, scale=2, **quiet) == 20
    a = _read_tree(plain)
    for gop, batch in ((3, 4), (3, 16), (0, 4), (12, 4)):
        coded = os.path.join(root, f'mpeg_{gop}_{batch}')
        assert make_lq.make_lq(gt, coded, scale=2, batch=batch, mpeg_qscale=7, mpeg_gop=gop, mpeg_search=5, **quiet) == 20
        b = _read_tree(coded)
        assert sorted(a) == sorted(b) and len(b) == 20
        for folder in ('000', '011'):
            names = sorted(k for k in a if k.startswith(folder))
            want = mpeg_ref.roundtrip_clip(np.stack([a[k] for k in names]), 7, gop, 5)
            for k, w in zip(names, want):
                assert np.array_equal(b[k], w), (gop, batch, k)
    for bad in (dict(mpeg_qscale=0), dict(mpeg_qscale=32), dict(mpeg_qscale=5, mpeg_gop=-1), dict(mpeg_qscale=5, mpeg_search=16)):
        with pytest.raises(ValueError):
            make_lq.make_lq(gt, os.path.join(root, 'bad'), scale=2, **bad, **quiet)
    with pytest.raises(SystemExit):
        make_lq.parse_args(['a', 'b', '--mpeg-qscale', '40'])
    args = make_lq.parse_args(['a', 'b', '--mpeg-qscale', '4', '--mpeg-gop', '0'])
    assert (args.mpeg_qscale, args.mpeg_gop, args.mpeg_search) == (4, 0, 7)


def test_eval_video_options():
    ev = _load_script('eval_video')
    args = ev.parse_args(['--gt', 'x', '--lq-from-gt', '4', '--mpeg-qscale', '6', '--mpeg-gop', '0', '--mpeg-search', '15'])
    assert (args.mpeg_qscale, args.mpeg_gop, args.mpeg_search) == (6, 0, 15)
    for bad in (['--mpeg-qscale', '32'], ['--mpeg-qscale', '6', '--mpeg-search', '16'], ['--mpeg-qscale', '6', '--mpeg-gop', '-1']):
        with pytest.raises(SystemExit):
            ev.parse_args(['--gt', 'x', '--lq-from-gt', '4'] + bad)
    with pytest.raises(SystemExit):
        ev.parse_args(['--gt', 'x', '--lq', 'y', '--mpeg-qscale', '6'])  # needs --lq-from-gt


def test_training_loop_with_lq_mpeg(gpu, tmp_path):
    """scripts/train_reds.py --lq-from-gt 4 --lq-mpeg 2 12: training steps on coded crop clips with finite losses, and a validation whose
    LQ frames are made from GT and coded at the default (LO + HI) // 2."""
    tr = _load_script('train_reds')
    root = str(tmp_path)
    meta = write_png_dataset(root, ['001', '002'], (20, 24), 4, frames=100)
    write_video_test_tree(os.path.join(root, 'val'), dict(folders=['000'], frames=6, lq_hw=(16, 20), scale=4))
    shutil.rmtree(os.path.join(root, 'lq'))
    shutil.rmtree(os.path.join(root, 'val', 'lq'))
    args = tr.parse_args(['--gt', os.path.join(root, 'gt'), '--meta', meta, '--lq-from-gt', '4', '--lq-mpeg', '2', '12',
                          '--val-gt', os.path.join(root, 'val', 'gt'), '--num-feat', '64', '--num-reconstruct-block', '2', '--gt-size', '64',
                          '--batch', '2', '--threads', '4', '--enlarge-ratio', '1', '--iters', '2', '--dcn-lr-mul', '0.25', '--periods', '2', '2',
                          '--restart-weights', '1', '0.5', '--tsa-iter', '0', '--print-freq', '1', '--save-freq', '100', '--val-freq', '2',
                          '--val-batch', '3'])
    assert args.lq_mpeg == [2, 12] and args.lq_mpeg_prob == 1.0 and args.val_mpeg_qscale is None
    lines = []
    losses = tr.train(args, log=lines.append)
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses)
    assert any('validation PSNR' in ln for ln in lines)
    for bad in (['--lq-mpeg', '12', '2'], ['--lq-mpeg', '0', '12'], ['--lq-mpeg', '2', '32'], ['--lq-mpeg-prob', '0.5'],
                ['--lq-mpeg', '2', '12', '--val-mpeg-qscale', '0']):
        with pytest.raises(SystemExit):
            tr.parse_args(['--gt', 'x', '--meta', 'y', '--lq-from-gt', '4'] + bad)
