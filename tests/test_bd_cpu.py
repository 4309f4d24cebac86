"""CPU: the host side of the BD downsampling feature - bd_shape and its refusals, the host weights against scipy, the fixture file, and
the argument handling and option plumbing of scripts/make_lq.py, scripts/eval_video.py, lq_from_gt, VideoTestClips and VideoTestDUFClips
with the device call replaced by a stand-in (as tests/test_imresize_cpu.py does)."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

from util_bd import FIXTURE_CASES, FIXTURE_FRAMES, GOLDEN, bd_f64, gauss13, load_golden
from util_data import png_bytes, write_video_test_tree


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_file_is_whole():
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    cases = load_golden()
    assert len(cases) == len(FIXTURE_CASES) == 12
    for case, ((h, w), scale) in zip(cases, FIXTURE_CASES):
        assert sorted(case) == ['input', 'output', 'scale']
        assert case['input'].dtype == torch.uint8 and tuple(case['input'].shape) == (FIXTURE_FRAMES, h, w, 3) and case['scale'] == scale
        out = case['output']
        assert out.dtype == torch.float32 and tuple(out.shape) == (FIXTURE_FRAMES, 3, -(-h // scale), -(-w // scale)) and bool(torch.isfinite(out).all())
        # the reference's output is the formula's: the float64 restatement the GPU test also uses sits within the reference's own rounding
        x = (case['input'].float() / 255).permute(0, 3, 1, 2)
        assert (bd_f64(x, scale) - out.double()).abs().max().item() < 1e-6


def test_bd_shape():
    import edvr_amd
    from edvr_amd import data
    assert edvr_amd.duf_downsample is data.duf_downsample and edvr_amd.bd_shape is data.bd_shape
    for case, ((h, w), scale) in zip(load_golden(), FIXTURE_CASES):
        assert data.bd_shape(h, w, scale) == tuple(case['output'].shape[2:])
    assert data.bd_shape(720, 1280, 4) == (180, 320) and data.bd_shape(2880, 5120, 4) == (720, 1280)
    assert data.bd_shape(37, 53, 2) == (19, 27) and data.bd_shape(37, 53, 3) == (13, 18) and data.bd_shape(37, 53, 4) == (10, 14)
    assert data.bd_shape(7, 7, 4) == (2, 2) and data.bd_shape(7, 9, 2) == (4, 5)  # smaller than the reference's pad admits, fine for the formula


def test_bd_shape_refusals():
    from edvr_amd.data import bd_shape
    for h, w, scale in ((64, 96, 1), (64, 96, 5), (64, 96, 0), (64, 96, 8), (64, 96, 2.5), (64, 96, 0.25), (64, 96, True),
                        (6, 96, 4), (64, 6, 4), (6, 6, 2), (0, 8, 2), (1, 1, 3)):
        with pytest.raises(ValueError):
            bd_shape(h, w, scale)


@pytest.mark.parametrize('scale,taps', [(2, 7), (3, 11), (4, 13)])
def test_host_weights_are_scipys(scale, taps):
    """The 13 float64 weights: their outer product IS generate_gaussian_kernel's filter (gaussian_filter of a 13 x 13 Dirac), exactly."""
    from scipy.ndimage import gaussian_filter
    from edvr_amd.data import bd_weights
    g = bd_weights(scale)
    assert g.dtype == np.float64 and g.shape == (13,) and np.count_nonzero(g) == taps
    assert np.array_equal(g, g[::-1]) and abs(g.sum() - 1) < 1e-15 and g.argmax() == 6
    dirac = np.zeros((13, 13))
    dirac[6, 6] = 1
    assert np.array_equal(np.outer(g, g), gaussian_filter(dirac, 0.4 * scale))
    assert np.abs(g - gauss13(scale)).max() < 1e-16  # the test helper's independent statement
    for bad in (1, 5, 2.5):
        with pytest.raises(ValueError):
            bd_weights(bad)


def test_cpu_tensors_and_bad_arguments_raise():
    from edvr_amd import data, ops
    with pytest.raises(NotImplementedError):
        data.duf_downsample(torch.rand(2, 3, 32, 32))
    with pytest.raises(NotImplementedError):
        data.duf_downsample(torch.rand(1, 2, 3, 32, 32), scale=2)
    with pytest.raises(NotImplementedError):
        ops.bd_downsample(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), 4, out_dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        data.duf_downsample(np.zeros((2, 3, 32, 32), np.float32))
    with pytest.raises(ValueError):
        data.duf_downsample(torch.rand(2, 3, 32, 32), kernel_size=11)
    with pytest.raises(ValueError):
        data.lq_from_gt(torch.rand(2, 3, 32, 32), 4, degradation='blur')


def _stand_ins(calls):
    """ops.bd_downsample / ops.imresize on the host for the plumbing tests: nearest sampling of the right SHAPE, recording the arguments."""
    def shrink(name, frames, ho, wo, out_dtype):
        u8 = frames.dtype == torch.uint8
        x = frames.permute(0, 3, 1, 2).float() / 255 if u8 else frames.float()
        calls.append((name, tuple(frames.shape), str(frames.dtype), out_dtype))
        out = torch.nn.functional.interpolate(x, size=(ho, wo), mode='nearest')
        return (out.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() if out_dtype == torch.uint8 else out

    def bd_downsample(frames, scale=4, out_dtype=torch.float32):
        from edvr_amd.data import bd_shape
        h, w = (frames.shape[1:3] if frames.dtype == torch.uint8 else frames.shape[-2:])
        return shrink(f'bd{scale}', frames, *bd_shape(h, w, scale), out_dtype)

    def imresize(frames, scale, antialiasing=True, out_dtype=torch.float32):
        from edvr_amd.data import imresize_shape
        h, w = (frames.shape[1:3] if frames.dtype == torch.uint8 else frames.shape[-2:])
        return shrink(f'bi{scale:g}', frames, *imresize_shape(h, w, scale, antialiasing), out_dtype)
    return bd_downsample, imresize


def _patch(monkeypatch, calls):
    from edvr_amd import ops
    bd, bi = _stand_ins(calls)
    monkeypatch.setattr(ops, 'bd_downsample', bd)
    monkeypatch.setattr(ops, 'imresize', bi)
    monkeypatch.setattr(ops, 'frames_u8_to_f32', lambda u8: u8.permute(0, 1, 4, 2, 3).float() / 255)


def test_lq_from_gt_degradations(monkeypatch):
    from edvr_amd import data
    calls = []
    _patch(monkeypatch, calls)
    gt = torch.rand(2, 3, 32, 48)
    assert tuple(data.lq_from_gt(gt, 4).shape) == (2, 3, 8, 12)                        # as before: bicubic, 8-bit
    assert tuple(data.lq_from_gt(gt, 4, True).shape) == (2, 3, 8, 12)
    assert tuple(data.lq_from_gt(gt, 4, degradation='bd').shape) == (2, 3, 8, 12)      # BD: float unless asked
    assert tuple(data.lq_from_gt(gt, 2, quantize=True, degradation='bd').shape) == (2, 3, 16, 24)
    assert tuple(data.lq_from_gt(gt, 4, quantize=False).shape) == (2, 3, 8, 12)
    assert calls == [('bi0.25', (2, 3, 32, 48), 'torch.float32', torch.uint8), ('bi0.25', (2, 3, 32, 48), 'torch.float32', torch.uint8),
                     ('bd4', (2, 3, 32, 48), 'torch.float32', torch.float32), ('bd2', (2, 3, 32, 48), 'torch.float32', torch.uint8),
                     ('bi0.25', (2, 3, 32, 48), 'torch.float32', torch.float32)]
    with pytest.raises(ValueError):
        data.lq_from_gt(gt, 5, degradation='bd')
    # duf_downsample folds (b, t) into the batch of one call
    calls.clear()
    assert tuple(data.duf_downsample(torch.rand(2, 3, 3, 30, 44), scale=3).shape) == (2, 3, 3, 10, 15)
    assert calls == [('bd3', (6, 3, 30, 44), 'torch.float32', torch.float32)]


def _host_read_img_seq(paths, device='cpu', require_mod_crop=False, scale=1, **k):
    from edvr_amd import data as D
    imgs = [D.decode_image(open(p, 'rb').read()) for p in paths]
    if require_mod_crop:
        imgs = [im[:im.shape[0] - im.shape[0] % scale, :im.shape[1] - im.shape[1] % scale] for im in imgs]
    return torch.stack([torch.from_numpy(im.transpose(2, 0, 1).copy()).float() / 255 for im in imgs])


def test_video_clips_options(tmp_path, monkeypatch):
    from edvr_amd import data as D
    spec = dict(folders=['000', '011'], frames=6, lq_hw=(8, 12), scale=4)
    write_video_test_tree(str(tmp_path), spec)
    calls = []
    _patch(monkeypatch, calls)
    monkeypatch.setattr(D, 'read_img_seq', _host_read_img_seq)
    opt = dict(name='REDS4', dataroot_gt=str(tmp_path / 'gt'), dataroot_lq=None, io_backend=dict(type='disk'), cache_data=True, num_frame=5,
               padding='reflection_circle')
    ds = D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'degradation': 'bd'}), device='cpu')
    assert ds.lq_from_gt == {'scale': 4, 'quantize': False, 'degradation': 'bd'}
    lq, gt = ds.clip('011')
    assert tuple(lq.shape) == (6, 3, 8, 12) and tuple(gt.shape) == (6, 3, 32, 48) and calls == [('bd4', (6, 3, 32, 48), 'torch.float32', torch.float32)]
    assert D.VideoTestClips(dict(opt, lq_from_gt={'scale': 4}), device='cpu').lq_from_gt == {'scale': 4, 'quantize': True, 'degradation': 'bi'}
    assert D.VideoTestClips(dict(opt, lq_from_gt={'scale': 2, 'degradation': 'bd', 'quantize': True}), device='cpu').lq_from_gt['quantize'] is True
    for bad in ({'scale': 8, 'degradation': 'bd'}, {'scale': 4, 'degradation': 'gauss'}):
        with pytest.raises(ValueError):
            D.VideoTestClips(dict(opt, lq_from_gt=bad), device='cpu')

    # VideoTestDUFClips: the reference's keys; dataroot_lq names the items only
    calls.clear()
    duf = D.VideoTestDUFClips(dict(opt, dataroot_lq=str(tmp_path / 'BDx4'), use_duf_downsampling=True, scale=4), device='cpu')
    assert duf.lq_from_gt == {'scale': 4, 'quantize': False, 'degradation': 'bd'} and len(duf) == 12 and duf.folders == spec['folders']
    assert duf.data_info['lq_path'][7] == str(tmp_path / 'BDx4' / '011' / '00000001.png')
    assert duf.data_info['gt_path'][7] == str(tmp_path / 'gt' / '011' / '00000001.png')
    plain = D.VideoTestClips(dict(opt, dataroot_lq=str(tmp_path / 'lq')), device='cpu')
    assert duf.data_info['border'] == plain.data_info['border'] and duf.data_info['idx'] == plain.data_info['idx']
    item = duf[7]
    assert tuple(item['lq'].shape) == (5, 3, 8, 12) and tuple(item['gt'].shape) == (3, 32, 48) and item['lq_path'] == duf.data_info['lq_path'][7]
    assert calls == [('bd4', (6, 3, 32, 48), 'torch.float32', torch.float32)]
    lazy = D.VideoTestDUFClips(dict(opt, cache_data=False, use_duf_downsampling=True, scale=2), device='cpu')
    calls.clear()
    item = lazy[0]
    assert tuple(item['lq'].shape) == (5, 3, 16, 24) and calls == [('bd2', (5, 3, 32, 48), 'torch.float32', torch.float32)]
    assert lazy.data_info['lq_path'] == lazy.data_info['gt_path']
    with pytest.raises(ValueError):
        D.VideoTestDUFClips(dict(opt, use_duf_downsampling=True, scale=8), device='cpu')
    # the key false or absent: VideoTestClips on the LQ folder
    calls.clear()
    off = D.VideoTestDUFClips(dict(opt, dataroot_lq=str(tmp_path / 'lq'), use_duf_downsampling=False, scale=4), device='cpu')
    assert off.lq_from_gt is None and off.data_info == plain.data_info and torch.equal(off[3]['lq'], plain[3]['lq']) and calls == []


def test_make_lq_bd(tmp_path, monkeypatch):
    from PIL import Image
    mk = _load('make_lq')
    a = mk.parse_args(['gt', 'lq'])
    assert a.degradation == 'bi' and a.scale == 4
    a = mk.parse_args(['gt', 'lq', '--scale', '3', '--degradation', 'bd'])
    assert a.degradation == 'bd' and a.scale == 3
    for bad in (['gt', 'lq', '--degradation', 'bd', '--scale', '8'], ['gt', 'lq', '--degradation', 'bd', '--scale', '1'],
                ['gt', 'lq', '--degradation', 'xx'], ['gt', 'lq', '--degradation', 'bd', '--no-antialias']):
        with pytest.raises(SystemExit):
            mk.parse_args(bad)
    rng = np.random.default_rng(0)
    gt = tmp_path / 'gt'
    os.makedirs(gt / 'a')
    for f in range(5):
        (gt / 'a' / f'{f:08d}.png').write_bytes(png_bytes(rng.integers(0, 256, (34, 47, 3), dtype=np.uint8)))
    calls = []
    _patch(monkeypatch, calls)
    n = mk.make_lq(str(gt), str(tmp_path / 'lq'), scale=4, batch=3, num_threads=2, device='cpu', log=lambda s: None, degradation='bd')
    # mod-cropped to a multiple of the scale, batches of <= 3 frames, uint8 in and out
    assert n == 5 and calls == [('bd4', (3, 32, 44, 3), 'torch.uint8', torch.uint8), ('bd4', (2, 32, 44, 3), 'torch.uint8', torch.uint8)]
    with Image.open(tmp_path / 'lq' / 'a' / '00000003.png') as im:
        assert im.size == (11, 8) and im.mode == 'RGB'
    calls.clear()
    with pytest.raises(ValueError):  # before any file is read
        mk.make_lq(str(gt), str(tmp_path / 'lq2'), scale=8, device='cpu', degradation='bd')
    with pytest.raises(ValueError):
        mk.make_lq(str(gt), str(tmp_path / 'lq2'), scale=4, device='cpu', degradation='gauss')
    (gt / 'tiny').mkdir()
    (gt / 'tiny' / '0.png').write_bytes(png_bytes(np.zeros((6, 48, 3), np.uint8)))
    with pytest.raises(ValueError):  # 6 rows: refused before the device call
        mk.make_lq(str(gt / '..' / 'gt'), str(tmp_path / 'lq3'), scale=2, device='cpu', log=lambda s: None, degradation='bd')
    assert all(c[1][1] != 6 for c in calls)


def test_eval_video_bd(tmp_path, monkeypatch):
    import json

    import edvr_amd
    from edvr_amd import data as D, metrics as M
    ev = _load('eval_video')
    a = ev.parse_args(['--gt', 'g', '--lq-from-gt', '4'])
    assert a.degradation == 'bi'
    a = ev.parse_args(['--gt', 'g', '--lq-from-gt', '4', '--degradation', 'bd', '--bicubic-baseline'])
    assert a.degradation == 'bd' and a.lq_from_gt == 4 and a.bicubic_baseline
    for bad in (['--gt', 'g', '--lq-from-gt', '8', '--degradation', 'bd'], ['--gt', 'g', '--lq', 'l', '--degradation', 'bd'],
                ['--gt', 'g', '--lq-from-gt', '4', '--degradation', 'xx']):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)

    spec = dict(folders=['000', '011'], frames=6, lq_hw=(8, 12), scale=4)
    write_video_test_tree(str(tmp_path), spec)

    class Net(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return torch.nn.functional.interpolate(x[:, x.shape[1] // 2], scale_factor=4, mode='bilinear', align_corners=False)

        def to(self, device):
            return self

    def psnr(a, b, crop_border=0, test_y_channel=False):
        return [float(10 * torch.log10(1 / ((x - t) ** 2).mean())) for x, t in zip(a, b)]

    def validate_video(net, lq, gt=None, num_frame=5, padding='reflection_circle', chunk=8, crop_border=0, test_y_channel=False):
        return M.validate_clip(net, lq, gt, num_frame=num_frame, padding=padding, batch=chunk, crop_border=crop_border, test_y_channel=test_y_channel)

    calls = []
    _patch(monkeypatch, calls)
    monkeypatch.setattr(edvr_amd, 'EDVR', Net)
    monkeypatch.setattr(D, 'read_img_seq', _host_read_img_seq)
    monkeypatch.setattr(M, 'calculate_psnr', psnr)
    monkeypatch.setattr(M, 'validate_video', validate_video)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    out = tmp_path / 'r.json'
    args = argparse.Namespace(lq=None, lq_from_gt=4, degradation='bd', bicubic_baseline=True, json=str(out), gt=str(tmp_path / 'gt'), weights=None,
                              name='REDS4', num_feat=64, num_reconstruct_block=2, num_frame=5, hr_in=False, with_predeblur=False, no_tsa=False,
                              padding='reflection', crop_border=0, test_y_channel=False, batch=4)
    lines = []
    summary = ev.evaluate(args, log=lines.append)
    assert list(summary) == spec['folders'] and len(lines) == 3 and all('(bicubic ' in s for s in lines)
    # per folder: one BD reduction of the whole GT clip (float, not quantised), then the bicubic x4 enlargement of the LQ frames
    assert [c for c in calls if c[0].startswith('bd')] == [('bd4', (6, 3, 32, 48), 'torch.float32', torch.float32)] * 2
    assert [c for c in calls if c[0].startswith('bi')] == [('bi4', (4, 3, 8, 12), 'torch.float32', torch.float32),
                                                            ('bi4', (2, 3, 8, 12), 'torch.float32', torch.float32)] * 2
    record = json.loads(out.read_text())
    assert record['degradation'] == 'bd' and record['psnr'] == summary and np.isfinite(record['bicubic_average'])
    # bi stays the default and is recorded; an LQ folder's degradation is unknown
    ev.evaluate(argparse.Namespace(**{**vars(args), 'degradation': 'bi'}), log=lines.append)
    assert json.loads(out.read_text())['degradation'] == 'bi'
    ev.evaluate(argparse.Namespace(**{**vars(args), 'lq': str(tmp_path / 'lq'), 'lq_from_gt': None}), log=lines.append)
    assert json.loads(out.read_text())['degradation'] is None
