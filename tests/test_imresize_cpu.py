"""CPU: the host side of the bicubic imresize feature - imresize_shape and its refusals, the fixture file, and the argument handling and
folder walking of scripts/make_lq.py and scripts/eval_video.py with the device call replaced by a stand-in (as
tests/test_video_script_cpu.py does)."""
import argparse
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from util_data import png_bytes, write_video_test_tree
from util_imresize import FIXTURE_CASES, GOLDEN, imresize_f64, load_golden


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_file_is_whole():
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    cases = load_golden()
    assert len(cases) == len(FIXTURE_CASES)
    for case, ((h, w), scale) in zip(cases, FIXTURE_CASES):
        assert case['input'].dtype == torch.uint8 and tuple(case['input'].shape) == (h, w, 3) and h <= 64 and w <= 96
        assert case['scale'] == scale and case['antialiasing'] is True
        out = case['output']
        assert out.dtype == torch.float32 and tuple(out.shape) == (3, math.ceil(h * scale), math.ceil(w * scale)) and bool(torch.isfinite(out).all())
        # the reference's output is the formula's: the float64 restatement the GPU test also uses sits within the reference's own rounding
        x = (case['input'].float() / 255).permute(2, 0, 1)
        assert (imresize_f64(x, scale, True) - out.double()).abs().max().item() < 2e-6


def test_imresize_shape_gives_the_fixture_shapes():
    import edvr_amd
    from edvr_amd import data
    assert edvr_amd.imresize is data.imresize and edvr_amd.imresize_shape is data.imresize_shape
    for case, ((h, w), scale) in zip(load_golden(), FIXTURE_CASES):
        assert data.imresize_shape(h, w, scale) == tuple(case['output'].shape[1:])
        assert data.imresize_shape(h, w, scale, antialiasing=False) == tuple(case['output'].shape[1:])
    assert data.imresize_shape(2880, 5120, 1 / 4) == (720, 1280) and data.imresize_shape(180, 320, 4) == (720, 1280)
    assert data.imresize_shape(37, 53, 1 / 4) == (10, 14) and data.imresize_shape(50, 70, 0.3) == (15, 21)
    assert data.imresize_shape(64, 96, 1 / 8) == (8, 12) and data.imresize_shape(2, 2, 8) == (16, 16)


def test_imresize_shape_refusals():
    from edvr_amd.data import imresize_shape
    for h, w, scale, aa in ((64, 96, 1 / 16, True), (64, 96, 8.5, True), (64, 96, 0, True), (64, 96, -1, True),
                            (5, 96, 1 / 4, True), (64, 5, 1 / 4, True), (1, 1, 4, True), (0, 8, 2, True), (11, 64, 1 / 8, True)):
        with pytest.raises(ValueError):
            imresize_shape(h, w, scale, aa)
    # the reach follows the formula: at x4 antialiased reduction 6 samples before the frame and 8 after the last of 2 outputs (12 and 16
    # at x8), 2 at any enlargement and without antialiasing
    assert imresize_shape(8, 8, 1 / 4) == (2, 2) and imresize_shape(16, 16, 1 / 8) == (2, 2) and imresize_shape(2, 2, 4) == (8, 8)
    for n in (5, 6):
        with pytest.raises(ValueError):
            imresize_shape(n, 64, 1 / 4)
    assert imresize_shape(5, 5, 1 / 4, antialiasing=False) == (2, 2)
    with pytest.raises(ValueError):
        imresize_shape(5, 5, 1 / 4, antialiasing=True)


def test_cpu_tensors_raise():
    from edvr_amd import data, ops
    with pytest.raises(NotImplementedError):
        data.imresize(torch.rand(3, 32, 32), 1 / 4)
    with pytest.raises(NotImplementedError):
        ops.imresize(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), 1 / 4, out_dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        data.imresize(np.zeros((32, 32, 3), np.float32), 1 / 4)


def _stand_in(calls):
    """ops.imresize on the host for the script tests: box-free nearest sampling of the right SHAPE, recording its arguments."""
    def imresize(frames, scale, antialiasing=True, out_dtype=torch.float32):
        from edvr_amd.data import imresize_shape
        u8 = frames.dtype == torch.uint8
        x = frames.permute(0, 3, 1, 2).float() / 255 if u8 else frames.float()
        ho, wo = imresize_shape(x.shape[-2], x.shape[-1], scale, antialiasing)
        calls.append((tuple(frames.shape), str(frames.dtype), float(scale), bool(antialiasing), out_dtype))
        out = torch.nn.functional.interpolate(x, size=(ho, wo), mode='nearest')
        return (out.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous() if out_dtype == torch.uint8 else out
    return imresize


def test_make_lq_walks_the_tree(tmp_path, monkeypatch):
    from PIL import Image
    from edvr_amd import ops
    mk = _load('make_lq')
    rng = np.random.default_rng(0)
    gt = tmp_path / 'gt'
    sizes = {'a': (34, 47), 'b': (32, 48)}
    for clip, hw in sizes.items():
        os.makedirs(gt / clip)
        for f in range(5):
            (gt / clip / f'{f:08d}.png').write_bytes(png_bytes(rng.integers(0, 256, hw + (3,), dtype=np.uint8)))
        (gt / clip / '.hidden').write_text('x')
        (gt / clip / 'notes.txt').write_text('x')
    os.makedirs(gt / 'empty')
    (gt / 'stray.png').write_bytes(b'')
    assert mk.walk(str(gt)) == [('a', [f'{f:08d}.png' for f in range(5)]), ('b', [f'{f:08d}.png' for f in range(5)])]
    calls = []
    monkeypatch.setattr(ops, 'imresize', _stand_in(calls))
    lines = []
    n = mk.make_lq(str(gt), str(tmp_path / 'lq'), scale=4, antialiasing=False, batch=3, num_threads=2, device='cpu', log=lines.append)
    assert n == 10 and lines == ['a: 5 frame(s)', 'b: 5 frame(s)']
    # mod-cropped to a multiple of the scale, batches of <= 3 frames, uint8 in and out, 1 / scale, the antialiasing flag passed on
    assert calls == [((3, 32, 44, 3), 'torch.uint8', 0.25, False, torch.uint8), ((2, 32, 44, 3), 'torch.uint8', 0.25, False, torch.uint8),
                     ((3, 32, 48, 3), 'torch.uint8', 0.25, False, torch.uint8), ((2, 32, 48, 3), 'torch.uint8', 0.25, False, torch.uint8)]
    for clip, (h, w) in sizes.items():
        assert sorted(os.listdir(tmp_path / 'lq' / clip)) == [f'{f:08d}.png' for f in range(5)]
        with Image.open(tmp_path / 'lq' / clip / '00000003.png') as im:
            assert im.size == (w // 4, h // 4) and im.mode == 'RGB'
    with pytest.raises(FileNotFoundError):
        mk.make_lq(str(tmp_path / 'lq' / 'a'), str(tmp_path / 'x'), device='cpu')
    (gt / 'tiny').mkdir()
    (gt / 'tiny' / '0.png').write_bytes(png_bytes(np.zeros((6, 48, 3), np.uint8)))
    with pytest.raises(ValueError):  # 4 rows (6 mod-cropped) are fewer than the x4 antialiased kernel reaches: refused before the device call
        mk.make_lq(str(gt), str(tmp_path / 'lq2'), scale=4, device='cpu', log=lambda s: None)
    assert all(c[0][1] != 4 for c in calls)


def test_make_lq_arguments():
    mk = _load('make_lq')
    a = mk.parse_args(['gt', 'lq'])
    assert (a.gt_root, a.lq_root, a.scale, a.no_antialias) == ('gt', 'lq', 4, False)
    a = mk.parse_args(['gt', 'lq', '--scale', '2', '--no-antialias'])
    assert a.scale == 2 and a.no_antialias
    for bad in (['gt'], ['gt', 'lq', '--scale', '16'], ['gt', 'lq', '--scale', '0']):
        with pytest.raises(SystemExit):
            mk.parse_args(bad)


def test_eval_video_arguments():
    ev = _load('eval_video')
    a = ev.parse_args(['--gt', 'g', '--lq', 'l'])
    assert a.lq == 'l' and a.lq_from_gt is None and not a.bicubic_baseline
    a = ev.parse_args(['--gt', 'g', '--lq-from-gt', '4', '--bicubic-baseline', '--json', 'r.json'])
    assert a.lq is None and a.lq_from_gt == 4 and a.bicubic_baseline and a.json == 'r.json'
    for bad in (['--gt', 'g'], ['--gt', 'g', '--lq-from-gt', '16'], ['--lq', 'l']):
        with pytest.raises(SystemExit):  # neither --lq nor --lq-from-gt is still an argparse error
            ev.parse_args(bad)


def test_eval_video_from_gt_with_baseline(tmp_path, monkeypatch):
    import json

    import edvr_amd
    from edvr_amd import data as D, metrics as M, ops
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

    def read_img_seq(paths, device='cpu', require_mod_crop=False, scale=1, **k):
        imgs = [D.decode_image(open(p, 'rb').read()) for p in paths]
        if require_mod_crop:
            imgs = [im[:im.shape[0] - im.shape[0] % scale, :im.shape[1] - im.shape[1] % scale] for im in imgs]
        return torch.stack([torch.from_numpy(im.transpose(2, 0, 1).copy()).float() / 255 for im in imgs])

    def psnr(a, b, crop_border=0, test_y_channel=False):
        return [float(10 * torch.log10(1 / ((x - t) ** 2).mean())) for x, t in zip(a, b)]

    def validate_video(net, lq, gt=None, num_frame=5, padding='reflection_circle', chunk=8, crop_border=0, test_y_channel=False):
        return M.validate_clip(net, lq, gt, num_frame=num_frame, padding=padding, batch=chunk, crop_border=crop_border, test_y_channel=test_y_channel)

    calls = []
    monkeypatch.setattr(edvr_amd, 'EDVR', Net)
    monkeypatch.setattr(D, 'read_img_seq', read_img_seq)
    monkeypatch.setattr(M, 'calculate_psnr', psnr)
    monkeypatch.setattr(M, 'validate_video', validate_video)
    monkeypatch.setattr(ops, 'imresize', _stand_in(calls))
    monkeypatch.setattr(ops, 'frames_u8_to_f32', lambda u8: u8.permute(0, 1, 4, 2, 3).float() / 255)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    out = tmp_path / 'r.json'
    args = argparse.Namespace(lq=None, lq_from_gt=4, bicubic_baseline=True, json=str(out), gt=str(tmp_path / 'gt'), weights=None, name='REDS4',
                              num_feat=64, num_reconstruct_block=2, num_frame=5, hr_in=False, with_predeblur=False, no_tsa=False,
                              padding='reflection', crop_border=0, test_y_channel=False, batch=4)
    lines = []
    summary = _load('eval_video').evaluate(args, log=lines.append)
    assert list(summary) == spec['folders'] and len(lines) == 3
    # per folder: one reduction of the whole GT clip to 8-bit LQ frames, then the x4 enlargement of the LQ frames in chunks of --batch
    down = [c for c in calls if c[2] == 0.25]
    up = [c for c in calls if c[2] == 4.0]
    assert down == [((6, 3, 32, 48), 'torch.float32', 0.25, True, torch.uint8)] * 2
    assert up == [((4, 3, 8, 12), 'torch.float32', 4.0, True, torch.float32), ((2, 3, 8, 12), 'torch.float32', 4.0, True, torch.float32)] * 2
    record = json.loads(out.read_text())
    assert record['psnr'] == summary and sorted(record['bicubic_psnr']) == spec['folders']
    for folder, line in zip(spec['folders'], lines):
        assert line == f'{folder}: PSNR {summary[folder]:.4f} dB (bicubic {record["bicubic_psnr"][folder]:.4f} dB)'
    assert lines[-1] == f'average over 2 folder(s): {record["average"]:.4f} dB (bicubic {record["bicubic_average"]:.4f} dB)'
    # without the new options nothing is added to the lines
    plain = argparse.Namespace(**{**vars(args), 'lq': str(tmp_path / 'lq'), 'lq_from_gt': None, 'bicubic_baseline': False, 'json': None})
    lines2 = []
    _load('eval_video').evaluate(plain, log=lines2.append)
    assert all('bicubic' not in s for s in lines2) and len(lines2) == 3
    with pytest.raises(ValueError):
        _load('eval_video').evaluate(argparse.Namespace(**{**vars(plain), 'lq': None}), log=lines2.append)
