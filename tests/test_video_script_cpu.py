"""CPU: control flow of scripts/eval_video.py (the feature-reusing evaluation of folder datasets) with CPU stand-ins for the GPU-only
pieces, as tests/test_scripts_cpu.py does for scripts/test_reds.py: it hands every clip to metrics.validate_video with --batch as the
chunk and reports what scripts/test_reds.py reports."""
import argparse
import importlib.util
import os

import torch

from util_data import write_video_test_tree


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_video_evaluation_script_flow(tmp_path, monkeypatch):
    import edvr_amd
    from edvr_amd import data as D, metrics as M
    spec = dict(folders=['000', '011'], frames=7, lq_hw=(8, 12), scale=4)
    write_video_test_tree(str(tmp_path), spec)

    class Net(torch.nn.Module):  # "restores" by bilinear x4 of the centre frame
        def __init__(self, *a, **k):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return torch.nn.functional.interpolate(x[:, x.shape[1] // 2], scale_factor=4, mode='bilinear', align_corners=False)

        def to(self, device):
            return self

    def read_img_seq(paths, device='cpu', **k):
        return torch.stack([torch.from_numpy(D.decode_image(open(p, 'rb').read()).transpose(2, 0, 1).copy()).float() / 255 for p in paths])

    def psnr(a, b, crop_border=0, test_y_channel=False):
        return [float(10 * torch.log10(1 / ((x - t) ** 2).mean())) for x, t in zip(a, b)]

    calls = []

    def validate_video(net, lq, gt=None, num_frame=5, padding='reflection_circle', chunk=8, crop_border=0, test_y_channel=False):
        calls.append((lq.shape[0], num_frame, padding, chunk))
        return M.validate_clip(net, lq, gt, num_frame=num_frame, padding=padding, batch=chunk, crop_border=crop_border, test_y_channel=test_y_channel)

    monkeypatch.setattr(edvr_amd, 'EDVR', Net)
    monkeypatch.setattr(D, 'read_img_seq', read_img_seq)
    monkeypatch.setattr(M, 'calculate_psnr', psnr)
    monkeypatch.setattr(M, 'validate_video', validate_video)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    args = argparse.Namespace(lq=str(tmp_path / 'lq'), gt=str(tmp_path / 'gt'), weights=None, name='REDS4', vimeo_meta=None, num_feat=64,
                              num_reconstruct_block=2, num_frame=5, hr_in=False, with_predeblur=False, no_tsa=False,
                              padding='reflection', crop_border=0, test_y_channel=False, batch=3)
    lines = []
    summary = _load('eval_video').evaluate(args, log=lines.append)
    assert calls == [(7, 5, 'reflection', 3)] * 2  # every clip whole, --batch as the chunk
    assert list(summary) == spec['folders'] and lines[-1].startswith('average over 2 folder(s)')
    windowed = _load('test_reds').evaluate(args, log=lambda s: None)
    assert summary == windowed
