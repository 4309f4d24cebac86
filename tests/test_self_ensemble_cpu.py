"""CPU: self-ensemble on the whole-video path (edvr_amd/video.py: self_ensemble) - the (tile x element) schedule with CPU stand-ins for
the device primitives and a stub network, the argument errors, the index map the kernels of csrc/ensemble.hip implement against the
definition, and scripts/eval_video.py's flag."""
import argparse
import importlib.util
import os
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

from util_data import write_video_test_tree


def _g(x, k):
    """The definition, spelled out: k = 4 t + 2 v + h; transpose if t, then flip rows if v, then flip columns if h."""
    t, v, h = k >> 2 & 1, k >> 1 & 1, k & 1
    if t:
        x = x.transpose(-1, -2)
    if v:
        x = x.flip(-2)
    if h:
        x = x.flip(-1)
    return x


def _g_inv(y, k):
    t, v, h = k >> 2 & 1, k >> 1 & 1, k & 1
    if h:
        y = y.flip(-1)
    if v:
        y = y.flip(-2)
    if t:
        y = y.transpose(-1, -2)
    return y


# ------------------------------------------------------------------------------------------------ the index map
@pytest.mark.parametrize('k', range(8))
def test_index_map_is_the_inverse_pair_of_the_definition(k):
    from edvr_amd import ops
    x = torch.arange(15).view(3, 5)
    g = _g(x, k)
    R, C = g.shape
    assert (R, C) == ((5, 3) if k & 4 else (3, 5))
    assert torch.equal(ops.d4_apply(x, k), g) and torch.equal(ops.d4_invert(g, k), x) and torch.equal(_g_inv(g, k), x)
    y = torch.arange(100, 115).view(R, C)  # any image of the transformed shape
    back = _g_inv(y, k)
    assert torch.equal(ops.d4_invert(y, k), back) and tuple(back.shape) == (3, 5)
    seen = set()
    for r in range(3):
        for q in range(5):
            i, j = ops.d4_index(k, r, q, R, C)
            assert 0 <= i < R and 0 <= j < C
            assert g[i, j] == x[r, q]        # the oriented read: g_k(x)[i][j] = x[r][q]
            assert back[r, q] == y[i, j]     # the oriented tail: g_k^-1(y)[r][q] = y[i][j]
            seen.add((i, j))
    assert len(seen) == 15                   # a bijection
    for bad in (8, -1, 1.5):
        with pytest.raises(ValueError):
            ops.d4_index(bad, 0, 0, 3, 5)


# ------------------------------------------------------------------------------------------------ arguments
def test_ensemble_elements_and_argument_errors():
    from edvr_amd import ensemble_elements
    assert ensemble_elements(None) is None
    assert ensemble_elements('flip4') == (0, 1, 2, 3) and ensemble_elements('d4') == tuple(range(8))
    assert ensemble_elements([5, 0, 2]) == (5, 0, 2) and ensemble_elements((7,)) == (7,)
    for bad in ('d8', 'flip', '', (), [], (0, 0), (1, 2, 1), (8,), (-1,), (0, 1.5), (True,), 3):
        with pytest.raises(ValueError):
            ensemble_elements(bad)
    net, _ = _stub_restorer(5, 'replicate', 4)
    from edvr_amd import VideoRestorer
    for bad in ('rot', (), (3, 3), (9,)):
        with pytest.raises(ValueError):
            VideoRestorer(net, num_frame=5, self_ensemble=bad)
    assert VideoRestorer(net, num_frame=5).tiled is False
    vr = VideoRestorer(net, num_frame=5, self_ensemble='flip4')
    assert vr.tiled and vr.elements == (0, 1, 2, 3)  # the ensemble turns the tiled path on, as pad_mode / tile do


# ------------------------------------------------------------------------------------------------ the schedule
class _StubNet(torch.nn.Module):
    """"Features" = (frame index, tile origin and element); the "restored" tile = the oriented crop, enlarged."""

    def __init__(self, num_frame):
        super().__init__()
        self.conv_l2_1 = torch.nn.Conv2d(2, 2, 3, 2, 1)
        self.hr_in = self.with_predeblur = False
        self.center_frame_idx = num_frame // 2
        self.extracted, self.extract_calls, self.restores, self.restorer = [], [], [], None

    def check_offsets(self, wait=True):
        pass

    def extract_features(self, frames, out=None):
        code = self.restorer.current  # (tile origin y, x, element) of the crop handed in
        assert tuple(frames.shape[2:]) == self.restorer.oriented_shape(code[2])
        for i in range(frames.shape[0]):
            self.extracted.append((int(frames[i, 0, 0, 0]),) + code)
        self.extract_calls.append(code)
        for o in out:
            assert o.shape[0] == frames.shape[0]
            o[:, 0] = frames[:, 0, :1, :1]
            o[:, 1] = float((code[0] * 100 + code[1]) * 10 + code[2])
        return list(out)

    def restore_from_features(self, pyr, x_center, b, t, out_dtype=torch.float32, out=None, keep=None, elem=None, accumulate='only', scale=1.0,
                              acc=None):
        assert all(f.shape[0] == b * t for f in pyr) and x_center.shape[0] == b and acc is None
        code = self.restorer.current
        assert code[2] == elem
        for f in pyr:  # every image of the window comes from this (tile, element) pair's own bank
            assert bool((f[:, 1, 0, 0] == (code[0] * 100 + code[1]) * 10 + elem).all())
        rows = pyr[0][:, 0, 0, 0].view(b, t).to(torch.int64).tolist()
        self.restores.append((code[0], code[1], elem, accumulate, rows))
        value = _g_inv(x_center.repeat_interleave(4, 2).repeat_interleave(4, 3), elem)
        ky, kx = keep
        value = value[:, :, ky:ky + out.shape[2], kx:kx + out.shape[3]]
        assert value.shape == out.shape
        if accumulate in ('first', 'only'):
            out.copy_(value)      # (the accumulator is not read by the first element: the output starts as torch.empty)
        else:
            out.add_(value)
        if accumulate in ('last', 'only'):
            out.mul_(scale)
        return out


def _stub_restorer(num_frame, padding, chunk, **kw):
    from edvr_amd import VideoRestorer

    class CpuRestorer(VideoRestorer):  # CPU stand-ins for the device primitives
        current = None

        def _check_input(self, t):
            pass

        def _slot_table(self, slots, device):
            return torch.tensor(slots, dtype=torch.int32)

        def _gather(self, srcs, table):
            return [s[table.long()] for s in srcs]

        def _crop(self, frames, y0, x0, th, tw):
            H, W = frames.shape[2:]
            x = F.pad(frames, (0, max(x0 + tw - W, 0), 0, max(y0 + th - H, 0)), mode=self.pad_mode) if self.pad_mode else frames
            return x[:, :, y0:y0 + th, x0:x0 + tw].contiguous()

        def _crop_d4(self, frames, y0, x0, th, tw, elem):
            self.current = (y0, x0, elem)
            return _g(self._crop(frames, y0, x0, th, tw), elem).contiguous()

        def oriented_shape(self, elem):
            th, tw = self.grid[0].src[2:]
            return (tw, th) if elem & 4 else (th, tw)

    net = _StubNet(num_frame).eval()
    vr = CpuRestorer(net, num_frame=num_frame, padding=padding, chunk=chunk, **kw)
    net.restorer = vr
    return net, vr


def _coded_frames(n, H, W):
    f = torch.empty(n, 3, H, W)
    f[:, 0] = torch.arange(n, dtype=torch.float32).view(n, 1, 1)
    f[:, 1] = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    f[:, 2] = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    return f


MODES = {1: ['only'], 2: ['first', 'last'], 3: ['first', 'middle', 'last'], 4: ['first', 'middle', 'middle', 'last']}


@pytest.mark.parametrize('ensemble', [(5, 0, 2), 'flip4', (3,), (6, 1)])
@pytest.mark.parametrize('tiles', [True, False])
def test_ensemble_schedule(ensemble, tiles):
    from edvr_amd import ensemble_elements, tile_grid, window_table
    t, n, chunk, (H, W) = 5, 9, 4, (22, 30)  # padded to 24 x 32; tiles (16, 16), overlap 8: 2 x 3 tiles
    kw = dict(tile=(16, 16), tile_overlap=8) if tiles else {}
    net, vr = _stub_restorer(t, 'reflection_circle', chunk, pad_mode='replicate', self_ensemble=ensemble, **kw)
    elements = ensemble_elements(ensemble)
    grid = tile_grid(H, W, kw.get('tile'), kw.get('tile_overlap'), 4)
    assert len(grid) == (6 if tiles else 1)
    pairs = [(tl.src[0], tl.src[1], k) for tl in grid for k in elements]  # the documented order: tile x element, element innermost
    frames = _coded_frames(n, H, W)
    peak = []
    with torch.no_grad():
        outs = []
        for out in vr.restore_chunks(iter(frames.unbind(0))):
            outs.append(out)
            peak.append((vr.bank_frames, len(vr.banks)))
    assert [o.shape[0] for o in outs] == [4, 4, 1]
    assert [(tl.src[0], tl.src[1], k) for tl, k in vr.pairs] == pairs and all(b == len(pairs) for _, b in peak)  # one bank per pair
    assert max(f for f, _ in peak) <= vr.slots <= vr.capacity <= chunk + 2 * (t - 1)
    # the output: the stub's result is the enlarged crop, so the average of the un-transformed results is the enlarged frame
    want = frames.repeat_interleave(4, 2).repeat_interleave(4, 3)
    acc = want.clone()
    for _ in elements[1:]:
        acc = acc + want
    want = acc * (1.0 / len(elements))
    assert torch.equal(torch.cat(outs, 0), want)
    # every (frame, tile, element) through the per-frame stage exactly once
    assert Counter(net.extracted) == Counter((f,) + p for f in range(n) for p in pairs)
    # ... pair by pair in the documented order within every extract step (a group crossing the end of the ring is two calls)
    calls = [c for i, c in enumerate(net.extract_calls) if i == 0 or c != net.extract_calls[i - 1] or len(pairs) == 1]
    if len(pairs) > 1:
        assert len(calls) % len(pairs) == 0 and calls == pairs * (len(calls) // len(pairs))
    # every restore step: pair by pair in that order, the accumulate modes first / middle ... / last per tile, every pair on its windows
    table = window_table(n, t, 'reflection_circle').tolist()
    assert len(net.restores) == len(pairs) * len(outs)
    modes = MODES[len(elements)]
    first = 0
    for c, out in enumerate(outs):
        step = net.restores[c * len(pairs):(c + 1) * len(pairs)]
        assert [(y, x, k) for y, x, k, _, _ in step] == pairs
        assert [m for _, _, _, m, _ in step] == modes * len(grid)
        assert all(rows == table[first:first + out.shape[0]] for *_, rows in step)
        first += out.shape[0]


def test_no_ensemble_calls_the_primitives_as_before():
    """self_ensemble=None: _crop with five arguments, restore_from_features without the new keywords (tests/test_video_tiles_cpu.py's stubs)."""
    net, vr = _stub_restorer(5, 'replicate', 4, pad_mode='replicate')
    seen = []

    def plain(pyr, x_center, b, t, out_dtype=torch.float32, out=None, keep=None):
        seen.append(keep)
        out.copy_(x_center.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :out.shape[2], :out.shape[3]])
        return out

    def extract(frames, out=None):
        return list(out)

    net.restore_from_features, net.extract_features = plain, extract
    vr._crop_d4 = None
    frames = _coded_frames(6, 22, 30)
    with torch.no_grad():
        out = torch.cat(list(vr.restore_chunks([frames])), 0)
    assert seen == [(0, 0), (0, 0)] and vr.pairs == [(vr.grid[0], None)]
    assert torch.equal(out, frames.repeat_interleave(4, 2).repeat_interleave(4, 3))


# ------------------------------------------------------------------------------------------------ scripts/eval_video.py
def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_video_parser_accepts_the_flag():
    ev = _load('eval_video')
    assert ev.parse_args(['--gt', 'g', '--lq', 'l']).self_ensemble is None
    for name in ('flip4', 'd4'):
        assert ev.parse_args(['--gt', 'g', '--lq', 'l', '--self-ensemble', name]).self_ensemble == name
    with pytest.raises(SystemExit):
        ev.parse_args(['--gt', 'g', '--lq', 'l', '--self-ensemble', 'rot8'])


def test_eval_video_reports_plain_and_ensemble_side_by_side(tmp_path, monkeypatch):
    import edvr_amd
    from edvr_amd import data as D, metrics as M
    spec = dict(folders=['000', '011'], frames=7, lq_hw=(8, 12), scale=4)
    write_video_test_tree(str(tmp_path), spec)

    class Net(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def to(self, device):
            return self

    def read_img_seq(paths, device='cpu', **k):
        return torch.stack([torch.from_numpy(D.decode_image(open(p, 'rb').read()).transpose(2, 0, 1).copy()).float() / 255 for p in paths])

    calls = []

    def validate_video(net, lq, gt=None, num_frame=5, padding='reflection_circle', chunk=8, crop_border=0, test_y_channel=False, self_ensemble=None):
        calls.append(self_ensemble)
        return None, [30.0 if self_ensemble is None else 31.0] * lq.shape[0]

    monkeypatch.setattr(edvr_amd, 'EDVR', Net)
    monkeypatch.setattr(D, 'read_img_seq', read_img_seq)
    monkeypatch.setattr(M, 'validate_video', validate_video)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    out_json = tmp_path / 'r.json'
    args = argparse.Namespace(lq=str(tmp_path / 'lq'), gt=str(tmp_path / 'gt'), weights=None, name='REDS4', num_feat=64, num_reconstruct_block=2,
                              num_frame=5, hr_in=False, with_predeblur=False, no_tsa=False, padding='reflection', crop_border=0,
                              test_y_channel=False, batch=3, self_ensemble='flip4', json=str(out_json))
    lines = []
    summary = _load('eval_video').evaluate(args, log=lines.append)
    assert calls == [None, 'flip4'] * 2                       # every clip: the plain pass, then the ensemble
    assert summary == {'000': 30.0, '011': 30.0}              # the return value stays the plain result
    assert all('30.0000 dB' in ln and 'self-ensemble flip4 31.0000 dB' in ln for ln in lines) and len(lines) == 3
    import json
    rec = json.load(open(out_json))
    assert rec['self_ensemble'] == 'flip4' and rec['self_ensemble_average'] == 31.0 and rec['average'] == 30.0
