"""CPU: temporal-reversal self-ensemble on the whole-video path (edvr_amd/video.py: time_reverse) - the window symmetry the shared
alignment rests on, the argument errors, the schedule of both arms with CPU stand-ins for the device primitives and a stub network,
and the flags of scripts/eval_video.py and scripts/bench_video.py."""
import argparse
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from util_data import write_video_test_tree

PADDINGS = ('replicate', 'reflection', 'reflection_circle', 'circle')


# ------------------------------------------------------------------------------------------------ the fact the sharing rests on
@pytest.mark.parametrize('padding', PADDINGS)
@pytest.mark.parametrize('t', [3, 5, 7])
def test_window_of_the_reversed_video_is_the_reversed_window(padding, t):
    """Output frame i of the forward video is output frame N - 1 - i of the reversed one, and frame f is frame N - 1 - f there: the
    reversed video's table, mapped back to forward frame numbers and forward output order, is the forward table with every row reversed."""
    from edvr_amd import window_table
    legal = []
    for n in range(1, 13):
        try:
            table = window_table(n, t, padding)
        except ValueError:
            assert not legal, f'{n} frames are too short although {legal[-1]} are not'
            continue
        legal.append(n)
        assert torch.equal((n - 1) - table.flip(0).flip(1), table), (padding, t, n)
    assert legal and legal[-1] == 12 and legal[0] <= 2 * t


# ------------------------------------------------------------------------------------------------ stubs
def _g_inv(y, k):
    t, v, h = k >> 2 & 1, k >> 1 & 1, k & 1
    if h:
        y = y.flip(-1)
    if v:
        y = y.flip(-2)
    if t:
        y = y.transpose(-1, -2)
    return y


def _g(x, k):
    t, v, h = k >> 2 & 1, k >> 1 & 1, k & 1
    if t:
        x = x.transpose(-1, -2)
    if v:
        x = x.flip(-2)
    if h:
        x = x.flip(-1)
    return x


class _StubNet(torch.nn.Module):
    """"Features" = (frame index, code of the (tile, element) pair); the "restored" tile = the oriented crop, enlarged.  Every call of
    the three entry points VideoRestorer uses is logged."""

    def __init__(self, num_frame):
        super().__init__()
        self.conv_l2_1 = torch.nn.Conv2d(2, 2, 3, 2, 1)
        self.hr_in = self.with_predeblur = False
        self.center_frame_idx = num_frame // 2
        self.log, self.restorer = [], None

    def check_offsets(self, wait=True):
        pass

    def _code(self):
        y0, x0, k = self.restorer.current
        return float((y0 * 100 + x0) * 10 + (0 if k is None else k))

    def extract_features(self, frames, out=None):
        for o in out:
            o[:, 0] = frames[:, 0, :1, :1]
            o[:, 1] = self._code()
        return list(out)

    def _rows(self, pyr, b, t):
        for f in pyr:  # every image of the window comes from this (tile, element) pair's own bank
            assert f.shape[0] == b * t and bool((f[:, 1, 0, 0] == self._code()).all())
        return pyr[0][:, 0, 0, 0].view(b, t).to(torch.int64)

    def align_windows(self, pyr, b, t, pair=False):
        rows = self._rows(pyr, b, t)
        self.log.append(('align', self.restorer.current, pair, rows.tolist()))
        return (rows, rows.flip(1), ['stats']) if pair else (rows, ['stats'])

    def restore_from_aligned(self, operand, x_center, b, t, out_dtype=torch.float32, out=None, keep=None, elem=None, accumulate='only', scale=1.0,
                             acc=None, bands=None, sink=None):
        assert x_center.shape[0] == b and acc is None and bands is None and out_dtype == torch.float32
        self.log.append(('tail', self.restorer.current, elem, accumulate, scale, operand.tolist(), sink is not None))
        value = _g_inv(x_center.repeat_interleave(4, 2).repeat_interleave(4, 3), elem)
        ky, kx = keep
        value = value[:, :, ky:ky + out.shape[2], kx:kx + out.shape[3]]
        assert value.shape == out.shape
        if accumulate in ('first', 'only'):
            out.copy_(value)      # (the accumulator is not read by the first term: the output starts as torch.empty)
        else:
            out.add_(value)
        if accumulate in ('last', 'only'):
            out.mul_(scale)
        return out

    def restore_from_features(self, pyr, x_center, b, t, **how):
        operand, sink = self.align_windows(pyr, b, t)
        return self.restore_from_aligned(operand, x_center, b, t, sink=sink, **how)


def _stub_restorer(num_frame, padding, chunk, **kw):
    from edvr_amd import VideoRestorer

    class CpuRestorer(VideoRestorer):  # CPU stand-ins for the device primitives
        current = None

        def _check_input(self, t):
            pass

        def _slot_table(self, slots, device):
            return torch.tensor(slots, dtype=torch.int32)

        def _gather(self, srcs, table):
            self.net.log.append(('gather', table.tolist()))
            return [s[table.long()] for s in srcs]

        def _crop(self, frames, y0, x0, th, tw):
            H, W = frames.shape[2:]
            x = F.pad(frames, (0, max(x0 + tw - W, 0), 0, max(y0 + th - H, 0)), mode=self.pad_mode) if self.pad_mode else frames
            return x[:, :, y0:y0 + th, x0:x0 + tw].contiguous()

        def _crop_d4(self, frames, y0, x0, th, tw, elem):
            return _g(self._crop(frames, y0, x0, th, tw), elem).contiguous()

        def _oriented(self, frames, tile, elem):
            self.current = (tile.src[0], tile.src[1], elem)
            return super()._oriented(frames, tile, elem)

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


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_errors():
    from edvr_amd import VideoRestorer
    net = _StubNet(5).eval()
    plain = VideoRestorer(net, num_frame=5)
    assert plain.tiled is False and plain.time_reverse is False and plain.share_alignment is False
    vr = VideoRestorer(net, num_frame=5, time_reverse=True)
    assert vr.tiled and vr.time_reverse is True and vr.share_alignment is True and vr.elements is None  # turns the tiled path on; shared by default
    assert VideoRestorer(net, num_frame=5, time_reverse=True, share_alignment=False).share_alignment is False
    assert VideoRestorer(net, num_frame=5, time_reverse=True, share_alignment=True, self_ensemble='flip4').elements == (0, 1, 2, 3)
    for share in (True, False):  # share_alignment without time_reverse
        with pytest.raises(ValueError):
            VideoRestorer(net, num_frame=5, share_alignment=share)
        with pytest.raises(ValueError):
            VideoRestorer(net, num_frame=5, time_reverse=False, share_alignment=share)
    for bad in (1, 0, 'yes', None, (True,)):  # non-bool values
        with pytest.raises(ValueError):
            VideoRestorer(net, num_frame=5, time_reverse=bad)
    for bad in (1, 0, 'no', (False,)):
        with pytest.raises(ValueError):
            VideoRestorer(net, num_frame=5, time_reverse=True, share_alignment=bad)
    for bad in ((8,), (0, 0), 'rot', (16,)):  # temporal reversal is no new element id: self_ensemble's checks stay
        with pytest.raises(ValueError):
            VideoRestorer(net, num_frame=5, time_reverse=True, self_ensemble=bad)


# ------------------------------------------------------------------------------------------------ the schedule
def _modes(count):
    return ['first'] + ['middle'] * (count - 2) + ['last']


@pytest.mark.parametrize('share', [True, False])
@pytest.mark.parametrize('ensemble', [None, (5, 0, 2)])
@pytest.mark.parametrize('tiles', [True, False])
def test_time_reverse_schedule(tiles, ensemble, share):
    from edvr_amd import tile_grid, window_table
    t, n, chunk, (H, W) = 5, 9, 4, (22, 30)  # padded to 24 x 32; tiles (16, 16), overlap 8: 2 x 3 tiles
    kw = dict(tile=(16, 16), tile_overlap=8) if tiles else {}
    net, vr = _stub_restorer(t, 'reflection_circle', chunk, pad_mode='replicate', self_ensemble=ensemble, time_reverse=True,
                             share_alignment=share, **kw)
    elements = ensemble if ensemble is not None else (None,)
    grid = tile_grid(H, W, kw.get('tile'), kw.get('tile_overlap'), 4)
    pairs = [(tl.src[0], tl.src[1], k) for tl in grid for k in elements]  # vr.pairs stays (tile x spatial element), element innermost
    frames = _coded_frames(n, H, W)
    with torch.no_grad():
        steps, outs = [], []
        for out in vr.restore_chunks(iter(frames.unbind(0))):
            outs.append(out)
            steps.append(list(net.log))
            del net.log[:]
            assert len(vr.banks) == len(pairs)  # no second bank for the reversed order
    assert [o.shape[0] for o in outs] == [4, 4, 1]
    assert [(tl.src[0], tl.src[1], k) for tl, k in vr.pairs] == pairs
    # the output: every term of the stub is the enlarged frame; 2 n terms add up in float32, then one multiply by 1 / (2 n)
    terms = 2 * len(elements)
    want = frames.repeat_interleave(4, 2).repeat_interleave(4, 3)
    acc = want.clone()
    for _ in range(terms - 1):
        acc = acc + want
    assert torch.equal(torch.cat(outs, 0), acc * (1.0 / terms))
    table = window_table(n, t, 'reflection_circle').tolist()
    # per chunk and (tile, element), in the work-list order: the exact gathers, alignments and tails of the arm
    first = 0
    for log, out in zip(steps, outs):
        rows = table[first:first + out.shape[0]]
        rev_rows = [r[::-1] for r in rows]
        first += out.shape[0]
        want_log = []
        for i, pair in enumerate(pairs):
            e = i % len(elements)
            elem = 0 if pair[2] is None else pair[2]
            fwd, rvs = _modes(terms)[2 * e], _modes(terms)[2 * e + 1]
            if share:
                want_log += [('gather',), ('align', pair, True, rows), ('tail', pair, elem, fwd, 1.0 / terms, rows, True),
                             ('tail', pair, elem, rvs, 1.0 / terms, rev_rows, False)]
            else:
                want_log += [('gather',), ('align', pair, False, rows), ('tail', pair, elem, fwd, 1.0 / terms, rows, True),
                             ('gather',), ('align', pair, False, rev_rows), ('tail', pair, elem, rvs, 1.0 / terms, rev_rows, True)]
        assert [e if e[0] != 'gather' else ('gather',) for e in log] == want_log
        gathers = [e[1] for e in log if e[0] == 'gather']
        assert len(gathers) == (1 if share else 2) * len(pairs)
        slot_rows = [[f % vr.slots for f in r] for r in rows]
        for j, g in enumerate(gathers):
            got = [g[q * t:(q + 1) * t] for q in range(len(rows))]
            if share or j % 2 == 0:
                assert got == slot_rows
            else:  # the second table is the first with every row reversed
                assert got == [r[::-1] for r in slot_rows]


def test_without_time_reverse_nothing_new_is_called():
    """time_reverse=False: the tiled path calls restore_from_features alone, with the keywords it passed before."""
    net, vr = _stub_restorer(5, 'replicate', 4, pad_mode='replicate')
    seen = []

    def plain(pyr, x_center, b, t, out_dtype=torch.float32, out=None, keep=None):
        seen.append(keep)
        out.copy_(x_center.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :out.shape[2], :out.shape[3]])
        return out

    net.restore_from_features, net.align_windows, net.restore_from_aligned = plain, None, None
    frames = _coded_frames(6, 22, 30)
    with torch.no_grad():
        out = torch.cat(list(vr.restore_chunks([frames])), 0)
    assert seen == [(0, 0), (0, 0)]
    assert torch.equal(out, frames.repeat_interleave(4, 2).repeat_interleave(4, 3))


# ------------------------------------------------------------------------------------------------ scripts
def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_video_parser_accepts_the_flag():
    ev = _load('eval_video')
    base = ['--gt', 'g', '--lq', 'l']
    assert ev.parse_args(base).time_reverse is False
    a = ev.parse_args(base + ['--time-reverse'])
    assert a.time_reverse is True and a.self_ensemble is None
    a = ev.parse_args(base + ['--time-reverse', '--self-ensemble', 'd4'])  # composes with the spatial ensemble ...
    assert a.time_reverse is True and a.self_ensemble == 'd4'
    for bad in ('d4t', 'time', 'd16'):  # ... whose choices stay flip4 | d4
        with pytest.raises(SystemExit):
            ev.parse_args(base + ['--self-ensemble', bad])


def test_bench_video_parser_makes_time_reverse_a_leg_of_its_own():
    bv = _load('bench_video')
    assert bv.parse_args([]).leg is None and bv.parse_args([]).time_reverse is False
    assert bv.parse_args(['--self-ensemble', 'flip4']).leg == 'ensemble'
    a = bv.parse_args(['--time-reverse', '--config', 'L_T5'])
    assert a.leg == 'time' and a.time_reverse and a.self_ensemble is None
    a = bv.parse_args(['--time-reverse', '--self-ensemble', 'flip4'])
    assert a.leg == 'time' and a.self_ensemble == 'flip4'
    for bad in (['--time-reverse', '--leg', 'pad'], ['--time-reverse', '--tile-blend', '32']):
        with pytest.raises(SystemExit):
            bv.parse_args(bad)


@pytest.mark.parametrize('ensemble', [None, 'flip4'])
def test_eval_video_reports_plain_and_time_reverse_side_by_side(tmp_path, monkeypatch, ensemble):
    import json
    import edvr_amd
    from edvr_amd import data as D, metrics as M
    write_video_test_tree(str(tmp_path), dict(folders=['000'], frames=7, lq_hw=(8, 12), scale=4))

    class Net(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def to(self, device):
            return self

    def read_img_seq(paths, device='cpu', **k):
        return torch.stack([torch.from_numpy(D.decode_image(open(p, 'rb').read()).transpose(2, 0, 1).copy()).float() / 255 for p in paths])

    calls = []

    def validate_video(net, lq, gt=None, num_frame=5, padding='reflection_circle', chunk=8, crop_border=0, test_y_channel=False,
                       self_ensemble=None, time_reverse=False):
        calls.append((self_ensemble, time_reverse))
        return None, [31.0 if time_reverse else 30.0] * lq.shape[0]

    monkeypatch.setattr(edvr_amd, 'EDVR', Net)
    monkeypatch.setattr(D, 'read_img_seq', read_img_seq)
    monkeypatch.setattr(M, 'validate_video', validate_video)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    out_json = tmp_path / 'r.json'
    args = argparse.Namespace(lq=str(tmp_path / 'lq'), gt=str(tmp_path / 'gt'), weights=None, name='REDS4', num_feat=64, num_reconstruct_block=2,
                              num_frame=5, hr_in=False, with_predeblur=False, no_tsa=False, padding='reflection', crop_border=0,
                              test_y_channel=False, batch=3, self_ensemble=ensemble, time_reverse=True, json=str(out_json))
    lines = []
    summary = _load('eval_video').evaluate(args, log=lines.append)
    assert calls == [(None, False), (ensemble, True)]             # the plain pass, then the ensemble with both time orders
    assert summary == {'000': 30.0}                               # the return value stays the plain result
    label = 'flip4+time-reverse' if ensemble else 'time-reverse'
    assert all('30.0000 dB' in ln and f'self-ensemble {label} 31.0000 dB' in ln for ln in lines) and len(lines) == 2
    rec = json.load(open(out_json))
    assert rec['time_reverse'] is True and rec['self_ensemble'] == ensemble and rec['self_ensemble_average'] == 31.0 and rec['average'] == 30.0
