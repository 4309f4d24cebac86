"""CPU: the deinterlacer's definition (tests/deint_ref.py) checked against itself and its stated properties, the coverage of
the structured clip the GPU test uses, the Y4M reader's `interlaced=`, y4m.deinterlaced and restore_y4m(deinterlace=...) with stand-ins
for the device pieces, and the command line of scripts/restore_video.py.  Everything is exact."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import deint_ref as D
import util_deint as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plane(n, R, C, depth, seed):
    return np.random.default_rng(seed).integers(0, 1 << depth, size=(n, R, C))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('depth', [8, 16])
@pytest.mark.parametrize('n, R, C', [(1, 2, 1), (1, 3, 4), (2, 2, 5), (2, 5, 7), (3, 6, 9), (3, 3, 2)])
def test_loop_form_equals_vectorised_form(n, R, C, depth):
    """Also: n = 1 and n = 2 meet every fold_T case (both reflections, repeated at n = 1), R = 2 and R = 3 the repeated fold_R."""
    maxv = (1 << depth) - 1
    plane = _plane(n, R, C, depth, seed=n * 100 + R * 10 + C + depth)
    ctx = _plane(2, R, C, depth, seed=7)
    for first in ('top', 'bottom'):
        for mode in ('field', 'frame'):
            for prev, nxt in ((None, None), (ctx[0], None), (None, ctx[1]), (ctx[0], ctx[1])):
                a = D.plane_loop(plane, maxv, first, mode, prev, nxt)
                b = D.plane_vec(plane, maxv, first, mode, prev, nxt)
                assert np.array_equal(a, b), (first, mode, prev is None, nxt is None)


def test_folds():
    assert [D.fold(i, 2) for i in range(-2, 4)] == [0, 1, 0, 1, 0, 1]
    assert [D.fold(i, 3) for i in range(-2, 5)] == [2, 1, 0, 1, 2, 1, 0]
    assert [D.fold(i, 5) for i in range(-2, 7)] == [2, 1, 0, 1, 2, 3, 4, 3, 2]
    for n in (1, 2, 3):
        for k in range(-2, 2 * n + 2):
            assert D.field_frame(k, n, False, False) == D.fold(k, 2 * n) // 2
            assert D.field_frame(k, n, True, True) == k // 2
    # one context frame: the other side reflects about its end of the batch, if need be into the context (n = 1)
    assert [D.field_frame(k, 1, True, False) for k in range(-2, 4)] == [-1, -1, 0, 0, 0, -1]
    assert [D.field_frame(k, 1, False, True) for k in range(-2, 4)] == [1, 0, 0, 0, 1, 1]
    assert [D.field_frame(k, 2, False, False) for k in range(-2, 6)] == [1, 0, 0, 0, 1, 1, 1, 0]


@pytest.mark.parametrize('first', ['top', 'bottom'])
def test_kept_rows_are_the_fields_rows_and_frame_mode_is_the_even_fields(first):
    plane = _plane(3, 7, 6, 8, seed=3)
    out = D.plane_vec(plane, 255, first, 'field')
    b = D.FIRST[first]
    for k in range(6):
        q = (k + b) % 2
        assert np.array_equal(out[k, q::2], plane[k // 2, q::2])
    assert np.array_equal(D.plane_vec(plane, 255, first, 'frame'), out[0::2])


def test_output_stays_a_sample_at_the_extremes():
    """All 0, all M and the fields alternately 0 / M at d = 16 (plane_vec asserts 0 <= out <= M itself; M + M must not wrap)."""
    M = 65535
    for clip in U.extreme_clips(3, 6, 5, '444p16'):
        for first in ('top', 'bottom'):
            out = D.deinterlace(clip, 6, 5, '444p16', first, 'field')
            planes = D.split(out, 6, 5, '444p16')
            assert all(0 <= p.min() and p.max() <= M for p in planes)
    zero, full, alt = U.extreme_clips(2, 6, 5, '444p16')
    assert np.array_equal(D.deinterlace(zero, 6, 5, '444p16', mode='frame'), zero)
    assert np.array_equal(D.deinterlace(full, 6, 5, '444p16', mode='frame'), full)
    got = D.split(D.deinterlace(alt, 6, 5, '444p16', 'top', 'field'), 6, 5, '444p16')[0]
    assert set(np.unique(got)) <= {0, M} and np.array_equal(got[0], np.zeros((6, 5))) and np.array_equal(got[1], np.full((6, 5), M))


def test_a_static_linear_ramp_is_reproduced():
    """Columns linear in the row index, the same in every frame: nothing moves, so the band closes around the sample the other field
    holds (and inside the plane every direction's mean of the rows above and below is that sample too) - every output frame is the
    input frame, at the reflecting rows as well."""
    R, C = 12, 6
    for slope_x in (0, 3):
        ramp = (10 + 4 * np.arange(R))[:, None] + slope_x * np.arange(C)[None, :]
        plane = np.repeat(ramp[None], 3, 0)
        for first in ('top', 'bottom'):
            for fn in (D.plane_vec, D.plane_loop):
                assert np.array_equal(fn(plane, 255, first, 'field'), np.repeat(ramp[None], 6, 0))


def test_far_apart_neighbours_in_time_leave_the_spatial_prediction():
    """Where p and nx sit far apart - from each other and from everything else - the band is wide and the output is pred."""
    n, R, C = 3, 8, 9
    plane = _plane(n, R, C, 8, seed=11) % 40 + 100  # 100 ... 139
    first = 'top'
    k = 2  # frame 1's top field: the missing rows are odd; p = field 1 (frame 0, odd rows), nx = field 3 (frame 1, odd rows)
    plane[0, 1::2] = 0
    plane[1, 1::2] = 255
    info = {}
    out = D.plane_vec(plane, 255, first, 'field', info=info)
    pred = np.empty((R // 2, C), np.int64)
    cur = plane[1]
    for r, y in enumerate(range(1, R, 2)):
        for x in range(C):
            c = lambda d: int(cur[D.fold(y - 1, R), min(max(x + d, 0), C - 1)])
            e = lambda d: int(cur[D.fold(y + 1, R), min(max(x + d, 0), C - 1)])
            scores = [sum(abs(c(j + u) - e(-j + u)) for u in (-1, 0, 1)) + (j != 0) for j in D.ORDER]
            j = D.ORDER[scores.index(min(scores))]
            pred[r, x] = (c(j) + e(-j)) >> 1
    assert np.array_equal(out[k, 1::2], pred)
    assert pred.min() >= 100 and pred.max() <= 139  # ... and nowhere near dmid = 127 by accident alone: the band is what let it through


@pytest.mark.parametrize('fmt, H, W', [('420', 6, 5), ('422p10', 5, 4), ('444p16', 4, 3)])
def test_a_whole_clip_equals_any_split_with_context(fmt, H, W):
    n = 5
    clip = U.random_frames(n, H, W, fmt, seed=21)
    for first in ('top', 'bottom'):
        for mode in ('field', 'frame'):
            whole = D.deinterlace(clip, H, W, fmt, first, mode)
            per = 2 if mode == 'field' else 1
            for cutset in ([1], [2], [4], [1, 2], [2, 3], [1, 2, 3, 4]):
                edges = [0] + cutset + [n]
                parts = []
                for lo, hi in zip(edges, edges[1:]):
                    parts.append(D.deinterlace(clip[lo:hi], H, W, fmt, first, mode, prev=clip[lo - 1] if lo else None, nxt=clip[hi] if hi < n else None))
                assert np.array_equal(np.concatenate(parts), whole), (first, mode, cutset)
                assert sum(p.shape[0] for p in parts) == per * n


def test_the_structured_clip_reaches_every_direction_and_every_clamp_state():
    """The coverage condition on the structured GPU input: the restatement picks every j of D4 and D6 is active at its upper end, at its
    lower end, and inactive - for both field orders, on the shape the GPU test uses."""
    for first in ('top', 'bottom'):
        info = {}
        D.deinterlace(U.structured_clip(3, 18, 65, '420', first), 18, 65, '420', first, 'field', info=info)
        for j in D.ORDER:
            assert (info['j'] == j).sum() >= 20, (first, j)
        for state in (-1, 0, 1):
            assert (info['clamp'] == state).sum() >= 20, (first, state)


# ---------------------------------------------------------------------------------------------------------------- the reader
@pytest.mark.parametrize('tag, expect', [('It', 't'), ('Ib', 'b'), ('Ip', 'p'), ('I?', '?'), ('', None)])
def test_reader_reads_interlaced_streams_when_asked(tag, expect):
    from edvr_amd.y4m import Y4MReader
    frames = U.random_frames(2, 4, 6, '420', seed=1)
    data = U.y4m_bytes(frames, 4, 6, f'F25:1 {tag} C420jpeg')
    r = Y4MReader(io.BytesIO(data), interlaced=True)
    assert r.interlace == expect
    assert np.array_equal(r.read(4)[:, 6:].numpy(), frames)
    if expect in ('t', 'b'):
        with pytest.raises(ValueError, match='deinterlace first'):
            Y4MReader(io.BytesIO(data))
        with pytest.raises(ValueError):
            Y4MReader(io.BytesIO(data), interlaced=False)
    else:
        assert Y4MReader(io.BytesIO(data)).interlace == expect


def test_reader_refuses_mixed_interlacing_always():
    from edvr_amd.y4m import Y4MReader
    data = U.y4m_bytes(U.random_frames(1, 4, 6, '420', seed=1), 4, 6, 'F25:1 Im C420jpeg')
    with pytest.raises(ValueError):
        Y4MReader(io.BytesIO(data), interlaced=True)
    with pytest.raises(ValueError):
        Y4MReader(io.BytesIO(data))


# ---------------------------------------------------------------------------------------------------------------- the generator
def _ref_op(calls=None):
    """ops.deinterlace on CPU tensors through the restatement."""
    def op(yuv, H, W, format='420', *, first='top', mode='field', prev=None, next=None, out=None):
        assert out is None
        fs = D.frame_size(H, W, format)
        if calls is not None:
            calls.append((yuv.shape[0], prev is not None, next is not None))
        cut = lambda t: None if t is None else t.numpy().reshape(-1)[:fs]
        return torch.from_numpy(D.deinterlace(yuv.numpy()[:, :fs], H, W, format, first, mode, prev=cut(prev), nxt=cut(next)))
    return op


@pytest.mark.parametrize('mode', ['field', 'frame'])
@pytest.mark.parametrize('fmt', ['420', '422p10'])
def test_deinterlaced_gives_the_whole_clip_for_every_piece_pattern(monkeypatch, fmt, mode):
    from edvr_amd import ops, y4m
    n, H, W = 8, 6, 5
    clip = U.random_frames(n, H, W, fmt, seed=5)
    whole = D.deinterlace(clip, H, W, fmt, 'bottom', mode)
    for pattern in ([1] * n, [n], [3, 1, 4], [1, n - 1]):
        calls = []
        monkeypatch.setattr(ops, 'deinterlace', _ref_op(calls))
        assert sum(pattern) == n
        at, pieces = 0, []
        for k in pattern:
            pieces.append(torch.from_numpy(clip[at:at + k]))
            at += k
        got = list(y4m.deinterlaced(iter(pieces), H, W, fmt, 'bottom', mode))
        assert [g.shape[0] for g in got] == [k * (2 if mode == 'field' else 1) for k in pattern]
        assert np.array_equal(torch.cat(got).numpy(), whole), pattern
        assert calls == [(k, i > 0, i < len(pattern) - 1) for i, k in enumerate(pattern)]
    assert list(y4m.deinterlaced(iter([]), H, W, fmt)) == []


def test_deinterlaced_holds_one_piece():
    """A piece leaves when the next one has arrived: the delay is one piece."""
    from edvr_amd import y4m
    seen = []

    def pieces():
        for i in range(3):
            seen.append(('read', i))
            yield torch.zeros(1, D.frame_size(4, 4, '420'), dtype=torch.uint8)

    import edvr_amd.ops as ops
    orig = ops.deinterlace
    ops.deinterlace = _ref_op()
    try:
        for i, _ in enumerate(y4m.deinterlaced(pieces(), 4, 4, '420')):
            seen.append(('out', i))
    finally:
        ops.deinterlace = orig
    assert seen == [('read', 0), ('read', 1), ('out', 0), ('read', 2), ('out', 1), ('out', 2)]


# ---------------------------------------------------------------------------------------------------------------- restore_y4m
class _Nearest4:
    """Stands in for VideoRestorer on the CPU: 'restores' by x4 replication, chunk by chunk."""
    made = []

    def __init__(self, net, out_dtype=None, **kwargs):
        assert out_dtype == torch.float32
        self.scale, self.kwargs = 4, kwargs
        _Nearest4.made.append(self)

    def restore_chunks(self, frames, length=None):
        for piece in frames:
            yield piece.repeat_interleave(4, 2).repeat_interleave(4, 3)


def _stand_ins(monkeypatch, calls):
    import util_yuv as Y
    from edvr_amd import ops, video

    def deint(*a, **k):
        calls.append('deinterlace')
        return _ref_op()(*a, **k)

    def decode(yuv, h, w, matrix, rng, chroma):
        calls.append(('yuv420_to_rgb', yuv.shape[0]))
        return Y.decode_def(yuv, h, w, matrix, rng, chroma)

    def encode(rgb, matrix, rng, out):
        calls.append(('rgb_to_yuv420', rgb.shape[0]))
        return out.copy_(Y.encode_def(rgb, matrix, rng))

    monkeypatch.setattr(ops, 'deinterlace', deint)
    monkeypatch.setattr(ops, 'yuv420_to_rgb', decode)
    monkeypatch.setattr(ops, 'rgb_to_yuv420', encode)
    monkeypatch.setattr(video, 'VideoRestorer', _Nearest4)
    return Y


@pytest.mark.parametrize('mode', ['field', 'frame'])
@pytest.mark.parametrize('tag, order, first', [('It', 'auto', 'top'), ('Ib', 'auto', 'bottom'), ('Ip', 'bff', 'bottom'), ('It', 'bff', 'bottom'), ('', 'tff', 'top')])
def test_restore_y4m_deinterlaces_between_the_copy_and_the_decode(monkeypatch, tag, order, first, mode):
    from edvr_amd import y4m
    calls = []
    Y = _stand_ins(monkeypatch, calls)
    n, H, W = 5, 8, 12
    frames = U.random_frames(n, H, W, '420', seed=9)
    data = U.y4m_bytes(frames, H, W, f'F30000:1001 {tag} A1:1 C420jpeg')
    out = io.BytesIO()
    per = 2 if mode == 'field' else 1
    assert y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(data), out, read_frames=2, deinterlace=mode, field_order=order, chunk=3) == per * n
    assert _Nearest4.made[-1].kwargs == dict(chunk=3)  # the restorer sees neither argument
    head = out.getvalue().split(b'\n')[0].split()
    assert b'Ip' in head and (b'F60000:1001' if mode == 'field' else b'F30000:1001') in head
    assert [f'W{4 * W}'.encode(), f'H{4 * H}'.encode()] == head[1:3]
    r = y4m.Y4MReader(io.BytesIO(out.getvalue()))
    prog = torch.from_numpy(D.deinterlace(frames, H, W, '420', first, mode))
    rgb = Y.decode_def(prog, H, W, 'bt601', 'limited', 'bilinear').repeat_interleave(4, 2).repeat_interleave(4, 3)
    assert torch.equal(r.read(per * n + 1)[:, 6:], Y.encode_def(rgb, 'bt709' if 4 * H > 576 or 4 * W >= 1280 else 'bt601', 'limited'))
    assert calls.count('deinterlace') == 3  # pieces of 2, 2 and 1 frames
    # every piece is deinterlaced before it is decoded, and a piece leaves once the next has been read
    assert [c for c in calls if c == 'deinterlace' or c[0] == 'yuv420_to_rgb'] == \
        ['deinterlace', ('yuv420_to_rgb', 2 * per), 'deinterlace', ('yuv420_to_rgb', 2 * per), 'deinterlace', ('yuv420_to_rgb', per)]


def test_restore_y4m_passes_progressive_streams_through_and_keeps_its_default(monkeypatch):
    from edvr_amd import y4m
    net = torch.nn.Linear(1, 1)
    n, H, W = 3, 8, 12
    frames = U.random_frames(n, H, W, '420', seed=10)
    outs = {}
    for key, tag, kw in (('plain', 'Ip', {}), ('auto', 'Ip', dict(deinterlace='field')), ('untagged', '', dict(deinterlace='frame', field_order='auto'))):
        calls = []
        _stand_ins(monkeypatch, calls)
        out = io.BytesIO()
        assert y4m.restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, f'F25:1 {tag} C420jpeg')), out, read_frames=2, **kw) == n
        assert 'deinterlace' not in calls
        assert calls == [('yuv420_to_rgb', 2), ('rgb_to_yuv420', 2), ('yuv420_to_rgb', 1), ('rgb_to_yuv420', 1)]  # the calls it always made
        assert b'F25:1' in out.getvalue().split(b'\n')[0].split()  # the rate is not doubled
        outs[key] = out.getvalue().split(b'\n', 1)[1]
    assert outs['plain'] == outs['auto'] == outs['untagged']
    # without deinterlace= an interlaced stream still raises, with any field_order
    calls = []
    _stand_ins(monkeypatch, calls)
    for kw in ({}, dict(field_order='tff')):
        with pytest.raises(ValueError, match='deinterlace first'):
            y4m.restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, 'F25:1 It C420jpeg')), io.BytesIO(), **kw)
    for kw in (dict(deinterlace='bob'), dict(deinterlace='field', field_order='top'), dict(deinterlace=True)):
        with pytest.raises(ValueError):
            y4m.restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, 'F25:1 It C420jpeg')), io.BytesIO(), **kw)
    with pytest.raises(ValueError):
        y4m.restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, 'F25:1 Im C420jpeg')), io.BytesIO(), deinterlace='field')
    assert calls == []
    assert (y4m.double_rate('30000:1001'), y4m.double_rate('25:1'), y4m.double_rate(None)) == ('60000:1001', '50:1', None)
    # no F tag: none is written
    out = io.BytesIO()
    y4m.restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, 'It C420jpeg')), out, deinterlace='field')
    assert not any(t.startswith(b'F') for t in out.getvalue().split(b'\n')[0].split()[1:])


def test_ops_deinterlace_refuses_the_cpu_and_bad_arguments_before_any_launch():
    from edvr_amd import ops
    yuv = torch.zeros(2, ops.yuv_frame_size(4, 4, '420'), dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        ops.deinterlace(yuv, 4, 4)
    for kw in (dict(first='left'), dict(mode='bob'), dict(format='411')):
        with pytest.raises(ValueError):
            ops.deinterlace(yuv, 4, 4, **kw)


# ---------------------------------------------------------------------------------------------------------------- the script
def _script():
    spec = importlib.util.spec_from_file_location('restore_video', os.path.join(ROOT, 'scripts', 'restore_video.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restore_video_command_line_takes_deinterlace(capsys):
    mod = _script()
    args = mod.parse_args(['-', '-'])
    assert (args.deinterlace, args.field_order) == (None, 'auto')
    args = mod.parse_args(['-', '-', '--deinterlace'])
    assert (args.deinterlace, args.field_order) == ('field', 'auto')
    args = mod.parse_args(['in.y4m', 'out.y4m', '--deinterlace', 'frame', '--field-order', 'bff'])
    assert (args.deinterlace, args.field_order) == ('frame', 'bff')
    args = mod.parse_args(['-', '-', '--deinterlace', '--field-order', 'tff', '--weights', 'w.pth'])
    assert (args.deinterlace, args.field_order, args.weights) == ('field', 'tff', 'w.pth')
    for bad in (['-', '-', '--deinterlace', 'bob'], ['-', '-', '--field-order', 'tff'], ['-', '-', '--deinterlace', '--field-order', 'top']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
