"""GPU: ops.field_match and ops.field_weave (csrc/telecine.hip) against the NumPy restatement of DESIGN 4.20 (tests/telecine_ref.py), exactly,
on the smallest shapes that reach every branch - planes of 4 rows, rows at, below and above the 16-row block and strip edge, widths below one
lane's run, at its tail, at the block tail and past one 256-column tile, bytes and words, every subsampling, 1 ... 3 frames with every
pattern of context frames, both field orders, Y4M-layout and dense buffers; block counts at the block grid's corners; sums past 2^32;
the error paths; y4m.inverse_telecined for every piece pattern; and restore_y4m(deinterlace='film') through a tiny EDVR against the
composition done by hand.  Every comparison is torch.equal."""
import ctypes
import io
import itertools

import numpy as np
import pytest
import torch

import deint_ref as D
import telecine_ref as T
import util_telecine as U

pytestmark = pytest.mark.gpu

FORMATS = ['420', '422', '444', '420p10', '444p16']
HEIGHTS = [4, 5, 7, 16, 17, 18, 33]
WIDTHS = [1, 2, 5, 15, 16, 17, 63, 64, 65, 257]
CONTEXTS = [(False, False), (True, True), (True, False), (False, True)]  # prev, prev2


def _y4m_layout(frames):
    """The frames as `buf[:, 6:]` of a Y4M read buffer on the device: rows 6 + framesize apart, 6 bytes in."""
    buf = torch.full((frames.shape[0], 6 + frames.shape[1]), 0x5a, dtype=torch.uint8, device='cuda')
    buf[:, 6:] = torch.from_numpy(frames).cuda()
    return buf[:, 6:]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_match(frames, H, W, fmt, first, prev=None, prev2=None, y4m=False, **kw):
    from edvr_amd import ops
    want = T.field_match(frames, H, W, fmt, first, prev, prev2, **kw)
    yuv = _y4m_layout(frames) if y4m else _dev(frames)
    got = ops.field_match(yuv, H, W, fmt, first=first, prev=_dev(prev), prev2=None if prev2 is None else _dev(prev2)[None], **kw)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (frames.shape[0], 7)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (H, W, fmt, first, prev is not None, prev2 is not None, y4m, got.cpu().tolist(), want.tolist())
    return got


@pytest.mark.parametrize('W', WIDTHS)
@pytest.mark.parametrize('H', HEIGHTS)
def test_field_match_on_random_frames(H, W):
    """Every (H, W); format, frame count, context and layout cycle with periods 5, 3, 4 and 2 over the 70 shapes, so each value of each
    meets small and large shapes; both field orders on every one.  Uniform random samples comb everywhere: every sum and count is large."""
    i = HEIGHTS.index(H) * len(WIDTHS) + WIDTHS.index(W)
    fmt, n, (has_prev, has_prev2) = FORMATS[i % 5], 1 + i % 3, CONTEXTS[(i // 2) % 4]
    frames = U.random_frames(n, H, W, fmt, seed=3000 + i)
    ctx = U.random_frames(2, H, W, fmt, seed=4000 + i)
    for first in ('top', 'bottom'):
        _check_match(frames, H, W, fmt, first, ctx[0] if has_prev else None, ctx[1] if has_prev2 else None, y4m=i % 2 == 0)


@pytest.mark.parametrize('fmt', FORMATS)
def test_field_match_every_format_and_context(fmt):
    """Each format on a plane past one tile (18 x 257), an odd one (7 x 65) and one narrower than a lane's run (5 x 5), n = 1, 2, 3, with
    every pattern of prev / prev2 in both layouts, and other thresholds."""
    for H, W, n in ((18, 257, 2), (7, 65, 3), (5, 5, 1)):
        frames = U.random_frames(n, H, W, fmt, seed=H * W + n)
        ctx = U.random_frames(2, H, W, fmt, seed=H * W)
        for c, (has_prev, has_prev2) in enumerate(CONTEXTS):
            _check_match(frames, H, W, fmt, 'top' if c % 2 else 'bottom', ctx[0] if has_prev else None, ctx[1] if has_prev2 else None, y4m=c < 2)
        _check_match(frames, H, W, fmt, 'top', ctx[0], ctx[1], y4m=True, nt=0, ct=0)
        _check_match(frames, H, W, fmt, 'bottom', ctx[0], ctx[1], nt=40, ct=255)


@pytest.mark.parametrize('fmt, H, W', [('420', 33, 65), ('422p10', 18, 257)])
def test_a_row_does_not_depend_on_the_batch(fmt, H, W):
    """A batch split in two, with the frames before it as context, gives the whole batch's rows - device against device - and `out=`."""
    from edvr_amd import ops
    n = 5
    clip = _dev(U.random_frames(n, H, W, fmt, seed=91))
    whole = ops.field_match(clip, H, W, fmt, first='bottom')
    for cut in range(1, n):
        a = ops.field_match(clip[:cut], H, W, fmt, first='bottom')
        b = ops.field_match(clip[cut:], H, W, fmt, first='bottom', prev=clip[cut - 1], prev2=clip[cut - 2] if cut >= 2 else None)
        assert torch.equal(torch.cat([a, b]), whole), cut
    out = torch.full((n, 7), -1, dtype=torch.int64, device='cuda')
    assert ops.field_match(clip, H, W, fmt, first='bottom', out=out) is out and torch.equal(out, whole)


def test_a_workgroup_walks_its_strip():
    """Enough strips (17 x 70 frames) that every workgroup takes both tiles of its strip, one after the other."""
    H, W, n = 260, 257, 70
    frames = U.random_frames(n, H, W, '420', seed=17)
    _check_match(frames, H, W, '420', 'top')


@pytest.mark.parametrize('first', ['top', 'bottom'])
def test_field_match_on_the_designed_clip(first):
    """The telecined film clip at an orphan-free and an orphan phase: the three static lines make mic exactly 80 - not more than mi."""
    for phase, fmt in ((0, '420'), (5, '420'), (3, '420p10')):
        video, _ = U.telecine(U.film_clip(fmt=fmt), first, phase, fmt=fmt)
        got = _check_match(video, U.FILM_H, U.FILM_W, fmt, first, y4m=phase == 0).cpu()
        matched = torch.where(got[:, 1] < got[:, 0], got[:, 3], got[:, 2]).tolist()
        assert matched[1:] == [80] * (len(matched) - 1) and (matched[0] == 80 or phase == 5)


@pytest.mark.parametrize('y0, x0', [(0, 0), (0, 17), (2, 0), (2, 17), (16, 32), (0, 32), (16, 0)])
def test_a_block_count_is_whole(y0, x0):
    """18 x 33: the block grid has full blocks, blocks of 1 column, of 2 rows and one of 2 x 1.  A 16 x 16 region whose every other row is
    raised - 15 of its rows comb - lies at each corner of the plane and on each corner block; everything else is flat.  At (0, 0) the
    region is one block and mic_c is all of it, 15 x 16, however lanes and waves divide it; elsewhere it straddles the block grid and
    mic_c is its largest part, not the sum."""
    H, W = 18, 33
    planes = [np.full((1, r, c), 100, np.int64) for r, c in D.plane_shapes(H, W, '420')]
    planes[0][0, y0 + (y0 < 16):y0 + 16:2, x0:x0 + 16] = 200  # (in the last two rows only row 16 can comb: it is the one raised there)
    frames = D.join(planes, '420')
    hot = T.comb(planes[0][0]) > 9
    parts = [int(hot[y:y + 16, x:x + 16].sum()) for y in (0, 16) for x in (0, 16, 32)]
    assert max(parts) > 0 and ((y0, x0) != (0, 0) or parts == [240, 0, 0, 0, 0, 0]) and ((y0, x0) not in ((0, 17), (2, 0), (2, 17)) or max(parts) < sum(parts))
    for y4m in (False, True):
        got = _check_match(frames, H, W, '420', 'top', y4m=y4m).cpu()
        assert int(got[0, 2]) == max(parts)


def test_the_extremes_pass_32_bits():
    """444p16, 300 x 300: all 0, all 65535 and rows alternating 0 / 65535 - the frame's comb sum is 298 x 300 x (65535 - 512) > 2^32, and so are A
    and C against a frame that alternates the other way."""
    H, W, fmt = 300, 300, '444p16'
    maxv = 65535

    def clip(kind):
        planes = []
        for r, c in D.plane_shapes(H, W, fmt):
            p = np.zeros((2, r, c), np.int64)
            if kind == 'max':
                p[:] = maxv
            elif kind == 'alternate':
                p[0, 1::2] = maxv
                p[1, 0::2] = maxv
            planes.append(p)
        return D.join(planes, fmt)

    for kind in ('zero', 'max', 'alternate'):
        frames = clip(kind)
        for first in ('top', 'bottom'):
            got = _check_match(frames, H, W, fmt, first, prev2=frames[1], y4m=kind == 'alternate').cpu()
            if kind == 'alternate':
                assert int(got[0, 0]) == 298 * 300 * (maxv - 512) > 2 ** 32 and int(got[1, 4]) == 150 * 300 * maxv > 2 ** 31
            else:
                assert not got.any()


def _check_weave(frames, H, W, fmt, first, indices, matches, prev=None, y4m_in=False, y4m_out=False):
    from edvr_amd import ops
    want = T.field_weave(frames, H, W, fmt, first, indices, matches, prev)
    yuv = _y4m_layout(frames) if y4m_in else _dev(frames)
    kw = dict(first=first, frames=indices, matches=matches, prev=_dev(prev))
    if y4m_out:
        buf = torch.full((want.shape[0], 6 + want.shape[1] + 2), 0xa5, dtype=torch.uint8, device='cuda')
        got = ops.field_weave(yuv, H, W, fmt, out=buf[:, 6:6 + want.shape[1]], **kw)
        assert got.data_ptr() == buf.data_ptr() + 6
        assert bool((buf[:, :6] == 0xa5).all()) and bool((buf[:, 6 + want.shape[1]:] == 0xa5).all())  # nothing outside the frames is written
    else:
        got = ops.field_weave(yuv, H, W, fmt, **kw)
    assert got.shape == want.shape and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (H, W, fmt, first, indices, matches, prev is not None, y4m_in, y4m_out)


@pytest.mark.parametrize('W', WIDTHS)
@pytest.mark.parametrize('H', HEIGHTS)
def test_field_weave_on_random_frames(H, W):
    """The same shapes, formats and layouts: a list that takes every frame with both matches (frame 0's p from prev), out of order."""
    i = HEIGHTS.index(H) * len(WIDTHS) + WIDTHS.index(W)
    fmt, n = FORMATS[i % 5], 1 + i % 3
    frames = U.random_frames(n, H, W, fmt, seed=5000 + i)
    prev = U.random_frames(1, H, W, fmt, seed=6000 + i)[0]
    pairs = [(f, m) for f in reversed(range(n)) for m in (1, 0)]
    for first in ('top', 'bottom'):
        _check_weave(frames, H, W, fmt, first, [f for f, _ in pairs], [m for _, m in pairs], prev, y4m_in=i % 2 == 0, y4m_out=(i // 3) % 2 == 0)


def test_field_weave_every_list_on_three_frames():
    """Every (frame, match) list of length 1 and 2 and a sample of length 3 on 3 frames, with and without prev, into a Y4M-layout buffer."""
    H, W, fmt = 7, 21, '422p10'
    frames = U.random_frames(3, H, W, fmt, seed=8)
    prev = U.random_frames(1, H, W, fmt, seed=9)[0]
    pairs = [(f, m) for f in range(3) for m in (0, 1)]
    lists = [list(c) for k in (1, 2) for c in itertools.product(pairs, repeat=k)] + [list(c) for c in itertools.product(pairs, repeat=3)][::7]
    for c, lst in enumerate(lists):
        needs_prev = (0, 1) in lst
        _check_weave(frames, H, W, fmt, 'top' if c % 2 else 'bottom', [f for f, _ in lst], [m for _, m in lst], prev if needs_prev or c % 3 == 0 else None,
                     y4m_in=c % 2 == 0, y4m_out=c % 4 < 2)


def test_errors():
    from edvr_amd import _lib, ops
    H, W, fmt = 6, 10, '422p10'
    fs = D.frame_size(H, W, fmt)
    yuv = _dev(U.random_frames(2, H, W, fmt, seed=1))
    assert ops.FIELD_MATCH_COLUMNS == ('S_c', 'S_p', 'mic_c', 'mic_p', 'A', 'B', 'C')
    weave = lambda *a, **kw: ops.field_weave(*a, **{'frames': [0], 'matches': [0], **kw})
    for op in (ops.field_match, weave):
        with pytest.raises(NotImplementedError):
            op(yuv.cpu(), H, W, fmt)
        with pytest.raises(NotImplementedError):
            op(yuv.float(), H, W, fmt)
        with pytest.raises(NotImplementedError):
            op(yuv, H, W, fmt, prev=yuv[0].cpu())
        for kw in (dict(format='411'), dict(format='420p8'), dict(first='left'), dict(first=0)):
            with pytest.raises(ValueError):
                op(yuv, H, W, **{'format': fmt, **kw})
        for h in (3, 2, 0):
            with pytest.raises(ValueError, match='4 rows'):
                op(yuv, h, W, '420')
        with pytest.raises(ValueError):
            op(yuv, H, 0, '420')
        with pytest.raises(ValueError):
            op(yuv.view(-1), H, W, fmt)
        with pytest.raises(ValueError, match='shorter'):
            op(yuv[:, :fs - 2], H, W, fmt)
        with pytest.raises(ValueError, match='stride'):
            op(torch.zeros(2, 2 * fs, dtype=torch.uint8, device='cuda')[:, ::2], H, W, fmt)
        flat = torch.zeros(4 * fs + 2, dtype=torch.uint8, device='cuda')
        with pytest.raises(ValueError, match='even'):
            op(flat[1:1 + 2 * fs].view(2, fs), H, W, fmt)
        with pytest.raises(ValueError, match='even'):
            op(yuv, H, W, fmt, prev=flat[1:1 + fs])
        for bad in (yuv[0, :fs - 2], yuv, yuv[:, :4]):
            with pytest.raises(ValueError, match='one frame'):
                op(yuv, H, W, fmt, prev=bad)
    with pytest.raises(ValueError, match='one frame'):
        ops.field_match(yuv, H, W, fmt, prev2=yuv)
    for kw in (dict(nt=-1), dict(ct=256), dict(nt=1.5), dict(ct=True)):
        with pytest.raises(ValueError, match='8-bit level'):
            ops.field_match(yuv, H, W, fmt, **kw)
    with pytest.raises(NotImplementedError):
        ops.field_match(yuv, H, W, fmt, out=torch.zeros(2, 7, dtype=torch.int32, device='cuda'))
    for bad in (torch.zeros(3, 7, dtype=torch.int64, device='cuda'), torch.zeros(2, 14, dtype=torch.int64, device='cuda')[:, ::2]):
        with pytest.raises(ValueError):
            ops.field_match(yuv, H, W, fmt, out=bad)
    # field_weave's lists and out
    for kw in (dict(frames=[], matches=[]), dict(frames=[0, 1], matches=[0]), dict(frames=[2], matches=[0]), dict(frames=[-1], matches=[0]),
               dict(frames=[0], matches=[2]), dict(frames=[0.0], matches=[0]), dict(frames=[True], matches=[0]), dict(frames=3, matches=0)):
        with pytest.raises(ValueError):
            ops.field_weave(yuv, H, W, fmt, **kw)
    with pytest.raises(ValueError, match='needs prev'):
        ops.field_weave(yuv, H, W, fmt, frames=[1, 0], matches=[1, 1])
    ops.field_weave(yuv, H, W, fmt, frames=[1, 0], matches=[1, 0])
    with pytest.raises(ValueError):
        weave(yuv, H, W, fmt, out=torch.zeros(2, fs, dtype=torch.uint8, device='cuda'))  # one frame is named
    with pytest.raises(ValueError, match='shorter'):
        weave(yuv, H, W, fmt, out=torch.zeros(1, fs - 2, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='even'):
        weave(yuv, H, W, fmt, out=flat[1:1 + fs].view(1, fs))
    both = torch.zeros(6, fs, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='overlaps'):
        weave(both[:2], H, W, fmt, out=both[1:2])
    with pytest.raises(ValueError, match='overlaps'):
        weave(both[:1], H, W, fmt, prev=both[3], out=both[3:4])
    # the C ABI refuses what the Python layer never sends
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    table = torch.zeros(2, 7, dtype=torch.int64, device='cuda')
    good = dict(yuv=ptr(yuv), prev=None, prev2=None, table=ptr(table), n=2, H=H, W=W, sx=1, sy=0, depth=10, si=fs, bff=0, nt=2, ct=9)
    call = lambda **kw: _lib.lib().edvr_field_match(*{**good, **kw}.values(), stream)
    for kw in (dict(H=3), dict(W=0), dict(n=0), dict(depth=7), dict(depth=17), dict(sx=0, sy=1), dict(sx=2), dict(yuv=None), dict(table=None), dict(yuv=ptr(yuv, 1)),
               dict(prev=ptr(yuv, 1)), dict(prev2=ptr(yuv, 1)), dict(si=fs + 1), dict(si=fs - 2), dict(bff=2), dict(nt=-1), dict(ct=256)):
        assert call(**kw) != 0, kw
    assert b'field_match' in _lib.lib().edvr_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(table, ops.field_match(yuv, H, W, fmt))
    out = torch.zeros(2, fs, dtype=torch.uint8, device='cuda')
    pairs = torch.tensor([[1, 1], [0, 0]], dtype=torch.int32, device='cuda')
    good = dict(yuv=ptr(yuv), prev=None, out=ptr(out), table=ptr(pairs), n=2, k=2, H=H, W=W, sx=1, sy=0, depth=10, si=fs, so=fs, bff=0)
    call = lambda **kw: _lib.lib().edvr_field_weave(*{**good, **kw}.values(), stream)
    for kw in (dict(H=3), dict(W=0), dict(n=0), dict(k=0), dict(depth=7), dict(sx=0, sy=1), dict(yuv=None), dict(out=None), dict(table=None), dict(si=fs - 2),
               dict(so=fs - 2), dict(bff=-1)):
        assert call(**kw) != 0, kw
    assert b'field_weave' in _lib.lib().edvr_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.field_weave(yuv, H, W, fmt, frames=[1, 0], matches=[1, 0]))


def _compositions(n, sizes=(1, 2, 3, 4)):
    """Every way to cut n frames into pieces of the given sizes, as lists."""
    if n == 0:
        yield []
    for s in sizes:
        if s <= n:
            for rest in _compositions(n - s, sizes):
                yield [s] + rest


def _pieces_equal_the_whole(video, first, patterns, **kw):
    """y4m.inverse_telecined over every pattern of pieces against the restatement on the whole clip, stats included."""
    from edvr_amd import y4m
    H, W, fmt = U.FILM_H, U.FILM_W, '420'
    info = {}
    want = torch.from_numpy(T.inverse_telecine(video, H, W, fmt, first, info=info, **kw))
    stats_want = dict(film_matches=info['matches'], film_combed=[i for i, c in enumerate(info['combed']) if c], film_dropped=info['dropped'],
                      film_dropped_scores=[info['scores'][d] for d in info['dropped']])
    clip = _y4m_layout(video)
    for pattern in patterns:
        edges = np.cumsum([0] + list(pattern))
        assert edges[-1] == video.shape[0]
        stats = {}
        got = list(y4m.inverse_telecined((clip[a:b] for a, b in zip(edges, edges[1:])), H, W, fmt, first, stats=stats, **kw))
        assert all(g.shape[0] for g in got)
        assert torch.equal(torch.cat(got).cpu(), want), pattern
        assert stats == stats_want, pattern
    return want, info


def _uniform(n, s):
    return [s] * (n // s) + [n % s] * (n % s > 0)


@pytest.mark.parametrize('phase', range(6))
def test_inverse_telecined_for_every_piece_pattern(phase):
    """The telecined designed clip through y4m.inverse_telecined, against the restatement on the whole clip: phases 0 - 3 give the film
    frames themselves, phases 4 - 5 begin with the fallback.  Pieces of 1, 2, 3 and 4 frames, one piece, and mixed sizes on the whole
    clip (16 - 17 frames); and EVERY composition of its first 12 frames - two whole cycles and an open one - into pieces of 1 ... 4 frames (1490),
    which puts a piece edge at every place relative to a cycle's end, a p match and the fallback's neighbours.  (Every composition of
    17 frames would be 39648 runs per phase; the decisions alone are checked for every split of 17 rows in test_telecine_cpu.py.)"""
    first = 'top' if phase % 2 else 'bottom'
    film = U.film_clip()
    video, src = U.telecine(film, first, phase)
    n = video.shape[0]
    patterns = [_uniform(n, s) for s in (1, 2, 3, 4)] + [[n], [2, 3, 4, 1, 2, 3] + [n - 15], [4, 1, 1, 4, 3, n - 13], [1, n - 1], [n - 1, 1]]
    want, info = _pieces_equal_the_whole(video, first, patterns)
    shown = [src[2 * v] for v in range(n) if v not in info['dropped']]
    if phase in U.ORPHAN_FREE:
        assert info['combed'] == [False] * n and torch.equal(want, torch.from_numpy(film[shown]))
    else:
        assert info['combed'] == [True] + [False] * (n - 1) and 0 not in info['dropped']
        assert torch.equal(want[1:], torch.from_numpy(film[shown[1:]])) and not torch.equal(want[0], torch.from_numpy(film[shown[0]]))
    _pieces_equal_the_whole(video[:12], first, _compositions(12))
    _pieces_equal_the_whole(video, first, [_uniform(n, s) for s in (1, 3)] + [[n]], decimate=False)


def test_inverse_telecined_deep_format_and_thresholds():
    """A 10-bit 4:2:2 clip with noise of +-2 levels, and thresholds under which every frame is combed: all of it the fallback."""
    from edvr_amd import y4m
    H, W, fmt = U.FILM_H, U.FILM_W, '422p10'
    video, _ = U.telecine(U.film_clip(fmt=fmt), 'top', 3, fmt=fmt)
    video = U.add_noise(video, H, W, fmt, 2, seed=4)
    clip = _dev(video)
    for kw in (dict(), dict(mi=0, ct=0), dict(nt=0, mi=79)):
        want = torch.from_numpy(T.inverse_telecine(video, H, W, fmt, 'top', **kw))
        got = torch.cat(list(y4m.inverse_telecined((clip[a:a + 3] for a in range(0, video.shape[0], 3)), H, W, fmt, 'top', **kw)))
        assert torch.equal(got.cpu(), want), kw


def test_restore_y4m_film_like_the_composition_by_hand():
    """An It stream of the telecined clip (32 x 64 so that the tiny EDVR takes it) read 4 frames at a time, is - byte for byte - the
    restatement's film frames restored as a progressive stream at 4 / 5 of the rate; without decimation the rate stays; 'field' is what it
    was: ops.deinterlace and the progressive restore."""
    from edvr_amd import ops
    from edvr_amd.y4m import restore_y4m
    from test_gpu_yuv import _net
    net = _net()
    H, W = 32, 64
    film = U.film_clip(7, H, W)
    video, _ = U.telecine(film, 'top', 0, H, W)
    n = video.shape[0]
    assert n == 8
    woven = U.y4m_bytes(video, H, W, 'F30000:1001 It A1:1 C420jpeg')
    with torch.no_grad():
        for decimate, rate in ((True, '24000:1001'), (False, '30000:1001')):
            info = {}
            hand = T.inverse_telecine(video, H, W, '420', 'top', decimate=decimate, info=info)
            assert hand.shape[0] == (n - 1 if decimate else n)
            want = io.BytesIO()
            assert restore_y4m(net, io.BytesIO(U.y4m_bytes(hand, H, W, f'F{rate} Ip A1:1 C420jpeg')), want, read_frames=4, chunk=4) == hand.shape[0]
            got, stats = io.BytesIO(), {}
            assert restore_y4m(net, io.BytesIO(woven), got, read_frames=4, chunk=4, deinterlace='film', film_decimate=decimate, stats=stats) == hand.shape[0]
            head = f'YUV4MPEG2 W{4 * W} H{4 * H} F{rate} Ip A1:1 C420jpeg\nFRAME\n'.encode()
            assert got.getvalue().startswith(head)
            assert got.getvalue().count(b'FRAME\n') >= hand.shape[0] and len(got.getvalue()) == len(head) - 6 + hand.shape[0] * (6 + 16 * H * W * 3 // 2)
            assert got.getvalue() == want.getvalue()
            assert stats['frames'] == hand.shape[0] and stats['film_matches'] == info['matches'] and stats['film_dropped'] == info['dropped']
            assert stats['film_combed'] == []
        # a progressive stream passes through: the same bytes as without the argument
        prog = U.y4m_bytes(film, H, W, 'F24:1 Ip C420jpeg')
        a, b = io.BytesIO(), io.BytesIO()
        restore_y4m(net, io.BytesIO(prog), a, read_frames=4, chunk=4)
        restore_y4m(net, io.BytesIO(prog), b, read_frames=4, chunk=4, deinterlace='film')
        assert a.getvalue() == b.getvalue()
        with pytest.raises(ValueError, match='film_params'):
            restore_y4m(net, io.BytesIO(woven), io.BytesIO(), deinterlace='film', film_params={'nt': 2, 'cycle': 5})
        # 'field' makes the calls it made: the deinterlaced clip restored as a progressive stream at twice the rate
        fields = ops.deinterlace(_dev(video), H, W, '420', first='top', mode='field').cpu().numpy()
        want, got = io.BytesIO(), io.BytesIO()
        restore_y4m(net, io.BytesIO(U.y4m_bytes(fields, H, W, 'F60000:1001 Ip A1:1 C420jpeg')), want, read_frames=4, chunk=4)
        restore_y4m(net, io.BytesIO(woven), got, read_frames=4, chunk=4, deinterlace='field')
        assert got.getvalue() == want.getvalue()
    net.check_offsets()
