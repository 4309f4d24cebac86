"""GPU: ops.deinterlace (csrc/deint.hip) against the NumPy restatement of DESIGN 4.19 (tests/deint_ref.py), exactly, on the smallest shapes
that reach every branch - planes of 2 and 3 rows (the repeated row reflection), widths below one lane's run, at the lane-run tail, at the
block tail and wide enough for the whole-segment accesses, bytes and words, every subsampling, 1 ... 3 frames with and without context
frames, both field orders, both modes, Y4M-layout and dense buffers on either side; the error paths; and restore_y4m(deinterlace=...)
through a tiny EDVR against the composition done by hand."""
import ctypes
import io

import numpy as np
import pytest
import torch

import deint_ref as D
import util_deint as U

pytestmark = pytest.mark.gpu

FORMATS = ['420', '422', '444', '420p10', '444p16']
HEIGHTS = [4, 5, 7, 18]
WIDTHS = [1, 2, 5, 63, 64, 65, 257]
CONTEXTS = [(False, False), (True, True), (True, False), (False, True)]


def _y4m_layout(frames):
    """The frames as `buf[:, 6:]` of a Y4M read buffer on the device: rows 6 + framesize apart, 6 bytes in."""
    buf = torch.full((frames.shape[0], 6 + frames.shape[1]), 0x5a, dtype=torch.uint8, device='cuda')
    buf[:, 6:] = torch.from_numpy(frames).cuda()
    return buf[:, 6:]


def _check(frames, H, W, fmt, first, mode, prev=None, nxt=None, y4m_in=False, y4m_out=False):
    from edvr_amd import ops
    want = D.deinterlace(frames, H, W, fmt, first, mode, prev=prev, nxt=nxt)
    yuv = _y4m_layout(frames) if y4m_in else torch.from_numpy(frames).cuda()
    kw = dict(first=first, mode=mode, prev=None if prev is None else torch.from_numpy(prev).cuda(),
              next=None if nxt is None else torch.from_numpy(nxt).cuda()[None])
    if y4m_out:
        buf = torch.full((want.shape[0], 6 + want.shape[1] + 2), 0xa5, dtype=torch.uint8, device='cuda')
        got = ops.deinterlace(yuv, H, W, fmt, out=buf[:, 6:6 + want.shape[1]], **kw)
        assert got.data_ptr() == buf.data_ptr() + 6
        assert bool((buf[:, :6] == 0xa5).all()) and bool((buf[:, 6 + want.shape[1]:] == 0xa5).all())  # nothing outside the frames is written
    else:
        got = ops.deinterlace(yuv, H, W, fmt, **kw)
    assert got.shape == want.shape and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (H, W, fmt, first, mode, prev is not None, nxt is not None, y4m_in, y4m_out)


@pytest.mark.parametrize('W', WIDTHS)
@pytest.mark.parametrize('H', HEIGHTS)
def test_random_frames_match_the_definition(H, W):
    """Every (H, W); format, frame count, context and layout cycle with periods 5, 3, 4 and 2 over the 28 shapes, so each value of each
    meets small and large shapes; both field orders and both modes on every one."""
    i = HEIGHTS.index(H) * len(WIDTHS) + WIDTHS.index(W)
    fmt, n, (has_prev, has_next) = FORMATS[i % 5], 1 + i % 3, CONTEXTS[(i // 2) % 4]
    frames = U.random_frames(n, H, W, fmt, seed=1000 + i)
    ctx = U.random_frames(2, H, W, fmt, seed=2000 + i)
    for first in ('top', 'bottom'):
        for mode in ('field', 'frame'):
            _check(frames, H, W, fmt, first, mode, ctx[0] if has_prev else None, ctx[1] if has_next else None, y4m_in=i % 2 == 0,
                   y4m_out=(i // 3) % 2 == 0)


@pytest.mark.parametrize('fmt', FORMATS)
def test_every_format_on_every_path(fmt):
    """Each format where its planes are wide enough for whole-segment lanes and block tails (18 x 257; chroma 129 wide where
    subsampled), odd (7 x 65) and narrower than a lane's window everywhere (5 x 5), with n = 1, 2, 3 and every context pattern."""
    for H, W, n in ((18, 257, 2), (7, 65, 3), (5, 5, 1)):
        frames = U.random_frames(n, H, W, fmt, seed=H * W + n)
        ctx = U.random_frames(2, H, W, fmt, seed=H * W)
        for c, (has_prev, has_next) in enumerate(CONTEXTS):
            _check(frames, H, W, fmt, 'top' if c % 2 else 'bottom', 'field', ctx[0] if has_prev else None, ctx[1] if has_next else None,
                   y4m_in=c < 2, y4m_out=c % 2 == 0)
        _check(frames, H, W, fmt, 'top', 'frame', ctx[0], ctx[1], y4m_in=True, y4m_out=True)


@pytest.mark.parametrize('first', ['top', 'bottom'])
def test_the_structured_clip(first):
    """The moving bar beside the static texture, on which the restatement takes every direction of D4 and every state of D6's clamp
    (asserted in test_deinterlace_cpu.py)."""
    frames = U.structured_clip(3, 18, 65, '420', first)
    for mode in ('field', 'frame'):
        _check(frames, 18, 65, '420', first, mode, y4m_in=True)
    _check(U.structured_clip(3, 18, 65, '422p10', first), 18, 65, '422p10', first, 'field')


@pytest.mark.parametrize('fmt, H, W', [('444p16', 6, 37), ('420', 7, 18), ('420p10', 4, 64)])
def test_the_extremes(fmt, H, W):
    """All 0, all M and the fields alternately 0 / M: 65535 + 65535 does not wrap, and the output stays a sample."""
    for clip in U.extreme_clips(3, H, W, fmt):
        for first in ('top', 'bottom'):
            _check(clip, H, W, fmt, first, 'field')
            _check(clip, H, W, fmt, first, 'field', prev=clip[1], nxt=clip[0], y4m_in=True)


@pytest.mark.parametrize('fmt, H, W', [('420', 18, 65), ('422p10', 7, 64)])
def test_a_frame_does_not_depend_on_its_place_in_the_batch(fmt, H, W):
    """Any split of a clip with its neighbours' frames as context gives the whole clip's frames - device against device."""
    from edvr_amd import ops
    n = 5
    clip = torch.from_numpy(U.random_frames(n, H, W, fmt, seed=77)).cuda()
    for mode in ('field', 'frame'):
        whole = ops.deinterlace(clip, H, W, fmt, first='bottom', mode=mode)
        per = 2 if mode == 'field' else 1
        for lo, hi in ((0, 1), (1, 2), (4, 5), (1, 4), (2, 5), (0, 3)):
            part = ops.deinterlace(clip[lo:hi], H, W, fmt, first='bottom', mode=mode, prev=clip[lo - 1] if lo else None, next=clip[hi] if hi < n else None)
            assert torch.equal(part, whole[per * lo:per * hi]), (mode, lo, hi)


def test_deinterlaced_pieces_on_the_device():
    from edvr_amd import ops, y4m
    n, H, W, fmt = 8, 6, 21, '420'
    clip = _y4m_layout(U.random_frames(n, H, W, fmt, seed=3))
    whole = ops.deinterlace(clip, H, W, fmt, first='top', mode='field')
    for pattern in ([1] * n, [n], [3, 1, 4], [1, n - 1]):
        edges = np.cumsum([0] + pattern)
        got = torch.cat(list(y4m.deinterlaced((clip[a:b] for a, b in zip(edges, edges[1:])), H, W, fmt, 'top', 'field')))
        assert torch.equal(got, whole), pattern


def test_errors():
    from edvr_amd import _lib, ops
    H, W, fmt = 6, 10, '422p10'
    fs = D.frame_size(H, W, fmt)
    yuv = torch.from_numpy(U.random_frames(2, H, W, fmt, seed=1)).cuda()
    with pytest.raises(NotImplementedError):
        ops.deinterlace(yuv.cpu(), H, W, fmt)
    with pytest.raises(NotImplementedError):
        ops.deinterlace(yuv.float(), H, W, fmt)
    with pytest.raises(NotImplementedError):
        ops.deinterlace(yuv, H, W, fmt, prev=yuv[0].cpu())
    with pytest.raises(NotImplementedError):
        ops.deinterlace(yuv, H, W, fmt, out=torch.zeros(4, fs, device='cuda'))
    for kw in (dict(format='411'), dict(format='420p8'), dict(first='left'), dict(first=0), dict(mode='bob'), dict(mode=None)):
        with pytest.raises(ValueError):
            ops.deinterlace(yuv, H, W, **{'format': fmt, **kw})
    for h in (3, 2, 0):
        with pytest.raises(ValueError, match='4 rows'):
            ops.deinterlace(yuv, h, W, '420')
    with pytest.raises(ValueError):
        ops.deinterlace(yuv, H, 0, '420')
    with pytest.raises(ValueError):
        ops.deinterlace(yuv.view(-1), H, W, fmt)
    with pytest.raises(ValueError, match='shorter'):
        ops.deinterlace(yuv[:, :fs - 2], H, W, fmt)
    with pytest.raises(ValueError, match='stride'):
        ops.deinterlace(torch.zeros(2, 2 * fs, dtype=torch.uint8, device='cuda')[:, ::2], H, W, fmt)
    flat = torch.zeros(4 * fs + 2, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='even'):
        ops.deinterlace(flat[1:1 + 2 * fs].view(2, fs), H, W, fmt)
    with pytest.raises(ValueError, match='even'):
        ops.deinterlace(yuv, H, W, fmt, out=flat[1:1 + 4 * fs].view(4, fs))
    with pytest.raises(ValueError, match='even'):
        ops.deinterlace(yuv, H, W, fmt, prev=flat[1:1 + fs])
    ops.deinterlace(flat[1:1 + 2 * D.frame_size(H, W, '422')].view(2, -1), H, W, '422')  # bytes may lie anywhere
    with pytest.raises(ValueError):
        ops.deinterlace(yuv, H, W, fmt, out=torch.zeros(2, fs, dtype=torch.uint8, device='cuda'))  # 'field' makes 4
    with pytest.raises(ValueError):
        ops.deinterlace(yuv, H, W, fmt, mode='frame', out=torch.zeros(4, fs, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='shorter'):
        ops.deinterlace(yuv, H, W, fmt, out=torch.zeros(4, fs - 2, dtype=torch.uint8, device='cuda'))
    for bad in (yuv[0, :fs - 2], yuv, yuv[:, :4]):
        with pytest.raises(ValueError, match='one frame'):
            ops.deinterlace(yuv, H, W, fmt, next=bad)
    both = torch.zeros(6, fs, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='overlaps'):
        ops.deinterlace(both[:2], H, W, fmt, out=both[1:5])
    with pytest.raises(ValueError, match='overlaps'):
        ops.deinterlace(both[:1], H, W, fmt, next=both[3], out=both[2:6:2])
    # the C ABI refuses what the Python layer never sends
    out = torch.zeros(4, fs, dtype=torch.uint8, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    f = _lib.lib().edvr_deinterlace
    good = dict(yuv=ptr(yuv), prev=None, next=None, out=ptr(out), n=2, H=H, W=W, sx=1, sy=0, depth=10, si=fs, so=fs, bff=0, rate=1)
    call = lambda **kw: f(*{**good, **kw}.values(), stream)
    for kw in (dict(H=3), dict(H=0), dict(W=0), dict(n=0), dict(n=-1), dict(depth=7), dict(depth=17), dict(sx=0, sy=1), dict(sx=2), dict(yuv=None), dict(out=None),
               dict(yuv=ptr(yuv, 1)), dict(out=ptr(out, 1)), dict(prev=ptr(yuv, 1)), dict(next=ptr(yuv, 1)), dict(si=fs + 1), dict(so=fs + 1), dict(si=fs - 2),
               dict(so=fs - 2), dict(bff=2), dict(rate=-1)):
        assert call(**kw) != 0, kw
    assert b'deinterlace' in _lib.lib().edvr_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.deinterlace(yuv, H, W, fmt))


def test_restore_y4m_deinterlaces_like_the_composition_by_hand():
    """An It stream of 6 frames of 16 x 32 through a tiny EDVR, read 4 frames at a time, is - byte for byte - ops.deinterlace on the
    whole clip followed by restore_y4m of that as a progressive stream at twice the rate."""
    from edvr_amd import ops
    from edvr_amd.y4m import Y4MReader, restore_y4m
    from test_gpu_yuv import _net
    net = _net()
    n, H, W = 6, 16, 32
    frames = U.structured_clip(n, H, W, '420', 'top')
    woven = U.y4m_bytes(frames, H, W, 'F25:1 It A1:1 C420jpeg')
    with torch.no_grad():
        prog = ops.deinterlace(torch.from_numpy(frames).cuda(), H, W, '420', first='top', mode='field').cpu().numpy()
        want = io.BytesIO()
        assert restore_y4m(net, io.BytesIO(U.y4m_bytes(prog, H, W, 'F50:1 Ip A1:1 C420jpeg')), want, read_frames=4, chunk=4) == 2 * n
        got = io.BytesIO()
        assert restore_y4m(net, io.BytesIO(woven), got, read_frames=4, chunk=4, deinterlace='field') == 2 * n
        with pytest.raises(ValueError, match='deinterlace first'):
            restore_y4m(net, io.BytesIO(woven), io.BytesIO(), read_frames=4, chunk=4)
    net.check_offsets()
    assert got.getvalue().startswith(f'YUV4MPEG2 W{4 * W} H{4 * H} F50:1 Ip A1:1 C420jpeg\nFRAME\n'.encode())
    assert got.getvalue() == want.getvalue()
    assert Y4MReader(io.BytesIO(woven), interlaced=True).interlace == 't'
