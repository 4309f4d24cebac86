"""GPU: letterbox / pillarbox bars, DESIGN 4.22 - ops.bar_profile (B1) and ops.yuv_crop (B7) against the NumPy restatement
(tests/bars_ref.py) and restore_y4m(crop=...) against the compositions by hand.  Every comparison is torch.equal / == on integers and
bytes: no tolerance appears anywhere."""
import ctypes
import io

import numpy as np
import pytest
import torch

import bars_ref as B
import deint_ref as D
import util_bars as UB
import util_yuv as U

pytestmark = pytest.mark.gpu

HEIGHTS = [4, 5, 7, 16, 17, 18, 33, 65]
WIDTHS = [1, 2, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513]
FILL = 0x5a


def _y4m_layout(frames):
    """The frames as `buf[:, 6:]` of a (n, 6 + framesize + 10) device buffer full of 0x5a: an over-read shows in the sums."""
    n, fs = frames.shape
    buf = torch.full((n, 6 + fs + 10), FILL, dtype=torch.uint8, device='cuda')
    buf[:, 6:6 + fs] = torch.from_numpy(frames).cuda()
    return buf, buf[:, 6:]


def _depth(fmt):
    return D.parse_format(fmt)[2]


# ---------------------------------------------------------------------------------------------------------------- bar_profile
@pytest.mark.parametrize('H', HEIGHTS)
def test_profile_on_random_frames(H):
    """Every width around the 16-sample run and the 256-column tile, every height around the 4-row wave and the 16-row tile; the format,
    the number of frames and the layout (dense / Y4M) cycle."""
    from edvr_amd import ops
    for k, W in enumerate(WIDTHS):
        case = HEIGHTS.index(H) * len(WIDTHS) + k
        fmt, n = UB.FORMATS[case % len(UB.FORMATS)], 1 + case % 3
        frames = UB.random_frames(n, H, W, fmt, seed=case)
        yuv = _y4m_layout(frames)[1] if case % 2 else torch.from_numpy(frames).cuda()
        got = ops.bar_profile(yuv, H, W, fmt)
        assert got.dtype == torch.int64 and got.shape == (n, H + W)
        assert torch.equal(got.cpu(), torch.from_numpy(B.profile(frames, H, W, fmt))), (H, W, fmt, n)


@pytest.mark.parametrize('H, W, fmt, fill', [
    (1100, 20, '420', None),        # tall and narrow: 69 row tiles of one column tile
    (17000, 20, '422', None),       # 1063 row tiles, more than the grid takes: a workgroup walks down several of them
    (4, 4100, '420p10', None),      # wide and short: 17 column tiles, the last one 4 columns wide
    (4, 65552, '444p16', 0xffff),   # a row sum of 65535 x 65552 > 2^32
    (65540, 2, '444p16', 0xffff),   # the column sums likewise; the workgroups walk
])
def test_profile_on_designed_shapes(H, W, fmt, fill):
    from edvr_amd import ops
    if fill is None:
        frames = UB.random_frames(1, H, W, fmt, seed=H)
    else:
        frames = D.join([np.full((1, r, c), fill, np.int64) for r, c in D.plane_shapes(H, W, fmt)], fmt)
    want = B.profile(frames, H, W, fmt)
    if fill is not None:
        assert want.max() > 1 << 32 and (want[0, :H] == fill * W).all() and (want[0, H:] == fill * H).all()
    got = ops.bar_profile(torch.from_numpy(frames).cuda(), H, W, fmt)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_profile_of_a_frame_does_not_depend_on_the_batch_and_out_is_honoured():
    from edvr_amd import ops
    H, W, fmt = 37, 300, '420p10'
    frames = UB.random_frames(5, H, W, fmt, seed=1)
    want = torch.from_numpy(B.profile(frames, H, W, fmt))
    buf, yuv = _y4m_layout(frames)
    whole = ops.bar_profile(yuv, H, W, fmt)
    assert torch.equal(whole.cpu(), want)
    for i in range(5):
        assert torch.equal(ops.bar_profile(yuv[i:i + 1], H, W, fmt)[0], whole[i])            # alone
    assert torch.equal(ops.bar_profile(yuv[1:4], H, W, fmt), whole[1:4])                     # a batch of 3, a slice of a longer buffer
    assert torch.equal(ops.bar_profile(torch.from_numpy(frames[2:5]).cuda(), H, W, fmt), whole[2:5])
    out = torch.full((5, H + W), -7, dtype=torch.int64, device='cuda')
    assert ops.bar_profile(yuv, H, W, fmt, out=out) is out and torch.equal(out, whole)       # cleared, then filled
    assert bool((buf[:, :6] == FILL).all()) and bool((buf[:, -10:] == FILL).all())


@pytest.mark.parametrize('fmt', UB.FORMATS)
def test_designed_clips_give_their_boxes(fmt):
    from edvr_amd import bars, ops
    H, W = 48, 64
    clip = [UB.letterbox(H, W, 8), UB.pillarbox(H, W, 12), UB.windowbox(H, W, 8, 12), None, (7, 39, 0, W)]
    frames = UB.designed_clip(clip, H, W, fmt, seed=4)
    table = ops.bar_profile(_y4m_layout(frames)[1], H, W, fmt)
    assert torch.equal(table.cpu(), torch.from_numpy(B.profile(frames, H, W, fmt)))
    assert bars.frame_boxes(table.cpu(), H, W, _depth(fmt)) == clip
    det = bars.BarDetector(H, W, _depth(fmt))
    det.push(table[:2].cpu())
    det.push(table[2:].cpu())
    assert det.boxes == clip and det.blank == [3]


# ---------------------------------------------------------------------------------------------------------------- yuv_crop
def _rects(fmt, H, W):
    """x0 in {0, step, 16, 18}; widths whose output rows are {1 step, 14, 16, 18, 34} bytes long where the format's steps allow that
    many samples and the next multiple of the step where they do not; the full frame."""
    sx, sy, depth = D.parse_format(fmt)
    step, bps = 1 << sx, 2 if depth > 8 else 1
    widths = sorted({step} | {-(-(nbytes // bps) // step) * step for nbytes in (14, 16, 18, 34)})
    out = [(2, x0, 6, w) for x0 in (0, step, 16, 18) for w in widths]
    return out + [(0, 0, H, W)]


@pytest.mark.parametrize('fmt', UB.FORMATS)
def test_crop_against_slicing(fmt):
    from edvr_amd import ops
    H, W, n = 14, 72, 3
    frames = UB.random_frames(n, H, W, fmt, seed=11)
    buf, yuv = _y4m_layout(frames)
    dense = torch.from_numpy(frames).cuda()
    for k, rect in enumerate(_rects(fmt, H, W)):
        want = torch.from_numpy(B.crop(frames, H, W, fmt, rect))
        got = ops.yuv_crop(yuv if k % 2 else dense, H, W, fmt, rect=rect)
        assert got.shape == (n, ops.yuv_frame_size(rect[2], rect[3], fmt)) and torch.equal(got.cpu(), want), (fmt, rect)
    # an odd frame (the chroma planes round up), a rect that ends on the last whole chroma sample; one frame
    Ho, Wo = 13, 71
    odd = UB.random_frames(1, Ho, Wo, fmt, seed=12)
    rect = (2, 18, 10, 52)
    assert torch.equal(ops.yuv_crop(torch.from_numpy(odd).cuda(), Ho, Wo, fmt, rect=rect).cpu(), torch.from_numpy(B.crop(odd, Ho, Wo, fmt, rect)))


@pytest.mark.parametrize('fmt', ['420', '422p10'])
def test_crop_into_a_y4m_buffer_leaves_the_rest_alone(fmt):
    from edvr_amd import ops
    H, W, n, rect = 14, 72, 3, (4, 18, 8, 34)
    frames = UB.random_frames(n, H, W, fmt, seed=13)
    want = torch.from_numpy(B.crop(frames, H, W, fmt, rect))
    fs = want.shape[1]
    out = torch.full((n, 6 + fs + 10), FILL, dtype=torch.uint8, device='cuda')
    assert ops.yuv_crop(_y4m_layout(frames)[1], H, W, fmt, rect=rect, out=out[:, 6:]).data_ptr() == out[:, 6:].data_ptr()
    assert torch.equal(out[:, 6:6 + fs].cpu(), want)
    assert bool((out[:, :6] == FILL).all()) and bool((out[:, 6 + fs:] == FILL).all())


def test_errors_before_any_launch(monkeypatch):
    from edvr_amd import _lib, ops
    seen = []
    monkeypatch.setattr(ops, 'LAUNCH_HOOK', lambda name, flops, launch, nbytes, executed=None: (seen.append((name, nbytes)), launch()))
    H, W = 12, 20
    fs = ops.yuv_frame_size(H, W)
    yuv = torch.randint(0, 256, (2, fs), dtype=torch.uint8, device='cuda')
    store = torch.zeros(8 * (H + W) + fs, dtype=torch.uint8, device='cuda')  # a table and a frame that share bytes
    wide = torch.zeros(2, 2 * fs + 2, dtype=torch.uint8, device='cuda')
    for bad, kw in ((yuv.cpu(), {}), (yuv.float(), {}), (yuv, dict(out=torch.zeros(2, H + W, dtype=torch.int64))),
                    (yuv, dict(out=torch.zeros(2, H + W, dtype=torch.int32, device='cuda')))):
        with pytest.raises(NotImplementedError):
            ops.bar_profile(bad, H, W, **kw)
    for bad, fmt, kw in ((yuv, '411', {}), (yuv, 420, {}), (yuv[0], '420', {}), (yuv[:, :-1], '420', {}), (yuv[:0], '420', {}), (wide[:, ::2], '420', {}),
                         (wide[:, 1:], '420p10', {}), (yuv, '444', {}), (yuv, '420', dict(out=torch.zeros(2, H + W + 1, dtype=torch.int64, device='cuda'))),
                         (yuv, '420', dict(out=torch.zeros(3, H + W, dtype=torch.int64, device='cuda'))),
                         (yuv, '420', dict(out=torch.zeros(2, 2 * (H + W), dtype=torch.int64, device='cuda')[:, ::2])),
                         (store[None, :fs], '420', dict(out=store[:8 * (H + W)].view(torch.int64)[None]))):
        with pytest.raises(ValueError):
            ops.bar_profile(bad, H, W, fmt, **kw)
    with pytest.raises(ValueError):
        ops.bar_profile(yuv, 0, W)
    with pytest.raises(NotImplementedError):
        ops.yuv_crop(yuv.cpu(), H, W, rect=(0, 0, 4, 4))
    with pytest.raises(NotImplementedError):
        ops.yuv_crop(yuv, H, W, rect=(0, 0, 4, 4), out=torch.zeros(2, 24, dtype=torch.uint8))
    small = ops.yuv_frame_size(4, 8)
    for fmt, kw in (('411', dict(rect=(0, 0, 4, 8))), ('420', dict(rect=(0, 0, 4))), ('420', dict(rect='auto')), ('420', dict(rect=(0, 0, 0, 8))),
                    ('420', dict(rect=(0, 0, 4, 0))), ('420', dict(rect=(-2, 0, 4, 8))), ('420', dict(rect=(10, 0, 4, 8))), ('420', dict(rect=(0, 14, 4, 8))),
                    ('420', dict(rect=(1, 0, 4, 8))), ('420', dict(rect=(0, 1, 4, 8))), ('420', dict(rect=(0, 0, 3, 8))), ('420', dict(rect=(0, 0, 4, 7))),
                    ('420', dict(rect=(0.0, 0, 4, 8))),
                    ('420', dict(rect=(0, 0, 4, 8), out=torch.zeros(3, small, dtype=torch.uint8, device='cuda'))),
                    ('420', dict(rect=(0, 0, 4, 8), out=torch.zeros(2, small - 1, dtype=torch.uint8, device='cuda'))),
                    ('420', dict(rect=(0, 0, 4, 8), out=torch.zeros(2, 2 * small, dtype=torch.uint8, device='cuda')[:, ::2])),
                    ('420', dict(rect=(0, 0, 4, 8), out=yuv[:, :small])), ('420', dict(rect=(0, 0, 4, 8), out=yuv[:, fs - small:]))):
        with pytest.raises(ValueError):
            ops.yuv_crop(yuv, H, W, fmt, **kw)
    with pytest.raises(ValueError):
        ops.yuv_crop(yuv[0], H, W, rect=(0, 0, 4, 8))
    # 4:2:2 has no row step: an odd y0 and h are fine there, an odd x0 is not
    y422 = torch.zeros(1, ops.yuv_frame_size(H, W, '422'), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError):
        ops.yuv_crop(y422, H, W, '422', rect=(1, 1, 3, 8))
    assert seen == []
    assert ops.yuv_crop(y422, H, W, '422', rect=(1, 2, 3, 8)).shape == (1, ops.yuv_frame_size(3, 8, '422'))
    assert ops.bar_profile(yuv, H, W).shape == (2, H + W)
    assert seen == [('yuv_crop', 2.0 * 48), ('bar_profile', 2.0 * (H * W + 8 * (H + W)))]
    # the C ABI refuses what the Python layer never sends
    table = torch.zeros(2, H + W, dtype=torch.int64, device='cuda')
    out = torch.zeros(2, small, dtype=torch.uint8, device='cuda')
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(yuv=ptr(yuv), table=ptr(table), n=2, H=H, W=W, sx=1, sy=1, depth=8, stride=fs)
    for kw in (dict(yuv=ptr(None)), dict(table=ptr(None)), dict(n=0), dict(n=32768), dict(H=0), dict(W=0), dict(sx=0, sy=1), dict(sx=2), dict(depth=7),
               dict(depth=17), dict(stride=fs - 1), dict(depth=10, stride=2 * fs + 1), dict(H=1 << 15, W=1 << 15)):
        assert _lib.lib().edvr_bar_profile(*{**good, **kw}.values(), stream) != 0, kw
    assert b'bar_profile' in _lib.lib().edvr_last_error()
    good = dict(yuv=ptr(yuv), out=ptr(out), n=2, H=H, W=W, sx=1, sy=1, depth=8, stride=fs, out_stride=small, y0=2, x0=4, h=4, w=8)
    for kw in (dict(yuv=ptr(None)), dict(out=ptr(None)), dict(n=0), dict(H=0), dict(sx=0, sy=1), dict(depth=17), dict(stride=fs - 1), dict(out_stride=small - 1),
               dict(y0=-2), dict(x0=-2), dict(h=0), dict(w=0), dict(y0=10), dict(x0=14), dict(y0=1), dict(x0=1), dict(h=3), dict(w=7), dict(h=1 << 30)):
        assert _lib.lib().edvr_yuv_crop(*{**good, **kw}.values(), stream) != 0, kw
    assert b'yuv_crop' in _lib.lib().edvr_last_error()
    assert _lib.lib().edvr_yuv_crop(*good.values(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.yuv_crop(yuv, H, W, rect=(2, 4, 4, 8)))


# ---------------------------------------------------------------------------------------------------------------- restore_y4m
EH, EW, ERECT, ETAGS = 48, 64, (8, 0, 32, 64), 'F25:1 Ip A16:15 C420jpeg'
_E2E = {}


def _clip(boxes, seed):
    return UB.designed_clip(boxes, EH, EW, '420', seed=seed)


def _restore(data, **kw):
    from edvr_amd.y4m import restore_y4m
    from test_gpu_yuv import _net
    out, stats = io.BytesIO(), {}
    with torch.no_grad():
        n = restore_y4m(_net(), io.BytesIO(data), out, read_frames=4, chunk=4, stats=stats, **kw)
    return n, out.getvalue(), stats


def _letterboxed():
    """6 frames of 48 x 64 with 8-row bars, and what restore_y4m writes for the 32 x 64 stream cropped by hand: computed once."""
    if not _E2E:
        frames = _clip([UB.letterbox(EH, EW, 8)] * 6, seed=21)
        by_hand = B.crop(frames, EH, EW, '420', ERECT)
        n, want, _ = _restore(UB.y4m_bytes(by_hand, 32, 64, ETAGS))
        assert n == 6 and want.startswith(b'YUV4MPEG2 W256 H128 F25:1 Ip A16:15 C420jpeg\nFRAME\n')
        _E2E.update(frames=frames, want=want)
    return _E2E['frames'], _E2E['want']


def test_restore_y4m_auto_and_rect_equal_the_stream_cropped_by_hand():
    from test_gpu_yuv import _net
    frames, want = _letterboxed()
    data = UB.y4m_bytes(frames, EH, EW, ETAGS)
    n, got, stats = _restore(data, crop='auto', crop_probe=4)
    assert n == 6 and got == want
    assert stats['crop'] == ERECT and stats['crop_box'] == (8, 40, 0, 64) and stats['bars_blank'] == [] and stats['bars_outside'] == []
    n, got, stats = _restore(data, crop=ERECT)
    assert n == 6 and got == want and stats['crop'] == ERECT
    n, got, stats = _restore(data)  # crop=None: 192 x 256, as before the argument
    assert n == 6 and got.startswith(b'YUV4MPEG2 W256 H192 F25:1 Ip A16:15 C420jpeg\nFRAME\n') and 'crop' not in stats
    _net().check_offsets()


def test_restore_y4m_crops_after_deinterlacing_and_before_the_delivery_size():
    """The stages compose: an It stream is deinterlaced at field rate, the bars are found on the progressive frames and dropped, the
    picture is restored and resampled - against the same composition by hand, detection included."""
    from edvr_amd import VideoRestorer, bars, ops
    from edvr_amd.y4m import fit_size
    from test_gpu_yuv import _net
    net = _net()
    frames, _ = _letterboxed()
    woven = UB.y4m_bytes(frames[:4], EH, EW, 'F25:1 It A16:15 C420jpeg')
    with torch.no_grad():
        prog = ops.deinterlace(torch.from_numpy(frames[:4]).cuda(), EH, EW, '420', first='top', mode='field')
        boxes = bars.frame_boxes(ops.bar_profile(prog, EH, EW, '420').cpu(), EH, EW, 8)
        rect = bars.aligned_rect(bars.video_box(boxes), EH, EW, (2, 2), (4, 4))
        assert rect is not None and rect[2] < EH and rect[3] == EW  # there is something to crop
        small = ops.yuv_crop(prog, EH, EW, '420', rect=rect)
        restored = VideoRestorer(net, out_dtype=torch.float32, chunk=4).restore(ops.yuv420_to_rgb(small, rect[2], rect[3], 'bt601', 'limited', 'bilinear'))
        want = UB.y4m_bytes(ops.rgb_to_yuv420(restored, 'bt601', 'limited').cpu().numpy(), 4 * rect[2], 4 * rect[3], 'F50:1 Ip A16:15 C420jpeg')
        Hd, Wd, aspect = fit_size(4 * rect[2], 4 * rect[3], '16:15', height=96, square=True)
        assert (Hd, Wd, aspect) != fit_size(4 * EH, 4 * EW, '16:15', height=96, square=True)  # the cropped size is what is fitted
        delivered = ops.resample(restored, (Hd, Wd))
        want_fit = UB.y4m_bytes(ops.rgb_to_yuv420(delivered, 'bt601', 'limited').cpu().numpy(), Hd, Wd, f'F50:1 Ip A{aspect} C420jpeg')
    n, got, stats = _restore(woven, deinterlace='field', crop='auto', crop_probe=4)
    assert n == 8 and stats['crop'] == rect and got == want
    n, got, stats = _restore(woven, deinterlace='field', crop=rect, out_height=96, square_pixels=True)
    assert n == 8 and got == want_fit
    net.check_offsets()


def test_restore_y4m_probe_skips_blank_frames_and_reports_a_growing_picture():
    from test_gpu_yuv import _net
    frames, want = _letterboxed()
    # four blank frames in front: the rect is found on the frames behind them, and the stream is that of the hand-cropped frames
    blank = _clip([None] * 4, seed=22)
    n, got, stats = _restore(UB.y4m_bytes(np.concatenate([blank, frames[:4]]), EH, EW, ETAGS), crop='auto', crop_probe=4)
    _, by_hand, _ = _restore(UB.y4m_bytes(B.crop(np.concatenate([blank, frames[:4]]), EH, EW, '420', ERECT), 32, 64, ETAGS))
    assert n == 8 and got == by_hand and stats['crop'] == ERECT and stats['bars_blank'] == [0, 1, 2, 3] and stats['bars_outside'] == []
    # the picture grows after the probe: cropped as decided, and reported
    grown = _clip([UB.letterbox(EH, EW, 2)] * 3, seed=23)
    n, got, stats = _restore(UB.y4m_bytes(np.concatenate([frames[:4], grown]), EH, EW, ETAGS), crop='auto', crop_probe=4)
    assert n == 7 and got.startswith(b'YUV4MPEG2 W256 H128 ') and stats['crop'] == ERECT and stats['bars_outside'] == [4, 5, 6]
    _net().check_offsets()
