"""CPU: letterbox / pillarbox bars, DESIGN 4.22 - the host arithmetic of edvr_amd/bars.py (B2 - B6) against the NumPy restatement
(tests/bars_ref.py) and on designed clips, the properties of the aligned rect, the streaming BarDetector, the flow of restore_y4m with CPU
stand-ins for the device pieces (ops.bar_profile / ops.yuv_crop stood in by the restatement), and the flags of the two scripts.  Every
comparison is == on integers and bytes."""
import importlib.util
import io
import os
import random

import numpy as np
import pytest
import torch

import bars_ref as B
import util_bars as UB
import util_yuv as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- bars.py
@pytest.mark.parametrize('depth', [8, 10, 16])
def test_boxes_against_the_restatement_on_random_tables(depth):
    """Tables whose sums scatter around the dark bound, exact ties included, with runs of dark rows and columns at both ends."""
    from edvr_amd import bars
    rng = np.random.default_rng(depth)
    for case in range(60):
        H, W, n = int(rng.integers(1, 24)), int(rng.integers(1, 24)), int(rng.integers(1, 6))
        limit = int(rng.integers(0, 256))
        level = limit << (depth - 8)
        table = np.empty((n, H + W), np.int64)
        for i in range(n):
            for at, N, other in ((0, H, W), (H, W, H)):
                bound = level * other
                v = bound + rng.integers(-3, 4, size=N)  # around the bound: <= is dark, ties are dark
                lead, trail = int(rng.integers(0, N + 1)), int(rng.integers(0, N + 1))
                v[:lead] = bound - rng.integers(0, 3, size=lead)
                v[N - trail:] = bound - rng.integers(0, 3, size=trail)
                table[i, at:at + N] = np.maximum(v, 0)
        want = B.frame_boxes(table, H, W, depth, limit)
        assert bars.frame_boxes(table, H, W, depth, limit) == want
        assert bars.frame_boxes(torch.from_numpy(table), H, W, depth, limit) == want  # a tensor, an array or lists
        assert bars.frame_boxes(table.tolist(), H, W, depth, limit) == want
        assert bars.video_box(want) == B.video_box(want)
        box = B.video_box(want)
        for step, m, g, mb in (((2, 2), (4, 4), 0, 8), ((1, 2), (4, 4), 1, 0), ((1, 1), (1, 1), 0, 3), ((2, 2), (16, 16), 2, 8)):
            assert bars.aligned_rect(box, H, W, step, m, g, mb) == B.aligned_rect(box, H, W, step, m, g, mb)


def _rect_of(frames, H, W, fmt, step, multiple, **kw):
    from edvr_amd import bars
    depth = 8 if 'p' not in fmt else int(fmt.split('p')[1])
    boxes = bars.frame_boxes(B.profile(frames, H, W, fmt), H, W, depth)
    return boxes, bars.aligned_rect(bars.video_box(boxes), H, W, step, multiple, **kw)


@pytest.mark.parametrize('fmt', UB.FORMATS)
def test_designed_boxes(fmt):
    """Letterbox, pillarbox and windowbox clips give the boxes they were built with, at every depth."""
    H, W = 48, 64
    for box in (UB.letterbox(H, W, 8), UB.pillarbox(H, W, 12), UB.windowbox(H, W, 8, 12)):
        frames = UB.designed_clip([box] * 3, H, W, fmt, seed=1)
        boxes, rect = _rect_of(frames, H, W, fmt, (1, 1), (1, 1))
        assert boxes == [box] * 3
        assert rect == (box[0], box[2], box[1] - box[0], box[3] - box[2])


def test_designed_alignment_and_belief():
    from edvr_amd import bars
    H, W = 48, 64
    # bars of odd height on 4:2:0: 7 rows at the top, 9 at the bottom -> the rect moves inward to rows [8, 38) and then to a multiple of 4
    boxes, rect = _rect_of(UB.designed_clip([(7, 39, 0, W)] * 2, H, W, '420'), H, W, '420', (2, 2), (2, 2))
    assert boxes == [(7, 39, 0, W)] * 2 and rect == (8, 0, 30, W)
    assert bars.aligned_rect((7, 39, 0, W), H, W, (2, 2), (4, 4)) == (8, 0, 28, W)      # len0 = 30 -> 28, the spare 2 rows: floor(2 / 4) * 2 = 0
    assert bars.aligned_rect((7, 39, 0, W), H, W, (2, 2), (16, 16)) is None             # 16 rows of 48: under half the frame
    assert bars.aligned_rect((6, 44, 0, W), H, W, (2, 2), (16, 16)) == (8, 0, 32, W)    # len0 = 38 -> 32, spare 6: floor(6 / 4) * 2 = 2
    # a bar of min_bar - 1 rows is kept: the axis keeps its whole length
    assert bars.aligned_rect((7, H, 0, W), H, W, 1, 1) == (0, 0, H, W)
    assert bars.aligned_rect((8, H, 0, W), H, W, 1, 1) == (8, 0, H - 8, W)
    assert bars.aligned_rect((4, H - 3, 0, W), H, W, 1, 1) == (0, 0, H, W)   # 7 in total
    assert bars.aligned_rect((4, H - 4, 0, W), H, W, 1, 1) == (4, 0, H - 8, W)
    assert bars.aligned_rect((0, H, 3, W), H, W, 1, 1, min_bar=3) == (0, 3, H, W - 3)
    # blank frames are ignored; an all-blank video has no box and no rect
    frames = UB.designed_clip([None, UB.letterbox(H, W, 8), None, UB.letterbox(H, W, 10)], H, W, '420')
    boxes, rect = _rect_of(frames, H, W, '420', (2, 2), (4, 4))
    assert boxes == [None, (8, 40, 0, W), None, (10, 38, 0, W)] and rect == (8, 0, 32, W)
    boxes, rect = _rect_of(UB.designed_clip([None] * 3, H, W, '420'), H, W, '420', (2, 2), (4, 4))
    assert boxes == [None] * 3 and bars.video_box(boxes) is None and rect is None
    # a box under half the frame is not believed
    assert bars.aligned_rect((13, 36, 0, W), H, W, 1, 1) is None and bars.aligned_rect((12, 36, 0, W), H, W, 1, 1) == (12, 0, 24, W)
    assert bars.aligned_rect((0, H, 20, 51), H, W, 1, 1) is None
    # the margin is applied only on sides that have a bar
    assert bars.aligned_rect((8, H, 0, W), H, W, 1, 1, margin=2) == (10, 0, H - 10, W)
    assert bars.aligned_rect((8, 40, 10, W), H, W, 1, 1, margin=3) == (11, 13, 26, W - 13)
    assert bars.aligned_rect((0, 40, 0, 54), H, W, 1, 1, margin=1) == (0, 0, 39, 53)


def test_aligned_rect_properties():
    """Over random (box, step, multiple, margin): the rect lies inside the box (after the margin), on the steps, its lengths are multiples
    of m, and it is maximal - fewer than m samples of the aligned box are left over."""
    from edvr_amd import bars
    rnd = random.Random(7)
    seen = 0
    for _ in range(6000):
        H, W = rnd.randint(40, 200), rnd.randint(40, 200)
        sy, sx = rnd.choice([(1, 1), (1, 2), (2, 2)])
        k = rnd.choice([1, 2, 4, 8, 16])
        my, mx = sy * k // np.gcd(sy, k), sx * k // np.gcd(sx, k)
        g = rnd.choice([0, 0, 1, 2, 5])
        t, l = rnd.randint(0, H // 4), rnd.randint(0, W // 4)  # boxes of more than half the frame: most are believed
        b, r = rnd.randint(H - H // 4, H), rnd.randint(W - W // 4, W)
        rect = bars.aligned_rect((t, b, l, r), H, W, (sy, sx), (int(my), int(mx)), g, 0)  # min_bar 0: B5 alone (and the half-frame rule)
        assert rect == B.aligned_rect((t, b, l, r), H, W, (sy, sx), (int(my), int(mx)), g, 0)
        if rect is None:
            continue
        seen += 1
        for o, length, lo, hi, N, s, m in ((rect[0], rect[2], t, b, H, sy, int(my)), (rect[1], rect[3], l, r, W, sx, int(mx))):
            lo, hi = lo + (g if lo > 0 else 0), hi - (g if hi < N else 0)
            a, len0, _, _ = B.axis(lo, hi, N, s, m)
            assert lo <= o and o + length <= hi         # inside the box
            assert o % s == 0 and length % m == 0       # on the steps, a multiple of m (a multiple of the step)
            assert 0 <= len0 - length < m               # maximal
            assert 2 * length >= N
    assert seen > 3000


def test_aligned_rect_and_check_rect_errors():
    from edvr_amd import bars
    for kw in (dict(step=0), dict(step=(2, 2), multiple=(3, 4)), dict(margin=-1), dict(min_bar=-1), dict(step=(1, 2, 3)), dict(margin=1.5)):
        with pytest.raises(ValueError):
            bars.aligned_rect((0, 8, 0, 8), 8, 8, **kw)
    for box in ((0, 9, 0, 8), (4, 4, 0, 8), (-1, 8, 0, 8), (0, 8, 5, 3)):
        with pytest.raises(ValueError):
            bars.aligned_rect(box, 8, 8)
    assert bars.check_rect([2, 4, 6, 8], 16, 16, 2) == (2, 4, 6, 8)
    for rect, step in (((0, 0, 0, 8), 1), ((0, 0, 8, 0), 1), ((-2, 0, 8, 8), 1), ((0, 0, 17, 8), 1), ((0, 10, 8, 8), 1), ((1, 0, 8, 8), 2),
                       ((0, 0, 7, 8), (2, 1)), ((0, 1, 8, 8), (1, 2)), ((0, 0, 8), 1), ('auto', 1), ((0, 0, 8.0, 8), 1), ((0, 0, True, 8), 1)):
        with pytest.raises(ValueError):
            bars.check_rect(rect, 16, 16, step)
    for bad in (-1, 256, 24.0, True):
        with pytest.raises(ValueError):
            bars.frame_boxes([[0] * 8], 4, 4, 8, bad)
    with pytest.raises(ValueError):
        bars.frame_boxes([[0] * 7], 4, 4)
    assert bars.parse_crop('64:32:0:8') == (8, 0, 32, 64) and bars.crop_string((8, 0, 32, 64)) == '64:32:0:8'
    for bad in ('64:32:0', '64x32', 'a:b:c:d', '64:32:0:-8', ''):
        with pytest.raises(ValueError):
            bars.parse_crop(bad)


def test_detector_equals_the_batch_functions_for_every_composition():
    from edvr_amd import bars
    H, W, fmt = 24, 32, '420p10'
    clip = [UB.letterbox(H, W, 4), None, UB.windowbox(H, W, 4, 6), UB.letterbox(H, W, 6), None, UB.windowbox(H, W, 2, 8)]
    table = B.profile(UB.designed_clip(clip, H, W, fmt, seed=2), H, W, fmt)
    boxes = bars.frame_boxes(table, H, W, 10)
    assert boxes == clip
    whole = bars.video_box(boxes)
    pieces = UB.compositions(6)
    assert len(pieces) == 32
    for sizes in pieces:
        det, at = bars.BarDetector(H, W, 10), 0
        for k in sizes:
            det.push(torch.from_numpy(table[at:at + k]))
            at += k
            assert det.boxes == boxes[:at] and det.box() == bars.video_box(boxes[:at])
        assert det.frames == 6 and det.blank == [1, 4] and det.nonblank == 4 and det.box() == whole == (2, 22, 0, 32)
        assert det.box(frames=2) == clip[0]
        assert det.rect((2, 2), (4, 4), min_bar=2) == bars.aligned_rect(whole, H, W, (2, 2), (4, 4), min_bar=2) == (2, 0, 20, 32)


def test_detector_lists_the_frames_outside_the_rect():
    """The picture grows at frame 4: decided on the first four frames, the rect cuts the later ones."""
    from edvr_amd import bars
    H, W = 48, 64
    clip = [UB.letterbox(H, W, 10)] * 4 + [UB.letterbox(H, W, 4), UB.letterbox(H, W, 8), None, UB.letterbox(H, W, 7), (10, 38, 0, W)]
    det = bars.BarDetector(H, W)
    det.push(B.profile(UB.designed_clip(clip, H, W, '420', seed=3), H, W, '420'))
    rect = det.rect((2, 2), (4, 4), frames=4)
    assert rect == (10, 0, 28, W)
    assert det.outside(rect) == [4, 7] == B.outside(det.boxes, rect)  # frame 5 reaches 2 rows beyond: within the tolerance
    assert det.outside(rect, tolerance=1) == [4, 5, 7] and det.outside(rect, tolerance=6) == []
    assert det.outside((0, 0, H, W)) == []


# ---------------------------------------------------------------------------------------------------------------- restore_y4m
class _Nearest4:
    """Stands in for VideoRestorer on the CPU: 'restores' by x4 replication, chunk by chunk; its size multiple is 4."""
    made = []

    def __init__(self, net, out_dtype=None, **kwargs):
        assert out_dtype == torch.float32
        self.scale, self.multiple, self.kwargs = 4, 4, kwargs
        _Nearest4.made.append(self)

    def restore_chunks(self, frames, length=None):
        for piece in frames:
            yield piece.repeat_interleave(4, 2).repeat_interleave(4, 3)


def _stand_ins(monkeypatch, calls):
    """Fixed signatures from before the crop arguments existed for everything that existed; the two new ops by the restatement."""
    from edvr_amd import ops, video

    def decode(yuv, h, w, matrix, rng, chroma):
        calls.append(('yuv420_to_rgb', yuv.shape[0], h, w, matrix, rng, chroma))
        return U.decode_def(yuv, h, w, matrix, rng, chroma)

    def encode(rgb, matrix, rng, out):
        calls.append(('rgb_to_yuv420', tuple(rgb.shape), matrix, rng))
        return out.copy_(U.encode_def(rgb, matrix, rng))

    def resample(frames, size, kernel='lanczos3', out=None):
        calls.append(('resample', tuple(frames.shape), tuple(size), kernel))
        return torch.nn.functional.interpolate(frames, size=tuple(size), mode='nearest')

    def bar_profile(yuv, H, W, format='420', *, out=None):
        calls.append(('bar_profile', yuv.shape[0], H, W, format))
        return torch.from_numpy(B.profile(yuv[:, :ops.yuv_frame_size(H, W, format)].numpy(), H, W, format))

    def yuv_crop(yuv, H, W, format='420', *, rect, out=None):
        calls.append(('yuv_crop', yuv.shape[0], H, W, format, tuple(rect)))
        return torch.from_numpy(B.crop(yuv[:, :ops.yuv_frame_size(H, W, format)].numpy(), H, W, format, rect))

    monkeypatch.setattr(ops, 'yuv420_to_rgb', decode)
    monkeypatch.setattr(ops, 'rgb_to_yuv420', encode)
    monkeypatch.setattr(ops, 'resample', resample)
    monkeypatch.setattr(ops, 'bar_profile', bar_profile)
    monkeypatch.setattr(ops, 'yuv_crop', yuv_crop)
    monkeypatch.setattr(video, 'VideoRestorer', _Nearest4)


H0, W0, TAGS = 24, 32, 'F24000:1001 Ip A32:27 C420jpeg'


def _letterboxed(n=5, bar=4, seed=5):
    return torch.from_numpy(UB.designed_clip([UB.letterbox(H0, W0, bar)] * n, H0, W0, '420', seed=seed))


def _by_hand(frames, rect, H=H0, W=W0):
    """The stream restore_y4m(crop=rect) must write, without a delivery size: crop, decode, x4, encode."""
    small = torch.from_numpy(B.crop(frames.numpy(), H, W, '420', rect))
    h, w = rect[2], rect[3]
    rgb = U.decode_def(small, h, w, 'bt601', 'limited', 'bilinear').repeat_interleave(4, 2).repeat_interleave(4, 3)
    return U.encode_def(rgb, 'bt601', 'limited')


@pytest.mark.parametrize('crop', ['auto', (4, 0, 16, 32)])
def test_restore_y4m_crops_between_the_stage_and_the_decode(monkeypatch, crop):
    from edvr_amd import y4m
    calls, stats = [], {}
    _stand_ins(monkeypatch, calls)
    frames = _letterboxed()
    out = io.BytesIO()
    n = y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(frames, H0, W0, TAGS)), out, read_frames=2, chunk=3, crop=crop,
                        crop_probe=3, crop_min_bar=4, stats=stats)
    assert n == 5 and _Nearest4.made[-1].kwargs == dict(chunk=3)  # the restorer sees none of the crop arguments
    assert out.getvalue().startswith(b'YUV4MPEG2 W128 H64 F24000:1001 Ip A32:27 C420jpeg\nFRAME\n')  # 4 x (16 x 32); A is copied
    rect = (4, 0, 16, 32)
    crops = [('yuv_crop', k, H0, W0, '420', rect) for k in (2, 2, 1)]
    decodes = [('yuv420_to_rgb', k, 16, 32, 'bt601', 'limited', 'bilinear') for k in (2, 2, 1)]
    encodes = [('rgb_to_yuv420', (k, 3, 64, 128), 'bt601', 'limited') for k in (2, 2, 1)]
    profiles = [('bar_profile', k, H0, W0, '420') for k in (2, 2, 1)]
    if crop == 'auto':
        # two pieces are profiled and held until 3 frames that are not blank have been seen, then replayed; the last is profiled as it passes
        assert calls == profiles[:2] + [crops[0], decodes[0], encodes[0], crops[1], decodes[1], encodes[1], profiles[2], crops[2], decodes[2], encodes[2]]
        assert stats == dict(frames=5, crop=rect, crop_box=(4, 20, 0, 32), bars_blank=[], bars_outside=[])
    else:
        assert calls == [c for trio in zip(crops, decodes, encodes) for c in trio]
        assert stats == dict(frames=5, crop=rect)
    r = y4m.Y4MReader(io.BytesIO(out.getvalue()))
    assert (r.width, r.height, r.aspect) == (128, 64, '32:27')
    assert torch.equal(r.read(8)[:, 6:], _by_hand(frames, rect))


def test_restore_y4m_fits_the_cropped_size(monkeypatch):
    """fit_size sees s h x s w: 64 x 128 A32:27 at out_height=32 with square pixels is 32 x 76, not the 32 x 50 of the 96 x 128 frame."""
    from edvr_amd import y4m
    calls = []
    _stand_ins(monkeypatch, calls)
    assert y4m.fit_size(64, 128, '32:27', height=32, square=True) == (32, 76, '1:1')
    assert y4m.fit_size(96, 128, '32:27', height=32, square=True) == (32, 50, '1:1')
    out = io.BytesIO()
    y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(_letterboxed(), H0, W0, TAGS)), out, read_frames=5, crop='auto', crop_probe=2,
                    crop_min_bar=4, out_height=32, square_pixels=True)
    assert out.getvalue().startswith(b'YUV4MPEG2 W76 H32 F24000:1001 Ip A1:1 C420jpeg\n')
    assert [c for c in calls if c[0] == 'resample'] == [('resample', (5, 3, 64, 128), (32, 76), 'lanczos3')]


def test_restore_y4m_auto_with_nothing_to_crop(monkeypatch):
    """Bars under min_bar, a box that is not believed, a blank video: nothing is cropped, no crop call is made and stats say so."""
    from edvr_amd import y4m
    for boxes, kw, want_box in (([UB.letterbox(H0, W0, 2)] * 3, {}, (2, 22, 0, 32)),               # 4 rows < min_bar 8: the whole frame
                                ([(8, 16, 0, W0)] * 3, dict(crop_min_bar=4), (8, 16, 0, 32)),      # 8 of 24 rows: not believed
                                ([None] * 3, {}, None)):
        calls, stats = [], {}
        _stand_ins(monkeypatch, calls)
        frames = torch.from_numpy(UB.designed_clip(boxes, H0, W0, '420', seed=6))
        out = io.BytesIO()
        assert y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(frames, H0, W0, TAGS)), out, read_frames=2, crop='auto', crop_probe=2,
                               stats=stats, **kw) == 3
        assert out.getvalue().startswith(b'YUV4MPEG2 W128 H96 ')
        assert not [c for c in calls if c[0] == 'yuv_crop'] and len([c for c in calls if c[0] == 'bar_profile']) == 2
        assert stats['crop'] == ((0, 0, H0, W0) if want_box == (2, 22, 0, 32) else None) and stats['crop_box'] == want_box
        assert stats['bars_blank'] == ([0, 1, 2] if want_box is None else [])


def test_restore_y4m_probe_waits_for_frames_that_are_not_blank(monkeypatch):
    """Four blank frames in front: the probe of 2 holds pieces until two frames with a box have come; a picture that grows after the
    decision is reported in bars_outside."""
    from edvr_amd import y4m
    calls, stats = [], {}
    _stand_ins(monkeypatch, calls)
    boxes = [None] * 4 + [UB.letterbox(H0, W0, 4)] * 3 + [UB.letterbox(H0, W0, 0)] * 2
    frames = torch.from_numpy(UB.designed_clip(boxes, H0, W0, '420', seed=8))
    out = io.BytesIO()
    assert y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(frames, H0, W0, TAGS)), out, read_frames=2, crop='auto', crop_probe=2,
                           crop_min_bar=4, stats=stats) == 9
    assert [c[0] for c in calls[:3]] == ['bar_profile'] * 3 and calls[3][0] == 'yuv_crop'  # 6 frames held: 4 blank, 2 with a box
    assert stats == dict(frames=9, crop=(4, 0, 16, 32), crop_box=(4, 20, 0, 32), bars_blank=[0, 1, 2, 3], bars_outside=[7, 8])
    # 4 x crop_probe frames held without enough of them: decided on what there is
    calls, stats = [], {}
    _stand_ins(monkeypatch, calls)
    out = io.BytesIO()
    y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(frames, H0, W0, TAGS)), out, read_frames=1, crop='auto', crop_probe=1,
                    crop_min_bar=4, stats=stats)
    assert [c[0] for c in calls[:5]] == ['bar_profile'] * 4 + ['yuv420_to_rgb'] and stats['crop'] is None and stats['crop_box'] is None
    assert stats['bars_blank'] == [0, 1, 2, 3] and stats['bars_outside'] == []


def test_restore_y4m_without_crop_makes_the_old_calls(monkeypatch):
    """crop=None: the stand-ins of everything that existed before - fixed signatures - receive exactly the old calls and the new ops
    none; a rect equal to the whole frame makes no crop call and writes the same stream."""
    from edvr_amd import y4m
    frames = _letterboxed(3)
    old = [('yuv420_to_rgb', 2, H0, W0, 'bt601', 'limited', 'bilinear'), ('rgb_to_yuv420', (2, 3, 96, 128), 'bt601', 'limited'),
           ('yuv420_to_rgb', 1, H0, W0, 'bt601', 'limited', 'bilinear'), ('rgb_to_yuv420', (1, 3, 96, 128), 'bt601', 'limited')]
    outs = []
    for kw in (dict(), dict(crop=None), dict(crop=(0, 0, H0, W0))):
        calls = []
        _stand_ins(monkeypatch, calls)
        out = io.BytesIO()
        assert y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(frames, H0, W0, TAGS)), out, read_frames=2, chunk=3, **kw) == 3
        assert calls == old, kw
        assert _Nearest4.made[-1].kwargs == dict(chunk=3)
        outs.append(out.getvalue())
    assert outs[0].startswith(b'YUV4MPEG2 W128 H96 F24000:1001 Ip A32:27 C420jpeg\n') and outs[0] == outs[1] == outs[2]


def test_restore_y4m_refuses_bad_crop_arguments(monkeypatch):
    from edvr_amd import y4m
    calls = []
    _stand_ins(monkeypatch, calls)
    data = U.y4m_bytes(_letterboxed(2), H0, W0, TAGS)
    for kw in (dict(crop='detect'), dict(crop=(0, 0, 16)), dict(crop=(0, 0, 0, 32)), dict(crop=(12, 0, 16, 32)), dict(crop=(0, 4, 16, 32)),
               dict(crop=(1, 0, 16, 32)), dict(crop=(0, 1, 16, 30), pad_mode='reflect'),   # off the chroma steps, with or without pad_mode
               dict(crop=(2, 0, 18, 32)), dict(crop=(0, 2, 16, 30)),             # on the chroma steps, but no multiple of 4 and no pad_mode
               dict(crop=(4.0, 0, 16, 32)), dict(crop='auto', crop_probe=0), dict(crop='auto', crop_probe=2.5), dict(crop='auto', crop_limit=256),
               dict(crop='auto', crop_limit=-1), dict(crop='auto', crop_margin=-1), dict(crop='auto', crop_min_bar=-2), dict(crop=(4, 0, 16, 32), crop_limit=300)):
        out = io.BytesIO()
        with pytest.raises(ValueError):
            y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(data), out, **kw)
        assert out.getvalue() == b'' and calls == [], kw  # refused before the header is written and before any launch
    # with pad_mode the chroma steps alone bind an explicit rect ...
    out = io.BytesIO()
    assert y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(data), out, crop=(2, 2, 18, 30), pad_mode='reflect') == 2
    assert out.getvalue().startswith(b'YUV4MPEG2 W120 H72 ') and _Nearest4.made[-1].kwargs == dict(pad_mode='reflect')
    # ... and the rect of 'auto': bars of 3 and 5 rows leave rows [4, 18) of a 4:2:0 frame - 14 rows with pad_mode, 12 without
    frames = torch.from_numpy(UB.designed_clip([(3, 19, 0, W0)] * 2, H0, W0, '420', seed=9))
    for kw, head in ((dict(pad_mode='replicate'), b'YUV4MPEG2 W128 H56 '), (dict(), b'YUV4MPEG2 W128 H48 ')):
        out, stats = io.BytesIO(), {}
        y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(frames, H0, W0, TAGS)), out, crop='auto', crop_min_bar=4, stats=stats, **kw)
        assert out.getvalue().startswith(head), (kw, out.getvalue()[:40])
        assert stats['crop'] == ((4, 0, 14, 32) if kw else (4, 0, 12, 32))


def test_cropped_generator(monkeypatch):
    from edvr_amd import y4m
    calls = []
    _stand_ins(monkeypatch, calls)
    frames = _letterboxed(5)
    pieces = [frames[:2], frames[2:3], frames[3:]]
    got = torch.cat(list(y4m.cropped(iter(pieces), H0, W0, '420', (4, 2, 16, 28))))
    assert torch.equal(got, torch.from_numpy(B.crop(frames.numpy(), H0, W0, '420', (4, 2, 16, 28))))
    assert [c[1] for c in calls] == [2, 1, 2]
    with pytest.raises(ValueError):
        next(y4m.cropped(iter(pieces), H0, W0, '420', (4, 1, 16, 28)))


# ---------------------------------------------------------------------------------------------------------------- the ops and the scripts
def test_ops_refuse_the_cpu():
    from edvr_amd import ops
    yuv = torch.zeros(2, ops.yuv_frame_size(8, 8), dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        ops.bar_profile(yuv, 8, 8)
    with pytest.raises(NotImplementedError):
        ops.yuv_crop(yuv, 8, 8, rect=(0, 0, 4, 4))
    with pytest.raises(ValueError):
        ops.bar_profile(yuv, 8, 8, '411')


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restore_video_crop_flags(capsys):
    mod = _script('restore_video')
    with pytest.raises(SystemExit) as e:
        mod.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--crop', '--crop-probe', '--crop-limit', '--crop-margin', '--bars-json'):
        assert opt in text, opt
    args = mod.parse_args(['-', '-'])
    assert (args.crop, args.crop_probe, args.crop_limit, args.crop_margin, args.bars_json) == (None, 48, 24, 0, None)
    args = mod.parse_args(['-', '-', '--crop', 'auto', '--crop-probe', '96', '--crop-limit', '32', '--crop-margin', '2', '--bars-json', 'b.json'])
    assert (args.crop, args.crop_probe, args.crop_limit, args.crop_margin, args.bars_json) == ('auto', 96, 32, 2, 'b.json')
    assert mod.parse_args(['-', '-', '--crop', '720:360:0:60']).crop == (60, 0, 360, 720)  # ffmpeg's W:H:X:Y -> (y0, x0, h, w)
    args = mod.parse_args(['-', '-', '--deinterlace', 'film', '--crop', 'auto', '--out-height', '1080', '--square-pixels'])
    assert (args.deinterlace, args.crop, args.out_height) == ('film', 'auto', 1080)
    for bad in (['-', '-', '--crop', '720x360'], ['-', '-', '--crop', '720:360:0'], ['-', '-', '--crop', '0:360:0:60'], ['-', '-', '--crop', 'yes'],
                ['-', '-', '--crop-probe', '96'], ['-', '-', '--crop', '720:360:0:60', '--crop-limit', '32'], ['-', '-', '--crop', 'auto', '--crop-probe', '0'],
                ['-', '-', '--crop', 'auto', '--crop-limit', '256'], ['-', '-', '--crop', 'auto', '--crop-margin', '-1'], ['-', '-', '--bars-json', 'b.json']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()


def test_detect_bars_flags(capsys):
    mod = _script('detect_bars')
    args = mod.parse_args(['in.y4m'])
    assert (args.input, args.limit, args.margin, args.multiple, args.min_bar, args.json) == ('in.y4m', 24, 0, 4, 8, None)
    args = mod.parse_args(['-', '--limit', '30', '--margin', '2', '--multiple', '16', '--json', 'bars.json'])
    assert (args.input, args.limit, args.margin, args.multiple, args.json) == ('-', 30, 2, 16, 'bars.json')
    for bad in ([], ['-', '--limit', '256'], ['-', '--margin', '-1'], ['-', '--multiple', '0'], ['-', '--read-frames', '0']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
