"""GPU: ops.mpeg_roundtrip (csrc/mpeg.hip) against the NumPy restatement tests/mpeg_ref.py - torch.equal, no tolerance -
at the shapes where the kernels can go wrong: one macroblock whose every displaced read clamps, odd sizes, the two bold rules of DESIGN
4.16, a pass-through clip beside a coded one, vectors at the range limit across tile edges, edge parameters, the largest residual, ties."""
import numpy as np
import pytest
import torch

import mpeg_ref
from util_mpeg import inverted_stripes_clip, moving_clip, noise_clip, tie_clip

pytestmark = pytest.mark.gpu


def _ref(frames, qscale, gop=12, search=7):
    return torch.from_numpy(mpeg_ref.roundtrip(frames.cpu().numpy(), qscale, gop, search))


def _check(gpu, frames, qscale, gop=12, search=7):
    from edvr_amd import ops
    got = ops.mpeg_roundtrip(frames.to(gpu), qscale, gop, search)
    assert got.dtype == torch.uint8 and got.shape == frames.shape
    want = _ref(frames, qscale, gop, search)
    diff = (got.cpu().int() - want.int()).abs()
    bad = [i for i in range(frames.shape[-4]) if bool(diff[..., i, :, :, :].any())]
    assert torch.equal(got.cpu(), want), (tuple(frames.shape), qscale, gop, search, 'frames that differ', bad, int(diff.max()))
    return got


@pytest.mark.parametrize('search', [7, 15])
def test_one_macroblock_every_displaced_read_clamps(gpu, search):
    out = _check(gpu, noise_clip(1, 2, 16, 16, 1), 6, 12, search)
    assert not torch.equal(out[0, 1].cpu(), noise_clip(1, 2, 16, 16, 1)[0, 1])


def test_odd_sizes(gpu):
    _check(gpu, moving_clip(3, 33, 47, (1, -2), 2)[None], 5)


@pytest.mark.parametrize('shape', [(1, 2, 1, 1), (1, 2, 8, 8), (1, 2, 20, 4)])
def test_the_bold_rules_of_the_jpeg_definition(gpu, shape):
    _check(gpu, noise_clip(*shape, 3), 4)


def test_training_shape_with_a_pass_through_clip(gpu):
    from edvr_amd import ops
    x = torch.stack([moving_clip(5, 64, 64, (2, -3), 4), moving_clip(5, 64, 64, (-1, 2), 5)])
    out = _check(gpu, x, [0, 9], 0)
    assert torch.equal(out[0].cpu(), x[0]) and not torch.equal(out[1].cpu(), x[1])
    xd = x.to(gpu)
    assert torch.equal(out, ops.mpeg_roundtrip(xd, torch.tensor([0, 9], dtype=torch.int32, device=gpu), 0))
    assert torch.equal(out, ops.mpeg_roundtrip(xd, (0, 9), 0))
    # a device table is clamped to 0 .. 31 by the kernels
    assert torch.equal(ops.mpeg_roundtrip(xd, torch.tensor([-3, 99], dtype=torch.int32, device=gpu)), ops.mpeg_roundtrip(xd, [0, 31]))
    # the scalar form, and a clip alone equals the same clip inside a batch
    both = ops.mpeg_roundtrip(xd, 9, 0)
    assert torch.equal(both, ops.mpeg_roundtrip(xd, [9, 9], 0))
    for i in range(2):
        assert torch.equal(both[i], ops.mpeg_roundtrip(xd[i], 9, 0)) and torch.equal(both[i], ops.mpeg_roundtrip(xd[i:i + 1], 9, 0)[0])
    assert torch.equal(both[1], out[1])
    assert torch.equal(both, ops.mpeg_roundtrip(xd, 9, 0))  # two calls are equal


@pytest.mark.parametrize('first, second', [(0, 9), (9, 0), (5, 9)])
def test_clips_of_one_frame(gpu, first, second):
    """b > 1 with t = 1: frame f of the call is clip f - a pass-through clip beside a coded one either way round, a table of two
    scales, and one-frame slices of longer clips, whose clips lie more than a frame apart."""
    from edvr_amd import ops
    x = torch.stack([moving_clip(1, 33, 47, (0, 0), 40), moving_clip(1, 33, 47, (0, 0), 41), moving_clip(1, 33, 47, (0, 0), 42)])
    table = [first, second, 7]
    out = _check(gpu, x, table)
    for i, q in enumerate(table):
        assert torch.equal(out[i].cpu(), x[i]) == (q == 0), i
        assert torch.equal(out[i], ops.mpeg_roundtrip(x[i].to(gpu), q)), i
    longer = torch.stack([moving_clip(4, 33, 47, (1, 1), 43), moving_clip(4, 33, 47, (-1, 2), 44), moving_clip(4, 33, 47, (2, 0), 45)]).to(gpu)
    for k in (0, 2, 3):
        view = longer[:, k:k + 1]
        assert view.stride(0) == 4 * 3 * 33 * 47
        got = ops.mpeg_roundtrip(view, table)
        assert torch.equal(got.cpu(), _ref(view.cpu(), table)), k
        dst = torch.full_like(longer, 7)
        assert ops.mpeg_roundtrip(view, table, out=dst[:, k:k + 1]).data_ptr() == dst[:, k:k + 1].data_ptr()
        assert torch.equal(dst[:, k:k + 1], got) and bool((dst[:, [j for j in range(4) if j != k]] == 7).all()), k


@pytest.mark.parametrize('h, w, search', [(80, 144, 4), (80, 144, 5), (80, 144, 6), (80, 144, 15), (64, 64, 4), (48, 52, 7)])
def test_interior_and_edge_windows(gpu, h, w, search):
    """Macroblocks whose search window lies inside the plane take aligned dword loads, at each of the four byte alignments R & 3 gives,
    beside edge macroblocks that take clamped byte loads; 64 x 64 at R = 4 and 48 x 52 (padded to 64) at R = 7 hold a macroblock whose
    window ends exactly at, and one dword short of, the plane's last column."""
    _check(gpu, moving_clip(3, h, w, (-search, search), 46)[None], 5, 0, search)


def test_vectors_at_the_range_limit_across_tile_edges(gpu):
    clip = moving_clip(3, 80, 144, (-7, 7), 6)
    _, stats = mpeg_ref.roundtrip_clip(clip.numpy(), 4, 12, 7, details=True)
    inner = stats['vectors'][1][1:-1, 1:-1].reshape(-1, 2)
    assert (inner == (-7, 7)).all(), inner  # (the clip does what it is for)
    _check(gpu, clip[None], 4)


@pytest.mark.parametrize('t, qscale, gop, search', [(1, 8, 12, 7), (4, 8, 0, 7), (4, 8, 1, 7), (4, 8, 2, 7), (3, 8, 12, 0), (3, 1, 12, 3), (3, 31, 12, 7)])
def test_edge_parameters(gpu, t, qscale, gop, search):
    _check(gpu, moving_clip(t, 40, 56, (1, 1), 7)[None], qscale, gop, search)


@pytest.mark.parametrize('qscale', [1, 31])
def test_the_largest_residual(gpu, qscale):
    _check(gpu, inverted_stripes_clip(3, 32, 32)[None], qscale, 0, 2)


def test_ties_go_to_the_first_candidate(gpu):
    clip = tie_clip(48, 64)
    _, stats = mpeg_ref.roundtrip_clip(clip.numpy(), 1, 12, 7, details=True)
    assert (stats['vectors'][1][1:-1, 1:-1, 1] == -4).all()
    _check(gpu, clip[None], 1)


def test_one_clip_without_the_batch_axis(gpu):
    from edvr_amd import ops
    clip = moving_clip(3, 24, 40, (0, 2), 8)
    out = ops.mpeg_roundtrip(clip.to(gpu), 7)
    assert out.shape == clip.shape and torch.equal(out.cpu(), _ref(clip, 7))


def test_strided_odd_offset_views_and_out(gpu):
    """Every other frame of a longer clip at an odd base address (byte accesses), a 4-byte aligned one (dword accesses), a view that has
    to be gathered first, and out= into a strided destination whose gaps are left alone."""
    from edvr_amd import ops
    b, t, h, w = 2, 3, 20, 28
    x = torch.stack([moving_clip(t, h, w, (1, -1), 9), moving_clip(t, h, w, (-2, 0), 10)])
    want = _ref(x, 6)
    frame = 3 * h * w
    for offset, gap in ((3, 17), (8, 0)):
        fstride, cstride = 2 * frame + gap, t * (2 * frame + gap) + 4 * gap
        buf = torch.zeros(offset + b * cstride + frame, dtype=torch.uint8, device=gpu)
        strides = (cstride, fstride, 3 * w, 3, 1)
        view = buf.as_strided((b, t, h, w, 3), strides, offset)
        view.copy_(x.to(gpu))
        assert torch.equal(ops.mpeg_roundtrip(view, 6).cpu(), want), (offset, gap)
        dst = torch.full_like(buf, 7)
        out = dst.as_strided((b, t, h, w, 3), strides, offset)
        assert ops.mpeg_roundtrip(view, 6, out=out) is out
        assert torch.equal(out.cpu(), want)
        written = torch.zeros_like(dst, dtype=torch.bool)
        written.as_strided((b, t, h, w, 3), strides, offset).fill_(True)
        assert bool((dst[~written] == 7).all()) and int(written.sum()) == b * t * frame
    wide = torch.zeros(b, t, h, w + 5, 3, dtype=torch.uint8, device=gpu)
    wide[:, :, :, 2:2 + w] = x.to(gpu)
    assert torch.equal(ops.mpeg_roundtrip(wide[:, :, :, 2:2 + w], 6).cpu(), want)  # rows not dense: gathered first
    longer = torch.cat([x, x.flip(1)], 1).to(gpu)
    assert torch.equal(ops.mpeg_roundtrip(longer[:, 3:], 6).cpu(), _ref(x.flip(1), 6))  # a slice of longer clips


def test_refusals(gpu):
    from edvr_amd import ops
    x = noise_clip(2, 2, 16, 16, 11).to(gpu)
    with pytest.raises(NotImplementedError):
        ops.mpeg_roundtrip(x.cpu(), 5)
    with pytest.raises(ValueError, match='overlaps'):
        ops.mpeg_roundtrip(x, 5, out=x)
    buf = torch.zeros(3, 2, 16, 16, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match='overlaps'):
        ops.mpeg_roundtrip(buf[:2], 5, out=buf[1:])
    for bad in (32, -1, 5.5, True, [5], [5, 32], torch.tensor([5, 5], device=gpu), torch.tensor([5], dtype=torch.int32, device=gpu)):
        with pytest.raises(ValueError):
            ops.mpeg_roundtrip(x, bad)
    for kw in ({'gop': -1}, {'gop': 2.0}, {'search': 16}, {'search': -1}, {'search': None}):
        with pytest.raises(ValueError):
            ops.mpeg_roundtrip(x, 5, **kw)
    for bad in (x.float(), x[0, 0], x[..., :2], x[None]):
        with pytest.raises(ValueError):
            ops.mpeg_roundtrip(bad, 5)
    with pytest.raises(ValueError):
        ops.mpeg_roundtrip(x, 5, out=torch.empty(2, 2, 16, 16, 3, dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError):
        ops.mpeg_roundtrip(x, 5, out=torch.empty(2, 3, 16, 16, 3, dtype=torch.uint8, device=gpu))
    frame = 3 * 16 * 16
    flat = torch.zeros(8 * frame, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):  # clips of `out` one frame apart: clip 1 would begin where frame 1 of clip 0 lies
        ops.mpeg_roundtrip(x, 5, out=flat.as_strided((2, 2, 16, 16, 3), (frame, frame, 48, 3, 1)))
    # such an input is read as the view says: gathered first
    lapped = flat.as_strided((2, 2, 16, 16, 3), (frame, frame, 48, 3, 1), 4 * frame)
    lapped[0].copy_(x[0]), lapped[1, 1].copy_(x[1, 1])
    assert torch.equal(ops.mpeg_roundtrip(lapped, 5), ops.mpeg_roundtrip(lapped.contiguous(), 5))


def test_workspace_query_and_booking(gpu):
    from edvr_amd import _lib, ops
    assert _lib.lib().edvr_mpeg_roundtrip_workspace(2, 5, 33, 47) == 2 * 2 * 5 * (48 * 48 * 3 // 2)
    assert _lib.lib().edvr_mpeg_roundtrip_workspace(0, 5, 33, 47) == 0
    seen = []

    def hook(name, flops, launch, nbytes, executed):
        seen.append((name, flops, nbytes))
        launch()

    x = noise_clip(2, 3, 33, 47, 12).to(gpu)
    prev, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, hook
    try:
        ops.mpeg_roundtrip(x, 5)
    finally:
        ops.LAUNCH_HOOK = prev
    assert seen == [('mpeg_roundtrip', 0.0, 6.0 * 2 * 3 * 33 * 47 + 2.0 * 2 * 2 * 3 * (48 * 48 * 3 // 2))]


def test_equals_the_frozen_fixture(gpu):
    import os
    from edvr_amd import ops
    gold = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mpeg_roundtrip.pt'))
    for case in gold['cases']:
        got = ops.mpeg_roundtrip(case['input'].to(gpu), case['qscale'], case['gop'], case['search'])
        assert torch.equal(got.cpu(), case['output']), case['name']
