"""-m gpu: scene cuts on the device - csrc/shots.hip (ops.frame_sad) bit for bit against the restatement of tests/util_shots.py over
sizes, layouts and both access widths, and VideoRestorer / restore_y4m with cuts against the per-shot concatenation of the same
configuration without them."""
import io

import pytest
import torch

import util_shots as S
import util_yuv as U

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 1), (4, 7, 13), (5, 36, 52), (2, 180, 320), (2, 97, 331)]


def _video(n, H, W, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
    return torch.rand(n, 3, H, W, generator=g) * 1.2 - 0.1  # a little outside [0, 1] on both sides


def _padded(frames, pad):
    """The same frames on the device, `pad` elements further apart than dense."""
    n, per = frames.shape[0], frames[0].numel()
    buf = torch.zeros(n, per + pad, dtype=frames.dtype, device='cuda')
    buf[:, :per] = frames.reshape(n, per).cuda()
    view = buf[:, :per].view(frames.shape)
    assert view.stride(0) == per + pad and view.data_ptr() == buf.data_ptr()
    return view


@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32], ids=['u8', 'f32'])
@pytest.mark.parametrize('n, H, W', SHAPES)
def test_frame_sad_is_the_restatement(n, H, W, dtype):
    from edvr_amd import ops
    frames = _video(n, H, W, dtype, seed=H * W + n)
    dev = frames.cuda()
    want = S.sad(frames)
    got = ops.frame_sad(dev)
    assert got.dtype == torch.int64 and got.shape == (n,) and got.is_cuda
    assert torch.equal(got.cpu(), want) and int(got[0]) == 0
    assert int(want[1:].min()) > 0 or H * W == 1
    # a slice: for the bytes of 7 x 13 (273 per frame) and 97 x 331 frames an odd base address; with and without the frame before it
    tail = dev[1:]
    assert tail.data_ptr() != dev.data_ptr()
    want_tail = want[1:].clone()
    want_tail[0] = 0
    assert torch.equal(ops.frame_sad(tail).cpu(), want_tail)
    assert torch.equal(ops.frame_sad(tail, prev=dev[0]).cpu(), want[1:])
    assert torch.equal(ops.frame_sad(tail, prev=dev[:1]).cpu(), want[1:])
    assert torch.equal(ops.frame_sad(dev[:1], prev=dev[1]).cpu(), want[1:2])  # one frame against another: |a - b| = |b - a|
    # frames further apart than dense: by a multiple of 16 bytes (the wide loads stay possible where the size allows them) and by 5 elements
    for pad in (16, 5):
        far = _padded(frames, pad)
        assert torch.equal(ops.frame_sad(far).cpu(), want), pad
        assert torch.equal(ops.frame_sad(far[1:], prev=far[0]).cpu(), want[1:]), pad
    out = torch.full((n,), -1, dtype=torch.int64, device='cuda')
    assert ops.frame_sad(dev, out=out) is out and torch.equal(out.cpu(), want)
    # a layout the kernel does not read (channels-last floats, planar bytes) is made dense first
    other = dev.permute(0, 3, 1, 2) if dtype == torch.uint8 else dev.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    if dtype == torch.float32:
        assert torch.equal(ops.frame_sad(other).cpu(), want)
    else:
        with pytest.raises(ValueError):
            ops.frame_sad(other)


def test_float_edge_values():
    from edvr_amd import ops
    ties = [(b + 0.5) / 255.0 for b in range(255)]
    special = [-0.0, -1e-9, -3.0, float('-inf'), 1.0, 1.0 + 1e-7, 7.5, float('inf'), float('nan'), 0.5, 1e-45, 0.0019607843, 0.99803925]
    vals = torch.tensor(ties + special, dtype=torch.float32)
    g = torch.Generator().manual_seed(5)
    n, H, W = 4, 24, 40
    idx = torch.randint(0, vals.numel(), (n, 3, H, W), generator=g)
    frames = vals[idx]
    frames[0].view(-1)[:vals.numel()] = vals  # every value at least once
    assert bool(torch.isnan(frames).any())
    want = S.sad(frames)
    assert torch.equal(ops.frame_sad(frames.cuda()).cpu(), want)
    assert torch.equal(ops.frame_sad(frames[:, :, :, :39].cuda()).cpu(), S.sad(frames[:, :, :, :39].contiguous()))  # the narrow loads
    # a float frame holding byte / 255 gives what the bytes give
    u8 = _video(5, 36, 52, torch.uint8, seed=9)
    as_float = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(ops.frame_sad(u8.cuda()), ops.frame_sad(as_float.cuda()))
    assert torch.equal(ops.frame_sad(u8.cuda()).cpu(), S.sad(u8))


@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32], ids=['u8', 'f32'])
def test_batching_does_not_change_the_numbers(dtype):
    from edvr_amd import ops
    frames = _video(9, 36, 52, dtype, seed=11).cuda()
    whole = ops.frame_sad(frames)
    parts, prev = [], None
    for a, b in ((0, 4), (4, 5), (5, 9)):
        parts.append(ops.frame_sad(frames[a:b], prev=prev))
        prev = frames[b - 1]
    assert torch.equal(torch.cat(parts), whole)
    assert torch.equal(whole.cpu(), S.sad(frames.cpu()))


def test_sums_beyond_32_bits():
    from edvr_amd import ops
    side = 4608
    frames = torch.zeros(2, side, side, 3, dtype=torch.uint8, device='cuda')
    frames[1] = 255
    got = ops.frame_sad(frames).tolist()
    assert got == [0, 219 * side * side] and got[1] > 2 ** 32   # Y8 of white - Y8 of black = 235 - 16
    assert ops.frame_sad(frames[1:], prev=frames[0]).tolist() == [219 * side * side]


def test_errors():
    from edvr_amd import ops
    f = torch.zeros(2, 3, 8, 8, device='cuda')
    with pytest.raises(ValueError):
        ops.frame_sad(f[:, :2])
    with pytest.raises(ValueError):
        ops.frame_sad(f, prev=torch.zeros(3, 8, 9, device='cuda'))
    with pytest.raises(ValueError):
        ops.frame_sad(f, prev=torch.zeros(8, 8, 3, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.frame_sad(f, out=torch.zeros(3, dtype=torch.int64, device='cuda'))
    with pytest.raises(NotImplementedError):
        ops.frame_sad(f.half())
    with pytest.raises(NotImplementedError):
        ops.frame_sad(f, prev=torch.zeros(3, 8, 8))


# ---------------------------------------------------------------------------------------------------------------- end to end
_CACHE = {}


def _net(name):
    if name not in _CACHE:
        from util_edvr import build
        _CACHE[name] = build(name)[0].cuda().eval()
    return _CACHE[name]


def _synthetic(H, W, dtype=torch.float32):
    key = ('video', H, W, dtype)
    if key not in _CACHE:
        v = S.synthetic_video(H, W, dtype)
        cuts, mafd, score = S.cuts_of(v, 10.0, 5)
        assert cuts == S.CUTS, (cuts, score)  # the input has its two cuts: what fails below is the detector, not the video
        _CACHE[key] = (v, mafd, score)
    return _CACHE[key]


def _per_shot(lq, **kw):
    from edvr_amd import VideoRestorer
    net = kw.pop('net')
    return torch.cat([VideoRestorer(net, **kw).restore(lq[a:b]) for a, b in S.shot_bounds(S.CUTS, lq.shape[0])])


@pytest.mark.parametrize('f4s', [True, False], ids=['split', 'nosplit'])
def test_auto_cuts_restore_every_shot_on_its_own(f4s):
    from edvr_amd import VideoRestorer, ops
    net = _net('M_T5')
    v, mafd, score = _synthetic(36, 52)
    lq = v.cuda()
    before = ops.set_f4s(inference=f4s)
    try:
        with torch.no_grad():
            vr = VideoRestorer(net, chunk=4, cuts='auto')
            got = vr.restore(lq)
            assert vr.cuts_found == S.CUTS
            assert vr.cut_scores == score and vr.cut_mafd == mafd
            want = _per_shot(lq, net=net, chunk=4)
            assert got.shape == want.shape == (22, 3, 144, 208)
            assert torch.equal(got, want)
            if f4s:
                # streamed: frame by frame and in pieces of 3 - the same frames, the same cuts, the same scores
                vr2 = VideoRestorer(net, chunk=4, cuts='auto')
                singles = torch.stack(list(vr2.restore_iter(iter(lq.unbind(0)))))
                assert vr2.cuts_found == S.CUTS and vr2.cut_scores == score
                threes = torch.stack(list(vr2.restore_iter(lq.split(3))))
                assert vr2.cuts_found == S.CUTS and vr2.cut_scores == score and vr2.cut_mafd == mafd
                assert torch.equal(singles, want) and torch.equal(threes, want)
                # ... and the cut matters: the frames whose windows crossed it are others now
                plain = VideoRestorer(net, chunk=4).restore(lq)
                changed = [i for i in range(22) if not torch.equal(plain[i], want[i])]
                assert all(i in changed for i in (5, 6, 7, 8)), changed
        net.check_offsets()
    finally:
        ops.set_f4s(inference=before[0])


@pytest.mark.parametrize('config', ['u8_reflect_ensemble', 'time_reverse'])
def test_explicit_cuts_compose_with_the_other_arguments(config):
    from edvr_amd import VideoRestorer
    net = _net('M_T5')
    if config == 'u8_reflect_ensemble':
        lq = _synthetic(37, 50, torch.uint8)[0].cuda()
        kw = dict(chunk=4, pad_mode='reflect', self_ensemble=(0, 3), out_dtype=torch.uint8)
        shape = (22, 148, 200, 3)
    else:
        lq = _synthetic(36, 52)[0].cuda()
        kw = dict(chunk=4, time_reverse=True)
        shape = (22, 3, 144, 208)
    with torch.no_grad():
        vr = VideoRestorer(net, cuts=S.CUTS, **kw)
        got = vr.restore(lq)
        want = _per_shot(lq, net=net, **kw)
        streamed = torch.stack(list(vr.restore_iter(lq.split(5))))
    net.check_offsets()
    assert vr.cuts_found == S.CUTS and vr.cut_scores is None
    assert got.shape == want.shape == shape and got.dtype == kw.get('out_dtype', torch.float32)
    assert torch.equal(got, want) and torch.equal(streamed, want)


def test_restore_y4m_with_cuts_is_the_shots_streams_concatenated():
    from edvr_amd.y4m import restore_y4m
    net = _net('M_noTSA')
    H, W = 36, 52
    v = _synthetic(H, W)[0]
    frames = U.encode_def(v, 'bt601', 'limited')
    tags = 'F25:1 Ip A1:1 C420jpeg'
    head = f'YUV4MPEG2 W{4 * W} H{4 * H} {tags}\n'.encode()
    with torch.no_grad():
        out, stats = io.BytesIO(), {}
        assert restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, tags)), out, read_frames=5, chunk=4, cuts=S.CUTS, stats=stats) == 22
        want = b''
        for a, b in S.shot_bounds(S.CUTS, 22):
            shot = io.BytesIO()
            assert restore_y4m(net, io.BytesIO(U.y4m_bytes(frames[a:b], H, W, tags)), shot, read_frames=5, chunk=4) == b - a
            assert shot.getvalue().startswith(head)
            want += shot.getvalue()[len(head):]
    net.check_offsets()
    assert out.getvalue().startswith(head) and out.getvalue()[len(head):] == want
    assert stats == dict(frames=22, cuts=S.CUTS, cut_scores=None, cut_mafd=None)
