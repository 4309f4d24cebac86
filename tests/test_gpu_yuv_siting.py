"""GPU: chroma siting in csrc/yuv.hip - ops.yuv_to_rgb / ops.rgb_to_yuv and the 8-bit 4:2:0 pair under 'left' and
'topleft', bit for bit against the definition evaluated on the host (tests/util_yuv_siting.py), at the smallest shapes at which each
path can go wrong, on a dense aligned batch and inside a Y4M buffer; (centre, centre) through the sited entry points against the
existing calls; and edvr_amd.y4m.restore_y4m with sitings against the composition done by hand.

    (1, 1)             all clamps at once                       (6, 48)   three threads per row: the column halo of the encode crosses
    (2, 2)             the smallest even frame                            threads, the row-above halo crosses row groups
    (3, 5), (5, 7)     odd edges, scalar accesses               (16, 32)  dense and aligned: the 16-byte accesses on both sides
                                                                (17, 33)  one past a thread boundary in both axes"""
import ctypes
import io

import pytest
import torch

import util_yuv_formats as F
import util_yuv_siting as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (3, 5), (5, 7), (6, 48), (16, 32), (17, 33)]
FORMATS = ['420', '422', '420p10', '422p16']
SITED = ('left', 'topleft')
MARK = 0xA5


def _layouts(frames):
    """(n, framesize) host bytes -> the two device layouts: a dense batch at an aligned base, and the rows of a Y4M buffer - base offset
    6, stride framesize + 6 - which the kernels can only reach with scalar plane accesses."""
    dense = frames.cuda()
    buf = torch.full((frames.shape[0], frames.shape[1] + 6), MARK, dtype=torch.uint8, device='cuda')
    buf[:, 6:] = dense
    assert dense.data_ptr() % 16 == 0 and buf[:, 6:].data_ptr() % 16 == 6
    return (('dense', dense), ('y4m', buf[:, 6:]))


_DEFS = {}


def _decode_want(H, W, fmt, siting, dtype=torch.float32):
    key = ('dec', H, W, fmt, siting, dtype)
    if key not in _DEFS:
        frames = S.edge_frames(2, H, W, fmt, seed=31 * H + W)
        _DEFS[key] = (frames, S.decode_def(frames, H, W, fmt, 'bt709', 'limited', 'bilinear', siting, dtype))
    return _DEFS[key]


def _encode_want(H, W, fmt, siting):
    key = ('enc', H, W, fmt, siting)
    if key not in _DEFS:
        rgb = S.hostile_rgb(2, H, W, seed=17 * H + W)
        _DEFS[key] = (rgb, S.encode_def(rgb, fmt, 'bt601', 'full' if 'p' in fmt else 'limited', siting))
    return _DEFS[key]


# ---------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('H, W', SHAPES)
def test_sited_decode_matches_the_definition(H, W, fmt):
    from edvr_amd import ops
    for siting in SITED:
        frames, want = _decode_want(H, W, fmt, siting)
        for name, yuv in _layouts(frames):
            got = ops.yuv_to_rgb(yuv, H, W, fmt, 'bt709', 'limited', 'bilinear', siting)
            assert got.shape == want.shape and torch.equal(got.cpu(), want), (siting, name)
            if fmt == '420':
                assert torch.equal(ops.yuv420_to_rgb(yuv, H, W, 'bt709', 'limited', siting=siting).cpu(), want), (siting, name)
            # replication has no siting
            assert torch.equal(ops.yuv_to_rgb(yuv, H, W, fmt, 'bt709', 'limited', 'nearest', siting), ops.yuv_to_rgb(yuv, H, W, fmt, 'bt709', 'limited', 'nearest'))


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('H, W', SHAPES)
def test_sited_encode_matches_the_definition(H, W, fmt):
    from edvr_amd import ops
    rng = 'full' if 'p' in fmt else 'limited'
    for siting in SITED:
        rgb, want = _encode_want(H, W, fmt, siting)
        dev = rgb.cuda()
        got = ops.rgb_to_yuv(dev, fmt, 'bt601', rng, siting=siting)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), siting
        for name, out in _layouts(torch.zeros_like(want)):
            assert ops.rgb_to_yuv(dev, fmt, 'bt601', rng, out=out, siting=siting) is out
            assert torch.equal(out.cpu(), want), (siting, name)
            if fmt == '420':
                out.zero_()
                ops.rgb_to_yuv420(dev, 'bt601', rng, out=out, siting=siting)
                assert torch.equal(out.cpu(), want), (siting, name)
            if name == 'y4m':  # the six bytes in front of every frame are not the kernel's
                whole = torch.as_strided(out, (out.shape[0], out.shape[1] + 6), (out.stride(0), 1), out.storage_offset() - 6)
                assert bool((whole[:, :6] == MARK).all())


@pytest.mark.parametrize('H, W', SHAPES)
def test_sited_uint8_rgb_pair_matches_the_definition(H, W):
    """8-bit 4:2:0 with interleaved uint8 RGB on the other side: the U8 instances, whose halo loads read packed bytes."""
    from edvr_amd import ops
    rgb8 = torch.randint(0, 256, (2, H, W, 3), generator=torch.Generator().manual_seed(H * W), dtype=torch.uint8)
    rgb8.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    for siting in SITED:
        frames, want = _decode_want(H, W, '420', siting, torch.uint8)
        enc = S.encode_def(rgb8, '420', 'bt709', 'limited', siting)
        for name, yuv in _layouts(frames):
            got = ops.yuv420_to_rgb(yuv, H, W, 'bt709', 'limited', 'bilinear', torch.uint8, siting)
            assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want), (siting, name)
        for name, out in _layouts(torch.zeros_like(enc)):
            ops.rgb_to_yuv420(rgb8.cuda(), 'bt709', 'limited', out=out, siting=siting)
            assert torch.equal(out.cpu(), enc), (siting, name)


@pytest.mark.parametrize('fmt', ['444', '444p10'])
@pytest.mark.parametrize('H, W', SHAPES)
def test_444_ignores_siting(H, W, fmt):
    from edvr_amd import ops
    frames = S.edge_frames(2, H, W, fmt, seed=H + W)
    rgb = S.hostile_rgb(2, H, W, seed=H * W).cuda()
    for siting in SITED:
        for name, yuv in _layouts(frames):
            got = ops.yuv_to_rgb(yuv, H, W, fmt, siting=siting)
            assert torch.equal(got, ops.yuv_to_rgb(yuv, H, W, fmt)) and torch.equal(got.cpu(), S.decode_def(frames, H, W, fmt, siting=siting)), name
        got = ops.rgb_to_yuv(rgb, fmt, siting=siting)
        assert torch.equal(got, ops.rgb_to_yuv(rgb, fmt)) and torch.equal(got.cpu(), S.encode_def(rgb.cpu(), fmt, siting=siting))


def test_topleft_on_422_is_left():
    from edvr_amd import ops
    H, W = 6, 48
    frames, rgb = S.edge_frames(2, H, W, '422p10', seed=1).cuda(), S.hostile_rgb(2, H, W, seed=2).cuda()
    assert torch.equal(ops.yuv_to_rgb(frames, H, W, '422p10', siting='topleft'), ops.yuv_to_rgb(frames, H, W, '422p10', siting='left'))
    assert torch.equal(ops.rgb_to_yuv(rgb, '422p10', siting='topleft'), ops.rgb_to_yuv(rgb, '422p10', siting='left'))


# ---------------------------------------------------------------------------------------------------------------- (centre, centre)
def _coef(mat, off):
    return (ctypes.c_float * 12)(*[v for row in mat for v in row], *off)


@pytest.mark.parametrize('fmt', FORMATS + ['444'])
@pytest.mark.parametrize('H, W', SHAPES)
def test_center_through_the_sited_entry_points_is_the_existing_call(H, W, fmt):
    """Each existing entry point is its sited form at (0, 0): the same bytes, and `siting='center'` in Python the same again."""
    from edvr_amd import _lib, ops
    lib = _lib.lib()
    sx, sy, depth, _ = ops.yuv_format(fmt)
    m, mi, off = ops.yuv_coeffs('bt709', 'limited', depth)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    frames = S.edge_frames(2, H, W, fmt, seed=H * W + 1)
    rgb = S.hostile_rgb(2, H, W, seed=H * W + 2).cuda()
    enc_want = ops.rgb_to_yuv(rgb, fmt, 'bt709', 'limited')
    assert torch.equal(ops.rgb_to_yuv(rgb, fmt, 'bt709', 'limited', siting='center'), enc_want)
    for (name, yuv), (_, out) in zip(_layouts(frames), _layouts(torch.zeros_like(frames))):
        want = ops.yuv_to_rgb(yuv, H, W, fmt, 'bt709', 'limited')
        assert torch.equal(ops.yuv_to_rgb(yuv, H, W, fmt, 'bt709', 'limited', siting='center'), want)
        got = torch.zeros_like(want)
        assert lib.edvr_yuv_to_rgb_sited_f32(ptr(yuv), ptr(got), 2, H, W, sx, sy, depth, yuv.stride(0), 3 * H * W, _coef(mi, off), 1, 0, 0, stream) == 0
        assert torch.equal(got, want), name
        assert lib.edvr_rgb_to_yuv_sited_f32(ptr(rgb), ptr(out), 2, H, W, sx, sy, depth, 3 * H * W, out.stride(0), _coef(m, off), 0, 0, stream) == 0
        assert torch.equal(out, enc_want), name
        if fmt == '420':
            want8 = ops.yuv420_to_rgb(yuv, H, W, 'bt709', 'limited', 'bilinear', torch.uint8)
            got8 = torch.zeros_like(want8)
            assert lib.edvr_yuv420_to_rgb_sited_u8(ptr(yuv), ptr(got8), 2, H, W, yuv.stride(0), _coef(mi, off), 1, 0, 0, stream) == 0
            assert torch.equal(got8, want8), name
            out.zero_()
            assert lib.edvr_rgb_to_yuv420_sited_u8(ptr(want8), ptr(out), 2, H, W, out.stride(0), _coef(m, off), 0, 0, stream) == 0
            assert torch.equal(out, ops.rgb_to_yuv420(want8, 'bt709', 'limited')), name


def test_the_c_abi_refuses_what_is_no_siting():
    from edvr_amd import _lib, ops
    lib = _lib.lib()
    H, W = 4, 4
    _, mi, off = ops.yuv_coeffs('bt601', 'limited', 8)
    yuv = torch.zeros(1, 24, dtype=torch.uint8, device='cuda')
    rgb = torch.zeros(1, 3, H, W, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    yp, rp = ctypes.c_void_p(yuv.data_ptr()), ctypes.c_void_p(rgb.data_ptr())
    for bad in ((2, 0), (-1, 0), (1, 2), (0, 1)):
        assert lib.edvr_yuv_to_rgb_sited_f32(yp, rp, 1, H, W, 1, 1, 8, 24, 48, _coef(mi, off), 1, *bad, stream) != 0, bad
        assert lib.edvr_rgb_to_yuv_sited_f32(rp, yp, 1, H, W, 1, 1, 8, 48, 24, _coef(mi, off), *bad, stream) != 0, bad
    with pytest.raises(ValueError):
        ops.yuv_to_rgb(yuv, H, W, siting='top')
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(rgb, siting='centre')


# ---------------------------------------------------------------------------------------------------------------- restore_y4m
class _Nearest4:
    """Stands in for VideoRestorer: 'restores' by a fixed x4 nearest upsample, chunk by chunk, on the device."""

    def __init__(self, net, out_dtype=None, **kwargs):
        assert out_dtype == torch.float32
        self.scale = 4

    def restore_chunks(self, frames, length=None):
        for piece in frames:
            yield piece.repeat_interleave(4, 2).repeat_interleave(4, 3)


def test_restore_y4m_follows_the_tag_and_defaults_stay(monkeypatch):
    """A C420mpeg2 stream: with siting_in='auto' it is decoded as 'left', encoded as 'left' and tagged C420mpeg2 - the composition
    definition(left) -> x4 -> definition(left); under the defaults it is what it was before sitings existed, the composition of the
    unsited definitions under a C420jpeg tag, byte for byte."""
    from edvr_amd import video, y4m
    monkeypatch.setattr(video, 'VideoRestorer', _Nearest4)
    net = torch.nn.Linear(1, 1).cuda()
    H, W = 6, 20
    frames = S.edge_frames(3, H, W, '420', seed=8)
    data = F.y4m_bytes(frames, H, W, 'F25:1 Ip A1:1 C420mpeg2')

    def by_hand(decode, encode, tag):
        rgb = decode(frames).repeat_interleave(4, 2).repeat_interleave(4, 3)
        return F.y4m_bytes(encode(rgb), 4 * H, 4 * W, f'F25:1 Ip A1:1 {tag}')

    out = io.BytesIO()
    assert y4m.restore_y4m(net, io.BytesIO(data), out, siting_in='auto', read_frames=2) == 3
    assert out.getvalue() == by_hand(lambda f: S.decode_def(f, H, W, '420', siting='left'), lambda r: S.encode_def(r, '420', siting='left'), 'C420mpeg2')
    assert y4m.Y4MReader(io.BytesIO(out.getvalue())).siting == 'left'
    plain = io.BytesIO()
    assert y4m.restore_y4m(net, io.BytesIO(data), plain, read_frames=2) == 3
    assert plain.getvalue() == by_hand(lambda f: F.decode_def(f, H, W, '420'), lambda r: F.encode_def(r, '420'), 'C420jpeg')
    mixed = io.BytesIO()  # 10 bits out, top-left for a UHD encoder: the tag cannot say so, the samples do
    y4m.restore_y4m(net, io.BytesIO(data), mixed, siting_in='auto', siting_out='topleft', out_format='420p10', matrix_out='bt709', read_frames=3)
    assert mixed.getvalue() == by_hand(lambda f: S.decode_def(f, H, W, '420', siting='left'),
                                       lambda r: S.encode_def(r, '420p10', 'bt709', siting='topleft'), 'C420p10')
