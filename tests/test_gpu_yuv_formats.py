"""GPU: every format of csrc/yuv.hip (ops.yuv_to_rgb / ops.rgb_to_yuv) bit for bit against the definition evaluated on the host
(tests/util_yuv_formats.py) over formats, depths, sizes, layouts and both access widths of either side; against the 8-bit
4:2:0 operators at '420'; and edvr_amd.y4m.restore_y4m on 10-bit, 4:2:2 and 4:4:4 streams against the composition done by hand."""
import ctypes
import io

import pytest
import torch

import util_yuv_formats as F
from test_gpu_yuv import COMBOS, SIZES, _float_rgb

pytestmark = pytest.mark.gpu

BASES = ('420', '422', '444')
DEPTHS = (8, 10, 12, 16)


@pytest.mark.parametrize('base', BASES)
@pytest.mark.parametrize('H, W', SIZES)
def test_decode_matches_the_definition(H, W, base):
    from edvr_amd import ops
    for depth in DEPTHS:
        fmt = F.name(base, depth)
        for n in (1, 3):
            yuv = F.random_frames(n, H, W, fmt, seed=100 * H + W + n + depth, above=3)  # a few words above 2^d - 1: not masked
            dev = yuv.cuda()
            for matrix, rng in COMBOS:
                for chroma in ('bilinear', 'nearest'):
                    got = ops.yuv_to_rgb(dev, H, W, fmt, matrix, rng, chroma)
                    want = F.decode_def(yuv, H, W, fmt, matrix, rng, chroma)
                    assert got.dtype == torch.float32 and got.shape == want.shape == (n, 3, H, W)
                    assert torch.equal(got.cpu(), want), (fmt, n, matrix, rng, chroma)
    assert torch.equal(ops.yuv_to_rgb(dev, H, W, fmt).cpu(), F.decode_def(yuv, H, W, fmt, 'bt601', 'limited', 'bilinear'))  # the defaults


@pytest.mark.parametrize('base', BASES)
@pytest.mark.parametrize('H, W', SIZES)
def test_encode_matches_the_definition(H, W, base):
    from edvr_amd import ops
    for n in (1, 3):
        wide = torch.zeros(n, 4, H, W)
        wide[:, :3] = _float_rgb(n, H, W, 11 * H + W + n)
        strided = wide.cuda()[:, :3]  # images 4 H W floats apart
        assert not strided.is_contiguous() or n == 1
        for depth in DEPTHS:
            fmt = F.name(base, depth)
            for matrix, rng in COMBOS:
                got = ops.rgb_to_yuv(strided, fmt, matrix, rng)
                assert got.dtype == torch.uint8 and got.shape == (n, F.frame_size(H, W, fmt))
                assert torch.equal(got.cpu(), F.encode_def(wide[:, :3], fmt, matrix, rng)), (fmt, n, matrix, rng)


def _layouts(n, fs, wide, device):
    """name -> (whole buffer, the (n, fs) batch view into it); `wide`: 16-bit samples, whose addresses stay even."""
    out, off = {}, 2 if wide else 1
    buf = torch.full((n * fs,), 0xAB, dtype=torch.uint8, device=device)
    out['dense, 16-byte aligned'] = (buf, buf.view(n, fs))
    buf = torch.full((n * fs + 16,), 0xAB, dtype=torch.uint8, device=device)
    out['dense, off'] = (buf, buf[off:off + n * fs].view(n, fs))
    buf = torch.full((n, fs + 6), 0xAB, dtype=torch.uint8, device=device)
    out['y4m buffer'] = (buf, buf[:, 6:])
    buf = torch.full((n, fs + 32), 0xAB, dtype=torch.uint8, device=device)
    out['aligned rows with a gap'] = (buf, buf[:, :fs])
    return out, off


@pytest.mark.parametrize('fmt', [F.name(b, d) for b in BASES for d in (8, 10)] + ['420p16', '444p12'])
@pytest.mark.parametrize('H, W', [(16, 16), (64, 96)])
def test_layouts_and_access_widths_agree(H, W, fmt):
    """The same frames dense, dense but off the 16-byte grid, inside a Y4M buffer (stride framesize + 6, 6 bytes in) and in aligned rows:
    identical results from the 16-byte and the scalar paths, on either side, and no byte outside the frames written."""
    from edvr_amd import _lib, ops
    n, fs = 3, F.frame_size(H, W, fmt)
    sx, sy, depth = F.parse(fmt)
    yuv = F.random_frames(n, H, W, fmt, seed=H + W, above=3)
    rgb = _float_rgb(n, H, W, H * W)
    want_dec = {c: F.decode_def(yuv, H, W, fmt, 'bt709', 'limited', c) for c in ('bilinear', 'nearest')}
    want_enc = F.encode_def(rgb, fmt, 'bt709', 'limited')
    assert fs % 16 == 0
    layouts, off = _layouts(n, fs, depth > 8, 'cuda')
    for name, (buf, view) in layouts.items():
        view.copy_(yuv.cuda())
        assert view.stride(1) == 1 and (view.data_ptr() % 16 == 0) == ('aligned' in name) and view.data_ptr() % off == 0
        for c, want in want_dec.items():
            assert torch.equal(ops.yuv_to_rgb(view, H, W, fmt, 'bt709', 'limited', c).cpu(), want), (name, c)
        buf.fill_(0xAB)
        got = ops.rgb_to_yuv(rgb.cuda(), fmt, 'bt709', 'limited', out=view)
        assert got is view and torch.equal(view.cpu(), want_enc), name
        if buf.dim() == 2:  # the bytes between the frames are untouched
            gap = buf[:, :6] if name == 'y4m buffer' else buf[:, fs:]
        else:
            gap = torch.cat([buf[:off], buf[off + n * fs:]]) if 'off' in name else buf[n * fs:]
        assert bool((gap == 0xAB).all()), name
    # the RGB side off 16 bytes: float planes one float in (the encode reads them; the decode writes them through the C ABI)
    flat = torch.zeros(n * 3 * H * W + 4, device='cuda')
    shifted = flat[1:1 + n * 3 * H * W].view(n, 3, H, W)
    shifted.copy_(rgb.cuda())
    assert shifted.data_ptr() % 16 == 4 and torch.equal(ops.rgb_to_yuv(shifted, fmt, 'bt709', 'limited').cpu(), want_enc)
    _, mi, o3 = ops.yuv_coeffs('bt709', 'limited', depth)
    coef = (ctypes.c_float * 12)(*[v for row in mi for v in row], *o3)
    dev = yuv.cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flat.zero_()
    _lib.check(_lib.lib().edvr_yuv_to_rgb_f32(ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(shifted.data_ptr()), n, H, W, sx, sy, depth, fs,
                                              3 * H * W, coef, 1, stream), 'edvr_yuv_to_rgb_f32')
    assert torch.equal(shifted.cpu(), want_dec['bilinear']) and float(flat[0]) == 0.0 and float(flat[-1]) == 0.0


@pytest.mark.parametrize('H, W', [(18, 34), (64, 96)])
def test_420_is_the_8_bit_420_operators(H, W):
    from edvr_amd import ops
    yuv = F.random_frames(3, H, W, '420', seed=H).cuda()
    rgb = _float_rgb(3, H, W, W).cuda()
    for matrix, rng in COMBOS:
        for chroma in ('bilinear', 'nearest'):
            assert torch.equal(ops.yuv_to_rgb(yuv, H, W, '420', matrix, rng, chroma), ops.yuv420_to_rgb(yuv, H, W, matrix, rng, chroma))
        assert torch.equal(ops.rgb_to_yuv(rgb, '420', matrix, rng), ops.rgb_to_yuv420(rgb, matrix, rng))
    assert torch.equal(ops.yuv_to_rgb(yuv, H, W), ops.yuv420_to_rgb(yuv, H, W)) and torch.equal(ops.rgb_to_yuv(rgb), ops.rgb_to_yuv420(rgb))


def test_errors():
    from edvr_amd import _lib, ops
    H, W, fmt = 6, 10, '422p10'
    fs = F.frame_size(H, W, fmt)
    yuv = F.random_frames(2, H, W, fmt, seed=1).cuda()
    rgb = torch.rand(2, 3, H, W, device='cuda')
    # 16-bit samples: an odd base address, an odd row stride
    flat = torch.zeros(2 * fs + 2, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='even'):
        ops.yuv_to_rgb(flat[1:1 + 2 * fs].view(2, fs), H, W, fmt)
    with pytest.raises(ValueError, match='even'):
        ops.rgb_to_yuv(rgb, fmt, out=flat[1:1 + 2 * fs].view(2, fs))
    rows = torch.zeros(2, fs + 1, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='even'):
        ops.yuv_to_rgb(rows[:, :fs], H, W, fmt)
    with pytest.raises(ValueError, match='even'):
        ops.rgb_to_yuv(rgb, fmt, out=rows[:, :fs])
    ops.yuv_to_rgb(rows[:, :F.frame_size(H, W, '422')], H, W, '422')  # bytes may lie anywhere
    ops.yuv_to_rgb(flat[1:1 + 2 * F.frame_size(H, W, '422')].view(2, -1), H, W, '422')
    with pytest.raises(NotImplementedError):
        ops.yuv_to_rgb(yuv.cpu(), H, W, fmt)
    with pytest.raises(NotImplementedError):
        ops.rgb_to_yuv(rgb.cpu(), fmt)
    with pytest.raises(NotImplementedError):
        ops.yuv_to_rgb(yuv.float(), H, W, fmt)
    with pytest.raises(NotImplementedError):
        ops.rgb_to_yuv((rgb * 255).to(torch.uint8), fmt)  # uint8 RGB stays with rgb_to_yuv420
    with pytest.raises(NotImplementedError):
        ops.rgb_to_yuv(rgb, fmt, out=torch.zeros(2, fs, device='cuda'))
    with pytest.raises(ValueError, match='stride'):
        ops.yuv_to_rgb(torch.zeros(2, 2 * fs, dtype=torch.uint8, device='cuda')[:, ::2], H, W, fmt)
    with pytest.raises(ValueError, match='shorter'):
        ops.yuv_to_rgb(yuv[:, :fs - 2], H, W, fmt)
    with pytest.raises(ValueError, match='shorter'):
        ops.yuv_to_rgb(yuv, H, W, '444p10')  # the same bytes are too few for 4:4:4
    with pytest.raises(ValueError, match='shorter'):
        ops.rgb_to_yuv(rgb, fmt, out=torch.zeros(2, fs - 2, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.rgb_to_yuv(rgb, fmt, out=torch.zeros(3, fs, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.yuv_to_rgb(yuv.view(-1), H, W, fmt)
    with pytest.raises(ValueError):
        ops.rgb_to_yuv(rgb[:, :2], fmt)
    for kw in (dict(fmt='411'), dict(fmt='420p8'), dict(fmt='444p17'), dict(matrix='bt2020'), dict(range='pc'), dict(chroma='bicubic')):
        with pytest.raises(ValueError):
            ops.yuv_to_rgb(yuv, H, W, **kw)
    for kw in (dict(fmt='mono'), dict(matrix='rec709'), dict(range='tv')):
        with pytest.raises(ValueError):
            ops.rgb_to_yuv(rgb, **kw)
    as_floats = torch.zeros(2 * 3 * H * W, device='cuda')
    with pytest.raises(ValueError, match='overlaps'):
        ops.rgb_to_yuv(as_floats.view(2, 3, H, W), fmt, out=as_floats.view(torch.uint8)[:2 * fs].view(2, fs))
    # the C ABI refuses what the Python layer never sends
    _, mi, o3 = ops.yuv_coeffs('bt601', 'limited', 10)
    coef = (ctypes.c_float * 12)(*[v for row in mi for v in row], *o3)
    out = torch.zeros(2, 3, H, W, device='cuda')
    yp, op, stream = ctypes.c_void_p(yuv.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dec, enc = _lib.lib().edvr_yuv_to_rgb_f32, _lib.lib().edvr_rgb_to_yuv_f32
    for (sx, sy, depth, stride, base) in ((1, 0, 7, fs, 0), (1, 0, 17, fs, 0), (0, 1, 10, fs, 0), (2, 0, 10, fs, 0), (1, 0, 10, fs - 2, 0),
                                          (1, 0, 10, fs + 1, 0), (1, 0, 10, fs, 1)):
        assert dec(ctypes.c_void_p(yuv.data_ptr() + base), op, 2, H, W, sx, sy, depth, stride, 3 * H * W, coef, 1, stream) != 0
        assert enc(op, ctypes.c_void_p(yuv.data_ptr() + base), 2, H, W, sx, sy, depth, 3 * H * W, stride, coef, stream) != 0
    assert dec(None, op, 2, H, W, 1, 0, 10, fs, 3 * H * W, coef, 1, stream) != 0 and dec(yp, op, 0, H, W, 1, 0, 10, fs, 3 * H * W, coef, 1, stream) != 0
    assert dec(yp, op, 2, H, W, 1, 0, 10, fs, 3 * H * W - 1, coef, 1, stream) != 0 and enc(op, yp, 2, H, 0, 1, 0, 10, 3 * H * W, fs, coef, stream) != 0
    assert dec(yp, op, 2, H, W, 1, 0, 10, fs, 3 * H * W, coef, 1, stream) == 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- restore_y4m
def _by_hand(net, frames, H, W, fmt_in, fmt_out, tags_out, **kw):
    from edvr_amd import VideoRestorer, ops
    rgb = ops.yuv_to_rgb(frames.cuda(), H, W, fmt_in, 'bt601', 'limited', 'bilinear')
    out = VideoRestorer(net, out_dtype=torch.float32, **kw).restore(rgb)
    assert out.shape == (frames.shape[0], 3, 4 * H, 4 * W)
    return F.y4m_bytes(ops.rgb_to_yuv(out, fmt_out, 'bt601', 'limited').cpu(), 4 * H, 4 * W, tags_out)


@pytest.mark.parametrize('H, W, tag, out_format, tag_out, kw', [
    (20, 24, 'C420p10', None, 'C420p10', dict(chunk=4)),
    (18, 22, 'C422', None, 'C422', dict(chunk=4, pad_mode='reflect')),
    (20, 24, 'C444p12', None, 'C444p12', dict(chunk=4, cuts=[3])),
    (20, 24, 'C420jpeg', '420p10', 'C420p10', dict(chunk=4)),  # 8 bits in, the float32 result quantised once, to 10 bits
])
def test_restore_y4m_is_the_composition_by_hand(H, W, tag, out_format, tag_out, kw):
    from edvr_amd import ops
    from edvr_amd.y4m import restore_y4m
    from test_gpu_yuv import _net
    net = _net()
    fmt_in, fmt_out = ops.yuv_format(tag[1:])[3], ops.yuv_format(tag_out[1:])[3]
    frames = F.random_frames(7, H, W, fmt_in, seed=H * W)
    data = F.y4m_bytes(frames, H, W, f'F25:1 Ip A1:1 {tag}')
    with torch.no_grad():
        want = _by_hand(net, frames, H, W, fmt_in, fmt_out, f'F25:1 Ip A1:1 {tag_out}', **kw)
        out = io.BytesIO()
        assert restore_y4m(net, io.BytesIO(data), out, read_frames=3, out_format=out_format, **kw) == 7
    net.check_offsets()
    assert want.startswith(f'YUV4MPEG2 W{4 * W} H{4 * H} F25:1 Ip A1:1 {tag_out}\nFRAME\n'.encode())
    assert len(want) == len(want.split(b'\n')[0]) + 1 + 7 * (6 + F.frame_size(4 * H, 4 * W, fmt_out))
    assert out.getvalue() == want
