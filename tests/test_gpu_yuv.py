"""GPU: the 8-bit 4:2:0 instances of csrc/yuv.hip (ops.yuv420_to_rgb / ops.rgb_to_yuv420, float32 and uint8 RGB) bit for bit against the definition evaluated on the host (tests/util_yuv.py),
over sizes, layouts and both access-width paths; the golden fixture of the reference through the kernels; and edvr_amd.y4m.restore_y4m
against the composition done by hand."""
import ctypes
import io
import os

import pytest
import torch

import util_yuv as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (16, 16), (18, 34), (37, 53), (64, 96)]
COMBOS = [(m, r) for m in ('bt601', 'bt709') for r in ('limited', 'full')]


def _yuv(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, U.frame_size(H, W)), generator=g, dtype=torch.uint8)


def _float_rgb(n, H, W, seed):
    """Floats a network could return: mostly inside [0, 1], some outside, bytes / 255, exact halves after scaling, non-finite ones."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, H, W, generator=g) * 1.4 - 0.2
    pick = torch.rand(n, 3, H, W, generator=g)
    k = torch.randint(0, 256, (n, 3, H, W), generator=g).float()
    x = torch.where(pick < 0.2, k / 255.0, x)
    x = torch.where((pick >= 0.2) & (pick < 0.3), (k.clamp(max=254) + 0.5) / 255.0, x)
    x = torch.where((pick >= 0.3) & (pick < 0.35), torch.full_like(x, 0.5), x)  # x 255 = 127.5 exactly
    flat = x.view(-1)
    if flat.numel() >= 4:
        flat[0], flat[1], flat[2], flat[3] = float('nan'), float('inf'), float('-inf'), -0.0
    return x


@pytest.mark.parametrize('H, W', SIZES)
def test_decode_matches_the_definition(H, W):
    from edvr_amd import ops
    for n in (1, 3):
        yuv = _yuv(n, H, W, 100 * H + W + n)
        dev = yuv.cuda()
        for matrix, rng in COMBOS:
            for chroma in ('bilinear', 'nearest'):
                for dt in (torch.float32, torch.uint8):
                    got = ops.yuv420_to_rgb(dev, H, W, matrix, rng, chroma, dt)
                    want = U.decode_def(yuv, H, W, matrix, rng, chroma, dt)
                    assert got.dtype == dt and got.shape == want.shape
                    assert torch.equal(got.cpu(), want), (n, matrix, rng, chroma, dt)
    assert torch.equal(ops.yuv420_to_rgb(dev, H, W).cpu(), U.decode_def(yuv, H, W, 'bt601', 'limited', 'bilinear'))  # the defaults


@pytest.mark.parametrize('H, W', SIZES)
def test_encode_matches_the_definition(H, W):
    from edvr_amd import ops
    for n in (1, 3):
        g = torch.Generator().manual_seed(7 * H + W + n)
        as_bytes = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
        wide = torch.zeros(n, 4, H, W)
        wide[:, :3] = _float_rgb(n, H, W, 11 * H + W + n)
        wide_dev = wide.cuda()
        strided = wide_dev[:, :3]  # images 4 H W floats apart
        assert not strided.is_contiguous() or n == 1
        for matrix, rng in COMBOS:
            for src, dev in ((as_bytes, as_bytes.cuda()), (wide[:, :3], strided)):
                got = ops.rgb_to_yuv420(dev, matrix, rng)
                assert got.dtype == torch.uint8 and got.shape == (n, U.frame_size(H, W))
                assert torch.equal(got.cpu(), U.encode_def(src, matrix, rng)), (n, matrix, rng, src.dtype)


def _layouts(n, fs, device):
    """name -> (whole buffer, the (n, fs) batch view into it)."""
    out = {}
    buf = torch.full((n * fs,), 0xAB, dtype=torch.uint8, device=device)
    out['dense, 16-byte aligned'] = (buf, buf.view(n, fs))
    buf = torch.full((n * fs + 16,), 0xAB, dtype=torch.uint8, device=device)
    out['dense, 1 byte off'] = (buf, buf[1:1 + n * fs].view(n, fs))
    buf = torch.full((n, fs + 6), 0xAB, dtype=torch.uint8, device=device)
    out['y4m buffer'] = (buf, buf[:, 6:])
    buf = torch.full((n, fs + 32), 0xAB, dtype=torch.uint8, device=device)
    out['aligned rows with a gap'] = (buf, buf[:, :fs])
    return out


@pytest.mark.parametrize('H, W', [(16, 16), (64, 96)])
def test_layouts_and_access_widths_agree(H, W):
    """The same frames dense, dense but misaligned, inside a Y4M buffer (stride framesize + 6, 6 bytes in) and in aligned rows: identical
    results from the 16-byte and the scalar paths, on either side, and no byte outside the frames written."""
    from edvr_amd import _lib, ops
    n, fs = 3, U.frame_size(H, W)
    yuv = _yuv(n, H, W, H + W)
    rgbf = _float_rgb(n, H, W, H * W)
    rgb8 = torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    want_dec = {(c, dt): U.decode_def(yuv, H, W, 'bt709', 'limited', c, dt) for c in ('bilinear', 'nearest') for dt in (torch.float32, torch.uint8)}
    want_enc = {torch.float32: U.encode_def(rgbf, 'bt709', 'limited'), torch.uint8: U.encode_def(rgb8, 'bt709', 'limited')}
    assert fs % 16 == 0
    for name, (buf, view) in _layouts(n, fs, 'cuda').items():
        view.copy_(yuv.cuda())
        assert view.stride(1) == 1 and (view.data_ptr() % 16 == 0) == ('aligned' in name)
        for (c, dt), want in want_dec.items():
            assert torch.equal(ops.yuv420_to_rgb(view, H, W, 'bt709', 'limited', c, dt).cpu(), want), (name, c, dt)
        for src in (rgbf, rgb8):
            buf.fill_(0xAB)
            got = ops.rgb_to_yuv420(src.cuda(), 'bt709', 'limited', out=view)
            assert got is view and torch.equal(view.cpu(), want_enc[src.dtype]), (name, src.dtype)
            if buf.dim() == 2:  # the bytes between the frames are untouched
                gap = buf[:, :6] if name == 'y4m buffer' else buf[:, fs:]
            else:
                gap = torch.cat([buf[:1], buf[1 + n * fs:]]) if 'off' in name else buf[n * fs:]
            assert bool((gap == 0xAB).all()), name
    # the RGB side off 16 bytes: float planes one float in, bytes one byte in (the encode reads them; the decode writes them through the C ABI)
    flat = torch.zeros(n * 3 * H * W + 4, device='cuda')
    off = flat[1:1 + n * 3 * H * W].view(n, 3, H, W)
    off.copy_(rgbf.cuda())
    assert off.data_ptr() % 16 == 4 and torch.equal(ops.rgb_to_yuv420(off, 'bt709', 'limited').cpu(), want_enc[torch.float32])
    _, mi, o3 = ops.yuv_coeffs('bt709', 'limited')
    coef = (ctypes.c_float * 12)(*[v for row in mi for v in row], *o3)
    dev = yuv.cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flat.zero_()
    _lib.check(_lib.lib().edvr_yuv420_to_rgb_f32(ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(off.data_ptr()), n, H, W, fs, 3 * H * W, coef, 1,
                                                 stream), 'edvr_yuv420_to_rgb_f32')
    assert torch.equal(off.cpu(), want_dec[('bilinear', torch.float32)]) and float(flat[0]) == 0.0 and float(flat[-1]) == 0.0
    flat8 = torch.zeros(n * 3 * H * W + 16, dtype=torch.uint8, device='cuda')
    off8 = flat8[1:1 + n * 3 * H * W].view(n, H, W, 3)
    for c in ('bilinear', 'nearest'):
        flat8.zero_()
        _lib.check(_lib.lib().edvr_yuv420_to_rgb_u8(ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(off8.data_ptr()), n, H, W, fs, coef,
                                                    int(c == 'bilinear'), stream), 'edvr_yuv420_to_rgb_u8')
        assert torch.equal(off8.cpu(), want_dec[(c, torch.uint8)]) and int(flat8[0]) == 0 and int(flat8[-15:].sum()) == 0, c
    off8.copy_(rgb8.cuda())
    assert torch.equal(ops.rgb_to_yuv420(off8, 'bt709', 'limited').cpu(), want_enc[torch.uint8])
    # the float32 8-bit 4:2:0 encode of the C ABI, which the operators no longer pass through
    m, _, _ = ops.yuv_coeffs('bt709', 'limited')
    coef = (ctypes.c_float * 12)(*[v for row in m for v in row], *o3)
    src, enc = rgbf.cuda(), torch.zeros(n, fs, dtype=torch.uint8, device='cuda')
    _lib.check(_lib.lib().edvr_rgb_to_yuv420_f32(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(enc.data_ptr()), n, H, W, 3 * H * W, fs, coef,
                                                 stream), 'edvr_rgb_to_yuv420_f32')
    assert torch.equal(enc.cpu(), want_enc[torch.float32])


def test_golden_fixture_through_the_kernels():
    """The reference's rgb2ycbcr / ycbcr2rgb (tests/golden/ycbcr.pt) against the KERNELS, under the conditions of tests/test_yuv_cpu.py."""
    from edvr_amd import ops
    from util_yuv import GOLDEN, golden_conditions, golden_yuv
    g = torch.load(GOLDEN)
    rgb, yc, mask = g['rgb'], g['ycbcr'], g['mask']
    n, H, W, _ = rgb.shape
    assert float(mask.float().mean()) >= 0.95
    for src in (rgb, rgb.permute(0, 3, 1, 2).float() / 255.0):
        enc = ops.rgb_to_yuv420(src.cuda(), 'bt601', 'limited').cpu()
        hw, q = H * W, (H // 2) * (W // 2)
        golden_conditions(enc[:, :hw].reshape(n, H, W), yc[..., 0], 'Y')
        golden_conditions(enc[:, hw:hw + q].reshape(n, H // 2, W // 2), yc[:, ::2, ::2, 1], 'Cb per block')
        golden_conditions(enc[:, hw + q:].reshape(n, H // 2, W // 2), yc[:, ::2, ::2, 2], 'Cr per block')
    dec = ops.yuv420_to_rgb(golden_yuv(g).cuda(), H, W, 'bt601', 'limited', 'nearest', torch.uint8).cpu()
    golden_conditions(dec[mask], g['back'][mask], 'decode (in gamut)')


@pytest.mark.parametrize('matrix, rng', COMBOS)
def test_round_trip_of_444_equivalent_content(matrix, rng):
    """2 x 2-constant RGB bytes lose nothing to the subsampling: encode then decode ('nearest') is within 2 LSB of the source (one
    rounding to YUV bytes, one to RGB bytes; 2 is what the definition gives on the CPU)."""
    from edvr_amd import ops
    g = torch.Generator().manual_seed(12)
    small = torch.randint(0, 256, (2, 19, 27, 3), generator=g, dtype=torch.uint8)
    rgb = small.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous().cuda()
    back = ops.yuv420_to_rgb(ops.rgb_to_yuv420(rgb, matrix, rng), 38, 54, matrix, rng, 'nearest', torch.uint8)
    d = (back.int() - rgb.int()).abs()
    print(f'{matrix} {rng}: max {int(d.max())}')
    assert int(d.max()) <= 2


def test_errors():
    from edvr_amd import ops
    H, W = 6, 10
    fs = U.frame_size(H, W)
    yuv = _yuv(2, H, W, 1).cuda()
    rgb = torch.rand(2, 3, H, W, device='cuda')
    with pytest.raises(NotImplementedError):
        ops.yuv420_to_rgb(yuv.cpu(), H, W)
    with pytest.raises(NotImplementedError):
        ops.rgb_to_yuv420(rgb.cpu())
    with pytest.raises(NotImplementedError):
        ops.yuv420_to_rgb(yuv.float(), H, W)
    with pytest.raises(NotImplementedError):
        ops.rgb_to_yuv420(rgb.half())
    with pytest.raises(NotImplementedError):
        ops.rgb_to_yuv420(rgb, out=torch.zeros(2, fs, device='cuda'))
    with pytest.raises(ValueError, match='stride'):
        ops.yuv420_to_rgb(torch.zeros(2, 2 * fs, dtype=torch.uint8, device='cuda')[:, ::2], H, W)
    with pytest.raises(ValueError, match='stride'):
        ops.rgb_to_yuv420(rgb, out=torch.zeros(2, 2 * fs, dtype=torch.uint8, device='cuda')[:, ::2])
    with pytest.raises(ValueError, match='shorter'):
        ops.yuv420_to_rgb(yuv[:, :fs - 1], H, W)
    with pytest.raises(ValueError, match='shorter'):
        ops.rgb_to_yuv420(rgb, out=torch.zeros(2, fs - 1, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(rgb, out=torch.zeros(3, fs, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb(yuv.view(-1), H, W)
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420(rgb[:, :2])
    for kw in (dict(matrix='bt2020'), dict(range='pc'), dict(chroma='bicubic'), dict(out_dtype=torch.float16)):
        with pytest.raises(ValueError):
            ops.yuv420_to_rgb(yuv, H, W, **kw)
    for kw in (dict(matrix='rec709'), dict(range='tv')):
        with pytest.raises(ValueError):
            ops.rgb_to_yuv420(rgb, **kw)
    as_bytes = torch.zeros(2 * H * W * 3, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='overlaps'):
        ops.rgb_to_yuv420(as_bytes.view(2, H, W, 3), out=as_bytes[:2 * fs].view(2, fs))


# ---------------------------------------------------------------------------------------------------------------- restore_y4m
_NET = {}


def _net():
    if 'net' not in _NET:
        from util_edvr import build
        net, _, _ = build('M_noTSA')
        _NET['net'] = net.cuda().eval()
    return _NET['net']


TAGS = 'F25:1 Ip A1:1 C420jpeg'


def _by_hand(net, frames, H, W, m_in, m_out, rng='limited', **kw):
    from edvr_amd import VideoRestorer, ops
    rgb = ops.yuv420_to_rgb(frames.cuda(), H, W, m_in, rng, 'bilinear')
    out = VideoRestorer(net, out_dtype=torch.float32, **kw).restore(rgb)
    assert out.shape == (frames.shape[0], 3, 4 * H, 4 * W)
    return U.y4m_bytes(ops.rgb_to_yuv420(out, m_out, rng).cpu(), 4 * H, 4 * W, TAGS)


@pytest.mark.parametrize('H, W, kw, matrices', [
    (20, 24, dict(chunk=4), ('bt601', 'bt601')),
    (18, 22, dict(chunk=4, pad_mode='reflect'), ('bt601', 'bt601')),
    (20, 24, dict(chunk=4, self_ensemble='flip4'), ('bt601', 'bt601')),
    (16, 320, dict(chunk=4), ('bt601', 'bt709')),  # 1280 columns out: the result is written as BT.709
])
def test_restore_y4m_is_the_composition_by_hand(H, W, kw, matrices):
    from edvr_amd.y4m import restore_y4m
    net = _net()
    frames = _yuv(7, H, W, H * W)
    data = U.y4m_bytes(frames, H, W, TAGS)
    with torch.no_grad():
        want = _by_hand(net, frames, H, W, *matrices, **kw)
        out = io.BytesIO()
        assert restore_y4m(net, io.BytesIO(data), out, read_frames=3, **kw) == 7  # the default matrices: the size rule
        explicit = io.BytesIO()
        restore_y4m(net, io.BytesIO(data), explicit, matrix_in=matrices[0], matrix_out=matrices[1], read_frames=3, **kw)
    net.check_offsets()
    assert want.startswith(f'YUV4MPEG2 W{4 * W} H{4 * H} {TAGS}\nFRAME\n'.encode())
    assert out.getvalue() == want
    assert explicit.getvalue() == want
