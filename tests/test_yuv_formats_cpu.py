"""CPU: the Y'CbCr definition for every Y4M format (tests/util_yuv_formats.py) against the 8-bit 4:2:0 definition, against
itself across depths, against the float64 formula and against the reference's rgb2ycbcr / ycbcr2rgb bytes (the golden fixture is
4:4:4); the format-aware YUV4MPEG2 reader and writer; the flow of restore_y4m with CPU stand-ins for the device pieces; the command
line of scripts/restore_video.py."""
import importlib.util
import io
import os

import pytest
import torch

import util_yuv as U8
import util_yuv_formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(m, r) for m in ('bt601', 'bt709') for r in ('limited', 'full')]
BASES = ('420', '422', '444')


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('H, W', [(1, 1), (7, 9), (16, 16)])
def test_definition_at_420_is_the_8_bit_definition(H, W):
    g = torch.Generator().manual_seed(H * W)
    yuv = torch.randint(0, 256, (2, U8.frame_size(H, W)), generator=g, dtype=torch.uint8)
    rgb = torch.rand(2, 3, H, W, generator=g) * 1.2 - 0.1
    rgb.view(-1)[0] = float('nan')
    assert F.frame_size(H, W, '420') == U8.frame_size(H, W)
    for matrix, rng in COMBOS:
        for chroma in ('bilinear', 'nearest'):
            assert torch.equal(F.decode_def(yuv, H, W, '420', matrix, rng, chroma), U8.decode_def(yuv, H, W, matrix, rng, chroma)), (matrix, rng, chroma)
        assert torch.equal(F.encode_def(rgb, '420', matrix, rng), U8.encode_def(rgb, matrix, rng)), (matrix, rng)


def test_coefficients_by_depth():
    from edvr_amd import ops
    for matrix, rng in COMBOS:
        assert ops.yuv_coeffs(matrix, rng, depth=8) == ops.yuv_coeffs(matrix, rng)
        for a, b in zip(F.coeffs64(matrix, rng, 8), U8.coeffs64(matrix, rng)):  # bit-identical at 8 bits
            assert torch.equal(a, b)
        for depth in range(8, 17):
            m, mi, off = F.coeffs64(matrix, rng, depth)
            pm, pmi, poff = ops.yuv_coeffs(matrix, rng, depth)
            assert torch.equal(torch.tensor(pm, dtype=torch.float64), m) and torch.equal(torch.tensor(pmi, dtype=torch.float64), mi)
            assert poff == off.tolist()
            assert (m @ mi - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-13
            k = 2.0 ** (depth - 8)
            assert poff == ([16 * k, 128 * k, 128 * k] if rng == 'limited' else [0.0, 2.0 ** (depth - 1), 2.0 ** (depth - 1)])
            # white lands on the top of the range, grey has no chroma
            top = 235 * k if rng == 'limited' else 2 ** depth - 1
            assert abs(float(m[0].sum()) * 255.0 + poff[0] - top) < 1e-9 and m[1:].sum(1).abs().max() < 1e-12
    for bad in (7, 17, 10.5):
        with pytest.raises(ValueError):
            ops.yuv_coeffs('bt601', 'limited', depth=bad)


@pytest.mark.parametrize('base', BASES)
@pytest.mark.parametrize('depth', [10, 12, 16])
def test_limited_range_decode_is_the_same_at_every_depth(base, depth):
    """Samples 2^(d - 8) s at depth d decode to what s decodes to at depth 8: the power of two passes through the adjugate, the offsets and
    the chroma filter exactly."""
    H, W = 7, 9
    g = torch.Generator().manual_seed(depth)
    s8 = torch.randint(0, 256, (2, F.frame_size(H, W, base)), generator=g, dtype=torch.uint8)
    sd = F.to_bytes(s8.to(torch.int32) * 2 ** (depth - 8), depth)
    for matrix in ('bt601', 'bt709'):
        for chroma in ('bilinear', 'nearest'):
            assert torch.equal(F.decode_def(sd, H, W, F.name(base, depth), matrix, 'limited', chroma),
                               F.decode_def(s8, H, W, base, matrix, 'limited', chroma)), (matrix, chroma)


@pytest.mark.parametrize('depth', [8, 10, 12, 16])
def test_encode_is_within_one_lsb_of_the_float64_formula(depth):
    """4:4:4, so that every sample is one pixel's: the float32 definition against the same matrices in float64.  Bound: 1 LSB and at most
    0.5 % of the samples different (measured with this definition: 1 LSB, 0.22 % at 16 bits in the worst matrix x range)."""
    rgb = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    fmt = F.name('444', depth)
    for matrix, rng in COMBOS:
        got = F.to_samples(F.encode_def(rgb, fmt, matrix, rng), depth).reshape(4, 3, 64, 64)
        want = F.encode_ref64(rgb, fmt, matrix, rng)
        d = (got - want).abs()
        share = float((d > 0).float().mean())
        print(f'depth {depth} {matrix} {rng}: max {int(d.max())} LSB, {share * 100:.4f} % differ')
        assert int(d.max()) <= 1 and share <= 0.005, (matrix, rng)


def test_444_reproduces_the_reference_on_the_golden_fixture():
    """tests/golden/ycbcr.pt holds the reference's rgb2ycbcr bytes in 4:4:4 and its ycbcr2rgb of them: compared directly, no subsampling
    in between, under the conditions of the 8-bit 4:2:0 test."""
    g = torch.load(U8.GOLDEN)
    rgb, yc, mask = g['rgb'], g['ycbcr'], g['mask']
    n, H, W, _ = rgb.shape
    enc = F.encode_def(rgb.permute(0, 3, 1, 2).float() / 255.0, '444', 'bt601', 'limited').reshape(n, 3, H, W)
    for k, what in enumerate(('Y', 'Cb', 'Cr')):
        U8.golden_conditions(enc[:, k], yc[..., k], what)
    planes = yc.permute(0, 3, 1, 2).reshape(n, -1).contiguous()
    for chroma in ('nearest', 'bilinear'):  # nothing to upsample: the same
        dec = F.decode_def(planes, H, W, '444', 'bt601', 'limited', chroma)
        as_bytes = torch.round(dec * 255.0).to(torch.uint8).permute(0, 2, 3, 1)
        U8.golden_conditions(as_bytes[mask], g['back'][mask], 'decode (in gamut)')


def test_definition_edges():
    """Odd sizes: chroma planes are ((H + sy) >> sy, (W + sx) >> sx), an odd edge replicates in the encode; samples clamp at 2^d - 1."""
    g = torch.Generator().manual_seed(2)
    rgb = torch.rand(1, 3, 3, 5, generator=g)
    padded = torch.cat([rgb, rgb[:, :, -1:]], 2)
    padded = torch.cat([padded, padded[..., -1:]], 3)  # (1, 3, 4, 6): the replicated edge spelled out
    for fmt, (hc, wc) in (('420p10', (2, 3)), ('422p10', (3, 3)), ('444p10', (3, 5))):
        assert F.plane_shapes(3, 5, fmt) == ((3, 5), (hc, wc)) and F.frame_size(3, 5, fmt) == 2 * (15 + 2 * hc * wc)
        enc = F.encode_def(rgb, fmt, 'bt709', 'full')
        assert enc.shape == (1, F.frame_size(3, 5, fmt))
        _, cb, cr = F.split_planes(enc, 3, 5, fmt)
        _, cbp, crp = F.split_planes(F.encode_def(padded, fmt, 'bt709', 'full'), 4, 6, fmt)
        assert torch.equal(cb, cbp[:, :hc, :wc]) and torch.equal(cr, crp[:, :hc, :wc])
    for depth in (8, 10, 16):
        fmt = F.name('444', depth)
        white = F.to_samples(F.encode_def(torch.full((1, 3, 2, 2), 7.0), fmt, 'bt601', 'full'), depth)
        assert white[0, :4].tolist() == [2 ** depth - 1] * 4 and white[0, 4:].tolist() == [2 ** (depth - 1)] * 8
        flat = F.to_bytes(torch.full((1, 3 * 15), 2 ** (depth - 1) - 3), depth)
        for chroma in ('nearest', 'bilinear'):
            out = F.decode_def(flat, 3, 5, fmt, 'bt601', 'limited', chroma)
            assert out.shape == (1, 3, 3, 5) and all(float(out[0, k].min()) == float(out[0, k].max()) for k in range(3))
    # bits above the depth are not masked: a 10-bit word of 0x8000 is a very bright sample, not 0
    lo, hi = F.to_bytes(torch.tensor([[0, 512, 512]]), 10), F.to_bytes(torch.tensor([[0x8000, 512, 512]]), 10)
    assert float(F.decode_def(lo, 1, 1, '444p10').max()) == 0.0 and float(F.decode_def(hi, 1, 1, '444p10').min()) == 1.0


def test_format_names():
    from edvr_amd import ops, y4m
    assert ops.yuv_format('420') == (1, 1, 8, '420') and ops.yuv_format('422p10') == (1, 0, 10, '422p10')
    assert ops.yuv_format('444p16') == (0, 0, 16, '444p16') and ops.yuv_format('420p9') == (1, 1, 9, '420p9')
    for alias in ('420jpeg', '420mpeg2', '420paldv'):
        assert ops.yuv_format(alias) == (1, 1, 8, '420')
    for bad in ('mono', '411', '440', '444alpha', '420p8', '420p17', '420p', '420p010', '422jpeg', '420jpegp10', 'p10', '', None, 420, '444p1x'):
        with pytest.raises(ValueError):
            ops.yuv_format(bad)
    assert len(y4m.ALL_FORMATS) == 27 and len(set(y4m.ALL_FORMATS)) == 27
    for name in y4m.ALL_FORMATS:
        sx, sy, depth, canonical = ops.yuv_format(name)
        assert canonical == name and (sx, sy, depth) == F.parse(name)
        for H, W in ((1, 1), (3, 5), (6, 10)):
            assert ops.yuv_frame_size(H, W, name) == F.frame_size(H, W, name)
    assert ops.yuv_frame_size(3, 5) == ops.yuv420_frame_size(3, 5)


def test_ops_refuse_the_cpu():
    from edvr_amd import ops
    with pytest.raises(NotImplementedError):
        ops.yuv_to_rgb(torch.zeros(1, F.frame_size(4, 4, '422p10'), dtype=torch.uint8), 4, 4, '422p10')
    with pytest.raises(NotImplementedError):
        ops.rgb_to_yuv(torch.zeros(1, 3, 4, 4), '444p12')


# ---------------------------------------------------------------------------------------------------------------- YUV4MPEG2
ACCEPTED = [('C420jpeg', '420'), ('C420mpeg2', '420'), ('C420paldv', '420'), ('C420', '420'), ('', '420'), ('C422', '422'), ('C444', '444')] + \
    [(f'C{b}p{d}', f'{b}p{d}') for b in BASES for d in range(9, 17)]


@pytest.mark.parametrize('tag, fmt', ACCEPTED)
def test_reader_accepts_every_format(tag, fmt):
    from edvr_amd import y4m
    H, W = 7, 10
    frames = F.random_frames(2, H, W, fmt, seed=len(tag))
    data = F.y4m_bytes(frames, H, W, f'F25:1 Ip A1:1 {tag} XCOLORRANGE=FULL')
    r = y4m.Y4MReader(io.BytesIO(data), formats=y4m.ALL_FORMATS)
    sx, sy, depth = F.parse(fmt)
    assert (r.format, r.depth, r.subsampling, r.framesize) == (fmt, depth, (sx, sy), F.frame_size(H, W, fmt))
    assert (r.width, r.height, r.fps, r.aspect, r.range, r.chroma) == (W, H, '25:1', '1:1', 'full', tag[1:] or None)
    buf = r.read(3)
    assert buf.shape == (2, 6 + r.framesize) and torch.equal(buf[:, 6:], frames) and bytes(buf[1, :6].tolist()) == b'FRAME\n'
    assert y4m.Y4MReader(io.BytesIO(data), formats=[fmt]).format == fmt
    if fmt != '420':  # without formats=, and with a collection that does not name it, the reader refuses it as before
        with pytest.raises(ValueError, match='8-bit 4:2:0 only'):
            y4m.Y4MReader(io.BytesIO(data))
        with pytest.raises(ValueError, match='not among'):
            y4m.Y4MReader(io.BytesIO(data), formats=['420'])
    else:
        plain = y4m.Y4MReader(io.BytesIO(data))
        assert (plain.format, plain.depth, plain.subsampling, plain.framesize) == ('420', 8, (1, 1), U8.frame_size(H, W))


@pytest.mark.parametrize('tags', ['Ip Cmono', 'C411', 'Ip C440', 'C444alpha', 'It C422', 'Ib C420p10', 'Im C444', 'C420p8', 'C420p17', 'C422p32',
                                  'Cmono16', 'C420p', 'C444p1O'])
def test_reader_always_rejects(tags):
    from edvr_amd import y4m
    data = f'YUV4MPEG2 W10 H6 F25:1 {tags}\n'.encode()
    with pytest.raises(ValueError):
        y4m.Y4MReader(io.BytesIO(data), formats=y4m.ALL_FORMATS)
    with pytest.raises(ValueError):
        y4m.Y4MReader(io.BytesIO(data))
    with pytest.raises(ValueError):
        y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W10 H6 C420\n'), formats=['420p7'])


def test_reader_names_the_truncated_16_bit_frame():
    from edvr_amd import y4m
    frames = F.random_frames(4, 6, 10, '422p10', seed=4)
    data = F.y4m_bytes(frames, 6, 10, 'F25:1 Ip C422p10')
    r = y4m.Y4MReader(io.BytesIO(data[:-5]), formats=y4m.ALL_FORMATS)
    assert r.framesize == 240 and r.read(2).shape[0] == 2
    with pytest.raises(ValueError, match=r'frame 3 is truncated: 235 of 240 bytes'):
        r.read(2)


@pytest.mark.parametrize('H, W', [(6, 10), (7, 9), (1, 1)])
@pytest.mark.parametrize('fmt', ['422', '444p10', '420p12'])
def test_writer_then_reader_is_the_identity(H, W, fmt):
    from edvr_amd import y4m
    frames = F.random_frames(3, H, W, fmt, seed=H * W)
    src = F.y4m_bytes(frames, H, W, f'F30:1 Ip A1:1 C{fmt}')
    r = y4m.Y4MReader(io.BytesIO(src), formats=y4m.ALL_FORMATS)
    out = io.BytesIO()
    w = y4m.Y4MWriter(out, r.width, r.height, r.fps, r.aspect, r.range, format=r.format)
    assert (w.format, w.framesize) == (fmt, F.frame_size(H, W, fmt))
    w.write(r.read(2))
    w.write(r.read(2))
    w.write(r.read(2))  # empty
    assert out.getvalue() == src and w.frames_written == 3
    with pytest.raises(ValueError):
        w.write(torch.zeros(1, 5 + w.framesize, dtype=torch.uint8))
    with pytest.raises(ValueError):
        y4m.Y4MWriter(io.BytesIO(), 4, 4, format='411')
    head = io.BytesIO()
    y4m.Y4MWriter(head, 4, 2, '25:1', None, 'limited', '420mpeg2')  # an alias is written as 8-bit 4:2:0 is written today
    assert head.getvalue() == b'YUV4MPEG2 W4 H2 F25:1 Ip C420jpeg\n'


class _Nearest4:
    """Stands in for VideoRestorer on the CPU: 'restores' by x4 replication, chunk by chunk."""

    def __init__(self, net, out_dtype=None, **kwargs):
        assert out_dtype == torch.float32
        self.scale, self.kwargs = 4, kwargs

    def restore_chunks(self, frames, length=None):
        for piece in frames:
            yield piece.repeat_interleave(4, 2).repeat_interleave(4, 3)


@pytest.mark.parametrize('H, W, tags, out_format, fmt_in, fmt_out', [
    (8, 12, 'F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL', None, '420p10', '420p10'),
    (6, 10, 'F25:1 Ip A4:3 C420jpeg', '444p10', '420', '444p10'),
    (7, 9, 'F24:1 C422', None, '422', '422'),
    (6, 10, 'F25:1 C444p12', '420mpeg2', '444p12', '420'),
])
def test_restore_y4m_flow_formats(monkeypatch, H, W, tags, out_format, fmt_in, fmt_out):
    """restore_y4m with CPU stand-ins for the three device pieces (the definition for the two conversions): the output header carries
    the output's format, (4 W, 4 H), the input's F / A and range; the payload is the composition done by hand."""
    from edvr_amd import ops, video, y4m
    calls = []

    def to_rgb(yuv, h, w, fmt, matrix, rng, chroma):
        calls.append(('decode', fmt))
        return F.decode_def(yuv, h, w, fmt, matrix, rng, chroma)

    def to_yuv(rgb, fmt, matrix, rng, out):
        calls.append(('encode', fmt))
        return out.copy_(F.encode_def(rgb, fmt, matrix, rng))

    def never(*a, **k):
        raise AssertionError('the 8-bit 4:2:0 operators serve 8-bit 4:2:0 in AND out only')

    monkeypatch.setattr(ops, 'yuv_to_rgb', to_rgb)
    monkeypatch.setattr(ops, 'rgb_to_yuv', to_yuv)
    monkeypatch.setattr(ops, 'yuv420_to_rgb', never)
    monkeypatch.setattr(ops, 'rgb_to_yuv420', never)
    monkeypatch.setattr(video, 'VideoRestorer', _Nearest4)
    net = torch.nn.Linear(1, 1)
    frames = F.random_frames(3, H, W, fmt_in, seed=9)
    data = F.y4m_bytes(frames, H, W, tags)
    rng = 'full' if 'FULL' in tags else 'limited'
    out = io.BytesIO()
    assert y4m.restore_y4m(net, io.BytesIO(data), out, read_frames=2, chunk=3, out_format=out_format) == 3
    assert sorted(calls) == [('decode', fmt_in)] * 2 + [('encode', fmt_out)] * 2  # two reads of the input, two chunks of output
    src = y4m.Y4MReader(io.BytesIO(data), formats=y4m.ALL_FORMATS)
    r = y4m.Y4MReader(io.BytesIO(out.getvalue()), formats=y4m.ALL_FORMATS)
    assert (r.width, r.height, r.fps, r.aspect, r.range, r.format) == (4 * W, 4 * H, src.fps, src.aspect, rng, fmt_out)
    head = out.getvalue().split(b'\n')[0].decode().split()
    assert head[:3] == ['YUV4MPEG2', f'W{4 * W}', f'H{4 * H}'] and 'Ip' in head
    assert ('C420jpeg' if fmt_out == '420' else 'C' + fmt_out) in head and ('XCOLORRANGE=FULL' in head) == (rng == 'full')
    rgb = F.decode_def(frames, H, W, fmt_in, 'bt601', rng, 'bilinear').repeat_interleave(4, 2).repeat_interleave(4, 3)
    assert torch.equal(r.read(4)[:, 6:], F.encode_def(rgb, fmt_out, 'bt601', rng))
    with pytest.raises(ValueError):
        y4m.restore_y4m(net, io.BytesIO(data), io.BytesIO(), out_format='411')
    with pytest.raises(ValueError):
        y4m.restore_y4m(net, io.BytesIO(data), io.BytesIO(), matrix_out='bt2020')


# ---------------------------------------------------------------------------------------------------------------- the script
def test_restore_video_out_format_option(capsys):
    spec = importlib.util.spec_from_file_location('restore_video', os.path.join(ROOT, 'scripts', 'restore_video.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit) as e:
        mod.parse_args(['--help'])
    assert e.value.code == 0
    assert '--out-format' in capsys.readouterr().out
    assert '-strict -1' in mod.__doc__
    assert mod.parse_args(['-', '-']).out_format is None
    assert mod.parse_args(['-', '-', '--out-format', '420p10']).out_format == '420p10'
    assert mod.parse_args(['-', '-', '--out-format', '420jpeg']).out_format == '420'
    for bad in ('411', '420p8', 'yuv420p10le', '444p17'):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(['-', '-', '--out-format', bad])
        assert e.value.code == 2, bad
    capsys.readouterr()
