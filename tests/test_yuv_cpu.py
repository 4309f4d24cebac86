"""CPU: the Y'CbCr 4:2:0 definition (tests/util_yuv.py) against the reference's rgb2ycbcr / ycbcr2rgb through the golden
fixture, the YUV4MPEG2 reader and writer of edvr_amd/y4m.py, the flow of restore_y4m with CPU stand-ins for the device pieces, and the
command line of scripts/restore_video.py."""
import importlib.util
import io
import os

import pytest
import torch

import util_yuv as U

from util_yuv import GOLDEN, golden_conditions, golden_yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_definition_reproduces_the_reference_on_the_golden_fixture():
    g = torch.load(GOLDEN)
    rgb, yc, mask = g['rgb'], g['ycbcr'], g['mask']
    n, H, W, _ = rgb.shape
    assert (n, H, W) == (2, 48, 64) and os.path.getsize(GOLDEN) < 100_000
    for a in (1, 2):  # the fixture's premise: every 2 x 2 block of the reference's planes is constant
        assert torch.equal(yc[:, ::2, ::2, a], yc[:, 1::2, ::2, a]) and torch.equal(yc[:, ::2, ::2, a], yc[:, ::2, 1::2, a])
    assert float(mask.float().mean()) >= 0.95
    for src in (rgb, rgb.permute(0, 3, 1, 2).float() / 255.0):  # bytes, and the floats a network would hand over
        enc = U.encode_def(src, 'bt601', 'limited')
        hw, q = H * W, (H // 2) * (W // 2)
        golden_conditions(enc[:, :hw].reshape(n, H, W), yc[..., 0], 'Y')
        golden_conditions(enc[:, hw:hw + q].reshape(n, H // 2, W // 2), yc[:, ::2, ::2, 1], 'Cb per block')
        golden_conditions(enc[:, hw + q:].reshape(n, H // 2, W // 2), yc[:, ::2, ::2, 2], 'Cr per block')
    dec = U.decode_def(golden_yuv(g), H, W, 'bt601', 'limited', 'nearest', torch.uint8)
    golden_conditions(dec[mask], g['back'][mask], 'decode (in gamut)')
    as_float = U.decode_def(golden_yuv(g), H, W, 'bt601', 'limited', 'nearest', torch.float32)
    assert torch.equal(torch.round(as_float * 255.0).to(torch.uint8).permute(0, 2, 3, 1), dec)


def test_coefficients():
    from edvr_amd import ops
    for matrix in U.MATRICES:
        for rng in U.RANGES:
            m, mi, off = U.coeffs64(matrix, rng)
            pm, pmi, poff = ops.yuv_coeffs(matrix, rng)
            assert torch.equal(torch.tensor(pm, dtype=torch.float64), m) and torch.equal(torch.tensor(pmi, dtype=torch.float64), mi)
            assert poff == off.tolist()
            assert (torch.linalg.inv(m) - mi).abs().max() < 1e-14 and (m @ mi - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-14
            # grey stays grey, and the rows are what the standards print
            assert (m[1:].sum(1)).abs().max() < 1e-15 and abs(float(m[0].sum()) - U.RANGES[rng][0] / 255.0) < 1e-15
    m = U.coeffs64('bt601', 'limited')[0] * 255.0
    assert (m[0] - torch.tensor([65.481, 128.553, 24.966], dtype=torch.float64)).abs().max() < 1e-9 and abs(float(m[1, 2]) - 112.0) < 1e-9
    with pytest.raises(ValueError):
        ops.yuv_coeffs('bt2020', 'limited')
    with pytest.raises(ValueError):
        ops.yuv_coeffs('bt601', 'tv')
    assert ops.yuv420_frame_size(3, 5) == 15 + 2 * 6 == U.frame_size(3, 5)


def test_definition_edges():
    """Odd sizes: the chroma planes are ceil(size / 2), an odd edge replicates in the encode, indices clamp in the decode."""
    rgb = torch.randint(0, 256, (1, 3, 5, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    enc = U.encode_def(rgb, 'bt709', 'full')
    assert enc.shape == (1, U.frame_size(3, 5))
    padded = torch.cat([rgb, rgb[:, -1:]], 1)
    padded = torch.cat([padded, padded[:, :, -1:]], 2)  # (1, 4, 6, 3): the replicated edge spelled out
    want = U.encode_def(padded, 'bt709', 'full')
    y, cb, cr = U.split_planes(want, 4, 6)
    assert torch.equal(enc[:, 15:], torch.cat([cb.reshape(1, -1), cr.reshape(1, -1)], 1).to(torch.uint8))
    assert torch.equal(enc[:, :15].reshape(1, 3, 5), y[:, :3, :5].to(torch.uint8))
    flat = torch.full((1, U.frame_size(3, 5)), 77, dtype=torch.uint8)  # constant planes stay constant under both filters
    for chroma in ('nearest', 'bilinear'):
        out = U.decode_def(flat, 3, 5, 'bt601', 'limited', chroma)
        assert out.shape == (1, 3, 3, 5) and all(float(out[0, k].min()) == float(out[0, k].max()) for k in range(3))
    nan = torch.full((1, 3, 2, 2), float('nan'))
    assert torch.equal(U.encode_def(nan, 'bt601', 'limited'), U.encode_def(torch.zeros(1, 3, 2, 2), 'bt601', 'limited'))


# ---------------------------------------------------------------------------------------------------------------- YUV4MPEG2
def _frames(n, H, W, seed=0):
    return torch.randint(0, 256, (n, U.frame_size(H, W)), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _reader(data):
    from edvr_amd.y4m import Y4MReader
    return Y4MReader(io.BytesIO(data))


@pytest.mark.parametrize('tags, expect', [
    ('F30000:1001 Ip A1:1 C420jpeg', dict(fps='30000:1001', aspect='1:1', chroma='420jpeg', range='limited')),
    ('F25:1 I? C420mpeg2 XYSCSS=420MPEG2', dict(fps='25:1', aspect=None, chroma='420mpeg2', range='limited')),
    ('F25:1 C420paldv XCOLORRANGE=FULL', dict(chroma='420paldv', range='full')),
    ('F50:1 Ip A128:117 C420 XCOLORRANGE=LIMITED', dict(aspect='128:117', chroma='420', range='limited')),
    ('', dict(fps=None, aspect=None, chroma=None, range='limited')),
])
def test_reader_accepts(tags, expect):
    frames = _frames(2, 6, 10)
    r = _reader(U.y4m_bytes(frames, 6, 10, tags))
    assert (r.width, r.height, r.framesize) == (10, 6, U.frame_size(6, 10))
    for k, v in expect.items():
        assert getattr(r, k) == v, k
    buf = r.read(2)
    assert torch.equal(buf[:, 6:], frames) and bytes(buf[1, :6].tolist()) == b'FRAME\n'


@pytest.mark.parametrize('data', [
    b'YUV4MPEG W10 H6 F25:1 Ip C420jpeg\n', b'RIFF....AVI \n', b'', b'YUV4MPEG2 W10 H6 F25:1',  # magic; a header without its newline
    b'YUV4MPEG2 W10 H6 F25:1 It C420jpeg\n', b'YUV4MPEG2 W10 H6 F25:1 Ib\n', b'YUV4MPEG2 W10 H6 F25:1 Im C420\n',
    b'YUV4MPEG2 W10 H6 F25:1 Ip C422\n', b'YUV4MPEG2 W10 H6 F25:1 Ip C444\n', b'YUV4MPEG2 W10 H6 F25:1 Ip Cmono\n', b'YUV4MPEG2 W10 H6 C411\n',
    b'YUV4MPEG2 W10 H6 F25:1 Ip C420p10\n', b'YUV4MPEG2 W10 H6 Ip C420p12\n', b'YUV4MPEG2 W10 H6 Ip C420p16\n', b'YUV4MPEG2 W10 H6 C444p10\n',
    b'YUV4MPEG2 H6 F25:1\n', b'YUV4MPEG2 W0 H6\n', b'YUV4MPEG2 W10 Hsix\n', b'YUV4MPEG2 W10 H6 XCOLORRANGE=WIDE\n',
])
def test_reader_rejects(data):
    with pytest.raises(ValueError):
        _reader(data)


def test_reader_on_a_pipe_across_the_end_and_frame_parameters():
    """A non-seekable stream that returns short reads; read(k) past the end returns what is left, then nothing."""
    from edvr_amd.y4m import Y4MReader
    frames = _frames(5, 7, 9, seed=3)
    data = U.y4m_bytes(frames, 7, 9, 'F24:1 Ip C420jpeg', frame_params=b' Ip XFOO=1')
    rd, wr = os.pipe()
    assert len(data) < 4096  # fits the pipe's buffer: no second thread is needed to feed it
    os.write(wr, data)
    os.close(wr)
    with os.fdopen(rd, 'rb', buffering=0) as stream:
        assert not stream.seekable()
        r = Y4MReader(stream)
        a, b, c = r.read(3), r.read(3), r.read(3)
    assert a.shape == (3, 6 + r.framesize) and b.shape == (2, 6 + r.framesize) and c.shape == (0, 6 + r.framesize)
    assert torch.equal(torch.cat([a, b])[:, 6:], frames) and r.frames_read == 5
    assert all(bytes(row[:6].tolist()) == b'FRAME\n' for row in torch.cat([a, b]))  # the parameters are dropped
    assert a.is_contiguous() and a.stride() == (6 + r.framesize, 1)


def test_reader_names_the_truncated_frame():
    frames = _frames(4, 6, 10, seed=4)
    data = U.y4m_bytes(frames, 6, 10)
    r = _reader(data[:-5])
    assert r.read(2).shape[0] == 2
    with pytest.raises(ValueError, match=r'frame 3 is truncated'):
        r.read(2)
    r = _reader(data[:-U.frame_size(6, 10)] + b'\n')  # the FRAME line alone
    r.read(3)
    with pytest.raises(ValueError, match=r'frame 3 is truncated: 1 of'):
        r.read(1)
    with pytest.raises(ValueError, match=r'frame 1: expected a FRAME line'):
        _reader(data[:data.index(b'FRAME') + 6 + U.frame_size(6, 10)] + b'JUNK\n').read(2)


@pytest.mark.parametrize('H, W', [(6, 10), (7, 9), (1, 1), (5, 8)])
@pytest.mark.parametrize('rng', ['limited', 'full'])
def test_writer_then_reader_is_the_identity(H, W, rng):
    from edvr_amd.y4m import Y4MReader, Y4MWriter
    frames = _frames(3, H, W, seed=H * W)
    src = U.y4m_bytes(frames, H, W, 'F30:1 Ip A1:1 C420jpeg' + (' XCOLORRANGE=FULL' if rng == 'full' else ''))
    r = Y4MReader(io.BytesIO(src))
    out = io.BytesIO()
    w = Y4MWriter(out, r.width, r.height, r.fps, r.aspect, r.range)
    w.write(r.read(2))
    w.write(r.read(2))
    w.write(r.read(2))  # empty
    assert out.getvalue() == src and w.frames_written == 3
    with pytest.raises(ValueError):
        w.write(torch.zeros(1, 6 + w.framesize, dtype=torch.uint8))  # no FRAME line
    with pytest.raises(ValueError):
        w.write(torch.zeros(1, 5 + w.framesize, dtype=torch.uint8))
    with pytest.raises(ValueError):
        Y4MWriter(io.BytesIO(), 4, 4, range='tv')


class _Nearest4:
    """Stands in for VideoRestorer on the CPU: 'restores' by x4 replication, chunk by chunk."""
    made = []

    def __init__(self, net, out_dtype=None, **kwargs):
        assert out_dtype == torch.float32
        self.scale, self.kwargs = 4, kwargs
        _Nearest4.made.append(self)

    def restore_chunks(self, frames, length=None):
        for piece in frames:
            yield piece.repeat_interleave(4, 2).repeat_interleave(4, 3)


@pytest.mark.parametrize('H, W, tags, m_in, m_out', [
    (8, 12, 'F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL', 'bt601', 'bt601'),
    (180, 320, 'F25:1 Ip A1:1 C420mpeg2', 'bt601', 'bt709'),       # the 720p result is read as 709
    (148, 12, 'F24:1 C420', 'bt601', 'bt709'),                     # 592 rows
    (8, 1280, 'F24:1 C420', 'bt709', 'bt709'),
])
def test_restore_y4m_flow_header_and_default_matrices(monkeypatch, H, W, tags, m_in, m_out):
    """restore_y4m with CPU stand-ins for the three device pieces (the definition for the two conversions): the output header carries
    (4 W, 4 H), the input's F / A and range; the payload is the composition done by hand with the size rule's matrices."""
    from edvr_amd import ops, video, y4m
    monkeypatch.setattr(ops, 'yuv420_to_rgb', lambda yuv, h, w, matrix, rng, chroma: U.decode_def(yuv, h, w, matrix, rng, chroma))
    monkeypatch.setattr(ops, 'rgb_to_yuv420', lambda rgb, matrix, rng, out: out.copy_(U.encode_def(rgb, matrix, rng)))
    monkeypatch.setattr(video, 'VideoRestorer', _Nearest4)
    assert (y4m.default_matrix(H, W), y4m.default_matrix(4 * H, 4 * W)) == (m_in, m_out)
    assert [y4m.default_matrix(*s) for s in ((576, 1279), (577, 8), (720, 1280), (480, 720))] == ['bt601', 'bt709', 'bt709', 'bt601']
    net = torch.nn.Linear(1, 1)
    frames = _frames(3, H, W, seed=9)
    rng = 'full' if 'FULL' in tags else 'limited'
    out = io.BytesIO()
    assert y4m.restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, tags)), out, read_frames=2, chunk=3, pad_mode='reflect') == 3
    assert _Nearest4.made[-1].kwargs == dict(chunk=3, pad_mode='reflect')
    r = y4m.Y4MReader(io.BytesIO(out.getvalue()))
    src = y4m.Y4MReader(io.BytesIO(U.y4m_bytes(frames, H, W, tags)))
    assert (r.width, r.height, r.fps, r.aspect, r.range) == (4 * W, 4 * H, src.fps, src.aspect, rng)
    assert out.getvalue().split(b'\n')[0].split()[1:3] == [f'W{4 * W}'.encode(), f'H{4 * H}'.encode()] and b' Ip ' in out.getvalue()[:80]
    rgb = U.decode_def(frames, H, W, m_in, rng, 'bilinear').repeat_interleave(4, 2).repeat_interleave(4, 3)
    assert torch.equal(r.read(4)[:, 6:], U.encode_def(rgb, m_out, rng))
    with pytest.raises(ValueError):
        y4m.restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, tags)), io.BytesIO(), matrix_in='bt2020')
    with pytest.raises(ValueError):
        y4m.restore_y4m(net, io.BytesIO(U.y4m_bytes(frames, H, W, tags)), io.BytesIO(), chroma='bicubic')


def test_ops_refuse_the_cpu():
    from edvr_amd import ops
    with pytest.raises(NotImplementedError):
        ops.yuv420_to_rgb(_frames(1, 4, 4), 4, 4)
    with pytest.raises(NotImplementedError):
        ops.rgb_to_yuv420(torch.zeros(1, 3, 4, 4))


# ---------------------------------------------------------------------------------------------------------------- the script
def _script():
    spec = importlib.util.spec_from_file_location('restore_video', os.path.join(ROOT, 'scripts', 'restore_video.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restore_video_command_line(capsys):
    mod = _script()
    with pytest.raises(SystemExit) as e:
        mod.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--weights', '--num-feat', '--hr-in', '--with-predeblur', '--no-tsa', '--padding', '--batch', '--pad-mode', '--tile', '--tile-overlap',
                '--tile-blend', '--self-ensemble', '--time-reverse', '--matrix-in', '--matrix-out', '--chroma'):
        assert opt in text, opt
    args = mod.parse_args(['-', '-', '--tile', '64', '64', '--self-ensemble', 'flip4', '--matrix-out', 'bt709'])
    assert (args.input, args.output, args.tile, args.self_ensemble, args.matrix_in, args.matrix_out, args.chroma, args.batch) == \
        ('-', '-', [64, 64], 'flip4', None, 'bt709', 'bilinear', 8)
    for bad in (['in.y4m'], ['-', '-', '--tile-blend', '8'], ['-', '-', '--tile-overlap', '8'], ['-', '-', '--matrix-in', 'bt2020'],
                ['-', '-', '--chroma', 'bicubic'], ['-', '-', '--batch', '0'], ['a.y4m', 'a.y4m'], ['-', '-', '--self-ensemble', 'd8']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
