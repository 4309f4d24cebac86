"""CPU: chroma siting - the definition in tests/util_yuv_siting.py against the unsited one and against what a siting
means (a ramp lands where the full-resolution ramp is), the BT.2020 matrix, and the container's tags.  No GPU."""
import io
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_yuv_formats as F  # noqa: E402
import util_yuv_siting as S  # noqa: E402

FORMATS = ['420', '422', '444', '420p10', '422p16', '444p12', '420p9']


def _frame(fmt, y, cb, cr):
    """Planes (n, h, w) of integers -> (n, framesize) uint8."""
    n = y.shape[0]
    return F.to_bytes(torch.cat([t.reshape(n, -1) for t in (y, cb, cr)], 1), F.parse(fmt)[2])


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('H, W', [(1, 1), (5, 7), (6, 10)])
def test_center_is_the_unsited_definition(fmt, H, W):
    yuv = F.random_frames(2, H, W, fmt, seed=H * W, above=2)
    for chroma in ('bilinear', 'nearest'):
        assert torch.equal(S.decode_def(yuv, H, W, fmt, 'bt709', 'limited', chroma, 'center'), F.decode_def(yuv, H, W, fmt, 'bt709', 'limited', chroma))
    rgb = S.hostile_rgb(2, H, W, seed=H + W)
    for rng in ('limited', 'full'):
        assert torch.equal(S.encode_def(rgb, fmt, 'bt601', rng, 'center'), F.encode_def(rgb, fmt, 'bt601', rng))


def test_center_is_the_8_bit_420_definition_for_bytes():
    import util_yuv as U
    H, W = 5, 7
    yuv = F.random_frames(2, H, W, '420', seed=3)
    assert torch.equal(S.decode_def(yuv, H, W, '420', out_dtype=torch.uint8), U.decode_def(yuv, H, W, out_dtype=torch.uint8))
    rgb8 = torch.randint(0, 256, (2, H, W, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    assert torch.equal(S.encode_def(rgb8, '420'), U.encode_def(rgb8))


@pytest.mark.parametrize('fmt', ['444', '444p10'])
def test_444_has_no_siting(fmt):
    H, W = 5, 6
    yuv, rgb = F.random_frames(1, H, W, fmt, seed=1), S.hostile_rgb(1, H, W, seed=2)
    for siting in ('left', 'topleft'):
        assert torch.equal(S.decode_def(yuv, H, W, fmt, siting=siting), F.decode_def(yuv, H, W, fmt))
        assert torch.equal(S.encode_def(rgb, fmt, siting=siting), F.encode_def(rgb, fmt))


def test_topleft_on_422_is_left_and_nearest_ignores_siting():
    H, W = 5, 9
    yuv, rgb = F.random_frames(1, H, W, '422p10', seed=1), S.hostile_rgb(1, H, W, seed=2)
    assert torch.equal(S.decode_def(yuv, H, W, '422p10', siting='topleft'), S.decode_def(yuv, H, W, '422p10', siting='left'))
    assert torch.equal(S.encode_def(rgb, '422p10', siting='topleft'), S.encode_def(rgb, '422p10', siting='left'))
    assert not torch.equal(S.decode_def(yuv, H, W, '422p10', siting='left'), S.decode_def(yuv, H, W, '422p10', siting='center'))
    y420 = F.random_frames(1, H, W, '420', seed=3)
    for siting in ('left', 'topleft'):
        assert torch.equal(S.decode_def(y420, H, W, '420', chroma='nearest', siting=siting), F.decode_def(y420, H, W, '420', chroma='nearest'))


def test_a_left_sited_ramp_decodes_onto_the_full_resolution_ramp():
    """c[k] = 16 + 4 k co-sited with luma column 2 k IS the plane C[x] = 16 + 2 x at the even columns, and its linear interpolation at the
    odd ones: decoded as 'left', 4:2:2 equals the 4:4:4 decode up to column 2 (Wc - 1) (past it, the clamp replicates).  As 'center' the
    same samples land half a luma column to the right."""
    H, W = 3, 24
    wc = W // 2
    y = torch.randint(16, 236, (1, H, W), generator=torch.Generator().manual_seed(0))
    ramp2 = (16 + 4 * torch.arange(wc)).expand(1, H, wc)
    ramp4 = (16 + 2 * torch.arange(W)).expand(1, H, W)
    full = F.decode_def(_frame('444', y, ramp4, ramp4.flip(2)), H, W, '444')
    sub = _frame('422', y, ramp2, (16 + 2 * (W - 1) - 4 * torch.arange(wc)).expand(1, H, wc))
    upto = 2 * (wc - 1) + 1
    assert torch.equal(S.decode_def(sub, H, W, '422', siting='left')[..., :upto], full[..., :upto])
    assert not torch.equal(S.decode_def(sub, H, W, '422', siting='center')[..., :upto], full[..., :upto])


def test_a_topleft_sited_ramp_decodes_onto_the_full_resolution_ramp_vertically():
    H, W = 24, 6
    hc, wc = H // 2, W // 2
    y = torch.randint(16, 236, (1, H, W), generator=torch.Generator().manual_seed(1))
    ramp2 = (16 + 4 * torch.arange(hc)).view(1, hc, 1).expand(1, hc, wc)
    ramp4 = (16 + 2 * torch.arange(H)).view(1, H, 1).expand(1, H, W)
    full = F.decode_def(_frame('444', y, ramp4, ramp4), H, W, '444')
    sub = _frame('420', y, ramp2, ramp2)
    upto = 2 * (hc - 1) + 1
    assert torch.equal(S.decode_def(sub, H, W, '420', siting='topleft')[:, :, :upto], full[:, :, :upto])
    for other in ('center', 'left'):  # both centre the rows
        assert not torch.equal(S.decode_def(sub, H, W, '420', siting=other)[:, :, :upto], full[:, :, :upto])


def test_a_linear_frame_encodes_onto_its_own_even_columns():
    """R, G, B linear in x: the values p before quantisation are linear in x, so [1 2 1] / 4 around column 2 l gives p[2 l] - the 'left'
    chroma is the 4:4:4 chroma at the even columns, up to one code of rounding - and the mean of columns 2 l and 2 l + 1 gives p at
    2 l + 1/2, half the slope per column further."""
    H, W, fmt = 4, 32, '422p10'
    x = torch.arange(W, dtype=torch.float32)
    slopes = torch.tensor([0.02, -0.01, 0.025], dtype=torch.float64)
    rgb = torch.stack([0.1 + 0.02 * x, 0.5 - 0.01 * x, 0.1 + 0.025 * x]).view(1, 3, 1, W).expand(1, 3, H, W).contiguous()
    assert 0.0 < float(rgb.min()) and float(rgb.max()) < 1.0
    m = F.coeffs64('bt601', 'limited', 10)[0]
    half = (m @ slopes * 255.0)[1:] / 2.0  # (Cb, Cr) codes per half column
    assert float(half.abs().min()) > 3.0
    wc = W // 2
    full = F.to_samples(S.encode_def(rgb, '444p10'), 10)[0, H * W:].reshape(2, H, W)[:, :, ::2]
    left = F.to_samples(S.encode_def(rgb, fmt, siting='left'), 10)[0, H * W:].reshape(2, H, wc)
    centre = F.to_samples(S.encode_def(rgb, fmt, siting='center'), 10)[0, H * W:].reshape(2, H, wc)
    inner = slice(1, wc - 1)
    assert int((left - full)[:, :, inner].abs().max()) <= 1
    off = (centre - full)[:, :, inner].double() - half.view(2, 1, 1)
    assert float(off.abs().max()) <= 1.0
    assert int((centre - full)[:, :, inner].abs().min()) >= 2


def test_a_frame_linear_in_y_encodes_topleft_onto_its_own_even_rows():
    H, W, fmt = 32, 4, '420p10'
    yy = torch.arange(H, dtype=torch.float32)
    rgb = torch.stack([0.1 + 0.02 * yy, 0.5 - 0.01 * yy, 0.1 + 0.025 * yy]).view(1, 3, H, 1).expand(1, 3, H, W).contiguous()
    hc, wc = H // 2, W // 2
    full = F.to_samples(S.encode_def(rgb, '444p10'), 10)[0, H * W:].reshape(2, H, W)[:, ::2, ::2]
    top = F.to_samples(S.encode_def(rgb, fmt, siting='topleft'), 10)[0, H * W:].reshape(2, hc, wc)
    left = F.to_samples(S.encode_def(rgb, fmt, siting='left'), 10)[0, H * W:].reshape(2, hc, wc)
    assert int((top - full)[:, 1:hc - 1].abs().max()) <= 1
    assert int((left - full)[:, 1:hc - 1].abs().min()) >= 2  # 'left' centres the rows


# ---------------------------------------------------------------------------------------------------------------- BT.2020
def test_bt2020_matrix():
    from edvr_amd import ops
    kr, kb = ops.YUV_MATRICES['bt2020nc']
    assert (kr, kb) == (0.2627, 0.0593)
    kg = 1.0 - kr - kb
    for rng, depth in (('limited', 10), ('limited', 8), ('full', 12)):
        m, mi, off = ops.yuv_coeffs('bt2020nc', rng, depth)
        k = 2.0 ** (depth - 8)
        ys, cs = (219.0 * k, 224.0 * k) if rng == 'limited' else (2.0 ** depth - 1,) * 2
        want = torch.tensor([[kr, kg, kb], [-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5], [0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))]],
                            dtype=torch.float64) * torch.tensor([[ys], [cs], [cs]], dtype=torch.float64) / 255.0
        got, inv = torch.tensor(m, dtype=torch.float64), torch.tensor(mi, dtype=torch.float64)
        assert float((got - want).abs().max()) < 1e-12
        assert float((got @ inv - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-13
        assert off == ([16.0 * k, 128.0 * k, 128.0 * k] if rng == 'limited' else [0.0, 2.0 ** (depth - 1), 2.0 ** (depth - 1)])
    m, _, off = ops.yuv_coeffs('bt2020nc', 'limited', 10)
    m, off = torch.tensor(m, dtype=torch.float64), torch.tensor(off, dtype=torch.float64)

    def code(r, g, b):
        return torch.round(m @ torch.tensor([r, g, b], dtype=torch.float64) * 255.0 + off).to(torch.int64).tolist()

    assert code(1, 1, 1) == [940, 512, 512] and code(0, 0, 0) == [64, 512, 512]
    for rgb, K in (((1, 0, 0), kr), ((0, 1, 0), kg), ((0, 0, 1), kb)):
        assert code(*rgb)[0] == round(876 * K) + 64
    assert code(0, 0, 1)[1] == 960 and code(1, 0, 0)[2] == 960  # the primaries reach the chroma extremes
    with pytest.raises(ValueError):
        ops.yuv_coeffs('bt2020c', 'limited', 10)  # constant luminance is another system, not a matrix


# ---------------------------------------------------------------------------------------------------------------- the container
TAGS = [('C420jpeg', 'center'), ('C420mpeg2', 'left'), ('C420paldv', 'topleft'), ('C420', None), ('', None), ('C422', None), ('C444', None)] + \
    [(f'C{b}p{d}', None) for b in ('420', '422', '444') for d in range(9, 17)]


@pytest.mark.parametrize('tag, siting', TAGS)
def test_reader_reports_the_siting_of_the_tag(tag, siting):
    from edvr_amd import y4m
    r = y4m.Y4MReader(io.BytesIO(f'YUV4MPEG2 W10 H6 F25:1 Ip {tag}\n'.encode()), formats=y4m.ALL_FORMATS)
    assert r.siting == siting
    assert y4m.resolve_siting('auto', r) == (siting or 'left')
    for name in ('center', 'left', 'topleft'):
        assert y4m.resolve_siting(name, r) == name
    if tag in ('C420jpeg', 'C420mpeg2', 'C420paldv', 'C420', ''):  # what the reader takes without `formats`
        assert y4m.Y4MReader(io.BytesIO(f'YUV4MPEG2 W10 H6 {tag}\n'.encode())).siting == siting


def test_writer_tags_round_trip_and_bad_names_raise():
    from edvr_amd import ops, y4m
    assert ops.YUV_SITINGS == {'center': (0, 0), 'left': (1, 0), 'topleft': (1, 1)}
    for siting, tag in (('center', b'C420jpeg'), ('left', b'C420mpeg2'), ('topleft', b'C420paldv')):
        out = io.BytesIO()
        w = y4m.Y4MWriter(out, 10, 6, '25:1', None, 'limited', '420', siting)
        assert w.siting == siting and tag in out.getvalue().split()
        assert y4m.Y4MReader(io.BytesIO(out.getvalue())).siting == siting
        other = io.BytesIO()
        y4m.Y4MWriter(other, 10, 6, format='422p10', siting=siting)  # a tag that cannot carry it
        assert other.getvalue() == b'YUV4MPEG2 W10 H6 Ip C422p10\n'
    out = io.BytesIO()
    y4m.Y4MWriter(out, 10, 6)
    assert b'C420jpeg' in out.getvalue()
    r = y4m.Y4MReader(io.BytesIO(b'YUV4MPEG2 W10 H6 C420\n'))
    for bad in ('centre', 'top', 'AUTO', None, 1):
        with pytest.raises(ValueError):
            y4m.Y4MWriter(io.BytesIO(), 10, 6, siting=bad)
        with pytest.raises(ValueError):
            y4m.resolve_siting(bad, r)
        with pytest.raises(ValueError):
            ops.yuv_to_rgb(torch.zeros(1, 90, dtype=torch.uint8), 6, 10, '420', siting=bad)
        with pytest.raises(ValueError):
            ops.yuv420_to_rgb(torch.zeros(1, 90, dtype=torch.uint8), 6, 10, siting=bad)
        with pytest.raises(ValueError):
            ops.rgb_to_yuv(torch.zeros(1, 3, 6, 10), '422', siting=bad)
        with pytest.raises(ValueError):
            ops.rgb_to_yuv420(torch.zeros(1, 3, 6, 10), siting=bad)
    with pytest.raises(ValueError):
        y4m.Y4MWriter(io.BytesIO(), 10, 6, siting='auto')  # a writer has no tag to follow
    with pytest.raises(ValueError):
        y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(b'YUV4MPEG2 W8 H8 C420\n'), io.BytesIO(), siting_in='middle')
    with pytest.raises(ValueError):
        y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(b'YUV4MPEG2 W8 H8 C420\n'), io.BytesIO(), siting_out='middle')


class _Nearest4:
    """Stands in for VideoRestorer on the CPU: 'restores' by x4 replication, chunk by chunk."""

    def __init__(self, net, out_dtype=None, **kwargs):
        self.scale = 4

    def restore_chunks(self, frames, length=None):
        for piece in frames:
            yield piece.repeat_interleave(4, 2).repeat_interleave(4, 3)


@pytest.mark.parametrize('tag, fmt, kwargs, s_in, s_out, out_tag', [
    ('C420mpeg2', '420', dict(siting_in='auto'), 'left', 'left', 'C420mpeg2'),
    ('C420paldv', '420', dict(siting_in='auto', siting_out='left'), 'topleft', 'left', 'C420mpeg2'),
    ('C420', '420', dict(siting_in='auto', siting_out='center'), 'left', 'center', 'C420jpeg'),
    ('C420jpeg', '420', dict(siting_in='auto', siting_out='topleft'), 'center', 'topleft', 'C420paldv'),
    ('C422p10', '422p10', dict(siting_in='auto'), 'left', 'left', 'C422p10'),
    ('C420p10', '420p10', dict(siting_in='topleft', siting_out='auto'), 'topleft', 'left', 'C420p10'),
    ('C420mpeg2', '420', dict(), 'center', 'center', 'C420jpeg'),
])
def test_restore_y4m_flow_sitings(monkeypatch, tag, fmt, kwargs, s_in, s_out, out_tag):
    """restore_y4m with CPU stand-ins for the device pieces (the definition for the conversions): the sitings reach the conversions as
    resolved, the output's tag carries the output's siting, and at (center, center) no `siting` keyword is passed at all."""
    from edvr_amd import ops, video, y4m
    seen = []

    def to_rgb420(yuv, h, w, matrix, rng, chroma, **kw):
        seen.append(('in', kw))
        return S.decode_def(yuv, h, w, '420', matrix, rng, chroma, **kw)

    def to_rgb(yuv, h, w, f, matrix, rng, chroma, **kw):
        seen.append(('in', kw))
        return S.decode_def(yuv, h, w, f, matrix, rng, chroma, **kw)

    def to_yuv420(rgb, matrix, rng, out, **kw):
        seen.append(('out', kw))
        return out.copy_(S.encode_def(rgb, '420', matrix, rng, **kw))

    def to_yuv(rgb, f, matrix, rng, out, **kw):
        seen.append(('out', kw))
        return out.copy_(S.encode_def(rgb, f, matrix, rng, **kw))

    monkeypatch.setattr(ops, 'yuv420_to_rgb', to_rgb420)
    monkeypatch.setattr(ops, 'yuv_to_rgb', to_rgb)
    monkeypatch.setattr(ops, 'rgb_to_yuv420', to_yuv420)
    monkeypatch.setattr(ops, 'rgb_to_yuv', to_yuv)
    monkeypatch.setattr(video, 'VideoRestorer', _Nearest4)
    H, W = 6, 10
    frames = F.random_frames(3, H, W, fmt, seed=5)
    out = io.BytesIO()
    assert y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(F.y4m_bytes(frames, H, W, f'F25:1 Ip {tag}')), out, read_frames=2, **kwargs) == 3
    assert out_tag in out.getvalue().split(b'\n')[0].decode().split()
    assert {tuple(kw.items()) for side, kw in seen if side == 'in'} == {(('siting', s_in),) if s_in != 'center' else ()}
    assert {tuple(kw.items()) for side, kw in seen if side == 'out'} == {(('siting', s_out),) if s_out != 'center' else ()}
    rgb = S.decode_def(frames, H, W, fmt, 'bt601', 'limited', 'bilinear', s_in).repeat_interleave(4, 2).repeat_interleave(4, 3)
    r = y4m.Y4MReader(io.BytesIO(out.getvalue()), formats=y4m.ALL_FORMATS)
    assert torch.equal(r.read(4)[:, 6:], S.encode_def(rgb, fmt, 'bt601', 'limited', s_out))


def test_restore_video_siting_options(capsys):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('restore_video', os.path.join(root, 'scripts', 'restore_video.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(['-', '-'])
    assert (args.siting, args.siting_out) == ('center', None)
    args = mod.parse_args(['-', '-', '--siting', 'auto', '--siting-out', 'topleft', '--matrix-in', 'bt2020nc', '--matrix-out', 'bt2020nc'])
    assert (args.siting, args.siting_out, args.matrix_in, args.matrix_out) == ('auto', 'topleft', 'bt2020nc', 'bt2020nc')
    for bad in (['-', '-', '--siting', 'centre'], ['-', '-', '--siting-out', 'top']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2
    capsys.readouterr()
