"""CPU: the delivery resampling of DESIGN 4.21 - the host tables of edvr_amd/resample.py (R1 - R5), the NumPy restatement
(tests/resample_ref.py) against stock F.interpolate(bicubic, antialias=True) where no tap leaves the frame, y4m.fit_size, the flow of
restore_y4m with CPU stand-ins for the device pieces (ops.resample stood in by the restatement), and the flags of restore_video.py."""
import importlib.util
import io
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import resample_ref as R
import util_yuv as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['lanczos3', 'bicubic', 'bilinear']
# (H, W) -> (Ho, Wo): the shapes the definition was checked on
SHAPES = [((48, 72), (27, 48)), ((40, 40), (90, 64)), ((64, 96), (8, 12)), ((33, 47), (33, 20)), ((5, 7), (17, 23)), ((6, 9), (48, 72))]


# ---------------------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('I, O', [(72, 48), (48, 27), (40, 90), (96, 12), (47, 20), (7, 23), (9, 72), (5, 3), (1920, 1080), (7, 7), (1, 8), (8, 1)])
def test_axis_table_by_R1_to_R5(I, O, kernel):
    from edvr_amd.resample import KERNELS as RADII, axis_table, taps
    first, w = axis_table(I, O, kernel)
    a, f = RADII[kernel], max(Fraction(1), Fraction(I, O))
    T = 1 if I == O else -((-2 * a * f.numerator) // f.denominator) + 1  # R3: ceil(2 a f) + 1; R5
    assert T == taps(I, O, kernel) <= 49
    assert first.dtype == np.int32 and first.shape == (O,) and w.dtype == np.float32 and w.shape == (O, T)
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= T * 2.0 ** -24
    if I == O:
        assert np.array_equal(first, np.arange(O)) and np.array_equal(w, np.ones((O, 1), np.float32))
    else:  # R2, R3: first_j - 1 = floor(u_j - a f), against the exact centre (float64 may sit on either side of an integer u_j - a f:
        # the tap that then enters or leaves has weight K(+-a) = 0)
        eps = Fraction(1, 10 ** 9)
        for j in range(O):
            lo = Fraction((2 * j + 1) * I - O, 2 * O) - a * f
            assert lo - 1 - eps < int(first[j]) - 1 <= lo + eps
    # the restatement forms the same tables on its own
    rf, rw = R.table(I, O, kernel)
    assert np.array_equal(rf, first) and np.array_equal(rw, w)


def test_axis_table_extremes_and_errors():
    from edvr_amd.resample import axis_table, taps
    assert axis_table(96, 12, 'lanczos3')[1].shape == (12, 49)  # the ratio 8
    assert taps(12, 96, 'lanczos3') == 7 and taps(96, 12, 'bicubic') == 33 and taps(96, 12, 'bilinear') == 17
    first, w = axis_table(5, 17, 'lanczos3')
    assert first.min() < 0 and (first + w.shape[1] - 1).max() > 4  # R4 is the kernel's: the tables are not clamped
    for I, O in ((97, 12), (12, 97), (0, 4), (4, 0), (-3, 3)):
        with pytest.raises(ValueError):
            axis_table(I, O, 'lanczos3')
    with pytest.raises(ValueError):
        axis_table(8, 4, 'lanczos2')


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _frames(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


@pytest.mark.parametrize('src, dst', SHAPES + [((5, 7), (3, 4))])
def test_restatement_agrees_with_stock_antialiased_bicubic_inside_the_frame(src, dst):
    """On every output sample whose taps all lie inside the frame on both axes (read from the tables) R1 - R7 with 'bicubic' are what
    F.interpolate(mode='bicubic', antialias=True, align_corners=False) computes; at the edges they differ by design - the stock op
    renormalises truncated rows, R4 repeats the edge sample.  Bound 1e-5 on values in [0, 1]: the stock op accumulates in float32."""
    x = _frames((2, 3) + src, seed=src[0] * dst[1])
    mask = np.outer(R.interior(src[0], dst[0], 'bicubic'), R.interior(src[1], dst[1], 'bicubic'))
    if (src, dst) == ((5, 7), (3, 4)):
        assert not mask.any()  # eight taps on five rows: nothing to compare, and the test says so
        return
    assert mask.any(), 'no interior sample: the comparison would be empty'
    ours = R.resample(x, dst, 'bicubic')
    stock = torch.nn.functional.interpolate(torch.from_numpy(x), size=dst, mode='bicubic', antialias=True, align_corners=False).numpy()
    assert ours.shape == stock.shape == (2, 3) + dst
    diff = np.abs(ours - stock)[:, :, mask].max()
    print(f'{src} -> {dst}: {int(mask.sum())} interior samples, max |ours - stock| = {diff:.3g}')
    assert diff <= 1e-5


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('src, dst', SHAPES)
def test_restatement_keeps_a_constant_frame_and_an_identity_axis(src, dst, kernel):
    """A flat frame stays flat to the rounding of the weights: a row of T float32 weights sums to 1 within T 2^-24 (R3 rounds each weight
    after the division), a pass adds half an ulp of its result - so |out - v| <= v (Tx + Ty) 2^-24 + 2^-24 for 0 <= v <= 1; 0 is exact."""
    Ty, Tx = R.table(src[0], dst[0], kernel)[1].shape[1], R.table(src[1], dst[1], kernel)[1].shape[1]
    for value in (1.0, 0.25, 0.7, 0.0):
        x = np.full((1, 1) + src, value, dtype=np.float32)
        err = np.abs(R.resample(x, dst, kernel).astype(np.float64) - np.float64(np.float32(value))).max()
        assert err <= (value * (Tx + Ty) + 1) * 2.0 ** -24 if value else err == 0.0, (value, err)
    x = _frames((1, 2) + src, seed=5)
    assert np.array_equal(R.resample(x, src, kernel), x)  # R5 on both axes
    if src[0] == dst[0]:  # 33 x 47 -> 33 x 20: the rows pass through, every column is resampled on its own
        assert np.array_equal(R.resample(x, dst, kernel)[:, :, 7], R.resample(x[:, :, 7:8], (1, dst[1]), kernel)[:, :, 0])


# ---------------------------------------------------------------------------------------------------------------- fit_size
def test_fit_size_examples_ties_and_aspect():
    from edvr_amd.y4m import fit_size
    assert fit_size(1920, 2880, '32:27', height=1080, square=True) == (1080, 1920, '1:1')
    assert fit_size(1920, 2880, '8:9', height=1080, square=True) == (1080, 1440, '1:1')
    assert fit_size(2304, 2880, '16:15', height=1080) == (1080, 1350, '16:15')
    assert fit_size(1920, 2880, '32:27', width=1920, square=True) == (1080, 1920, '1:1')  # the mirror
    assert fit_size(1920, 2880, '32:27', size=(1920, 1080)) == (1080, 1920, '1:1')        # 32:27 x (2880 x 1080) / (1920 x 1920)
    assert fit_size(1920, 2880, '32:27', size=(1440, 1080)) == (1080, 1440, '4:3')        # the anamorphic size keeps the display aspect
    # the display aspect survives the rounding: W x SAR / H before == after
    Ho, Wo, tag = fit_size(1920, 2880, '32:27', height=1000)
    num, den = map(int, tag.split(':'))
    assert (Ho, Wo) == (1000, 1500) and Fraction(Wo, Ho) * Fraction(num, den) == Fraction(2880, 1920) * Fraction(32, 27)
    Ho, Wo, tag = fit_size(480, 720, '10:11', height=333)
    num, den = map(int, tag.split(':'))
    assert (Ho, Wo) == (333, 500) and Fraction(Wo, Ho) * Fraction(num, den) == Fraction(720, 480) * Fraction(10, 11)
    # ties go up; multiple=1; at least one multiple
    assert fit_size(4, 6, None, height=2) == (2, 4, None)                 # 3 -> 4
    assert fit_size(4, 6, None, height=2, multiple=1) == (2, 3, None)
    assert fit_size(8, 20, None, height=2, multiple=4) == (2, 4, None)    # 5 -> 4
    assert fit_size(8, 24, None, height=2, multiple=4) == (2, 8, None)    # 6 -> 8
    assert fit_size(6, 4, None, width=2) == (4, 2, None)                  # 3 -> 4 on the other axis
    assert fit_size(64, 8, None, height=8, multiple=4) == (8, 4, None)    # 1 -> at least one multiple
    # an unknown aspect stays unknown, and counts as 1:1 for the arithmetic
    assert fit_size(480, 720, None, height=240) == (240, 360, None)
    assert fit_size(480, 720, '0:0', height=240) == (240, 360, '0:0')
    assert fit_size(480, 720, None, height=240, square=True) == (240, 360, '1:1')
    assert fit_size(480, 720, '1:1', size=(720, 480)) == (480, 720, '1:1')


@pytest.mark.parametrize('kw', [
    dict(), dict(height=8, width=8), dict(size=(8, 8), height=8), dict(size=(8, 8), square=True), dict(height=0), dict(width=-2),
    dict(size=(0, 8)), dict(size=(8,)), dict(height=1), dict(height=200), dict(width=2000), dict(height=8, multiple=0),
])
def test_fit_size_errors(kw):
    from edvr_amd.y4m import fit_size
    with pytest.raises(ValueError):
        fit_size(16, 24, '1:1', **kw)


def test_fit_size_refuses_a_bad_aspect_and_frame():
    from edvr_amd.y4m import fit_size
    for aspect in ('4/3', '4:', ':3', '0:3', '-4:3'):
        with pytest.raises(ValueError):
            fit_size(16, 24, aspect, height=8)
    with pytest.raises(ValueError):
        fit_size(0, 24, None, height=8)


# ---------------------------------------------------------------------------------------------------------------- restore_y4m
class _Nearest4:
    """Stands in for VideoRestorer on the CPU: 'restores' by x4 replication, chunk by chunk.  Its signature is the one from before
    the delivery arguments: a new keyword reaching it is a TypeError."""
    made = []

    def __init__(self, net, out_dtype=None, **kwargs):
        assert out_dtype == torch.float32
        self.scale, self.kwargs = 4, kwargs
        _Nearest4.made.append(self)

    def restore_chunks(self, frames, length=None):
        for piece in frames:
            yield piece.repeat_interleave(4, 2).repeat_interleave(4, 3)


def _yuv(n, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)), dtype=torch.uint8, generator=g)


def _stand_ins(monkeypatch, calls):
    from edvr_amd import ops, video

    def decode(yuv, h, w, matrix, rng, chroma):
        calls.append(('yuv420_to_rgb', h, w, matrix, rng, chroma))
        return U.decode_def(yuv, h, w, matrix, rng, chroma)

    def encode(rgb, matrix, rng, out):
        calls.append(('rgb_to_yuv420', tuple(rgb.shape), matrix, rng))
        return out.copy_(U.encode_def(rgb, matrix, rng))

    def resample(frames, size, kernel='lanczos3', out=None):
        calls.append(('resample', tuple(frames.shape), tuple(size), kernel))
        return torch.from_numpy(R.resample(frames.numpy(), size, kernel))

    monkeypatch.setattr(ops, 'yuv420_to_rgb', decode)
    monkeypatch.setattr(ops, 'rgb_to_yuv420', encode)
    monkeypatch.setattr(ops, 'resample', resample)
    monkeypatch.setattr(video, 'VideoRestorer', _Nearest4)


@pytest.mark.parametrize('H, W, tags, select, expect', [
    # (Ho, Wo, A, matrix_out, kernel)
    (8, 12, 'F30000:1001 Ip A32:27 C420jpeg', dict(out_height=18, square_pixels=True), (18, 32, '1:1', 'bt601', 'lanczos3')),
    (8, 12, 'F25:1 Ip A32:27 C420jpeg', dict(out_height=18, resample='bicubic'), (18, 28, '8:7', 'bt601', 'bicubic')),
    (8, 320, 'F24:1 C420', dict(out_width=640), (16, 640, None, 'bt601', 'lanczos3')),        # 32 x 1280 would be written as BT.709
    (8, 12, 'F24:1 A1:1 C420jpeg', dict(out_size=(34, 20), resample='bilinear'), (20, 34, '15:17', 'bt601', 'bilinear')),
])
def test_restore_y4m_delivers_at_the_fitted_size(monkeypatch, H, W, tags, select, expect):
    """With a selector: the header carries the delivered W, H and fit_size's A, matrix_out follows the DELIVERED size, every chunk goes
    through ops.resample between the restorer and the encode, on_chunk sees what is written, and the payload is the composition by
    hand."""
    from edvr_amd import y4m
    calls, seen = [], []
    _stand_ins(monkeypatch, calls)
    Ho, Wo, aspect, m_out, kernel = expect
    frames = _yuv(5, H, W, seed=3)
    out = io.BytesIO()
    n = y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(frames, H, W, tags)), out, read_frames=2, chunk=3,
                        on_chunk=lambda c: seen.append(tuple(c.shape)), **select)
    assert n == 5 and _Nearest4.made[-1].kwargs == dict(chunk=3)
    head = out.getvalue().split(b'\n')[0].decode().split()
    assert head[1:3] == [f'W{Wo}', f'H{Ho}'] and ([t for t in head if t[0] == 'A'] == ([f'A{aspect}'] if aspect else []))
    r = y4m.Y4MReader(io.BytesIO(out.getvalue()))
    assert (r.width, r.height, r.aspect, r.fps) == (Wo, Ho, aspect, tags.split()[0][1:])
    assert seen == [(2, 3, Ho, Wo), (2, 3, Ho, Wo), (1, 3, Ho, Wo)]
    assert [c for c in calls if c[0] == 'resample'] == [('resample', (k, 3, 4 * H, 4 * W), (Ho, Wo), kernel) for k in (2, 2, 1)]
    assert [c[2] for c in calls if c[0] == 'rgb_to_yuv420'] == [m_out] * 3
    rgb = U.decode_def(frames, H, W, 'bt601' if W < 1280 else 'bt709', 'limited', 'bilinear').repeat_interleave(4, 2).repeat_interleave(4, 3)
    want = U.encode_def(torch.from_numpy(R.resample(rgb.numpy(), (Ho, Wo), kernel)), m_out, 'limited')
    assert torch.equal(r.read(8)[:, 6:], want)


def test_restore_y4m_without_a_selector_makes_the_old_calls(monkeypatch):
    """No selector: the stand-ins - fixed signatures from before the arguments existed - receive exactly the old calls, ops.resample none;
    a delivered size equal to 4 H x 4 W makes no resample call either."""
    from edvr_amd import y4m
    H, W, tags = 8, 12, 'F25:1 Ip A32:27 C420jpeg'
    frames = _yuv(3, H, W, seed=4)
    old = [('yuv420_to_rgb', H, W, 'bt601', 'limited', 'bilinear'), ('yuv420_to_rgb', H, W, 'bt601', 'limited', 'bilinear'),
           ('rgb_to_yuv420', (2, 3, 32, 48), 'bt601', 'limited'), ('rgb_to_yuv420', (1, 3, 32, 48), 'bt601', 'limited')]
    outs = []
    for select in (dict(), dict(out_size=(48, 32)), dict(out_height=32), dict(out_width=48)):
        calls = []
        _stand_ins(monkeypatch, calls)
        out = io.BytesIO()
        assert y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(frames, H, W, tags)), out, read_frames=2, chunk=3, **select) == 3
        assert sorted(calls) == sorted(old), select
        assert _Nearest4.made[-1].kwargs == dict(chunk=3)
        outs.append(out.getvalue())
    assert outs[0].startswith(b'YUV4MPEG2 W48 H32 F25:1 Ip A32:27 C420jpeg\n')
    assert all(o == outs[0] for o in outs[1:])


def test_restore_y4m_refuses_bad_delivery_arguments(monkeypatch):
    from edvr_amd import y4m
    _stand_ins(monkeypatch, [])
    data = U.y4m_bytes(_yuv(1, 8, 12), 8, 12, 'F25:1 Ip A1:1 C420jpeg')
    for kw in (dict(out_height=16, out_width=24), dict(out_size=(24, 16), square_pixels=True), dict(square_pixels=True), dict(out_height=2),
               dict(out_height=16, resample='lanczos2'), dict(resample='nearest'), dict(out_width=0)):
        out = io.BytesIO()
        with pytest.raises(ValueError):
            y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(data), out, **kw)
        assert out.getvalue() == b'', kw  # refused before the header is written


# ---------------------------------------------------------------------------------------------------------------- the op and the script
def test_ops_resample_refuses_the_cpu():
    from edvr_amd import ops
    with pytest.raises(NotImplementedError):
        ops.resample(torch.zeros(1, 3, 8, 8), (4, 4))


def test_resample_tile_follows_the_ratio():
    """Host arithmetic of the library: 64 columns; 32 rows, fewer as H / Ho grows toward 8 - the LDS stays within 64 KB."""
    from edvr_amd import ops
    from edvr_amd.resample import taps
    tile = lambda H, W, Ho, Wo, k='lanczos3': ops.resample_tile(H, W, Ho, Wo, taps(H, Ho, k), taps(W, Wo, k))
    assert tile(1920, 2880, 1080, 1920) == (32, 64) and tile(720, 1280, 1080, 1920) == (32, 64)
    assert tile(640, 96, 80, 12) == (16, 64)  # the ratio 8, 49 taps
    tohs = [tile(80 * r, 96, 80, 12)[0] for r in range(1, 9)]
    assert tohs == sorted(tohs, reverse=True) and tohs[0] == 32 and tohs[-1] == 16
    for toh, r in zip(tohs, range(1, 9)):  # the rows of mid, the tables: what csrc/resample.hip asks for
        Ty, Tx = taps(80 * r, 80, 'lanczos3'), taps(96, 12, 'lanczos3')
        assert 4 * (min(80 * r, (toh - 1) * r + Ty) * 64 + Tx * 64 + toh * Ty + 64 + toh) <= 64 * 1024
    with pytest.raises(ValueError):
        ops.resample_tile(8, 8, 4, 4, 50, 5)
    with pytest.raises(ValueError):
        ops.resample_tile(80, 8, 9, 8, 49, 1)


def _script():
    spec = importlib.util.spec_from_file_location('restore_video', os.path.join(ROOT, 'scripts', 'restore_video.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restore_video_delivery_flags(capsys):
    mod = _script()
    with pytest.raises(SystemExit) as e:
        mod.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--out-size', '--out-height', '--out-width', '--square-pixels', '--resample'):
        assert opt in text, opt
    args = mod.parse_args(['-', '-'])
    assert (args.out_size, args.out_height, args.out_width, args.square_pixels, args.resample) == (None, None, None, False, 'lanczos3')
    args = mod.parse_args(['-', '-', '--deinterlace', 'film', '--out-height', '1080', '--square-pixels'])
    assert (args.out_size, args.out_height, args.out_width, args.square_pixels, args.resample) == (None, 1080, None, True, 'lanczos3')
    args = mod.parse_args(['-', '-', '--out-size', '1920x1080', '--resample', 'bicubic'])
    assert (args.out_size, args.resample) == ((1920, 1080), 'bicubic')
    assert mod.parse_args(['-', '-', '--out-width', '1280']).out_width == 1280
    for bad in (['-', '-', '--out-height', '1080', '--out-width', '1920'], ['-', '-', '--out-size', '1920x1080', '--out-height', '1080'],
                ['-', '-', '--out-size', '1920x1080', '--out-width', '1920'], ['-', '-', '--out-size', '1920x1080', '--square-pixels'],
                ['-', '-', '--square-pixels'], ['-', '-', '--out-size', '1920'], ['-', '-', '--out-size', '0x1080'], ['-', '-', '--out-size', '1920:1080'],
                ['-', '-', '--out-height', '0'], ['-', '-', '--out-height', '1080', '--resample', 'nearest'], ['-', '-', '--resample', 'bicubic']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
