"""GPU: ops.resample (csrc/resample.hip) against the NumPy restatement of DESIGN 4.21 (tests/resample_ref.py), bit for bit, on the smallest
shapes that reach every path - frames shorter than a row of taps (both edges clamped at once), the ratios 8 and 1/8, identity axes,
anisotropic ratios, outputs on and around the tile's edges, vector and scalar loads and stores, sliced and offset tensors on either side,
one and three planes; the batch rule R7; the error paths; and restore_y4m(out_height=...) through a tiny EDVR against the composition
done by hand."""
import ctypes
import io

import numpy as np
import pytest
import torch

import resample_ref as R
import util_yuv as U

pytestmark = pytest.mark.gpu

KERNELS = ['lanczos3', 'bicubic', 'bilinear']


def _frames(shape, seed):
    """float32 in [-0.5, 1.5] with a flat patch of 0 and one of 1 in every plane."""
    x = np.random.default_rng(seed).random(shape, dtype=np.float32) * 2.0 - 0.5
    H, W = shape[-2:]
    x[..., : max(H // 3, 1), : max(W // 3, 1)] = 0.0
    x[..., H - max(H // 3, 1):, W - max(W // 3, 1):] = 1.0
    return x.astype(np.float32)


def _same(got, x, size, kernel):
    want = torch.from_numpy(R.resample(x, size, kernel))
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got, want), f'{tuple(x.shape)} -> {size} {kernel}: {int((got != want).sum())} of {want.numel()} differ, ' \
                                   f'max {float((got - want).abs().max()):.3g}'


def _check(shape, size, kernel, seed=0):
    from edvr_amd import ops
    x = _frames(shape, seed)
    _same(ops.resample(torch.from_numpy(x).cuda(), size, kernel), x, size, kernel)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('size', [(3, 4), (17, 23)])
def test_both_edges_clamped_at_once(size, kernel):
    """5 x 7 samples: a row of taps is longer than the frame, so one output sample repeats the first AND the last sample (R4)."""
    first, w = R.table(5, size[0], kernel)
    assert w.shape[1] > 5 or kernel != 'lanczos3'
    if w.shape[1] > 5:
        assert ((first < 0) & (first + w.shape[1] - 1 > 4)).any()
    _check((2, 3, 5, 7), size, kernel, seed=1)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('shape, size', [((1, 3, 64, 96), (8, 12)), ((1, 3, 6, 9), (48, 72))])
def test_the_ratios_8_and_one_eighth(shape, size, kernel):
    if kernel == 'lanczos3' and size == (8, 12):
        assert R.table(64, 8, kernel)[1].shape[1] == 49
    _check(shape, size, kernel, seed=2)


@pytest.mark.parametrize('kernel', KERNELS)
def test_identity_axes(kernel):
    from edvr_amd import ops
    _check((2, 3, 33, 47), (33, 20), kernel, seed=3)
    _check((2, 3, 33, 47), (66, 47), kernel, seed=3)
    x = torch.from_numpy(_frames((2, 3, 33, 47), 3)).cuda()
    assert torch.equal(ops.resample(x, (33, 47), kernel), x)  # R5 on both axes: the input, bit for bit


@pytest.mark.parametrize('kernel', KERNELS)
def test_anisotropic_ratios(kernel):
    _check((1, 3, 96, 144), (54, 96), kernel, seed=4)  # 16 / 9 down the rows, 3 / 2 along them


def _tile(H, W, Ho, Wo, kernel='lanczos3'):
    from edvr_amd import ops
    return ops.resample_tile(H, W, Ho, Wo, R.table(H, Ho, kernel)[1].shape[1], R.table(W, Wo, kernel)[1].shape[1])


@pytest.mark.parametrize('dh', [-1, 0, 1, None])
def test_outputs_on_and_around_the_tile_edges(dh):
    """Ho in {toh - 1, toh, toh + 1, 2 toh + 1} x Wo in {tow - 1, tow, tow + 1, 2 tow + 1} from a source about 1.5 x larger: the last
    tile of a row / column of tiles holds all, one or all-but-one of its samples."""
    from edvr_amd import ops
    toh, tow = _tile(48, 96, 32, 64)
    Ho = 2 * toh + 1 if dh is None else toh + dh
    for Wo in (tow - 1, tow, tow + 1, 2 * tow + 1):
        H, W = (3 * Ho + 1) // 2, (3 * Wo + 1) // 2
        assert _tile(H, W, Ho, Wo) == (toh, tow)
        _check((1, 2, H, W), (Ho, Wo), 'lanczos3', seed=Ho + Wo)
    # the smaller tile of a steep reduction: toh has shrunk
    toh8, _ = _tile(8 * (toh + 1), 16, toh + 1, 16)
    assert toh8 < toh
    for Ho in (toh8, toh8 + 1) if dh == 0 else ():
        _check((1, 1, 8 * Ho, 16), (Ho, 16), 'lanczos3', seed=Ho)


@pytest.mark.parametrize('c', [1, 3])
def test_access_widths_and_layouts(c):
    from edvr_amd import ops
    # W and Wo odd: scalar loads and stores
    _check((2, c, 45, 67), (30, 45), 'lanczos3', seed=5)
    # W and Wo multiples of 4, aligned: 16-byte loads and stores - and the same bits from every other layout of the same samples
    x = _frames((4, c, 24, 40), 6)
    size = (36, 28)
    g = torch.from_numpy(x).cuda()
    assert g.data_ptr() % 16 == 0
    vec = ops.resample(g, size)
    _same(vec, x, size, 'lanczos3')
    # a source that is frames 1:3 of a longer tensor
    _same(ops.resample(g[1:3], size), x[1:3], size, 'lanczos3')
    # a source whose storage starts one float past a 16-byte boundary: scalar loads, the same bits
    store = torch.empty(x.size + 1, dtype=torch.float32, device='cuda')
    off = store[1:].view(x.shape)
    off.copy_(g)
    assert off.data_ptr() % 16 == 4
    assert torch.equal(ops.resample(off, size), vec)
    # out= a slice of a longer tensor: written there, the rest untouched
    long = torch.full((7, c) + size, -7.0, dtype=torch.float32, device='cuda')
    assert ops.resample(g, size, out=long[2:6]).data_ptr() == long[2].data_ptr()
    assert torch.equal(long[2:6], vec) and bool((long[:2] == -7.0).all()) and bool((long[6:] == -7.0).all())
    # out= one float past a 16-byte boundary: scalar stores, the same bits, nothing before or behind
    store = torch.full((vec.numel() + 2,), -7.0, dtype=torch.float32, device='cuda')
    o = store[1:-1].view(vec.shape)
    ops.resample(g, size, out=o)
    assert torch.equal(o, vec) and float(store[0]) == -7.0 and float(store[-1]) == -7.0
    # a channel slice: dense planes, a larger image stride
    if c == 3:
        _same(ops.resample(g[:, 1:3], size, 'bicubic'), x[:, 1:3], size, 'bicubic')
        wide = torch.full((4, 5) + size, -7.0, dtype=torch.float32, device='cuda')
        ops.resample(g, size, out=wide[:, 1:4])
        assert torch.equal(wide[:, 1:4], vec) and bool((wide[:, 0] == -7.0).all()) and bool((wide[:, 4] == -7.0).all())


def test_a_frame_does_not_depend_on_its_place_in_the_batch():
    from edvr_amd import ops
    x = torch.from_numpy(_frames((5, 3, 37, 52), 7)).cuda()
    whole = ops.resample(x, (50, 31), 'bicubic')
    for i in range(5):
        assert torch.equal(ops.resample(x[i:i + 1], (50, 31), 'bicubic')[0], whole[i])


def test_errors_before_any_launch(monkeypatch):
    from edvr_amd import _lib, ops
    seen = []
    monkeypatch.setattr(ops, 'LAUNCH_HOOK', lambda name, flops, launch, nbytes, executed=None: (seen.append((name, nbytes)), launch()))
    x = torch.zeros(2, 3, 16, 24, device='cuda')
    with pytest.raises(NotImplementedError):
        ops.resample(x.cpu(), (8, 8))
    for bad, size, kw in ((x.half(), (8, 8), {}), (x.double(), (8, 8), {}), (x[0], (8, 8), {}), (x[None], (8, 8), {}), (x, (8, 8), dict(kernel='lanczos2')),
                          (x, (1, 8), {}), (x, (8, 2), {}), (x, (129, 24), {}), (x, (16, 193), {}), (x, (0, 8), {}), (x, (8,), {}), (x, 8, {}),
                          (x, (8, 8), dict(out=torch.zeros(2, 3, 8, 9, device='cuda'))), (x, (8, 8), dict(out=torch.zeros(2, 3, 8, 8, device='cuda').double())),
                          (x, (8, 8), dict(out=torch.zeros(2, 3, 8, 8))), (x, (8, 8), dict(out=torch.zeros(2, 3, 8, 16, device='cuda')[..., ::2])),
                          (x, (16, 24), dict(out=x))):
        with pytest.raises(ValueError):
            ops.resample(bad, size, **kw)
    assert seen == []
    out = ops.resample(x, (8, 36))
    assert seen == [('resample', 4.0 * 2 * 3 * (16 * 24 + 8 * 36))] and out.shape == (2, 3, 8, 36)
    # the C ABI refuses what the Python layer never sends
    from edvr_amd.resample import device_table
    fy, wy, ty = device_table(16, 8, 'lanczos3', x.device)
    fx, wx, tx = device_table(24, 36, 'lanczos3', x.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(src=ptr(x), dst=ptr(out), n=2, c=3, H=16, W=24, si=3 * 16 * 24, Ho=8, Wo=36, so=3 * 8 * 36, fy=ptr(fy), wy=ptr(wy), Ty=ty, fx=ptr(fx),
                wx=ptr(wx), Tx=tx)
    call = lambda **kw: _lib.lib().edvr_resample_f32(*{**good, **kw}.values(), stream)
    for kw in (dict(src=None), dict(dst=None), dict(fy=None), dict(wy=None), dict(fx=None), dict(wx=None), dict(n=0), dict(n=65536), dict(c=0), dict(H=0),
               dict(Wo=0), dict(Ty=0), dict(Ty=50), dict(Tx=0), dict(Tx=50), dict(Ho=1), dict(Wo=2), dict(Ho=129), dict(Wo=193),
               dict(si=3 * 16 * 24 - 1), dict(so=3 * 8 * 36 - 1)):
        assert call(**kw) != 0, kw
    assert b'resample' in _lib.lib().edvr_last_error()
    want = out.clone()
    out.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ---------------------------------------------------------------------------------------------------------------- restore_y4m
def test_restore_y4m_delivers_like_the_composition_by_hand():
    """7 frames of 20 x 24 A32:27 through a tiny EDVR with out_height=60, square_pixels=True: 80 x 96 becomes 60 x 86 A1:1, and the
    bytes are decode, VideoRestorer.restore, ops.resample, rgb_to_yuv420 done by hand under the expected header."""
    from edvr_amd import VideoRestorer, ops
    from edvr_amd.y4m import fit_size, restore_y4m
    from test_gpu_yuv import _net, _yuv
    net = _net()
    n, H, W = 7, 20, 24
    assert fit_size(4 * H, 4 * W, '32:27', height=60, square=True) == (60, 86, '1:1')
    frames = _yuv(n, H, W, 11)
    data = U.y4m_bytes(frames, H, W, 'F25:1 Ip A32:27 C420jpeg')
    seen = []
    with torch.no_grad():
        rgb = ops.yuv420_to_rgb(frames.cuda(), H, W, 'bt601', 'limited', 'bilinear')
        restored = VideoRestorer(net, out_dtype=torch.float32, chunk=4).restore(rgb)
        small = ops.resample(restored, (60, 86))
        want = U.y4m_bytes(ops.rgb_to_yuv420(small, 'bt601', 'limited').cpu(), 60, 86, 'F25:1 Ip A1:1 C420jpeg')
        got = io.BytesIO()
        assert restore_y4m(net, io.BytesIO(data), got, read_frames=3, chunk=4, out_height=60, square_pixels=True,
                           on_chunk=lambda c: seen.append(c.clone())) == n
        same = io.BytesIO()  # a delivered size equal to 4 H x 4 W: the stream of a call without a selector
        plain = io.BytesIO()
        restore_y4m(net, io.BytesIO(data), same, read_frames=3, chunk=4, out_size=(4 * W, 4 * H))
        restore_y4m(net, io.BytesIO(data), plain, read_frames=3, chunk=4)
    net.check_offsets()
    assert got.getvalue().startswith(b'YUV4MPEG2 W86 H60 F25:1 Ip A1:1 C420jpeg\nFRAME\n')
    assert got.getvalue() == want
    assert torch.equal(torch.cat(seen), small)  # on_chunk sees what is written
    assert same.getvalue() == plain.getvalue() and plain.getvalue().startswith(b'YUV4MPEG2 W96 H80 F25:1 Ip A32:27 C420jpeg\n')


def test_restore_y4m_deinterlaces_then_delivers():
    """The stages compose: an It stream, deinterlaced at field rate, restored, resampled - against the same composition by hand."""
    import util_deint as UD
    from edvr_amd import VideoRestorer, ops
    from edvr_amd.y4m import restore_y4m
    from test_gpu_yuv import _net
    net = _net()
    n, H, W = 4, 16, 32
    frames = UD.structured_clip(n, H, W, '420', 'top')
    woven = UD.y4m_bytes(frames, H, W, 'F25:1 It A16:15 C420jpeg')
    with torch.no_grad():
        prog = ops.deinterlace(torch.from_numpy(frames).cuda(), H, W, '420', first='top', mode='field')
        restored = VideoRestorer(net, out_dtype=torch.float32, chunk=4).restore(ops.yuv420_to_rgb(prog, H, W, 'bt601', 'limited', 'bilinear'))
        small = ops.resample(restored, (36, 72), 'bicubic')
        want = U.y4m_bytes(ops.rgb_to_yuv420(small, 'bt601', 'limited').cpu(), 36, 72, 'F50:1 Ip A16:15 C420jpeg')
        got = io.BytesIO()
        assert restore_y4m(net, io.BytesIO(woven), got, read_frames=3, chunk=4, deinterlace='field', out_width=72, resample='bicubic') == 2 * n
    net.check_offsets()
    assert got.getvalue() == want
