"""-m gpu: self-ensemble on the whole-video path (edvr_amd/video.py: self_ensemble; csrc/ensemble.hip: the oriented reads and the
oriented, accumulating rectangle tails) - kernel by kernel against the torch composition of the definition and of today's whole-tile
ops, and the whole network bit for bit against the definition evaluated with today's VideoRestorer on host-transformed frames."""
import pytest
import torch
import torch.nn.functional as F

from util_edvr import CONFIGS, randomize_offsets

pytestmark = pytest.mark.gpu


def _g(x, k):
    """The definition: k = 4 t + 2 v + h; transpose if t, then flip rows if v, then flip columns if h."""
    if k & 4:
        x = x.transpose(-1, -2)
    if k & 2:
        x = x.flip(-2)
    if k & 1:
        x = x.flip(-1)
    return x


def _g_inv(y, k):
    if k & 1:
        y = y.flip(-1)
    if k & 2:
        y = y.flip(-2)
    if k & 4:
        y = y.transpose(-1, -2)
    return y


def _up(v, m):
    return (v + m - 1) // m * m


def _bytes(n, h, w, seed=0):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _video(n, h, w, seed=0):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ oriented reads
@pytest.mark.parametrize('hw', [(30, 46), (7, 45), (6, 6)])
@pytest.mark.parametrize('k', range(8))
def test_oriented_read_is_the_symmetry_of_pad_and_slice(gpu, k, hw):
    from edvr_amd import ops
    H, W = hw
    n = 3
    u8 = _bytes(n, H, W, seed=H + W).to(gpu)
    as_float = ops.frames_u8_to_f32(u8[None])[0]                      # the existing conversion of these bytes
    big = torch.rand(n + 2, 5, H, W, generator=torch.Generator().manual_seed(1)).to(gpu)
    strided = big[1:1 + n, 1:4]                                       # an image-strided float source
    Hp, Wp = _up(H, 4), _up(W, 4)
    rects = [(0, 0, Hp, Wp),                                          # the whole padded frame (a multiple of 4, not of the LDS tile)
             (1, 1, H - 2, W - 2),                                    # interior
             (1, W - 3, H - 1, 4),                                    # width 4 (narrower than any LDS tile), across the right edge
             (H - 2, 2, Hp - H + 2, W - 2)]                           # across the bottom edge
    for mode in ('reflect', 'replicate'):
        for src, ref_src in ((u8, as_float), (strided, strided), (as_float, as_float)):
            padded = F.pad(ref_src, (0, W - 1, 0, H - 1), mode=mode)
            for y0, x0, th, tw in rects:
                got = ops.crop_pad_frames_d4(src, y0, x0, th, tw, mode, k)
                want = _g(padded[:, :, y0:y0 + th, x0:x0 + tw], k)
                assert got.is_contiguous() and got.dtype == torch.float32 and got.shape == want.shape
                assert torch.equal(got, want), (k, mode, src.dtype, (y0, x0, th, tw))
    assert torch.equal(ops.crop_pad_frames_d4(u8, 1, 1, 4, 4, None, k), _g(as_float[:, :, 1:5, 1:5], k))  # pad_mode=None: a plain crop
    with pytest.raises(ValueError):
        ops.crop_pad_frames_d4(u8, 0, 0, H + 1, W, None, k)
    with pytest.raises(ValueError):
        ops.crop_pad_frames_d4(u8, 0, 0, 2 * H, W, 'reflect', k)
    with pytest.raises(ValueError):
        ops.crop_pad_frames_d4(u8, 0, 0, 4, 4, 'reflect', 8)
    with pytest.raises(NotImplementedError):
        ops.crop_pad_frames_d4(u8.cpu(), 0, 0, 4, 4, mode, k)


# ------------------------------------------------------------------------------------------------ oriented, accumulating tails
# (destination size (Ho, Wo), where the rectangle lands (oy, ox), rectangle in the un-transformed 32 x 48 tile result (ky, kx, kh, kw)):
# the rectangles of tests/test_gpu_video_tiles.py and one of odd origin
RECTS = [((40, 64), (0, 0), (0, 0, 16, 24)),
         ((40, 64), (8, 16), (16, 0, 16, 48)),
         ((40, 64), (4, 12), (8, 12, 20, 28)),
         ((37, 61), (3, 5), (8, 12, 20, 28)),
         ((37, 61), (5, 2), (3, 5, 22, 31)),
         ((32, 48), (0, 0), (0, 0, 32, 48)),
         ((40, 64), (3, 1), (1, 3, 30, 44))]


def test_rects_cover_the_rectangle_store_tests():
    import test_gpu_video_tiles as plain
    assert RECTS[:len(plain.RECTS)] == plain.RECTS and len(RECTS) == len(plain.RECTS) + 1


@pytest.mark.parametrize('up', [True, False])
@pytest.mark.parametrize('k', range(8))
def test_oriented_tails_accumulate_the_whole_tile_values(gpu, k, up):
    from edvr_amd import ops
    n, N, fh, fw = 2, 4, 32, 48                                        # the result in the frame's orientation: 32 x 48
    g = torch.Generator().manual_seed(40 + k)
    # every element has a result of its own, in its own orientation: the whole-tile value = today's whole-tile op on it
    elements = [k, (k + 3) % 8, (k + 5) % 8, (k + 6) % 8]
    tiles = []
    for e in elements:
        hy, wy = (fw, fh) if e & 4 else (fh, fw)
        if up:
            base = (torch.randn(n, 3, hy // 4, wy // 4, generator=g) * 0.8 + 0.5).to(gpu)
            y = (torch.randn(n, 3, hy, wy, generator=g) * 0.5).to(gpu)
            tiles.append((y, base, ops.upsample4x_add_(y.clone(), base)))
        else:
            x = (torch.randn(n, 5, hy, wy, generator=g) * 0.6 + 0.5).to(gpu)[:, 1:4]  # an image-strided result (the hr_in tail's input)
            tiles.append((x, None, x))
    for (Ho, Wo), (oy, ox), (ky, kx, kh, kw) in RECTS:
        for count in (3, 4):                                           # first / middle / last and first / middle / middle / last
            modes = ['first'] + ['middle'] * (count - 2) + ['last']
            scale = 1.0 / count
            values = [_g_inv(full, e)[:, :, ky:ky + kh, kx:kx + kw] for e, (_, _, full) in zip(elements[:count], tiles)]
            acc = values[0]
            for v in values[1:]:
                acc = acc + v                                          # float32 adds in the order of the launches
            want = acc * scale
            want_u8 = ops.f32_to_u8_hwc(want.contiguous())             # to_u8 by the existing byte op
            # float32 output: the accumulator is the output
            dst = torch.full((N, 3, Ho, Wo), 77.0, device=gpu)
            view = dst[1:1 + n, :, oy:oy + kh, ox:ox + kw]
            for e, m, (y, base, _) in zip(elements, modes, tiles):
                got = ops.upsample4x_add_rect_d4(y, base, view, ky, kx, e, m, scale) if up else ops.copy_rect_d4(y, view, ky, kx, e, m, scale)
                assert got is view
            assert torch.equal(view, want), (k, count, (ky, kx, kh, kw), 'float32')
            untouched = torch.ones_like(dst, dtype=torch.bool)
            untouched[1:1 + n, :, oy:oy + kh, ox:ox + kw] = False
            assert bool((dst[untouched] == 77).all())
            # uint8 output: a float32 scratch accumulates, the last launch alone writes bytes
            scratch = torch.full((N, 3, Ho, Wo), 55.0, device=gpu)
            out = torch.full((N, Ho, Wo, 3), 77, dtype=torch.uint8, device=gpu)
            a_view, o_view = scratch[1:1 + n, :, oy:oy + kh, ox:ox + kw], out[1:1 + n, oy:oy + kh, ox:ox + kw]
            for e, m, (y, base, _) in zip(elements, modes, tiles):
                if m == 'last':
                    assert bool((out == 77).all())                     # no byte written before the last launch
                if up:
                    ops.upsample4x_add_u8_rect_d4(y, base, o_view, a_view, ky, kx, e, m, scale)
                else:
                    ops.f32_to_u8_hwc_rect_d4(y, o_view, a_view, ky, kx, e, m, scale)
            assert torch.equal(o_view, want_u8), (k, count, (ky, kx, kh, kw), 'uint8')
            untouched = torch.ones_like(out, dtype=torch.bool)
            untouched[1:1 + n, oy:oy + kh, ox:ox + kw] = False
            assert bool((out[untouched] == 77).all())
            assert bool((scratch[untouched.permute(0, 3, 1, 2)] == 55).all())
    # an ensemble of one: the value itself
    (Ho, Wo), (oy, ox), (ky, kx, kh, kw) = RECTS[3]
    y, base, full = tiles[0]
    dst = torch.full((n, 3, Ho, Wo), 77.0, device=gpu)
    view = dst[:, :, oy:oy + kh, ox:ox + kw]
    ops.upsample4x_add_rect_d4(y, base, view, ky, kx, k, 'only', 1.0) if up else ops.copy_rect_d4(y, view, ky, kx, k, 'only', 1.0)
    assert torch.equal(view, _g_inv(full, k)[:, :, ky:ky + kh, kx:kx + kw])
    with pytest.raises(ValueError):
        ops.copy_rect_d4(tiles[0][2], view, ky, kx, k, 'sum', 1.0)
    with pytest.raises(ValueError):                                    # reaches beyond the result in the frame's orientation
        ops.copy_rect_d4(tiles[0][2], torch.empty(n, 3, 8, 8, device=gpu), fh - 4, 0, k, 'only', 1.0)


# ------------------------------------------------------------------------------------------------ whole path
def _net(name, seed=10):
    from edvr_amd import EDVR
    kwargs, _ = CONFIGS[name]
    torch.manual_seed(seed)
    return randomize_offsets(EDVR(**kwargs)).eval(), kwargs


# name, (H, W), pad_mode, tile, overlap
CASES = {'M_24x40': ('M_T5', (24, 40), None, None, None),
         'M_30x46_reflect': ('M_T5', (30, 46), 'reflect', None, None),
         'L_deblur_hr_56x72_reflect': ('L_deblur_hr', (56, 72), 'reflect', None, None),
         'M_62x90_tiles': ('M_T5', (62, 90), 'reflect', (32, 48), 8)}
ENSEMBLES = {'flip4': (0, 1, 2, 3), 'd4': tuple(range(8)), 'seq_5_0_2': (5, 0, 2)}
_NETS, _PLAIN = {}, {}  # the networks and the per-element references R(g_k(crop)) are computed once and shared


def _case(case, gpu):
    from edvr_amd import tile_grid
    name, (H, W), pad_mode, tile, overlap = CASES[case]
    if name not in _NETS:
        net, kwargs = _net(name)
        _NETS[name] = (net.to(gpu), kwargs)
    net, kwargs = _NETS[name]
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    lq = _video(9, H, W, seed=3).to(gpu)
    padded = F.pad(lq, (0, _up(W, m) - W, 0, _up(H, m) - H), mode=pad_mode) if pad_mode else lq
    return net, m, s, lq, padded, tile_grid(H, W, tile, overlap, m), dict(pad_mode=pad_mode, tile=tile, tile_overlap=overlap)


def _definition(case, gpu, f4s, elements, lq=None, key=None):
    """The definition with today's VideoRestorer: per tile, acc = sum over the elements (in order, float32) of g^-1(R(g(crop of P(lq)))),
    times 1 / n, the kept rectangles put together and cropped - float32 (9, 3, s H, s W)."""
    from edvr_amd import VideoRestorer
    net, m, s, lq0, padded, grid, _ = _case(case, gpu)
    if lq is not None:
        H, W = lq.shape[-2:]
        mode = CASES[case][2]
        padded = F.pad(lq, (0, _up(W, m) - W, 0, _up(H, m) - H), mode=mode) if mode else lq
    H, W = CASES[case][1]
    want = torch.empty(9, 3, s * H, s * W, device=gpu)
    for ti, ((y0, x0, th, tw), (ky, kx, kh, kw), (oy, ox)) in enumerate(grid):
        crop = padded[:, :, y0:y0 + th, x0:x0 + tw]
        acc = None
        for k in elements:
            ck = (case, key, f4s, ti, k)
            if ck not in _PLAIN:
                _PLAIN[ck] = VideoRestorer(net, chunk=4).restore(_g(crop, k).contiguous())
            back = _g_inv(_PLAIN[ck], k)
            acc = back if acc is None else acc + back
        acc = acc * (1.0 / len(elements))
        want[:, :, s * oy:s * (oy + kh), s * ox:s * (ox + kw)] = acc[:, :, s * ky:s * (ky + kh), s * kx:s * (kx + kw)]
    return want


@pytest.mark.parametrize('f4s', [True, False])
@pytest.mark.parametrize('ensemble', sorted(ENSEMBLES))
@pytest.mark.parametrize('case', sorted(CASES))
def test_self_ensemble_is_the_definition(gpu, case, ensemble, f4s):
    from edvr_amd import VideoRestorer, ops
    elements = ENSEMBLES[ensemble]
    arg = elements if ensemble.startswith('seq') else ensemble
    net, m, s, lq, padded, grid, kw = _case(case, gpu)
    H, W = CASES[case][1]
    prev = ops.set_f4s(inference=f4s)
    try:
        with torch.no_grad():
            want = _definition(case, gpu, f4s, elements)
            want_u8 = ops.f32_to_u8_hwc(want)
            vr = VideoRestorer(net, chunk=4, self_ensemble=arg, **kw)   # 9 frames, chunk 4: the ring wraps, the last group is short
            got = vr.restore(lq)
            assert got.is_contiguous() and got.dtype == torch.float32 and tuple(got.shape) == (9, 3, s * H, s * W)
            assert torch.equal(got, want), (case, ensemble, 'float32')
            assert len(vr.pairs) == len(grid) * len(elements)
            got8 = VideoRestorer(net, chunk=4, out_dtype=torch.uint8, self_ensemble=arg, **kw).restore(lq)
            assert got8.is_contiguous() and got8.dtype == torch.uint8 and tuple(got8.shape) == (9, s * H, s * W, 3)
            assert torch.equal(got8, want_u8), (case, ensemble, 'uint8')
        torch.cuda.synchronize()
    finally:
        ops.set_f4s(inference=prev[0])
    net.check_offsets()


def test_uint8_frames_stay_bytes_and_streaming_equals_restore(gpu):
    from edvr_amd import VideoRestorer, ops
    case, elements = 'M_30x46_reflect', (5, 0, 2)
    net, m, s, _, _, grid, kw = _case(case, gpu)
    H, W = CASES[case][1]
    lq8 = _bytes(9, H, W, seed=4).to(gpu)
    with torch.no_grad():
        want = _definition(case, gpu, ops.F4S_INFERENCE, elements, lq=ops.frames_u8_to_f32(lq8[None])[0], key='bytes')
        for dt, ref in ((torch.float32, want), (torch.uint8, ops.f32_to_u8_hwc(want))):
            vr = VideoRestorer(net, chunk=4, out_dtype=dt, self_ensemble=elements, **kw)
            assert torch.equal(vr.restore(lq8), ref), dt
            seen = []
            frames = []
            for f in vr.restore_iter(iter(lq8.unbind(0))):             # frame by frame
                frames.append(f)
                seen.append((vr.bank_frames, len(vr.banks)))
            assert torch.equal(torch.stack(frames), ref), dt
            # as documented: one bank per (tile, element) pair, each a ring of at most `capacity` frames
            assert all(nb == len(grid) * len(elements) for _, nb in seen) and max(bf for bf, _ in seen) <= vr.slots <= vr.capacity <= 4 + 2 * 4
            assert vr.banks is None and len(vr.pairs) == len(grid) * len(elements)
    torch.cuda.synchronize()
    net.check_offsets()


def test_an_ensemble_of_the_identity_is_the_plain_tiled_path(gpu):
    from edvr_amd import VideoRestorer
    net, m, s, lq, _, grid, kw = _case('M_62x90_tiles', gpu)
    with torch.no_grad():
        for dt in (torch.float32, torch.uint8):
            plain = VideoRestorer(net, chunk=4, out_dtype=dt, **kw).restore(lq)
            one = VideoRestorer(net, chunk=4, out_dtype=dt, self_ensemble=(0,), **kw).restore(lq)
            assert torch.equal(one, plain), dt
    torch.cuda.synchronize()
    net.check_offsets()


def test_validate_video_with_self_ensemble(gpu):
    from edvr_amd import VideoRestorer, metrics
    net, m, s, lq, _, _, kw = _case('M_30x46_reflect', gpu)
    lq = lq[:6]
    H, W = CASES['M_30x46_reflect'][1]
    gt = torch.rand(6, 3, 4 * H, 4 * W, generator=torch.Generator().manual_seed(8)).to(gpu)
    with torch.no_grad():
        out, psnr = metrics.validate_video(net, lq, gt, num_frame=5, chunk=4, pad_mode='reflect', self_ensemble='flip4')
        want = VideoRestorer(net, chunk=4, pad_mode='reflect', self_ensemble='flip4').restore(lq)
        plain, _ = metrics.validate_video(net, lq, gt, num_frame=5, chunk=4, pad_mode='reflect')
    assert torch.equal(out, want) and not torch.equal(out, plain)
    assert psnr == metrics.calculate_psnr(want[:4], gt[:4], 0, False) + metrics.calculate_psnr(want[4:], gt[4:], 0, False) and len(psnr) == 6
    net.check_offsets()
