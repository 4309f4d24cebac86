"""-m gpu: frames of any size on the whole-video path (edvr_amd/video.py: pad_mode / tile; csrc/video.hip: crop_pad_frames and the
rectangle stores) - kernel by kernel against ATen, the whole network bit for bit against the plain path on host-padded frames and on
each tile's crop, and against the fp64 oracle."""
import pytest
import torch
import torch.nn.functional as F

from util_edvr import CONFIGS, oracle_kwargs, randomize_offsets

pytestmark = pytest.mark.gpu

INTERMEDIATE_RTOL = 2e-4   # the project's whole-network bound (tests/test_gpu_video.py, tests/test_gpu_edvr.py)
PSNR_TOL_DB = 1e-3


def _net(name, seed=10):
    from edvr_amd import EDVR
    kwargs, _ = CONFIGS[name]
    torch.manual_seed(seed)
    return randomize_offsets(EDVR(**kwargs)).eval(), kwargs


def _video(n, h, w, seed=0):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


def _bytes(n, h, w, seed=0):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _up(v, m):
    return (v + m - 1) // m * m


def _host_pad(x, m, mode):
    H, W = x.shape[-2:]
    return F.pad(x, (0, _up(W, m) - W, 0, _up(H, m) - H), mode=mode)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('mode', ['reflect', 'replicate'])
@pytest.mark.parametrize('width', [44, 45, 6])
def test_crop_pad_frames_is_pad_and_slice(gpu, mode, width):
    from edvr_amd import ops
    H, W, n = 21, width, 3
    u8 = _bytes(n, H, W, seed=width).to(gpu)
    as_float = ops.frames_u8_to_f32(u8[None])[0]                      # the floats the plain path feeds the network for these bytes
    big = torch.rand(n + 2, 5, H, W, generator=torch.Generator().manual_seed(1)).to(gpu)
    strided = big[1:1 + n, 1:4]                                       # an image-strided float source
    ph, pw = (H - 1, W - 1) if mode == 'reflect' else (9, 11)         # as far as the mode reaches
    rects = [(0, 0, H, W), (2, 1, 8, 4), (4, 0, 12, _up(W, 4) if _up(W, 4) - W <= pw else W),  # inside / crossing the right edge
             (H - 5, 0, 5 + min(ph, 7), W), (H - 4, W - 3, 4 + min(ph, 4), 3 + min(pw, 5)),  # crossing the bottom edge / both
             (0, 0, H + min(ph, 3), W + min(pw, 4 - W % 4))]
    for src, ref_src in ((u8, as_float), (strided, strided), (as_float, as_float)):
        padded = F.pad(ref_src, (0, pw, 0, ph), mode=mode)
        for y0, x0, th, tw in rects:
            got = ops.crop_pad_frames(src, y0, x0, th, tw, mode)
            assert got.is_contiguous() and got.dtype == torch.float32
            assert torch.equal(got, padded[:, :, y0:y0 + th, x0:x0 + tw]), (src.dtype, (y0, x0, th, tw))
    # pad_mode=None: a plain crop; a rectangle that leaves the frame is refused
    assert torch.equal(ops.crop_pad_frames(u8, 1, 2, 7, 4, None), as_float[:, :, 1:8, 2:6])
    with pytest.raises(ValueError):
        ops.crop_pad_frames(u8, 0, 0, H + 1, W, None)
    with pytest.raises(ValueError):
        ops.crop_pad_frames(u8, 0, 0, 2 * H, W, 'reflect')            # beyond the mirror image
    with pytest.raises(ValueError):
        ops.crop_pad_frames(u8, H, 0, 4, 4, 'replicate')              # origin outside the frame
    with pytest.raises(ValueError):
        ops.crop_pad_frames(u8.permute(0, 3, 1, 2), 0, 0, 4, 4, mode)  # uint8 is HWC
    with pytest.raises(NotImplementedError):
        ops.crop_pad_frames(u8.cpu(), 0, 0, 4, 4, mode)


def _as_bytes(x):
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)


# (destination size (Ho, Wo), where the rectangle lands (oy, ox), rectangle in the tile result (ky, kx, kh, kw)); the tile result is 32 x 48
RECTS = [((40, 64), (0, 0), (0, 0, 16, 24)),      # a corner, everything in whole 16-byte groups
         ((40, 64), (8, 16), (16, 0, 16, 48)),    # an edge
         ((40, 64), (4, 12), (8, 12, 20, 28)),    # the interior
         ((37, 61), (3, 5), (8, 12, 20, 28)),     # destination width not a multiple of 4: unaligned stores
         ((37, 61), (5, 2), (3, 5, 22, 31)),      # nothing aligned: the scalar path
         ((32, 48), (0, 0), (0, 0, 32, 48))]      # the whole result


@pytest.mark.parametrize('case', range(len(RECTS)))
def test_rectangle_stores_are_slices_of_the_whole_tile_ops(gpu, case):
    from edvr_amd import ops
    (Ho, Wo), (oy, ox), (ky, kx, kh, kw) = RECTS[case]
    g = torch.Generator().manual_seed(20 + case)
    n, h, w = 2, 8, 12
    base = (torch.randn(n, 3, h, w, generator=g) * 0.8 + 0.5).to(gpu)
    y = (torch.randn(n, 3, 4 * h, 4 * w, generator=g) * 0.5).to(gpu)
    wide = torch.randn(n, 5, 4 * h, 4 * w, generator=g).to(gpu)
    x = wide[:, 1:4]                                                   # an image-strided (n, 3, 32, 48) result (the hr_in tail's input)
    y_before = y.clone()
    full_f = ops.upsample4x_add_(y.clone(), base)
    full_u = ops.upsample4x_add_u8(y, base)
    x_u = ops.f32_to_u8_hwc(x)
    N = n + 2                                                          # the destination holds more images: an image stride of its own
    for name, want, run, u8 in (
            ('upsample4x_add_rect', full_f, lambda d: ops.upsample4x_add_rect(y, base, d, ky, kx), False),
            ('upsample4x_add_u8_rect', full_u, lambda d: ops.upsample4x_add_u8_rect(y, base, d, ky, kx), True),
            ('f32_to_u8_hwc_rect', x_u, lambda d: ops.f32_to_u8_hwc_rect(x, d, ky, kx), True),
            ('copy_rect', x, lambda d: ops.copy_rect(x, d, ky, kx), False)):
        if u8:
            dst = torch.full((N, Ho, Wo, 3), 77, dtype=torch.uint8, device=gpu)
            view, ref = dst[1:1 + n, oy:oy + kh, ox:ox + kw], want[:, ky:ky + kh, kx:kx + kw]
        else:
            dst = torch.full((N, 3, Ho, Wo), 77.0, device=gpu)
            view, ref = dst[1:1 + n, :, oy:oy + kh, ox:ox + kw], want[:, :, ky:ky + kh, kx:kx + kw]
        assert run(view) is view
        assert torch.equal(view, ref), name                            # the kept pixels: exactly what the whole-tile kernel stores
        untouched = torch.ones_like(dst, dtype=torch.bool)
        (untouched[1:1 + n, oy:oy + kh, ox:ox + kw] if u8 else untouched[1:1 + n, :, oy:oy + kh, ox:ox + kw]).fill_(False)
        assert bool((dst[untouched] == 77).all()), name                # ... and nothing else
    assert torch.equal(y, y_before)  # (y is an input here: left as it is)
    with pytest.raises(ValueError):
        ops.upsample4x_add_rect(y, base, torch.empty(n, 3, 4 * h + 4, 8, device=gpu), 0, 0)     # taller than the result
    with pytest.raises(ValueError):
        ops.copy_rect(x, torch.empty(n, 3, 8, 8, device=gpu), 30, 0)                            # reaches below it
    with pytest.raises(ValueError):
        ops.f32_to_u8_hwc_rect(x, torch.empty(n, 3, 8, 8, dtype=torch.uint8, device=gpu))      # CHW bytes
    with pytest.raises(ValueError):
        ops.upsample4x_add_u8_rect(y, base, torch.empty(n, 8, 16, 3, dtype=torch.uint8, device=gpu)[:, :, ::2])  # gaps inside a row


# ------------------------------------------------------------------------------------------------ padding, whole network
@pytest.mark.parametrize('f4s', [True, False])
@pytest.mark.parametrize('name,hw', [('M_T5', (30, 46)), ('L_T7', (30, 46)), ('L_deblur_hr', (56, 72))])
def test_padding_is_the_plain_path_on_host_padded_frames(gpu, name, hw, f4s):
    from edvr_amd import VideoRestorer, ops
    net, kwargs = _net(name)
    net = net.to(gpu)
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    H, W = hw
    lq = _video(9, H, W, seed=3).to(gpu)
    lq8 = _bytes(9, H, W, seed=4).to(gpu)
    prev = ops.set_f4s(inference=f4s)
    try:
        with torch.no_grad():
            for mode in ('reflect', 'replicate'):
                for src, as_float in ((lq, lq), (lq8, ops.frames_u8_to_f32(lq8[None])[0])):
                    padded = _host_pad(as_float, m, mode)
                    for dt in (torch.float32, torch.uint8):
                        want = VideoRestorer(net, chunk=4, out_dtype=dt).restore(padded)
                        want = want[:, :s * H, :s * W] if dt == torch.uint8 else want[..., :s * H, :s * W]
                        vr = VideoRestorer(net, chunk=4, out_dtype=dt, pad_mode=mode)
                        got = vr.restore(src)
                        assert got.is_contiguous() and got.dtype == dt and got.shape == want.shape
                        assert torch.equal(got, want), (name, mode, src.dtype, dt, 'restore')
                        one = torch.stack(list(vr.restore_iter(iter(src.unbind(0)))))
                        assert torch.equal(one, want), (name, mode, src.dtype, dt, 'restore_iter')
                        if mode == 'reflect' and dt == torch.float32:
                            uneven = torch.cat(list(vr.restore_chunks([src[:3], src[3:4], src[4:]])), 0)
                            assert torch.equal(uneven, want), (name, mode, src.dtype, dt, 'restore_chunks')
        torch.cuda.synchronize()
    finally:
        ops.set_f4s(inference=prev[0])


@pytest.mark.parametrize('name,hw', [('M_T5', (30, 46)), ('L_deblur_hr', (56, 72))])
def test_padding_matches_the_oracle_on_every_window(gpu, name, hw):
    from edvr_amd import VideoRestorer, window_table
    from oracle import edvr_oracle as EO
    net, kwargs = _net(name)
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    t, n, (H, W) = kwargs['num_frame'], 9, hw
    lq = _video(n, H, W)
    windows = _host_pad(lq, m, 'reflect')[window_table(n, t, 'reflection_circle').long()]
    with torch.no_grad():
        ref = EO.edvr_forward({k: v.double() for k, v in net.state_dict().items()}, windows.double(), **oracle_kwargs(kwargs))
        ref = ref[..., :s * H, :s * W]
        net = net.to(gpu)
        out = VideoRestorer(net, chunk=4, pad_mode='reflect').restore(lq.to(gpu))
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    gt = torch.rand(ref.shape, generator=torch.Generator().manual_seed(1))
    for i in range(n):
        r = ((out[i].double().cpu() - ref[i]).abs().max() / ref[i].abs().max().clamp_min(1e-30)).item()
        p_ours, p_ref = EO.psnr(out[i:i + 1].cpu(), gt[i:i + 1]), EO.psnr(ref[i:i + 1].float().contiguous(), gt[i:i + 1])
        print(f'{name} frame {i}: rel {r:.2e}, PSNR {p_ours:.5f} vs {p_ref:.5f} dB')
        assert r < INTERMEDIATE_RTOL, (i, r)
        assert abs(p_ours - p_ref) <= PSNR_TOL_DB, (i, p_ours, p_ref)


# ------------------------------------------------------------------------------------------------ tiles, whole network
@pytest.mark.parametrize('f4s', [True, False])
@pytest.mark.parametrize('name,hw,tile,overlap', [('M_T5', (62, 90), (32, 48), 8), ('L_deblur_hr', (120, 136), (64, 80), 32)])
def test_every_kept_rectangle_is_the_plain_path_on_that_tile(gpu, name, hw, tile, overlap, f4s):
    from edvr_amd import VideoRestorer, ops, tile_grid
    net, kwargs = _net(name)
    net = net.to(gpu)
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    H, W = hw
    grid = tile_grid(H, W, tile, overlap, m)
    assert len(grid) == 9  # 3 x 3 tiles after clamping
    lq = _video(9, H, W, seed=5).to(gpu)
    padded = _host_pad(lq, m, 'reflect')
    prev = ops.set_f4s(inference=f4s)
    try:
        with torch.no_grad():
            for dt in (torch.float32, torch.uint8):
                got = VideoRestorer(net, chunk=4, padding='reflection', out_dtype=dt, pad_mode='reflect', tile=tile, tile_overlap=overlap).restore(lq)
                assert tuple(got.shape) == ((9, s * H, s * W, 3) if dt == torch.uint8 else (9, 3, s * H, s * W)) and got.is_contiguous()
                for (y0, x0, th, tw), (ky, kx, kh, kw), (oy, ox) in grid:
                    crop = padded[:, :, y0:y0 + th, x0:x0 + tw].contiguous()
                    want = VideoRestorer(net, chunk=4, padding='reflection', out_dtype=dt).restore(crop)
                    ys, xs = slice(s * ky, s * (ky + kh)), slice(s * kx, s * (kx + kw))
                    yd, xd = slice(s * oy, s * (oy + kh)), slice(s * ox, s * (ox + kw))
                    if dt == torch.uint8:
                        same = torch.equal(got[:, yd, xd], want[:, ys, xs])
                    else:
                        same = torch.equal(got[:, :, yd, xd], want[:, :, ys, xs])
                    assert same, (name, dt, (y0, x0), 'split kernels on' if f4s else 'split kernels off')
            # one tile >= the frame is the padding-only result
            big = VideoRestorer(net, chunk=4, pad_mode='reflect', tile=(_up(H, m) + m, _up(W, m)), tile_overlap=0).restore(lq)
            assert torch.equal(big, VideoRestorer(net, chunk=4, pad_mode='reflect').restore(lq))
        torch.cuda.synchronize()
    finally:
        ops.set_f4s(inference=prev[0])
    net.check_offsets()


def test_tiles_lower_the_peak_memory(gpu):
    from edvr_amd import VideoRestorer, ops, tile_grid
    net, kwargs = _net('M_T5')
    net = net.to(gpu)
    H = W = 256
    tile = (144, 144)  # with the default overlap of 32: 2 x 2 tiles
    assert len(tile_grid(H, W, tile, None, 4)) == 4
    lq = _video(9, H, W, seed=6).to(gpu)
    peaks = {}
    with torch.no_grad():
        for key, kw in (('tiled', {'tile': tile}), ('untiled', {})):
            vr = VideoRestorer(net, chunk=4, out_dtype=torch.uint8, **kw)
            # warm-up with the arm's own launches: weights packed, the grow-only kernel workspaces (ops.workspace) at this arm's size -
            # each arm's figure is what one restore allocates on top of that steady state
            vr.restore(lq)
            ops.reserve_amax_slots(gpu)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = vr.restore(lq)
            torch.cuda.synchronize()
            peaks[key] = torch.cuda.max_memory_allocated() - before
            del out
    net.check_offsets()
    print(f'peak memory of one restore of 9 frames of {H} x {W}, chunk 4: untiled {peaks["untiled"] / 2 ** 20:.1f} MB, 2 x 2 tiles {peaks["tiled"] / 2 ** 20:.1f} MB')
    assert peaks['tiled'] < peaks['untiled'], peaks


def test_validate_video_with_padding(gpu):
    from edvr_amd import VideoRestorer, metrics
    net, kwargs = _net('M_T5')
    net = net.to(gpu)
    H, W = 30, 46
    lq = _video(6, H, W, seed=7).to(gpu)
    gt = torch.rand(6, 3, 4 * H, 4 * W, generator=torch.Generator().manual_seed(8)).to(gpu)
    with torch.no_grad():
        out, psnr = metrics.validate_video(net, lq, gt, num_frame=5, chunk=4, pad_mode='reflect')
        want = VideoRestorer(net, chunk=4, pad_mode='reflect').restore(lq)
        tiled, _ = metrics.validate_video(net, lq, None, num_frame=5, chunk=4, pad_mode='reflect', tile=(16, 32), tile_overlap=8)
    assert tuple(out.shape) == (6, 3, 4 * H, 4 * W) and torch.equal(out, want)
    assert psnr == metrics.calculate_psnr(want[:4], gt[:4], 0, False) + metrics.calculate_psnr(want[4:], gt[4:], 0, False) and len(psnr) == 6
    assert tuple(tiled.shape) == tuple(out.shape) and bool(torch.isfinite(tiled).all())
