"""-m gpu: blended tile seams on the whole-video path (edvr_amd/video.py: tile_blend; csrc/ensemble.hip: the `*_rect_blend` tails) - the
tails launch by launch against the torch expression of the definition, the whole network against each tile's crop restored by the plain
path and blended on the device by the definition.  Everything is compared with torch.equal: the definition fixes every rounding."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from util_edvr import CONFIGS, randomize_offsets

pytestmark = pytest.mark.gpu


def _up(v, m):
    return (v + m - 1) // m * m


def _ramp(B):
    """r(j) on the HOST (IEEE float32 division), j = 0 ... B - 1."""
    return (2 * torch.arange(B, dtype=torch.float32) + 1) / torch.tensor(float(2 * B), dtype=torch.float32)


def _axis(n, lo, hi):
    """-> (weights (n,), in a low band (n,), in a high band (n,)) of an extended length n with bands lo / hi (output pixels)."""
    w = torch.ones(n, dtype=torch.float32)
    low, high = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    if lo:
        w[:lo], low[:lo] = _ramp(lo), True
    if hi:
        w[n - hi:], high[n - hi:] = 1.0 - _ramp(hi), True
    return w, low, high


def _weights(kh, kw, bands, device):
    """-> w (kh, kw) float32 = w_y * w_x, first (no low band), last (no high band) of a rectangle."""
    wy, ly, hy = _axis(kh, bands[0], bands[1])
    wx, lx, hx = _axis(kw, bands[2], bands[3])
    w = wy[:, None] * wx[None, :]
    return w.to(device), (~(ly[:, None] | lx[None, :])).to(device), (~(hy[:, None] | hx[None, :])).to(device)


def _contribute(pre, v, bands, mode, scale):
    """What one launch leaves in the float32 accumulator rectangle `pre` (the definition, one torch kernel per rounding), and the mask
    of the pixels it is the last contributor of."""
    w, first, last = _weights(v.shape[-2], v.shape[-1], bands, v.device)
    p = torch.mul(w, v)
    s = torch.where(first & (mode in ('first', 'only')), p, torch.add(pre, p))
    done = last & (mode in ('last', 'only'))
    return torch.where(done, torch.mul(s, scale), s), done


# ------------------------------------------------------------------------------------------------ the tails
# (ky, kx, kh, kw) inside a 48 x 48 corner (the result is 48 x 80 or, transposed, 80 x 48), B, ((Ho, Wo), (oy, ox)) of the destination view
TAIL_RECTS = [((8, 12, 24, 28), 8, ((56, 64), (4, 8))),    # everything in whole 16-byte groups: the wide path
              ((8, 12, 24, 28), 8, ((53, 61), (3, 5))),    # wide loads of y, an accumulator that is not 16-byte aligned
              ((3, 5, 22, 31), 8, ((53, 61), (3, 5))),     # odd origin and width: the scalar path
              ((8, 12, 24, 28), 6, ((56, 64), (4, 8))),    # bands that split a group of 4: the scalar path
              ((0, 0, 48, 48), 24, ((56, 64), (4, 8)))]    # more than one 32 x 32 tile of the transposing kernels; bands that meet
BAND_SIDES = [(0, 0), (0, 1), (1, 0), (1, 1)]              # (low, high) of an axis
MODES = ['first', 'middle', 'last', 'only']


@pytest.mark.parametrize('up', [True, False])
@pytest.mark.parametrize('k', range(8))
def test_blend_tails_are_the_definition(gpu, k, up):
    from edvr_amd import ops
    n, N, scale = 2, 4, 1.0 / 3
    g = torch.Generator().manual_seed(70 + k)
    if up:  # y 12 x 20 (x 4: a 48 x 80 result), in the tile's own orientation
        base = (torch.randn(n, 3, 12, 20, generator=g) * 0.8 + 0.5).to(gpu)
        y = (torch.randn(n, 3, 48, 80, generator=g) * 0.5).to(gpu)
        full = ops.upsample4x_add_(y.clone(), base)
    else:   # an image-strided 48 x 80 result (the hr_in tail's input)
        y = (torch.randn(n, 5, 48, 80, generator=g) * 0.6 + 0.5).to(gpu)[:, 1:4]
        base, full = None, y
    back = ops.d4_invert(full, k)                                      # the plain tail's values in the frame's orientation
    for (ky, kx, kh, kw), B, ((Ho, Wo), (oy, ox)) in TAIL_RECTS:
        v = back[:, :, ky:ky + kh, kx:kx + kw]
        fill = torch.randn(N, 3, Ho, Wo, generator=g).to(gpu)          # what earlier contributors left; the rest must stay
        inside = torch.zeros(N, 3, Ho, Wo, dtype=torch.bool, device=gpu)
        inside[1:1 + n, :, oy:oy + kh, ox:ox + kw] = True
        for (yl, yh), (xl, xh), mode in itertools.product(BAND_SIDES, BAND_SIDES, MODES):
            bands = (B * yl, B * yh, B * xl, B * xh)
            what = (k, up, (ky, kx, kh, kw), bands, mode)
            want, done = _contribute(fill[1:1 + n, :, oy:oy + kh, ox:ox + kw], v, bands, mode, scale)
            # float32 output: the accumulator is the output
            dst = fill.clone()
            view = dst[1:1 + n, :, oy:oy + kh, ox:ox + kw]
            got = (ops.upsample4x_add_rect_blend(y, base, view, ky, kx, bands, k, mode, scale) if up
                   else ops.copy_rect_blend(y, view, ky, kx, bands, k, mode, scale))
            assert got is view
            assert torch.equal(view, want), what + ('float32',)
            assert torch.equal(dst[~inside], fill[~inside]), what
            # uint8 output: a pixel's last contributor stores bytes, every other one the float32 accumulator
            scratch = fill.clone()
            out = torch.full((N, Ho, Wo, 3), 77, dtype=torch.uint8, device=gpu)
            a_view, o_view = scratch[1:1 + n, :, oy:oy + kh, ox:ox + kw], out[1:1 + n, oy:oy + kh, ox:ox + kw]
            if up:
                ops.upsample4x_add_u8_rect_blend(y, base, o_view, a_view, ky, kx, bands, k, mode, scale)
            else:
                ops.f32_to_u8_hwc_rect_blend(y, o_view, a_view, ky, kx, bands, k, mode, scale)
            want_u8 = torch.where(done[None, :, :, None], ops.f32_to_u8_hwc(want.contiguous()), torch.full_like(o_view, 77))
            assert torch.equal(o_view, want_u8), what + ('uint8',)
            assert torch.equal(a_view[:, :, ~done], want[:, :, ~done]), what + ('accumulator',)
            assert bool((out[~inside.permute(0, 2, 3, 1)] == 77).all()) and torch.equal(scratch[~inside], fill[~inside]), what
    # argument checks in the style of the *_rect_d4 ones
    view = torch.empty(n, 3, 24, 28, device=gpu)
    tail = (lambda *a: ops.upsample4x_add_rect_blend(y, base, view, 8, 12, *a)) if up else (lambda *a: ops.copy_rect_blend(y, view, 8, 12, *a))
    for bad in ((8, 0, 4, 0), (16, 16, 0, 0), (8, 0, 0), (-8, 0, 0, 0), (8.0, 0, 0, 0)):  # two widths, overlapping, three, negative, float
        with pytest.raises(ValueError):
            tail(bad, k, 'only', 1.0)
    with pytest.raises(ValueError):
        tail((8, 0, 0, 0), k, 'sum', 1.0)
    with pytest.raises(ValueError):
        tail((8, 0, 0, 0), 8, 'only', 1.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ whole path
def _g(x, k):
    from edvr_amd import ops
    return ops.d4_apply(x, k)


# name, (H, W), tile, overlap (= tile_blend): the two cases of test_every_kept_rectangle_is_the_plain_path_on_that_tile
CASES = {'M_62x90': ('M_T5', (62, 90), (32, 48), 8),
         'L_deblur_hr_120x136': ('L_deblur_hr', (120, 136), (64, 80), 32)}
FRAMES, CHUNK = 7, 4        # a chunk boundary and the temporal padding are both crossed
_NETS, _PLAIN = {}, {}      # the networks and the per-(tile, element) references R(g_k(crop)) are computed once and shared


def _case(case, gpu, lq=None):
    from edvr_amd import EDVR, tile_bands, tile_grid
    name, (H, W), tile, overlap = CASES[case]
    if name not in _NETS:
        kwargs, _ = CONFIGS[name]
        torch.manual_seed(10)
        _NETS[name] = (randomize_offsets(EDVR(**kwargs)).eval().to(gpu), kwargs)
    net, kwargs = _NETS[name]
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    if lq is None:
        lq = torch.rand(FRAMES, 3, H, W, generator=torch.Generator().manual_seed(5)).to(gpu)
    padded = F.pad(lq, (0, _up(W, m) - W, 0, _up(H, m) - H), mode='reflect')
    grid, blend = tile_grid(H, W, tile, overlap, m), tile_bands(H, W, tile, overlap, overlap, m)
    assert len(grid) == 9 and len(blend) == 9
    return net, m, s, lq, padded, grid, blend, dict(pad_mode='reflect', tile=tile, tile_overlap=overlap, tile_blend=overlap)


def _definition(case, gpu, f4s, elements=None, lq=None, key=None):
    """The definition with the plain VideoRestorer: every tile's crop (under every element) restored on its own, then over the work
    list (tiles row-major, element innermost) acc = w * v / acc = acc + w * v per pixel, the last contributor times 1 / n with an
    ensemble - float32 (FRAMES, 3, s H, s W).  Starts from NaN: a pixel without a first contributor shows."""
    from edvr_amd import VideoRestorer
    net, m, s, _, padded, grid, blend, _ = _case(case, gpu, lq)
    H, W = CASES[case][1]
    acc = torch.full((FRAMES, 3, s * H, s * W), float('nan'), device=gpu)
    ks = elements or (0,)
    for ti, (tile, tb) in enumerate(zip(grid, blend)):
        y0, x0, th, tw = tile.src
        crop = padded[:, :, y0:y0 + th, x0:x0 + tw]
        (ey, ex, eh, ew), (oy, ox) = tb.ext, tb.dst
        assert (oy, ox) == (y0 + ey, x0 + ex)
        for e, k in enumerate(ks):
            ck = (case, key, f4s, ti, k)
            if ck not in _PLAIN:
                from edvr_amd import ops
                _PLAIN[ck] = ops.d4_invert(VideoRestorer(net, chunk=CHUNK).restore(_g(crop, k).contiguous()), k)
            v = _PLAIN[ck][:, :, s * ey:s * (ey + eh), s * ex:s * (ex + ew)]
            ys, xs = slice(s * oy, s * (oy + eh)), slice(s * ox, s * (ox + ew))
            mode = 'only' if len(ks) == 1 else 'first' if e == 0 else 'last' if e == len(ks) - 1 else 'middle'
            acc[:, :, ys, xs], _ = _contribute(acc[:, :, ys, xs], v, tuple(s * b for b in tb.bands), mode, 1.0 / len(ks) if elements else 1.0)
    assert bool(torch.isfinite(acc).all())
    return acc


def _band_mask(case, gpu):
    net, m, s, _, _, grid, blend, _ = _case(case, gpu)
    H, W = CASES[case][1]
    band = torch.zeros(s * H, s * W, dtype=torch.bool, device=gpu)
    b = CASES[case][3]
    for t in grid:
        oy, ox = t.dst
        if oy > 0:
            band[s * (oy - b // 2):s * (oy + b // 2)] = True
        if ox > 0:
            band[:, s * (ox - b // 2):s * (ox + b // 2)] = True
    return band


@pytest.mark.parametrize('f4s', [True, False])
@pytest.mark.parametrize('case', sorted(CASES))
def test_blended_tiles_are_the_definition(gpu, case, f4s):
    from edvr_amd import VideoRestorer, ops
    net, m, s, lq, _, grid, _, kw = _case(case, gpu)
    H, W = CASES[case][1]
    prev = ops.set_f4s(inference=f4s)
    try:
        with torch.no_grad():
            want = _definition(case, gpu, f4s)
            got = VideoRestorer(net, chunk=CHUNK, **kw).restore(lq)
            assert got.is_contiguous() and got.dtype == torch.float32 and tuple(got.shape) == (FRAMES, 3, s * H, s * W)
            assert torch.equal(got, want), (case, 'float32')
            got8 = VideoRestorer(net, chunk=CHUNK, out_dtype=torch.uint8, **kw).restore(lq)
            assert got8.is_contiguous() and tuple(got8.shape) == (FRAMES, s * H, s * W, 3)
            assert torch.equal(got8, ops.f32_to_u8_hwc(want)), (case, 'uint8')
            # outside the bands: bit for bit the unblended tiled result (a multiply by 1.0f is exact); inside, the tiles differ
            cut = VideoRestorer(net, chunk=CHUNK, **{**kw, 'tile_blend': None}).restore(lq)
            band = _band_mask(case, gpu)
            assert torch.equal(got[..., ~band], cut[..., ~band]) and not torch.equal(got[..., band], cut[..., band])
        torch.cuda.synchronize()
    finally:
        ops.set_f4s(inference=prev[0])
    net.check_offsets()


@pytest.mark.parametrize('ensemble', ['flip4', 'seq_0_5'])
def test_blending_composes_with_self_ensemble(gpu, ensemble):
    from edvr_amd import VideoRestorer, ops
    case = 'M_62x90'
    elements, arg = ((0, 1, 2, 3), 'flip4') if ensemble == 'flip4' else ((0, 5), (0, 5))
    net, m, s, lq, _, grid, _, kw = _case(case, gpu)
    with torch.no_grad():
        want = _definition(case, gpu, ops.F4S_INFERENCE, elements)
        vr = VideoRestorer(net, chunk=CHUNK, self_ensemble=arg, **kw)
        assert torch.equal(vr.restore(lq), want), (ensemble, 'float32')
        assert len(vr.pairs) == len(grid) * len(elements)
        got8 = VideoRestorer(net, chunk=CHUNK, out_dtype=torch.uint8, self_ensemble=arg, **kw).restore(lq)
        assert torch.equal(got8, ops.f32_to_u8_hwc(want)), (ensemble, 'uint8')
    torch.cuda.synchronize()
    net.check_offsets()


def test_streaming_uint8_frames_equals_restore(gpu):
    from edvr_amd import VideoRestorer, ops
    case = 'M_62x90'
    H, W = CASES[case][1]
    lq8 = torch.randint(0, 256, (FRAMES, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(gpu)
    net, m, s, _, _, grid, _, kw = _case(case, gpu)
    with torch.no_grad():
        want = _definition(case, gpu, ops.F4S_INFERENCE, lq=ops.frames_u8_to_f32(lq8[None])[0], key='bytes')
        vr = VideoRestorer(net, chunk=CHUNK, out_dtype=torch.uint8, **kw)
        whole = vr.restore(lq8)
        assert torch.equal(whole, ops.f32_to_u8_hwc(want))
        frames = list(vr.restore_iter(iter(lq8.unbind(0))))            # frame by frame
        assert torch.equal(torch.stack(frames), whole)
    torch.cuda.synchronize()
    net.check_offsets()


def test_validate_video_with_tile_blend(gpu):
    from edvr_amd import VideoRestorer, metrics
    case = 'M_62x90'
    net, m, s, lq, _, _, _, kw = _case(case, gpu)
    H, W = CASES[case][1]
    gt = torch.rand(FRAMES, 3, s * H, s * W, generator=torch.Generator().manual_seed(8)).to(gpu)
    with torch.no_grad():
        out, psnr = metrics.validate_video(net, lq, gt, num_frame=5, chunk=CHUNK, **kw)
        want = VideoRestorer(net, chunk=CHUNK, **kw).restore(lq)
        cut, _ = metrics.validate_video(net, lq, gt, num_frame=5, chunk=CHUNK, **{**kw, 'tile_blend': None})
    assert torch.equal(out, want) and not torch.equal(out, cut)
    assert psnr == metrics.calculate_psnr(want[:CHUNK], gt[:CHUNK], 0, False) + metrics.calculate_psnr(want[CHUNK:], gt[CHUNK:], 0, False)
    assert len(psnr) == FRAMES


def test_geometry_error_comes_at_the_first_frame(gpu):
    from edvr_amd import VideoRestorer
    net, _, _, _, _, _, _, _ = _case('M_62x90', gpu)
    vr = VideoRestorer(net, chunk=CHUNK, tile=(32, 32), tile_overlap=16, tile_blend=16)   # accepted: the frame decides
    lq = torch.rand(FRAMES, 3, 52, 52, generator=torch.Generator().manual_seed(1)).to(gpu)
    with torch.no_grad(), pytest.raises(ValueError, match='tile_blend 16'):
        vr.restore(lq)
