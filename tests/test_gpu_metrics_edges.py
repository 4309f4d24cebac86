"""psnr_sse_kernel and ssim_kernel (edvr_amd/csrc/metrics.hip) where such kernels go wrong: rounding ties, tile and block edges, crops, image
strides, structured and non-finite content - against the references of tests/util_metrics.py (checked on the CPU by
tests/test_metrics_refs_cpu.py) and against the reference's own scores in tests/golden/metrics_edges.pt.

Tolerances are the project's (tests/test_metrics.py): RGB sums are integers and compare with ==, RGB PSNR to 1e-12, Y PSNR to 1e-4 dB (the
reference averages in float32), SSIM to 1e-10 (two float64 computations, separable against 2-D window).  The Y sums are also held to
sse_y_ref, the kernel's own definition, at the rounding of a float64 sum of `count` non-negative terms in any order: 2 count 2^-53 relative."""
import math

import pytest
import torch

import util_metrics as UM
from oracle import edvr_oracle as EO

pytestmark = pytest.mark.gpu
_gid = lambda g: '%dx%d_crop%d' % g  # noqa: E731


def _close(a, b, tol):
    return (math.isinf(a) and math.isinf(b)) or abs(a - b) <= tol


def _modes(pred, gt):
    for c, ych in UM.MODES:
        yield c, ych, UM.take_channels(pred, c), UM.take_channels(gt, c)


def _sse(gpu, pred, gt, crop, ych):
    from edvr_amd import metrics
    sse, count = metrics.sum_squared_error_uint8(pred.to(gpu), gt.to(gpu), crop, ych)
    return sse.cpu().tolist(), count


def _ssim(gpu, pred, gt, crop, ych):
    from edvr_amd import metrics
    return metrics.calculate_ssim(pred.to(gpu), gt.to(gpu), crop, ych)


# ------------------------------------------------------------------------------------------------ every geometry x every content
@pytest.mark.parametrize('geom', UM.PSNR_GEOMS, ids=_gid)
def test_psnr_every_geometry_and_content(gpu, geom):
    from edvr_amd import metrics
    h, w, crop = geom
    n, worst_y, worst_db = UM.psnr_n(h, w), 0.0, 0.0
    for kind in UM.psnr_kinds(h, w):
        pair = UM.make_pair(kind, n, 3, h, w)
        for c, ych, pred, gt in _modes(*pair):
            tag = (geom, kind, c, ych)
            got, count = _sse(gpu, pred, gt, crop, ych)
            want, want_count = UM.sse_ref(pred, gt, crop, ych)
            psnr = metrics.calculate_psnr(pred.to(gpu), gt.to(gpu), crop, ych)
            assert count == want_count and len(got) == len(psnr) == n, tag
            for i in range(n):
                ref_db = EO.psnr_cropped(pred[i], gt[i], crop, ych)
                if ych and c == 3:
                    rel = abs(got[i] - want[i]) / want[i] if want[i] else abs(got[i])
                    worst_y, worst_db = max(worst_y, rel), max(worst_db, 0.0 if math.isinf(ref_db) else abs(psnr[i] - ref_db))
                    assert rel <= 2 * count * 2.0 ** -53, (tag, i, got[i], want[i])
                    assert _close(psnr[i], ref_db, 1e-4), (tag, i, psnr[i], ref_db)
                else:
                    assert got[i] == want[i] and got[i] == float(int(got[i])), (tag, i, got[i], want[i])  # integers, exact
                    assert _close(psnr[i], ref_db, 1e-12), (tag, i, psnr[i], ref_db)
                assert psnr[i] == UM.psnr_of(got[i], count), (tag, i)
                if kind == 'identical':
                    assert got[i] == 0.0 and psnr[i] == math.inf, (tag, i, got[i])
            if c == 1 and ych:  # the flag is ignored on one channel, as the reference ignores it
                assert got == _sse(gpu, pred, gt, crop, False)[0], tag
    print('PSNR %dx%d crop %d: Y SSE max rel dev from the float64 reference %.3e, Y PSNR max dev from the oracle %.3e dB' % (h, w, crop, worst_y, worst_db))


@pytest.mark.parametrize('geom', UM.SSIM_GEOMS, ids=_gid)
def test_ssim_every_geometry_and_content(gpu, geom):
    h, w, crop = geom
    worst = (0.0, None)
    for kind in UM.KINDS:
        pair = UM.make_pair(kind, 3, 3, h, w)
        for c, ych, pred, gt in _modes(*pair):
            tag = (geom, kind, c, ych)
            got = _ssim(gpu, pred, gt, crop, ych)
            assert len(got) == 3, tag
            for i in range(3):
                want = EO.ssim_cropped(pred[i], gt[i], crop, ych)
                worst = max(worst, (abs(got[i] - want), tag), key=lambda t: t[0])
                assert abs(got[i] - want) <= 1e-10, (tag, i, got[i], want)
                if kind == 'identical':
                    assert abs(got[i] - 1.0) <= 1e-10, (tag, i, got[i])
            if c == 1 and ych:
                assert got == _ssim(gpu, pred, gt, crop, False), tag  # bit-equal: the flag is ignored on one channel
    ck = UM.make_pair('checker', 3, 3, h, w)[0]
    for c, ych, pred, _ in _modes(ck, ck):
        assert all(abs(v - 1.0) <= 1e-10 for v in _ssim(gpu, pred, pred, crop, ych)), (geom, 'checker against itself', c, ych)
    print('SSIM %dx%d crop %d: max |kernel - oracle| %.3e at %s' % (h, w, crop, worst[0], worst[1]))


def test_ssim_refuses_a_crop_that_leaves_no_window(gpu):
    pred, gt = UM.make_pair('rand', 1, 3, 20, 40)
    with pytest.raises(ValueError):
        _ssim(gpu, pred, gt, 5, False)  # 10 rows left
    assert len(_ssim(gpu, pred, gt, 4, False)) == 1  # 12 rows: a valid region of 2 x 22


# ------------------------------------------------------------------------------------------------ one differing pixel
@pytest.mark.parametrize('ych', (False, True), ids=('rgb', 'y'))
@pytest.mark.parametrize('crop', (0, 3))
def test_psnr_counts_every_pixel_once_and_none_outside_the_crop(gpu, crop, ych):
    """70 x 70 images equal but for ONE pixel: the SSE is that of the 1 x 1 image pair holding the two pixels, bit for bit (one non-zero term,
    no rounding), or exactly 0 where the pixel lies outside the crop.  The positions sit on the 256-pixel turns and the two blocks' ends."""
    h = w = 70
    if crop == 0:
        spots = [divmod(p, w) for p in (0, 255, 256, 4095, 4096, 4899)]
        inside = [True] * 6
    else:
        spots = [(3, 3), (66, 66), (2, 3), (3, 2), (67, 66), (66, 67)]
        inside = [True, True, False, False, False, False]
    base = UM.make_pair('rand', 1, 3, h, w)[0]
    pred = base.expand(len(spots), 3, h, w).contiguous()
    gt = pred.clone()
    for j, (y, x) in enumerate(spots):
        gt[j, :, y, x] = (pred[j, :, y, x] + 0.5) % 1.0
    got, count = _sse(gpu, pred, gt, crop, ych)
    assert count == (h - 2 * crop) ** 2 * (1 if ych else 3)
    for j, (y, x) in enumerate(spots):
        alone, _ = _sse(gpu, pred[j:j + 1, :, y:y + 1, x:x + 1].contiguous(), gt[j:j + 1, :, y:y + 1, x:x + 1].contiguous(), 0, ych)
        assert alone[0] > 0, (spots[j], alone)
        if not ych:
            assert alone == UM.sse_ref(pred[j:j + 1, :, y:y + 1, x:x + 1], gt[j:j + 1, :, y:y + 1, x:x + 1], 0, False)[0], (spots[j], alone)
        assert got[j] == (alone[0] if inside[j] else 0.0), (crop, ych, spots[j], got[j], alone[0])


def test_ssim_sees_one_pixel_on_tile_seams_and_corners(gpu):
    """58 x 75 (3 x 5 tiles, the last column one pixel wide): pred = gt but for one pixel forced to 0 or 1, at the image corners, on both
    sides of a tile seam, in the last tile column and next to it"""
    h, w = 58, 75
    spots = [(0, 0), (57, 74)] + [(y + 5, x + 5) for y, x in ((15, 15), (16, 16), (47, 64), (31, 63))]
    gt = UM.make_pair('ramp_noise', 1, 3, h, w)[1].expand(len(spots), 3, h, w).contiguous()
    pred = gt.clone()
    for j, (y, x) in enumerate(spots):
        pred[j, :, y, x] = (gt[j, :, y, x] < 0.5).float()
    worst = 0.0
    for c, ych, p, g in _modes(pred, gt):
        got = _ssim(gpu, p, g, 0, ych)
        for j in range(len(spots)):
            want = EO.ssim_cropped(p[j], g[j], 0, ych)
            assert want < 1.0 and abs(got[j] - want) <= 1e-10, (spots[j], c, ych, got[j], want)
            worst = max(worst, abs(got[j] - want))
    print('SSIM one pixel at 58x75: max |kernel - oracle| %.3e' % worst)


# ------------------------------------------------------------------------------------------------ what the kernels must not depend on
@pytest.mark.parametrize('geom', ((40, 44, 7), (70, 70, 30)), ids=_gid)
def test_pixels_outside_the_crop_are_not_read(gpu, geom):
    """two pairs that agree inside the crop and differ arbitrarily outside it score bit-equal (SSIM where the crop leaves a window)"""
    h, w, crop = geom
    a, b = UM.make_pair('wide', 3, 3, h, w), UM.make_pair('wide', 3, 3, h, w, salt=1)
    for t, u in zip(a, b):
        assert not torch.equal(t, u)
        u[:, :, crop:h - crop, crop:w - crop] = t[:, :, crop:h - crop, crop:w - crop]
        assert not torch.equal(t, u)
    for (c, ych, p0, g0), (_, _, p1, g1) in zip(_modes(*a), _modes(*b)):
        assert _sse(gpu, p0, g0, crop, ych) == _sse(gpu, p1, g1, crop, ych), (geom, c, ych)
        if UM.ssim_tiles(h, w, crop)[0] > 0:
            assert _ssim(gpu, p0, g0, crop, ych) == _ssim(gpu, p1, g1, crop, ych), (geom, c, ych)
    assert UM.ssim_tiles(40, 44, 7)[0] > 0


@pytest.mark.parametrize('kind', ('rand', 'wide'))
def test_images_of_a_batch_score_as_they_do_alone_and_twice_the_same(gpu, kind):
    for metric, geoms in ((_sse, ((64, 65, 0), (70, 70, 30))), (_ssim, ((58, 75, 0), (40, 44, 7)))):
        for h, w, crop in geoms:
            for c, ych, pred, gt in _modes(*UM.make_pair(kind, 3, 3, h, w)):
                got = metric(gpu, pred, gt, crop, ych)
                assert got == metric(gpu, pred, gt, crop, ych), (metric.__name__, h, w, crop, c, ych)
                values = got[0] if metric is _sse else got
                for i in range(3):
                    one = metric(gpu, pred[i:i + 1], gt[i:i + 1], crop, ych)
                    assert (one[0] if metric is _sse else one) == [values[i]], (metric.__name__, h, w, crop, c, ych, i)


# ------------------------------------------------------------------------------------------------ the C entry points, called directly
def _direct_sse(a, b, n, c, h, w, a_stride, b_stride, crop, y):
    """edvr_psnr_sse_f32 as sum_squared_error_uint8 calls it, but with the caller's image strides; the partials start as NaN, so a block
    that wrote nothing shows.  Returns the partials on the device."""
    from edvr_amd import _lib
    blocks = UM.psnr_blocks(h, w)
    partial = torch.full((n, blocks), math.nan, dtype=torch.float64, device=a.device)
    _lib.check(_lib.lib().edvr_psnr_sse_f32(a.data_ptr(), b.data_ptr(), partial.data_ptr(), n, c, h, w, a_stride, b_stride, crop, y, blocks,
                                            torch.cuda.current_stream(a.device).cuda_stream), 'edvr_psnr_sse_f32')
    return partial


def _direct_ssim(a, b, n, c, h, w, a_stride, b_stride, crop, y):
    from edvr_amd import _lib
    L = _lib.lib()
    tiles = L.edvr_ssim_partials(h, w, crop)
    assert tiles == UM.ssim_tiles(h, w, crop)[2] * UM.ssim_tiles(h, w, crop)[3]
    partial = torch.full((n, 1 if y else c, tiles), math.nan, dtype=torch.float64, device=a.device)
    _lib.check(L.edvr_ssim_f32(a.data_ptr(), b.data_ptr(), partial.data_ptr(), n, c, h, w, a_stride, b_stride, crop, y,
                               torch.cuda.current_stream(a.device).cuda_stream), 'edvr_ssim_f32')
    return partial


def test_idle_psnr_block_writes_an_exact_zero(gpu):
    """70 x 70 with crop 30: the grid has two blocks (sized from 4900 pixels), all 100 pixels go to block 0"""
    h, w, crop, n = 70, 70, 30, 3
    assert UM.psnr_block_pixels(h, w, crop).tolist() == [100, 0]
    for kind in ('wide', 'black_white'):
        for c, ych, pred, gt in _modes(*UM.make_pair(kind, n, 3, h, w)):
            y = 1 if (ych and c == 3) else 0
            part = _direct_sse(pred.to(gpu), gt.to(gpu), n, c, h, w, c * h * w, c * h * w, crop, y)
            part = part.cpu()
            assert part[:, 1].tolist() == [0.0] * n and part[:, 0].tolist() == _sse(gpu, pred, gt, crop, ych)[0], (kind, c, ych, part)
            if not y:
                assert part[:, 0].tolist() == UM.sse_ref(pred, gt, crop, ych)[0], (kind, c, ych, part)


@pytest.mark.parametrize('y', (0, 1), ids=('rgb', 'y'))
def test_image_strides(gpu, y):
    """pred = channels 1..3 of a 6-channel tensor, gt = channels 0..2 of a 5-channel one: image strides of 6 h w and 5 h w, the other channels
    full of values that would show; bit-equal to the contiguous call.  The wrappers of metrics.py always copy, so this calls the library."""
    n = 3
    for fn, (h, w, crop) in ((_direct_sse, (64, 65, 0)), (_direct_ssim, (27, 42, 0))):
        pred, gt = UM.make_pair('rand', n, 3, h, w)
        big, big2 = UM.make_pair('wide', n, 6, h, w, salt=2)[0].to(gpu), UM.make_pair('wide', n, 5, h, w, salt=3)[0].to(gpu)
        big[:, 1:4], big2[:, 0:3] = pred.to(gpu), gt.to(gpu)
        a, b = big[:, 1:4], big2[:, 0:3]
        assert a.stride() == (6 * h * w, h * w, w, 1) and b.stride() == (5 * h * w, h * w, w, 1) and a.data_ptr() == big.data_ptr() + 4 * h * w
        got = fn(a, b, n, 3, h, w, a.stride(0), b.stride(0), crop, y)
        want = fn(pred.to(gpu), gt.to(gpu), n, 3, h, w, 3 * h * w, 3 * h * w, crop, y)
        assert not torch.isnan(want).any() and torch.equal(got, want), (fn.__name__, y)
        assert torch.equal(want, fn(pred.to(gpu), gt.to(gpu), n, 3, h, w, 0, 0, crop, y))  # stride 0 = contiguous
        if fn is _direct_sse:
            assert want.sum(1).tolist() == _sse(gpu, pred, gt, crop, bool(y))[0]
        else:
            count = UM.ssim_tiles(h, w, crop)[0] * UM.ssim_tiles(h, w, crop)[1]
            assert (want.sum(2) / count).mean(1).tolist() == _ssim(gpu, pred, gt, crop, bool(y))


def test_validate_clip_passes_crop_and_y_channel_through(gpu):
    from util_edvr import build
    from edvr_amd import metrics
    net, _, _ = build('M_T5')
    net = net.to(gpu).eval()
    g = torch.Generator().manual_seed(11)
    lq = torch.rand(7, 3, 16, 24, generator=g)
    gt = torch.rand(7, 3, 64, 96, generator=g).to(gpu)
    outs, scores = metrics.validate_clip(net, lq.to(gpu), gt, num_frame=5, padding='reflection_circle', batch=3, crop_border=3, test_y_channel=True)
    assert len(scores) == 7
    for i in range(7):
        assert [scores[i]] == metrics.calculate_psnr(outs[i:i + 1], gt[i:i + 1], 3, True), i
    assert scores == metrics.calculate_psnr(outs, gt, 3, True) and scores != metrics.calculate_psnr(outs, gt) and scores != metrics.calculate_psnr(outs, gt, 3)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_kernels_reproduce_the_reference_on_edge_contents(gpu):
    """tests/golden/metrics_edges.pt: the reference's own tensor2img, calculate_psnr and calculate_ssim on ties, wide, inf and const"""
    from edvr_amd import metrics
    worst = 0.0
    for case in UM.load_golden():
        pred, gt, crop = case['pred'].to(gpu), case['gt'].to(gpu), case['crop_border']
        for ych in (False, True):
            tag = (case['kind'], case['h'], case['w'], crop, ych)
            psnr, ssim = metrics.calculate_psnr(pred, gt, crop, ych)[0], metrics.calculate_ssim(pred, gt, crop, ych)[0]
            assert _close(psnr, case['psnr'][ych], 1e-4 if ych else 1e-12), (tag, psnr, case['psnr'][ych])
            assert abs(ssim - case['ssim'][ych]) <= 1e-10, (tag, ssim, case['ssim'][ych])
            worst = max(worst, abs(ssim - case['ssim'][ych]))
    print('SSIM against the reference on edge contents: max |kernel - reference| %.3e' % worst)
