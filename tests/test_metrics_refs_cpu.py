"""The references and case tables of tests/util_metrics.py, checked on the CPU before tests/test_gpu_metrics_edges.py holds the PSNR / SSIM
kernels to them: they reproduce the reference's own scores (tests/golden/psnr.pt, ssim.pt and metrics_edges.pt), every content kind has the
property it is named for, every geometry reaches the kernel path its comment names, and the kernel's SSIM algorithm (separable, float64)
agrees with the 2-D window of the oracle far inside the 1e-10 the GPU tests allow."""
import math
import os

import numpy as np
import pytest
import torch

import util_metrics as UM
from oracle import edvr_oracle as EO

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
F32 = np.float32


def _close(a, b, tol):
    return (math.isinf(a) and math.isinf(b)) or abs(a - b) <= tol


def _bytes(t):
    return EO.tensor2img_uint8(t).numpy().astype(np.int64)


def test_references_reproduce_the_goldens_of_test_metrics():
    """sse_rgb_ref / sse_y_ref as dB and ssim_cropped / ssim_separable against psnr.pt and ssim.pt, at the tolerances of tests/test_metrics.py"""
    d, s = torch.load(os.path.join(GOLD, 'psnr.pt')), torch.load(os.path.join(GOLD, 'ssim.pt'))
    for case in d['cases']:
        pred, gt = (d['pred'][:, :1], d['gt'][:, :1]) if case['gray'] else (d['pred'], d['gt'])
        sse, count = UM.sse_ref(pred, gt, case['crop_border'], case['test_y_channel'])
        for i, want in enumerate(case['psnr']):
            assert _close(UM.psnr_of(sse[i], count), want, 1e-4 if case['test_y_channel'] else 1e-12), (case, i, sse[i], count)
    for case in s['cases']:
        pred, gt = (d['pred'][:, :1], d['gt'][:, :1]) if case['gray'] else (d['pred'], d['gt'])
        for i, want in enumerate(case['ssim']):
            for fn in (EO.ssim_cropped, UM.ssim_separable):
                assert abs(fn(pred[i], gt[i], case['crop_border'], case['test_y_channel']) - want) <= 1e-12, (case, i, fn.__name__)


def test_golden_of_the_reference_is_reproduced():
    """metrics_edges.pt (the reference's own tensor2img, calculate_psnr and calculate_ssim on ties / wide / inf / const): RGB PSNR exact to
    1e-12, Y PSNR to 1e-4 dB (the reference averages in float32), SSIM to 1e-12; the file holds the very tensors the builders give"""
    cases = UM.load_golden()
    assert [(c['kind'], c['h'], c['w'], c['crop_border']) for c in cases] == list(UM.GOLDEN_CASES) and len(cases) == 7
    assert os.path.getsize(UM.GOLDEN) < 200 * 1000
    for case in cases:
        pred, gt, crop = case['pred'], case['gt'], case['crop_border']
        built = UM.make_pair(case['kind'], 1, 3, case['h'], case['w'])
        assert torch.equal(pred, built[0]) and torch.equal(gt, built[1]), case['kind']
        for ych in (False, True):
            sse, count = UM.sse_ref(pred, gt, crop, ych)
            assert _close(UM.psnr_of(sse[0], count), case['psnr'][ych], 1e-4 if ych else 1e-12), (case['kind'], crop, ych, sse, count)
            assert _close(EO.psnr_cropped(pred[0], gt[0], crop, ych), case['psnr'][ych], 1e-4 if ych else 1e-12), (case['kind'], crop, ych)
            for fn in (EO.ssim_cropped, UM.ssim_separable):
                assert abs(fn(pred[0], gt[0], crop, ych) - case['ssim'][ych]) <= 1e-12, (case['kind'], crop, ych, fn.__name__)


def test_ties_are_exact_halves_that_round_to_even():
    allk = UM.ties_from_k(np.arange(255))
    x = allk * F32(255.0)
    assert x.dtype == F32 and np.array_equal(x, np.arange(255, dtype=F32) + F32(0.5))  # all 255 values, exactly k + 0.5 in float32
    want = np.arange(255) + (np.arange(255) % 2)  # the even neighbour
    assert np.array_equal(_bytes(torch.from_numpy(allk)), want)
    for t in UM.make_pair('ties', 3, 3, 27, 42):
        x = t.numpy() * F32(255.0)
        assert np.array_equal(x - np.floor(x), np.full(x.shape, 0.5, F32))
        b = _bytes(t)
        assert (b % 2 == 0).all() and np.array_equal(np.abs(b - x.astype(np.float64)), np.full(x.shape, 0.5))
        assert len(np.unique(np.floor(x))) > 200 and (np.floor(x) % 2 == 1).any() and (np.floor(x) % 2 == 0).any()  # halves that go up and down
        assert (np.floor(x + F32(0.5)) != b).any()  # round-half-away-from-zero would give other bytes


def test_content_kinds_have_their_properties():
    n, c, h, w = 3, 3, 27, 42
    pred, gt = UM.make_pair('identical', n, c, h, w)
    assert np.array_equal(_bytes(pred), _bytes(gt)) and bool((pred != gt).all())  # equal bytes, unequal floats
    assert len(np.unique(_bytes(pred))) == 256
    assert UM.sse_ref(pred, gt, 0, False)[0] == [0.0] * n and UM.sse_ref(pred, gt, 0, True)[0] == [0.0] * n
    assert UM.psnr_of(0.0, 1) == math.inf and EO.ssim_cropped(pred[0], gt[0]) == 1.0
    for t in UM.make_pair('wide', n, c, h, w):  # clamps on both sides, about half the pixels in all
        lo, hi = (t < 0).float().mean().item(), (t > 1).float().mean().item()
        assert lo > 0.2 and hi > 0.2 and 0.4 < lo + hi < 0.9, (lo, hi)
    for kind in ('checker', 'checker_inv'):  # saturated: bytes 0 and 255 only, alternating
        pred, gt = UM.make_pair(kind, n, c, h, w)
        for t in (pred, gt):
            assert set(np.unique(_bytes(t))) == {0, 255}
        b = _bytes(pred)
        assert (b[..., 1:] != b[..., :-1]).all() and (b[..., 1:, :] != b[..., :-1, :]).all()
    pred, gt = UM.make_pair('checker_inv', n, c, h, w)
    assert (np.abs(_bytes(pred) - _bytes(gt)) == 255).all()
    pred, gt = UM.make_pair('checker', n, c, h, w)
    same = _bytes(pred) == _bytes(gt)  # shifted right / down / diagonally with the edge replicated: channels differ in where they agree
    assert same[:, 0, :, 0].all() and not same[:, 0, :, 1:].any()
    assert same[:, 1, 0].all() and not same[:, 1, 1:].any()
    assert same[:, 2, 1:, 1:].all() and same[:, 2, 0, 0].all() and not same[:, 2, 0, 1:].any() and not same[:, 2, 1:, 0].any()
    pred, gt = UM.make_pair('const', n, c, h, w)
    assert (_bytes(pred) == 255).all() and (_bytes(gt) == 128).all()
    pred, gt = UM.make_pair('black_white', n, c, h, w)
    assert (_bytes(pred) == 0).all() and (_bytes(gt) == 255).all()
    assert UM.sse_rgb_ref(pred, gt).tolist() == [65025 * c * h * w] * n
    pred, gt = UM.make_pair('inf', n, c, h, w)
    assert (pred == math.inf).sum().item() == n and (pred == -math.inf).sum().item() == n and bool(torch.isfinite(gt).all())
    assert (_bytes(pred)[pred.numpy() == math.inf] == 255).all() and (_bytes(pred)[pred.numpy() == -math.inf] == 0).all()
    assert (pred == math.inf).nonzero()[:, 1].tolist() == [0] * n and (pred == -math.inf).nonzero()[:, 1].tolist() == [c - 1] * n
    for hh, ww, crop in UM.SSIM_GEOMS + UM.PSNR_GEOMS[2:5]:  # both pixels lie inside the crop wherever the crop leaves more than one
        yy, xx = UM.make_pair('inf', 1, 3, hh, ww)[0].isinf().nonzero()[:, 2:].T
        assert len(yy) == 2 and bool(((yy >= crop) & (yy < hh - crop) & (xx >= crop) & (xx < ww - crop)).all()), (hh, ww, crop)
    pred, gt = UM.make_pair('inf', n, 1, 1, 1)  # a single value: +inf only
    assert (pred == math.inf).all()
    pred, gt = UM.make_pair('ramp_noise', n, c, 58, 75)
    assert pred[:, :, -1].mean() - pred[:, :, 0].mean() > 0.9 and bool((pred != gt).any())
    pred, gt = UM.make_pair('rand', n, c, h, w)
    assert 0 <= pred.min() and pred.max() <= 1 and 0 <= gt.min() and gt.max() <= 1 and not torch.equal(pred[0], pred[1])
    for kind in UM.KINDS:  # seeded: the same case gives the same tensors; another salt gives others where anything is random
        a, b, other = UM.make_pair(kind, 2, 3, 13, 17), UM.make_pair(kind, 2, 3, 13, 17), UM.make_pair(kind, 2, 3, 13, 17, salt=1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].dtype == torch.float32 and a[0].shape == (2, 3, 13, 17)
        assert torch.equal(a[0], other[0]) == (kind in ('const', 'black_white', 'checker', 'checker_inv')), kind


def test_ssim_geometries_reach_what_they_claim():
    """(valid region, tiles (rows, columns), size of the last tile (rows, columns)) computed from the shapes as csrc/metrics.hip computes them"""
    want = {(11, 11, 0): ((1, 1), (1, 1), (1, 1)), (13, 43, 1): ((1, 31), (1, 2), (1, 15)), (26, 26, 0): ((16, 16), (1, 1), (16, 16)),
            (27, 42, 0): ((17, 32), (2, 2), (1, 16)), (58, 75, 0): ((48, 65), (3, 5), (16, 1)), (40, 44, 7): ((16, 20), (1, 2), (16, 4))}
    assert set(want) == set(UM.SSIM_GEOMS)
    clamped = {}
    for (h, w, crop) in UM.SSIM_GEOMS:
        vh, vw, ty, tx = UM.ssim_tiles(h, w, crop)
        assert ((vh, vw), (ty, tx), (vh - 16 * (ty - 1), vw - 16 * (tx - 1))) == want[(h, w, crop)], (h, w, crop)
        # the 26 x 26 window of the last tile runs past the cropped image: those loads are clamped (and feed masked outputs only)
        clamped[(h, w, crop)] = (16 * (ty - 1) + 25 > h - 2 * crop - 1, 16 * (tx - 1) + 25 > w - 2 * crop - 1)
    assert clamped[(40, 44, 7)] == (False, True) and clamped[(58, 75, 0)] == (False, True) and clamped[(27, 42, 0)] == (True, False)
    assert clamped[(26, 26, 0)] == (False, False)  # one full tile: nothing clamped, nothing masked
    assert UM.ssim_tiles(58, 75, 0)[2] >= 3 and UM.ssim_tiles(58, 75, 0)[3] >= 3  # a tile with all eight neighbours
    assert UM.ssim_tiles(20, 40, 5)[0] <= 0  # what calculate_ssim refuses


def test_psnr_geometries_reach_what_they_claim():
    """blocks as sum_squared_error_uint8 sizes the grid, and the pixels each block receives from the kernel's loop"""
    want_blocks = {(1, 1, 0): 1, (3, 3, 1): 1, (64, 64, 0): 1, (64, 65, 0): 2, (70, 70, 30): 2, (1032, 1024, 0): 256, (1032, 1024, 5): 256}
    assert set(want_blocks) == set(UM.PSNR_GEOMS)
    for (h, w, crop) in UM.PSNR_GEOMS:
        assert UM.psnr_blocks(h, w) == want_blocks[(h, w, crop)]
        px = UM.psnr_block_pixels(h, w, crop)
        assert px.sum() == (h - 2 * crop) * (w - 2 * crop) and len(px) == want_blocks[(h, w, crop)]
    assert UM.psnr_block_pixels(3, 3, 1).tolist() == [1]
    assert UM.psnr_block_pixels(64, 64, 0).tolist() == [4096] and 64 * 64 == 4096  # the last size with one block
    assert UM.psnr_block_pixels(64, 65, 0).tolist() == [2048 + 64, 2048]
    assert UM.psnr_block_pixels(70, 70, 30).tolist() == [100, 0]  # block 1 receives nothing
    for crop in (0, 5):
        assert 1032 * 1024 > 1 << 20 and (1032 * 1024 + 4095) // 4096 > 256  # the cap binds: the block stride is 256 * 256 = 65,536
        px = UM.psnr_block_pixels(1032, 1024, crop)
        assert px.min() >= 15 * 256 and px.max() > px.min()  # 16 or 17 turns per thread, a ragged last turn
        assert UM.psnr_n(1032, 1024) == 1 and UM.psnr_kinds(1032, 1024) == ('rand', 'black_white')
    assert 65025 * 3 * 1032 * 1024 < 2 ** 53 and UM.psnr_n(70, 70) == 3 and UM.psnr_kinds(70, 70) == UM.KINDS


@pytest.mark.parametrize('geom', UM.SSIM_GEOMS, ids=lambda g: '%dx%d_crop%d' % g)
def test_separable_ssim_is_the_2d_window(geom):
    """horizontal then vertical 11-tap pass over five moments (the kernel's algorithm, NumPy float64) against the oracle's 2-D window, on every
    (geometry, content) pair: within 1e-12, so the 1e-10 of the GPU tests is met by the algorithm itself with room to spare"""
    h, w, crop = geom
    worst = 0.0
    for kind in UM.KINDS:
        pred, gt = UM.make_pair(kind, 3, 3, h, w)
        for c, ych in UM.MODES:
            p, g = UM.take_channels(pred, c), UM.take_channels(gt, c)
            for i in range(3):
                want, got = EO.ssim_cropped(p[i], g[i], crop, ych), UM.ssim_separable(p[i], g[i], crop, ych)
                assert math.isfinite(want) and abs(got - want) <= 1e-12, (geom, kind, c, ych, i, got, want)
                worst = max(worst, abs(got - want))
                if kind == 'identical':
                    assert want == 1.0 and abs(got - 1.0) <= 1e-12
    print('%dx%d crop %d: separable vs 2-D SSIM max |diff| %.3e' % (h, w, crop, worst))


def test_y_reference_is_the_oracles():
    """sse_y_ref differs from psnr_cropped only in the float64 sum (psnr_cropped: float32 mean): the same planes, the same squares"""
    pred, gt = UM.make_pair('wide', 2, 3, 27, 42)
    for crop in (0, 7):
        sse, count = UM.sse_ref(pred, gt, crop, True)
        assert count == (27 - 2 * crop) * (42 - 2 * crop)
        for i in range(2):
            assert abs(UM.psnr_of(sse[i], count) - EO.psnr_cropped(pred[i], gt[i], crop, True)) <= 1e-4
    one = UM.take_channels(pred, 1), UM.take_channels(gt, 1)
    assert UM.sse_ref(*one, 0, True) == UM.sse_ref(*one, 0, False)  # one channel: the flag is ignored
