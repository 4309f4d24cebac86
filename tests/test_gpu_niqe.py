"""GPU: csrc/niqe.hip (metrics.niqe_moments / metrics.calculate_niqe) against the reference's calculate_niqe recorded in
tests/golden/niqe.pt (scripts/make_niqe_golden.py) and against the NumPy restatement of the definition (tests/util_niqe.py); the layouts,
the crop, the batch and restore_y4m's on_chunk hook.

Tolerance against the reference: the fixture's `tol` = 4 x max |ref - ref64|, the reference's own float32 noise.  Moments
against the restatement: counts exact, sums to 1e-6 relative - one float32 ulp on every z moves a sum of squares by 2 x 2^-23 = 2.4e-7,
the bound leaves four times that; the order of the float64 additions contributes 1e-13.
"""
import io
import os

import numpy as np
import pytest
import torch

import util_niqe as N

pytestmark = pytest.mark.gpu

_CACHE = {}


def _data():
    if not _CACHE:
        from edvr_amd import metrics
        d = N.load_cases()
        _CACHE.update(tol=d['tol'], cases={c['name']: c for c in d['cases']}, restated={},
                      params=metrics.load_niqe_params(os.path.join(N.GOLDEN, 'niqe_pris_params.npz')))
    return _CACHE


def _restated(name):
    """(n, 2, blocks, 5, 5) of the restatement, computed once per case"""
    d = _data()
    if name not in d['restated']:
        c = d['cases'][name]
        d['restated'][name] = np.stack([N.moments(img, c['crop_border'])[0] for img in c['img'].numpy()])
    return d['restated'][name]


NAMES = ['noise', 'smooth', 'cropped', 'grey']


@pytest.mark.parametrize('name', NAMES)
def test_calculate_niqe_matches_the_reference(gpu, name):
    from edvr_amd import metrics
    d = _data()
    c = d['cases'][name]
    got = metrics.calculate_niqe(N.chw_float(c['img']).to(gpu), c['crop_border'], params=d['params'])
    err = [abs(g - r) for g, r in zip(got, c['ref'])]
    print(f'{name}: got {got} ref {c["ref"]} |d| {err} tol {d["tol"]:.3e}')
    assert len(got) == c['img'].shape[0] and max(err) <= d['tol']
    by_path = metrics.calculate_niqe(N.chw_float(c['img']).to(gpu), c['crop_border'], params=os.path.join(N.GOLDEN, 'niqe_pris_params.npz'))
    assert by_path == got


@pytest.mark.parametrize('name', NAMES)
def test_moments_match_the_restatement(gpu, name):
    from edvr_amd import metrics
    c = _data()['cases'][name]
    got = metrics.niqe_moments(N.chw_float(c['img']).to(gpu), c['crop_border'])
    want = _restated(name)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 3], want[..., 3])  # the counts
    for k in (0, 2, 4):
        rel = np.abs(got[..., k] - want[..., k]) / want[..., k]
        print(f'{name} k={k}: max relative difference {rel.max():.3e}')
        assert rel.max() <= 1e-6
    # every pixel of a block is on one side or the other in these images (no constant neighbourhood): nothing was skipped
    n_px = np.array([96 * 96, 48 * 48]).reshape(1, 2, 1, 1)
    assert np.array_equal(got[..., 1] + got[..., 3], np.broadcast_to(n_px, got[..., 1].shape))


def test_a_frame_does_not_depend_on_its_place_in_the_batch(gpu):
    from edvr_amd import metrics
    x = N.chw_float(_data()['cases']['noise']['img']).to(gpu)
    both = metrics.niqe_moments(x)
    for i in range(2):
        assert torch.equal(both[i], metrics.niqe_moments(x[i:i + 1])[0])
        assert torch.equal(both[i], metrics.niqe_moments(x[i])[0])  # (3, h, w)


@pytest.mark.parametrize('name', ['noise', 'cropped'])
def test_uint8_entry_equals_float_entry(gpu, name):
    from edvr_amd import metrics
    d = _data()
    c = d['cases'][name]
    as_bytes, as_float = c['img'].to(gpu), N.chw_float(c['img']).to(gpu)
    assert torch.equal(metrics.niqe_moments(as_bytes, c['crop_border']), metrics.niqe_moments(as_float, c['crop_border']))
    assert metrics.calculate_niqe(as_bytes, c['crop_border'], params=d['params']) == metrics.calculate_niqe(as_float, c['crop_border'], params=d['params'])


def test_crop_and_discarded_pixels_are_never_read(gpu):
    """Case 3 (203 x 301, crop_border=4) against its kept 192 x 288 rectangle alone: the halo replicates the KEPT edge; and a 96 x 200 frame
    against its first 192 columns."""
    from edvr_amd import metrics
    img = _data()['cases']['cropped']['img']
    whole = metrics.niqe_moments(N.chw_float(img).to(gpu), 4)
    alone = metrics.niqe_moments(N.chw_float(img[:, 4:196, 4:292].contiguous()).to(gpu), 0)
    assert tuple(whole.shape) == (1, 2, 6, 5, 5) and torch.equal(whole, alone)
    as_bytes = metrics.niqe_moments(img[:, 4:196, 4:292].contiguous().to(gpu), 0)
    assert torch.equal(whole, as_bytes)
    g = torch.Generator().manual_seed(96200)
    wide = torch.randint(0, 256, (1, 96, 200, 3), generator=g, dtype=torch.uint8)
    assert torch.equal(metrics.niqe_moments(N.chw_float(wide).to(gpu)), metrics.niqe_moments(N.chw_float(wide[:, :, :192].contiguous()).to(gpu)))
    assert torch.equal(metrics.niqe_moments(wide.to(gpu)), metrics.niqe_moments(wide[:, :, :192].contiguous().to(gpu)))


def test_refusals(gpu):
    from edvr_amd import metrics
    d = _data()
    x = N.chw_float(d['cases']['noise']['img'])
    with pytest.raises(NotImplementedError):
        metrics.calculate_niqe(x, params=d['params'])  # a CPU tensor
    with pytest.raises(NotImplementedError):
        metrics.niqe_moments(x)
    with pytest.raises(NotImplementedError, match='gray'):
        metrics.calculate_niqe(x.to(gpu), params=d['params'], convert_to='gray')
    with pytest.raises(ValueError, match='96'):
        metrics.calculate_niqe(x[:, :, :95].contiguous().to(gpu), params=d['params'])
    with pytest.raises(ValueError, match='96'):
        metrics.niqe_moments(x.to(gpu), crop_border=1)  # 94 rows left
    with pytest.raises(ValueError, match='params'):
        metrics.calculate_niqe(x.to(gpu))
    from edvr_amd import _lib
    L = _lib.lib()
    assert L.edvr_niqe_blocks(96, 192, 0) == 2 and L.edvr_niqe_blocks(203, 301, 4) == 6 and L.edvr_niqe_blocks(95, 400, 0) == 0
    assert L.edvr_niqe_blocks(96, 96, 48) == 0 and L.edvr_niqe_blocks(96, 96, -1) == 0
    out = torch.zeros(50, dtype=torch.float64, device=gpu)
    xs = x[:1, :, :95].contiguous().to(gpu)
    assert L.edvr_niqe_moments_f32(xs.data_ptr(), out.data_ptr(), 1, 3, 95, 192, 0, 0, None) != 0  # refused by the library too: no launch
    assert not out.any()


def test_restore_y4m_on_chunk_sees_every_output_frame_once(gpu):
    """7 frames of 16 x 24 through the M_T5 test network: the hook receives every restored frame once, in order, as float32 RGB on the
    device, and the written stream is byte for byte that of a run without the hook."""
    import util_yuv as U
    from util_edvr import build
    from edvr_amd import VideoRestorer, ops
    from edvr_amd.y4m import restore_y4m
    net = build('M_T5')[0].to(gpu).eval()
    H, W = 16, 24
    frames = torch.randint(0, 256, (7, U.frame_size(H, W)), generator=torch.Generator().manual_seed(1624), dtype=torch.uint8)
    data = U.y4m_bytes(frames, H, W)
    seen = []
    with torch.no_grad():
        plain, hooked = io.BytesIO(), io.BytesIO()
        assert restore_y4m(net, io.BytesIO(data), plain, read_frames=3, chunk=3) == 7
        assert restore_y4m(net, io.BytesIO(data), hooked, read_frames=3, chunk=3, on_chunk=lambda c: seen.append(c.clone())) == 7
        want = VideoRestorer(net, out_dtype=torch.float32, chunk=3).restore(ops.yuv420_to_rgb(frames.to(gpu), H, W, 'bt601', 'limited', 'bilinear'))
    assert hooked.getvalue() == plain.getvalue()
    assert all(c.dtype == torch.float32 and c.is_cuda and c.shape[1:] == (3, 4 * H, 4 * W) for c in seen)
    assert torch.equal(torch.cat(seen), want)
