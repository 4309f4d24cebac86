"""CPU: blended tile seams on the whole-video path (edvr_amd/video.py: tile_blend) - the band geometry, the argument errors, the
schedule of weighted read-modify-write tails with host stand-ins, and the script option; no kernels.  The device side is
tests/test_gpu_video_blend.py."""
import importlib.util
import os
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F


def _up(v, m):
    return (v + m - 1) // m * m


def _ramp(B):
    return (2 * torch.arange(B, dtype=torch.float32) + 1) / torch.tensor(float(2 * B), dtype=torch.float32)


def _axis_weights(n, lo, hi):
    w = torch.ones(n, dtype=torch.float32)
    if lo:
        w[:lo] = _ramp(lo)
    if hi:
        w[n - hi:] = 1.0 - _ramp(hi)
    return w


# ------------------------------------------------------------------------------------------------ geometry
def _check_bands(H, W, tile, overlap, b, m):
    from edvr_amd.video import tile_bands, tile_grid
    grid = tile_grid(H, W, tile, overlap, m)
    blend = tile_bands(H, W, tile, overlap, b, m)
    assert len(blend) == len(grid)
    exact = [[Fraction(0)] * W for _ in range(H)] if H * W <= 4096 else None    # exact rational weight sums (small frames)
    total = torch.zeros(H, W, dtype=torch.float32)                                # float32 sums, in work-list order
    firsts, lasts = torch.zeros(H, W, dtype=torch.int32), torch.zeros(H, W, dtype=torch.int32)
    bands_y, bands_x = set(), set()
    for t, tb in zip(grid, blend):
        (y0, x0, th, tw), (ky, kx, kh, kw) = t.src, t.keep
        (ey, ex, eh, ew), (oy, ox), (yl, yh, xl, xh) = tb.ext, tb.dst, tb.bands
        assert all(v in (0, b) for v in tb.bands) and (oy, ox) == (y0 + ey, x0 + ex)
        # the extended rectangle: the kept one plus b / 2 into each neighbouring band, inside its tile and the frame
        assert (ey, eh) == (ky - yl // 2, kh + yl // 2 + yh // 2) and (ex, ew) == (kx - xl // 2, kw + xl // 2 + xh // 2)
        assert 0 <= ey and ey + eh <= th and 0 <= ex and ex + ew <= tw and yl + yh <= eh and xl + xh <= ew
        assert 0 <= oy and oy + eh <= H and 0 <= ox and ox + ew <= W
        assert (yl > 0) == (t.dst[0] > 0) and (xl > 0) == (t.dst[1] > 0) and (yh > 0) == (t.dst[0] + kh < H) and (xh > 0) == (t.dst[1] + kw < W)
        if yl:
            bands_y.add((oy, oy + b))                                            # [c - b / 2, c + b / 2) around the cut c = t.dst[0]
            assert oy + b // 2 == t.dst[0]
        if yh:
            bands_y.add((oy + eh - b, oy + eh))
        if xl:
            bands_x.add((ox, ox + b))
            assert ox + b // 2 == t.dst[1]
        if xh:
            bands_x.add((ox + ew - b, ox + ew))
        wy, wx = _axis_weights(eh, yl, yh), _axis_weights(ew, xl, xh)
        total[oy:oy + eh, ox:ox + ew] += wy[:, None] * wx[None, :]
        first = torch.ones(eh, ew, dtype=torch.int32)
        first[:yl], first[:, :xl] = 0, 0
        last = torch.ones(eh, ew, dtype=torch.int32)
        last[eh - yh:], last[:, ew - xh:] = 0, 0
        firsts[oy:oy + eh, ox:ox + ew] += first
        lasts[oy:oy + eh, ox:ox + ew] += last
        if exact is not None:
            def frac(i, n, lo, hi):
                return Fraction(2 * i + 1, 2 * lo) if i < lo else 1 - Fraction(2 * (i - (n - hi)) + 1, 2 * hi) if i >= n - hi else Fraction(1)
            fy, fx = [frac(i, eh, yl, yh) for i in range(eh)], [frac(j, ew, xl, xh) for j in range(ew)]
            for i in range(eh):
                for j in range(ew):
                    exact[oy + i][ox + j] += fy[i] * fx[j]
    # every band is the high band of one tile row / column and the low band of the next (the set holds it once); bands are disjoint
    for bands, size in ((sorted(bands_y), H), (sorted(bands_x), W)):
        for (a0, a1), (b0, b1) in zip(bands, bands[1:]):
            assert a1 <= b0
        assert all(0 <= a0 and a1 <= size for a0, a1 in bands)
    assert len(bands_y) == len({t.dst[0] for t in grid}) - 1 and len(bands_x) == len({t.dst[1] for t in grid}) - 1
    assert bool((firsts == 1).all()) and bool((lasts == 1).all())               # one first and one last contributor per pixel
    ulp = 2.0 ** -23
    assert float((total - 1).abs().max()) <= 2 * ulp, (H, W, tile, overlap, b, m)
    if exact is not None:
        assert all(v == 1 for row in exact for v in row)
    return blend


@pytest.mark.parametrize('m', [4, 16])
def test_band_geometry(m):
    from edvr_amd.video import tile_bands
    th, tw = 6 * m, 8 * m
    sizes = sorted(set([m, 3 * m + 2, 6 * m, 6 * m + 1, 8 * m + 3, 11 * m + m // 2, 12 * m, 16 * m - 1, 19 * m + 1]))
    ok = refused = 0
    for overlap in range(2 * m, th - 2 * m + 1, 2 * m):
        for b in sorted({2 * m, overlap}):
            for H in sizes:
                for W in sizes[::2] if m == 16 else sizes:
                    try:
                        tile_bands(H, W, (th, tw), overlap, b, m)
                    except ValueError as e:
                        assert 'tile_blend' in str(e) and 'kept lengths' in str(e)
                        refused += 1
                        continue
                    _check_bands(H, W, (th, tw), overlap, b, m)
                    ok += 1
    assert ok > 100 and refused > 0, (ok, refused)                                # (the inward-shifted last tile makes the refusals)


def test_band_geometry_of_the_device_cases():
    _check_bands(62, 90, (32, 48), 8, 8, 4)
    blend = _check_bands(120, 136, (64, 80), 32, 32, 16)
    assert blend[4].ext == (0, 0, 64, 64) and blend[4].bands == (32, 32, 32, 32)  # the middle tile: its columns are all band
    _check_bands(544, 960, (304, 512), None, 32, 4)                              # the default overlap


def test_geometry_errors():
    """A kept length between two cuts below b.  (The issue also names "tile 12, overlap 8, b 8, m 4 on a frame where the last kept length
    is 2": no frame gives that - the last kept length is tile - cut offset - (padded - size) >= tile - shared / 2 - (m - 1) with
    shared <= tile - m, i.e. more than b / 2; what these sizes do violate, with three tiles or more, is the length between two cuts.)"""
    from edvr_amd.video import _tile_axis, tile_bands
    assert [k for _, _, k in _tile_axis(20, 20, 12, 8, 4)] == [8, 4, 8]          # cuts 8 and 12: 4 < b = 8
    with pytest.raises(ValueError, match=r'kept lengths \[8, 4, 8\]'):
        tile_bands(20, 40, (12, 40), 8, 8, 4)
    assert [k for _, _, k in _tile_axis(52, 52, 32, 16, 4)] == [24, 8, 20]       # next to the inward-shifted last tile
    with pytest.raises(ValueError, match='column cuts'):
        tile_bands(32, 52, (32, 32), 16, 16, 4)
    for size in range(13, 200):                                                  # the last kept length is never below b / 2 = 4 here
        axis = _tile_axis(size, _up(size, 4), 12, 8, 4)
        assert axis[-1][2] >= 5 or len(axis) == 1
    with pytest.raises(ValueError):
        tile_bands(64, 64, (32, 32), 8, 12, 4)                                   # not a multiple of 2 m
    with pytest.raises(ValueError):
        tile_bands(64, 64, (32, 32), 8, 16, 4)                                   # above the overlap
    with pytest.raises(ValueError):
        tile_bands(64, 64, (32, 32), 8, 0, 4)


# ------------------------------------------------------------------------------------------------ schedule
def _stub_result(x, s):
    """The stub network's "restoration" of an (oriented) crop: depends on where a pixel lies in the tile, so that neighbouring tiles
    (and the elements of an ensemble) disagree in the bands."""
    up = x.repeat_interleave(s, 2).repeat_interleave(s, 3)
    ramp = torch.linspace(0.9, 1.1, up.shape[2]).view(1, 1, -1, 1) + torch.linspace(-0.05, 0.05, up.shape[3]).view(1, 1, 1, -1)
    return up * ramp


def _to_u8(v):
    return (v.clamp(0, 1) * 255).round().to(torch.uint8)


class _StubNet(torch.nn.Module):
    def __init__(self, num_frame, hr_in=False):
        super().__init__()
        self.conv_l2_1 = torch.nn.Conv2d(2, 2, 3, 2, 1)
        self.hr_in = self.with_predeblur = hr_in
        self.center_frame_idx = num_frame // 2
        self.calls = []

    def check_offsets(self, wait=True):
        pass

    def extract_features(self, frames, out=None):
        return list(out)

    def restore_from_features(self, pyr, x_center, b, t, out_dtype=torch.float32, out=None, keep=None, **kw):
        """Host stand-ins for the tails: the plain store, or - with bands= - the weighted read-modify-write of the definition."""
        from edvr_amd import ops
        self.calls.append(dict(kw))
        s = 1 if self.hr_in else 4
        ky, kx = keep
        u8 = out_dtype == torch.uint8
        kh, kw_ = (out.shape[1], out.shape[2]) if u8 else (out.shape[2], out.shape[3])
        elem = kw.get('elem')
        v = ops.d4_invert(_stub_result(x_center, s), elem or 0)[:, :, ky:ky + kh, kx:kx + kw_]
        if 'bands' not in kw:
            assert not kw
            out.copy_(_to_u8(v).permute(0, 2, 3, 1) if u8 else v)
            return out
        yl, yh, xl, xh = kw['bands']
        mode, scale, acc = kw.get('accumulate', 'only'), kw.get('scale', 1.0), kw.get('acc')
        assert (acc is not None) == u8 and (elem is not None or (mode == 'only' and scale == 1.0))
        w = _axis_weights(kh, yl, yh)[:, None] * _axis_weights(kw_, xl, xh)[None, :]
        first = torch.ones(kh, kw_, dtype=torch.bool)
        first[:yl], first[:, :xl] = False, False
        last = torch.ones(kh, kw_, dtype=torch.bool)
        last[kh - yh:], last[:, kw_ - xh:] = False, False
        first, last = first & (mode in ('first', 'only')), last & (mode in ('last', 'only'))
        store = acc if u8 else out
        p = w * v
        r = torch.where(first, p, store + p)
        r = torch.where(last, r * scale, r)
        if u8:
            acc.copy_(torch.where(last, acc, r))
            out.copy_(torch.where(last[None, :, :, None], _to_u8(r).permute(0, 2, 3, 1), out))
        else:
            out.copy_(r)
        return out


def _stub_restorer(num_frame, chunk, hr_in=False, **kw):
    from edvr_amd import VideoRestorer, ops

    class CpuRestorer(VideoRestorer):  # CPU stand-ins for the device primitives
        def _check_input(self, t):
            pass

        def _slot_table(self, slots, device):
            return torch.tensor(slots, dtype=torch.int32)

        def _gather(self, srcs, table):
            return [s[table.long()] for s in srcs]

        def _crop(self, frames, y0, x0, th, tw):
            H, W = frames.shape[2:]
            x = F.pad(frames, (0, max(x0 + tw - W, 0), 0, max(y0 + th - H, 0)), mode=self.pad_mode) if self.pad_mode else frames
            return x[:, :, y0:y0 + th, x0:x0 + tw].contiguous()

        def _crop_d4(self, frames, y0, x0, th, tw, elem):
            return ops.d4_apply(self._crop(frames, y0, x0, th, tw), elem).contiguous()

        def _scratch(self, shape, device):
            return torch.full(shape, float('nan'))

    net = _StubNet(num_frame, hr_in).eval()
    return net, CpuRestorer(net, num_frame=num_frame, padding='replicate', chunk=chunk, **kw)


def _direct(frames, H, W, tile, overlap, b, m, s, pad_mode, elements):
    """The definition evaluated pixel by pixel over full-frame weight maps built from the CUTS (not from the per-tile band lengths the
    schedule passes): every pixel's contributors in work-list order, acc = w * v, then acc + w * v; the ensemble's 1 / n at the end."""
    from edvr_amd import ops
    from edvr_amd.video import tile_grid
    grid = tile_grid(H, W, tile, overlap, m)
    n = frames.shape[0]
    padded = F.pad(frames, (0, _up(W, m) - W, 0, _up(H, m) - H), mode=pad_mode)
    cuts_y, cuts_x = sorted({t.dst[0] for t in grid}) + [H], sorted({t.dst[1] for t in grid}) + [W]
    B, ramp = s * b, _ramp(s * b)

    def axis_map(cuts, i, size):  # weight of tile row / column i over the whole axis, 0 where it does not contribute
        w = torch.zeros(s * size, dtype=torch.float32)
        lo, hi = s * cuts[i], s * cuts[i + 1]
        w[lo:hi] = 1.0
        if i > 0:
            w[lo - B // 2:lo + B // 2] = ramp
        if i + 2 < len(cuts):
            w[hi - B // 2:hi + B // 2] = 1.0 - ramp
        return w

    acc = torch.full((n, 3, s * H, s * W), float('nan'))
    started = torch.zeros(s * H, s * W, dtype=torch.bool)
    for t in grid:
        y0, x0, th, tw = t.src
        w = axis_map(cuts_y, cuts_y.index(t.dst[0]), H)[:, None] * axis_map(cuts_x, cuts_x.index(t.dst[1]), W)[None, :]
        on = w > 0
        crop = padded[:, :, y0:y0 + th, x0:x0 + tw]
        for k in elements or (0,):
            v = torch.zeros(n, 3, s * _up(H, m), s * _up(W, m))
            v[:, :, s * y0:s * (y0 + th), s * x0:s * (x0 + tw)] = ops.d4_invert(_stub_result(ops.d4_apply(crop, k).contiguous(), s), k)
            p = w * v[:, :, :s * H, :s * W]
            acc = torch.where(on & ~started, p, torch.where(on, acc + p, acc))
            started = started | on
    assert bool(started.all())
    return acc * (1.0 / len(elements)) if elements else acc


@pytest.mark.parametrize('elements', [None, (0, 3, 5)])
@pytest.mark.parametrize('hr_in', [False, True])
def test_blended_schedule_is_the_definition(elements, hr_in):
    m, s = (16, 1) if hr_in else (4, 4)
    H, W, tile, overlap, b = (22, 30, (16, 16), 8, 8) if not hr_in else (120, 136, (64, 80), 32, 32)   # 2 x 3 and 3 x 3 tiles
    frames = torch.rand(6, 3, H, W, generator=torch.Generator().manual_seed(1))
    kw = dict(pad_mode='replicate', tile=tile, tile_overlap=overlap, tile_blend=b, self_ensemble=elements)
    want = _direct(frames, H, W, tile, overlap, b, m, s, 'replicate', elements)
    assert bool(torch.isfinite(want).all())
    for dt in (torch.float32, torch.uint8):
        net, vr = _stub_restorer(3, 4, hr_in, out_dtype=dt, **kw)
        with torch.no_grad():
            out = vr.restore(frames)
        assert len(vr.blend_grid) == len(vr.grid) and len(net.calls) == 2 * len(vr.pairs)  # two chunks
        assert all('bands' in c and (('elem' in c) == (elements is not None)) for c in net.calls)
        if dt == torch.uint8:
            assert torch.equal(out, _to_u8(want).permute(0, 2, 3, 1))
        else:
            assert torch.equal(out, want)
    # outside the bands and without an ensemble: the unblended tiled result
    if elements is None:
        net, vr = _stub_restorer(3, 4, hr_in, **{**kw, 'tile_blend': None})
        with torch.no_grad():
            cut = vr.restore(frames)
        assert all(c == {} for c in net.calls)                                    # tile_blend=None: no new keyword reaches the network
        differ = (cut != want).any(0).any(0)
        band = torch.zeros(s * H, s * W, dtype=torch.bool)
        for t in vr.grid:
            for c, axis in ((t.dst[0], 0), (t.dst[1], 1)):
                if c > 0:
                    idx = slice(s * (c - b // 2), s * (c + b // 2))
                    band[(idx, slice(None)) if axis == 0 else (slice(None), idx)] = True
        assert bool(differ.any()) and not bool((differ & ~band).any())


def test_argument_errors():
    with pytest.raises(ValueError, match='without tile'):
        _stub_restorer(5, 4, tile_blend=8)
    with pytest.raises(ValueError, match='multiple of 8'):
        _stub_restorer(5, 4, tile=(32, 32), tile_overlap=16, tile_blend=12)
    with pytest.raises(ValueError, match='multiple of 32'):
        _stub_restorer(5, 4, hr_in=True, tile=(96, 96), tile_overlap=32, tile_blend=16)
    with pytest.raises(ValueError, match='must not exceed tile_overlap 8'):
        _stub_restorer(5, 4, tile=(32, 32), tile_overlap=8, tile_blend=16)
    with pytest.raises(ValueError, match='must not exceed tile_overlap 32'):
        _stub_restorer(5, 4, tile=(64, 64), tile_blend=40)                        # the default overlap 8 m
    with pytest.raises(ValueError):
        _stub_restorer(5, 4, tile=(32, 32), tile_overlap=8, tile_blend=-8)
    # the geometry is the frame's: accepted at construction, refused at the first frame, naming the sizes
    net, vr = _stub_restorer(3, 2, tile=(32, 32), tile_overlap=16, tile_blend=16)
    with torch.no_grad(), pytest.raises(ValueError, match=r'kept lengths \[24, 8, 20\]'):
        vr.restore(torch.rand(4, 3, 52, 52))
    with torch.no_grad():                                                         # the same restorer on a frame that fits
        assert tuple(vr.restore(torch.rand(4, 3, 48, 48)).shape) == (4, 3, 192, 192)


# ------------------------------------------------------------------------------------------------ scripts
def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_video_passes_tile_blend_on(tmp_path, monkeypatch):
    import edvr_amd
    from edvr_amd import data as D, metrics as M
    from util_data import write_video_test_tree
    mod = _load('eval_video')
    args = mod.parse_args(['--lq', 'a', '--gt', 'b', '--tile', '32', '48', '--tile-overlap', '8', '--tile-blend', '8'])
    assert args.tile_blend == 8 and mod.parse_args(['--lq', 'a', '--gt', 'b']).tile_blend is None
    with pytest.raises(SystemExit):
        mod.parse_args(['--lq', 'a', '--gt', 'b', '--tile-blend', '8'])          # needs --tile
    spec = dict(folders=['000'], frames=5, lq_hw=(8, 12), scale=4)
    write_video_test_tree(str(tmp_path), spec)

    class Net(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def to(self, device):
            return self

    def read_img_seq(paths, device='cpu', **k):
        return torch.stack([torch.from_numpy(D.decode_image(open(p, 'rb').read()).transpose(2, 0, 1).copy()).float() / 255 for p in paths])

    calls = []

    def validate_video(net, lq, gt=None, **kw):
        calls.append(kw)
        return None, [30.0] * lq.shape[0]

    monkeypatch.setattr(edvr_amd, 'EDVR', Net)
    monkeypatch.setattr(D, 'read_img_seq', read_img_seq)
    monkeypatch.setattr(M, 'validate_video', validate_video)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    for extra, want in ((['--tile', '32', '48', '--tile-overlap', '8', '--tile-blend', '8'], dict(tile=(32, 48), tile_overlap=8, tile_blend=8)),
                        (['--tile', '32', '48'], dict(tile=(32, 48))), ([], {})):
        del calls[:]
        args = mod.parse_args(['--lq', str(tmp_path / 'lq'), '--gt', str(tmp_path / 'gt'), '--num-feat', '64', '--batch', '3'] + extra)
        mod.evaluate(args, log=lambda s: None)
        assert len(calls) == 1
        got = {k: v for k, v in calls[0].items() if k in ('pad_mode', 'tile', 'tile_overlap', 'tile_blend', 'self_ensemble')}
        assert got == want, (extra, calls[0])


def test_validate_video_passes_tile_blend_only_when_given(monkeypatch):
    from edvr_amd import metrics, video
    seen = []

    class Fake:
        def __init__(self, net, **kw):
            seen.append(kw)

        def restore_chunks(self, pieces, length=None):
            for p in pieces:
                yield p

    monkeypatch.setattr(video, 'VideoRestorer', Fake)
    lq = torch.rand(3, 3, 8, 8)
    metrics.validate_video(None, lq, None, tile=(32, 32), tile_overlap=8, tile_blend=8)
    metrics.validate_video(None, lq, None, tile=(32, 32), tile_overlap=8)
    assert seen[0]['tile_blend'] == 8 and 'tile_blend' not in seen[1]
