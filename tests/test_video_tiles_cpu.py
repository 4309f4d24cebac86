"""CPU: frames of any size on the whole-video path (edvr_amd/video.py: pad_mode / tile) - the tile geometry, the lockstep schedule over
per-tile banks and the argument errors; no kernels.  The device side is tests/test_gpu_video_tiles.py."""
import pytest
import torch
import torch.nn.functional as F

PADDINGS = ('replicate', 'reflection', 'reflection_circle', 'circle')


def _up(v, m):
    return (v + m - 1) // m * m


def _check_grid(H, W, tile, overlap, m):
    from edvr_amd.video import tile_grid
    grid = tile_grid(H, W, tile, overlap, m)
    Hp, Wp = _up(H, m), _up(W, m)
    th, tw = min(tile[0], Hp), min(tile[1], Wp)
    written = torch.zeros(H, W, dtype=torch.int32)
    for src, keep, dst in grid:
        y0, x0, sh, sw = src
        ky, kx, kh, kw = keep
        assert (sh, sw) == (th, tw)                                             # exactly the tile shape ...
        assert 0 <= y0 and y0 + th <= Hp and 0 <= x0 and x0 + tw <= Wp           # ... inside the padded frame
        assert y0 % m == 0 and x0 % m == 0 and ky % m == 0 and kx % m == 0       # origins and cuts are multiples of m
        assert (ky + kh) % m == 0 or y0 + ky + kh == H
        assert (kx + kw) % m == 0 or x0 + kx + kw == W
        assert kh > 0 and kw > 0 and ky >= 0 and kx >= 0 and ky + kh <= th and kx + kw <= tw
        assert dst == (y0 + ky, x0 + kx)
        written[dst[0]:dst[0] + kh, dst[1]:dst[1] + kw] += 1
        assert dst[0] + kh <= H and dst[1] + kw <= W
        # a kept pixel is at least overlap / 2 away from every tile edge that is not an edge of the padded frame
        if y0 > 0:
            assert ky >= overlap // 2
        if y0 + th < Hp:
            assert th - (ky + kh) >= overlap // 2
        if x0 > 0:
            assert kx >= overlap // 2
        if x0 + tw < Wp:
            assert tw - (kx + kw) >= overlap // 2
    assert bool((written == 1).all()), (H, W, tile, overlap, m)                  # exactly once: no gap, no pixel written twice
    return grid


@pytest.mark.parametrize('m', [4, 16])
def test_tile_grid_invariants(m):
    th, tw = 6 * m, 8 * m
    sizes = sorted(set([1, m - 1, m, m + 1, 3 * m + 2, 6 * m - 1, 6 * m, 6 * m + 1, 8 * m, 8 * m + 3, 11 * m + m // 2, 12 * m, 16 * m, 19 * m + 1, 24 * m + 5]))
    n = 0
    for overlap in range(0, th - 2 * m + 1, 2 * m):                              # 0 ... tile - 2 m
        for H in sizes:
            for W in sizes:
                grid = _check_grid(H, W, (th, tw), overlap, m)
                n += 1
                if th >= _up(H, m) and tw >= _up(W, m):                         # one tile >= the padded frame: the padding-only case
                    assert grid == [((0, 0, _up(H, m), _up(W, m)), (0, 0, H, W), (0, 0))]
    assert n > 500


def test_tile_grid_counts_and_defaults():
    from edvr_amd import tile_grid
    assert len(tile_grid(62, 90, (32, 48), 8, 4)) == 9                           # 64 x 92 padded: 3 x 3 tiles of (32, 48)
    assert len(tile_grid(120, 136, (64, 80), 32, 16)) == 9                      # 128 x 144 padded, stride (32, 48): 3 x 3 tiles
    assert len(tile_grid(544, 960, (304, 512), None, 4)) == 4                   # the default overlap is 8 m = 32
    assert tile_grid(544, 960, (304, 512), None, 4) == tile_grid(544, 960, (304, 512), 32, 4)
    assert tile_grid(270, 480, None, None, 4) == [((0, 0, 272, 480), (0, 0, 270, 480), (0, 0))]
    # the last row / column is shifted inwards, never padded further
    g = tile_grid(100, 100, (48, 48), 8, 4)
    assert max(t.src[0] for t in g) == 100 - 48 and max(t.src[1] for t in g) == 100 - 48


# ---- lockstep schedule: CPU stand-ins for the device primitives, a stub net whose "features" are (frame index, tile origin)
class _StubNet(torch.nn.Module):
    def __init__(self, num_frame, hr_in=False):
        super().__init__()
        self.conv_l2_1 = torch.nn.Conv2d(2, 2, 3, 2, 1)
        self.hr_in = self.with_predeblur = hr_in
        self.center_frame_idx = num_frame // 2
        self.extracted, self.windows, self.occupancy, self.restorer = [], [], [], None

    def check_offsets(self, wait=True):
        pass

    def extract_features(self, frames, out=None):
        # channel 0 of the test's frames = frame index, channels 1 / 2 = the pixel's (y, x) in the frame: the tile's first pixel
        # names the tile
        for i in range(frames.shape[0]):
            self.extracted.append((int(frames[i, 0, 0, 0]), int(frames[i, 1, 0, 0]), int(frames[i, 2, 0, 0])))
        self.occupancy.append(self.restorer.bank_frames)
        for o in out:
            assert o.shape[0] == frames.shape[0]
            o[:, 0] = frames[:, 0, :1, :1]
            o[:, 1] = frames[:, 1, 0, 0].view(-1, 1, 1) * 1000 + frames[:, 2, 0, 0].view(-1, 1, 1)
        return list(out)

    def restore_from_features(self, pyr, x_center, b, t, out_dtype=torch.float32, out=None, keep=None):
        assert all(f.shape[0] == b * t for f in pyr) and x_center.shape[0] == b
        origin = int(x_center[0, 1, 0, 0]) * 1000 + int(x_center[0, 2, 0, 0])
        levels = [f[:, 0, 0, 0].view(b, t).to(torch.int64).tolist() for f in pyr]
        assert levels[0] == levels[1] == levels[2]
        for f in pyr:  # every image of the window comes from this tile's own bank
            assert bool((f[:, 1, 0, 0] == origin).all())
        self.windows.append((origin, levels[0]))
        s = 1 if self.hr_in else 4
        result = x_center.repeat_interleave(s, 2).repeat_interleave(s, 3)  # the "restored" tile: its own crop, enlarged
        ky, kx = keep
        self.restorer.writes[0] += 1
        cnt = self.restorer.count_of(out)
        cnt += 1
        out.copy_(result[:, :, ky:ky + out.shape[2], kx:kx + out.shape[3]])
        return out


def _stub_restorer(num_frame, padding, chunk, hr_in=False, **kw):
    from edvr_amd import VideoRestorer

    class CpuRestorer(VideoRestorer):  # CPU stand-ins for the device primitives
        writes = None

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

        def count_of(self, view):
            """a write counter with the geometry of the output `view` is a view of (how often each output pixel is written)"""
            base = view._base
            key = base.data_ptr()
            if key not in self.counters:
                self.counters[key] = (base, torch.zeros(base.shape, dtype=torch.int32))
            return torch.as_strided(self.counters[key][1], view.shape, view.stride(), view.storage_offset())

    net = _StubNet(num_frame, hr_in).eval()
    vr = CpuRestorer(net, num_frame=num_frame, padding=padding, chunk=chunk, **kw)
    vr.writes, vr.counters = [0], {}
    net.restorer = vr
    return net, vr


def _coded_frames(n, H, W):
    f = torch.empty(n, 3, H, W)
    f[:, 0] = torch.arange(n, dtype=torch.float32).view(n, 1, 1)
    f[:, 1] = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    f[:, 2] = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    return f


def _batches(frames, pattern):
    i = k = 0
    while i < frames.shape[0]:
        m = min(pattern[k % len(pattern)], frames.shape[0] - i)
        yield frames[i] if pattern == (1,) else frames[i:i + m]
        i, k = i + m, k + 1


@pytest.mark.parametrize('padding', PADDINGS)
@pytest.mark.parametrize('chunk', (1, 4))
@pytest.mark.parametrize('n', (5, 17))
@pytest.mark.parametrize('pattern', ((1,), (3, 1, 7, 2)))
def test_tiled_schedule(padding, chunk, n, pattern):
    from edvr_amd import tile_grid, window_table
    t, H, W = 5, 22, 30  # padded to 24 x 32; tiles (16, 16), overlap 8: 2 x 3 tiles
    net, vr = _stub_restorer(t, padding, chunk, pad_mode='replicate', tile=(16, 16), tile_overlap=8)
    grid = tile_grid(H, W, (16, 16), 8, 4)
    assert len(grid) == 6
    frames = _coded_frames(n, H, W)
    table = window_table(n, t, padding).tolist()
    with torch.no_grad():
        outs = list(vr.restore_chunks(_batches(frames, pattern)))
    out = torch.cat(outs, 0)
    # the output: every pixel of every frame written exactly once, each from the tile that keeps it (the stub's result is the enlarged crop)
    assert tuple(out.shape) == (n, 3, 4 * H, 4 * W)
    assert torch.equal(out, frames.repeat_interleave(4, 2).repeat_interleave(4, 3))
    assert len(vr.counters) == len(outs)
    for base, cnt in vr.counters.values():
        assert bool((cnt == 1).all())
    # every (frame, tile) through the per-frame stage exactly once
    origins = [(tl.src[0], tl.src[1]) for tl in grid]
    assert sorted(net.extracted) == sorted((f, y, x) for f in range(n) for y, x in origins)
    # every restore call saw the window of its frames from its own tile's bank, tile by tile within a chunk
    per_tile = {y * 1000 + x: [] for y, x in origins}
    for origin, rows in net.windows:
        per_tile[origin] += rows
    for rows in per_tile.values():
        assert rows == table
    assert [o for o, _ in net.windows[:len(grid)]] == [y * 1000 + x for y, x in origins]
    limit = chunk + 2 * (t - 1)
    assert max(net.occupancy) <= vr.capacity <= limit and vr.slots <= limit  # per tile: its bank is a ring of `slots` frames
    assert vr.writes[0] == len(grid) * len(outs)


def test_padding_only_is_one_tile_and_hr_in_scale():
    net, vr = _stub_restorer(3, 'replicate', 2, hr_in=True, pad_mode='reflect')
    frames = _coded_frames(6, 40, 50)  # hr_in: multiples of 16 -> 48 x 64
    with torch.no_grad():
        out = vr.restore(frames)
    assert len(vr.grid) == 1 and vr.grid[0].src == (0, 0, 48, 64) and vr.grid[0].keep == (0, 0, 40, 50)
    assert torch.equal(out, frames)  # scale 1
    assert sorted(net.extracted) == [(f, 0, 0) for f in range(6)]


def test_argument_errors():
    from edvr_amd import tile_grid
    with pytest.raises(ValueError):
        _stub_restorer(5, 'replicate', 4, tile=(30, 32))                  # not a multiple of m
    with pytest.raises(ValueError):
        _stub_restorer(5, 'replicate', 4, hr_in=True, tile=(40, 48))      # m = 16 with hr_in
    with pytest.raises(ValueError):
        _stub_restorer(5, 'replicate', 4, tile=(32, 32), tile_overlap=32)  # overlap >= tile
    with pytest.raises(ValueError):
        _stub_restorer(5, 'replicate', 4, tile=(32, 32), tile_overlap=4)   # not a multiple of 2 m
    with pytest.raises(ValueError):
        _stub_restorer(5, 'replicate', 4, tile=(32, 32))                   # the default overlap 8 m = 32 is not below the tile
    with pytest.raises(ValueError):
        _stub_restorer(5, 'replicate', 4, pad_mode='circular')
    with pytest.raises(ValueError):
        _stub_restorer(5, 'replicate', 4, tile_overlap=8)                  # overlap without tile
    with pytest.raises(ValueError):
        tile_grid(64, 64, (32, 32), 40, 4)
    # 'reflect' on a frame smaller than its pad: 2 rows cannot be mirrored into 2 more without repeating the edge
    net, vr = _stub_restorer(3, 'replicate', 2, pad_mode='reflect')
    with torch.no_grad(), pytest.raises(ValueError, match='2 x 9'):
        vr.restore(_coded_frames(4, 2, 9))
    # a size that is not a multiple still raises what it raises today with pad_mode=None - with and without tiles
    for kw in ({}, {'tile': (16, 16), 'tile_overlap': 8}):
        net, vr = _stub_restorer(3, 'replicate', 2, **kw)
        with torch.no_grad(), pytest.raises(AssertionError, match='multiple of 4'):
            vr.restore(_coded_frames(4, 22, 32))


def test_defaults_take_the_plain_path():
    """Without pad_mode / tile the restorer never touches the new primitives (the stub of tests/test_video_cpu.py has none of them)."""
    net, vr = _stub_restorer(5, 'reflection_circle', 4)
    assert not vr.tiled and vr.multiple == 4 and vr.scale == 4

    def boom(*a, **k):
        raise AssertionError('the plain path must not crop')
    vr._crop = boom
    seen = []
    net.restore_from_features = lambda pyr, x_center, b, t, out_dtype=torch.float32: seen.append(b) or x_center.clone()
    with torch.no_grad():
        out = vr.restore(_coded_frames(9, 8, 8))
    assert seen == [4, 4, 1] and tuple(out.shape) == (9, 3, 8, 8)
