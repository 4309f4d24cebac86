"""Whole-video restoration: every frame's features are extracted ONCE.

`EDVR.forward` takes a window of `num_frame` neighbours per output frame, and `metrics.validate_clip` restores a video by building
one window per frame (generate_frame_indices, basicsr/data/data_util.py:35-88) - as the reference does (video_base_model.py:44-98).
The network's per-frame stage (`EDVR.extract_features`: conv_first / predeblur, the extraction blocks, the two pyramid convs) then runs
num_frame times on every frame although its result depends on the frame alone.  `VideoRestorer` runs it once per frame into a bounded
feature BANK and builds each chunk of windows by one gather launch (ops.gather_images) over the bank; alignment, fusion and
reconstruction (`EDVR.restore_from_features`) see exactly the tensors a `forward` of `chunk` windows would compute.

Frames of ANY size (`pad_mode`, `tile`): the frame is extended at the bottom and right to the network's size multiple and covered by
equal tiles (`tile_grid`); the per-frame stage reads tiles straight from the caller's frames (ops.crop_pad_frames: crop, pad and the
byte conversion in one launch), every tile has a bank of its own, and the last kernel of each tile's restore pass stores the KEPT
rectangle of its result into the chunk's full-frame output (the `*_rect` tails of csrc/video.hip).  By default nothing is blended:
inside its kept rectangle a tile's result is final, and equals what the plain path computes on that tile's crop.  `tile_blend` cross-fades
neighbouring tiles over a band around each cut instead (`tile_bands`; the `*_rect_blend` tails of csrc/ensemble.hip).

Self-ensemble (`self_ensemble`): the video is restored under each of up to eight symmetries of the square, the symmetry is undone and
the results are averaged.  A symmetry is the same shape of work as a tile - the per-frame stage reads an ORIENTED crop
(ops.crop_pad_frames_d4), every (tile, element) pair has a bank of its own (the per-frame features are not equivariant), and the last
kernel of each pair's restore pass stores the inverse symmetry of its kept rectangle, accumulating over the elements (the `*_rect_d4`
tails of csrc/ensemble.hip).

Temporal reversal (`time_reverse`): every element also runs on the video in reversed frame order.  The window of an output frame in the
reversed video is its forward window reversed, and alignment and temporal attention treat each (neighbour, centre) pair on its own, so
the reversed pass reads the same bank, the same gather and the same aligned features: one attention launch with two outputs
(ops.tsa_temporal_pair) hands the fusion its operand in both frame orders, and only fusion, reconstruction and tail run twice.

No-grad inference only: there is no backward through the bank.
"""
from collections import namedtuple

import torch

from . import ops
from .metrics import generate_frame_indices

_CIRCLE = ('reflection_circle', 'circle')


def window_table(n_frames, num_frame, padding='reflection_circle'):
    """(n_frames, num_frame) int32 table (CPU): row i = generate_frame_indices(i, n_frames, num_frame, padding), the frames of output
    frame i's window.  A video too short for the padding mode (an index outside [0, n_frames)) is a ValueError."""
    rows = [generate_frame_indices(i, n_frames, num_frame, padding) for i in range(n_frames)]
    if any(not 0 <= f < n_frames for r in rows for f in r):
        raise ValueError(f"a video of {n_frames} frame(s) is too short for windows of {num_frame} with '{padding}' padding")
    return torch.tensor(rows, dtype=torch.int32).reshape(n_frames, num_frame)


ENSEMBLES = {'flip4': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}


def ensemble_elements(self_ensemble):
    """None | 'flip4' | 'd4' | a sequence of distinct element ids -> None or the tuple of ids, in the order they run.  Element
    k = 4 t + 2 v + h (t, v, h in {0, 1}) acts on the last two axes: g_k(x) = x.transpose(-1, -2) if t, then .flip(-2) if v, then
    .flip(-1) if h (ops.d4_apply; ops.d4_invert undoes it)."""
    if self_ensemble is None:
        return None
    if isinstance(self_ensemble, str):
        if self_ensemble not in ENSEMBLES:
            raise ValueError(f"self_ensemble must be None, 'flip4', 'd4' or a sequence of element ids 0 ... 7, got {self_ensemble!r}")
        return ENSEMBLES[self_ensemble]
    try:
        ids = tuple(self_ensemble)
    except TypeError:
        raise ValueError(f"self_ensemble must be None, 'flip4', 'd4' or a sequence of element ids 0 ... 7, got {self_ensemble!r}") from None
    if not ids:
        raise ValueError('self_ensemble: an empty sequence of elements (None turns the ensemble off)')
    if any(isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < 8 for k in ids):
        raise ValueError(f'self_ensemble: element ids are integers 0 ... 7 (4 t + 2 v + h), got {ids}')
    if len(set(ids)) != len(ids):
        raise ValueError(f'self_ensemble: element ids must be distinct, got {ids}')
    return ids


Tile = namedtuple('Tile', 'src keep dst')
Tile.__doc__ = """src = (y0, x0, th, tw): the tile in padded-frame coordinates; keep = (ky, kx, kh, kw): the rectangle inside the tile whose
result is final; dst = (oy, ox): where that rectangle lies in the frame (= (y0 + ky, x0 + kx)).  Input pixels throughout."""


def _round_up(v, m):
    return (v + m - 1) // m * m


def _tile_axis(size, padded, tile, overlap, m):
    """One axis: [(origin, first kept, kept count)] of equal tiles of `tile` covering [0, padded), kept parts partitioning [0, size)."""
    if tile >= padded:
        return [(0, 0, size)]
    stride = tile - overlap
    count = -(-(padded - tile) // stride) + 1
    origins = [min(i * stride, padded - tile) for i in range(count)]  # the last tile is shifted inwards, not padded further
    # neighbours share [origins[i + 1], origins[i] + tile) (>= overlap, more for the shifted last tile): cut in its middle, on a multiple of m
    cuts = [0] + [origins[i + 1] + (origins[i] + tile - origins[i + 1]) // (2 * m) * m for i in range(count - 1)] + [size]
    return [(o, cuts[i] - o, cuts[i + 1] - cuts[i]) for i, o in enumerate(origins)]


def tile_grid(H, W, tile=None, overlap=None, multiple=4):
    """Equal tiles covering a frame of (H, W) extended at the bottom and right to the next multiples of `multiple` (pure Python).
    tile = (th, tw) in input pixels, multiples of `multiple`, clamped to the padded frame (None: one tile = the padded frame);
    overlap: input pixels neighbouring tiles share at least - a multiple of 2 * multiple, smaller than the tile (None: 8 * multiple).
    Returns a list of Tile, row by row.  Every source rectangle has the (clamped) tile shape and lies inside the padded frame; the kept rectangles cover the (H, W) frame exactly once; a kept pixel is at least
    overlap / 2 away from every tile edge that is not an edge of the padded frame; origins and cuts are multiples of `multiple`."""
    m = int(multiple)
    if H < 1 or W < 1 or m < 1:
        raise ValueError(f'tile_grid: a frame of {H} x {W}, multiple {m}')
    Hp, Wp = _round_up(H, m), _round_up(W, m)
    if tile is None:
        tile, overlap = (Hp, Wp), 0 if overlap is None else overlap
    th, tw = int(tile[0]), int(tile[1])
    if th < m or tw < m or th % m or tw % m:
        raise ValueError(f'tile {(th, tw)} must be positive multiples of {m}')
    if overlap is None:
        overlap = 8 * m
    overlap = int(overlap)
    if overlap < 0 or overlap % (2 * m):
        raise ValueError(f'tile_overlap {overlap} must be a multiple of {2 * m}')
    if overlap >= min(th, tw):
        raise ValueError(f'tile {(th, tw)} must be larger than tile_overlap {overlap}')
    th, tw = min(th, Hp), min(tw, Wp)
    return [Tile((y0, x0, th, tw), (ky, kx, kh, kw), (y0 + ky, x0 + kx))
            for y0, ky, kh in _tile_axis(H, Hp, th, overlap, m) for x0, kx, kw in _tile_axis(W, Wp, tw, overlap, m)]


TileBlend = namedtuple('TileBlend', 'ext dst bands')
TileBlend.__doc__ = """ext = (ey, ex, eh, ew): the EXTENDED rectangle inside the tile - its kept rectangle plus half a band into each neighbouring
band; dst = (oy, ox): where it lies in the frame; bands = (y low, y high, x low, x high): how many of its first / last rows / columns are
a band shared with the lower- / higher-index neighbour, each 0 or the blend width.  Input pixels throughout."""


def _blend_axis(axis, size, tile, b, name):
    """One axis of tile_bands: `axis` = _tile_axis' [(origin, first kept, kept count)] of tiles of `tile` -> [(first, count, low band,
    high band)] of the extended parts, relative to the tile, after checking that the bands [cut - b / 2, cut + b / 2) are disjoint and
    lie inside the frame."""
    half, count = b // 2, len(axis)
    cuts = [o + k0 for o, k0, _ in axis] + [size]  # cuts[0] = 0; cuts[1 ... count - 1] are the interior ones
    for i in range(1, count):
        if cuts[i + 1] - cuts[i] < (b if i + 1 < count else half) or cuts[i] - cuts[i - 1] < (b if i > 1 else half):
            raise ValueError(f'tile_blend {b}: the {name} cuts {cuts[1:count]} of a frame of {size} leave kept lengths '
                             f'{[cuts[j + 1] - cuts[j] for j in range(count)]}; bands of {b} around the cuts need at least {b} between two '
                             f'cuts and {half} before the first and after the last (a larger tile, a smaller overlap or a smaller tile_blend)')
    out = []
    for i, (o, k0, kn) in enumerate(axis):
        lo, hi = (b if i > 0 else 0), (b if i + 1 < count else 0)
        first, n = k0 - lo // 2, kn + lo // 2 + hi // 2
        assert first >= 0 and first + n <= tile and lo + hi <= n, 'a band reaches outside a tile it blends'  # (b <= overlap)
        out.append((first, n, lo, hi))
    return out


def tile_bands(H, W, tile=None, overlap=None, blend=None, multiple=4):
    """The blending geometry that goes with tile_grid(H, W, tile, overlap, multiple) (pure Python): a list of TileBlend, tile by tile in
    the grid's order.  blend = b: a positive multiple of 2 * multiple, at most the overlap.  Around every interior cut c of an axis lies
    the band [c - b / 2, c + b / 2), inside both neighbouring tiles; a tile stores its kept rectangle extended by b / 2 into each
    neighbouring band.  ValueError where two bands of an axis would meet or a band would leave the (H, W) frame - a kept length between
    two cuts below b or an outer one below b / 2, which happens next to the inward-shifted last tile."""
    m = int(multiple)
    grid = tile_grid(H, W, tile, overlap, m)
    if overlap is None:
        overlap = 8 * m if tile is not None else 0
    if isinstance(blend, bool) or not isinstance(blend, int) or blend <= 0 or blend % (2 * m):
        raise ValueError(f'tile_blend {blend!r} must be a positive multiple of {2 * m}')
    if blend > overlap:
        raise ValueError(f'tile_blend {blend} must not exceed tile_overlap {overlap}')
    Hp, Wp = _round_up(H, m), _round_up(W, m)
    th, tw = grid[0].src[2:]
    rows = _blend_axis(_tile_axis(H, Hp, th, overlap, m), H, th, blend, 'row')
    cols = _blend_axis(_tile_axis(W, Wp, tw, overlap, m), W, tw, blend, 'column')
    out = [TileBlend((ey, ex, eh, ew), None, (ylo, yhi, xlo, xhi)) for ey, eh, ylo, yhi in rows for ex, ew, xlo, xhi in cols]
    return [tb._replace(dst=(t.src[0] + tb.ext[0], t.src[1] + tb.ext[1])) for t, tb in zip(grid, out)]


def band_ramp(B, device=None):
    """r(j), j = 0 ... B - 1: the weight of the higher-index tile across a band of B output pixels - the correctly rounded float32
    quotient of float(2 j + 1) by float(2 B).  The lower-index tile has 1 - r(j) (a float32 subtraction)."""
    return (2 * torch.arange(B, dtype=torch.float32, device=device) + 1) / torch.tensor(float(2 * B), dtype=torch.float32, device=device)


class WindowSchedule:
    """Which frames to extract and which output frames to restore, as frames of a video of UNKNOWN length arrive (pure Python).

    push(k) - k more frames have arrived - and finish() generate steps in execution order (the state below advances with them):
        ('extract', first, count)   run the per-frame stage on frames [first, first + count) (each frame exactly once, in order)
        ('restore', first, rows)    restore output frames first, first + 1, ...; rows[j] = the window of output frame first + j
    After a step, frames below `lo` are dead.  A window whose far end lies `num_frame // 2` frames ahead is known as soon as that frame
    has arrived (the padding of the first frames reads forward only: up to frame num_frame - 1 in the circle modes); the last
    num_frame // 2 windows depend on the length and come from finish().  Output frames leave in groups of `chunk` (what is left at the
    end in up to two smaller ones), so the launches of a group have the shapes of a forward with b = chunk.

    What stays alive: the frames the next group's windows reach back to (num_frame // 2 behind its first frame) and - the video may end
    with the latest frame, and the circle modes then reach num_frame - 1 frames back from it - the latest num_frame extracted frames.
    `capacity` is the largest number of live frames any length produces (found by running the schedule itself over short and long
    videos; it never exceeds chunk + 2 * (num_frame - 1)): the size of the ring the bank is kept in."""

    def __init__(self, num_frame, padding='reflection_circle', chunk=8, _probe=True):
        if num_frame < 1 or num_frame % 2 == 0:
            raise ValueError(f'num_frame must be odd, got {num_frame}')
        if padding not in ('replicate', 'reflection', 'reflection_circle', 'circle'):
            raise ValueError(f'Wrong padding mode: {padding}.')
        if chunk < 1:
            raise ValueError(f'chunk must be at least 1, got {chunk}')
        self.t, self.p, self.padding, self.chunk = num_frame, num_frame // 2, padding, int(chunk)
        self.back = num_frame - 1 if (padding in _CIRCLE and num_frame > 1) else self.p  # how far the last windows reach back from the last frame
        self.arrived = self.ext = self.out = self.lo = 0
        self.peak = 0
        if _probe:
            limit = self.chunk + 2 * (num_frame - 1)
            self.capacity = max(self._peak_of(n) for n in range(num_frame, 3 * (self.chunk + num_frame) + 2))
            assert self.capacity <= max(limit, 1), (self.capacity, limit)

    def _peak_of(self, n):
        s = WindowSchedule(self.t, self.padding, self.chunk, _probe=False)
        for _ in range(n):
            for _step in s.push(1):
                pass
        for _step in s.finish():
            pass
        return s.peak

    def _complete(self, i):
        """Is the window of output frame i known and present (without knowing the length)?"""
        need = i + self.p
        if i < self.p and self.padding in _CIRCLE:
            need = max(need, self.t - 1)
        return need <= self.arrived - 1

    def _group(self, first, rows):
        hi = max(max(r) for r in rows)
        if hi >= self.ext:
            step = ('extract', self.ext, hi + 1 - self.ext)
            self.ext = hi + 1
            self.peak = max(self.peak, self.ext - self.lo)
            yield step
        assert min(min(r) for r in rows) >= self.lo, 'a window reaches behind the live frames'
        yield ('restore', first, rows)
        self.out = first + len(rows)
        keep = self.out - self.p
        if self.back > self.p:
            keep = min(keep, self.ext - 1 - self.back)
        self.lo = max(self.lo, min(keep, self.ext))

    def push(self, k=1):
        """k more frames have arrived: a generator of the steps that have become possible (the state advances as it is consumed)."""
        self.arrived += int(k)
        while self._complete(self.out + self.chunk - 1):
            first = self.out
            rows = [generate_frame_indices(i, self.arrived, self.t, self.padding) for i in range(first, first + self.chunk)]
            yield from self._group(first, rows)

    def finish(self):
        """The input has ended: the steps for the output frames still owed."""
        n = self.arrived
        if self.out < n:
            table = window_table(n, self.t, self.padding).tolist()
            while self.out < n:
                first = self.out
                yield from self._group(first, table[first:min(first + self.chunk, n)])


class VideoRestorer:
    """Restore whole videos with `net` (an EDVR in eval mode, on the GPU), extracting every frame's features once.

        vr = VideoRestorer(net, padding='reflection_circle', chunk=8)
        out = vr.restore(lq)                       # (N, 3, H, W) float32 in [0, 1] or (N, H, W, 3) uint8 -> all N restored frames
        for frame in vr.restore_iter(frames): ...  # streaming: frames (or small batches of them) in, restored frames out, in order

    num_frame: the network's window (None: read from its fusion layer); padding: generate_frame_indices' mode for the first and last
    frames; chunk: output frames per alignment / fusion / reconstruction pass (= `validate_clip`'s batch);
    out_dtype: torch.float32 -> (N, 3, H', W') as `forward` returns them, torch.uint8 -> (N, H', W', 3) bytes with tensor2img
    semantics (clamp, x 255, round half to even), written by the network's last kernel.

    The bank holds the three pyramid levels of at most `capacity` <= chunk + 2 * (num_frame - 1) frames whatever the length of the
    video; the input frames are kept (as views of what the caller handed in, or as the converted uint8 pieces) until no window's
    centre needs them.  Around every chunk the bookkeeping of a forward happens: offset statistics and overflow flags of earlier
    chunks that have reached the host are examined before, this chunk's are sent after; nothing waits for the GPU -
    `net.check_offsets()` after the last chunk evaluates what is still on its way, as after a run of forwards.

    Frames of any size - opt-in; with the defaults the size must be a multiple of m = 4 (16 with hr_in) and nothing above changes:
    pad_mode 'reflect' | 'replicate': frames of (H, W) are extended at the bottom and right to the next multiples of m with
    torch.nn.functional.pad's rule, the output is the first (s H, s W) pixels (s = 4, or 1 with hr_in) of the network's result.
    tile (th, tw), tile_overlap (input pixels; None: 8 m): the padded frame is covered by equal tiles (`tile_grid`), each with a bank of
    its own (same ring, same capacity); an extract step runs the per-frame stage tile by tile, a restore step everything else tile by
    tile, each tile's last kernel storing its kept rectangle into the chunk's full-frame output - bit for bit what this class computes on
    that tile's crop of the padded frames.  Near the cuts the result differs from the untiled one (the network's receptive field is
    larger than any sensible overlap); what shrinks is the memory of everything after the gather, by about the tiles' share of the frame.
    Either argument turns the tiled path on: uint8 frames then stay bytes (no full-frame float copy), all pieces must share one dtype.

    self_ensemble None | 'flip4' (elements 0 ... 3: the flips) | 'd4' (0 ... 7: flips and the transpose) | a sequence of distinct
    element ids k = 4 t + 2 v + h, run in the order given (`ensemble_elements`).  With P the bottom / right extension of pad_mode in the
    frame's own orientation, R what this class computes without the argument (float32; on a tile's crop in the tiled path) and g_k the
    symmetry,
        acc = g_k0^-1(R(g_k0(P(lq))));  acc = acc + g_ki^-1(R(g_ki(P(lq)))) for i = 1 ... n - 1, in that order, in float32
        out = crop(acc * (1 / n))       (uint8 output: the tensor2img bytes of that value)
    It turns the tiled path on as well and composes with pad_mode and tile (the symmetry acts on each tile's crop).  The work list is
    (tile x element), element innermost; windows, temporal padding and chunking are untouched (no temporal reversal).
    WHAT IT COSTS: n times the time of the plain path (every kernel of the network runs once per element; the new oriented reads and
    accumulating tails are bandwidth-sized) and n banks per tile (same ring, same capacity each), plus - with uint8 output - one
    float32 (chunk, 3, s H, s W) accumulator that lives across chunks.  A transposing element runs the network on (W, H) frames.

    tile_blend None | b (input pixels; needs tile; a positive multiple of 2 m, at most tile_overlap): neighbouring tiles are cross-faded
    over a band instead of being cut.  Around every interior cut c of an axis lies the band [c - b / 2, c + b / 2) (`tile_bands`; bands
    of an axis that would meet, or a band outside the frame, are a ValueError at the first frame); a tile stores its kept rectangle
    extended by b / 2 into each neighbouring band.  With B = s b and j = 0 ... B - 1 the output pixel of a band in the frame's orientation,
        r(j) = float32(2 j + 1) / float32(2 B)     the higher-index tile's weight; the lower-index tile has 1.0f - r(j); 1.0f off the bands
        w = w_y * w_x                              (all float32, round to nearest; four tiles meet in a corner)
    and over a pixel's contributors in work-list order (tiles row-major, element innermost), v being the float32 the unblended path
    stores for that tile (and element) there,
        acc = w * v;  acc = acc + w * v ...;  with an ensemble of n the last stores (acc + w * v) * (1 / n)
    each product rounded before its add.  Without an ensemble a pixel outside every band is bit for bit the unblended tiled result.
    No network work is added - the bands are computed by both tiles already; the tails turn from stores into read-modify-writes inside
    the bands, and uint8 output keeps the float32 (chunk, 3, s H, s W) accumulator an ensemble needs.

    time_reverse False | True: every spatial element g_k ((0,) when self_ensemble is None) also runs on the video in reversed frame order.
    With rev(v) = v.flip(0) and P, R, g_k as above, per tile, in float32,
        terms, in this order:  for k in elements:  g_k^-1(R(g_k(P(lq)))),  then  g_k^-1(rev(R(rev(g_k(P(lq))))))
        acc = first term;  acc = acc + next term ...;  out = crop(acc * (1 / (2 n)))        (n = len(elements))
    through the accumulating tails of self_ensemble (first / middle / last by the position 2 e + r of 2 n; the identity element when
    there is no spatial ensemble; with tile_blend their weighted forms, the two time orders adjacent in the work-list order); uint8
    output is the tensor2img bytes of that value, accumulated in the tagged float32 scratch.  It turns the tiled path on; windows,
    temporal padding, chunking, bank capacity and streaming are unchanged, and `pairs` / `banks` stay (tile x spatial element).
    share_alignment (needs time_reverse; default True): output frame i's window in the reversed video is its forward window reversed
    (every padding mode), PCD aligns image j with the centre frame and nothing else, and the attention map of image j likewise - so per
    (tile, element) and chunk there is ONE gather and ONE EDVR.align_windows(pair=True), whose attention kernel stores the modulated
    features in both frame orders, then two EDVR.restore_from_aligned calls (fusion, reconstruction, upsampling, tail).  Offset
    statistics are queued once (the DCNs ran once), the overflow guard after each tail.  False: the plain implementation - a second
    gather with every row of the slot table reversed and a second EDVR.restore_from_features - kept as the in-tree cross-check (the arms
    are bit-identical in the tests) and as a fallback.
    WHAT IT COSTS: shared, 2 x fusion, reconstruction and upsampling and 1 x alignment and attention per element (by the module
    definitions about 15 of 115 conv-units per output frame saved for each of the T frames of a window; DESIGN 4.10 has the
    measurement), the second copy of the modulated features (chunk x T x C x h x w float32) while the first tail runs, no further bank;
    unshared, 2 x everything after the per-frame stage.  With uint8 output the float32 accumulator, as with an ensemble.

    cuts None | 'auto' | a strictly increasing sequence of frame indices c_1 < ... < c_k (frame c_j begins a new shot): windows stay
    inside a shot.  The result is the concatenation of what this configuration WITHOUT cuts returns for each shot [c_j, c_(j+1))
    restored as a video of its own - its own temporal padding, chunks (the last ones of a shot may be short, no chunk straddles a cut)
    and temporal reversal; every other argument only ever sees one shot.  'auto' finds the cuts: ops.frame_sad measures
    the 8-bit luma change between consecutive frames, shots.cut_scores turns it into ffmpeg's scene score on the 0 ... 255 scale, and
    a frame scoring at least cut_threshold (default 10.0) begins a shot unless that would leave a shot shorter than min_shot (default
    and lower bound max(num_frame, 2): what the circle paddings ask of a video) - shots.select_cuts.  Explicit cuts are checked
    against the same lower bound: ValueError at construction, for the last shot where the length becomes known (`restore`: before any
    launch; a stream: at its end); cut_threshold / min_shot without cuts='auto' likewise.  After a run `cuts_found` holds the cuts,
    with 'auto' `cut_scores` and `cut_mafd` every frame's score and mean absolute difference.
    WHERE THE HOST WAITS: explicit cuts - nowhere; 'auto' in `restore` - once, up front, for one launch over the whole video; 'auto'
    on a stream - per arriving piece for its 8 k bytes, behind an event recorded right after that piece's frame_sad, i.e. before any
    restoration work the piece leads to; the restorer pulls ONE piece ahead (measures piece p + 1 before it waits for piece p's
    numbers), so that this event also lies ahead of the work of piece p - 1 and the GPU does not drain at every piece.  Beyond
    today's, at most min_shot - 1 decided-upon frames and that one piece are held (as views of the caller's pieces)."""

    def __init__(self, net, num_frame=None, padding='reflection_circle', chunk=8, out_dtype=torch.float32, pad_mode=None, tile=None,
                 tile_overlap=None, self_ensemble=None, tile_blend=None, time_reverse=False, share_alignment=None, cuts=None,
                 cut_threshold=None, min_shot=None):
        if out_dtype not in (torch.float32, torch.uint8):
            raise ValueError(f'out_dtype must be torch.float32 or torch.uint8, got {out_dtype}')
        if pad_mode not in (None, 'reflect', 'replicate'):
            raise ValueError(f"pad_mode must be None, 'reflect' or 'replicate', got {pad_mode!r}")
        self.multiple, self.scale = (16, 1) if net.hr_in else (4, 4)
        if tile is not None:
            tile_grid(self.multiple, self.multiple, tile, tile_overlap, self.multiple)  # argument errors now, not at the first frame
            tile = (int(tile[0]), int(tile[1]))
        elif tile_overlap is not None:
            raise ValueError('tile_overlap without tile')
        if tile_blend is not None:
            if tile is None:
                raise ValueError('tile_blend without tile')
            tile_bands(self.multiple, self.multiple, tile, tile_overlap, tile_blend, self.multiple)  # its argument errors now as well
        self.pad_mode, self.tile, self.tile_overlap, self.tile_blend = pad_mode, tile, tile_overlap, tile_blend
        self.elements = ensemble_elements(self_ensemble)
        if not isinstance(time_reverse, bool):
            raise ValueError(f'time_reverse must be True or False, got {time_reverse!r}')
        if share_alignment is not None and not isinstance(share_alignment, bool):
            raise ValueError(f'share_alignment must be True or False, got {share_alignment!r}')
        if share_alignment is not None and not time_reverse:
            raise ValueError('share_alignment chooses how the reversed pass of time_reverse runs: it needs time_reverse=True')
        self.time_reverse, self.share_alignment = time_reverse, time_reverse and share_alignment is not False
        self.tiled = pad_mode is not None or tile is not None or self.elements is not None or time_reverse
        self.net, self.padding, self.chunk, self.out_dtype = net, padding, int(chunk), out_dtype
        self.num_feat = net.conv_l2_1.in_channels
        if num_frame is None:
            fusion = net.fusion.feat_fusion if getattr(net, 'with_tsa', True) else net.fusion
            num_frame = fusion.in_channels // self.num_feat
        self.num_frame = int(num_frame)
        ctr = getattr(net, 'center_frame_idx', self.num_frame // 2)
        if ctr != self.num_frame // 2:
            raise ValueError(f'windows are centred on the frame they restore: center_frame_idx {ctr} != num_frame // 2 = {self.num_frame // 2}')
        self.capacity = WindowSchedule(self.num_frame, padding, self.chunk).capacity
        # scene cuts: None | 'auto' | a checked list; a shot is never shorter than what window_table asks of a video in the circle modes
        floor = max(self.num_frame, 2)
        auto = isinstance(cuts, str) and cuts == 'auto'
        if not auto and (cut_threshold is not None or min_shot is not None):
            raise ValueError("cut_threshold and min_shot steer the detector: they need cuts='auto'")
        if min_shot is not None and (isinstance(min_shot, bool) or not isinstance(min_shot, int) or min_shot < floor):
            raise ValueError(f'min_shot must be an integer of at least max(num_frame, 2) = {floor}, got {min_shot!r}')
        self.min_shot = floor if min_shot is None else min_shot
        self.cut_threshold = 10.0 if cut_threshold is None else float(cut_threshold)
        if self.cut_threshold != self.cut_threshold:
            raise ValueError('cut_threshold is NaN')
        if cuts is not None and not auto:
            if isinstance(cuts, str):
                raise ValueError(f"cuts must be None, 'auto' or a strictly increasing sequence of frame indices, got {cuts!r}")
            from .shots import check_cuts
            cuts = check_cuts(cuts, self.min_shot)
        self.cuts = cuts
        self.cuts_found = None  # after a run with cuts: the cuts, in order; and with 'auto' ...
        self.cut_scores = None  # ... every frame's score ...
        self.cut_mafd = None    # ... and mean absolute frame difference (shots.cut_scores)
        self.bank = None       # [f1, f2, f3] rings of `slots` images; frame f lives in image f % slots
        self.slots = 0
        self.schedule = None    # the WindowSchedule of the running restore
        self._groups = []       # (first frame, count, [bound or None per level], [depth per level]) of every extract call with live frames
        self._pieces = []       # (first frame, float32 (k, 3, H, W)) input frames not dead yet (tiled path: as they came, uint8 (k, H, W, 3) too)
        self.grid = None        # tiled path: [Tile] of the running restore, and per tile ...
        self.blend_grid = None  # ... with tile_blend its TileBlend, ...
        self.pairs = None       # ... the work list [(Tile, element id or None)]: tile x element, element innermost, and per pair ...
        self.banks = None       # ... its [f1, f2, f3] rings
        self._tile_groups = None  # ... and its _groups

    # ---- device primitives (the schedule test replaces them by CPU stand-ins)
    def _check_input(self, t):
        if not t.is_cuda:
            raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')

    def _slot_table(self, slots, device):
        host = torch.tensor(slots, dtype=torch.int32).pin_memory()  # (pinned + non_blocking: the host does not wait for the stream)
        return host.to(device, non_blocking=True)

    def _gather(self, srcs, table):
        return ops.gather_images(srcs, table)

    def _crop(self, frames, y0, x0, th, tw):
        """The tile at (y0, x0) of `frames` (uint8 HWC or float32 CHW) extended by pad_mode, as float32 (k, 3, th, tw)."""
        return ops.crop_pad_frames(frames, y0, x0, th, tw, self.pad_mode)

    def _crop_d4(self, frames, y0, x0, th, tw, elem):
        """ops.d4_apply(self._crop(...), elem) in one launch: the oriented tile a self-ensemble element reads."""
        return ops.crop_pad_frames_d4(frames, y0, x0, th, tw, self.pad_mode, elem)

    def _scratch(self, shape, device):
        """The float32 accumulator of a chunk with uint8 output: a grow-only buffer of its own (ops.workspace under a tag - the
        untagged one is the kernels' scratch and is rewritten by the launches between two elements)."""
        count = 1
        for d in shape:
            count *= d
        return ops.workspace(4 * count, device, tag='self_ensemble')[:4 * count].view(torch.float32).view(shape)

    def _oriented(self, frames, tile, elem):
        return self._crop(frames, *tile.src) if elem is None else self._crop_d4(frames, *tile.src, elem)

    # ---- input
    def _check_mode(self):
        if self.net.training:
            raise RuntimeError('VideoRestorer is an inference path: put the network in eval() mode')
        if torch.is_grad_enabled():
            raise RuntimeError('VideoRestorer has no backward (features are written into a bank in place): call it under torch.no_grad()')

    def _as_frames(self, item):
        """One frame or a batch of frames, float32 CHW in [0, 1] or uint8 HWC -> float32 (k, 3, H, W)."""
        self._check_input(item)
        if item.dtype == torch.uint8:
            if item.dim() == 3:
                item = item[None]
            if item.dim() != 4 or item.shape[-1] != 3:
                raise ValueError(f'uint8 frames are (H, W, 3) or (k, H, W, 3), got {tuple(item.shape)}')
            if self.tiled:
                return item  # the tiles are read from the bytes (ops.crop_pad_frames): no full-frame float copy
            return ops.frames_u8_to_f32(item[None])[0]
        if item.dtype != torch.float32:
            raise NotImplementedError(f'edvr_amd: {item.dtype} frames are not supported here (float32 CHW in [0, 1] or uint8 HWC)')
        if item.dim() == 3:
            item = item[None]
        if item.dim() != 4:
            raise ValueError(f'float32 frames are (3, H, W) or (k, 3, H, W), got {tuple(item.shape)}')
        return item

    def _frames(self, a, b):
        """Input frames [a, b) as one (b - a, 3, H, W) tensor: a view where one piece holds them all."""
        parts = []
        for first, piece in self._pieces:
            lo, hi = max(a, first), min(b, first + piece.shape[0])
            if lo < hi:
                parts.append(piece[lo - first:hi - first])
        assert sum(p.shape[0] for p in parts) == b - a, f'input frames [{a}, {b}) are not all held'
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)

    # ---- bank
    def _pyramid_shapes(self, h, w):
        net = self.net
        if net.hr_in:
            assert h % 16 == 0 and w % 16 == 0, 'The height and width must be multiple of 16.'
        else:
            assert h % 4 == 0 and w % 4 == 0, 'The height and width must be multiple of 4.'
        if net.hr_in and net.with_predeblur:
            h, w = h // 4, w // 4
        h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return [(self.num_feat, h, w), (self.num_feat, h2, w2), (self.num_feat, (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1)]

    @property
    def bank_frames(self):
        """Frames the bank holds right now (extracted and not dead)."""
        return 0 if self.schedule is None else self.schedule.ext - self.schedule.lo

    def _extract(self, first, count, length):
        frames = self._frames(first, first + count)
        if self.bank is None:
            self.slots = self.capacity if length is None else max(1, min(self.capacity, length))
            self.bank = [torch.empty((self.slots,) + s, dtype=torch.float32, device=frames.device)
                         for s in self._pyramid_shapes(frames.shape[2], frames.shape[3])]
        self._extract_into(self.bank, self._groups, frames, first, count)

    def _extract_into(self, bank, groups, frames, first, count):
        if self.schedule.ext - self.schedule.lo > self.slots:
            raise RuntimeError(f'VideoRestorer: {self.schedule.ext - self.schedule.lo} live frames do not fit the bank of {self.slots}')
        done = 0
        while done < count:  # a group that crosses the end of the ring is extracted in two parts
            slot = (first + done) % self.slots
            m = min(count - done, self.slots - slot)
            pyr = self.net.extract_features(frames[done:done + m], out=[lv[slot:slot + m] for lv in bank])
            bounds = [ops.get_bound(f) for f in pyr]
            groups.append((first + done, m, bounds, [ops._bound_depth(f) if b is not None else 0 for f, b in zip(pyr, bounds)]))
            done += m

    def _bank_bounds(self, bank=None, groups=None):
        """The bank's magnitude bound per level = the largest bound of the live extract groups (none where a group has none)."""
        bank, groups = (self.bank, self._groups) if bank is None else (bank, groups)
        lo = self.schedule.lo
        groups[:] = [g for g in groups if g[0] + g[1] > lo]
        for lv, level in enumerate(bank):
            bs = [g[2][lv] for g in groups]
            ops.void_bound(level)
            if bs and all(b is not None for b in bs):
                b = bs[0]
                for o in bs[1:]:
                    b = torch.maximum(b, o)
                ops.set_bound(level, b, max(g[3][lv] for g in groups))

    def _restore(self, first, rows):
        net, t = self.net, self.num_frame
        net.check_offsets(wait=False)  # what a forward does before its launches: statistics / overflow flags that have landed
        if self.bank[0].is_cuda:
            ops.split_guard_check(wait=False)
        self._bank_bounds()
        table = self._slot_table([f % self.slots for r in rows for f in r], self.bank[0].device)
        pyr = self._gather(self.bank, table)
        return net.restore_from_features(pyr, self._frames(first, first + len(rows)), len(rows), t, out_dtype=self.out_dtype)

    # ---- frames of any size: edge padding and tiles
    def _frame_size(self, frames):
        return tuple(frames.shape[1:3]) if frames.dtype == torch.uint8 else tuple(frames.shape[2:4])

    def _setup_tiles(self, frames, length):
        H, W = self._frame_size(frames)
        m = self.multiple
        if self.pad_mode is None:  # tiles alone: the size rule of the plain path
            assert H % m == 0 and W % m == 0, f'The height and width must be multiple of {m}.'
        Hp, Wp = _round_up(H, m), _round_up(W, m)
        if self.pad_mode == 'reflect' and (Hp - H > H - 1 or Wp - W > W - 1):
            raise ValueError(f"pad_mode='reflect' mirrors without repeating the edge: a frame of {H} x {W} is too small to be extended to {Hp} x {Wp}")
        self.grid = tile_grid(H, W, self.tile, self.tile_overlap, m)
        self.blend_grid = None if self.tile_blend is None else tile_bands(H, W, self.tile, self.tile_overlap, self.tile_blend, m)
        th, tw = self.grid[0].src[2:]
        self.slots = self.capacity if length is None else max(1, min(self.capacity, length))
        self.pairs = [(tile, k) for tile in self.grid for k in (self.elements or (None,))]
        # (a transposing element's network runs on (tw, th) tiles)
        self.banks = [[torch.empty((self.slots,) + s, dtype=torch.float32, device=frames.device)
                       for s in (self._pyramid_shapes(tw, th) if k is not None and k & 4 else self._pyramid_shapes(th, tw))]
                      for _, k in self.pairs]
        self._tile_groups = [[] for _ in self.pairs]

    def _extract_tiled(self, first, count, length):
        frames = self._frames(first, first + count)
        if self.banks is None:
            self._setup_tiles(frames, length)
        for (tile, k), bank, groups in zip(self.pairs, self.banks, self._tile_groups):
            self._extract_into(bank, groups, self._oriented(frames, tile, k), first, count)

    def _restore_tiled(self, first, rows):
        net, t, s, b = self.net, self.num_frame, self.scale, len(rows)
        centre = self._frames(first, first + b)
        H, W = self._frame_size(centre)
        u8 = self.out_dtype == torch.uint8
        out = torch.empty((b, s * H, s * W, 3) if u8 else (b, 3, s * H, s * W), dtype=self.out_dtype, device=centre.device)
        table = self._slot_table([f % self.slots for r in rows for f in r], centre.device)
        n = len(self.elements) if self.elements is not None else 0
        blend = self.blend_grid
        rev = self.time_reverse
        terms = 2 * max(n, 1) if rev else n  # what adds up per tile: the elements, each in both time orders with time_reverse
        table_rev = None
        if rev and not self.share_alignment:  # the plain arm: the same bank, every window's frames in reversed order
            table_rev = self._slot_table([f % self.slots for r in rows for f in reversed(r)], centre.device)
        # uint8 output: the elements, the two time orders (and blended tiles) add up in float32
        acc = self._scratch((b, 3, s * H, s * W), centre.device) if (terms or blend is not None) and u8 else None
        for i, ((tile, k), bank, groups) in enumerate(zip(self.pairs, self.banks, self._tile_groups)):
            net.check_offsets(wait=False)  # per tile (and element) what a forward does before its launches, as in _restore
            if bank[0].is_cuda:
                ops.split_guard_check(wait=False)
            self._bank_bounds(bank, groups)
            pyr = self._gather(bank, table)
            (ky, kx, kh, kw), (oy, ox) = tile.keep, tile.dst
            if blend is not None:  # the extended rectangle instead of the kept one
                (ky, kx, kh, kw), (oy, ox), bands = blend[i // max(n, 1)]
            ys, xs = slice(s * oy, s * (oy + kh)), slice(s * ox, s * (ox + kw))
            how = {}
            if k is not None:  # the oriented, accumulating tail: the float32 output accumulates in place, the bytes in `acc`
                e = i % n
                how = dict(elem=k, accumulate='only' if n == 1 else 'first' if e == 0 else 'last' if e == n - 1 else 'middle', scale=1.0 / n,
                           acc=acc[:, :, ys, xs] if u8 else None)
            if blend is not None:  # the weighted tail (identity element without an ensemble)
                how.update(bands=tuple(s * v for v in bands), acc=acc[:, :, ys, xs] if u8 else None)
            how.update(out_dtype=self.out_dtype, out=out[:, ys, xs] if u8 else out[:, :, ys, xs], keep=(s * ky, s * kx))
            x_center = self._oriented(centre, tile, k)
            if not rev:
                net.restore_from_features(pyr, x_center, b, t, **how)
                continue
            # time_reverse: this pair's two terms, positions 2 e and 2 e + 1 of `terms`, through the accumulating tails (the identity
            # element without a spatial ensemble).  A window's centre frame is the same in both time orders.
            e = i % max(n, 1)
            mode = lambda pos: 'first' if pos == 0 else 'last' if pos == terms - 1 else 'middle'
            how.update(elem=0 if k is None else k, scale=1.0 / terms, acc=acc[:, :, ys, xs] if u8 else None)
            if self.share_alignment:  # one alignment and one attention pass give the fusion's operand in both orders
                mod, mod_rev, sink = net.align_windows(pyr, b, t, pair=True)
                del pyr
                net.restore_from_aligned(mod, x_center, b, t, sink=sink, **dict(how, accumulate=mode(2 * e)))
                del mod
                net.restore_from_aligned(mod_rev, x_center, b, t, **dict(how, accumulate=mode(2 * e + 1)))
                del mod_rev
            else:
                net.restore_from_features(pyr, x_center, b, t, **dict(how, accumulate=mode(2 * e)))
                del pyr
                net.restore_from_features(self._gather(bank, table_rev), x_center, b, t, **dict(how, accumulate=mode(2 * e + 1)))
        return out

    # ---- public
    def _run(self, steps, length):
        for kind, first, arg in steps:
            self._check_mode()
            if kind == 'extract':
                (self._extract_tiled if self.tiled else self._extract)(first, arg, length)
            else:
                out = (self._restore_tiled if self.tiled else self._restore)(first, arg)
                nxt = first + len(arg)  # input frames are read by their extraction and as their own output's residual base
                self._pieces = [(f, p) for f, p in self._pieces if f + p.shape[0] > nxt]
                yield out

    # one shot = one video: a fresh schedule, bank(s) and piece list (_begin_shot), frames in (_feed), the end (_end_shot), clean-up (_clear)
    def _begin_shot(self):
        self.schedule = WindowSchedule(self.num_frame, self.padding, self.chunk, _probe=False)
        self.bank, self._groups, self._pieces = None, [], []
        self.grid = self.blend_grid = self.pairs = self.banks = self._tile_groups = None

    def _feed(self, piece, length):
        """`piece` (what _as_frames returned; with cuts a view of it that ends at the cut) joins the running shot."""
        if self.tiled and self._pieces and piece.dtype != self._pieces[-1][1].dtype:
            raise ValueError(f'the frames of one video share one dtype: {piece.dtype} after {self._pieces[-1][1].dtype}')
        self._pieces.append((self.schedule.arrived, piece))
        yield from self._run(self.schedule.push(piece.shape[0]), length)

    def _end_shot(self, length):
        yield from self._run(self.schedule.finish(), length)

    def _clear(self):
        self.bank, self._groups, self._pieces = None, [], []  # (the schedule and the tile grid stay for inspection)
        self.banks = self._tile_groups = None

    def restore_chunks(self, frames, length=None):
        """restore_iter that yields each chunk's output tensor ((b, 3, H', W') or (b, H', W', 3)) instead of single frames.
        length: the number of frames if known - a video shorter than `capacity` then gets a smaller bank."""
        self._check_mode()
        if self.cuts is not None:
            yield from self._restore_shots(frames, length, self.cuts)
            return
        self._begin_shot()
        try:
            for item in frames:
                piece = self._as_frames(item)
                if piece.shape[0] == 0:
                    continue
                yield from self._feed(piece, length)
            yield from self._end_shot(length)
        finally:
            self._clear()

    # ---- scene cuts: every shot is a video of its own
    def _sad_to_host(self, piece, prev):
        """ops.frame_sad of an arriving piece against the last frame before it, on its way into pinned memory: (host int64 (k,), event).
        Launched BEFORE any restoration work the piece leads to, so the event waits for nothing that comes after the piece."""
        sad = ops.frame_sad(piece, prev)
        host = torch.empty(sad.shape, dtype=torch.int64, pin_memory=True)
        host.copy_(sad, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return host, event

    def _wait_sad(self, host, event):
        event.synchronize()  # the one place the host waits with cuts='auto'
        return host.tolist()

    def _restore_shots(self, frames, length, cuts):
        """restore_chunks with cuts: the pieces are split at the cuts, each shot runs through _begin_shot / _feed / _end_shot as a video
        of its own (its own temporal padding, chunks and - per tile and element - banks), and no chunk straddles a cut.  cuts: a checked
        list, or 'auto' - then an arriving piece is measured (ops.frame_sad against the last frame of the piece before, which is kept
        alive) as soon as it is pulled, one piece ahead of the one being decided, a ShotDetector decides, and a frame joins its shot
        once no undecided candidate precedes it (at most min_shot - 1 frames wait, as views of the caller's pieces)."""
        from .shots import ShotDetector, check_cuts
        auto = isinstance(cuts, str)
        det = ShotDetector(self.cut_threshold, self.min_shot) if auto else None
        if not auto and length is not None:
            check_cuts(cuts, self.min_shot, int(length))  # the last shot too, before any launch
        self.cuts_found, self.cut_scores, self.cut_mafd = [], ([] if auto else None), ([] if auto else None)
        pending = list(cuts) if not auto else []  # cuts not reached yet
        held = []        # (first frame, piece): arrived frames that have not joined a shot yet
        arrived = fed = start = 0
        last = None      # auto: the last frame that arrived
        dtype = None

        def shot_length(begin):
            if auto or length is None:
                return None
            return (pending[0] if pending else int(length)) - begin

        def release(upto, new_cuts):
            """frames [fed, upto) join their shots; new_cuts: the cuts among them (each ends the running shot)"""
            nonlocal fed, start, held
            stops = [c for c in new_cuts if fed <= c <= upto] + [upto]  # (a cut at `fed`: the piece before ended where the shot does)
            for stop in stops:
                for first, piece in held:
                    lo, hi = max(fed, first), min(stop, first + piece.shape[0])
                    if lo < hi:
                        yield from self._feed(piece[lo - first:hi - first], shot_length(start))
                fed = max(fed, stop)
                if stop in new_cuts:
                    yield from self._end_shot(shot_length(start))
                    self._clear()
                    self.cuts_found.append(stop)
                    if pending and pending[0] == stop:
                        pending.pop(0)
                    start = stop
                    self._begin_shot()
            held = [(f, p) for f, p in held if f + p.shape[0] > fed]

        def pieces():
            nonlocal dtype
            for item in frames:
                piece = self._as_frames(item)
                if piece.shape[0] == 0:
                    continue
                if dtype is not None and piece.dtype != dtype:
                    raise ValueError(f'the frames of one video share one dtype: {piece.dtype} after {dtype}')
                dtype = piece.dtype
                yield piece

        def measured():
            """auto: (piece, host, event) - a piece leaves when the piece AFTER it has been pulled and measured (or the input has ended),
            so its event lies ahead of the restoration work of the piece before it in the stream: the host's wait for it ends while
            that work still runs, and the GPU does not drain at every piece."""
            nonlocal last
            ahead = None
            for piece in pieces():
                now = (piece,) + self._sad_to_host(piece, last)
                last = piece[-1]
                if ahead is not None:
                    yield ahead
                ahead = now
            if ahead is not None:
                yield ahead

        self._begin_shot()
        try:
            for item in (measured() if auto else pieces()):
                piece = item[0] if auto else item
                held.append((arrived, piece))
                arrived += piece.shape[0]
                if auto:
                    size = self._frame_size(piece) if piece.dtype == torch.uint8 else tuple(piece.shape[2:4])
                    new = det.push_sad(self._wait_sad(*item[1:]), size[0] * size[1])
                    upto = det.released
                else:
                    new = [c for c in pending if c < arrived]  # a cut at `arrived` is acted on when its frame is here
                    upto = arrived
                yield from release(upto, new)
            if auto:
                new = det.finish()
                self.cut_scores, self.cut_mafd = list(det.scores), list(det.mafd)
            else:
                new = []
                check_cuts(cuts, self.min_shot, arrived)  # the stream has ended: cuts beyond it, or a last shot too short
            if arrived:
                yield from release(arrived, new)
                yield from self._end_shot(shot_length(start))
        finally:
            if auto:
                self.cut_scores, self.cut_mafd = list(det.scores), list(det.mafd)
            self._clear()

    def restore_iter(self, frames, length=None):
        """Streaming form: `frames` is an iterable of frames ((3, H, W) float32 / (H, W, 3) uint8) or of small batches of them, of
        unknown length; yields the restored frames in order, each as soon as its chunk of windows is complete - the last
        num_frame // 2 (whose padding depends on the length) when the input ends."""
        for out in self.restore_chunks(frames, length):
            yield from out.unbind(0)

    def restore(self, lq):
        """lq: (N, 3, H, W) float32 in [0, 1] or (N, H, W, 3) uint8, on the GPU -> all N restored frames."""
        self._check_mode()
        self._check_input(lq)
        if lq.dim() != 4:
            raise ValueError(f'expected (N, 3, H, W) float32 or (N, H, W, 3) uint8 frames, got {tuple(lq.shape)}')
        if lq.shape[0] == 0:
            raise ValueError('restore: no frames')
        n = lq.shape[0]
        if self.cuts is None:
            outs = list(self.restore_chunks(lq.split(self.chunk), length=n))
        else:
            from .shots import check_cuts, cut_scores, select_cuts
            if self.cuts == 'auto':  # the length is known: one launch over the whole video and one wait, up front
                u8 = lq.dtype == torch.uint8
                if lq.dtype not in (torch.uint8, torch.float32) or lq.shape[-1 if u8 else 1] != 3:
                    raise ValueError(f'expected (N, 3, H, W) float32 or (N, H, W, 3) uint8 frames, got {lq.dtype} {tuple(lq.shape)}')
                H, W = self._frame_size(lq)
                mafd, scores = cut_scores(self._wait_sad(*self._sad_to_host(lq, None)), H * W)
                cuts = select_cuts(scores, n, self.cut_threshold, self.min_shot)
            else:
                cuts, mafd, scores = check_cuts(self.cuts, self.min_shot, n), None, None
            # every shot arrives as restore() of the shot alone would hand it in: the same launches on the same data
            bounds = [0] + cuts + [n]
            pieces = [p for a, b in zip(bounds, bounds[1:]) for p in lq[a:b].split(self.chunk)]
            outs = list(self._restore_shots(pieces, n, cuts))
            self.cut_mafd, self.cut_scores = mafd, scores
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
