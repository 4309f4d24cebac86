"""Letterbox / pillarbox bars: the host side of DESIGN 4.22 (B2 - B6), integers and lists only - no torch, no NumPy, no float.

ops.bar_profile measures on the device (B1): per frame the row sums P and the column sums Q of the luma plane, one int64 table row
(P then Q).  Here: which rows and columns are dark (B2), every frame's box (B3), the video's box (B4), the rect that lies inside it on
the chroma steps with lengths the network takes (B5), and whether to believe it (B6).  ops.yuv_crop copies the rect (B7).  Boxes are
(top, bottom, left, right) - rows [top, bottom), columns [left, right) - or None for a blank frame; rects are (y0, x0, h, w).
No bit-compatibility with ffmpeg's cropdetect is claimed; `limit` = 24 is its default (limited-range black is 16).
"""

DEFAULT_LIMIT = 24    # B2: an 8-bit level; a row or column whose mean does not exceed it is dark
DEFAULT_MIN_BAR = 8   # B6: an axis that would lose fewer samples keeps its whole length
DEFAULT_PROBE = 48    # restore_y4m(crop='auto'): non-blank frames the rect is decided on


def _rows(table):
    """A table as a list of lists of ints: a tensor, an array (tolist) or nested sequences."""
    if hasattr(table, 'tolist'):
        table = table.tolist()
    return [list(row) for row in table]


def _level(limit):
    if isinstance(limit, bool) or not isinstance(limit, int) or not 0 <= limit <= 255:
        raise ValueError(f'limit is an 8-bit level, an integer in 0 ... 255, got {limit!r}')
    return limit


def _leading(values, bound):
    k = 0
    for v in values:
        if v > bound:
            break
        k += 1
    return k


def frame_boxes(table, H, W, depth=8, limit=DEFAULT_LIMIT):
    """B2, B3: the box of every frame of a table (n, H + W) of ops.bar_profile - (top, bottom, left, right), or None for a blank frame
    (every row dark, or every column).  depth: the samples' bit depth, 8 ... 16; the limit is shifted by depth - 8."""
    H, W, depth = int(H), int(W), int(depth)
    if H < 1 or W < 1 or not 8 <= depth <= 16:
        raise ValueError(f'a frame of {H} x {W} at {depth} bits')
    level = _level(limit) << (depth - 8)
    boxes = []
    for row in _rows(table):
        if len(row) != H + W:
            raise ValueError(f'a row of the table holds H + W = {H + W} sums, got {len(row)}')
        P, Q = row[:H], row[H:]
        t, l = _leading(P, level * W), _leading(Q, level * H)
        if t == H or l == W:
            boxes.append(None)
            continue
        b, r = _leading(reversed(P), level * W), _leading(reversed(Q), level * H)
        boxes.append((t, H - b, l, W - r))
    return boxes


def video_box(boxes):
    """B4: over the frames that have a box, the least top and left and the greatest bottom and right; None without one."""
    boxes = [b for b in boxes if b is not None]
    if not boxes:
        return None
    return min(b[0] for b in boxes), max(b[1] for b in boxes), min(b[2] for b in boxes), max(b[3] for b in boxes)


def _pair(v, what):
    try:
        a, b = (v, v) if isinstance(v, int) and not isinstance(v, bool) else v
    except (TypeError, ValueError):
        raise ValueError(f'{what} is an integer or (rows, columns), got {v!r}') from None
    for x in (a, b):
        if isinstance(x, bool) or not isinstance(x, int) or x < 1:
            raise ValueError(f'{what} is positive, got {v!r}')
    return a, b


def _axis(lo, hi, N, step, m, margin, min_bar):
    """B5 and the first rule of B6 along one axis: (offset, length)."""
    if lo > 0:
        lo += margin
    if hi < N:
        hi -= margin
    a, e = -(-lo // step) * step, hi // step * step
    len0 = e - a
    length = len0 // m * m  # (floor: a margin that eats the box leaves a negative length, which B6 does not believe)
    if N - length < min_bar:
        return 0, N
    return a + (len0 - length) // (2 * step) * step, length


def aligned_rect(box, H, W, step=1, multiple=1, margin=0, min_bar=DEFAULT_MIN_BAR):
    """B5, B6: the rect (y0, x0, h, w) inside `box` whose offsets are multiples of `step` and whose lengths are multiples of `multiple`
    (each an integer or (rows, columns); a multiple is a multiple of its step), centred in what the rounding leaves; margin: samples
    taken off every side of the box that has a bar.  An axis that would lose fewer than min_bar samples keeps its whole length.  None:
    no box, or a rect with an axis shorter than half the frame's - not believed."""
    if box is None:
        return None
    H, W = int(H), int(W)
    (sy, sx), (my, mx) = _pair(step, 'step'), _pair(multiple, 'multiple')
    if my % sy or mx % sx:
        raise ValueError(f'the multiple {(my, mx)} is no multiple of the step {(sy, sx)}')
    if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0 or isinstance(min_bar, bool) or not isinstance(min_bar, int) or min_bar < 0:
        raise ValueError(f'margin and min_bar are integers, at least 0: got {margin!r} and {min_bar!r}')
    t, b, l, r = box
    if not (0 <= t < b <= H and 0 <= l < r <= W):
        raise ValueError(f'the box {box} does not lie inside the {H} x {W} frame')
    y0, h = _axis(t, b, H, sy, my, margin, min_bar)
    x0, w = _axis(l, r, W, sx, mx, margin, min_bar)
    if 2 * h < H or 2 * w < W:
        return None
    return y0, x0, h, w


def check_rect(rect, H, W, step=1):
    """A rect (y0, x0, h, w) as four ints.  ValueError: not four integers, empty, outside the (H, W) frame, or an offset or length that
    is no multiple of `step` (an integer or (rows, columns))."""
    sy, sx = _pair(step, 'step')
    try:
        y0, x0, h, w = rect
    except (TypeError, ValueError):
        raise ValueError(f'rect is (y0, x0, h, w), got {rect!r}') from None
    for v in (y0, x0, h, w):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f'rect is four integers (y0, x0, h, w), got {rect!r}')
    if h < 1 or w < 1:
        raise ValueError(f'the rect {(y0, x0, h, w)} is empty')
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f'the rect {(y0, x0, h, w)} does not lie inside the {H} x {W} frame')
    if y0 % sy or h % sy or x0 % sx or w % sx:
        raise ValueError(f'the rect {(y0, x0, h, w)} is off the steps: rows in multiples of {sy}, columns of {sx}')
    return y0, x0, h, w


class BarDetector:
    """frame_boxes / video_box over a stream: push(table) takes the tables piece by piece, in frame order, and the state is exactly
    what the batch functions give on the concatenated table, whatever the pieces.  boxes: every frame's box so far (None: blank);
    blank: the indices of the blank frames; nonblank: how many frames have a box."""

    def __init__(self, H, W, depth=8, limit=DEFAULT_LIMIT):
        self.H, self.W, self.depth, self.limit = int(H), int(W), int(depth), _level(limit)
        frame_boxes([], self.H, self.W, self.depth, self.limit)  # argument errors now
        self.boxes = []

    def push(self, table):
        new = frame_boxes(table, self.H, self.W, self.depth, self.limit)
        self.boxes.extend(new)
        return new

    @property
    def frames(self):
        return len(self.boxes)

    @property
    def blank(self):
        return [i for i, b in enumerate(self.boxes) if b is None]

    @property
    def nonblank(self):
        return sum(b is not None for b in self.boxes)

    def box(self, frames=None):
        """B4 over the first `frames` frames (None: all so far)."""
        return video_box(self.boxes if frames is None else self.boxes[:frames])

    def rect(self, step=1, multiple=1, margin=0, min_bar=DEFAULT_MIN_BAR, frames=None):
        return aligned_rect(self.box(frames), self.H, self.W, step, multiple, margin, min_bar)

    def outside(self, rect, tolerance=2):
        """The frames whose own box reaches more than `tolerance` samples beyond `rect` on any side: picture the crop cuts off."""
        y0, x0, h, w = check_rect(rect, self.H, self.W)
        return [i for i, b in enumerate(self.boxes) if b is not None and
                (b[0] < y0 - tolerance or b[1] > y0 + h + tolerance or b[2] < x0 - tolerance or b[3] > x0 + w + tolerance)]


def crop_string(rect):
    """ffmpeg's crop order: 'W:H:X:Y'."""
    y0, x0, h, w = rect
    return f'{w}:{h}:{x0}:{y0}'


def parse_crop(text):
    """'W:H:X:Y' (ffmpeg's crop order) -> the rect (y0, x0, h, w).  ValueError for anything else."""
    parts = str(text).split(':')
    if len(parts) != 4 or not all(p.isascii() and p.isdigit() for p in parts):
        raise ValueError(f'a crop is W:H:X:Y, four non-negative integers, got {text!r}')
    w, h, x0, y0 = (int(p) for p in parts)
    return y0, x0, h, w
