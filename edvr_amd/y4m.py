"""YUV4MPEG2 ("Y4M") in, YUV4MPEG2 out: the container around ops.yuv420_to_rgb / VideoRestorer / ops.rgb_to_yuv420 (8-bit 4:2:0) and
ops.yuv_to_rgb / ops.rgb_to_yuv (4:2:0, 4:2:2 and 4:4:4 at 8 ... 16 bits), with no dependency.

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python scripts/restore_video.py - - --weights ... | ffmpeg -i - out.mp4

(ffmpeg's yuv4mpegpipe muxer writes anything but 8-bit 4:2:0 only with `-strict -1`.)

A Y4M stream is one text line `YUV4MPEG2 W<width> H<height> F<num>:<den> I<interlacing> A<num>:<den> C<chroma> X<comment>...`, then per
frame a line `FRAME[ parameters]` and the raw planes: for 8-bit 4:2:0 the H W luma bytes, then the (ceil(H / 2), ceil(W / 2)) Cb and Cr
planes - exactly the batch row ops.yuv420_to_rgb reads; for the other formats the chroma planes are full-size along an
axis that is not subsampled and a sample above 8 bits is a little-endian 16-bit word - the batch row ops.yuv_to_rgb reads.  Everything
here works on non-seekable streams (pipes), holds a bounded number of frames and uses no threads: pinned host buffers and non_blocking
copies keep the device busy while the host reads and writes.  Interlaced streams (It, Ib) are read on request and deinterlaced on the
device, at field rate, before the colour conversion: `deinterlaced` / `restore_y4m(deinterlace=...)` around ops.deinterlace.
The result can leave at a delivery size instead of s W x s H: `fit_size` / `restore_y4m(out_height=..., square_pixels=...)` around
ops.resample, on the float32 frames before the one quantisation.  Letterbox / pillarbox bars can be dropped before the
network pays for them: `cropped` / `BarProbe` / `restore_y4m(crop=...)` around ops.yuv_crop and ops.bar_profile, on the byte planes
between the deinterlace stage and the colour conversion.
"""
import math
from fractions import Fraction

import torch

from . import ops
from .bars import DEFAULT_LIMIT, DEFAULT_MIN_BAR, DEFAULT_PROBE, BarDetector, aligned_rect, check_rect
from .resample import KERNELS as RESAMPLE_KERNELS
from .telecine import DEFAULT_MI, PulldownDetector

MAGIC = b'YUV4MPEG2'
FRAME = b'FRAME\n'
CHROMA_420 = ('420jpeg', '420mpeg2', '420paldv', '420')
# the chroma siting (ops.YUV_SITINGS) the three 8-bit 4:2:0 tags stand for, as muxers pair them with chroma locations; no other tag says
SITING_OF_TAG = {'420jpeg': 'center', '420mpeg2': 'left', '420paldv': 'topleft'}
TAG_OF_SITING = {v: k for k, v in SITING_OF_TAG.items()}
# every format ops.yuv_to_rgb / ops.rgb_to_yuv convert, by its canonical name: '420', '420p9' ... '420p16', '422' ..., '444' ... '444p16'
ALL_FORMATS = tuple(base + (f'p{d}' if d > 8 else '') for base in ('420', '422', '444') for d in range(8, 17))


def default_matrix(H, W):
    """What players assume when a stream does not say: BT.709 for HD sizes (W >= 1280 or H > 576), BT.601 below."""
    return 'bt709' if W >= 1280 or H > 576 else 'bt601'


def _aspect_fraction(aspect):
    """The A tag 'num:den' as a Fraction; None and the unknown aspect 0:0 count as 1:1."""
    if aspect is None:
        return Fraction(1)
    num, sep, den = str(aspect).partition(':')
    if not (sep and num.isascii() and den.isascii() and num.isdigit() and den.isdigit()):
        raise ValueError(f'the aspect A{aspect} is not <num>:<den>')
    if int(num) == 0 or int(den) == 0:
        if int(num) == 0 and int(den) == 0:
            return Fraction(1)
        raise ValueError(f'the aspect A{aspect} has a zero on one side')
    return Fraction(int(num), int(den))


def _round_to_multiple(x, multiple):
    """The multiple of `multiple` nearest to the Fraction x, ties up, at least `multiple`."""
    return max(math.floor(x / multiple + Fraction(1, 2)), 1) * multiple


def fit_size(H, W, aspect, *, size=None, height=None, width=None, square=False, multiple=2):
    """The delivered size of an (H, W) frame with sample aspect `aspect` (the A tag: 'num:den' or None; None and 0:0 count as 1:1 and
    stay absent): (Ho, Wo, aspect_out), in integers and fractions only.  Exactly one selector: size=(Wo, Ho) - that size as
    stated; height=N - Ho = N and Wo = W N / H, times num / den when `square` (the samples become square: a 2880 x 1920 A32:27 frame at
    height 1080 is 1920 x 1080), rounded to the nearest multiple of `multiple` (ties up, at least `multiple`); width=N - the mirror.
    aspect_out is '1:1' when `square`; otherwise the input's aspect times (W Ho) / (H Wo), reduced, so that the display aspect survives
    the rounding (an unknown aspect - no tag, 0:0 - stays as it is).  ValueError: no or two selectors, non-positive
    numbers, an axis ratio outside [1/8, 8] (ops.resample's range), `square` with size= (the user states the size: no aspect arithmetic
    applies)."""
    given = [name for name, v in (('size', size), ('height', height), ('width', width)) if v is not None]
    if len(given) != 1:
        raise ValueError(f'exactly one of size=, height= and width= selects the delivered size, got {given or "none"}')
    H, W, multiple = int(H), int(W), int(multiple)
    if H < 1 or W < 1 or multiple < 1:
        raise ValueError(f'a frame and the multiple are positive, got {H} x {W} and multiple {multiple}')
    sar = _aspect_fraction(aspect)
    if size is not None:
        if square:
            raise ValueError('square applies to height= and width=: size= states both axes')
        try:
            Wo, Ho = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f'size is (Wo, Ho), got {size!r}') from None
    elif height is not None:
        Ho = int(height)
        if Ho < 1:
            raise ValueError(f'height must be positive, got {height}')
        Wo = _round_to_multiple(Fraction(W * Ho, H) * (sar if square else 1), multiple)
    else:
        Wo = int(width)
        if Wo < 1:
            raise ValueError(f'width must be positive, got {width}')
        Ho = _round_to_multiple(Fraction(H * Wo, W) / (sar if square else 1), multiple)
    if Ho < 1 or Wo < 1:
        raise ValueError(f'the delivered size must be positive, got {Wo} x {Ho}')
    for name, i, o in (('height', H, Ho), ('width', W, Wo)):
        if i > 8 * o or o > 8 * i:
            raise ValueError(f'the {name} ratio {i} / {o} is outside [1/8, 8]')
    if square:
        return Ho, Wo, '1:1'
    unknown = aspect is None or not any(int(v) for v in str(aspect).split(':'))
    if unknown or Fraction(W * Ho, H * Wo) == 1:
        return Ho, Wo, aspect  # as written; an unknown aspect (no tag, 0:0) stays unknown
    out = sar * Fraction(W * Ho, H * Wo)
    return Ho, Wo, f'{out.numerator}:{out.denominator}'


def _host_buffer(shape):
    """uint8 host memory, pinned where a device exists (non_blocking copies need it)."""
    return torch.empty(shape, dtype=torch.uint8, pin_memory=torch.cuda.is_available())


def _bytes_of(t):
    return memoryview(t.numpy()).cast('B')


class Y4MReader:
    """Reads progressive YUV4MPEG2 from a binary stream (a file, a pipe, sys.stdin.buffer, io.BytesIO): nothing seeks.

    formats: None - 8-bit 4:2:0 only, the format ops.yuv420_to_rgb reads - or a collection of format names (`ops.yuv_format`), such as
    ALL_FORMATS: 4:2:0, 4:2:2 and 4:4:4 at 8 ... 16 bits, which ops.yuv_to_rgb reads.

    Accepted: C420jpeg, C420mpeg2, C420paldv, C420 and no C tag - the same planes, whose tag names the chroma siting (`siting` below;
    the reader only reports it, `restore_y4m(siting_in='auto')` and the siting argument of the ops use it); with `formats`, also those of
    C422, C444 and C420p9 ... C444p16 that it names; Ip, I? and no I tag;
    XCOLORRANGE=FULL | LIMITED (no tag: limited).  ValueError: a bad magic, a missing or non-positive W / H, interlaced video (It, Ib,
    Im), a format that `formats` does not name (without it: C422, C444 and every high-bit-depth format), Cmono / C411 / C440 / C444alpha
    and depths outside 8 ... 16 always, a frame line that is not `FRAME`, and a truncated frame (the message names the frame index).

    width, height, fps ('30000:1001' as written, or None), aspect (likewise), range ('limited' | 'full'), chroma (the tag's value or
    None), format (the canonical name: '420', '422p10' ...), depth, subsampling ((sx, sy): log2 of the chroma decimation per axis),
    framesize (bytes, by the format); `frames_read` counts what read() returned so far.
    siting: what the tag says about where the chroma samples lie (ops.YUV_SITINGS) - 'center' for C420jpeg, 'left' for
    C420mpeg2, 'topleft' for C420paldv, None where the tag says nothing: C420, no tag, every C422 / C444 and every p9 ... p16 tag.
    (C420paldv is read as top-left co-sited chroma, which is how muxers use the tag for that chroma location; true PAL-DV siting, with Cb
    and Cr on alternate lines, is not implemented.)
    interlaced: True also accepts It and Ib - frames that weave two fields, for `deinterlaced` / restore_y4m(deinterlace=...) (DESIGN
    4.19); Im (mixed, flagged per frame) stays a ValueError.  interlace: the I tag's value - None, 'p', '?' and, with `interlaced`, 't' | 'b'."""

    def __init__(self, stream, formats=None, interlaced=False):
        self.stream = stream
        line = stream.readline(1024)
        if not line.startswith(MAGIC + b' ') or not line.endswith(b'\n'):
            raise ValueError(f'not a YUV4MPEG2 stream: the header starts with {line[:16]!r}')
        self.width = self.height = self.fps = self.aspect = self.chroma = None
        self.range, interlace = 'limited', None
        for tok in line[len(MAGIC):].decode('ascii', 'replace').split():
            tag, val = tok[0], tok[1:]
            if tag == 'W':
                self.width = self._positive(val, 'W')
            elif tag == 'H':
                self.height = self._positive(val, 'H')
            elif tag == 'F':
                self.fps = val
            elif tag == 'A':
                self.aspect = val
            elif tag == 'I':
                interlace = val
            elif tag == 'C':
                self.chroma = val
            elif tag == 'X' and val.upper().startswith('COLORRANGE='):
                rng = val[len('COLORRANGE='):].upper()
                if rng not in ('FULL', 'LIMITED'):
                    raise ValueError(f'XCOLORRANGE is FULL or LIMITED, got {rng!r}')
                self.range = rng.lower()
        if self.width is None or self.height is None:
            raise ValueError('the YUV4MPEG2 header gives no W / H')
        if interlace not in ((None, 'p', '?', 't', 'b') if interlaced else (None, 'p', '?')):
            if interlaced:
                raise ValueError(f'I{interlace} is not supported: progressive (Ip, I?), top-field-first (It) and bottom-field-first (Ib) video are')
            raise ValueError(f'interlaced video (I{interlace}) is not supported: deinterlace first')
        self.interlace = interlace
        if formats is None:
            if self.chroma is not None and self.chroma not in CHROMA_420:
                raise ValueError(f'C{self.chroma} is not supported: 8-bit 4:2:0 only ({", ".join("C" + c for c in CHROMA_420)})')
            sx, sy, self.depth, self.format = 1, 1, 8, '420'
        else:
            accepted = {ops.yuv_format(f)[3] for f in formats}
            try:
                sx, sy, self.depth, self.format = ops.yuv_format('420' if self.chroma is None else self.chroma)
            except ValueError:
                raise ValueError(f'C{self.chroma} is not supported: 4:2:0, 4:2:2 and 4:4:4 at 8 ... 16 bits are') from None
            if self.format not in accepted:
                raise ValueError(f'C{self.chroma} is not among the accepted formats ({", ".join(sorted(accepted))})')
        self.subsampling = (sx, sy)
        self.siting = SITING_OF_TAG.get(self.chroma)
        self.framesize = ops.yuv_frame_size(self.height, self.width, self.format)
        self.frames_read = 0

    @staticmethod
    def _positive(val, tag):
        if not val.isdigit() or int(val) < 1:
            raise ValueError(f'the YUV4MPEG2 header has {tag}{val}')
        return int(val)

    def _fill(self, view):
        """Reads until `view` is full or the stream ends (a pipe returns what it has); the number of bytes read."""
        got, readinto = 0, getattr(self.stream, 'readinto', None)
        while got < len(view):
            if readinto is not None:
                k = readinto(view[got:])
            else:
                piece = self.stream.read(len(view) - got)
                k = len(piece)
                view[got:got + k] = piece
            if not k:
                break
            got += k
        return got

    def read(self, k):
        """Up to k frames as ONE uint8 (j, 6 + framesize) host buffer (pinned where a device exists), j <= k, j = 0 at the end of the
        stream: each row is `FRAME\\n` and the frame's planes, so that `buf[:, 6:]` on the device is the batch ops.yuv420_to_rgb reads and
        the whole buffer is what a Y4MWriter of the same size writes.  Parameters after FRAME are read and dropped."""
        row = len(FRAME) + self.framesize
        buf = _host_buffer((max(int(k), 0), row))
        flat = _bytes_of(buf) if buf.numel() else None
        j = 0
        while j < buf.shape[0]:
            line = self.stream.readline(1024)
            if not line:
                break
            if not (line == FRAME or line.startswith(b'FRAME ')) or not line.endswith(b'\n'):
                raise ValueError(f'frame {self.frames_read + j}: expected a FRAME line, got {line[:16]!r}')
            flat[j * row:j * row + len(FRAME)] = FRAME
            got = self._fill(flat[j * row + len(FRAME):(j + 1) * row])
            if got != self.framesize:
                raise ValueError(f'frame {self.frames_read + j} is truncated: {got} of {self.framesize} bytes')
            j += 1
        self.frames_read += j
        return buf[:j]


class Y4MWriter:
    """Writes progressive YUV4MPEG2: the header on construction (`Ip`, `C420jpeg` for format '420' and `C<canonical name>` for any
    other of `ops.yuv_format`, F / A as given - strings such as '30000:1001', omitted when None - and XCOLORRANGE=FULL for range
    'full'), then `write(buf)` for every uint8 host buffer (k, 6 + framesize) whose rows already begin with `FRAME\\n` - the bytes go
    out as they are, in one write.  siting (ops.YUV_SITINGS): for 8-bit 4:2:0 the tag is `C420jpeg` ('center', the default),
    `C420mpeg2` ('left') or `C420paldv` ('topleft'); the tags of every other format cannot carry a siting - it is checked and otherwise
    ignored, and whoever encodes such a stream says it there (ffmpeg: `-chroma_sample_location left` / `topleft` on the output side)."""

    def __init__(self, stream, W, H, fps=None, aspect=None, range='limited', format='420', siting='center'):
        if range not in ops.YUV_RANGES:
            raise ValueError(f'range must be one of {sorted(ops.YUV_RANGES)}, got {range!r}')
        if siting not in TAG_OF_SITING:
            raise ValueError(f'siting must be one of {sorted(TAG_OF_SITING)}, got {siting!r}')
        if int(W) < 1 or int(H) < 1:
            raise ValueError(f'a frame has at least one row and column, got {H} x {W}')
        self.stream, self.width, self.height, self.range = stream, int(W), int(H), range
        self.format = ops.yuv_format(format)[3]
        self.siting = siting
        self.framesize = ops.yuv_frame_size(self.height, self.width, self.format)
        self.frames_written = 0
        head = [MAGIC.decode(), f'W{self.width}', f'H{self.height}'] + ([f'F{fps}'] if fps else []) + ['Ip'] + ([f'A{aspect}'] if aspect else [])
        head += ['C' + TAG_OF_SITING[siting] if self.format == '420' else 'C' + self.format] + (['XCOLORRANGE=FULL'] if range == 'full' else [])
        stream.write((' '.join(head) + '\n').encode('ascii'))

    def write(self, buf):
        if buf.is_cuda or buf.dtype != torch.uint8 or buf.dim() != 2 or buf.shape[1] != len(FRAME) + self.framesize or not buf.is_contiguous():
            raise ValueError(f'frames are written from a contiguous uint8 host buffer (k, {len(FRAME) + self.framesize}), got '
                             f'{buf.dtype} {tuple(buf.shape)}')
        if buf.shape[0] == 0:
            return
        marks = torch.tensor(list(FRAME), dtype=torch.uint8)
        if not torch.equal(buf[:, :len(FRAME)], marks.expand(buf.shape[0], -1)):
            raise ValueError('every row of the buffer begins with the FRAME line')
        self.stream.write(_bytes_of(buf))
        self.frames_written += buf.shape[0]


def resolve_siting(siting, reader):
    """A siting argument -> a name of ops.YUV_SITINGS: 'auto' is what the reader's tag says (`Y4MReader.siting`) or, where the tag is
    silent, 'left' - the default chroma location of H.264, HEVC and AV1 4:2:0 and the siting of every 4:2:2."""
    if siting == 'auto':
        return reader.siting or 'left'
    if siting not in ops.YUV_SITINGS:
        raise ValueError(f"siting must be 'auto' or one of {sorted(ops.YUV_SITINGS)}, got {siting!r}")
    return siting


FIELD_ORDERS = {'tff': 'top', 'bff': 'bottom'}  # restore_y4m's field_order -> ops.deinterlace's `first`


def deinterlaced(pieces, H, W, format='420', first='top', mode='field'):
    """A generator over deinterlaced device byte batches: `pieces` is an iterable of uint8 (k, >= framesize) batches of consecutive
    interlaced frames, k >= 1 and any mix of sizes (`buf[:, 6:]` of the reader's buffers); every piece goes through ops.deinterlace
    (first, mode: as there) with the last frame of the piece before as `prev` and the first frame of the piece after as `next`, so the
    concatenated result is what ONE call on the whole clip gives, whatever the pieces.  A piece is held until the next one has
    arrived: a delay of one piece and that much memory; the last piece goes out with next=None."""
    held = before = None
    for piece in pieces:
        if held is not None:
            yield ops.deinterlace(held, H, W, format, first=first, mode=mode, prev=before, next=piece[0])
            before = held[-1]
        held = piece
    if held is not None:
        yield ops.deinterlace(held, H, W, format, first=first, mode=mode, prev=before, next=None)


def double_rate(fps):
    """The F tag of a field-rate stream: '30000:1001' -> '60000:1001'; None (no tag) stays None."""
    if fps is None:
        return None
    num, sep, den = fps.partition(':')
    if not (sep and num.isdigit() and den.isdigit()):
        raise ValueError(f'the frame rate F{fps} is not <num>:<den>: it cannot be doubled')
    return f'{2 * int(num)}:{den}'


def film_rate(fps):
    """The F tag of a decimated film-rate stream: 4 / 5 of the rate, reduced - '30000:1001' -> '24000:1001'; None (no tag) stays None."""
    if fps is None:
        return None
    num, sep, den = fps.partition(':')
    if not (sep and num.isascii() and den.isascii() and num.isdigit() and den.isdigit()) or int(den) == 0:
        raise ValueError(f'the frame rate F{fps} is not <num>:<den>: its film rate cannot be formed')
    num, den = 4 * int(num), 5 * int(den)
    g = math.gcd(num, den)
    return f'{num // g}:{den // g}'


def inverse_telecined(pieces, H, W, format='420', first='top', decimate=True, nt=2, ct=9, mi=DEFAULT_MI, stats=None):
    """A generator over device byte batches of FILM frames: `pieces` is an iterable of uint8 (k, >= framesize) batches of
    consecutive frames of a telecined stream, k >= 1 and any mix of sizes (`buf[:, 6:]` of the reader's buffers).  Every frame is
    measured (ops.field_match, with the two frames before it as context), matched to the field that completes its first field and
    scored as a repeat (telecine.PulldownDetector); of every cycle of 5 the most repeated frame is dropped (decimate) and every kept
    frame is woven from its matching fields (ops.field_weave) - or, where even the better weave is combed, deinterlaced from its first
    field (ops.deinterlace(mode='frame') with the frames around it as prev / next).  The concatenated result is the definition applied
    to the whole clip, whatever the pieces.  Batches that turn out empty are not yielded.
    Held: the pieces that reach back to the frame before the oldest frame not yet written - a frame waits for the end of its cycle
    of 5 and, combed, for the frame after it - and the last two frames for the next piece's measurement.  One host wait per piece, on
    an event recorded right after that piece's field_match launch and the copy of its table to pinned memory; the NEXT piece is
    fetched (its copy to the device issued by whoever makes the pieces) and measured before that wait, so the device has work while
    the host decides.  stats: a dict that receives 'film_matches' (0 = c, 1 = p per input frame), 'film_combed' and 'film_dropped'
    (input frame indices) and 'film_dropped_scores' (D of the dropped frames) when the stream has ended."""
    fs = ops.yuv_frame_size(H, W, format)
    det = PulldownDetector(mi=mi, decimate=decimate)
    held = []        # (index of the piece's first frame, piece), oldest first
    last2 = []       # the last two frames that arrived
    ready = []       # (index, match, combed) of the kept frames whose fate is final, not yet written
    waiting = None   # (pinned table, event) of the piece measured last
    arrived = 0

    def frame(i):
        for start, piece in held:
            if start <= i < start + piece.shape[0]:
                return piece[i - start]
        raise AssertionError(f'frame {i} is no longer held')

    def decide(final):
        nonlocal waiting
        if waiting is not None:
            table, event = waiting
            if event is not None:
                event.synchronize()
            ready.extend((i, m, c) for i, m, c, kept in det.push(table) if kept)
            waiting = None
        if final:
            ready.extend((i, m, c) for i, m, c, kept in det.finish() if kept)

    def written(final):
        """The frames of `ready` that can be written now, as one batch (None: none) - a combed one needs the frame after it."""
        take = 0
        while take < len(ready) and (not ready[take][2] or ready[take][0] + 1 < arrived or final):
            take += 1
        if not take:
            return None
        now = ready[:take]
        del ready[:take]
        out = torch.empty((take, fs), dtype=torch.uint8, device=held[0][1].device)
        at = 0
        for start, piece in held:  # one weave per piece that holds some of the frames
            mine = [(i, m) for i, m, _ in now if start <= i < start + piece.shape[0]]
            if mine:
                ops.field_weave(piece, H, W, format, first=first, frames=[i - start for i, _ in mine], matches=[m for _, m in mine],
                                prev=frame(start - 1) if mine[0] == (start, 1) else None, out=out[at:at + len(mine)])
                at += len(mine)
        for j, (i, _, combed) in enumerate(now):
            if combed:  # T9's fallback, over what the weave put there
                ops.deinterlace(frame(i)[None], H, W, format, first=first, mode='frame', prev=frame(i - 1) if i else None,
                                next=frame(i + 1) if i + 1 < arrived else None, out=out[j:j + 1])
        oldest = (ready[0][0] if ready else det.released) - 1  # a p weave and the fallback read the frame before
        while held and held[0][0] + held[0][1].shape[0] <= min(oldest, arrived - 1):
            held.pop(0)
        return out

    for piece in pieces:
        k = piece.shape[0]
        table = ops.field_match(piece, H, W, format, first=first, prev=last2[-1] if last2 else None, prev2=last2[-2] if len(last2) > 1 else None,
                                nt=nt, ct=ct)
        host = _host_buffer((k, 7 * 8)).view(torch.int64)
        host.copy_(table, non_blocking=True)
        event = None
        if piece.is_cuda:
            event = torch.cuda.Event()
            event.record()
        decide(False)  # the piece before this one: its table has been on its way since before this piece was fetched
        waiting = (host, event)
        held.append((arrived, piece))
        arrived += k
        last2 = (last2 + [piece[j] for j in range(max(k - 2, 0), k)])[-2:]
        out = written(False)
        if out is not None:
            yield out
    decide(True)
    if held:
        out = written(True)
        if out is not None:
            yield out
    if stats is not None:
        stats.update(film_matches=list(det.matches), film_combed=[i for i, c in enumerate(det.combed) if c], film_dropped=list(det.dropped),
                     film_dropped_scores=[det.scores[i] for i in det.dropped])


def cropped(pieces, H, W, format, rect):
    """A generator over cropped device byte batches: every uint8 (k, >= framesize) batch of `pieces` goes through
    ops.yuv_crop with rect = (y0, x0, h, w) and leaves as (k, yuv_frame_size(h, w, format)).  The rect is checked before the first
    piece is fetched (ValueError: outside the frame, off the chroma steps, empty)."""
    sx, sy = ops.yuv_format(format)[:2]
    rect = check_rect(rect, int(H), int(W), (1 << sy, 1 << sx))
    for piece in pieces:
        yield ops.yuv_crop(piece, H, W, format, rect=rect)


class BarProbe:
    """restore_y4m(crop='auto') in front of the crop: profiles the byte batches of `pieces` as they arrive
    (ops.bar_profile; the table copied to pinned memory behind the launch) and holds them; decide() returns the rect of B4 - B6 -
    or None: nothing to believe - once `probe` non-blank frames have been seen, 4 probe frames are held or the stream has ended,
    after ONE host wait where no held frame is blank: on the event behind the last table's copy.  replay() then yields the held
    pieces and every later one as they are; the later ones are profiled too, without a wait, and finish() reads their tables:
    `blank` (frame indices), `outside` (frames whose own box reaches beyond the rect: the picture grew after the probe) and `box`
    (the probe's video box).  step, multiple: B5's, (rows, columns)."""

    def __init__(self, pieces, H, W, format='420', *, probe=DEFAULT_PROBE, limit=DEFAULT_LIMIT, margin=0, min_bar=DEFAULT_MIN_BAR, step=1, multiple=1):
        self.source, self.H, self.W, self.format = iter(pieces), int(H), int(W), format
        self.probe, self.margin, self.min_bar, self.step, self.multiple = int(probe), margin, min_bar, step, multiple
        self.detector = BarDetector(self.H, self.W, ops.yuv_format(format)[2], limit)
        self.held, self.unread = [], []  # pieces not yet replayed; (pinned table, event) not yet read
        self.rect = self.box = None
        self.blank, self.outside = [], []

    def _measure(self, piece):
        table = ops.bar_profile(piece, self.H, self.W, self.format)
        host = _host_buffer((piece.shape[0], 8 * (self.H + self.W))).view(torch.int64)
        host.copy_(table, non_blocking=True)
        event = None
        if piece.is_cuda:
            event = torch.cuda.Event()
            event.record()
        self.unread.append((host, event))

    def _read(self):
        for host, event in self.unread:
            if event is not None:
                event.synchronize()
            self.detector.push(host)
        self.unread = []

    def decide(self):
        held, look_at = 0, self.probe
        for piece in self.source:
            self._measure(piece)
            self.held.append(piece)
            held += piece.shape[0]
            if held >= min(look_at, 4 * self.probe):
                self._read()
                if self.detector.nonblank >= self.probe or held >= 4 * self.probe:
                    break
                look_at = held + self.probe - self.detector.nonblank  # blank frames in front: at least that many more
        self._read()
        self.box = self.detector.box()
        self.rect = aligned_rect(self.box, self.H, self.W, self.step, self.multiple, self.margin, self.min_bar)
        return self.rect

    def replay(self):
        while self.held:
            yield self.held.pop(0)
        for piece in self.source:
            self._measure(piece)
            yield piece

    def finish(self):
        self._read()
        self.blank = self.detector.blank
        self.outside = self.detector.outside(self.rect) if self.rect is not None else []


def resolve_field_order(deinterlace, field_order, reader):
    """restore_y4m's (deinterlace, field_order) -> (`first` of ops.deinterlace or None: nothing to do, mode).  'auto' follows the
    reader's I tag - It: 'top', Ib: 'bottom', anything else: progressive, passed through; 'tff' / 'bff' deinterlace whatever the tag says.
    mode is `deinterlace` itself: 'field' | 'frame' for ops.deinterlace, 'film' for `inverse_telecined`."""
    if deinterlace not in (None, 'field', 'frame', 'film'):
        raise ValueError(f"deinterlace must be None, 'field', 'frame' or 'film', got {deinterlace!r}")
    if field_order != 'auto' and field_order not in FIELD_ORDERS:
        raise ValueError(f"field_order must be 'auto' or one of {sorted(FIELD_ORDERS)}, got {field_order!r}")
    if deinterlace is None:
        return None, None
    if field_order == 'auto':
        return {'t': 'top', 'b': 'bottom'}.get(getattr(reader, 'interlace', None)), deinterlace
    return FIELD_ORDERS[field_order], deinterlace


def restore_y4m(net, src, dst, *, matrix_in=None, matrix_out=None, chroma='bilinear', read_frames=8, on_chunk=None, stats=None, out_format=None,
                siting_in='center', siting_out=None, deinterlace=None, field_order='auto', film_decimate=True, film_params=None,
                out_size=None, out_height=None, out_width=None, square_pixels=False, resample='lanczos3', crop=None, crop_probe=DEFAULT_PROBE,
                crop_limit=DEFAULT_LIMIT, crop_margin=0, crop_min_bar=DEFAULT_MIN_BAR, **restorer_kwargs):
    """Restore a Y4M stream with `net` (an EDVR in eval mode, on the GPU) into a Y4M stream; returns the number of frames.  Call it under
    torch.no_grad().

        src (a binary stream or a Y4MReader) -> read_frames frames per read into pinned memory -> one copy to the device
            -> ops.yuv420_to_rgb(buf[:, 6:], float32) -> VideoRestorer(net, out_dtype=torch.float32, **restorer_kwargs).restore_chunks
            -> ops.rgb_to_yuv420(chunk, out=buf[:, 6:]) -> one copy into pinned memory -> dst (a binary stream)

    The frames never exist as RGB bytes and the network's float32 result is quantised once, to YUV bytes.  matrix_in / matrix_out:
    a name of ops.YUV_MATRICES ('bt601' | 'bt709' | 'bt2020nc'); None follows `default_matrix` for that side's OWN frame size - a 180 x 320 input is read as BT.601 and its 720 x 1280
    result written as BT.709, because that is how it will be played.  The range (XCOLORRANGE) is copied from the input, F and A likewise;
    the output is s W x s H, s = 4 (1 for an hr_in network).  chroma: the upsampling filter of the decode.  restorer_kwargs: chunk,
    pad_mode, tile, tile_overlap, tile_blend, self_ensemble, time_reverse, ... as VideoRestorer takes them - sizes that are no multiple
    of 4 (16 with hr_in) need pad_mode.  Memory: read_frames input frames per buffer, the restorer's bank and pieces, two chunks of output.
    The host writes chunk i while the device works on chunk i + 1; nothing else waits.  on_chunk: called as on_chunk(chunk) with every
    restored float32 RGB chunk (k, 3, s H, s W) on the device, in order, before it is converted back - for scoring the output
    (metrics.calculate_niqe) or a preview; it must not modify the chunk.  Without it the launches are unchanged.
    cuts (a restorer_kwarg, with cut_threshold / min_shot): None | 'auto' | frame indices - windows stay inside a shot (VideoRestorer);
    'auto' scores the decoded float32 RGB, piece by piece as it is read.  The chunks that leave are then short at the end of every shot;
    nothing here depends on their size.  stats: a dict that receives 'frames' and, with cuts, 'cuts', 'cut_scores' and 'cut_mafd' (the
    restorer's cuts_found / cut_scores / cut_mafd) when the stream has ended.
    Formats: a raw stream is opened with ALL_FORMATS - 4:2:0, 4:2:2 and 4:4:4 at 8 ... 16 bits.  out_format: None writes the
    input's format, a name of `ops.yuv_format` that one: `out_format='420p10'` (or '444p10') on 8-bit input quantises the network's
    float32 result once, to 10 bits, instead of banding it at 8.  8-bit 4:2:0 in and out goes through ops.yuv420_to_rgb / rgb_to_yuv420
    as above, everything else through ops.yuv_to_rgb(buf[:, 6:], H, W, format, ...) / ops.rgb_to_yuv(chunk, format, ..., out=buf[:, 6:]).
    Chroma siting: siting_in - 'center' (the default: what this function always did), 'left', 'topleft', or 'auto': the
    reader's tag (`Y4MReader.siting`) and 'left' where the tag is silent, which is right for nearly all H.264 / HEVC / AV1 footage -
    decoding left-sited chroma as centred shifts the colour by half an input pixel, two output pixels.  siting_out: the siting the output
    is encoded for and, for 8-bit 4:2:0, tagged with (Y4MWriter); None - the resolved input siting.  The transfer function is never
    touched.  With both sitings 'center' the calls are the ones made before the argument existed.
    Interlaced video: deinterlace - None (an interlaced stream raises, as it always did), 'field' (every field becomes a
    frame: 2 n frames out, F doubled - a 25i tape is restored as the 50 pictures per second it holds) or 'frame' (the first field of
    every frame); a raw stream is then opened with interlaced=True.  field_order: 'auto' - the stream's tag (It / Ib); an Ip or
    untagged stream passes through untouched, no launch - or 'tff' / 'bff', which deinterlace whatever the tag says (mis-tagged
    captures).  The stage (`deinterlaced`: ops.deinterlace piece by piece with its neighbours' frames as context) sits between the copy
    to the device and the colour conversion; everything after it sees a progressive video of its output frames - `cuts` indices count
    those - and the output is written Ip.
    Film: deinterlace='film' undoes 2:3 pulldown instead - `inverse_telecined` in the same place: fields that belong to one
    film frame are woven back together, bit for bit, and (film_decimate, the default) the most repeated frame of every 5 is dropped; F
    is then written as `film_rate` of the input's, 4 / 5 of it ('30000:1001' -> '24000:1001'), and unchanged with film_decimate=False.
    film_params: a dict with any of nt, ct, mi, the thresholds of the definition.  stats also receives 'film_matches', 'film_combed',
    'film_dropped' and 'film_dropped_scores'; frames listed in 'film_combed' had no clean match and were deinterlaced from one field -
    many of them mean the passage is video, not film: use 'field'.
    Delivery size: out_size=(Wo, Ho), out_height=N or out_width=N (one of them; square_pixels with the last two) write
    the result at `fit_size(s H, s W, A, ...)` instead of s W x s H, with that call's A tag: every restored float32 chunk goes through
    ops.resample (resample: 'lanczos3' | 'bicubic' | 'bilinear') on the device before the one quantisation - a 720 x 480 A32:27 disc
    with out_height=1080, square_pixels=True leaves as 1920 x 1080 A1:1, not as 2880 x 1920 for a second scaler to quantise again.
    matrix_out then defaults by the delivered size and on_chunk receives the delivered chunk - what is written.  A delivered size
    equal to s W x s H makes no launch; without a selector no call differs from those made before the arguments existed.
    Bars: crop - None, a rect (y0, x0, h, w) of the progressive frames the deinterlace / film stage emits, or 'auto' - drops
    letterbox / pillarbox bars on the byte planes, between that stage and the decode (`cropped`: ops.yuv_crop): everything after sees
    an h x w video - the decode, the restorer with all its arguments (`cuts` indices are unchanged), fit_size(s h, s w, A, ...), the
    matrix defaults, the header.  A is copied: the samples keep their shape.  A rect is on the format's chroma steps and, unless
    pad_mode is given, h and w are multiples of the restorer's size multiple: ValueError before anything is launched or written.
    'auto' (`BarProbe`): the pieces are profiled as they arrive (ops.bar_profile) and held until crop_probe frames that are not blank
    have been seen (or 4 crop_probe frames are held, or the stream ends); the rect is then decided from their common box (bars.py:
    crop_limit - the 8-bit level up to which a row or column's mean counts as dark; crop_margin - samples taken off each side that has
    a bar; crop_min_bar - an axis that would lose fewer samples is left alone), aligned inward to the chroma steps and the size multiple
    (the chroma steps alone with pad_mode), and the held pieces are replayed - the one host wait.  A rect with an axis under half the
    frame's is not believed: nothing is cropped.  Later pieces are profiled without a wait; stats receives 'crop' (the rect or None),
    'crop_box' (the probe's box), 'bars_blank' and 'bars_outside' - frames whose own picture reaches beyond the rect: the picture
    grew after the probe, use scripts/detect_bars.py and give the rect.  A rect equal to the whole frame makes no launch; with
    crop=None no call differs from those made before the argument existed."""
    from .video import VideoRestorer
    if resample not in RESAMPLE_KERNELS:
        raise ValueError(f'resample must be one of {sorted(RESAMPLE_KERNELS)}, got {resample!r}')
    fit = {k: v for k, v in (('size', out_size), ('height', out_height), ('width', out_width)) if v is not None}
    if not fit and square_pixels:
        raise ValueError('square_pixels needs out_height or out_width')
    if deinterlace is None:
        reader = src if isinstance(src, Y4MReader) else Y4MReader(src, formats=ALL_FORMATS)
    else:
        reader = src if isinstance(src, Y4MReader) else Y4MReader(src, formats=ALL_FORMATS, interlaced=True)
    first, mode = resolve_field_order(deinterlace, field_order, reader)
    fmt_in = reader.format
    fmt_out = fmt_in if out_format is None else ops.yuv_format(out_format)[3]
    plain420 = fmt_in == '420' and fmt_out == '420'  # the 8-bit 4:2:0 operators (uint8 samples, 4:2:0 instances of csrc/yuv.hip) on both sides
    if int(read_frames) < 1:
        raise ValueError(f'read_frames must be at least 1, got {read_frames}')
    for name in (matrix_in, matrix_out):
        if name is not None and name not in ops.YUV_MATRICES:
            raise ValueError(f'matrix must be one of {sorted(ops.YUV_MATRICES)}, got {name!r}')
    if chroma not in ('bilinear', 'nearest'):
        raise ValueError(f"chroma must be 'bilinear' or 'nearest', got {chroma!r}")
    siting_in = resolve_siting(siting_in, reader)
    siting_out = siting_in if siting_out is None else resolve_siting(siting_out, reader)
    # (no keyword at 'center': the calls of every caller and stand-in that predates the argument)
    kw_in = {} if siting_in == 'center' else {'siting': siting_in}
    kw_out = {} if siting_out == 'center' else {'siting': siting_out}
    if crop is not None:
        if crop != 'auto':
            crop = check_rect(crop, reader.height, reader.width, tuple(1 << s for s in reversed(reader.subsampling)))
        if isinstance(crop_probe, bool) or not isinstance(crop_probe, int) or crop_probe < 1:
            raise ValueError(f'crop_probe is a number of frames, at least 1, got {crop_probe!r}')
        aligned_rect((0, 1, 0, 1), 1, 1, margin=crop_margin, min_bar=crop_min_bar)  # their argument errors now
        BarDetector(reader.height, reader.width, ops.yuv_format(fmt_in)[2], crop_limit)  # ... and the limit's
    vr = VideoRestorer(net, out_dtype=torch.float32, **restorer_kwargs)
    device = next(net.parameters()).device
    H, W = reader.height, reader.width
    fps = double_rate(reader.fps) if first is not None and mode == 'field' else reader.fps
    film = {}
    if first is not None and mode == 'film':
        unknown = set(film_params or {}) - {'nt', 'ct', 'mi'}
        if unknown:
            raise ValueError(f'film_params holds nt, ct and mi, got {sorted(unknown)}')
        if film_decimate:
            fps = film_rate(reader.fps)

    def batches():
        while True:
            host = reader.read(read_frames)
            if host.shape[0] == 0:
                return
            yield host.to(device, non_blocking=True)[:, len(FRAME):]

    def progressive():
        if first is None:
            return batches()
        if mode == 'film':
            return inverse_telecined(batches(), reader.height, reader.width, fmt_in, first, bool(film_decimate), stats=film, **(film_params or {}))
        return deinterlaced(batches(), reader.height, reader.width, fmt_in, first, mode)

    bars, stage = None, None  # the BarProbe of crop='auto'; the byte batches behind the crop (None: `progressive()`, as before the argument)
    if crop is not None:
        steps = tuple(1 << s for s in reversed(reader.subsampling))  # (rows, columns)
        m = 1 if restorer_kwargs.get('pad_mode') is not None else vr.multiple
        multiple = tuple(s * m // math.gcd(s, m) for s in steps)
        if crop == 'auto':
            # the header states the size: the rect is decided on the first frames, before anything is written
            bars = BarProbe(progressive(), H, W, fmt_in, probe=crop_probe, limit=crop_limit, margin=crop_margin, min_bar=crop_min_bar,
                            step=steps, multiple=multiple)
            rect, stage = bars.decide(), bars.replay()
        else:
            rect, stage = crop, progressive()
            if rect[2] % multiple[0] or rect[3] % multiple[1]:
                raise ValueError(f'the crop {rect[2]} x {rect[3]} (rows x columns) is no multiple of {m}, the size the network takes: '
                                 f'give pad_mode, or a rect that is')
        if rect is not None and rect != (0, 0, H, W):
            stage = cropped(stage, H, W, fmt_in, rect)
            H, W = rect[2], rect[3]
    Ho, Wo, aspect = vr.scale * H, vr.scale * W, reader.aspect
    delivered = None  # (Ho, Wo) where the restored chunks are resampled
    if fit:
        Hd, Wd, aspect = fit_size(Ho, Wo, reader.aspect, square=bool(square_pixels), **fit)
        if (Hd, Wd) != (Ho, Wo):
            delivered = Ho, Wo = Hd, Wd
    matrix_in = matrix_in or default_matrix(H, W)
    matrix_out = matrix_out or default_matrix(Ho, Wo)
    writer = Y4MWriter(dst, Wo, Ho, fps, aspect, reader.range, fmt_out, siting_out)
    row = len(FRAME) + writer.framesize
    marks = torch.tensor(list(FRAME), dtype=torch.uint8).to(device)

    def decoded():
        for yuv in (progressive() if stage is None else stage):
            if plain420:
                yield ops.yuv420_to_rgb(yuv, H, W, matrix_in, reader.range, chroma, **kw_in)
            else:
                yield ops.yuv_to_rgb(yuv, H, W, fmt_in, matrix_in, reader.range, chroma, **kw_in)

    pending = None  # (pinned buffer, event after its copy) of the chunk before this one

    def flush():
        if pending is not None:
            if pending[1] is not None:
                pending[1].synchronize()
            writer.write(pending[0])

    for out in vr.restore_chunks(decoded()):
        if delivered is not None:
            out = ops.resample(out, delivered, resample)
        buf = torch.empty((out.shape[0], row), dtype=torch.uint8, device=device)
        buf[:, :len(FRAME)] = marks
        if on_chunk is not None:
            on_chunk(out)
        if plain420:
            ops.rgb_to_yuv420(out, matrix_out, reader.range, out=buf[:, len(FRAME):], **kw_out)
        else:
            ops.rgb_to_yuv(out, fmt_out, matrix_out, reader.range, out=buf[:, len(FRAME):], **kw_out)
        host = _host_buffer(tuple(buf.shape))
        host.copy_(buf, non_blocking=True)
        done = None
        if device.type == 'cuda':
            done = torch.cuda.Event()
            done.record()
        flush()
        pending = (host, done)
    flush()
    if hasattr(dst, 'flush'):
        dst.flush()
    if stats is not None:
        stats['frames'] = writer.frames_written
        stats.update(film)
        if bars is not None:
            bars.finish()
            stats.update(crop=bars.rect, crop_box=bars.box, bars_blank=bars.blank, bars_outside=bars.outside)
        elif crop is not None:
            stats.update(crop=crop)
        if getattr(vr, 'cuts', None) is not None:
            stats.update(cuts=vr.cuts_found, cut_scores=vr.cut_scores, cut_mafd=vr.cut_mafd)
    return writer.frames_written
