"""Inverse telecine: which fields of a 2:3 pulldown stream belong together, and which frames repeat.

The device measures (ops.field_match: per frame the comb sums and block counts of two candidate weaves and three field differences,
exact integers); everything here is plain integer arithmetic on the rows of that table, on the host, the same for every batching:

    T6  m_i = p if S_p < S_c else c (ties: c);  combed_i = mic of the chosen candidate > mi (strict)
    T7  D_i = A_i + X, X = B_i for (m_(i-1), m_i) = (c, c), B_(i-1) for (p, p), C_i for (p, c), 0 for (c, p);  D_0 = +inf
    T8  cycles [5 g, 5 g + 5) anchored at frame 0: every cycle that lies wholly inside the stream drops its frame of least D, the
        first of equals; a trailing partial cycle drops nothing

A row is (S_c, S_p, mic_c, mic_p, A, B, C) (ops.FIELD_MATCH_COLUMNS); matches are 0 for c and 1 for p, as ops.field_weave takes them.
`PulldownDetector` is the streaming form: told about frames as they arrive, it releases a frame as soon as its fate no longer
depends on what follows.
"""
import math

CYCLE = 5
DEFAULT_MI = 80
S_C, S_P, MIC_C, MIC_P, A, B, C = range(7)


def _rows(table):
    rows = table.tolist() if hasattr(table, 'tolist') else [list(r) for r in table]
    for r in rows:
        if len(r) != 7:
            raise ValueError(f'a row of the table has the 7 columns of ops.FIELD_MATCH_COLUMNS, got {len(r)}')
    return [[int(v) for v in r] for r in rows]


def _check_mi(mi):
    if isinstance(mi, bool) or not isinstance(mi, int) or mi < 0:
        raise ValueError(f'mi is a count of samples, a non-negative integer, got {mi!r}')
    return mi


def _match(row, mi):
    m = 1 if row[S_P] < row[S_C] else 0
    return m, row[MIC_P if m else MIC_C] > mi


def _score(row, before, m, m_before):
    """T7 for a frame that has one before it."""
    if m_before == 0:
        x = row[B] if m == 0 else 0
    else:
        x = row[C] if m == 0 else before[B]
    return row[A] + x


def match_fields(table, mi=DEFAULT_MI):
    """T6: (matches, combed) - two lists as long as the table."""
    mi = _check_mi(mi)
    pairs = [_match(r, mi) for r in _rows(table)]
    return [m for m, _ in pairs], [c for _, c in pairs]


def duplicate_scores(table, matches):
    """T7: D, a list as long as the table; D[0] is math.inf."""
    rows = _rows(table)
    if len(matches) != len(rows):
        raise ValueError(f'{len(matches)} matches for {len(rows)} frames')
    return [math.inf if i == 0 else _score(rows[i], rows[i - 1], matches[i], matches[i - 1]) for i in range(len(rows))]


def select_drops(D, n):
    """T8: the frames dropped from a stream of n frames, in order - one per whole cycle."""
    if len(D) < n:
        raise ValueError(f'{len(D)} scores for {n} frames')
    drops = []
    for g in range(n // CYCLE):
        cyc = D[CYCLE * g:CYCLE * g + CYCLE]
        drops.append(CYCLE * g + cyc.index(min(cyc)))
    return drops


class PulldownDetector:
    """match_fields / duplicate_scores / select_drops for a stream of unknown length, fed in pieces of any size.

        det = PulldownDetector(mi=80, decimate=True)
        det.push(rows_of_the_new_frames)  -> [(index, match, combed, kept), ...] for the frames whose fate is final, in order
        det.finish()                      -> the rest: the frames of a trailing partial cycle, all kept

    A frame's match and combed flag are known when it arrives; whether it is kept, when its cycle of 5 is complete (at once with
    decimate=False).  For every piece pattern the released tuples are exactly what the batch functions decide on the whole table.
    State for a consumer: `arrived`, `released` (frames below it have been returned), `matches`, `combed` (flags), `scores` (D),
    `dropped` (indices) of every frame so far."""

    def __init__(self, mi=DEFAULT_MI, decimate=True):
        self.mi, self.decimate = _check_mi(mi), bool(decimate)
        self.matches, self.combed, self.scores, self.dropped = [], [], [], []
        self.released = 0
        self.finished = False
        self._before = None  # the row of the last frame

    @property
    def arrived(self):
        return len(self.matches)

    def _release(self, upto, drop=None):
        out = [(i, self.matches[i], self.combed[i], i != drop) for i in range(self.released, upto)]
        self.released = upto
        return out

    def push(self, rows):
        if self.finished:
            raise RuntimeError('PulldownDetector: push after finish')
        out = []
        for row in _rows(rows):
            m, combed = _match(row, self.mi)
            self.scores.append(math.inf if self._before is None else _score(row, self._before, m, self.matches[-1]))
            self.matches.append(m)
            self.combed.append(combed)
            self._before = row
            if not self.decimate:
                out += self._release(self.arrived)
            elif self.arrived % CYCLE == 0:
                cyc = self.scores[-CYCLE:]
                drop = self.arrived - CYCLE + cyc.index(min(cyc))
                self.dropped.append(drop)
                out += self._release(self.arrived, drop)
        return out

    def finish(self):
        """The stream has ended: the frames of the open cycle are kept."""
        self.finished = True
        return self._release(self.arrived)
