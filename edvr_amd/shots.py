"""Scene cuts: which frames of a video belong together.

The device measures (ops.frame_sad: the sum of absolute 8-bit luma differences of consecutive frames, an exact integer); everything
here is plain float64 and integer arithmetic on the host, the same for every batching of the frames:

    mafd_i  = SAD_i / (H W)                                 mean absolute frame difference on the 0 ... 255 scale; mafd_0 := 0
    score_i = min(mafd_i, |mafd_i - mafd_(i-1)|)            the rule of ffmpeg's scene-change filters; mafd runs on across cuts
    cuts    = select_cuts(scores, n, threshold, min_shot)   a cut at i: frame i begins a new shot

`ShotDetector` is the streaming form: told about frames as they arrive, it confirms or declines a candidate as soon as the answer no
longer depends on how long the video is.
"""

DEFAULT_THRESHOLD = 10.0


def cut_scores(sad, pixels, prev_mafd=0.0):
    """(mafd, scores): two float64 lists as long as `sad`.  sad: the integers ops.frame_sad returned (a list, or a CPU tensor) for
    consecutive frames; pixels = H W; prev_mafd: the mafd of the frame before sad[0] (0.0 at the start of a video, whose first frame
    has sad 0 and scores 0)."""
    pixels = int(pixels)
    if pixels < 1:
        raise ValueError(f'pixels must be at least 1, got {pixels}')
    mafd, scores, before = [], [], float(prev_mafd)
    for s in (sad.tolist() if hasattr(sad, 'tolist') else sad):
        m = int(s) / pixels
        mafd.append(m)
        scores.append(min(m, abs(m - before)))
        before = m
    return mafd, scores


def _check_rule(threshold, min_shot):
    if isinstance(min_shot, bool) or not isinstance(min_shot, int) or min_shot < 1:
        raise ValueError(f'min_shot must be a positive integer, got {min_shot!r}')
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError('threshold is NaN')
    return threshold, min_shot


def select_cuts(scores, n, threshold=DEFAULT_THRESHOLD, min_shot=2):
    """The cuts of a video of n frames, in order: start = 0; for i = 1 ... n - 1, i is a cut iff scores[i] >= threshold,
    i - start >= min_shot and n - i >= min_shot, and then start = i.  Every shot therefore has at least min_shot frames; a candidate
    too close to the previous cut or to the end is dropped and its frames stay in the running shot.  scores[0] is not looked at."""
    threshold, min_shot = _check_rule(threshold, min_shot)
    if len(scores) < n:
        raise ValueError(f'{len(scores)} scores for {n} frames')
    cuts, start = [], 0
    for i in range(1, n):
        if scores[i] >= threshold and i - start >= min_shot and n - i >= min_shot:
            cuts.append(i)
            start = i
    return cuts


def check_cuts(cuts, min_shot, n=None):
    """Explicit cuts as a list: strictly increasing integers >= 1 that leave no shot shorter than min_shot (the last one is checked
    where the length n is known).  ValueError otherwise."""
    try:
        cuts = list(cuts)
    except TypeError:
        raise ValueError(f"cuts must be None, 'auto' or a sequence of frame indices, got {cuts!r}") from None
    if any(isinstance(c, bool) or not isinstance(c, int) for c in cuts):
        raise ValueError(f'cuts are integer frame indices, got {cuts}')
    if any(c < 1 for c in cuts):
        raise ValueError(f'a cut is the index of the first frame of a new shot, at least 1: got {cuts}')
    if any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f'cuts must be strictly increasing, got {cuts}')
    bounds = [0] + cuts + ([n] if n is not None else [])
    for a, b in zip(bounds, bounds[1:]):
        if b - a < min_shot:
            raise ValueError(f'cuts {cuts}' + (f' of a video of {n} frames' if n is not None else '') +
                             f' leave a shot of {b - a} frame(s), frames [{a}, {b}): every shot needs at least min_shot = {min_shot}')
    return cuts


class ShotDetector:
    """select_cuts for a video of unknown length, fed in pieces of any size.

        det = ShotDetector(threshold=10.0, min_shot=5)
        det.push(scores_of_the_new_frames)  -> the cuts confirmed by this piece     (or push_sad(sads, H * W))
        det.finish()                        -> [] (what is still undecided at the end is too close to it)

    Candidate i is decided once frame i + min_shot - 1 has arrived - `n - i >= min_shot` is then true whatever follows - or at the
    end of the stream; candidates are decided in order, so `cuts` is exactly select_cuts(scores, n, threshold, min_shot) for every
    piece pattern.  State for a consumer: `arrived` frames seen, `released` - frames below it belong to their shot for good (no
    undecided candidate precedes them; arrived - released < min_shot), `cuts`, `confirmed_at[cut]` = `arrived` when it was confirmed,
    `scores` and `mafd` of every frame."""

    def __init__(self, threshold=DEFAULT_THRESHOLD, min_shot=2):
        self.threshold, self.min_shot = _check_rule(threshold, min_shot)
        self.scores, self.mafd, self.cuts, self.confirmed_at = [], [], [], {}
        self.start = 0       # first frame of the running shot
        self.released = 0    # the next frame to decide (frame 0 is never a candidate)
        self.finished = False

    @property
    def arrived(self):
        return len(self.scores)

    def _decide(self, final):
        new, n = [], len(self.scores)
        while self.released < n:
            i = self.released
            if i >= 1 and self.scores[i] >= self.threshold and i - self.start >= self.min_shot:
                if n - i < self.min_shot:
                    if not final:
                        break  # wait for frame i + min_shot - 1
                else:
                    new.append(i)
                    self.confirmed_at[i] = n
                    self.start = i
            self.released = i + 1
        self.cuts += new
        return new

    def push(self, scores):
        """The scores of the frames that have just arrived (the first frame of the video has any score: it is not looked at)."""
        if self.finished:
            raise RuntimeError('ShotDetector: push after finish')
        self.scores += [float(s) for s in scores]
        self.mafd += [None] * (len(self.scores) - len(self.mafd))
        return self._decide(False)

    def push_sad(self, sad, pixels):
        """The same from ops.frame_sad's integers for the new frames (chained through `prev`) and pixels = H W."""
        before = self.mafd[-1] if self.mafd else 0.0
        mafd, scores = cut_scores(sad, pixels, before)
        first = len(self.scores)
        new = self.push(scores)
        self.mafd[first:] = mafd
        return new

    def finish(self):
        """The stream has ended: every frame is released; returns the cuts confirmed now (none: they would be too close to the end)."""
        self.finished = True
        return self._decide(True)
