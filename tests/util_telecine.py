"""Inputs shared by the inverse-telecine tests (test_telecine_cpu.py, test_gpu_telecine.py): the designed film clip, 2:3 pulldown of it
at six truncation phases, noise, and random frames."""
import numpy as np

import deint_ref as D
from util_deint import random_frames, y4m_bytes  # noqa: F401  (the same random frames and Y4M wrapper as the deinterlacing tests)

FILM_H, FILM_W, FILM_FRAMES = 36, 70, 14

# (fields of the even film frames, fields of the odd ones, fields cut from the start of the stream).  The first four leave every first
# field with its partner; the last two begin with an orphan: a first field whose partner was cut.
PHASES = [(2, 3, 0), (2, 3, 2), (3, 2, 0), (3, 2, 1), (2, 3, 1), (3, 2, 2)]
ORPHAN_FREE = (0, 1, 2, 3)


def _picture(t, R, C, sh):
    """Film frame t on an (R, C) grid: a ramp that moves 3 columns per frame over a vertical sawtooth, a flat box that jumps about, and
    three static one-row lines, which comb a progressive frame as much as the definition tolerates (80 samples of a 16 x 16 block)."""
    yy, xx = np.mgrid[0:R, 0:C]
    pic = 40 + 6 * ((xx + 3 * t) % 24) + 2 * (yy % 9)
    bx, by = (3 + 7 * t) % max(C - 24, 1), (2 + 3 * t) % max(R - 18, 1)
    pic[by:by + 16, bx:bx + 24] = 16 + (37 * t) % 200
    for r in (R - 9, R - 7, R - 5):
        pic[r] = 235
    return pic.astype(np.int64) << sh


def film_clip(n=FILM_FRAMES, H=FILM_H, W=FILM_W, fmt='420'):
    """uint8 (n, framesize): n progressive film frames, every plane by the same recipe at its own size."""
    sh = D.parse_format(fmt)[2] - 8
    return D.join([np.stack([_picture(t, R, C, sh) for t in range(n)]) for R, C in D.plane_shapes(H, W, fmt)], fmt)


def field_sources(n_film, phase):
    """The film frame behind every field of the telecined stream, in time order."""
    even, odd, cut = PHASES[phase]
    fields = [j for j in range(n_film) for _ in range(odd if j % 2 else even)]
    return fields[cut:]


def telecine(film, first, phase, H=FILM_H, W=FILM_W, fmt='420'):
    """Pulldown of uint8 (n, framesize) film frames: (video frames uint8 (m, framesize), src) - field f of the stream shows film frame
    src[f] on the rows of parity (f + q) % 2; video frame v weaves fields 2 v and 2 v + 1; a last odd field is dropped."""
    q = D.FIRST[first]
    src = field_sources(film.shape[0], phase)
    m = len(src) // 2
    planes = D.split(film, H, W, fmt)
    out = []
    for p in planes:
        v = np.empty((m,) + p.shape[1:], np.int64)
        for i in range(m):
            v[i, q::2] = p[src[2 * i], q::2]
            v[i, 1 - q::2] = p[src[2 * i + 1], 1 - q::2]
        out.append(v)
    return D.join(out, fmt), src[:2 * m]


def add_noise(frames, H, W, fmt, amp, seed):
    """Independent uniform noise of -amp ... amp levels (of the format's depth) on every sample of every video frame, clipped."""
    if not amp:
        return frames
    rng = np.random.default_rng(seed)
    maxv = (1 << D.parse_format(fmt)[2]) - 1
    return D.join([np.clip(p + rng.integers(-amp, amp + 1, size=p.shape), 0, maxv) for p in D.split(frames, H, W, fmt)], fmt)


def partners(src):
    """Per video frame: the match that completes its first field - 0 (c) where its second field shows the same film frame, 1 (p) where
    the field before does, None for an orphan (neither does)."""
    out = []
    for v in range(len(src) // 2):
        f = src[2 * v]
        out.append(0 if src[2 * v + 1] == f else 1 if v and src[2 * v - 1] == f else None)
    return out
