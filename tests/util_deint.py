"""Inputs shared by the deinterlacing tests (test_deinterlace_cpu.py, test_gpu_deinterlace.py): random interlaced frames, the structured
clip whose coverage the CPU test asserts, the extremes, and a Y4M stream around frames."""
import numpy as np

import deint_ref as D


def random_frames(n, H, W, fmt, seed):
    """uint8 (n, framesize): uniform samples of the format's depth (little-endian words above 8 bits)."""
    rng = np.random.default_rng(seed)
    depth = D.parse_format(fmt)[2]
    planes = [rng.integers(0, 1 << depth, size=(n, r, c)) for r, c in D.plane_shapes(H, W, fmt)]
    return D.join(planes, fmt)


def _picture(t, R, C, maxv):
    """What a progressive camera sees at field time t on an (R, C) grid: left, a static texture; right, a bright bar in two parts that
    moves 3 columns per field - the upper part's edges move one column per row (slope +1 left, -1 right), the lower part's two columns
    per row (slope +1/2, -1/2) - over a dim static ramp."""
    yy, xx = np.mgrid[0:R, 0:C]
    static = C // 3
    pic = np.where(xx < static, maxv // 8 + ((xx * 7 + yy * 13 + (xx * yy) % 5 * 3) % 17) * (maxv // 40), maxv // 10 + (xx * (maxv // 16)) // max(C, 1))
    cx = static + 10 + 3 * t
    half = R // 2
    upper = (yy < half) & (xx >= cx - 8 + yy) & (xx <= cx + 8 - yy)
    lower = (yy >= half) & (xx >= cx - 12 + 2 * (yy - half)) & (xx <= cx + 12 - 2 * (yy - half))
    bar = (upper | lower) & (xx >= static)
    return np.where(bar, (maxv * 9) // 10, pic).astype(np.int64)


def structured_clip(n, H, W, fmt='420', first='top'):
    """uint8 (n, framesize): every plane weaves, per frame i, the rows of `first`'s parity of the picture at time 2 i with the other
    rows of the picture at time 2 i + 1 (each plane on its own grid)."""
    b = D.FIRST[first]
    maxv = (1 << D.parse_format(fmt)[2]) - 1
    planes = []
    for R, C in D.plane_shapes(H, W, fmt):
        pl = np.empty((n, R, C), np.int64)
        for i in range(n):
            pl[i, b::2] = _picture(2 * i, R, C, maxv)[b::2]
            pl[i, 1 - b::2] = _picture(2 * i + 1, R, C, maxv)[1 - b::2]
        planes.append(pl)
    return D.join(planes, fmt)


def extreme_clips(n, H, W, fmt):
    """Three clips: every sample 0, every sample M = 2^d - 1, and the two fields of every frame alternately 0 and M (the largest
    differences and sums the rule can meet: M + M must not wrap)."""
    maxv = (1 << D.parse_format(fmt)[2]) - 1
    out = []
    for kind in ('zero', 'max', 'alternate'):
        planes = []
        for R, C in D.plane_shapes(H, W, fmt):
            pl = np.zeros((n, R, C), np.int64)
            if kind == 'max':
                pl[:] = maxv
            elif kind == 'alternate':
                pl[:, 1::2] = maxv
            planes.append(pl)
        out.append(D.join(planes, fmt))
    return out


def y4m_bytes(frames, H, W, tags):
    """A YUV4MPEG2 stream around uint8 (n, framesize) frames; tags: the header after W and H, e.g. 'F25:1 It C420jpeg'."""
    head = f'YUV4MPEG2 W{W} H{H} {tags}\n'.encode()
    return head + b''.join(b'FRAME\n' + np.ascontiguousarray(f).tobytes() for f in frames)
