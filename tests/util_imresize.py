"""Shared by the imresize tests: the fixture of scripts/make_imresize_golden.py and a float64 restatement of the resampling formula
(basicsr/utils/matlab_functions.py:6-170) as one dense matrix per axis with symmetric index folding."""
import math
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'imresize.pt')
FIXTURE_CASES = [((64, 96), 1 / 4), ((37, 53), 1 / 4), ((48, 60), 1 / 2), ((45, 63), 1 / 3), ((50, 70), 0.3), ((30, 44), 2.0), ((30, 44), 4.0)]


def load_golden():
    return torch.load(GOLDEN, weights_only=True)['cases']


def _cubic(x):
    a = x.abs()
    return (1.5 * a ** 3 - 2.5 * a ** 2 + 1) * (a <= 1) + (-0.5 * a ** 3 + 2.5 * a ** 2 - 4 * a + 2) * ((a > 1) & (a <= 2))


def axis_matrix(n_in, scale, antialiasing=True):
    """(ceil(n_in * scale), n_in) float64: row x holds the normalised cubic weights of output x, taps outside the frame folded back
    by the symmetric extension (... 1 0 | 0 1 ...)."""
    n_out = math.ceil(n_in * scale)
    aa = scale < 1 and antialiasing
    kw = 4 / scale if aa else 4.0
    x = torch.arange(1, n_out + 1, dtype=torch.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = torch.floor(u - kw / 2)
    p = math.ceil(kw) + 2
    idx = left[:, None] + torch.arange(p, dtype=torch.float64)[None]  # 1-based
    d = u[:, None] - idx
    w = scale * _cubic(d * scale) if aa else _cubic(d)
    w = w / w.sum(1, keepdim=True)
    i = idx.long() - 1
    i = torch.where(i < 0, -i - 1, torch.where(i >= n_in, 2 * n_in - 1 - i, i))
    assert ((i >= 0) & (i < n_in))[w != 0].all(), 'the frame is shorter than the symmetric extension reaches'
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    m.scatter_add_(1, i.clamp(0, n_in - 1), w)
    return m


def imresize_f64(x, scale, antialiasing=True):
    """x (..., h, w) -> (..., h', w') in float64: rows first, then columns."""
    x = x.double()
    my, mx = axis_matrix(x.shape[-2], scale, antialiasing), axis_matrix(x.shape[-1], scale, antialiasing)
    return (my @ x) @ mx.t()


def to_u8(x):
    """tensor2img of a float tensor in float32: clamp, x 255, round half to even."""
    return (x.float().clamp(0, 1) * 255).round().to(torch.uint8)
