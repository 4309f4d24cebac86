"""Shared by the BD downsampling tests: the fixture of scripts/make_bd_golden.py and a float64 restatement of the formula
(duf_downsample, basicsr/data/data_util.py:281-331):

    out[i, j] = sum_{a, b = 0..12} g[a] g[b] x[R(i s - 6 + a, h), R(j s - 6 + b, w)],  R(p, n) = -p (p < 0), 2 (n - 1) - p (p >= n), p

with g the 1-D Gaussian of sigma 0.4 s truncated at int(4 sigma + 0.5) samples and normalised - written out here, independent of
edvr_amd.data.bd_weights."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bd_downsample.pt')
FIXTURE_CASES = [((h, w), s) for (h, w) in ((64, 96), (37, 53), (45, 63), (30, 44)) for s in (2, 3, 4)]
FIXTURE_FRAMES = 2


def load_golden():
    return torch.load(GOLDEN, weights_only=True)['cases']


def gauss13(scale):
    sigma, d = 0.4 * scale, np.arange(-6, 7)
    g = np.where(np.abs(d) <= int(4 * sigma + 0.5), np.exp(-d.astype(np.float64) ** 2 / (2 * sigma * sigma)), 0.0)
    return g / g.sum()


def axis_matrix(n, scale):
    """(ceil(n / scale), n) float64: row i holds g at the reflected positions of i * scale - 6 .. i * scale + 6."""
    assert n >= 7, 'one reflection must cover the reach of 6'
    m = np.zeros((-(-n // scale), n))
    for i in range(m.shape[0]):
        for a, ga in enumerate(gauss13(scale)):
            p = i * scale - 6 + a
            m[i, -p if p < 0 else (2 * (n - 1) - p if p >= n else p)] += ga
    return torch.from_numpy(m)


def bd_f64(x, scale):
    """x (..., h, w) -> (..., ceil(h / scale), ceil(w / scale)) in float64."""
    return (axis_matrix(x.shape[-2], scale) @ x.double()) @ axis_matrix(x.shape[-1], scale).t()


def to_u8(x):
    """tensor2img of a float tensor in float32: clamp, x 255, round half to even."""
    return (x.float().clamp(0, 1) * 255).round().to(torch.uint8)
