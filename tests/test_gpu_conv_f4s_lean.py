"""-m gpu: the lean column-pass instances of the split-operand F(4x4) kernel (csrc/winograd_f4s.hip) against the generic ones.

A work item (64 output channels x 32 tiles) wholly inside the tensor, with a plain store, none / relu / lrelu and at most one addend,
takes an instance without row / column / channel tests; every other item of the same launch keeps the generic instance.  The two must
give the SAME BITS - y and the y_amax slot - and both sit within the F(4x4) kernels' tolerance of an fp64 convolution.  The shapes are
the smallest that mix both kinds of item in one launch, for both block shapes (64x8 and 32x16 pixels), plus one all-lean launch each."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_f4 import RTOL_F4, _rel

pytestmark = pytest.mark.gpu

# (n, ci, co, h, w): expected lean items of a launch, of how many
SHAPES = {
    'mixed_64x8': ((2, 32, 64, 20, 160), 8, 18),    # 3 x 3 blocks of 64x8, last column and last row partial: 2 * 2 per image
    'mixed_32x16': ((2, 40, 144, 28, 80), 8, 36),   # 3 x 2 blocks of 32x16, partial in x, y and channels (144 = 64 + 64 + 16), 5 chunks
    'all_64x8': ((1, 64, 128, 16, 128), 8, 8),
    'all_32x16': ((1, 32, 64, 32, 32), 2, 2),
}
ACTS = {'none': 0, 'relu': 1, 'lrelu': 2}
PRE_MAP = (2, 1, 0)  # image i takes image i // 2 of `pre`


@functools.lru_cache(maxsize=None)
def _case(shape_key, c2=0, ci=None):
    """Inputs and the fp64 convolution (bias included) of one shape, computed once and never modified."""
    (n, c, co, h, w), _, _ = SHAPES[shape_key]
    c = c if ci is None else ci
    g = torch.Generator().manual_seed(1000 + 17 * sorted(SHAPES).index(shape_key) + c2 + c)
    x1 = torch.randn(n, c, h, w, generator=g)
    x2 = torch.randn(n, c2, h, w, generator=g) if c2 else None
    wt = torch.randn(co, c + c2, 3, 3, generator=g) * 0.1
    b = torch.randn(co, generator=g)
    res = torch.randn(n, co, h, w, generator=g)
    pre = torch.randn((n + 1) // 2, co, h, w, generator=g)
    conv = F.conv2d((x1 if x2 is None else torch.cat([x1, x2], 1)).double(), wt.double(), b.double(), 1, 1)
    return x1, x2, wt, b, res, pre, conv


def _reference(conv, act, add, res, pre, n):
    v = conv
    if add == 'pre':
        v = v + pre[[i // PRE_MAP[0] * PRE_MAP[1] + PRE_MAP[2] for i in range(n)]].double()
    if act == 'relu':
        v = F.relu(v)
    elif act == 'lrelu':
        v = F.leaky_relu(v, 0.1)
    if add == 'res1':
        v = 0.5 * v + res.double()
    return v


def _lean_items(n, c1, c2, h, w, co, act, add, y_amax=True):
    from edvr_amd import _lib, ops
    d = _lib.ConvDesc()
    d.c1, d.c2, d.n, d.h, d.w, d.co, d.ks, d.stride, d.algo, d.act = c1, c2, n, h, w, co, 3, 1, ops.CONV_WINOGRAD_F4S, ACTS[act]
    d.x1 = d.wpk_f4s = d.x_amax = 4096  # (host-only query: nothing is dereferenced)
    if c2:
        d.x2 = 4096
    if y_amax:
        d.y_amax = 4096
    if add == 'res1':
        d.res1, d.y_scale = 4096, 0.5
    elif add == 'pre':
        d.pre, d.pre_n, d.pre_img_stride = 4096, (n + 1) // 2, co * h * w
        d.pre_div, d.pre_mul, d.pre_add = PRE_MAP
    return _lib.lib().edvr_conv2d_f4s_lean_items(ctypes.byref(d))


def _run_both(gpu, x1, x2, wt, b, act, add, res, pre):
    """The same launch with the lean instances on and off: (y, y_amax bits) of each."""
    from edvr_amd import _lib, ops
    L = _lib.lib()
    wg = wt.to(gpu)
    wpk, wf4s = ops.pack_conv_weight(wg), ops.pack_conv_weight(wg, f4s=True)
    x1g, x2g = x1.to(gpu), None if x2 is None else x2.to(gpu)
    kw = dict(x2=x2g, act=ACTS[act], wpk_f4s=wf4s, algo=ops.CONV_WINOGRAD_F4S)
    if add == 'res1':
        kw.update(res1=res.to(gpu), y_scale=0.5)
    elif add == 'pre':
        kw.update(pre=pre.to(gpu), pre_map=PRE_MAP)
    out = []
    prev = L.edvr_conv2d_f4s_set_lean(1)
    try:
        for on in (1, 0):
            L.edvr_conv2d_f4s_set_lean(on)
            y = ops.conv2d(x1g, wpk, None if b is None else b.to(gpu), wt.shape[0], 3, **kw)
            bound = ops.get_bound(y)
            assert bound is not None
            torch.cuda.synchronize()
            out.append((y, int(bound.view(torch.int32).item()) & 0xffffffff))
    finally:
        L.edvr_conv2d_f4s_set_lean(prev)
    return out


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('add', ['none', 'res1', 'pre'])
@pytest.mark.parametrize('act', list(ACTS))
@pytest.mark.parametrize('shape_key', list(SHAPES))
def test_lean_equals_generic_bitwise(gpu, shape_key, act, add):
    from edvr_amd import _lib
    (n, c, co, h, w), lean, total = SHAPES[shape_key]
    L = _lib.lib()
    prev = L.edvr_conv2d_f4s_set_lean(1)
    try:
        assert _lean_items(n, c, 0, h, w, co, act, add) == lean > 0
        L.edvr_conv2d_f4s_set_lean(0)
        assert _lean_items(n, c, 0, h, w, co, act, add) == 0
    finally:
        L.edvr_conv2d_f4s_set_lean(prev)
    x1, x2, wt, b, res, pre, conv = _case(shape_key)
    (y_on, a_on), (y_off, a_off) = _run_both(gpu, x1, x2, wt, b, act, add, res, pre)
    ref = _reference(conv, act, add, res, pre, n)
    e_on, e_off = _rel(y_on, ref), _rel(y_off, ref)
    print(f'{shape_key} {act} {add}: lean items {lean}/{total}, rel err lean {e_on:.3g} generic {e_off:.3g}, y_amax bits {a_on:#x} {a_off:#x}')
    assert _same_bits(y_on, y_off)
    assert a_on == a_off
    assert e_on < RTOL_F4 and e_off < RTOL_F4, (e_on, e_off)
    # the slot is the maximum over everything stored (rows below the image included: still a bound)
    assert torch.tensor(a_on, dtype=torch.int64).to(torch.int32).view(torch.float32).item() >= y_on.abs().max().item()


def test_lean_two_inputs(gpu):
    """x1 + x2 (c1 = c2 = 32) on the mixed 64x8 shape: the staging waves switch from x1 to x2 inside every item."""
    (n, c, co, h, w), lean, _ = SHAPES['mixed_64x8']
    x1, x2, wt, b, res, pre, conv = _case('mixed_64x8', c2=32)
    assert _lean_items(n, c, 32, h, w, co, 'lrelu', 'res1') == lean
    (y_on, a_on), (y_off, a_off) = _run_both(gpu, x1, x2, wt, b, 'lrelu', 'res1', res, pre)
    assert _same_bits(y_on, y_off) and a_on == a_off
    assert _rel(y_on, _reference(conv, 'lrelu', 'res1', res, pre, n)) < RTOL_F4


@pytest.mark.parametrize('ci', [33, 34])
def test_lean_padding_channels(gpu, ci):
    """ci = 33 / 34 on the all-lean 32x16 shape: the last chunk's channel pairs are (32, 33) with one / two real planes and three
    pairs of padding (a one-plane and an empty input buffer)."""
    (n, _, co, h, w), lean, _ = SHAPES['all_32x16']
    x1, x2, wt, b, res, pre, conv = _case('all_32x16', ci=ci)
    assert _lean_items(n, ci, 0, h, w, co, 'relu', 'pre') == lean
    (y_on, a_on), (y_off, a_off) = _run_both(gpu, x1, x2, wt, b, 'relu', 'pre', res, pre)
    assert _same_bits(y_on, y_off) and a_on == a_off
    assert _rel(y_on, _reference(conv, 'relu', 'pre', res, pre, n)) < RTOL_F4


def _nonfinite(bits):
    return (bits & 0x7f800000) == 0x7f800000


@pytest.mark.parametrize('value', [float('inf'), float('-inf'), float('nan')])
def test_lean_sticky_nonfinite_residual(gpu, value):
    """One non-finite element of the residual inside a lean item (the first block of the mixed shape): the slot keeps it, same bits."""
    (n, c, co, h, w), _, _ = SHAPES['mixed_64x8']
    x1, x2, wt, b, res, pre, conv = _case('mixed_64x8')
    res = res.clone()
    res[1, 37, 5, 70] = value  # image 1, block row 0, block column 1: inside
    (y_on, a_on), (y_off, a_off) = _run_both(gpu, x1, x2, wt, b, 'none', 'res1', res, pre)
    assert _same_bits(y_on, y_off)
    assert a_on == a_off and _nonfinite(a_on), (hex(a_on), hex(a_off))
    assert (a_on & 0x007fffff != 0) == (value != value)  # a NaN stays a NaN, an infinity an infinity


def test_lean_sticky_nan_input(gpu):
    (n, c, co, h, w), _, _ = SHAPES['all_32x16']
    x1, x2, wt, b, res, pre, conv = _case('all_32x16')
    x1 = x1.clone()
    x1[0, 3, 9, 9] = float('nan')
    (y_on, a_on), (y_off, a_off) = _run_both(gpu, x1, x2, wt, b, 'lrelu', 'none', res, pre)
    assert _same_bits(y_on, y_off)
    assert a_on == a_off and _nonfinite(a_on) and (a_on & 0x007fffff), (hex(a_on), hex(a_off))


def test_lean_all_minus_zero(gpu):
    """relu = max(v, 0 * v) of a negative v is -0: zero input and a negative bias store -0 everywhere; the slot stays 0."""
    (n, c, co, h, w), _, _ = SHAPES['all_32x16']
    x1, x2, wt, b, res, pre, conv = _case('all_32x16')
    (y_on, a_on), (y_off, a_off) = _run_both(gpu, torch.zeros_like(x1), None, wt, -torch.ones(co), 'relu', 'none', res, pre)
    assert _same_bits(y_on, y_off)
    assert bool((y_on.view(torch.int32) == -(1 << 31)).all())
    assert a_on == a_off == 0


def test_lean_only_negative_outputs(gpu):
    """Zero input, negative biases, no activation: every stored value is negative and finite, so the signed maximum stays at its start
    value and the slot comes from the unsigned one alone - the bits of the largest |bias|."""
    (n, c, co, h, w), _, _ = SHAPES['all_32x16']
    x1, x2, wt, b, res, pre, conv = _case('all_32x16')
    bias = -(1.0 + b.abs())
    (y_on, a_on), (y_off, a_off) = _run_both(gpu, torch.zeros_like(x1), None, wt, bias, 'none', 'none', res, pre)
    assert _same_bits(y_on, y_off)
    assert bool((y_on < 0).all())
    want = int(bias.abs().max().view(torch.int32).item())
    assert a_on == a_off == want, (hex(a_on), hex(a_off), hex(want))
