"""No GPU: the host side of the split-operand F(4x4) kernel's lean column-pass instances (csrc/winograd_f4s.hip).

edvr_conv2d_f4s_lean_items counts the work items (64 output channels x 32 tiles) of a launch that take a lean instance: blocks wholly
inside the tensor, plain NCHW store, none / relu / lrelu with one slope per block, at most one addend.  The counts below follow from
the block geometry alone (f4s_geometry: 64x8-pixel or 32x16-pixel blocks, whichever pads the image less).  The second half proves the
identity the lean instances' y_amax rests on: two running maxima over RAW bit patterns give max(bits & 0x7fffffff)."""
import ctypes
import itertools

import numpy as np
import pytest

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SIGMOID = 0, 1, 2, 3
OUT_PIXEL_SHUFFLE2 = 1


def _desc(n, c, h, w, co, **kw):
    from edvr_amd import _lib, ops
    d = _lib.ConvDesc()
    d.c1, d.n, d.h, d.w, d.co, d.ks, d.stride, d.algo = c, n, h, w, co, 3, 1, ops.CONV_WINOGRAD_F4S
    d.wpk_f4s = d.x_amax = 4096  # (any non-null, 16-byte aligned value: nothing is dereferenced)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _items(d):
    from edvr_amd import _lib
    return _lib.lib().edvr_conv2d_f4s_lean_items(ctypes.byref(d))


@pytest.fixture
def lean_on():
    from edvr_amd import _lib
    prev = _lib.lib().edvr_conv2d_f4s_set_lean(1)
    yield
    _lib.lib().edvr_conv2d_f4s_set_lean(prev)


@pytest.mark.parametrize('h,w,co,per_image', [
    (180, 320, 128, 220),  # 64x8 blocks, 5 x 23, the last block row partial: 5 * 22 * 2 of 230
    (90, 160, 128, 50),    # 32x16 blocks, 5 x 6, the last block row partial: 5 * 5 * 2 of 60
    (45, 80, 128, 8),      # 32x16 blocks, 3 x 3, partial in x and y: 2 * 2 * 2 of 18
    (180, 320, 216, 330),  # four channel blocks, the fourth (24 channels) never: 5 * 22 * 3 of 460
])
def test_lean_items_follow_the_block_geometry(lean_on, h, w, co, per_image):
    for n in (1, 3):
        assert _items(_desc(n, 64, h, w, co)) == n * per_image
        assert _items(_desc(n, 64, h, w, co, act=ACT_LRELU, res1=4096, y_scale=0.5, y_amax=4096)) == n * per_image
        assert _items(_desc(n, 64, h, w, co, act=ACT_RELU, pre=4096, pre_n=1, pre_div=n, pre_img_stride=co * h * w)) == n * per_image


def test_lean_items_exclusions(lean_on):
    n, c, h, w, co = 1, 64, 16, 128, 128
    assert _items(_desc(n, c, h, w, co)) == 8  # 2 x 2 blocks of 64x8, two channel blocks, all inside
    assert _items(_desc(n, c, h, w, co, gate=4096, gate_slope=0.1)) == 0
    assert _items(_desc(n, c, h, w, co, res1=4096, res2=4096)) == 0
    assert _items(_desc(n, c, h, w, co, abs_sum=4096, abs_sum_channels=co)) == 0
    assert _items(_desc(n, c, h, w, co, out_mode=OUT_PIXEL_SHUFFLE2)) == 0
    assert _items(_desc(n, c, h, w, co, act=ACT_SIGMOID)) == 0
    assert _items(_desc(n, c, h, w, co, act=ACT_SIGMOID, act_from=64)) == 0
    # act_from inside a block: that block has two slopes; the blocks from act_from's own block boundary on have one
    assert _items(_desc(n, c, h, w, co, act=ACT_LRELU, act_from=64)) == 4
    assert _items(_desc(n, c, h, w, co, act=ACT_LRELU, act_from=65)) == 0
    assert _items(_desc(n, c, h, w, co, act=ACT_LRELU, act_from=1)) == 4
    assert _items(_desc(n, c, h, w, co, act=ACT_NONE, act_from=65)) == 8  # no activation: act_from means nothing
    # not the split-operand kernel's launch at all
    assert _items(_desc(n, c, h, w, co, wpk_f4s=None)) == 0
    assert _items(_desc(n, c, h, w, co, stride=2)) == 0
    assert _items(_desc(n, c, h, 126, co)) == 0  # w % 4 != 0


def test_lean_switch_returns_the_previous_setting():
    from edvr_amd import _lib
    L = _lib.lib()
    first = L.edvr_conv2d_f4s_set_lean(0)
    try:
        assert first in (0, 1)
        assert _items(_desc(1, 64, 16, 128, 128)) == 0  # switched off: every item takes the generic instances
        assert L.edvr_conv2d_f4s_set_lean(1) == 0
        assert _items(_desc(1, 64, 16, 128, 128)) == 8
        assert L.edvr_conv2d_f4s_set_lean(7) == 1  # any non-zero value is "on"
        assert L.edvr_conv2d_f4s_set_lean(1) == 1
    finally:
        L.edvr_conv2d_f4s_set_lean(first)


# ---------------------------------------------------------------------------------------------- the y_amax identity
def _slot_generic(bits):
    """Today's slot semantics: the unsigned maximum of (bits & 0x7fffffff) - a NaN orders above +inf, non-finite values are sticky."""
    return int((bits & np.uint32(0x7fffffff)).max())


def _slot_lean(bits):
    """The lean instances: P = signed maximum of the raw patterns, U = unsigned maximum, both starting at 0; combined once."""
    p = max(0, int(bits.view(np.int32).max()))
    u = max(0, int(bits.max()))
    return max(max(p, 0), u & 0x7fffffff)


SPECIAL = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x3f800000, 0xbf800000,
           0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7f800001, 0xff800001, 0x7fc00000, 0xffc00000, 0x7fffffff, 0xffffffff]


def test_two_raw_maxima_give_the_abs_bits_maximum():
    for k in (1, 2, 3):
        for combo in itertools.product(SPECIAL, repeat=k):  # every set of up to three special values: -0, denormals, +-inf, NaNs of either sign
            bits = np.array(combo, dtype=np.uint32)
            assert _slot_lean(bits) == _slot_generic(bits), [hex(v) for v in combo]
    rng = np.random.default_rng(5)
    for _ in range(300):
        bits = rng.integers(0, 1 << 32, size=int(rng.integers(1, 40)), dtype=np.uint64).astype(np.uint32)
        if rng.random() < 0.5:
            bits[int(rng.integers(0, bits.size))] = SPECIAL[int(rng.integers(0, len(SPECIAL)))]
        if rng.random() < 0.3:
            bits |= np.uint32(0x80000000)  # only negative values: P stays at its start value
        assert _slot_lean(bits) == _slot_generic(bits)
