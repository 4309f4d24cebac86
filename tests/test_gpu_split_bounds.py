"""-m gpu: the magnitude bounds of the split-operand kernels (csrc/winograd_f4s.hip, csrc/conv1x1_s.hip, the amax reduction).

Every split kernel scales its operands into the f16 range from a device-side bound.  The kernel that produces a tensor writes that
bound (`y_amax`), the next layer reads it (`x_amax`), and the overflow guard (ops.split_guard_*) reads the same slots to learn of
non-finite values, which must stay in the slot (NaN bits order above +inf).  Checked here against float64 references:
  - a seeded random-shape sweep of the split F(4x4) kernel: every epilogue, the three column-pass variants (scalar, vector, vector +
    PixelShuffle), both block shapes, ragged rows / columns, channel padding, strided views, the data gradient, the abs_sum epilogue;
  - the y_amax contract: a bound, exact where no block reaches past the image, within rounding of the zero-padded extent elsewhere,
    and folded into (not written over) whatever the slot held;
  - a non-finite sentinel matrix: one NaN / +inf / -inf per launch, from every source, at every position class of a tile and of
    the image: it must reach the output where the float64 reference has it, and the slot, and the guard."""
import ctypes
import random
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_f4 import RTOL_F4, _rel
from test_gpu_conv_f4s import C1X1_CASES, _c1x1_tensors

pytestmark = pytest.mark.gpu

F4S_NAME = 'conv3x3_winograd_f4s_kernel'
NONFINITE = [float('nan'), float('inf'), float('-inf')]


def _geometry(h, w):
    """csrc/winograd_f4s.hip f4s_geometry: (block height, block width) of the launch - 8 x 64, or 16 x 32 where that pads less."""
    pad16 = -(-w // 64) * 64 * (-(-h // 8) * 8)
    pad8 = -(-w // 32) * 32 * (-(-h // 16) * 16)
    return (16, 32) if pad8 < pad16 else (8, 64)


class _Names:
    """Kernel names of the launches inside the block, as ops.conv2d resolves them (edvr_conv2d_kernel_name on the launch's own desc)."""

    def __enter__(self):
        from edvr_amd import ops
        self.seen = []
        ops.LAUNCH_HOOK = lambda name, flops, launch, *a: (self.seen.append(name), launch())
        return self

    def __exit__(self, *exc):
        from edvr_amd import ops
        ops.LAUNCH_HOOK = None

    def convs(self):
        return [k for k in self.seen if k.startswith('conv')]


@pytest.fixture
def guard(gpu, monkeypatch):
    """The overflow guard in 'raise' mode with nothing pending; left the same way for the next test."""
    from edvr_amd import ops

    def drain():
        ops._arena(gpu).take_unexamined()
        ops._GUARD_PENDING.clear()
    monkeypatch.setattr(ops, 'SPLIT_GUARD', 'raise')
    drain()
    yield ops
    drain()


def _assert_guard_trips(ops, dev):
    ops.split_guard_submit(dev)
    with pytest.raises(ops.SplitOperandOverflow):
        ops.split_guard_check(wait=True)
    ops.split_guard_check(wait=True)  # once: nothing else pending


def _assert_guard_quiet(ops, dev):
    ops.split_guard_submit(dev)
    ops.split_guard_check(wait=True)


# ------------------------------------------------------------------------------------------------ 1. random-shape sweep
F4S_MODES = ['plain', 'relu', 'lrelu', 'sigmoid_from', 'relu_res1', 'lrelu_res2', 'res1_scaled', 'gate_relu', 'gate_lrelu_scaled',
             'shuffle', 'x2', 'x2_map']
_VIEWS = {3: 'x1_slice', 5: 'res_slice', 7: 'out_slice', 9: 'misaligned'}  # case index % 11 -> strided view of the case


def _f4s_cases(n_cases, seed):
    rng = random.Random(seed)
    cases = []
    for i in range(n_cases):
        mode = F4S_MODES[i % len(F4S_MODES)]
        c1 = rng.choice([3, 8, 20, 36, 64, 100, 128])
        co = rng.choice([16, 48, 64, 70, 100, 128, 216])
        if i % 11 == 0 or i % 12 == 5:  # no block reaches past the image: the bound must be max |y| bit for bit
            h, w = 16 * rng.randint(1, 3), 64 * rng.randint(1, 2)
        else:
            h, w = rng.randint(4, 40), 4 * rng.randint(8, 40)  # w in 32..160, a multiple of 4 (the kernel's eligibility rule)
        n = rng.randint(1, 2)
        c2 = 0
        if mode.startswith('x2'):
            c1, c2 = rng.choice([(16, 16), (64, 64), (100, 20), (36, 12)])  # c1 even: a staging wave's channel pair never straddles
            if mode == 'x2_map':
                n = rng.choice([2, 3]) * rng.randint(1, 2)
        if mode == 'shuffle':
            co = co // 4 * 4
        view = _VIEWS.get(i % 11, 'none')
        if view == 'res_slice' and 'res' not in mode:
            view = 'out_slice'
        flip = i % 11 == 10  # the data-gradient packing (transpose_flip)
        cases.append((n, c1, c2, h, w, co, mode, view, flip))
    return cases


CASES_F4S = _f4s_cases(44, 20261016)


def _case_id(c):
    return 'n%d_c%d+%d_%dx%d_co%d_%s_%s%s' % (c[:8] + ('_flip' if c[8] else '',))


def test_f4s_sweep_covers_every_path():
    """The sweep reaches all three column-pass variants, both block shapes, ragged rows and columns, and exact geometries."""
    seen = set()
    for n, c1, c2, h, w, co, mode, view, flip in CASES_F4S:
        bh, bw = _geometry(h, w)
        seen.add(('block', bh))
        if w >= bw:
            seen.add('shuffle_vec' if mode == 'shuffle' else 'vec')
        if w % bw:
            seen.add('scalar')
        if h % 4:
            seen.add('rows_in<4')
        if h % bh == 0 and w % bw == 0:
            seen.add('exact')
        if co % 64:
            seen.add('co_padding')
        if flip:
            seen.add('flip')
        seen.add(view)
    want = {('block', 8), ('block', 16), 'vec', 'shuffle_vec', 'scalar', 'rows_in<4', 'exact', 'co_padding', 'flip', 'x1_slice',
            'res_slice', 'out_slice', 'misaligned'}
    assert want <= seen, want - seen


def _epilogue(conv, mode, co, g, h, w):
    """The epilogue of `mode` on a float64 conv result over the zero-padded extent; returns (y, conv2d kwargs, residual / gate
    tensors drawn from g - zero outside the h x w image, as the kernel reads them)."""
    from edvr_amd import ops
    kw, extra = {}, {}
    y = conv

    def draw():
        t = torch.randn(y.shape, generator=g)
        t[..., h:, :] = 0.0
        t[..., :, w:] = 0.0
        return t
    if mode in ('lrelu', 'lrelu_res2', 'shuffle', 'x2', 'x2_map'):
        y, kw['act'] = F.leaky_relu(y, 0.1), ops.ACT_LRELU
    elif mode in ('relu', 'relu_res1'):
        y, kw['act'] = F.relu(y), ops.ACT_RELU
    elif mode == 'sigmoid_from':
        af = 2 * co // 3
        y = torch.cat([y[:, :af], torch.sigmoid(y[:, af:])], 1)
        kw.update(act=ops.ACT_SIGMOID, act_from=af)
    if mode in ('res1_scaled', 'gate_lrelu_scaled'):
        kw['y_scale'] = 0.3
        y = y * 0.3
    if mode.startswith('gate'):
        slope = 0.0 if mode == 'gate_relu' else 0.1
        gt = draw().relu()
        gt[0, 0, 0, :3] = 0.0  # (exact zeros: the gate's boundary case)
        y = y * torch.where(gt > 0, 1.0, slope).double()
        extra['gate'] = gt
        kw['gate_slope'] = slope
    nres = {'relu_res1': 1, 'res1_scaled': 1, 'lrelu_res2': 2}.get(mode, 0)
    for k in range(nres):
        r = draw()
        y = y + r.double()
        extra[f'res{k + 1}'] = r
    if mode == 'shuffle':
        kw['out_mode'] = ops.OUT_PIXEL_SHUFFLE2
    return y, kw, extra


def _pad_hw(t, hp, wp):
    return F.pad(t, (0, wp - t.shape[3], 0, hp - t.shape[2]))


@pytest.mark.parametrize('case', CASES_F4S, ids=_case_id)
def test_f4s_matches_fp64_on_random_shapes(gpu, case):
    """Values against float64 (the fp32 F(4x4) kernel's tolerance, and not less accurate than that kernel on the same input), the
    kernel the launch reached, and the epilogue's bound: >= max |y|; == max |y| where no block reaches past the image; else within
    rounding of the float64 maximum over the kernel's zero-padded extent (the vector path includes rows below the image)."""
    from edvr_amd import ops
    n, c1, c2, h, w, co, mode, view, flip = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    x1 = torch.randn(n, c1, h, w, generator=g)
    x2 = x2_map = None
    xin = x1
    if mode == 'x2':
        x2 = torch.randn(n, c2, h, w, generator=g)
        xin = torch.cat([x1, x2], 1)
    elif mode == 'x2_map':
        t = 2 if n % 2 == 0 else 3
        x2 = torch.randn(n, c2, h, w, generator=g)
        x2_map = (t, t, t // 2)
        xin = torch.cat([x1, x2[[(i // t) * t + t // 2 for i in range(n)]]], 1)
    ci = c1 + c2
    if flip:  # data gradient: the weight of a co -> ci layer, packed transposed and flipped (its input gradient is a ci -> co conv)
        wt = torch.randn(ci, co, 3, 3, generator=g) * 0.05
        wconv = wt.transpose(0, 1).flip(2, 3)
    else:
        wt = torch.randn(co, ci, 3, 3, generator=g) * 0.05
        wconv = wt
    b = torch.randn(co, generator=g)
    bh, bw = _geometry(h, w)
    hp, wp = -(-h // bh) * bh, -(-w // bw) * bw
    conv_pad = F.conv2d(_pad_hw(xin.double(), hp, wp), wconv.double(), b.double(), 1, 1)  # the kernel's zero-padded extent
    ypad, kw, extra = _epilogue(conv_pad, mode, co, g, h, w)
    extra = {k: v[..., :h, :w].contiguous() for k, v in extra.items()}
    ref = ypad[..., :h, :w]
    pad_max = ypad.abs().max().item()
    if mode == 'shuffle':
        ref = F.pixel_shuffle(ref, 2)

    wg = wt.to(gpu)
    wpk = ops.pack_conv_weight(wg, transpose_flip=flip)
    wf4 = ops.pack_conv_weight(wg, transpose_flip=flip, f4=True)
    wf4s = ops.pack_conv_weight(wg, transpose_flip=flip, f4s=True)
    if view == 'x1_slice':  # channel slice at a 16-byte aligned offset: images (c1 + 4) planes apart
        base = torch.randn(n, c1 + 4, h, w, generator=g)
        base[:, 4:] = x1
        x1g = base.to(gpu)[:, 4:]
    elif view == 'misaligned':  # 4 bytes off 16-byte alignment: must not reach the split kernel, must still be right
        flat = torch.zeros(x1.numel() + 1, device=gpu)
        x1g = flat[1:].view(x1.shape)
        x1g.copy_(x1.to(gpu))
    else:
        x1g = x1.to(gpu)
    for k, v in extra.items():
        if view == 'res_slice':
            big = torch.randn(n, co + 4, h, w, generator=g)
            big[:, 2:2 + co] = v
            kw[k] = big.to(gpu)[:, 2:2 + co]
        else:
            kw[k] = v.to(gpu)
    out = outbuf = None
    oshape = tuple(ref.shape)
    if view == 'out_slice':
        outbuf = torch.full((n, oshape[1] + 3) + oshape[2:], float('nan'), device=gpu)
        out = outbuf[:, 1:1 + oshape[1]]
    x2g = None if x2 is None else x2.to(gpu)
    bg = b.to(gpu)
    with _Names() as names:
        y = ops.conv2d(x1g, wpk, bg, co, 3, x2=x2g, x2_map=x2_map, wpk_f4s=wf4s, algo=ops.CONV_WINOGRAD_F4S, out=out, **kw)
    y32 = ops.conv2d(x1g, wpk, bg, co, 3, x2=x2g, x2_map=x2_map, wpk_f4=wf4, algo=ops.CONV_WINOGRAD_F4, **kw)
    torch.cuda.synchronize()
    assert tuple(y.shape) == oshape
    if outbuf is not None:
        assert torch.isnan(outbuf[:, :1]).all() and torch.isnan(outbuf[:, 1 + oshape[1]:]).all()  # nothing written beside the view
    e_split = _rel(y, ref)
    assert e_split < RTOL_F4, e_split
    if view == 'misaligned':
        assert F4S_NAME not in names.convs(), names.seen
        return
    assert names.convs() == [F4S_NAME], names.seen
    e_f32 = _rel(y32, ref)
    if ci >= 8:  # (below one 8-channel chunk the operands' rounding, 22 bits against 24, is not diluted by the accumulation: the
        #          split measured 2.1x the fp32 kernel's error at 3 channels - both 10x inside RTOL_F4)
        assert e_split < 1.5 * e_f32 + 2e-7, (e_split, e_f32)

    bound = ops.get_bound(y)
    assert bound is not None
    bv, ymax = bound.item(), y.abs().max().item()
    assert bv >= ymax, (bv, ymax)
    if h % bh == 0 and w % bw == 0:
        assert bv == ymax, (bv, ymax)
    else:
        assert bv <= (1 + 1e-4) * pad_max, (bv, pad_max, ymax)


@pytest.mark.parametrize('shape', [(2, 64, 19, 64, 216), (1, 32, 13, 36, 216), (3, 48, 16, 96, 100)])
def test_f4s_abs_sum_epilogue_matches_fp64(gpu, shape):
    """edvr_conv2d_desc.abs_sum on the split kernel: per-image sums of |y| over the first channels, against float64."""
    from edvr_amd import _lib, ops
    n, c, h, w, co = shape
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(co, c, 3, 3, generator=g) * 0.1
    b = torch.randn(co, generator=g)
    nch = 2 * co // 3
    conv = F.conv2d(x.double(), wt.double(), b.double(), 1, 1)
    want = conv[:, :nch].abs().sum((1, 2, 3))
    xg, wg = x.to(gpu), wt.to(gpu)
    wpk, wf4s = ops.pack_conv_weight(wg), ops.pack_conv_weight(wg, f4s=True)
    d = _lib.ConvDesc()
    d.c1, d.n, d.h, d.w, d.co, d.ks, d.stride, d.algo = c, n, h, w, co, 3, 1, ops.CONV_WINOGRAD_F4S
    d.x1, d.wpk_f4s, d.x_amax, d.act = xg.data_ptr(), wf4s.data_ptr(), wf4s.data_ptr(), ops.ACT_SIGMOID
    assert _lib.lib().edvr_conv2d_abs_sum_supported(ctypes.byref(d)) == 1
    with _Names() as names:
        y, sums = ops.conv2d(xg, wpk, b.to(gpu), co, 3, act=ops.ACT_SIGMOID, act_from=nch, wpk_f4s=wf4s, algo=ops.CONV_WINOGRAD_F4S,
                             abs_sum_channels=nch)
    assert names.convs() == [F4S_NAME], names.seen
    ref = torch.cat([conv[:, :nch], torch.sigmoid(conv[:, nch:])], 1)
    assert _rel(y, ref) < RTOL_F4
    assert ((sums[0].double().cpu() - want).abs() / want).max().item() < 1e-5


# ------------------------------------------------------------------------------------------------ 2. the y_amax contract
@pytest.mark.parametrize('case', C1X1_CASES)
def test_split_conv1x1_bound_is_exact(gpu, case):
    """conv1x1_s stores every element it computes: its bound is max |y| bit for bit."""
    from edvr_amd import ops
    n, c1, c2, h, w, co, actn, nres, x2map = case
    x1, x2, wt, b, ref, act, act_from, res = _c1x1_tensors(case)
    wg = wt.to(gpu)
    kw = dict(x2=None if x2 is None else x2.to(gpu), x2_map=x2map, act=act, act_from=act_from)
    for k, r in enumerate(res):
        kw[f'res{k + 1}'] = r.to(gpu)
    with _Names() as names:
        y = ops.conv2d(x1.to(gpu), ops.pack_conv_weight(wg), b.to(gpu), co, 1, wpk_f4s=ops.pack_conv_weight(wg, f4s=True), **kw)
    assert names.convs() == ['conv1x1_split_kernel'], names.seen
    assert _rel(y, ref) < 2e-6
    bound = ops.get_bound(y)
    assert bound is not None and bound.item() == y.abs().max().item()


def test_f4s_bound_ignores_the_padding_channels(gpu):
    """The vector path computes whole 64-channel blocks; the channels beyond co read the residual of channel co - 1.  They are not
    outputs and must not enter the bound: here channel 69's conv cancels its residual (y = 0 there), so a bound that counted the
    padding channels would read |residual| = 100 instead of max |y|."""
    from edvr_amd import ops
    g = torch.Generator().manual_seed(22)
    n, c, h, w, co = 1, 16, 16, 64, 70  # no block reaches past the image: the bound is max |y| bit for bit
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(co, c, 3, 3, generator=g) * 0.05
    wt[co - 1] = 0.0
    b = torch.randn(co, generator=g)
    b[co - 1] = -100.0
    r = torch.randn(n, co, h, w, generator=g)
    r[:, co - 1] = 100.0
    wg = wt.to(gpu)
    with _Names() as names:
        y = ops.conv2d(x.to(gpu), ops.pack_conv_weight(wg), b.to(gpu), co, 3, res1=r.to(gpu), wpk_f4s=ops.pack_conv_weight(wg, f4s=True),
                       algo=ops.CONV_WINOGRAD_F4S)
    assert names.convs() == [F4S_NAME], names.seen
    assert torch.equal(y[:, co - 1].cpu(), torch.zeros(n, h, w))
    assert ops.get_bound(y).item() == y.abs().max().item() < 50.0


def _raw_launch(ops, d):
    from edvr_amd import _lib
    _lib.check(_lib.lib().edvr_conv2d_f32(ctypes.byref(d), ops._stream()), 'edvr_conv2d_f32')


@pytest.mark.parametrize('kind', ['f4s_vec', 'f4s_scalar', 'conv1x1_s'])
def test_y_amax_folds_into_the_slot(gpu, kind):
    """include/edvr_amd.h: y_amax[0] = max(y_amax[0], max |y|) - the caller zeroes the slot or folds bounds.  A larger value in the
    slot survives the launch, a smaller one is replaced."""
    from edvr_amd import _lib, ops
    g = torch.Generator().manual_seed(21)
    ks, (n, c, h, w, co) = (1, (1, 320, 6, 20, 64)) if kind == 'conv1x1_s' else (3, (2, 32, 10, 64 if kind == 'f4s_vec' else 36, 70))
    x = torch.randn(n, c, h, w, generator=g).to(gpu)
    wg = (torch.randn(co, c, ks, ks, generator=g) * 0.1).to(gpu)
    b = torch.randn(co, generator=g).to(gpu)
    wpk, wf4s = ops.pack_conv_weight(wg), ops.pack_conv_weight(wg, f4s=True)
    bound = ops.amax(x)
    name = ctypes.create_string_buffer(96)
    results = []
    for prefill in [0.0, 1e6, 1e-3]:
        y = torch.empty(n, co, h, w, device=gpu)
        slot = torch.full((1,), prefill, device=gpu)
        d = _lib.ConvDesc()
        d.x1, d.c1, d.x1_img_stride, d.n, d.h, d.w = x.data_ptr(), c, c * h * w, n, h, w
        d.wpk, d.bias, d.co, d.ks, d.stride, d.act = wpk.data_ptr(), b.data_ptr(), co, ks, 1, ops.ACT_LRELU
        d.y, d.y_img_stride, d.algo = y.data_ptr(), co * h * w, ops.CONV_WINOGRAD_F4S if ks == 3 else ops.CONV_AUTO
        d.wpk_f4s, d.x_amax, d.y_amax = wf4s.data_ptr(), bound.data_ptr(), slot.data_ptr()
        _lib.lib().edvr_conv2d_kernel_name(ctypes.byref(d), name, 96)
        assert name.value.decode() == ('conv1x1_split_kernel' if ks == 1 else F4S_NAME), name.value
        _raw_launch(ops, d)
        torch.cuda.synchronize()
        results.append((prefill, slot.item(), y.abs().max().item()))
    ymax = results[0][2]
    assert all(r[2] == ymax for r in results)  # the slot does not change the output
    if kind == 'f4s_vec':
        assert results[0][1] >= ymax  # (rows below the image count on the vector path)
    else:
        assert results[0][1] == ymax
    assert results[1][1] == 1e6                 # a larger prefilled bound survives
    assert results[2][1] == results[0][1]       # a smaller one is replaced


# ------------------------------------------------------------------------------------------------ 3. non-finite sentinels
def _nf_check(ops, dev, y, ref, bound):
    """The non-finite value does not disappear, the slot sees it, the guard raises (once)."""
    torch.cuda.synchronize()
    bad_ref = ~torch.isfinite(ref)
    bad_y = ~torch.isfinite(y.cpu())
    assert bad_ref.any()
    assert bad_y[bad_ref].all(), 'a non-finite value of the reference is finite in the output'
    if bad_y.any():
        assert not torch.isfinite(bound).all().item(), f'the output holds non-finite values, the bound slot holds {bound.item()}'
    _assert_guard_trips(ops, dev)


# geometry of each column-pass variant: 10 rows (the last tile row has 2), one 8 x 64 block column (w = 64: vector rows), or a block
# column only partly inside the image (w = 36: per-element stores); `shuffle`: the vector path with the PixelShuffle store
_NF_PATHS = {'vec': (10, 64, 0), 'scalar': (10, 36, 0), 'shuffle': (10, 64, 1)}


def _nf_setup(gpu, path, nres=0, c2=0, x2_map=False, gate=False, seed=0):
    from edvr_amd import ops
    h, w, shuffle = _NF_PATHS[path]
    g = torch.Generator().manual_seed(100 + seed)
    n, c1, co = (2, 16, 64)
    x1 = torch.randn(n, c1, h, w, generator=g)
    x2 = torch.randn(n if not x2_map else 1, c2, h, w, generator=g) if c2 else None
    wt = torch.randn(co, c1 + c2, 3, 3, generator=g) * 0.1
    b = torch.randn(co, generator=g)
    res = [torch.randn(n, co, h, w, generator=g) for _ in range(nres)]
    gt = torch.randn(n, co, h, w, generator=g).relu() if gate else None
    kw = dict(act=ops.ACT_LRELU if not gate else ops.ACT_NONE, out_mode=ops.OUT_PIXEL_SHUFFLE2 if shuffle else ops.OUT_NCHW)
    if x2_map:
        kw['x2_map'] = (2, 0, 0)  # both images read image 0 of x2
    return dict(x1=x1, x2=x2, wt=wt, b=b, res=res, gate=gt, kw=kw, co=co)


def _nf_run(gpu, s):
    """The split F(4x4) launch of setup `s` and its float64 direct-conv reference."""
    from edvr_amd import ops
    x1, x2, wt, b, res, gt, kw, co = s['x1'], s['x2'], s['wt'], s['b'], s['res'], s['gate'], dict(s['kw']), s['co']
    if x2 is None:
        xin = x1
    elif 'x2_map' in kw:
        xin = torch.cat([x1, x2[[0] * x1.shape[0]]], 1)
    else:
        xin = torch.cat([x1, x2], 1)
    ref = F.conv2d(xin.double(), wt.double(), b.double(), 1, 1)
    if kw['act'] == ops.ACT_LRELU:
        ref = F.leaky_relu(ref, 0.1)
    if gt is not None:
        ref = ref * torch.where(gt > 0, 1.0, s['gate_slope']).double()
        kw.update(gate=gt.to(gpu), gate_slope=s['gate_slope'])
    for k, r in enumerate(res):
        ref = ref + r.double()
        kw[f'res{k + 1}'] = r.to(gpu)
    if kw['out_mode'] == ops.OUT_PIXEL_SHUFFLE2:
        ref = F.pixel_shuffle(ref, 2)
    wg = wt.to(gpu)
    with _Names() as names:
        y = ops.conv2d(x1.to(gpu), ops.pack_conv_weight(wg), b.to(gpu), co, 3, x2=None if x2 is None else x2.to(gpu),
                       wpk_f4s=ops.pack_conv_weight(wg, f4s=True), algo=ops.CONV_WINOGRAD_F4S, **kw)
    assert names.convs() == [F4S_NAME], names.seen
    bound = ops.get_bound(y)
    assert bound is not None
    return y, ref, bound


@pytest.mark.parametrize('val', NONFINITE, ids=['nan', 'inf', '-inf'])
@pytest.mark.parametrize('src', ['res1', 'res2'])
@pytest.mark.parametrize('path', ['vec', 'scalar'])
def test_f4s_nonfinite_residual_at_every_tile_position(guard, gpu, path, src, val):
    """A residual enters after the products: the epilogue's bound must record it wherever it sits in the 4 x 4 tile (the vector path
    takes max |y| over the whole tile, the scalar path over every stored element).  (The PixelShuffle store takes no residual.)"""
    ops = guard
    s = _nf_setup(gpu, path, nres=2 if src == 'res2' else 1)
    r = s['res'][-1]
    for ty, tx in [(4, 8), (8, 16)]:  # an interior tile, and a tile of the last (2-row) tile row
        for i in range(4):
            for j in range(4):
                if ty + i >= r.shape[2]:
                    continue
                keep = r[1, 5, ty + i, tx + j].item()
                r[1, 5, ty + i, tx + j] = val
                y, ref, bound = _nf_run(gpu, s)
                _nf_check(ops, gpu, y, ref, bound)
                r[1, 5, ty + i, tx + j] = keep


# image positions of an input element: corners, edges, interior, the last (ragged) rows
def _img_positions(h, w):
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0), (h // 2, w - 1), (5, 21), (h - 2, w // 2 + 3)]


@pytest.mark.parametrize('val', NONFINITE, ids=['nan', 'inf', '-inf'])
@pytest.mark.parametrize('src', ['x1', 'x2', 'x2_map'])
@pytest.mark.parametrize('path', ['vec', 'scalar', 'shuffle'])
def test_f4s_nonfinite_input(guard, gpu, path, src, val):
    ops = guard
    s = _nf_setup(gpu, path, c2=16 if src != 'x1' else 0, x2_map=src == 'x2_map', seed=1)
    t = s['x1'] if src == 'x1' else s['x2']
    h, w = t.shape[2:]
    for (py, px) in _img_positions(h, w):
        keep = t[0, 3, py, px].item()
        t[0, 3, py, px] = val
        y, ref, bound = _nf_run(gpu, s)
        _nf_check(ops, gpu, y, ref, bound)
        t[0, 3, py, px] = keep


@pytest.mark.parametrize('val', NONFINITE, ids=['nan', 'inf', '-inf'])
@pytest.mark.parametrize('path', ['vec', 'scalar', 'shuffle'])
def test_f4s_nonfinite_weight_and_bias(guard, gpu, path, val):
    ops = guard
    s = _nf_setup(gpu, path, seed=2)
    for where in [(0, 0, 0, 0), (37, 9, 1, 1), (63, 15, 2, 1)]:
        s['wt'] = s['wt'].clone()
        keep = s['wt'][where].item()
        s['wt'][where] = val
        y, ref, bound = _nf_run(gpu, s)
        _nf_check(ops, gpu, y, ref, bound)
        s['wt'][where] = keep
    for co in [0, 42]:
        keep = s['b'][co].item()
        s['b'][co] = val
        y, ref, bound = _nf_run(gpu, s)
        _nf_check(ops, gpu, y, ref, bound)
        s['b'][co] = keep


@pytest.mark.parametrize('slope', [0.0, 0.1])
@pytest.mark.parametrize('path', ['vec', 'scalar'])
def test_f4s_nan_gate_is_not_a_source(guard, gpu, path, slope):
    """gate > 0 ? 1 : slope takes a NaN gate as non-positive (torch.where(g > 0, 1, slope) does the same): a finite output, a
    finite bound, a quiet guard."""
    ops = guard
    s = _nf_setup(gpu, path, gate=True, seed=3)
    s['gate_slope'] = slope
    for (py, px) in [(0, 0), (5, 6), (9, 33), (4, 8)]:
        s['gate'][1, 7, py, px] = float('nan')
    y, ref, bound = _nf_run(gpu, s)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and torch.isfinite(y).all()
    assert _rel(y, ref) < RTOL_F4
    assert torch.isfinite(bound).all() and bound.item() >= y.abs().max().item()
    _assert_guard_quiet(ops, gpu)


def _c1x1_nf_setup(seed):
    g = torch.Generator().manual_seed(200 + seed)
    n, c1, c2, h, w, co = 2, 320, 64, 5, 7, 70
    return dict(x1=torch.randn(n, c1, h, w, generator=g), x2=torch.randn(n, c2, h, w, generator=g),
                wt=torch.randn(co, c1 + c2, 1, 1, generator=g) * 0.05, b=torch.randn(co, generator=g),
                res=[torch.randn(n, co, h, w, generator=g) for _ in range(2)], co=co)


def _c1x1_nf_run(gpu, s):
    from edvr_amd import ops
    xin = torch.cat([s['x1'], s['x2']], 1)
    ref = F.leaky_relu(F.conv2d(xin.double(), s['wt'].double(), s['b'].double()), 0.1) + s['res'][0].double() + s['res'][1].double()
    wg = s['wt'].to(gpu)
    with _Names() as names:
        y = ops.conv2d(s['x1'].to(gpu), ops.pack_conv_weight(wg), s['b'].to(gpu), s['co'], 1, x2=s['x2'].to(gpu), act=ops.ACT_LRELU,
                       res1=s['res'][0].to(gpu), res2=s['res'][1].to(gpu), wpk_f4s=ops.pack_conv_weight(wg, f4s=True))
    assert names.convs() == ['conv1x1_split_kernel'], names.seen
    bound = ops.get_bound(y)
    assert bound is not None
    return y, ref, bound


@pytest.mark.parametrize('val', NONFINITE, ids=['nan', 'inf', '-inf'])
@pytest.mark.parametrize('src', ['x1', 'x2', 'weight', 'res1', 'res2'])
def test_conv1x1_s_nonfinite(guard, gpu, src, val):
    ops = guard
    s = _c1x1_nf_setup(0)
    if src in ('x1', 'x2'):
        t, spots = s[src], [(0, 0, 0, 0), (1, 17, 2, 3), (1, 63, 4, 6)]
    elif src == 'weight':
        t, spots = s['wt'], [(0, 0, 0, 0), (33, 200, 0, 0), (69, 383, 0, 0)]
    else:
        t, spots = s['res'][int(src[-1]) - 1], [(0, 0, 0, 0), (1, 40, 2, 3), (1, 69, 4, 6), (0, 64, 3, 1)]
    for where in spots:
        keep = t[where].item()
        t[where] = val
        y, ref, bound = _c1x1_nf_run(gpu, s)
        _nf_check(ops, gpu, y, ref, bound)
        t[where] = keep


def _amax_views(gpu):
    """(name, view, positions) covering the reduction kernel's position classes: the unrolled body and the remainder of the 16-byte
    loop, the tail of an image whose length is not a multiple of 4, misaligned images (element loop), channel-sliced batches.  The
    elements of the base tensors OUTSIDE the views are NaN: the kernel may not read them."""
    nan = float('nan')
    big = torch.randn(2, 64, 45, 80, device=gpu)  # one long array: the four-deep loop, its remainder, no tail
    odd = torch.randn(1, 3, 5, 7, device=gpu)     # 105 elements: 26 quads + a 1-element tail
    tiny = torch.randn(1, 1, 1, 3, device=gpu)    # tail only
    base = torch.randn(4, 6, 10, 12, device=gpu)
    base[:, 0], base[:, 4:] = nan, nan
    sl = base[:, 1:4]                                   # channel slice: images 6 planes apart, 16-byte aligned
    base = torch.randn(2, 8, 5, 7, device=gpu)
    base[:, :4], base[:, 7:] = nan, nan
    sl_tail = base[:, 4:7]                              # aligned channel slice of 105 elements per image: a tail per image
    base = torch.randn(3, 5, 7, 9, device=gpu)
    base[:, 0] = nan
    mis = base[:, 1:]                                   # channel slice 63 elements in: misaligned images
    base = torch.randn(2 * 3 * 8 * 8 + 2, device=gpu)
    base[0], base[-1] = nan, nan
    flat = base[1:-1].view(2, 3, 8, 8)                  # one long misaligned array
    return [
        ('big', big, [(0, 0, 0, 0), (0, 10, 20, 33), (1, 63, 44, 76), (1, 63, 44, 79)]),
        ('odd', odd, [(0, 0, 0, 0), (0, 1, 2, 3), (0, 2, 4, 6)]),
        ('tiny', tiny, [(0, 0, 0, 2)]),
        ('slice', sl, [(0, 0, 0, 0), (3, 2, 9, 11), (2, 1, 5, 6)]),
        ('slice_tail', sl_tail, [(0, 0, 0, 0), (1, 2, 4, 6), (1, 1, 4, 6)]),
        ('misaligned_slice', mis, [(0, 0, 0, 0), (2, 3, 6, 8)]),
        ('misaligned_flat', flat, [(0, 0, 0, 0), (1, 2, 7, 7)]),
    ]


@pytest.mark.parametrize('val', NONFINITE, ids=['nan', 'inf', '-inf'])
def test_amax_kernel_keeps_nonfinite_values(guard, gpu, val):
    ops = guard
    for name, v, spots in _amax_views(gpu):
        assert ops.amax(v).item() == v.abs().max().item(), name  # (finite: nothing outside the view is read)
        for where in spots:
            keep = v[where].item()
            v[where] = val
            got = ops.amax(v).item()
            if val != val:
                assert got != got, (name, where, got)
            else:
                assert got == float('inf'), (name, where, got)
            _assert_guard_trips(ops, gpu)
            v[where] = keep
        assert ops.amax(v).item() == v.abs().max().item(), name
    _assert_guard_quiet(ops, gpu)
