"""The split-operand DIRECT convolution (csrc/conv2d_s.hip, conv2d's `wpk_ds`): 3x3 / stride 2, conv_first and the small 1x1 convs
against F.conv2d in float64, with the fp32 direct kernel's own error on the same case as the yardstick of the bound."""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACTS = {'none': 0, 'relu': 1, 'lrelu': 2, 'sigmoid': 3}

# (n, c1, c2, h, w, co, ks, stride, act, act_from, residuals, x2_map)
S2_CASES = [
    (2, 128, 0, 18, 36, 128, 3, 2, 'lrelu', 0, 0, None),   # ragged row and column tiles
    (1, 128, 0, 17, 67, 128, 3, 2, 'lrelu', 0, 0, None),   # odd h and w: the de-interleaved halo of an odd width, bottom / right padding
    (3, 64, 0, 16, 64, 64, 3, 2, 'none', 0, 1, None),      # the MT = 2 / NS = 2 instantiation (EDVR-M)
    (1, 128, 0, 20, 40, 200, 3, 2, 'relu', 0, 2, None),    # a full block plus tail tiles
]
FIRST_CASES = [
    (2, 3, 0, 12, 40, 128, 3, 1, 'lrelu', 0, 0, None),     # three real channels in one quad
    (1, 3, 0, 9, 21, 64, 3, 1, 'lrelu', 0, 0, None),       # ... ragged
]
C1_CASES = [
    (1, 128, 0, 17, 23, 128, 1, 1, 'none', 0, 0, None),    # 391 pixels
    (2, 128, 128, 9, 20, 128, 1, 1, 'lrelu', 0, 0, None),  # two inputs
    (4, 128, 128, 8, 16, 200, 1, 1, 'lrelu', 0, 2, (2, 1, 0)),  # x2 through the image map, residuals
    (1, 136, 0, 5, 7, 33, 1, 1, 'sigmoid', 16, 0, None),   # act_from with a ragged co
]


def _rel(y, ref):
    return (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


@functools.lru_cache(maxsize=None)
def _tensors(case):
    """Inputs and the float64 reference of a case, made once on the host and shared (nobody writes them)."""
    n, c1, c2, h, w, co, ks, stride, actn, act_from, nres, x2map = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    x1 = torch.randn(n, c1, h, w, generator=g)
    n2 = n if x2map is None else (n // x2map[0]) * max(x2map[1], 1)
    x2 = torch.randn(n2, c2, h, w, generator=g) if c2 else None
    wt = torch.randn(co, c1 + c2, ks, ks, generator=g) * (0.1 if ks == 3 else 0.05)
    b = torch.randn(co, generator=g)
    if x2 is None:
        xin = x1
    elif x2map is None:
        xin = torch.cat([x1, x2], 1)
    else:
        xin = torch.cat([x1, x2[[(i // x2map[0]) * x2map[1] + x2map[2] for i in range(n)]]], 1)
    ref = F.conv2d(xin.double(), wt.double(), b.double(), stride, ks // 2)
    if actn == 'relu':
        ref = F.relu(ref)
    elif actn == 'lrelu':
        ref = F.leaky_relu(ref, 0.1)
    elif actn == 'sigmoid':
        ref = torch.cat([ref[:, :act_from], torch.sigmoid(ref[:, act_from:])], 1)
    res = tuple(torch.randn(ref.shape, generator=g) for _ in range(nres))
    for r in res:
        ref = ref + r.double()
    return x1, x2, wt, b, ref, res


def _hooked(ops, fn):
    seen = []
    ops.LAUNCH_HOOK = lambda name, flops, launch, *a: (seen.append(name), launch())
    try:
        out = fn()
    finally:
        ops.LAUNCH_HOOK = None
    return out, [k for k in seen if k.startswith('conv')]


def _run_case(gpu, case):
    from edvr_amd import ops
    n, c1, c2, h, w, co, ks, stride, actn, act_from, nres, x2map = case
    x1, x2, wt, b, ref, res = _tensors(case)
    wg = wt.to(gpu)
    wpk, wds = ops.pack_conv_weight(wg), ops.pack_conv_weight(wg, ds=True)
    rg = [r.to(gpu) for r in res]
    kw = dict(x2=None if x2 is None else x2.to(gpu), x2_map=x2map, stride=stride, act=ACTS[actn], act_from=act_from,
              res1=rg[0] if nres > 0 else None, res2=rg[1] if nres > 1 else None)
    x1g, bg = x1.to(gpu), b.to(gpu)
    ys, names_s = _hooked(ops, lambda: ops.conv2d(x1g, wpk, bg, co, ks, wpk_ds=wds, **kw))
    y32, names_32 = _hooked(ops, lambda: ops.conv2d(x1g, wpk, bg, co, ks, **kw))
    assert len(names_s) == 1 and names_s[0].startswith('conv2d_split_kernel<%d, %d, ' % (ks, stride)), names_s
    assert len(names_32) == 1 and names_32[0].startswith('conv2d_mfma_kernel<%d, %d, ' % (ks, stride)), names_32
    assert names_s[0].split('<')[1] == names_32[0].split('<')[1]  # the same tile choice
    assert ys.shape == ref.shape
    es, e32 = _rel(ys, ref), _rel(y32, ref)
    print(f'{case}: split {es:.3e}  fp32 {e32:.3e}')
    assert es < 1.5 * e32 + 2e-7, (es, e32)
    if e32 <= 1.3e-6:
        assert es < 2e-6, (es, e32)
    else:
        print(f'fp32 direct kernel above 1.3e-6 on {case}: relative bound only (split {es:.3e}, fp32 {e32:.3e})')
    bound = ops.get_bound(ys)  # the epilogue's max |y|
    top = ys.abs().max().item()
    assert bound is not None and abs(bound.item() - top) <= 1e-6 * top, (bound, top)
    assert ops.get_bound(y32) is None


@pytest.mark.parametrize('case', S2_CASES)
def test_split_stride2_matches_fp64(gpu, case):
    _run_case(gpu, case)


@pytest.mark.parametrize('case', FIRST_CASES)
def test_split_conv_first_matches_fp64(gpu, case):
    _run_case(gpu, case)


@pytest.mark.parametrize('case', C1_CASES)
def test_split_small_1x1_matches_fp64(gpu, case):
    _run_case(gpu, case)


@pytest.fixture
def guard(gpu, monkeypatch):
    from edvr_amd import ops

    def drain():
        ops._arena(gpu).take_unexamined()
        ops._GUARD_PENDING.clear()
    monkeypatch.setattr(ops, 'SPLIT_GUARD', 'raise')
    drain()
    yield ops
    drain()


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('ks,stride', [(3, 2), (1, 1)])
def test_split_direct_non_finite_input_trips_the_guard(gpu, guard, bad, ks, stride):
    ops = guard
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 128, 10, 36, generator=g)
    wg = (torch.randn(128, 128, ks, ks, generator=g) * 0.05).to(gpu)
    wpk, wds = ops.pack_conv_weight(wg), ops.pack_conv_weight(wg, ds=True)
    y = ops.conv2d(x.to(gpu), wpk, None, 128, ks, stride=stride, wpk_ds=wds)
    ops.split_guard_submit(gpu)
    ops.split_guard_check(wait=True)  # finite: quiet
    assert torch.isfinite(ops.get_bound(y)).all()
    x[0, 7, 4, 9] = bad
    xg = x.to(gpu)
    y = ops.conv2d(xg, wpk, None, 128, ks, stride=stride, wpk_ds=wds, x_amax=torch.full((1,), 8.0, device=gpu))
    assert not torch.isfinite(ops.get_bound(y)).all()
    ops.split_guard_submit(gpu)
    with pytest.raises(ops.SplitOperandOverflow):
        ops.split_guard_check(wait=True)
    ops.split_guard_check(wait=True)  # once: nothing else pending


def test_bounds_reaching_the_direct_split_kernel_in_a_network_are_bounds(gpu):
    """A whole no-grad forward under ops.BOUND_CHECK: every bound handed to the direct split kernel (conv_first's from a reduction over
    the frames, the pyramid's and TSA's from producers' epilogues, pooling, interpolation) is compared with the data inside conv2d -
    never below max |x| (it raises) - and is recorded apart from the kernels that training has too; none is 2^12 above the data."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from util_edvr import build
    from edvr_amd import ops
    net, x, _ = build('M_T5')
    net = net.to(gpu).eval()
    ops.BOUND_CHECK, ops.BOUND_CHECK_LOG[:], ops.BOUND_CHECK_LOG_DIRECT[:] = True, [], []
    try:
        with torch.no_grad():
            y, names = _hooked(ops, lambda: net(x.to(gpu)))
    finally:
        ops.BOUND_CHECK = False
    n_direct = sum(1 for k in names if k.startswith('conv2d_split_kernel'))
    assert torch.isfinite(y).all()
    assert n_direct >= 3 and len(ops.BOUND_CHECK_LOG_DIRECT) == n_direct, (n_direct, len(ops.BOUND_CHECK_LOG_DIRECT), names)
    assert len(ops.BOUND_CHECK_LOG) >= 10
    assert all(1.0 <= r < 4096.0 for _, r in ops.BOUND_CHECK_LOG_DIRECT), ops.BOUND_CHECK_LOG_DIRECT


@pytest.mark.parametrize('scale', [1e-25, 1e-4, 1.0, 1e6, 1e25])
@pytest.mark.parametrize('ks,stride', [(3, 2), (1, 1)])
def test_split_direct_is_scale_invariant(gpu, scale, ks, stride):
    """Inputs of 1e-25 .. 1e25, one outlier 300x the rest and a bound 64x loose: finite, and the tolerance of the plain cases."""
    from edvr_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 128, 12, 36, generator=g) * scale
    x[0, 3, 2, 2] *= 300.0  # an outlier sets the bound; everything else sits 2^-8 below it
    wt = torch.randn(128, 128, ks, ks, generator=g) * 0.05
    ref = F.conv2d(x.double(), wt.double(), None, stride, ks // 2)
    xg, wg = x.to(gpu), wt.to(gpu)
    wpk, wds = ops.pack_conv_weight(wg), ops.pack_conv_weight(wg, ds=True)
    (ys, names) = _hooked(ops, lambda: ops.conv2d(xg, wpk, None, 128, ks, stride=stride, wpk_ds=wds, x_amax=ops.amax(xg) * 64.0))
    assert names[0].startswith('conv2d_split_kernel'), names
    y32 = ops.conv2d(xg, wpk, None, 128, ks, stride=stride)
    es, e32 = _rel(ys, ref), _rel(y32, ref)
    print(f'scale {scale:g} ks {ks} stride {stride}: split {es:.3e}  fp32 {e32:.3e}')
    assert torch.isfinite(ys).all()
    assert es < 1.5 * e32 + 2e-7, (es, e32)
    assert es < 2e-6 or e32 > 1.3e-6, (es, e32)


def test_split_direct_falls_back_where_it_does_not_apply(gpu):
    """gate, y_scale, PixelShuffle output, EDVR_CONV_DIRECT, c1 % 4 != 0 with a second input, no wpk_ds: the fp32 direct kernel, and
    bit for bit what the same call gives without the packing."""
    from edvr_amd import ops
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 128, 12, 36, generator=g).to(gpu)
    wg = (torch.randn(128, 128, 3, 3, generator=g) * 0.05).to(gpu)
    gate = torch.randn(2, 128, 6, 18, generator=g).to(gpu)
    xa, xb = torch.randn(1, 130, 8, 16, generator=g).to(gpu), torch.randn(1, 126, 8, 16, generator=g).to(gpu)
    w1 = (torch.randn(64, 256, 1, 1, generator=g) * 0.05).to(gpu)
    calls = [
        (x, wg, 3, dict(stride=2, gate=gate, gate_slope=0.1)),
        (x, wg, 3, dict(stride=2, y_scale=0.5)),
        (x, wg, 3, dict(stride=2, out_mode=ops.OUT_PIXEL_SHUFFLE2)),
        (x, wg, 3, dict(stride=2, algo=ops.CONV_DIRECT)),
        (xa, w1, 1, dict(x2=xb)),
    ]
    for xin, wt, ks, kw in calls:
        wpk, wds = ops.pack_conv_weight(wt), ops.pack_conv_weight(wt, ds=True)
        y, names = _hooked(ops, lambda: ops.conv2d(xin, wpk, None, wt.shape[0], ks, wpk_ds=wds, **kw))
        y0, names0 = _hooked(ops, lambda: ops.conv2d(xin, wpk, None, wt.shape[0], ks, **kw))
        assert names == names0 and names[0].startswith('conv2d_mfma_kernel'), (kw.keys(), names, names0)
        assert torch.equal(y, y0), kw.keys()
        assert ops.get_bound(y) is None
    # no wpk_ds: what it always was, also next to a packing for another kernel in wpk_f4s
    wpk = ops.pack_conv_weight(wg)
    y, names = _hooked(ops, lambda: ops.conv2d(x, wpk, None, 128, 3, stride=2, wpk_f4s=ops.pack_conv_weight(wg, f4s=True)))
    assert names[0].startswith('conv2d_mfma_kernel'), names
    ref = F.conv2d(x.double().cpu(), wg.double().cpu(), None, 2, 1)
    assert _rel(y, ref) < 2e-6


@pytest.mark.parametrize('co,ci,ks', [(40, 11, 3), (33, 136, 1)])
def test_split_direct_packing(gpu, co, ci, ks):
    """The device buffer unpacked on the host: (hi + lo) / s_W is the weight to 2^-21 of max |w|, the padding is zero."""
    from edvr_amd import ops
    g = torch.Generator().manual_seed(7)
    wt = torch.randn(co, ci, ks, ks, generator=g) * 0.3
    buf = ops.pack_conv_weight(wt.to(gpu), ds=True).cpu()
    s_w, inv = buf[:2].view(torch.float32).tolist()
    top = wt.abs().max().item()
    assert s_w * inv == 1.0 and 2.0 ** 14 <= top * s_w < 2.0 ** 15
    assert not buf[2:16].any()
    cop, quads = (co + 31) // 32 * 32, (ci + (31 if ks == 1 else 7)) // (32 if ks == 1 else 8) * (8 if ks == 1 else 2)
    assert buf.numel() == 16 + quads * ks * ks * cop * 4
    body = buf[16:].view(quads, ks * ks, cop, 4)
    halves = body.contiguous().view(torch.float16).view(quads, ks * ks, cop, 4, 2).double()  # (hi, lo): little-endian halves of a dword
    val = (halves[..., 0] + halves[..., 1]) / s_w                                            # [quad][tap][co'][channel of the quad]
    full = val.permute(2, 0, 3, 1).reshape(cop, quads * 4, ks, ks)                           # (co', channel, kh, kw)
    assert (full[:co, :ci] - wt.double()).abs().max().item() <= 2.0 ** -21 * top
    assert not body.view(quads, ks * ks, cop, 4).permute(2, 0, 3, 1).reshape(cop, quads * 4, ks * ks)[co:].any()
    assert not body.permute(2, 0, 3, 1).reshape(cop, quads * 4, ks * ks)[:, ci:].any()
