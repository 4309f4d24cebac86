"""The pre-activation addend of the F(4x4) Winograd kernels (edvr_conv2d_desc.pre) and its user, functional.conv_shared_x2.

y = act(conv(x) + bias + pre[map(i)]): the half of a two-input conv whose second input is shared by several images (PCDAlignment's
reference features: one per clip of t frames) is convolved once per shared image and enters the other half's epilogue before bias
and activation.  CPU: the algebra in NumPy float64.  -m gpu, against float64 references:
  - layer level, split (f4s) and fp32 (f4) kernels, both block shapes, channel padding, ragged rows, the scalar edge path, every
    activation, t = 5 and 7 maps in the (div, mul, add) form EDVR.forward produces - at the F(4x4) tests' tolerance (3e-5 of max |ref|);
  - identity: the two-input launch against conv_a(nbr, pre=conv_b(ref)), both against float64;
  - pre = None is the same launch as a call without the argument, bit for bit;
  - one NaN / +inf / -inf in `pre` reaches y, the y_amax slot and the overflow guard; the bound is >= max |y| and exact where no
    block passes the image edge;
  - the host checks;
  - module level: `aligned` of EDVR-L (t = 5 and 7) with the path on and off, eager and replayed from a graph, against the float64
    oracle at the whole-network tolerance (2e-4 of max |ref|); state_dict keys / load_state_dict."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_f4 import RTOL_F4, _rel
from test_gpu_split_bounds import F4S_NAME, NONFINITE, _assert_guard_quiet, _geometry, _Names, _nf_check, guard  # noqa: F401

F4_NAME = 'conv3x3_winograd_f4_kernel'
INTERMEDIATE_RTOL = 2e-4  # whole-network tolerance (tests/test_gpu_edvr.py)


# ------------------------------------------------------------------------------------------------ CPU: the algebra
def _conv3x3_np(x, w):
    """Direct 3x3 / pad-1 correlation in float64: x (n, c, h, w), w (co, c, 3, 3)."""
    n, c, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((n, w.shape[0], h, wd))
    for i in range(3):
        for j in range(3):
            y += np.einsum('nchw,oc->nohw', xp[:, :, i:i + h, j:j + wd], w[:, :, i, j])
    return y


@pytest.mark.parametrize('t,c1,c2', [(5, 8, 8), (7, 6, 10)])
def test_conv_of_a_concat_is_the_sum_of_its_halves(t, c1, c2):
    """conv(cat[nbr, ref[map]], W) == conv(nbr, W[:, :c1]) + conv(ref, W[:, c1:])[map] in float64, with the map EDVR.forward builds."""
    rng = np.random.default_rng(t)
    b, co, h, w = 2, 5, 6, 9
    nbr, ref = rng.standard_normal((b * t, c1, h, w)), rng.standard_normal((b * t, c2, h, w))
    wt, bias = rng.standard_normal((co, c1 + c2, 3, 3)), rng.standard_normal(co)
    div, mul, add = t, t, t // 2
    idx = [(i // div) * mul + add for i in range(b * t)]
    whole = _conv3x3_np(np.concatenate([nbr, ref[idx]], 1), wt) + bias[None, :, None, None]
    p = _conv3x3_np(ref[add::mul][:b], wt[:, c1:])  # once per clip
    halves = _conv3x3_np(nbr, wt[:, :c1]) + bias[None, :, None, None] + p[[i // div for i in range(b * t)]]
    assert np.abs(whole - halves).max() <= 1e-12 * np.abs(whole).max()


# ------------------------------------------------------------------------------------------------ layer level
def _act64(y, act, act_from=0):
    from edvr_amd import ops
    if act == ops.ACT_RELU:
        return F.relu(y)
    if act == ops.ACT_LRELU:
        return F.leaky_relu(y, 0.1)
    if act == ops.ACT_SIGMOID:
        return torch.cat([y[:, :act_from], torch.sigmoid(y[:, act_from:])], 1)
    return y


# n, n_pre, map, c, h, w, co, act: both block shapes (16 x 32 where it pads less, else 8 x 64), co % 64 != 0, h % block height != 0,
# w past the last full block (the scalar edge path), every activation, the (t, t, ctr)-style maps of t = 5 and 7 reduced to the
# shared images ((t, 1, 0)) and in full ((t, t, ctr) into a tensor of n images), the identity map
PRE_CASES = [
    (10, 2, (5, 1, 0), 32, 16, 64, 64, 'lrelu'),     # exact 8 x 64 blocks, t = 5
    (14, 2, (7, 1, 0), 16, 10, 64, 70, 'lrelu'),     # t = 7, channel padding, 2 rows in the last tile row
    (10, 10, (5, 5, 2), 16, 13, 36, 100, 'relu'),    # the map EDVR.forward produces, into n images; 16 x 32 blocks; scalar edge path
    (7, 7, (7, 7, 3), 8, 19, 100, 48, 'none'),       # vector and scalar blocks in one row of blocks, ragged rows
    (5, 1, (5, 0, 0), 36, 16, 96, 128, 'sigmoid_from'),
    (3, 3, None, 64, 32, 32, 216, 'sigmoid_from'),   # identity map, 16 x 32 blocks exact
    (4, 2, (2, 1, 0), 20, 9, 160, 64, 'none'),
]


def _pre_tensors(case, seed=0):
    from edvr_amd import ops
    n, n_pre, pmap, c, h, w, co, actn = case
    g = torch.Generator().manual_seed(1000 + seed + sum(case[:2]) + c + h + w + co)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(co, c, 3, 3, generator=g) * 0.1
    b = torch.randn(co, generator=g)
    p = torch.randn(n_pre, co, h, w, generator=g)
    act, act_from = {'none': (ops.ACT_NONE, 0), 'relu': (ops.ACT_RELU, 0), 'lrelu': (ops.ACT_LRELU, 0),
                     'sigmoid_from': (ops.ACT_SIGMOID, 2 * co // 3)}[actn]
    idx = list(range(n)) if pmap is None else [(i // pmap[0]) * pmap[1] + pmap[2] for i in range(n)]
    ref = _act64(F.conv2d(x.double(), wt.double(), b.double(), 1, 1) + p.double()[idx], act, act_from)
    return x, wt, b, p, act, act_from, ref


def test_pre_cases_cover_every_path():
    seen = set()
    for n, n_pre, pmap, c, h, w, co, actn in PRE_CASES:
        bh, bw = _geometry(h, w)
        seen.update({('block', bh), actn, 'map' if pmap else 'identity'})
        if w % bw:
            seen.add('scalar')
        if w >= bw:
            seen.add('vec')
        if h % bh:
            seen.add('ragged_rows')
        if co % 64:
            seen.add('co_padding')
        if pmap and pmap[0] in (5, 7):
            seen.add(('t', pmap[0]))
    assert {('block', 8), ('block', 16), 'none', 'relu', 'lrelu', 'sigmoid_from', 'map', 'identity', 'scalar', 'vec', 'ragged_rows',
            'co_padding', ('t', 5), ('t', 7)} <= seen


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', ['f4s', 'f4'])
@pytest.mark.parametrize('case', PRE_CASES)
def test_pre_matches_fp64(gpu, case, kernel):
    from edvr_amd import ops
    n, n_pre, pmap, c, h, w, co, actn = case
    x, wt, b, p, act, act_from, ref = _pre_tensors(case)
    wg = wt.to(gpu)
    kw = dict(wpk_f4s=ops.pack_conv_weight(wg, f4s=True), algo=ops.CONV_WINOGRAD_F4S) if kernel == 'f4s' else \
        dict(wpk_f4=ops.pack_conv_weight(wg, f4=True), algo=ops.CONV_WINOGRAD_F4)
    with _Names() as names:
        y = ops.conv2d(x.to(gpu), ops.pack_conv_weight(wg), b.to(gpu), co, 3, act=act, act_from=act_from, pre=p.to(gpu), pre_map=pmap, **kw)
    torch.cuda.synchronize()
    assert names.convs() == [F4S_NAME if kernel == 'f4s' else F4_NAME], names.seen
    e = _rel(y, ref)
    print(f'pre {kernel} {case}: rel err {e:.3e}')
    assert e < RTOL_F4, e
    if kernel == 'f4s':  # the bound rules of tests/test_gpu_split_bounds.py
        bv, ymax = ops.get_bound(y).item(), y.abs().max().item()
        bh, bw = _geometry(h, w)
        assert bv >= ymax, (bv, ymax)
        if h % bh == 0 and w % bw == 0:
            assert bv == ymax, (bv, ymax)


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', ['f4s', 'f4'])
@pytest.mark.parametrize('t', [5, 7])
def test_split_halves_match_the_two_input_conv(gpu, t, kernel):
    """conv(cat[nbr, ref[map]]) by the two-input launch against conv_a(nbr, pre=conv_b(ref)), both against float64, five seeds.  The
    halves add two rounded fp32 sums where the single launch accumulates one: the new path's worst error may exceed the old path's
    worst by no more than the spread (max - min) the old path itself shows over the seeds.
    Measured on MI355X (worst of five seeds, old / new): f4s t = 5 6.95e-6 / 4.46e-6, t = 7 7.75e-6 / 4.50e-6; f4 t = 5 8.51e-6 /
    6.53e-6, t = 7 1.28e-5 / 6.48e-6 - each half accumulates 64 channels where the single launch accumulates 128."""
    from edvr_amd import ops
    b, c, co, h, w = 2, 64, 64, 19, 100  # vector and scalar blocks, ragged rows
    n, pmap = b * t, (t, t, t // 2)
    e_old, e_new = [], []
    for seed in range(5):
        g = torch.Generator().manual_seed(77 + 10 * t + seed)
        feat = torch.randn(n, c, h, w, generator=g)  # nbr and ref are the SAME tensor in EDVR.forward
        wt = torch.randn(co, 2 * c, 3, 3, generator=g) * 0.05
        bias = torch.randn(co, generator=g)
        idx = [(i // t) * t + t // 2 for i in range(n)]
        ref = F.leaky_relu(F.conv2d(torch.cat([feat, feat[idx]], 1).double(), wt.double(), bias.double(), 1, 1), 0.1)
        fg, wg, bg = feat.to(gpu), wt.to(gpu), bias.to(gpu)

        def packs(ci_range=None):
            k = dict(ci_range=ci_range) if ci_range else {}
            if kernel == 'f4s':
                return ops.pack_conv_weight(wg, **k), dict(wpk_f4s=ops.pack_conv_weight(wg, f4s=True, **k), algo=ops.CONV_WINOGRAD_F4S)
            return ops.pack_conv_weight(wg, **k), dict(wpk_f4=ops.pack_conv_weight(wg, f4=True, **k), algo=ops.CONV_WINOGRAD_F4)
        wpk, kw = packs()
        old = ops.conv2d(fg, wpk, bg, co, 3, x2=fg, x2_map=pmap, act=ops.ACT_LRELU, **kw)
        wpk_b, kw_b = packs((c, 2 * c))
        p = ops.conv2d(fg[t // 2::t], wpk_b, None, co, 3, **kw_b)
        assert p.shape[0] == b
        wpk_a, kw_a = packs((0, c))
        new = ops.conv2d(fg, wpk_a, bg, co, 3, act=ops.ACT_LRELU, pre=p, pre_map=(t, 1, 0), **kw_a)
        torch.cuda.synchronize()
        e_old.append(_rel(old, ref))
        e_new.append(_rel(new, ref))
    print(f'identity {kernel} t={t}: old {["%.3e" % e for e in e_old]} new {["%.3e" % e for e in e_new]}')
    assert max(e_new) < RTOL_F4 and max(e_old) < RTOL_F4, (e_old, e_new)
    assert max(e_new) <= max(e_old) + (max(e_old) - min(e_old)), (e_old, e_new)


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', ['f4s', 'f4'])
def test_no_pre_is_the_same_launch(gpu, kernel):
    """pre=None: the descriptor's new fields are zero and the result equals a call that never names them, bit for bit - also through the
    residual / gate epilogues that share the registers, and on the scalar edge path."""
    from edvr_amd import ops
    g = torch.Generator().manual_seed(5)
    n, c, h, w, co = 3, 32, 13, 100, 70
    x, wt, b = torch.randn(n, c, h, w, generator=g).to(gpu), (torch.randn(co, c, 3, 3, generator=g) * 0.1).to(gpu), torch.randn(co, generator=g).to(gpu)
    r, gt = torch.randn(n, co, h, w, generator=g).to(gpu), torch.randn(n, co, h, w, generator=g).relu().to(gpu)
    kw = dict(wpk_f4s=ops.pack_conv_weight(wt, f4s=True), algo=ops.CONV_WINOGRAD_F4S) if kernel == 'f4s' else \
        dict(wpk_f4=ops.pack_conv_weight(wt, f4=True), algo=ops.CONV_WINOGRAD_F4)
    wpk = ops.pack_conv_weight(wt)
    for extra in (dict(act=ops.ACT_LRELU), dict(act=ops.ACT_RELU, res1=r), dict(gate=gt, gate_slope=0.1), dict(act=ops.ACT_SIGMOID, act_from=40)):
        a = ops.conv2d(x, wpk, b, co, 3, **extra, **kw)
        bb = ops.conv2d(x, wpk, b, co, 3, pre=None, pre_map=None, **extra, **kw)
        assert torch.equal(a, bb)
    # ... and a zero addend changes nothing but the sign of a zero: act(v + 0) == act(v)
    z = torch.zeros(1, co, h, w, device=gpu)
    a = ops.conv2d(x, wpk, b, co, 3, act=ops.ACT_LRELU, **kw)
    bb = ops.conv2d(x, wpk, b, co, 3, act=ops.ACT_LRELU, pre=z, pre_map=(n, 0, 0), **kw)
    assert torch.equal(a, bb)


@pytest.mark.gpu
@pytest.mark.parametrize('val', NONFINITE, ids=['nan', 'inf', '-inf'])
@pytest.mark.parametrize('path', ['vec', 'scalar'])
def test_nonfinite_pre_reaches_output_slot_and_guard(guard, gpu, path, val):  # noqa: F811
    """One non-finite element of `pre` at a corner, an interior and an off-corner position of a tile (and in the last, 2-row tile row):
    y has it where the float64 reference has it, the y_amax slot holds it, the guard raises - as for one in res1."""
    ops = guard
    h, w = (10, 64) if path == 'vec' else (10, 36)
    g = torch.Generator().manual_seed(9)
    n, c, co = 4, 16, 64
    x, wt, b = torch.randn(n, c, h, w, generator=g), torch.randn(co, c, 3, 3, generator=g) * 0.1, torch.randn(co, generator=g)
    p = torch.randn(2, co, h, w, generator=g)
    wg = wt.to(gpu)
    wpk, wf4s = ops.pack_conv_weight(wg), ops.pack_conv_weight(wg, f4s=True)
    conv = F.conv2d(x.double(), wt.double(), b.double(), 1, 1)

    def run():
        with _Names() as names:
            y = ops.conv2d(x.to(gpu), wpk, b.to(gpu), co, 3, act=ops.ACT_LRELU, pre=p.to(gpu), pre_map=(2, 1, 0), wpk_f4s=wf4s, algo=ops.CONV_WINOGRAD_F4S)
        assert names.convs() == [F4S_NAME], names.seen
        return y, F.leaky_relu(conv + p.double()[[0, 0, 1, 1]], 0.1), ops.get_bound(y)
    y, ref, bound = run()  # finite: quiet guard, a true bound
    torch.cuda.synchronize()
    assert bound.item() >= y.abs().max().item()
    _assert_guard_quiet(ops, gpu)
    for ty, tx in [(4, 8), (8, 16), (0, 32)]:  # an interior tile, a tile of the last (2-row) tile row, a tile of the edge block (scalar path: w = 36)
        for i, j in [(0, 0), (3, 3), (1, 2), (0, 3), (2, 1)]:  # corners, interior, off-corner
            if ty + i >= h or tx + j >= w:
                continue
            keep = p[1, 5, ty + i, tx + j].item()
            p[1, 5, ty + i, tx + j] = val
            y, ref, bound = run()
            _nf_check(ops, gpu, y, ref, bound)
            assert (~torch.isfinite(y.cpu())).sum().item() == 2  # images 2 and 3 read it, nothing else does
            p[1, 5, ty + i, tx + j] = keep


@pytest.mark.gpu
def test_host_checks_reject_what_the_epilogue_cannot_do(gpu):
    from edvr_amd import _lib, ops
    g = torch.Generator().manual_seed(3)
    n, c, h, w, co = 4, 32, 16, 64, 64
    x, wt = torch.randn(n, c, h, w, generator=g).to(gpu), (torch.randn(co, c, 3, 3, generator=g) * 0.1).to(gpu)
    p, r = torch.randn(2, co, h, w, generator=g).to(gpu), torch.randn(n, co, h, w, generator=g).to(gpu)
    wpk, wf4s, wf4 = ops.pack_conv_weight(wt), ops.pack_conv_weight(wt, f4s=True), ops.pack_conv_weight(wt, f4=True)
    kw = dict(wpk_f4s=wf4s, algo=ops.CONV_WINOGRAD_F4S)
    ops.conv2d(x, wpk, None, co, 3, pre=p, pre_map=(2, 1, 0), **kw)  # the valid call
    for bad, msg in [(dict(pre=p, pre_map=(2, 1, 0), res1=r), 'pre excludes'),
                     (dict(pre=p, pre_map=(2, 1, 0), gate=r), 'pre excludes'),
                     (dict(pre=p, pre_map=(2, 1, 0), out_mode=ops.OUT_PIXEL_SHUFFLE2), 'pre excludes'),
                     (dict(pre=p, pre_map=(1, 1, 0)), 'image map'),       # image 3 -> 3 >= n_pre = 2
                     (dict(pre=p, pre_map=(2, 1, 1)), 'image map'),       # image 3 -> 2
                     (dict(pre=p, pre_map=None), 'image map'),            # identity map over 4 images, 2 in pre
                     (dict(pre=p, pre_map=(2, 1, -1)), 'image map')]:
        with pytest.raises(RuntimeError, match=msg):
            ops.conv2d(x, wpk, None, co, 3, **bad, **kw)
    for shape in [(2, co + 1, h, w), (2, co, h + 1, w), (2, co, h, w - 4)]:
        with pytest.raises(RuntimeError, match='pre shape'):
            ops.conv2d(x, wpk, None, co, 3, pre=torch.zeros(shape, device=gpu), pre_map=(2, 1, 0), **kw)
    # a kernel without the operand: the direct / F(2x2) kernels, and an addend that is not 16-byte aligned
    for algo_kw in (dict(algo=ops.CONV_DIRECT), dict(algo=ops.CONV_WINOGRAD)):
        with pytest.raises(RuntimeError, match='F\\(4x4\\) Winograd kernels only'):
            ops.conv2d(x, wpk, None, co, 3, pre=p, pre_map=(2, 1, 0), **algo_kw)
    flat = torch.zeros(p.numel() + 1, device=gpu)
    with pytest.raises(RuntimeError, match='F\\(4x4\\) Winograd kernels only'):
        ops.conv2d(x, wpk, None, co, 3, pre=flat[1:].view(p.shape), pre_map=(2, 1, 0), wpk_f4=wf4, algo=ops.CONV_WINOGRAD_F4)
    # the raw descriptor: an image stride below one image of (co, h, w)
    y = torch.empty(n, co, h, w, device=gpu)
    d = _lib.ConvDesc()
    d.x1, d.c1, d.x1_img_stride, d.n, d.h, d.w = x.data_ptr(), c, c * h * w, n, h, w
    d.wpk, d.co, d.ks, d.stride, d.y, d.y_img_stride = wpk.data_ptr(), co, 3, 1, y.data_ptr(), co * h * w
    d.wpk_f4, d.algo = wf4.data_ptr(), ops.CONV_WINOGRAD_F4
    d.pre, d.pre_img_stride, d.pre_div, d.pre_mul, d.pre_n = p.data_ptr(), co * h * w - 4, 2, 1, 2
    assert _lib.lib().edvr_conv2d_f32(ctypes.byref(d), None) == -1
    assert b'pre must be' in _lib.lib().edvr_last_error()
    assert ops.conv_pre_supported(n, c, h, w, co, True) and ops.conv_pre_supported(n, c, h, w, co, False)
    assert not ops.conv_pre_supported(n, c, h, w + 2, co, False)  # w % 4 != 0: no F(4x4) kernel


# ------------------------------------------------------------------------------------------------ module level
L_CONFIGS = {  # EDVR-L's width; sizes at which all three pyramid levels reach the F(4x4) kernels (w >= 32 at 1/4 size)
    'L_T5': (dict(num_feat=128, num_frame=5, num_reconstruct_block=2, center_frame_idx=None), (2, 5, 3, 32, 128)),
    'L_T7': (dict(num_feat=128, num_frame=7, num_reconstruct_block=2, center_frame_idx=None), (1, 7, 3, 32, 128)),
}


def _build_l(name, seed=10):
    from edvr_amd import EDVR
    from util_edvr import randomize_offsets
    kwargs, shape = L_CONFIGS[name]
    torch.manual_seed(seed)
    net = randomize_offsets(EDVR(**kwargs)).eval()
    return net, torch.rand(*shape, generator=torch.Generator().manual_seed(0)), kwargs


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(L_CONFIGS))
def test_pcd_alignment_with_shared_reference_half(gpu, name, monkeypatch):
    from edvr_amd import functional as F_, graphs
    from oracle import edvr_oracle as EO
    from util_edvr import oracle_kwargs
    net, x, kwargs = _build_l(name)
    keys = list(net.state_dict())
    versions = {k: v._version for k, v in net.state_dict(keep_vars=True).items()}
    taps_ref = {}
    with torch.no_grad():
        ref = EO.edvr_forward({k: v.double() for k, v in net.state_dict().items()}, x.double(), taps=taps_ref, **oracle_kwargs(kwargs))
    net, xg = net.to(gpu), x.to(gpu)
    errs, launches = {}, {}
    for on in (True, False):
        monkeypatch.setattr(F_, 'PRE_SPLIT', on)
        monkeypatch.setattr(F_, 'PRE_SPLIT_MIN_ITEMS', 0)  # (these sizes are below the one-item-per-CU threshold: take the path anyway)
        net.taps = {}
        with torch.no_grad(), _Names() as names:
            out = net(xg)
        torch.cuda.synchronize()
        launches[on] = len(names.convs())
        errs['eager', on] = (_rel(net.taps['aligned'].reshape(taps_ref['aligned'].shape), taps_ref['aligned']), _rel(out, ref))
        net.taps = {}
        gr = graphs.GraphedEDVR(net, xg, warmup=1)
        out_g = gr(xg)
        torch.cuda.synchronize()
        errs['graph', on] = (_rel(net.taps['aligned'].reshape(taps_ref['aligned'].shape), taps_ref['aligned']), _rel(out_g, ref))
        assert torch.equal(gr(xg), out_g)  # a fixed launch sequence: replays are bit-identical
        del gr
        net.taps = None
    print(f'{name}: (aligned, out) rel err vs fp64 {errs}; conv launches {launches}')
    assert launches[True] == launches[False] + 4, launches  # offset_conv1 l3 / l2 / l1 and cas_offset_conv1: one more launch each
    for k, (ea, eo) in errs.items():
        assert ea < INTERMEDIATE_RTOL and eo < INTERMEDIATE_RTOL, (k, ea, eo)
    # the module still owns one (128, 256, 3, 3) parameter per layer: keys, shapes and versions as before
    sd = net.state_dict(keep_vars=True)
    assert list(sd) == keys and {k: v._version for k, v in sd.items()} == versions
    assert tuple(sd['pcd_align.offset_conv1.l1.weight'].shape) == (128, 256, 3, 3) and tuple(sd['pcd_align.cas_offset_conv1.weight'].shape) == (128, 256, 3, 3)


@pytest.mark.gpu
def test_load_state_dict_invalidates_the_packed_halves(gpu, monkeypatch):
    from edvr_amd import functional as F_
    from oracle import edvr_oracle as EO
    from util_edvr import oracle_kwargs
    monkeypatch.setattr(F_, 'PRE_SPLIT', True)
    monkeypatch.setattr(F_, 'PRE_SPLIT_MIN_ITEMS', 0)
    net, x, kwargs = _build_l('L_T5')
    other, _, _ = _build_l('L_T5', seed=11)
    net, xg = net.to(gpu), x.to(gpu)
    with torch.no_grad():
        first = net(xg).clone()
        net.load_state_dict(other.state_dict(), strict=True)  # the reference's keys, in-place copy_: versions move, the packs follow
        taps_ref = {}
        ref = EO.edvr_forward({k: v.double() for k, v in other.state_dict().items()}, x.double(), taps=taps_ref, **oracle_kwargs(kwargs))
        net.taps = {}
        out = net(xg)
    assert not torch.equal(out, first)
    assert _rel(net.taps['aligned'].reshape(taps_ref['aligned'].shape), taps_ref['aligned']) < INTERMEDIATE_RTOL
    assert _rel(out, ref) < INTERMEDIATE_RTOL


def test_conv_items_follow_the_kernel_geometry():
    """functional._conv_items == the item count of csrc/winograd_f4s.hip f4s_geometry (the block shape that pads less), on the shapes of
    the headline workload's three pyramid levels and on small ones."""
    from edvr_amd import functional as F_
    for n, h, w, co in [(50, 180, 320, 128), (50, 90, 160, 128), (50, 45, 80, 128), (7, 32, 48, 128), (5, 32, 32, 64), (3, 13, 36, 70)]:
        bh, bw = _geometry(h, w)
        assert F_._conv_items(n, h, w, co) == n * -(-co // 64) * -(-h // bh) * -(-w // bw), (n, h, w, co)
    assert F_._conv_items(50, 45, 80, 128) > 256 > F_._conv_items(7, 32, 48, 128)  # every level of the headline clip splits; a 32 x 48 clip does not


@pytest.mark.gpu
def test_small_layers_keep_the_two_input_launch(gpu, monkeypatch):
    """Below one work item per CU the split cannot pay (functional.conv_shared_x2): the launch sequence is the two-input one, and the
    result is the two-input launch's bit for bit."""
    from edvr_amd import functional as F_
    g = torch.Generator().manual_seed(4)
    m = torch.nn.Conv2d(128, 64, 3, 1, 1).to(gpu)
    feat = torch.randn(10, 64, 32, 64, generator=g).to(gpu)
    assert F_._conv_items(10, 32, 64, 64) <= torch.cuda.get_device_properties(gpu).multi_processor_count
    monkeypatch.setattr(F_, 'PRE_SPLIT', True)
    with torch.no_grad(), _Names() as names:
        y = F_.conv_shared_x2(m, feat, feat, (5, 5, 2), act=F_.ACT_LRELU)
    assert len(names.convs()) == 1, names.seen
    with torch.no_grad():
        assert torch.equal(y, F_.conv(m, feat, x2=feat, x2_map=(5, 5, 2), act=F_.ACT_LRELU))
        monkeypatch.setattr(F_, 'PRE_SPLIT_MIN_ITEMS', 0)
        with _Names() as names:
            F_.conv_shared_x2(m, feat, feat, (5, 5, 2), act=F_.ACT_LRELU)
    assert len(names.convs()) == 2, names.seen
