"""-m gpu: every DCN kernel on what a diverging conv_offset produces - offsets of 1e4 px, at and beyond +-2^31, of FLT_MAX, +-inf and
NaN on a quarter of the taps, on every tap of the "dead" pixels and of one dead tile - against the C oracle in fp64.  The rule
(include/edvr_amd.h): a sampling position outside (-1, H) x (-1, W), +-inf and NaN included, adds nothing to y, dX or dW and has
dOffset = dMask = 0.  The oracle's answer does not depend on the poison value, bit for bit: one reference per (geometry, base field).

The fields come from tests/util_dcn_poison.py over the geometries, base fields and routes of the two edge files;
tests/test_dcn_poison_cpu.py proves on the CPU what this file relies on.  Every call asserts the kernel it ran (ops.LAUNCH_HOOK in the
forward, ops.dcnv2_backward_kernel_name in the backward); tolerances are those of tests/test_gpu_dcn.py.  x, masks, weights and dy are
finite throughout: a NaN mask on an invalid tap is 0 x NaN in the reference too, and not what this file is about.

What these tests found, on the kernels as they were:
  * dcn_tap.h resolve_tap (column-buffer forward, the window and device-atomic backward routes, DCNv1; its twin in dcn_any.hip): a
    position of 2^31 or more - int_range, fltmax, +inf - converted to INT_MAX, `h0 + 1` wrapped, and the clamp of the lower / right
    corner, compiled as min(max(h0, -1) + 1, H - 1), came out as INT_MIN: the corner loads, unconditional because their weight is 0,
    read 8 GiB below the plane - an illegal memory access in the first int_range case.  The floor is now kept inside [-2, n] before
    the conversion (cell_origin); a valid tap's is untouched.
  * the five places that restate the validity rule by hand built their weights from lh = h - floorf(h) ungated: an invalid tap at
    +-inf or NaN had lh = NaN, and its zero mask (or zero dcol) did not stop it: 0 x NaN.
That the tests can fail - a SCRATCH copy of the library (never committed) with the five NaN gates taken out again and cell_origin kept,
run once through this file: 45 of 125 tests fail, all on the kinds inf, nan and mixed (far, int_range, fltmax pass: lh is finite there):
  dcn_fused.hip      finish_taps   `valid ? h - fh : 0.f` -> `h - fh`: y = NaN wherever a pixel holds such a tap (A 1088 .. 2048 of 2048
                                   elements, D all 184960) in fused R = 3 and R = 7: test_forward_kernels[*-inf / nan / mixed], 20 cases;
                                   with it the autograd, DCNv1 and deform_conv_ext tests, whose forward is this kernel
  dcn_tapwin.hip     state_half    the same line: the same 20 cases, the fp32 tap-window kernel
  dcn_tapwin_s.hip   state_half    the same line: the same 20 cases, the split kernel packed per call and per parameter
  dcn_bwd_fused.hip  consume       `valid ? s_y * o_m : 0.f` -> `s_y * o_m` (and s_x): dOffset = NaN at 6170 .. 24306 of F1's 36460
                                   poisoned components: test_backward_routes[fused-F1 / F2-...], 10 cases, test_split_dw_after_every_route[fused]
  dcn.hip            strip kernel  `valid ? ph - fh : 0.f` -> `ph - fh`: dX = NaN (a NaN column weight times a zero row weight in the
                                   5 x 5 patch; 34288 .. 38080 of S1's 38080 elements): test_backward_routes[strip-S1 / S2-...], 10 cases,
                                   test_split_dw_after_every_route[strip]
The column-buffer kernel, the window and device-atomic routes and dcn_any gate every weight by the tap's validity: finite in that run.
With the gates in, the largest error against the oracle over all cases was 2.0e-6 in the forward (FWD_RTOL = 2e-5) and 1.0e-6 in the
backward (BWD_RTOL = 1e-4); a tap-window kernel's result moved by at most 2.1e-7 of the output scale between kinds (bound 2e-5)."""
import pytest
import torch

import util_dcn_bwd as UB
import util_dcn_poison as P
from test_gpu_dcn import BWD_RTOL, FWD_RTOL, _rel
from test_gpu_dcn_bwd_edges import NAMES, ROUTE_CASES, _backward
from test_gpu_dcn_tapwin_edges import FUSED, _Runner, _to_device

pytestmark = pytest.mark.gpu

COLUMN = 'dcnv2_fwd[dcn_im2col_kernel]'
FWD_KERNELS = ('column', 'fused3', 'fused7', 'tapwin', 'split', 'packed')
_far_cache = {}


def _forward_all(gpu, label, field, kind):
    """{kernel: y} of one forward case on the six forward paths, each asserting the kernel it ran; computed once per case."""
    key = ('fwd', label, field, kind)
    if key not in _far_cache:
        from edvr_amd import ops
        x, _, m, w, b = P.fwd_tensors(label, field)
        off = P.fwd_offsets(label, field, kind)[0]
        run = _Runner(ops, _to_device(label, (x, off, m, w, b, None), gpu), P.FWD_GEOMS[label][2])
        bound = ops.amax(run.dev[0])
        _far_cache[key] = dict(column=run._call(COLUMN, halo_hint=-1), fused3=run._call(FUSED, halo_hint=3), fused7=run.halo7(), tapwin=run.fp32(),
                               split=run.split(bound), packed=run.packed(bound))
    return _far_cache[key]


@pytest.mark.parametrize('field,kind', P.FWD_CASES)
@pytest.mark.parametrize('label', sorted(P.FWD_GEOMS))
def test_forward_kernels(gpu, label, field, kind):
    """Column-buffer path, zero-centred halo kernel at R = 3 and R = 7, fp32 tap-window kernel, split tap-window kernel packing per call
    and per parameter: y finite, within FWD_RTOL of the oracle (the split form no further than 1.5 x the fp32 form + 2e-7, packed ==
    per call), exactly the bias at the dead pixels, and against the same kernel's result under `far`: bit for bit where the code path
    does not depend on the poison value, within 2e-5 of the output scale (the edge file's cross-kernel bound) for the tap-window
    kernels, whose window shift does."""
    ref = P.fwd_oracle(label, field)
    ys, far = _forward_all(gpu, label, field, kind), _forward_all(gpu, label, field, 'far')
    b = P.fwd_tensors(label, field)[4]
    dead = P.dead_pixels(*P.FWD_GEOMS[label][4:]).to(gpu)
    want_dead = (torch.zeros(ref.shape[1]) if b is None else b).to(gpu).view(1, -1, 1).expand(ref.shape[0], -1, int(dead.sum()))
    scale = ref.abs().max().item()
    errs = {k: _rel(y, ref) for k, y in ys.items()}
    shift = {k: (ys[k] - far[k]).abs().max().item() / scale for k in FWD_KERNELS}
    print(f'\n[dcn-poison] fwd {label} {field} {kind}: rel err vs fp64 oracle  ' + '  '.join(f'{k} {errs[k]:.3e}' for k in FWD_KERNELS) +
          '   vs far / max|ref|  ' + '  '.join(f'{k} {shift[k]:.1e}' for k in FWD_KERNELS))
    bad = []
    for k in FWD_KERNELS:
        y = ys[k]
        if not torch.isfinite(y).all():
            bad.append((k, 'not finite: %d NaN, %d inf of %d' % (int(torch.isnan(y).sum()), int(torch.isinf(y).sum()), y.numel())))
            continue
        if not errs[k] < FWD_RTOL:
            bad.append((k, 'rel err %.3e' % errs[k]))
        if not torch.equal(y[:, :, dead], want_dead):
            bad.append((k, 'dead pixels differ from the bias by %.3e' % (y[:, :, dead] - want_dead).abs().max().item()))
        if k in ('column', 'fused3', 'fused7'):
            if not torch.equal(y, far[k]):
                bad.append((k, 'differs from its result under far by %.3e of the scale' % shift[k]))
        elif not shift[k] <= 2e-5:
            bad.append((k, 'differs from its result under far by %.3e of the scale' % shift[k]))
    assert not bad, bad
    assert errs['split'] < 1.5 * errs['tapwin'] + 2e-7 and errs['packed'] < 1.5 * errs['tapwin'] + 2e-7, errs
    assert torch.equal(ys['split'], ys['packed'])


def _backward_case(gpu, route, label, field, kind, split=False):
    key = ('bwd', route, label, field, kind, split)
    if key not in _far_cache:
        from edvr_amd import ops
        x, _, m, w, dy = UB.case_tensors(label, field)
        dev = [t.to(gpu) for t in (x, P.bwd_offsets(label, field, kind)[0], m, w, dy)]
        kw = dict(xm_bound=ops.amax(dev[0]), dy_bound=ops.amax(dev[4])) if split else {}
        _far_cache[key] = _backward(ops, route, label, dev, **kw)
    return _far_cache[key]


def _check_gradients(grads, ref, mask, tol, what):
    """All five finite and within tol of the oracle; dOffset (both components) and dMask exactly 0 at the poisoned taps."""
    errs, bad = {}, []
    for name, a, r in zip(NAMES, grads, ref):
        if a is None and r is None:
            continue
        if not torch.isfinite(a).all():
            bad.append((name, 'not finite: %d NaN, %d inf of %d' % (int(torch.isnan(a).sum()), int(torch.isinf(a).sum()), a.numel())))
            continue
        errs[name] = _rel(a, r)
        if not errs[name] < tol:
            bad.append((name, 'rel err %.3e' % errs[name]))
    print(f'\n[dcn-poison] {what}: rel err vs fp64 oracle  ' + '  '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    mask = mask.to(grads[1].device)
    at_off, at_msk = grads[1][P.tap_to_offset_mask(mask)], grads[2][mask]
    if not torch.equal(at_off, torch.zeros_like(at_off)):
        bad.append(('doffset', '%d of %d poisoned components are not 0' % (int((~(at_off == 0)).sum()), at_off.numel())))
    if not torch.equal(at_msk, torch.zeros_like(at_msk)):
        bad.append(('dmask', '%d of %d poisoned taps are not 0' % (int((~(at_msk == 0)).sum()), at_msk.numel())))
    assert not bad, (what, bad)
    return errs


@pytest.mark.parametrize('field,kind', P.BWD_CASES)
@pytest.mark.parametrize('route,label', ROUTE_CASES)
def test_backward_routes(gpu, route, label, field, kind):
    """Every dX route on its two geometries: the five gradients finite and within BWD_RTOL of the oracle, dOffset and dMask exactly 0 at
    the poisoned taps, and dMask / dOffset (one thread's arithmetic per element) bit for bit what the same route gives under `far`."""
    grads, far = _backward_case(gpu, route, label, field, kind), _backward_case(gpu, route, label, field, 'far')
    _check_gradients(grads, P.bwd_oracle(label, field), P.bwd_offsets(label, field, kind)[1], BWD_RTOL, f'bwd {route} {label} {field} {kind}')
    assert torch.equal(grads[1], far[1]) and torch.equal(grads[2], far[2])


@pytest.mark.parametrize('route', list(UB.ROUTES))
def test_split_dw_after_every_route(gpu, route):
    """The dW product on split operands (gemm_nt_split_kernel) fed by the columns each route leaves behind on the `mixed` field: within
    BWD_RTOL, and no further from the oracle than 1.5 x the fp32 product + 2e-7."""
    from edvr_amd import _lib
    label = UB.ROUTES[route][1][0]
    assert _lib.lib().edvr_dcnv2_bwd_split_applies() == 1
    ref, mask = P.bwd_oracle(label, 'ladder'), P.bwd_offsets(label, 'ladder', 'mixed')[1]
    g32 = _backward_case(gpu, route, label, 'ladder', 'mixed')
    gs = _backward_case(gpu, route, label, 'ladder', 'mixed', split=True)
    _check_gradients(gs, ref, mask, BWD_RTOL, f'bwd split dW {route} {label} ladder mixed')
    e32, es = _rel(g32[3], ref[3]), _rel(gs[3], ref[3])
    print(f'\n[dcn-poison] {route} {label}: dweight rel err  split {es:.3e}  fp32 {e32:.3e}')
    assert es < BWD_RTOL and es < 1.5 * e32 + 2e-7, (es, e32)


# ------------------------------------------------------------------------------------------------ the other entry points, `mixed` only
def test_autograd_function_without_a_hint(gpu):
    """edvr_amd.modulated_deform_conv as a user calls it on geometry F1: no halo hint, the scatter hint from the statistics of the
    poisoned offsets themselves (non-finite sums) or none."""
    from edvr_amd import modulated_deform_conv
    from oracle import dcn_oracle as O
    x, _, m, w, dy = UB.case_tensors('F1', 'ladder')
    off, mask = P.bwd_offsets('F1', 'ladder', 'mixed')
    dg = P.BWD_GEOMS['F1'][2]
    ref_y = O.c_forward(x.double(), off.double(), m.double(), w.double(), None, 1, 1, 1, 1, dg)
    leaves = [t.to(gpu).requires_grad_() for t in (x, off, m, w)]
    y = modulated_deform_conv(*leaves, None, 1, 1, 1, 1, dg)
    assert torch.isfinite(y).all() and _rel(y.detach(), ref_y) < FWD_RTOL
    dead = P.dead_pixels(*P.BWD_GEOMS['F1'][4:]).to(gpu)
    assert (y.detach()[:, :, dead] == 0).all()
    y.backward(dy.to(gpu))
    _check_gradients([t.grad for t in leaves] + [None], list(P.bwd_oracle('F1', 'ladder'))[:4] + [None], mask, BWD_RTOL, 'autograd F1 ladder mixed')


def test_dcnv1_on_poisoned_offsets(gpu):
    """DeformConv (no mask) on the first row of test_gpu_dcn1.CASES, both scatter hints, at that file's tolerances."""
    import test_gpu_dcn1 as T1
    from edvr_amd import ops
    from oracle import dcn_oracle as O
    case = T1.CASES[0]
    x, off, w, dy, cfg = T1._mk(case)
    B, dg = case[0], case[10]
    mask = P.poison_mask(B, dg, off.shape[2], off.shape[3], 71001)
    off = P.poison(off, mask, 'mixed', 71002)
    assert P.invalid_in_float32(off.numpy(), dg)[mask].all() and 0.25 <= mask.float().mean().item() <= 0.5
    ref_y = O.c_dcn1_forward(x.double(), off.double(), w.double(), *cfg)
    ref_g = O.c_dcn1_backward(x.double(), off.double(), w.double(), dy.double(), *cfg)
    assert torch.isfinite(ref_y).all() and all(torch.isfinite(r).all() for r in ref_g)
    xg, og, wg, dyg = (t.to(gpu) for t in (x, off, w, dy))
    y = ops.dcnv1_forward(xg, og, wg, *cfg)
    assert torch.isfinite(y).all() and _rel(y, ref_y) < 2e-5
    for hint in (ops.DCN_SCATTER_LDS, ops.DCN_SCATTER_DEVICE):
        grads = ops.dcnv1_backward(xg, og, wg, dyg, *cfg, scatter_hint=hint)
        for name, a, r in zip(('dx', 'doffset', 'dweight'), grads, ref_g):
            assert torch.isfinite(a).all() and _rel(a, r) < 1e-4, (name, hint)
        at = grads[1][P.tap_to_offset_mask(mask).to(gpu)]
        assert torch.equal(at, torch.zeros_like(at)), hint


@pytest.mark.parametrize('dtype,tol', [(torch.float64, 1e-12), (torch.float16, 3e-3)], ids=['f64', 'f16'])
def test_float64_and_float16_on_poisoned_offsets(gpu, dtype, tol):
    """csrc/dcn_any.hip on the first row of test_gpu_dcn_dtypes.CASES at that file's tolerances; float16 takes its own value set (+-6e4,
    +-inf, NaN: none of the finite float32 values fits)."""
    import test_gpu_dcn_dtypes as TD
    from edvr_amd import modulated_deform_conv
    from oracle import dcn_oracle as O
    case = TD.CASES[0]
    t, cfg = TD._mk(case, dtype)
    B, dg = case[0], case[10]
    mask = P.poison_mask(B, dg, t['offset'].shape[2], t['offset'].shape[3], 72001)
    t['offset'] = P.poison(t['offset'], mask, 'mixed', 72002, half=dtype == torch.float16)
    assert P.invalid_in_float32(t['offset'].numpy(), dg)[mask].all()
    fin = t['offset'][torch.isfinite(t['offset'])]
    assert torch.equal(fin.to(dtype).double(), fin)  # the values the low-precision run sees
    ref_y = O.c_forward(t['x'], t['offset'], t['mask'], t['weight'], t['bias'], *cfg)
    ref_g = O.c_backward(t['x'], t['offset'], t['mask'], t['weight'], t['dy'], t['bias'] is not None, *cfg)
    dev = {k: (None if v is None else v.to(gpu, dtype)) for k, v in t.items()}
    leaves = [dev[k].requires_grad_() for k in ('x', 'offset', 'mask', 'weight', 'bias')]
    y = modulated_deform_conv(*leaves, *cfg)
    assert y.dtype == dtype and torch.isfinite(y).all() and _rel(y.detach(), ref_y) < tol
    y.backward(dev['dy'])
    _check_gradients([leaf.grad for leaf in leaves], ref_g, mask, tol, f'dcn_any {dtype}')


def test_deform_conv_ext_call_sites_on_poisoned_offsets(gpu):
    """One call through edvr_amd/compat/deform_conv_ext.py with the reference's argument lists (first row of
    test_gpu_compat_ext.MDCN_CASES): its backward takes the dX strategy from the statistics its forward noted - non-finite here."""
    import test_gpu_compat_ext as TC
    from edvr_amd.compat import deform_conv_ext as ext
    from oracle import dcn_oracle as O
    B, C, H, W, Co, k, stride, pad, dil, groups, dg, with_bias = case = TC.MDCN_CASES[0]
    assert (k, stride, pad, dil, groups, with_bias) == (3, 1, 1, 1, 1, True)
    g = torch.Generator().manual_seed(sum(map(int, case)))  # that test's own draws: its offsets are known to hold no tap that float32 rounds into another cell
    x = torch.randn(B, C, H, W, generator=g)
    base = torch.randn(B, dg * 18, H, W, generator=g) * 1.5
    m = torch.rand(B, dg * 9, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) * 0.1
    b = torch.randn(Co, generator=g)
    dy = torch.randn(B, Co, H, W, generator=g)
    mask = P.poison_mask(B, dg, H, W, 73001)
    off = P.poison(base, mask, 'mixed', 73002)
    cfg = (stride, pad, dil, groups, dg)
    ref_y = O.c_forward(x.double(), off.double(), m.double(), w.double(), b.double(), *cfg)
    ref_g = O.c_backward(x.double(), off.double(), m.double(), w.double(), dy.double(), True, *cfg)
    out = TC._reference_mdcn_call_sites(ext, x.to(gpu), off.to(gpu), m.to(gpu), w.to(gpu), b.to(gpu), *cfg, dy.to(gpu))
    assert torch.isfinite(out[0]).all() and _rel(out[0], ref_y) < FWD_RTOL
    _check_gradients(out[1:], ref_g, mask, BWD_RTOL, 'deform_conv_ext')
