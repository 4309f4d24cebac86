"""-m gpu: the five dX routes of the DCNv2 backward (dcn_bwd_fused_kernel; dcn_bwd_dx_strip_kernel + dcn_bwd_coord_kernel<false>;
dcn_bwd_coord_tile_kernel<3> / <6>; dcn_bwd_coord_kernel<true>) at the exact edges of their cells and windows, against the C oracle
in fp64.  Every call first asserts, through edvr_dcnv2_bwd_kernel_name, the kernel it is about to run: a silent fallback fails.

The fields and geometries come from tests/util_dcn_bwd.py; tests/test_dcn_bwd_geom_cpu.py proves that, per route, they put at least
half a wave of taps into every edge class of that route's window, onto each strict limit of the validity rule (h == -1, h == H,
w == -1, w == W), into each clipped-corner class and at offsets of exactly -1.0.  The older cases rest on white noise: none of their
taps sits on such a position, and the integer, half-integer and mostly-out-of-bounds cases written for the fused kernel never reach
it (W < 32: the staged strip pair).  A mistake there leaves the
sampled value and dMask unchanged and shows in dOffset or dX only.  Tolerances are those of tests/test_gpu_dcn.py.  Every input is
finite, every offset within +-80 px.

When written, the largest error against the oracle (BWD_RTOL = 1e-4), over the five gradients:
  route    exact fields (ladder*, sub, border)    noise16
  fused    6.1e-7 (dx, F1 border)                 3.9e-6 (doffset, F1)
  strip    6.2e-7 (dx, S1 border)                 4.8e-6 (dmask, S1)
  tile3    5.4e-7 (dx, F1 border)                 3.9e-6 (doffset, F1)
  tile6    6.5e-7 (dx, F1 border)                 3.9e-6 (doffset, F1)
  device   9.3e-7 (dx, F1 border)                 3.9e-6 (doffset, F1)
Across routes on F1 dMask was bit-identical and dOffset within 1.5e-7 of its largest element (bound 2e-5); the split dW product
stayed within 5.3e-7 of the oracle.  Nothing failed on the real kernels.

That these tests can fail - from one-line changes in a SCRATCH copy of the kernels (never committed), each run once through this file
and tests/test_gpu_dcn.py:
  * dcn_bwd_fused.hip, `h > -1.f` -> `h >= -1.f` in `valid`: fails here on fused F1 / F2 with ladder_int, sub and border (oracle
    comparison, guard-band test) and in the cross-route comparison on those three fields - 11 tests; tests/test_gpu_dcn.py passes whole.
  * dcn_bwd_fused.hip, `wr <= IH - 2` -> `wr <= IH - 1`: fails here on fused F1 with ladder, ladder_int, ladder_half and noise16, in
    the cross-route comparison on those, in the repeatability and split-dW tests on F1 ladder - 10 tests; the older file sees it too
    (three CASES rows under 'strip', the strided-slices test at sigma 1.5).
  * dcn.hip, strip kernel, `lane > 61` -> `lane > 62`: fails here on strip S1 with ladder_half, sub, border, S2 with ladder, sub,
    border and both guard-band cases - 8 tests; the older file sees it on its two multi-strip rows.
"""
import functools

import pytest
import torch

import util_dcn_bwd as U
from test_gpu_dcn import BWD_RTOL, _rel

pytestmark = pytest.mark.gpu

NAMES = ('dx', 'doffset', 'dmask', 'dweight', 'dbias')
ROUTE_CASES = [(route, label) for route, (_, labels) in U.ROUTES.items() for label in labels]
SENTINEL = -12345.5


@functools.lru_cache(maxsize=None)
def _case(label, field):
    """CPU tensors (x, off, m, w, dy), the oracle's fp64 gradients and the dOffset flip mask: computed once, shared, never written to."""
    ref, flip = U.oracle_backward(label, field)
    if field in U.EXACT_FIELDS:
        assert not flip.any()  # (proven on the CPU: tests/test_dcn_bwd_geom_cpu.py)
    else:
        assert flip.sum().item() <= 2
    return U.case_tensors(label, field), ref, flip


def _backward(ops, route, label, dev, **kw):
    """ops.dcnv2_backward under the route's hint, after asserting the kernel the launch will pick."""
    hint, dg = U.HINTS[U.ROUTES[route][0]], U.GEOMS[label][2]
    x, off, m, w, dy = dev
    assert ops.dcnv2_backward_kernel_name(x, w, 1, 1, 1, 1, dg, hint) == U.KERNEL_NAMES[route], (route, label)
    out = ops.dcnv2_backward(x, off, m, w, dy, True, 1, 1, 1, 1, dg, scatter_hint=hint, **kw)
    torch.cuda.synchronize()
    return out


def _errors(grads, ref, flip):
    errs = {}
    for name, a, r in zip(NAMES, grads, ref):
        a = a.double().cpu()
        if name == 'doffset' and flip.any():  # (noise16 only; empty on the exact fields)
            a, r = a.masked_fill(flip, 0.), r.masked_fill(flip, 0.)
        errs[name] = _rel(a, r)
    return errs


@pytest.mark.parametrize('field', U.FIELDS)
@pytest.mark.parametrize('route,label', ROUTE_CASES)
def test_backward_routes_at_their_cell_edges(gpu, route, label, field):
    """All five gradients of every route against the oracle in fp64 at BWD_RTOL, relative to the largest element."""
    from edvr_amd import ops
    tensors, ref, flip = _case(label, field)
    grads = _backward(ops, route, label, [t.to(gpu) for t in tensors])
    errs = _errors(grads, ref, flip)
    print(f'\n[dcn-bwd-edges] {route} {label} {field}: rel err vs fp64 oracle  ' + '  '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    for name in NAMES:
        assert errs[name] < BWD_RTOL, (name, errs)


@pytest.mark.parametrize('route,label', ROUTE_CASES)
def test_gradient_slices_are_written_inside_their_guard_bands(gpu, route, label):
    """The training path's call on the `border` field: offsets and masks are channel slices of one tensor, dOffset and dMask channel
    slices of one buffer with four sentinel planes before, between and after them (per image: between images as well), x and dy
    16-byte aligned views at a storage offset of 4 floats.  Every sentinel is unchanged, every plane of the slices is written, no
    input is written, and the gradients are the oracle's."""
    from edvr_amd import ops
    (x, off, m, w, dy), ref, flip = _case(label, 'border')
    B, C, dg, Co, H, W = U.GEOMS[label]
    n_off, n_m = dg * 18, dg * 9
    om = torch.cat([off, m], 1).to(gpu)
    om0 = om.clone()
    views, bufs = [], []
    for t in (x, dy):
        buf = torch.zeros(t.numel() + 8, device=gpu)
        v = buf[4:4 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.storage_offset() == 4 and v.data_ptr() % 16 == 0 and v.is_contiguous()
        views.append(v)
        bufs.append(buf)
    gbuf = torch.full((B, 4 + n_off + 4 + n_m + 4, H, W), SENTINEL, device=gpu)
    doff, dmsk = gbuf[:, 4:4 + n_off], gbuf[:, 8 + n_off:8 + n_off + n_m]
    doff.fill_(float('nan'))
    dmsk.fill_(float('nan'))
    dx, _, _, dw, db = _backward(ops, route, label, [views[0], om[:, :n_off], om[:, n_off:], w.to(gpu), views[1]], doffset=doff, dmask=dmsk)
    for band in (gbuf[:, :4], gbuf[:, 4 + n_off:8 + n_off], gbuf[:, 8 + n_off + n_m:]):
        assert band.shape[1] == 4 and (band == SENTINEL).all()
    assert torch.isfinite(doff).all() and torch.isfinite(dmsk).all()
    assert torch.equal(om, om0) and torch.equal(views[0].cpu(), x) and torch.equal(views[1].cpu(), dy)
    for buf in bufs:
        assert (buf[:4] == 0).all() and (buf[-4:] == 0).all()
    errs = _errors((dx, doff, dmsk, dw, db), ref, flip)
    for name in NAMES:
        assert errs[name] < BWD_RTOL, (name, errs)


@pytest.mark.parametrize('field', ['ladder', 'sub'])
@pytest.mark.parametrize('route,label', ROUTE_CASES)
def test_two_launches_agree(gpu, route, label, field):
    """dOffset and dMask are one thread's arithmetic per element, the column GEMM and the split-K reduction of dW are deterministic:
    bit for bit.  dX differs by the order of its atomics only: 1e-5 of its largest element, the bound tests/test_gpu_dcn.py uses for
    'the same code'."""
    from edvr_amd import ops
    tensors, _, _ = _case(label, field)
    dev = [t.to(gpu) for t in tensors]
    a, b = _backward(ops, route, label, dev), _backward(ops, route, label, dev)
    for name, u, v in zip(NAMES[1:], a[1:], b[1:]):
        assert torch.equal(u, v), (name, (u - v).abs().max().item())
    assert _rel(a[0], b[0].double().cpu()) < 1e-5


@pytest.mark.parametrize('field', U.FIELDS)
def test_routes_agree_on_doffset_and_dmask(gpu, field):
    """Geometry F1 runs on four routes.  dOffset and dMask are the same arithmetic per (pixel, tap) on each - no summation-order
    freedom beyond the channel sum -: within 2e-5 of their largest element, the cross-path bound of tests/test_gpu_dcn.py."""
    from edvr_amd import ops
    tensors, _, _ = _case('F1', field)
    dev = [t.to(gpu) for t in tensors]
    routes = [r for r, (_, labels) in U.ROUTES.items() if 'F1' in labels]
    assert routes == ['fused', 'tile3', 'tile6', 'device']
    got = {r: _backward(ops, r, 'F1', dev)[1:3] for r in routes}
    for r in routes[:-1]:
        for name, a, b in zip(('doffset', 'dmask'), got[r], got['device']):
            d = (a - b).abs().max().item() / b.abs().max().item()
            print(f'\n[dcn-bwd-edges] F1 {field}: {name} {r} vs device  {d:.3e}')
            assert d <= 2e-5, (r, name, d)


@pytest.mark.parametrize('field', ['ladder', 'sub'])
@pytest.mark.parametrize('route,label', [('fused', 'F1'), ('strip', 'S1')])
def test_split_dw_after_the_fused_kernel_and_after_the_strip_pair(gpu, route, label, field):
    """The dW product on split operands (csrc/gemm_nt_s.hip) fed by the columns the fused kernel and the strip pair leave behind: the
    assertions of test_backward_split_dw_matches_oracle, which never selects either (hint AUTO)."""
    from edvr_amd import _lib, ops
    tensors, ref, _ = _case(label, field)
    dev = [t.to(gpu) for t in tensors]
    assert _lib.lib().edvr_dcnv2_bwd_split_applies() == 1
    g32 = _backward(ops, route, label, dev)
    gs = _backward(ops, route, label, dev, xm_bound=ops.amax(dev[0]), dy_bound=ops.amax(dev[4]))
    e32, es = _rel(g32[3], ref[3]), _rel(gs[3], ref[3])
    print(f'\n[dcn-bwd-edges] {route} {label} {field}: dweight rel err  split {es:.3e}  fp32 {e32:.3e}')
    assert es < BWD_RTOL and es < 1.5 * e32 + 2e-7, (es, e32)
    for a, c in zip(gs[:3] + gs[4:], g32[:3] + g32[4:]):  # everything else is the same code: equal up to the order of the dx atomics
        assert _rel(a, c.double().cpu()) < 1e-5
