"""-m gpu: the tap-window DCNv2 forward kernels (csrc/dcn_tapwin.hip, fp32; csrc/dcn_tapwin_s.hip, split operands on the f16 matrix
pipe) at the edges of their staged windows, against the C oracle in fp64.

The fields come from tests/util_tapwin.py; tests/test_tapwin_geom_cpu.py proves that they put at least half a wave of lanes on
each of the window's eight edge classes - per kernel instance family and at every column alignment - and windows over every image
border.  The older cases' smooth fields never reach four of those classes: an off-by-one in the window predicate, in the alignment or
in the clipping would read the neighbouring channel's window there - wrong numbers, not a fault.  Tolerances are those of
tests/test_gpu_dcn.py.  Every offset stays within +-30 px and every input is finite.

When written: the largest error against the oracle over all cases was 2.8e-6 (FWD_RTOL = 2e-5), fp32 and split forms alike.  With
`rx <= IW - 2` changed to `rx <= IW - 1` in a scratch copy of either kernel, the cases B / D / E-ladder and B / D / E-noise3 (and
D-noise1) fail with errors of 2e-4 .. 0.3 while every TAPWIN_CASES test of tests/test_gpu_dcn.py still passes.  (ladder_int cannot
see that particular change: at integer positions the right-hand corners carry zero weight.  Nor can A and C: in an image one tile wide
a lane in the window's last column has its right-hand corners outside the image.)"""
import functools

import pytest
import torch

import util_tapwin as U
from test_gpu_dcn import FWD_RTOL, _rel

pytestmark = pytest.mark.gpu

FP32, SPLIT, FUSED, PACK = ('dcnv2_fwd[dcn_tapwin_fwd_kernel]', 'dcnv2_fwd[dcn_tapwin_split_fwd_kernel]', 'dcnv2_fwd[dcn_fused_fwd_kernel]',
                            'dcn_split_pack_weight')


@functools.lru_cache(maxsize=None)
def _case(label, field, mask='rand', bias=True):
    """CPU tensors (x, off, m, w, b) of a geometry / field and the oracle's fp64 result, computed once and shared (never written to).
    mask: 'rand' = uniform in [0, 1), 'signed' = uniform in [-2, 2).  Geometry E never has a bias."""
    from oracle import dcn_oracle as O
    B, C, dg, Co, H, W = U.EDGE_GEOMS[label]
    g = torch.Generator().manual_seed(7000 + 31 * ord(label) + U.EDGE_FIELDS.index(field))
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) * 0.1
    b = torch.randn(Co, generator=g) if (bias and label != 'E') else None
    off = U.edge_field(label, field)
    m = torch.rand(B, dg * 9, H, W, generator=g)
    if mask == 'signed':
        m = m * 4 - 2
    assert off.abs().max().item() <= 30. and all(torch.isfinite(t).all() for t in (x, off, m, w))
    ref = O.c_forward(x.double(), off.double(), m.double(), w.double(), None if b is None else b.double(), 1, 1, 1, 1, dg)
    return x, off, m, w, b, ref


def _to_device(label, case, gpu):
    """-> (x, off, m, w, b) on the device.  Geometry E: offsets and masks are channel slices of ONE (B, 3 dg 9, H, W) tensor (image
    stride != planes x plane size), x is a 16-byte aligned view at a non-zero storage offset."""
    x, off, m, w, b, _ = case
    if label != 'E':
        return [None if t is None else t.to(gpu) for t in (x, off, m, w, b)]
    om = torch.cat([off, m], 1).to(gpu)
    n_off = off.shape[1]
    buf = torch.zeros(x.numel() + 4, device=gpu)
    xv = buf[4:].view(x.shape)
    xv.copy_(x)
    assert xv.storage_offset() == 4 and xv.data_ptr() % 16 == 0 and om[:, :n_off].stride(0) != n_off * off.shape[2] * off.shape[3]
    return [xv, om[:, :n_off], om[:, n_off:], w.to(gpu), None]


class _Runner:
    """The entry points under test, each asserting through ops.LAUNCH_HOOK the kernel it ran on: a silent fallback fails."""

    def __init__(self, ops, dev, dg):
        self.ops, self.dev, self.dg = ops, dev, dg
        self.w_param = torch.nn.Parameter(dev[3], requires_grad=False)  # same storage as dev[3]

    def _call(self, want, **kw):
        ops, names = self.ops, []
        ops.LAUNCH_HOOK = lambda name, flops, launch, *a: (names.append(name), launch())
        try:
            with torch.no_grad():
                y = ops.dcnv2_forward(*self.dev, 1, 1, 1, 1, self.dg, **kw)
        finally:
            ops.LAUNCH_HOOK = None
        assert names[-1:] == [want] and set(names[:-1]) <= {PACK}, (names, want)
        return y

    def fp32(self, act=0):
        return self._call(FP32, act=act, halo_hint=self.ops.DCN_HALO_TAPWIN)

    def split(self, bound, act=0):
        return self._call(SPLIT, act=act, halo_hint=self.ops.DCN_HALO_TAPWIN, xm_bound=bound)

    def packed(self, bound, act=0):
        assert self.w_param.data_ptr() == self.dev[3].data_ptr()
        return self._call(SPLIT, act=act, halo_hint=self.ops.DCN_HALO_TAPWIN, xm_bound=bound, w_param=self.w_param)

    def halo7(self, act=0):
        return self._call(FUSED, act=act, halo_hint=7)


@pytest.mark.parametrize('field', U.EDGE_FIELDS)
@pytest.mark.parametrize('label', sorted(U.EDGE_GEOMS))
def test_tap_window_kernels_at_their_window_edges(gpu, label, field):
    """fp32 tap-window, split packing per call, split with the weights packed per parameter: each against the oracle at FWD_RTOL; the
    split form no further from it than 1.5 x the fp32 form + 2e-7; packed == per call and two launches of one call bit for bit; fp32
    tap-window and the R = 7 halo kernel within 2e-5 of the output scale."""
    from edvr_amd import ops
    case = _case(label, field)
    ref, dg = case[5], U.EDGE_GEOMS[label][2]
    run = _Runner(ops, _to_device(label, case, gpu), dg)
    bound = ops.amax(run.dev[0])
    y32, ys, yp, y7 = run.fp32(), run.split(bound), run.packed(bound), run.halo7()
    again = run.fp32(), run.split(bound), run.packed(bound)
    e32, es, ep = _rel(y32, ref), _rel(ys, ref), _rel(yp, ref)
    d7 = (y32 - y7).abs().max().item() / ref.abs().max().item()
    print(f'\n[tapwin-edges] {label} {field}: rel err vs fp64 oracle  fp32 {e32:.3e}  split {es:.3e}  packed {ep:.3e}  |tapwin - R7| / max|ref| {d7:.3e}')
    assert e32 < FWD_RTOL and es < FWD_RTOL and ep < FWD_RTOL, (e32, es, ep)
    assert es < 1.5 * e32 + 2e-7 and ep < 1.5 * e32 + 2e-7, (es, ep, e32)
    assert torch.equal(ys, yp)
    assert d7 <= 2e-5, d7
    for a, b_ in zip((y32, ys, yp), again):
        assert torch.equal(a, b_)


@pytest.mark.parametrize('label', ['B', 'E'])
def test_sigmoid_epilogue_of_the_three_forward_kernels(gpu, label):
    """act = ACT_SIGMOID through dcn_fused (R = 7), dcn_tapwin and dcn_tapwin_s.  The bound is derived:  0.25 (the sigmoid's largest
    slope) x the pre-activation tolerance FWD_RTOL x max|ref|,  plus 1e-6 = 16 fp32 ulp at 1.0 for v_exp_f32 and v_rcp_f32 (about 1 ulp
    each) and the roundings around them."""
    from edvr_amd import ops
    case = _case(label, 'ladder')
    ref, dg = case[5], U.EDGE_GEOMS[label][2]
    run = _Runner(ops, _to_device(label, case, gpu), dg)
    bound = ops.amax(run.dev[0])
    want, tol = torch.sigmoid(ref), 0.25 * FWD_RTOL * ref.abs().max().item() + 1e-6
    S = ops.ACT_SIGMOID
    for name, y in (('fused R7', run.halo7(S)), ('tapwin fp32', run.fp32(S)), ('tapwin split', run.split(bound, S)), ('tapwin split packed', run.packed(bound, S))):
        err = (y.double().cpu() - want).abs().max().item()
        print(f'\n[tapwin-edges] {label} sigmoid {name}: max abs err {err:.3e} (bound {tol:.3e})')
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize('label', ['B', 'E'])
def test_split_kernel_with_masks_outside_the_unit_interval(gpu, label):
    """Masks uniform in [-2, 2): xm_bound's contract is  >= max|x| * max(1, max|mask|)  - amax(x) * 2 here, and a bound loose by a
    further factor of 1024 (the looseness the DCN dW test uses) is a bound too."""
    from edvr_amd import ops
    case = _case(label, 'ladder', mask='signed')
    ref, dg = case[5], U.EDGE_GEOMS[label][2]
    assert case[2].min().item() < -1.5 and case[2].max().item() > 1.5 and case[2].abs().max().item() <= 2.
    run = _Runner(ops, _to_device(label, case, gpu), dg)
    e32 = _rel(run.fp32(), ref)
    tight = ops.amax(run.dev[0]) * 2
    ys = run.split(tight)
    assert torch.equal(ys, run.packed(tight))
    for name, y in (('x 2', ys), ('x 2048', run.split(tight * 1024))):
        es = _rel(y, ref)
        print(f'\n[tapwin-edges] {label} signed masks, bound amax(x) {name}: rel err split {es:.3e}  fp32 {e32:.3e}')
        assert torch.isfinite(y).all() and e32 < FWD_RTOL and es < FWD_RTOL and es < 1.5 * e32 + 2e-7, (name, es, e32)


def test_no_bias_with_a_ragged_output_channel_tail(gpu):
    """bias = None together with Co = 72 (an MT = 3 launch whose last channel tile holds 8 live rows) on the fp32 and the split form."""
    from edvr_amd import ops
    case = _case('B', 'ladder', bias=False)
    ref, dg = case[5], U.EDGE_GEOMS['B'][2]
    assert case[4] is None and U.EDGE_GEOMS['B'][3] == 72
    run = _Runner(ops, _to_device('B', case, gpu), dg)
    bound = ops.amax(run.dev[0])
    y32, ys, yp = run.fp32(), run.split(bound), run.packed(bound)
    e32, es = _rel(y32, ref), _rel(ys, ref)
    print(f'\n[tapwin-edges] B no bias: rel err fp32 {e32:.3e}  split {es:.3e}')
    assert e32 < FWD_RTOL and es < FWD_RTOL and es < 1.5 * e32 + 2e-7, (e32, es)
    assert torch.equal(ys, yp)
