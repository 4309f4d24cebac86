"""-m gpu: the small kernels that carry the training step around the convolutions - csrc/backward.hip and the forward /
activation-gradient kernels of csrc/elementwise.hip that feed it - one kernel at a time through its edvr_amd.ops wrapper against
the explicit fp64 references of tests/util_glue.py (pinned to torch autograd by tests/test_glue_refs_cpu.py): ties of the max
pooling, clipped windows, saturated sigmoids, the delicate point of the Charbonnier gradient, the channel-loop remainders of the
TSA gradient, the residual recovery of the activation gradient, and the SECOND trip of every grid-stride loop (the launches are
capped at 4096 blocks of 256 threads; the training shapes are far above that, the rest of the suite never is).

Tolerances, relative to max|ref| as in tests/test_gpu_glue.py: 2e-6 for pure fp32 elementwise work, 1e-5 where a sigmoid or the
Charbonnier sum is involved, 1e-4 for the TSA temporal gradients; exact where the kernel only moves data or every value is an
integer."""
import ctypes
import math
import types

import pytest
import torch

import util_glue as R
from util_glue import rel

pytestmark = pytest.mark.gpu
TOL, TOL_SIG, TOL_TSA = 2e-6, 1e-5, 1e-4
U = 2.0 ** -24  # unit roundoff of fp32
CAP = 4096 * 256  # work items of one trip through a grid-stride loop (grid_for)
PLANES = [(11, 8), (9, 7), (1, 1), (1, 6), (7, 1), (2, 2), (16, 16)]
TSA_SHAPES = [(1, 1, 1, 1, 1), (2, 16, 13, 5, 7), (1, 3, 9, 6, 9), (1, 5, 8, 4, 4), (2, 7, 30, 9, 20)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _act_code(act):
    from edvr_amd import ops
    return {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'lrelu': ops.ACT_LRELU, 'sigmoid': ops.ACT_SIGMOID}[act]


def _second_trip(items):
    """The case reaches the second trip of the loop (and only that one), and its last block is a partial one."""
    assert CAP < items <= 2 * CAP and items % 256 != 0, items


# ------------------------------------------------------------------------------------------ 1. pure data movement
@pytest.mark.parametrize('case', [(16, 12, 8, 6), (15, 11, 8, 6), (1, 1, 1, 1), (2, 5, 1, 3), (7, 2, 4, 1)])
def test_zero_stuff2(gpu, case):
    from edvr_amd import ops
    H, W, ho, wo = case
    dz = torch.randn(2, 3, ho, wo, generator=_gen(40))
    assert torch.equal(ops.zero_stuff2(dz.to(gpu), H, W).cpu(), R.zero_stuff2_ref(dz, H, W))


@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (2, 3, 10, 14), (1, 2, 6, 2)])
def test_pixel_unshuffle2(gpu, shape):
    from edvr_amd import ops
    x = torch.randn(shape, generator=_gen(41))
    assert torch.equal(ops.pixel_unshuffle2(x.to(gpu)).cpu(), R.pixel_unshuffle2_ref(x))


# ------------------------------------------------------------------------------------------ 2. frame_reduce_add_
def _check_frame_reduce(gpu, b, t, center, chw, seed=42):
    from edvr_amd import ops
    g = _gen(seed)
    src, dst = torch.randn(b * t, *chw, generator=g), torch.randn(b * t, *chw, generator=g)
    ref, mag = R.frame_reduce_ref(src, dst, t, center)
    got = ops.frame_reduce_add_(src.to(gpu), dst.to(gpu), t, center).cpu().view(b, t, *chw)
    err = (got[:, center].double() - ref).abs()
    worst = (err / mag.clamp_min(1e-30)).max().item() / U
    print(f'frame_reduce_add_ b={b} t={t} center={center} chw={chw}: max error {worst:.2f} of the allowed {t + 1} roundings')
    assert (err <= (t + 1) * U * mag).all()  # one rounding per addition: t - 1 in the sum, one into dst
    others = [k for k in range(t) if k != center]
    assert torch.equal(got[:, others], dst.view(b, t, *chw)[:, others])  # bit-identical: the other frames are not touched


@pytest.mark.parametrize('chw', [(1, 1, 1), (1, 5, 7), (4, 9, 20)])
@pytest.mark.parametrize('b', [1, 3])
@pytest.mark.parametrize('t', [1, 3, 7, 16])
def test_frame_reduce_add(gpu, t, b, chw):
    for center in sorted({0, t // 2, t - 1}):
        _check_frame_reduce(gpu, b, t, center, chw)


# ------------------------------------------------------------------------------------------ 3. pooling
@pytest.mark.parametrize('hw', PLANES)
def test_pool_maxavg_backward_ties(gpu, hw):
    """Integer-valued x from {0, 1, 2} (most windows tied), integer gradient on the max half, none on the avg half: the gradient of
    a window goes to its FIRST maximum in row-major order, and the result is exact."""
    from edvr_amd import ops
    x = R.tied_planes(*hw)
    dy = torch.randint(-3, 4, (2, 6, R.pool_out(hw[0]), R.pool_out(hw[1])), generator=_gen(43)).float()
    dy[:, 3:] = 0
    got = ops.pool_maxavg_backward(x.to(gpu), dy.to(gpu)).cpu()
    assert torch.equal(got.double(), R.pool_maxavg_bwd_ref(x, dy))


@pytest.mark.parametrize('hw', PLANES)
def test_pool_maxavg_backward_avg_half_and_both(gpu, hw):
    from edvr_amd import ops
    g = _gen(44)
    dy = torch.randn(2, 6, R.pool_out(hw[0]), R.pool_out(hw[1]), generator=g)
    avg_only = dy.clone()
    avg_only[:, :3] = 0
    x = R.tied_planes(*hw)  # (the avg half must not care where the maxima are)
    e_avg = rel(ops.pool_maxavg_backward(x.to(gpu), avg_only.to(gpu)), R.pool_maxavg_bwd_ref(x, avg_only))
    x = torch.randn(2, 3, *hw, generator=g)
    e_both = rel(ops.pool_maxavg_backward(x.to(gpu), dy.to(gpu)), R.pool_maxavg_bwd_ref(x, dy))
    print(f'pool_maxavg_backward {hw}: avg half {e_avg:.2e}, both halves {e_both:.2e}')
    assert e_avg < TOL and e_both < TOL


@pytest.mark.parametrize('hw', PLANES)
def test_pool_maxavg_forward(gpu, hw):
    from edvr_amd import ops
    for x in (R.tied_planes(*hw), torch.randn(2, 3, *hw, generator=_gen(45))):
        ref = R.pool_maxavg_ref(x)
        got = ops.pool_maxavg(x.to(gpu)).cpu()
        assert torch.equal(got[:, :3].double(), ref[:, :3])
        assert rel(got[:, 3:], ref[:, 3:]) < TOL


# ------------------------------------------------------------------------------------------ 4. TSA combine, saturated sigmoids
def _saturating_attn(shape, g):
    """Random values mixed with 0, +-1, +-20, +-88 (exp(88) is the last finite power in fp32), +-90 and +-104 (it overflows)."""
    attn = torch.randn(shape, generator=g) * 3
    special = torch.tensor([0., 1, -1, 20, -20, 88, -88, 90, -90, 104, -104])
    flat = attn.view(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:flat.numel() // 3]
    flat[pos] = special[torch.arange(pos.numel()) % special.numel()]
    return attn


def _check_combine(gpu, shape, seed=46):
    from edvr_amd import ops
    g = _gen(seed)
    feat, add, dy = (torch.randn(shape, generator=g) for _ in range(3))
    attn = _saturating_attn(shape, g)
    y = ops.tsa_combine(feat.to(gpu), attn.to(gpu), add.to(gpu))
    dfeat, dattn = ops.tsa_combine_backward(feat.to(gpu), attn.to(gpu), dy.to(gpu))
    rf, ra = R.tsa_combine_bwd_ref(feat, attn, dy)
    for name, got, ref in (('y', y, R.tsa_combine_ref(feat, attn, add)), ('dfeat', dfeat, rf), ('dattn', dattn, ra)):
        assert torch.isfinite(got).all(), name
        e = rel(got, ref)
        print(f'tsa_combine {tuple(shape)} {name}: {e:.2e}')
        assert e < TOL_SIG, name


def test_tsa_combine_saturated(gpu):
    _check_combine(gpu, (2, 8, 6, 10))


# ------------------------------------------------------------------------------------------ 5. Charbonnier
def _charbonnier_inputs(n, seed, delicate=False):
    g = _gen(seed)
    p, t = torch.rand(n, generator=g), torch.rand(n, generator=g)
    if delicate:
        q = n // 4
        p[:q] = t[:q]  # d = 0 exactly
        t[q:2 * q] *= 1e-4  # (small targets: pred - target resolves differences of 1e-8)
        mag = 10.0 ** (-8 + 3 * torch.rand(q, generator=g))  # |d| in [1e-8, 1e-5], around sqrt(eps) = 1e-6
        p[q:2 * q] = t[q:2 * q] + mag * (torch.randint(0, 2, (q,), generator=g) * 2 - 1)
    return p, t


def _check_charbonnier(gpu, p, t, scale):
    from edvr_amd import ops
    rl, rg = R.charbonnier_ref(p, t, 1e-12, scale)
    loss, grad = ops.charbonnier(p.to(gpu), t.to(gpu), grad_scale=scale)
    e_loss, e_grad = abs(loss.item() - rl.item()) / rl.item(), rel(grad, rg)
    print(f'charbonnier n={p.numel()} scale={scale}: loss {e_loss:.2e}, gradient {e_grad:.2e}')
    assert e_loss < TOL_SIG
    assert torch.isfinite(grad).all() and e_grad < TOL_SIG
    assert (grad.cpu()[p == t] == 0).all()
    return loss


def test_charbonnier_grad_scale_and_scaled_loss(gpu):
    from edvr_amd.autograd import charbonnier_loss
    p, t = _charbonnier_inputs(2880, 47)
    p, t = p.view(2, 3, 20, 24), t.view(2, 3, 20, 24)
    _check_charbonnier(gpu, p, t, 0.37)
    rl, rg = R.charbonnier_ref(p, t, 1e-12, 0.37)
    pg = p.to(gpu).requires_grad_()
    loss = charbonnier_loss(pg, t.to(gpu))
    (0.37 * loss).backward()
    assert abs(loss.item() - rl.item()) / rl.item() < TOL_SIG
    assert rel(pg.grad, rg) < TOL_SIG


def test_charbonnier_without_gradient(gpu):
    from edvr_amd import ops
    p, t = _charbonnier_inputs(2880, 48)
    with_grad = _check_charbonnier(gpu, p, t, 1.0)
    loss, grad = ops.charbonnier(p.to(gpu), t.to(gpu), want_grad=False)
    assert grad is None
    rl, _ = R.charbonnier_ref(p, t)
    assert abs(loss.item() - rl.item()) / rl.item() < TOL_SIG
    # the same 12 block sums, added by atomics in an order that may differ between the two launches: 11 roundings each way
    assert abs(loss.item() - with_grad.item()) <= 2 * 11 * U * rl.item()


def test_charbonnier_at_zero_and_around_sqrt_eps(gpu):
    p, t = _charbonnier_inputs(2880, 49, delicate=True)
    d = (p.double() - t.double()).abs()[720:1440]
    assert (p[:720] == t[:720]).all() and d.min() > 5e-9 and d.max() < 2e-5 and (d < 1e-6).any() and (d > 1e-6).any()
    _check_charbonnier(gpu, p, t, 1.0)


def test_charbonnier_several_trips_per_thread(gpu):
    """The launch is capped at 1024 blocks: 2 * 262 144 + 77 elements give every thread 2 trips and 77 threads a third one."""
    p, t = _charbonnier_inputs(2 * 262144 + 77, 50, delicate=True)
    _check_charbonnier(gpu, p, t, 0.37)


# ------------------------------------------------------------------------------------------ 6. TSA temporal attention
def _tsa_inputs(shape, seed=51):
    b, t, c, h, w = shape
    g = _gen(seed)
    emb, al = torch.randn(shape, generator=g) * 0.3, torch.randn(shape, generator=g)
    er, dy = torch.randn(b, c, h, w, generator=g) * 0.3, torch.randn(shape, generator=g)
    return emb, er, al, dy


def _single_pass(gpu, emb, er, al, dy):
    """edvr_tsa_temporal_bwd_f32 without a workspace: the one-thread-per-(clip, pixel) kernel no wrapper launches."""
    from edvr_amd import _lib
    b, t, c, h, w = al.shape
    ins = [v.to(gpu).contiguous() for v in (emb, er, al, dy)]
    outs = [torch.empty_like(ins[0]), torch.empty_like(ins[1]), torch.empty_like(ins[2])]
    ptrs = [ctypes.c_void_p(v.data_ptr()) for v in ins + outs]
    rc = _lib.lib().edvr_tsa_temporal_bwd_f32(*ptrs, b, t, c, h * w, ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'edvr_tsa_temporal_bwd_f32')
    return outs


@pytest.mark.parametrize('shape', TSA_SHAPES)
def test_tsa_temporal_backward(gpu, shape):
    """Channel counts off the unroll factor of the two channel loops (1, 9, 13, 30), t = 1 and t = 16; both forms of the kernel."""
    from edvr_amd import ops
    emb, er, al, dy = _tsa_inputs(shape)
    refs = R.tsa_temporal_bwd_ref(emb, er, al, dy)
    two = ops.tsa_temporal_backward(emb.to(gpu), er.to(gpu), al.to(gpu), dy.to(gpu))
    one = _single_pass(gpu, emb, er, al, dy)
    same = all(torch.equal(a, b) for a, b in zip(one, two))
    for name, a, b, r in zip(('d_emb', 'd_emb_ref', 'd_aligned'), two, one, refs):
        e2, e1 = rel(a, r), rel(b, r)
        print(f'tsa_temporal_backward {shape} {name}: two-pass {e2:.2e}, single-pass {e1:.2e}')
        assert e2 < TOL_TSA and e1 < TOL_TSA, name
    print(f'tsa_temporal_backward {shape}: single-pass and two-pass results bit-identical: {same}')


def test_tsa_temporal_backward_refuses_17_frames(gpu):
    from edvr_amd import ops
    emb, er, al, dy = (v.to(gpu) for v in _tsa_inputs((1, 17, 2, 3, 3)))
    with pytest.raises(RuntimeError, match=r'tsa_temporal_bwd: bad arguments \(t <= 16\)'):
        ops.tsa_temporal_backward(emb, er, al, dy)


@pytest.mark.parametrize('shape', TSA_SHAPES)
def test_tsa_temporal_forward(gpu, shape):
    from edvr_amd import ops
    emb, er, al, _ = _tsa_inputs(shape)
    ro, rp = R.tsa_temporal_ref(emb, er, al)
    out, prob = ops.tsa_temporal(emb.to(gpu), er.to(gpu), al.to(gpu), want_prob=True)
    assert rel(out, ro) < TOL_SIG and rel(prob, rp) < TOL_SIG


# ------------------------------------------------------------------------------------------ 7. activation gradients
def _act_case(shape, act, nres, act_from, seed=52):
    """dy, the pre-activation z (|z| in [0.25, 2]: |act(z)| >= 0.025 is far above the ~1e-6 the residual round trip fl(a + r) - r
    can be off by, so the sign the kernel recovers is the true one), residuals with |r| <= 4 and y = act(z) + res1 + res2 in fp32
    as the forward's epilogue stores it (channels below act_from: no activation)."""
    g = _gen(seed)
    dy = torch.randn(shape, generator=g)
    z = (0.25 + 1.75 * torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    res = [torch.randn(shape, generator=g).mul_(1.7).clamp_(-4, 4) for _ in range(nres)]  # (not on a coarse binary grid: the sums round)
    y = torch.cat([z[:, :act_from], R.act_fwd(z[:, act_from:], act)], 1)
    for r in res:
        y = y + r
    return dy, z, res + [None] * (2 - nres), y


@pytest.mark.parametrize('act_from', [0, 5])
@pytest.mark.parametrize('nres', [0, 1, 2], ids=['plain', 'res1', 'res1+res2'])
@pytest.mark.parametrize('act', R.ACTS)
def test_act_backward(gpu, act, nres, act_from):
    """Every activation with no, one and two residuals to subtract first.  relu is the delicate one: its output 0 comes back from
    fl(fl(r1 + r2) - r1) - r2 as +-1e-7, and a gate that tests `> 0` opens for a third of the negative pre-activations."""
    from edvr_amd import ops
    dy, z, (r1, r2), y = _act_case((2, 8, 6, 10), act, nres, act_from)
    to = lambda v: v.to(gpu) if v is not None else None
    got = ops.act_backward(dy.to(gpu), y.to(gpu), _act_code(act), act_from=act_from, res1=to(r1), res2=to(r2))
    e = rel(got, R.act_bwd_ref(dy, z, act, act_from))
    print(f'act_backward {act} residuals={nres} act_from={act_from}: {e:.2e}')
    assert e < (TOL_SIG if act == 'sigmoid' else TOL)


def _check_fused_unshuffle(gpu, shape, act):
    from edvr_amd import ops
    dy, z, _, y = _act_case(shape, act, 0, 0, seed=53)
    ref = R.pixel_unshuffle2_ref(R.act_bwd_ref(dy, z, act))
    got = ops.pixel_unshuffle2_act_backward(dy.to(gpu), y.to(gpu), _act_code(act))
    assert rel(got, ref) < (TOL_SIG if act == 'sigmoid' else TOL)
    two = ops.pixel_unshuffle2(ops.act_backward(dy.to(gpu), y.to(gpu), _act_code(act)) if act != 'none' else dy.to(gpu))
    assert torch.equal(got, two)  # bit for bit the two-launch form


@pytest.mark.parametrize('shape', [(2, 3, 10, 14), (3, 1, 2, 2), (1, 1, 2, 6)])
@pytest.mark.parametrize('act', R.ACTS)
def test_pixel_unshuffle2_act_backward(gpu, act, shape):
    _check_fused_unshuffle(gpu, shape, act)


# ------------------------------------------------------------------------------------------ 8. the second trip of the loops
def test_second_trip_pixel_unshuffle2_1072764(gpu):
    from edvr_amd import ops
    x = torch.randn(1, 3, 2 * 297, 2 * 301, generator=_gen(60))
    _second_trip(x.numel())
    assert torch.equal(ops.pixel_unshuffle2(x.to(gpu)).cpu(), R.pixel_unshuffle2_ref(x))


@pytest.mark.parametrize('act', ['lrelu', 'sigmoid'])
def test_second_trip_pixel_unshuffle2_act_backward_1162161(gpu, act):
    shape = (1, 13, 2 * 297, 2 * 301)
    _second_trip(math.prod(shape) // 4)  # one work item per 2 x 2 block
    _check_fused_unshuffle(gpu, shape, act)


def test_second_trip_zero_stuff2_1162161(gpu):
    from edvr_amd import ops
    H, W = 297, 301
    dz = torch.randn(1, 13, (H + 1) // 2, (W + 1) // 2, generator=_gen(61))
    ref = R.zero_stuff2_ref(dz, H, W)
    _second_trip(ref.numel())  # one work item per element of the stuffed tensor
    assert torch.equal(ops.zero_stuff2(dz.to(gpu), H, W).cpu(), ref)


def test_second_trip_frame_reduce_add_1051587(gpu):
    b, chw = 3, (3, 331, 353)
    _second_trip(b * math.prod(chw))  # one work item per element of a clip's centre frame
    _check_frame_reduce(gpu, b, 3, 1, chw)


@pytest.mark.parametrize('case', [('generic', 12, 297, 301, 0, 1072764), ('generic', 12, 297, 302, 1, 1076328),
                                  ('wide', 26, 297, 302, 0, 1166022), ('wide', 26, 297, 300, 0, 1158300)],
                         ids=['generic-w301-1072764', 'generic-w302-unaligned-1076328', 'wide-w302-1166022', 'wide-w300-1158300'])
def test_second_trip_upsample2x_backward(gpu, case):
    """The generic kernel (odd width; even width behind a 4-byte aligned gradient) with one work item per input pixel, and the
    16-byte kernel with lane exchanges (one item per input pixel PAIR; an odd and an even number of pairs per row), whose last
    block of the second trip runs with inactive lanes that still take part in the exchanges."""
    from edvr_amd import ops
    kernel, nc, h, w, shift, items = case
    assert items == (nc * h * w if kernel == 'generic' else nc * h * w // 2)
    _second_trip(items)
    dy = torch.randn(1, nc, 2 * h, 2 * w, generator=_gen(62))
    flat = torch.zeros(dy.numel() + shift, device=gpu)
    flat[shift:] = dy.to(gpu).reshape(-1)
    dyg = flat[shift:].view(dy.shape)
    assert dyg.is_contiguous() and (dyg.data_ptr() % 16 == 0) == (shift == 0)
    e = rel(ops.upsample2x_backward(dyg, 1.5), R.upsample2x_bwd_ref(dy, 1.5))
    print(f'upsample2x_backward {case}: {e:.2e}')
    assert e < TOL


def test_second_trip_pool_maxavg_backward_1049488(gpu):
    """11 926 planes of 11 x 8, half of them with tied windows."""
    from edvr_amd import ops
    g = _gen(63)
    n, c, h, w = 2, 5963, 11, 8
    x = torch.cat([torch.randint(0, 3, (1, c, h, w), generator=g).float(), torch.randn(1, c, h, w, generator=g)])
    _second_trip(x.numel())
    dy = torch.randn(n, 2 * c, R.pool_out(h), R.pool_out(w), generator=g)
    assert rel(ops.pool_maxavg_backward(x.to(gpu), dy.to(gpu)), R.pool_maxavg_bwd_ref(x, dy)) < TOL
    dy = torch.randint(-3, 4, dy.shape, generator=g).float()
    dy[:, c:] = 0
    assert torch.equal(ops.pool_maxavg_backward(x.to(gpu), dy.to(gpu)).cpu().double(), R.pool_maxavg_bwd_ref(x, dy))


def test_second_trip_pool_maxavg_forward_1048824(gpu):
    from edvr_amd import ops
    g = _gen(64)
    n, c, h, w = 3, 14567, 11, 8
    x = torch.cat([torch.randint(0, 3, (1, c, h, w), generator=g).float(), torch.randn(2, c, h, w, generator=g)])
    ref, got = R.pool_maxavg_ref(x), ops.pool_maxavg(x.to(gpu)).cpu()
    _second_trip(ref.numel() // 2)  # one work item per window: a max and an avg output
    assert torch.equal(got[:, :c].double(), ref[:, :c]) and rel(got[:, c:], ref[:, c:]) < TOL


def test_second_trip_tsa_temporal_backward_frames1051242_refs1576863(gpu):
    """Both passes: one work item per (clip, frame, pixel), then one per (clip, channel, pixel)."""
    from edvr_amd import ops
    shape = b, t, c, h, w = (1, 2, 3, 723, 727)
    _second_trip(b * t * h * w)
    _second_trip(b * c * h * w)
    emb, er, al, dy = _tsa_inputs(shape, seed=65)
    got = ops.tsa_temporal_backward(emb.to(gpu), er.to(gpu), al.to(gpu), dy.to(gpu))
    for a, r in zip(got, R.tsa_temporal_bwd_ref(emb, er, al, dy)):
        assert rel(a, r) < TOL_TSA


@pytest.mark.parametrize('shape,items', [((1, 2, 3, 723, 727), 1051242), ((1, 3, 2, 700, 2004), 1052100)],
                         ids=['scalar-1051242', 'vec4-1052100'])
def test_second_trip_tsa_temporal_forward(gpu, shape, items):
    """One work item per (clip, frame, pixel) where h * w is no multiple of 4, per group of four pixels where it is."""
    from edvr_amd import ops
    b, t, c, h, w = shape
    assert items == (b * t * h * w // 4 if h * w % 4 == 0 else b * t * h * w)
    _second_trip(items)
    emb, er, al, _ = _tsa_inputs(shape, seed=66)
    ro, rp = R.tsa_temporal_ref(emb, er, al)
    out, prob = ops.tsa_temporal(emb.to(gpu), er.to(gpu), al.to(gpu), want_prob=True)
    assert rel(out, ro) < TOL_SIG and rel(prob, rp) < TOL_SIG


def test_second_trip_tsa_combine_forward_and_backward_1051587(gpu):
    shape = (3, 3, 331, 353)
    _second_trip(math.prod(shape))
    _check_combine(gpu, shape, seed=67)


def test_second_trip_add_1051587(gpu):
    from edvr_amd import ops
    g = _gen(68)
    a, b = torch.randn(3, 3, 331, 353, generator=g), torch.randn(3, 3, 331, 353, generator=g)
    _second_trip(a.numel())
    assert torch.equal(ops.add(a.to(gpu), b.to(gpu)).cpu(), a + b)  # one correctly rounded addition per element
    assert rel(ops.add(a.to(gpu), b.to(gpu)), a.double() + b.double()) < TOL


@pytest.mark.parametrize('act,nres,act_from', [('lrelu', 0, 0), ('sigmoid', 2, 1)], ids=['lrelu', 'sigmoid-res1+res2-from1'])
def test_second_trip_act_backward_1051587(gpu, act, nres, act_from):
    from edvr_amd import ops
    shape = (3, 3, 331, 353)
    dy, z, (r1, r2), y = _act_case(shape, act, nres, act_from, seed=69)
    _second_trip(dy.numel())
    to = lambda v: v.to(gpu) if v is not None else None
    got = ops.act_backward(dy.to(gpu), y.to(gpu), _act_code(act), act_from=act_from, res1=to(r1), res2=to(r2))
    e = rel(got, R.act_bwd_ref(dy, z, act, act_from))
    print(f'act_backward {act} {shape}: {e:.2e}')
    assert e < (TOL_SIG if act == 'sigmoid' else TOL)


@pytest.mark.parametrize('case', [('wide', 4, 297, 3540, 1051380), ('block', 24, 297, 302, 1076328), ('generic', 3, 297, 301, 1072764)],
                         ids=['wide-w3540-1051380', 'block-w302-1076328', 'generic-w301-1072764'])
def test_second_trip_upsample2x_forward(gpu, case):
    """The three x2 kernels: one work item per four input pixels of a row (w % 4 == 0), per two (even w), per OUTPUT pixel."""
    from edvr_amd import ops
    kernel, nc, h, w, items = case
    assert items == {'wide': nc * h * w // 4, 'block': nc * h * w // 2, 'generic': nc * h * w * 4}[kernel]
    _second_trip(items)
    x = torch.randn(1, nc, h, w, generator=_gen(70))
    assert rel(ops.upsample2x(x.to(gpu), 2.0), R.upsample2x_ref(x, 2.0)) < TOL


# ------------------------------------------------------------------------------------------ 9. autograd plumbing
def _upstream(shape, kind, g):
    """None: `out.sum().backward()` hands the Function an expanded (stride 0) gradient of ones.  'transposed': a gradient of the
    right shape whose last two axes are a transposed view - contiguous in shape only."""
    if kind == 'expanded':
        return None
    return torch.randn(*shape[:-2], shape[-1], shape[-2], generator=g).transpose(-1, -2)


def _backward(out, grad, device=None):
    if grad is None:
        out.sum().backward()
    else:
        grad = grad.transpose(-1, -2).contiguous().to(device).transpose(-1, -2) if device is not None else grad.double()
        assert device is None or not grad.is_contiguous() or grad.shape[-1] == 1 or grad.shape[-2] == 1
        out.backward(grad)


@pytest.mark.parametrize('kind', ['expanded', 'transposed'])
def test_autograd_functions_take_any_gradient_layout(gpu, kind):
    """The Functions of edvr_amd/autograd.py that wrap one of these kernels each (Upsample2x, PoolMaxAvg, TsaTemporal, TsaCombine,
    Add), through edvr_amd.functional, with upstream gradients that are not dense: the wrappers make them contiguous before a
    kernel reads them through a raw pointer.  ConvFn and DcnFromPackedFn: the two tests below."""
    from edvr_amd import functional as F_
    g = _gen(71)

    def run(fn_gpu, fn_ref, inputs, tol):
        leaves64 = [v.double().requires_grad_() for v in inputs]
        out64 = fn_ref(*leaves64)
        grad = _upstream(out64.shape, kind, g)
        _backward(out64, grad)
        leaves = [v.to(gpu).requires_grad_() for v in inputs]
        out = fn_gpu(*leaves)
        assert out.shape == out64.shape
        _backward(out, grad, gpu)
        for a, r in zip(leaves, leaves64):
            assert rel(a.grad, r.grad) < tol, fn_gpu.__name__

    run(lambda x: F_.upsample2x(x, 2.0), lambda x: R.upsample2x_ref(x, 2.0), [torch.randn(2, 5, 9, 7, generator=g)], TOL)
    run(lambda x: F_.upsample2x(x, 2.0), lambda x: R.upsample2x_ref(x, 2.0), [torch.randn(2, 5, 6, 8, generator=g)], TOL)
    run(F_.pool_maxavg, lambda x: torch.cat([torch.nn.functional.max_pool2d(x, 3, 2, 1), torch.nn.functional.avg_pool2d(x, 3, 2, 1)], 1),
        [torch.randn(2, 4, 11, 8, generator=g)], TOL)
    emb, er, al, _ = _tsa_inputs((2, 5, 9, 6, 9), seed=72)
    run(F_.tsa_temporal, lambda e, r, a: a * torch.sigmoid((e * r.unsqueeze(1)).sum(2)).unsqueeze(2), [emb, er, al], TOL_TSA)
    run(F_.tsa_combine, lambda f, a, d: f * torch.sigmoid(a) * 2 + d, [torch.randn(2, 6, 5, 7, generator=g) for _ in range(3)], TOL_SIG)
    run(F_.add, lambda a, b: a + b, [torch.randn(2, 6, 5, 7, generator=g) for _ in range(2)], TOL)


GRAD_RTOL = 5e-4  # conv / DCN gradients, fp32 against fp64, relative to max|ref grad| of each tensor (tests/test_gpu_train.py)
KINK_BAND = 1e-4  # a leaky-ReLU pre-activation below this may fall on the other side of 0 in fp32 (tests/test_gpu_train.py)

CONV_FN_CASES = {  # the four glue kernels of ConvFn.backward
    'sigmoid-from16-res1': dict(n=1, c1=16, co=24, h=8, w=12, act='sigmoid', act_from=16, res=True),  # act_backward, residual
    'stride2': dict(n=2, c1=32, co=32, h=15, w=11, stride=2),  # zero_stuff2 reads the upstream gradient itself
    'stride2-lrelu': dict(n=1, c1=32, co=32, h=16, w=12, stride=2, act='lrelu'),  # act_backward, then zero_stuff2
    'pixel-shuffle-lrelu': dict(n=1, c1=32, co=64, h=6, w=10, act='lrelu', shuffle=True),  # pixel_unshuffle2_act_backward
    'frame-map': dict(n=6, c1=32, c2=32, co=32, h=10, w=12, x2_map=(3, 3, 1)),  # frame_reduce_add_
}


def _fp32_parameters(m64):
    with torch.no_grad():
        for p in m64.parameters():
            p.copy_(p.float().double())


def _off_the_kink(pre, bias):
    """Nudge the bias of every channel that has a pre-activation inside KINK_BAND (there the fp32 forward and the fp64 reference may
    pick different sides of the leaky ReLU, and the comparison of gradients means nothing)."""
    with torch.no_grad():
        for _ in range(50):
            bias.copy_(bias.float().double())  # (the fp32 run gets the same parameters)
            ch = (pre().abs() < KINK_BAND).any(0).any(-1).any(-1)
            if not ch.any():
                return
            bias[ch] += 3.7e-3
    raise AssertionError('could not move the test inputs off the activation kink')


@pytest.mark.parametrize('kind', ['expanded', 'transposed'])
@pytest.mark.parametrize('name', list(CONV_FN_CASES))
def test_conv_function_takes_any_gradient_layout(gpu, name, kind):
    """ConvFn through functional.conv on a small nn.Conv2d against fp64 F.conv2d autograd: its backward hands the upstream gradient
    to act_backward, pixel_unshuffle2_act_backward, zero_stuff2 and (through the data gradient) frame_reduce_add_."""
    import torch.nn.functional as F
    from edvr_amd import functional as F_
    cfg = dict(dict(c2=0, stride=1, act='none', act_from=0, res=False, shuffle=False, x2_map=None), **CONV_FN_CASES[name])
    n, c1, c2, co, h, w, stride, act, af = (cfg[k] for k in ('n', 'c1', 'c2', 'co', 'h', 'w', 'stride', 'act', 'act_from'))
    torch.manual_seed(4321 + list(CONV_FN_CASES).index(name))  # nn.Conv2d's init draws from the global generator
    g = _gen(73)
    m64 = torch.nn.Conv2d(c1 + c2, co, 3, stride, 1).double()
    _fp32_parameters(m64)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    inputs = [torch.randn(n, c1, h, w, generator=g)] + ([torch.randn(n, c2, h, w, generator=g)] if c2 else [])
    inputs += [torch.randn(n, co, ho, wo, generator=g)] if cfg['res'] else []
    leaves64 = [v.double().requires_grad_() for v in inputs]

    def conv_input(x, x2):  # image i reads image (i // div) * mul + add of x2
        if x2 is None:
            return x
        div, mul, add = cfg['x2_map']
        return torch.cat([x, x2[[(i // div) * mul + add for i in range(n)]]], 1)

    x2_64 = leaves64[1] if c2 else None
    if act == 'lrelu':
        _off_the_kink(lambda: m64(conv_input(leaves64[0], x2_64)), m64.bias)
    y64 = m64(conv_input(leaves64[0], x2_64))
    stock = {'none': lambda v: v, 'lrelu': lambda v: F.leaky_relu(v, 0.1), 'sigmoid': torch.sigmoid}[act]
    y64 = torch.cat([y64[:, :af], stock(y64[:, af:])], 1)
    if cfg['res']:
        y64 = y64 + leaves64[-1]
    if cfg['shuffle']:
        y64 = F.pixel_shuffle(y64, 2)
    grad = _upstream(y64.shape, kind, g)
    _backward(y64, grad)

    m = torch.nn.Conv2d(c1 + c2, co, 3, stride, 1)
    m.load_state_dict({k: v.float() for k, v in m64.state_dict().items()})
    m = m.to(gpu)
    leaves = [v.to(gpu).requires_grad_() for v in inputs]
    out = F_.conv(m, leaves[0], x2=leaves[1] if c2 else None, x2_map=cfg['x2_map'], act=_act_code(act), act_from=af,
                  res1=leaves[-1] if cfg['res'] else None, out_mode=F_.OUT_PIXEL_SHUFFLE2 if cfg['shuffle'] else F_.OUT_NCHW)
    assert type(out.grad_fn).__name__.startswith('ConvFn') and rel(out.detach(), y64.detach()) < 2e-5
    _backward(out, grad, gpu)
    pairs = list(zip(leaves, leaves64)) + [(m.weight, m64.weight), (m.bias, m64.bias)]
    for i, (a, r) in enumerate(pairs):
        e = rel(a.grad, r.grad)
        print(f'ConvFn {name} {kind} gradient {i}: {e:.2e}')
        assert e < GRAD_RTOL, i
    if c2:  # only the frame the map reads receives a gradient
        others = [i for i in range(n) if i % 3 != 1]
        assert not leaves[1].grad[others].any() and leaves[1].grad[[1, 4]].any()


@pytest.mark.parametrize('kind', ['expanded', 'transposed'])
def test_dcn_function_takes_any_gradient_layout(gpu, kind):
    """DcnFromPackedFn (functional.dcn_from_packed) with a fused leaky ReLU: its backward starts with act_backward on the upstream
    gradient.  Against fp64 autograd of the floor / gather restatement of DCNv2 (oracle/dcn_oracle.py)."""
    import torch.nn.functional as F
    from edvr_amd import functional as F_
    from oracle import dcn_oracle as O
    g = _gen(74)
    n, c, h, w, dg = 1, 16, 8, 10, 2
    x = torch.randn(n, c, h, w, generator=g)
    om = torch.randn(n, 3 * dg * 9, h, w, generator=g)
    om[:, 2 * dg * 9:] = om[:, 2 * dg * 9:].sigmoid()
    wgt, bias = torch.randn(c, c, 3, 3, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1
    l64 = [v.double().requires_grad_() for v in (x, om, wgt, bias)]
    pre = lambda: O.dcnv2_torch(l64[0], l64[1][:, :2 * dg * 9], l64[1][:, 2 * dg * 9:], l64[2], l64[3], 1, 1, 1, 1, dg)
    _off_the_kink(pre, l64[3])
    y64 = F.leaky_relu(pre(), 0.1)
    grad = _upstream(y64.shape, kind, g)
    _backward(y64, grad)
    dev = [v.detach().float().to(gpu).requires_grad_() for v in l64]
    m = types.SimpleNamespace(weight=dev[2], bias=dev[3], kernel_size=(3, 3), stride=1, padding=1, dilation=1, groups=1, deformable_groups=dg)
    out = F_.dcn_from_packed(m, dev[0], dev[1], act=F_.ACT_LRELU)
    assert type(out.grad_fn).__name__.startswith('DcnFromPackedFn') and rel(out.detach(), y64.detach()) < 2e-5
    _backward(out, grad, gpu)
    for name, a, r in zip(('x', 'offsets and masks', 'weight', 'bias'), dev, l64):
        e = rel(a.grad, r.grad)
        print(f'DcnFromPackedFn {kind} gradient of {name}: {e:.2e}')
        assert e < GRAD_RTOL, name
