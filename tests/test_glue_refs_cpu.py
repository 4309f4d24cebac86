"""The explicit fp64 references of tests/util_glue.py against torch fp64 autograd of the stock operators (F.max_pool2d /
F.avg_pool2d, F.interpolate, F.pixel_shuffle, the formulas of oracle/edvr_oracle.py) at tiny shapes.  No GPU: this pins the
references the GPU tests of the glue kernels (tests/test_gpu_glue_bwd.py) are measured with."""
import pytest
import torch
import torch.nn.functional as F

import util_glue as R

PLANES = [(11, 8), (9, 7), (1, 1), (1, 6), (7, 1), (2, 2), (16, 16)]
EXACT = 1e-13  # both sides are fp64 evaluations of the same few operations


def _close(a, b, tol=EXACT):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def _stock_pool(x64):
    return torch.cat([F.max_pool2d(x64, 3, 2, 1), F.avg_pool2d(x64, 3, 2, 1)], 1)


@pytest.mark.parametrize('hw', PLANES)
def test_pool_backward_tie_rule_is_atens(hw):
    """ATen's max-pool backward sends the gradient of a tied window to its first maximum in row-major order: the explicit reference
    equals it EXACTLY on integer-valued inputs (everything is representable), max half alone and both halves."""
    x = R.tied_planes(*hw)
    g = torch.Generator().manual_seed(1)
    x64 = x.double().requires_grad_()
    y = _stock_pool(x64)
    assert torch.equal(R.pool_maxavg_ref(x)[:, :3], y[:, :3].detach())
    _close(R.pool_maxavg_ref(x), y.detach())
    dy = torch.randint(-3, 4, y.shape, generator=g).double()
    dy[:, 3:] = 0
    (gx,) = torch.autograd.grad(y, x64, dy, retain_graph=True)
    assert torch.equal(R.pool_maxavg_bwd_ref(x, dy), gx)
    dy = torch.randn(y.shape, generator=g).double()
    (gx,) = torch.autograd.grad(y, x64, dy)
    _close(R.pool_maxavg_bwd_ref(x, dy), gx)


def test_pool_tie_case_really_has_ties():
    """At least half of the windows of the 11 x 8 and 9 x 7 cases hold their maximum more than once - the tie tests cannot silently
    stop testing ties - and a tied window's argmax is the smallest flat index among its maxima."""
    for h, w in [(9, 7), (11, 8)]:
        x = R.tied_planes(h, w)
        arg, count = R.pool_argmax_first(x)
        assert (count > 1).double().mean().item() >= 0.5
        for oy in range(arg.shape[2]):
            for ox in range(arg.shape[3]):
                ys = [y for y in range(2 * oy - 1, 2 * oy + 2) if 0 <= y < h]
                xs = [v for v in range(2 * ox - 1, 2 * ox + 2) if 0 <= v < w]
                win = torch.stack([x[:, :, yy, xx] for yy in ys for xx in xs], -1)
                flat = torch.tensor([yy * w + xx for yy in ys for xx in xs])
                first = flat[(win == win.max(-1, keepdim=True).values).int().argmax(-1)]  # argmax of a 0/1 tensor: the first 1
                assert torch.equal(arg[:, :, oy, ox], first)


@pytest.mark.parametrize('hw', PLANES)
def test_pool_random_floats(hw):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, *hw, generator=g)
    x64 = x.double().requires_grad_()
    y = _stock_pool(x64)
    _close(R.pool_maxavg_ref(x), y.detach())
    dy = torch.randn(y.shape, generator=g)
    (gx,) = torch.autograd.grad(y, x64, dy.double())
    _close(R.pool_maxavg_bwd_ref(x, dy), gx)


@pytest.mark.parametrize('t,center', [(1, 0), (3, 1), (7, 6), (16, 0)])
def test_frame_reduce(t, center):
    """Gradient of a reference frame every frame of its clip read (x2_map): the sum over the clip lands on the centre frame."""
    g = torch.Generator().manual_seed(3)
    b, chw = 2, (2, 3, 5)
    src, dst = torch.randn(b * t, *chw, generator=g), torch.randn(b * t, *chw, generator=g)
    ref, mag = R.frame_reduce_ref(src, dst, t, center)
    frames = dst.double().view(b, t, *chw).clone().requires_grad_()
    idx = torch.full((t,), center)
    (frames[:, idx] * 1.0).backward(src.double().view(b, t, *chw))  # every frame reads frame `center`
    _close(ref, dst.double().view(b, t, *chw)[:, center] + frames.grad[:, center])
    assert torch.equal(frames.grad[:, [k for k in range(t) if k != center]], torch.zeros(b, t - 1, *chw, dtype=torch.float64))
    _close(mag, dst.double().view(b, t, *chw)[:, center].abs() + src.double().view(b, t, *chw).abs().sum(1))
    assert (mag >= ref.abs() - 1e-12).all()


@pytest.mark.parametrize('case', [(16, 12, 8, 6), (15, 11, 8, 6), (1, 1, 1, 1), (2, 5, 1, 3), (7, 2, 4, 1)])
def test_zero_stuff2_is_the_adjoint_of_a_stride2_slice(case):
    H, W, ho, wo = case
    dz = torch.randn(2, 3, ho, wo, generator=torch.Generator().manual_seed(4)).double()
    z = torch.zeros(2, 3, H, W, dtype=torch.float64, requires_grad=True)
    z[..., ::2, ::2].backward(dz)
    assert torch.equal(R.zero_stuff2_ref(dz, H, W), z.grad)


@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (2, 3, 10, 14), (1, 2, 6, 2), (1, 1, 2, 6)])
def test_pixel_unshuffle2(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).double()
    assert torch.equal(R.pixel_unshuffle2_ref(x), F.pixel_unshuffle(x, 2))
    n, c, h2, w2 = shape
    z = torch.zeros(n, 4 * c, h2 // 2, w2 // 2, dtype=torch.float64, requires_grad=True)
    F.pixel_shuffle(z, 2).backward(x)
    assert torch.equal(R.pixel_unshuffle2_ref(x), z.grad)


@pytest.mark.parametrize('hw', [(8, 8), (5, 3), (1, 1), (1, 2), (2, 6), (3, 130), (7, 9)])
def test_upsample2x(hw):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, *hw, generator=g).double().requires_grad_()
    y = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False) * 1.5
    _close(R.upsample2x_ref(x.detach(), 1.5), y.detach())
    dy = torch.randn(y.shape, generator=g).double()
    y.backward(dy)
    _close(R.upsample2x_bwd_ref(dy, 1.5), x.grad)


@pytest.mark.parametrize('shape', [(1, 1, 1, 1, 1), (2, 16, 13, 5, 7), (1, 3, 9, 6, 9), (1, 5, 8, 4, 4)])
def test_tsa_temporal(shape):
    """edvr_oracle.tsa_fusion: prob = sigmoid((emb * emb_ref.unsqueeze(1)).sum(2)), al = aligned * prob.unsqueeze(2)."""
    b, t, c, h, w = shape
    g = torch.Generator().manual_seed(7)
    emb, al, er = torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(b, c, h, w, generator=g)
    leaves = [v.double().requires_grad_() for v in (emb, er, al)]
    prob = torch.sigmoid((leaves[0] * leaves[1].unsqueeze(1)).sum(2))
    out = leaves[2] * prob.unsqueeze(2)
    dy = torch.randn(shape, generator=g)
    out.backward(dy.double())
    ro, rp = R.tsa_temporal_ref(emb, er, al)
    _close(ro, out.detach())
    _close(rp, prob.detach())
    for got, leaf in zip(R.tsa_temporal_bwd_ref(emb, er, al, dy), leaves):
        _close(got, leaf.grad)


def test_tsa_combine_with_saturated_attention():
    """edvr_oracle.tsa_fusion: feat * sigmoid(attn) * 2 + attn_add, also where the sigmoid is saturated."""
    g = torch.Generator().manual_seed(8)
    f, a, add, dy = (torch.randn(2, 4, 5, 7, generator=g) for _ in range(4))
    a.view(-1)[:13] = torch.tensor([0., 1, -1, 20, -20, 88, -88, 90, -90, 104, -104, 30, -30])
    leaves = [v.double().requires_grad_() for v in (f, a, add)]
    y = leaves[0] * torch.sigmoid(leaves[1]) * 2 + leaves[2]
    y.backward(dy.double())
    _close(R.tsa_combine_ref(f, a, add), y.detach())
    df, da = R.tsa_combine_bwd_ref(f, a, dy)
    _close(df, leaves[0].grad)
    _close(da, leaves[1].grad)
    assert torch.equal(leaves[2].grad, dy.double())
    assert torch.isfinite(df).all() and torch.isfinite(da).all()


@pytest.mark.parametrize('scale', [1.0, 0.37])
def test_charbonnier(scale):
    from oracle import edvr_oracle as EO
    g = torch.Generator().manual_seed(9)
    p, t = torch.rand(2, 3, 5, 8, generator=g), torch.rand(2, 3, 5, 8, generator=g)
    p.view(-1)[:40] = t.view(-1)[:40]  # d = 0: gradient exactly 0
    p.view(-1)[40:60] = t.view(-1)[40:60] + 1e-6  # |d| ~ sqrt(eps)
    p64 = p.double().requires_grad_()
    loss = EO.charbonnier_sum(p64, t.double())
    (scale * loss).backward()
    rl, rg = R.charbonnier_ref(p, t, 1e-12, scale)
    _close(rl, loss.detach())
    _close(rg, p64.grad, 1e-12)
    assert torch.equal(rg.view(-1)[:40], torch.zeros(40, dtype=torch.float64))


@pytest.mark.parametrize('act', R.ACTS)
@pytest.mark.parametrize('act_from', [0, 2])
def test_activation_gates(act, act_from):
    """The conv epilogue's activations (channels >= act_from) and their gates against autograd of the stock functions."""
    g = torch.Generator().manual_seed(10)
    z = torch.randn(2, 5, 4, 6, generator=g).double().requires_grad_()
    stock = {'none': lambda v: v, 'relu': torch.relu, 'lrelu': lambda v: F.leaky_relu(v, 0.1), 'sigmoid': torch.sigmoid}[act]
    y = torch.cat([z[:, :act_from], stock(z[:, act_from:])], 1)
    _close(R.act_fwd(z.detach(), act)[:, act_from:], y.detach()[:, act_from:])
    dy = torch.randn(z.shape, generator=g)
    y.backward(dy.double())
    _close(R.act_bwd_ref(dy, z.detach(), act, act_from), z.grad)
