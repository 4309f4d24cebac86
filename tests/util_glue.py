"""Explicit fp64 references of the training glue kernels (csrc/backward.hip and the forward / activation-gradient kernels of
csrc/elementwise.hip that feed it).  Every function is a plain loop over windows / taps or a closed-form index expression, written
from the comments of the kernels and NOT through torch autograd or the stock ATen operators: tests/test_glue_refs_cpu.py checks
each of them against fp64 autograd of the stock op, tests/test_gpu_glue_bwd.py compares the kernels with them.

Loops run over the window / tap positions of ONE plane and are vectorised over the (n, c) planes, so that a case with more than
a million work items (many small planes) still takes well under a second."""
import math

import torch

ACTS = ('none', 'relu', 'lrelu', 'sigmoid')


def rel(a, ref):
    """max|a - ref| relative to max|ref| (the project's measure, tests/test_gpu_glue.py)."""
    return ((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def sigmoid64(v):
    return 1.0 / (1.0 + torch.exp(-v.double()))


# ---------------------------------------------------------------------------------------------- pooling 3x3 / stride 2 / pad 1
def pool_out(n):
    return (n - 1) // 2 + 1


def _window(o, n):
    return [i for i in range(2 * o - 1, 2 * o + 2) if 0 <= i < n]


def tied_planes(h, w, n=2, c=3):
    """Integer-valued x from {0, 1, 2}: most 3x3 windows hold their maximum more than once."""
    return torch.randint(0, 3, (n, c, h, w), generator=torch.Generator().manual_seed(100)).float()


def pool_maxavg_ref(x):
    """cat(max over the window's in-range elements, (sum of them) / 9): count_include_pad, padding never wins the maximum."""
    x = x.double()
    n, c, h, w = x.shape
    ho, wo = pool_out(h), pool_out(w)
    y = torch.zeros(n, 2 * c, ho, wo, dtype=torch.float64)
    for oy in range(ho):
        for ox in range(wo):
            best = torch.full((n, c), -math.inf, dtype=torch.float64)
            total = torch.zeros(n, c, dtype=torch.float64)
            for yy in _window(oy, h):
                for xx in _window(ox, w):
                    v = x[:, :, yy, xx]
                    best = torch.where(v > best, v, best)
                    total = total + v
            y[:, :c, oy, ox] = best
            y[:, c:, oy, ox] = total / 9.0
    return y


def pool_argmax_first(x):
    """(n, c, ho, wo) flat index yy * w + xx of the FIRST maximum of every window in row-major order, and the number of window
    elements equal to that maximum (> 1: the window is tied)."""
    x = x.double()
    n, c, h, w = x.shape
    ho, wo = pool_out(h), pool_out(w)
    arg = torch.full((n, c, ho, wo), -1, dtype=torch.int64)
    count = torch.zeros(n, c, ho, wo, dtype=torch.int64)
    for oy in range(ho):
        for ox in range(wo):
            best = torch.full((n, c), -math.inf, dtype=torch.float64)
            a = torch.full((n, c), -1, dtype=torch.int64)
            for yy in _window(oy, h):  # row-major walk; only a strictly larger value replaces the maximum found so far
                for xx in _window(ox, w):
                    v = x[:, :, yy, xx]
                    take = (v > best) | (a < 0)
                    best = torch.where(take, v, best)
                    a = torch.where(take, torch.full_like(a, yy * w + xx), a)
            arg[:, :, oy, ox] = a
            for yy in _window(oy, h):
                for xx in _window(ox, w):
                    count[:, :, oy, ox] += (x[:, :, yy, xx] == best).long()
    return arg, count


def pool_maxavg_bwd_ref(x, dy):
    """dx of y = cat(maxpool(x), avgpool(x)): every in-range element of a window receives gavg / 9, the first maximum in row-major
    order receives gmax."""
    x, dy = x.double(), dy.double()
    n, c, h, w = x.shape
    ho, wo = pool_out(h), pool_out(w)
    gmax, gavg = dy[:, :c], dy[:, c:]
    arg, _ = pool_argmax_first(x)
    dx = torch.zeros(n, c, h * w, dtype=torch.float64)
    for oy in range(ho):
        for ox in range(wo):
            dx.scatter_add_(2, arg[:, :, oy, ox].unsqueeze(2), gmax[:, :, oy, ox].unsqueeze(2))
            for yy in _window(oy, h):
                for xx in _window(ox, w):
                    dx[:, :, yy * w + xx] += gavg[:, :, oy, ox] / 9.0
    return dx.view(n, c, h, w)


# ---------------------------------------------------------------------------------------------- data movement
def frame_reduce_ref(src, dst, t, center):
    """(dst[b, center] + sum_t src[b, t], |dst[b, center]| + sum_t |src[b, t]|) as (b, c, h, w) fp64 tensors, for (b * t, c, h, w)
    inputs; the second one scales the rounding-error bound of the fp32 kernel."""
    s = src.double().view(-1, t, *src.shape[1:])
    d = dst.double().view(-1, t, *dst.shape[1:])[:, center]
    return d + s.sum(1), d.abs() + s.abs().sum(1)


def zero_stuff2_ref(dz, H, W):
    """z (n, c, H, W) with z[2 oy, 2 ox] = dz[oy, ox] and zero elsewhere."""
    n, c, ho, wo = dz.shape
    z = torch.zeros(n, c, H, W, dtype=dz.dtype)
    z[..., ::2, ::2][..., :ho, :wo] = dz
    return z


def pixel_unshuffle2_ref(x):
    """y[n, 4 oc + 2 sy + sx, oy, ox] = x[n, oc, 2 oy + sy, 2 ox + sx]."""
    n, c, h2, w2 = x.shape
    h, w = h2 // 2, w2 // 2
    return x.reshape(n, c, h, 2, w, 2).permute(0, 1, 3, 5, 2, 4).reshape(n, 4 * c, h, w)


# ---------------------------------------------------------------------------------------------- bilinear x2, align_corners=False
def bilinear2_matrix(n):
    """(2n, n) fp64 matrix of one axis: output o reads s = max((o + 0.5) / 2 - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, n - 1)."""
    m = torch.zeros(2 * n, n, dtype=torch.float64)
    for o in range(2 * n):
        s = max((o + 0.5) * 0.5 - 0.5, 0.0)
        i0 = int(s)
        i1 = min(i0 + 1, n - 1)
        m[o, i0] += 1.0 - (s - i0)
        m[o, i1] += s - i0
    return m


def upsample2x_ref(x, scale=1.0):
    my, mx = bilinear2_matrix(x.shape[-2]), bilinear2_matrix(x.shape[-1])
    return scale * torch.einsum('oh,nchw,pw->ncop', my, x.double(), mx)


def upsample2x_bwd_ref(dy, scale=1.0):
    """Adjoint of upsample2x_ref."""
    my, mx = bilinear2_matrix(dy.shape[-2] // 2), bilinear2_matrix(dy.shape[-1] // 2)
    return scale * torch.einsum('oh,ncop,pw->nchw', my, dy.double(), mx)


# ---------------------------------------------------------------------------------------------- TSA
def tsa_temporal_ref(emb, emb_ref, aligned):
    """(aligned * p, p), p[b, t] = sigmoid(<emb[b, t], emb_ref[b]> over channels)."""
    prob = sigmoid64((emb.double() * emb_ref.double().unsqueeze(1)).sum(2))
    return aligned.double() * prob.unsqueeze(2), prob


def tsa_temporal_bwd_ref(emb, emb_ref, aligned, dout):
    """d_aligned = dout * p, ds = <dout, aligned> p (1 - p), d_emb = ds * emb_ref, d_emb_ref = sum_t ds[t] * emb[t]."""
    emb, emb_ref, aligned, dout = emb.double(), emb_ref.double(), aligned.double(), dout.double()
    _, prob = tsa_temporal_ref(emb, emb_ref, aligned)
    ds = ((dout * aligned).sum(2) * prob * (1.0 - prob)).unsqueeze(2)  # (b, t, 1, h, w)
    return ds * emb_ref.unsqueeze(1), (ds * emb).sum(1), dout * prob.unsqueeze(2)


def tsa_combine_ref(feat, attn, attn_add):
    return feat.double() * sigmoid64(attn) * 2.0 + attn_add.double()


def tsa_combine_bwd_ref(feat, attn, dy):
    """(dfeat, dattn) of y = feat * s * 2 + add, s = sigmoid(attn); dadd = dy."""
    s = sigmoid64(attn)
    return dy.double() * s * 2.0, dy.double() * feat.double() * 2.0 * s * (1.0 - s)


# ---------------------------------------------------------------------------------------------- Charbonnier (reduction = sum)
def charbonnier_ref(pred, target, eps=1e-12, grad_scale=1.0):
    """(sum sqrt(d^2 + eps), grad_scale * d / sqrt(d^2 + eps)), d = pred - target."""
    d = pred.double() - target.double()
    r = torch.sqrt(d * d + eps)
    return r.sum(), grad_scale * d / r


# ---------------------------------------------------------------------------------------------- epilogue activations
def act_fwd(z, act):
    """The conv epilogue's activation in the dtype of z (fp32 input: what the forward stored)."""
    if act == 'relu':
        return torch.clamp_min(z, 0.0)
    if act == 'lrelu':
        return torch.where(z > 0, z, 0.1 * z)
    if act == 'sigmoid':
        return 1.0 / (1.0 + torch.exp(-z))
    return z


def act_gate(z, act):
    """act'(z) in fp64 from the pre-activation."""
    z = z.double()
    if act == 'relu':
        return (z > 0).double()
    if act == 'lrelu':
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.1))
    if act == 'sigmoid':
        s = sigmoid64(z)
        return s * (1.0 - s)
    return torch.ones_like(z)


def act_bwd_ref(dy, z, act, act_from=0):
    """dz = dy * act'(z) on channels >= act_from, dy below."""
    gate = act_gate(z, act)
    gate[:, :act_from] = 1.0
    return dy.double() * gate
