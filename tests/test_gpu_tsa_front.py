"""-m gpu: ops.tsa_front (csrc/tsa_front_s.hip) - TSA fusion's temporal attention and its two 1x1 heads in one kernel that never stores
the modulated features.  Contract: bit for bit what the three launches give (tsa_temporal + two conv2d calls on conv1x1_split_kernel),
y_amax slots included, and the fp64 formula to the tolerance of the 1x1 split tests (tests/test_gpu_conv_f4s.py: 2e-6 of max |ref|).

The streaming split kernel only takes convs from 320 input channels up, so for the narrow cases the three-launch arm runs it on the
same operand padded with ZERO channels (and zero weight columns) to 320: the padded k-steps add +-0 to sums that are never -0 (they
start from +0), the weight scale comes from the same max |w| and the input scale from the same explicit bound - the same bits."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL = 2e-6  # test_split_conv1x1_matches_fp64's bound, relative to max |ref|
FUSED = 'tsa_front_split_kernel'

# (b, t, c, h, w, co, centre or None)
SHAPES = {
    'one_kstep_per_frame': (1, 3, 8, 4, 8, 32, None),       # one k-step per frame, one partial pixel block
    'c64_hw180': (2, 5, 64, 9, 20, 64, None),               # 320 channels; hw = 180: neither a multiple of 128 pixels nor of 32
    'slab_straddles_frame': (1, 5, 72, 8, 36, 72, None),    # 64- and 32-channel weight slabs straddle frame boundaries; co no multiple of 32
    't7_width': (1, 7, 128, 12, 32, 128, None),             # the T7 width: 896 channels
    'odd_hw': (2, 5, 64, 5, 7, 64, None),                   # hw = 35: no 16-byte rows - the attention pass on 4-byte loads
    'ref_view_first': (2, 5, 16, 4, 8, 32, 0),              # emb_ref = a strided view (frame 0 / frame t - 1 of a (b, t, c, h, w) tensor)
    'ref_view_last': (2, 5, 16, 4, 8, 32, 4),
}
_CACHE = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _inputs(name, gpu):
    """Operands of a case (made once, shared, never modified) and the fp64 formula's results."""
    if name in _CACHE:
        return _CACHE[name]
    b, t, c, h, w, co, ctr = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    emb = torch.randn(b, t, c, h, w, generator=g) * 0.3
    refs = torch.randn(b, t if ctr is not None else 1, c, h, w, generator=g) * 0.3
    aligned = torch.randn(b, t, c, h, w, generator=g)
    wf, wa = torch.randn(co, t * c, 1, 1, generator=g) * 0.05, torch.randn(co, t * c, 1, 1, generator=g) * 0.05
    bf, ba = torch.randn(co, generator=g), torch.randn(co, generator=g)
    ref_frame = refs[:, ctr if ctr is not None else 0]
    prob = torch.sigmoid((emb.double() * ref_frame.double().unsqueeze(1)).sum(2, keepdim=True))
    mod = (aligned.double() * prob).view(b, t * c, h, w)
    want = tuple(F.leaky_relu(F.conv2d(mod, wt.double(), bs.double()), 0.1) for wt, bs in ((wf, bf), (wa, ba)))
    refs_g = refs.to(gpu)
    d = dict(emb=emb.to(gpu), emb_ref=refs_g[:, ctr] if ctr is not None else refs_g[:, 0].contiguous(), aligned=aligned.to(gpu),
             wf=wf.to(gpu), wa=wa.to(gpu), bf=bf.to(gpu), ba=ba.to(gpu), want=want, co=co, refs=refs_g)
    if ctr is not None:
        assert not d['emb_ref'].is_contiguous() or b == 1
    _CACHE[name] = d
    return d


def _hooked(ops, fn):
    seen = []
    ops.LAUNCH_HOOK = lambda name, flops, launch, *a: (seen.append(name), launch())
    try:
        out = fn()
    finally:
        ops.LAUNCH_HOOK = None
    return out, seen


def _three_launches(ops, emb, emb_ref, aligned, wf, bf, wa, ba, co, bound):
    """tsa_temporal + two convs on conv1x1_split_kernel -> (feat, attn, feat's y_amax, attn's y_amax)."""
    b, t, c, h, w = aligned.shape
    ci, cip = t * c, max(t * c, 320)
    mod = ops.tsa_temporal(emb, emb_ref, aligned).view(b, ci, h, w)
    if cip > ci:
        mod = torch.cat([mod, torch.zeros(b, cip - ci, h, w, device=mod.device)], 1)
    outs = []
    for wt, bs in ((wf, bf), (wa, ba)):
        wp = torch.cat([wt, torch.zeros(co, cip - ci, 1, 1, device=wt.device)], 1) if cip > ci else wt
        (y, seen) = _hooked(ops, lambda: ops.conv2d(mod, ops.pack_conv_weight(wp), bs, co, 1, act=ops.ACT_LRELU,
                                                     wpk_f4s=ops.pack_conv_weight(wp, f4s=True), x_amax=bound))
        assert [k for k in seen if k.startswith('conv')] == ['conv1x1_split_kernel'], seen
        outs.append((y, ops.get_bound(y)))
    return outs[0][0], outs[1][0], outs[0][1], outs[1][1]


def _fused(ops, emb, emb_ref, aligned, wf, bf, wa, ba, co, bound):
    (feat, attn), seen = _hooked(ops, lambda: ops.tsa_front(emb, emb_ref, aligned, ops.pack_conv_weight(wf, f4s=True), bf,
                                                            ops.pack_conv_weight(wa, f4s=True), ba, co, x_amax=bound))
    assert seen == [FUSED], seen
    return feat, attn, ops.get_bound(feat), ops.get_bound(attn)


def _check_against_three(ops, d, bound, emb=None, aligned=None):
    args = (d['emb'] if emb is None else emb, d['emb_ref'], d['aligned'] if aligned is None else aligned, d['wf'], d['bf'], d['wa'], d['ba'], d['co'], bound)
    got, again, ref = _fused(ops, *args), _fused(ops, *args), _three_launches(ops, *args)
    for name, x, y, z in zip(('feat', 'attn', 'feat y_amax', 'attn y_amax'), got, again, ref):
        assert x is not None and z is not None, name
        assert _same_bits(x, y), f'{name}: two launches of the fused kernel differ'
        assert _same_bits(x, z), (f'{name}: fused and three-launch results differ in {(_bits(x) != _bits(z)).sum().item()} of {x.numel()} elements, '
                                  f'max |diff| {(x - z).abs().nan_to_num(0).max().item():.3g}')
    return got


@pytest.mark.parametrize('name', list(SHAPES))
def test_tsa_front_equals_three_launches_and_fp64(gpu, name):
    from edvr_amd import ops
    d = _inputs(name, gpu)
    bound = ops.amax(d['aligned'].flatten(0, 1)) * 1.5
    feat, attn, fb, ab = _check_against_three(ops, d, bound)
    assert torch.equal(feat, _three_launches(ops, d['emb'], d['emb_ref'], d['aligned'], d['wf'], d['bf'], d['wa'], d['ba'], d['co'], bound)[0])
    for y, want, yb in ((feat, d['want'][0], fb), (attn, d['want'][1], ab)):
        err = ((y.double().cpu() - want).abs().max() / want.abs().max()).item()
        print(f'{name}: rel err {err:.3g} of max |ref|')
        assert err < RTOL, (name, err)
        assert yb.item() == y.abs().max().item()  # the epilogue's max |y|


@pytest.mark.parametrize('loose', [1024.0, 1.0], ids=['bound_2^10_loose', 'bound_tight'])
def test_tsa_front_input_scale(gpu, loose):
    """The input-scale path: a bound 2^10 above the data (ten bits fewer for the low half) and the exact maximum."""
    from edvr_amd import ops
    d = _inputs('c64_hw180', gpu)
    bound = ops.amax(d['aligned'].flatten(0, 1)) * loose
    feat, attn, _, _ = _check_against_three(ops, d, bound)
    for y, want in ((feat, d['want'][0]), (attn, d['want'][1])):
        err = ((y.double().cpu() - want).abs().max() / want.abs().max()).item()
        print(f'bound x{loose:g}: rel err {err:.3g} of max |ref|')
        assert err < RTOL, (loose, err)


@pytest.mark.parametrize('where', ['aligned', 'emb'])
def test_tsa_front_nan_reaches_both_amax_slots(gpu, where):
    """A NaN in `aligned` (one product) or in `emb` (a whole frame's pixel through its probability) must come out where and as the three
    launches leave it - in both outputs and, sticky, in both y_amax slots (the overflow guard reads those)."""
    from edvr_amd import ops
    d = _inputs('c64_hw180', gpu)
    bad = d[where].clone()
    bad[1, 3, 17, 4, 11] = float('nan')
    bound = ops.amax(d['aligned'].flatten(0, 1)) * 1.5  # (of the clean tensor: a bound is handed on, not re-measured)
    try:
        feat, attn, fb, ab = _check_against_three(ops, d, bound, **{where: bad})
    finally:  # the NaN slots of this test are not a later forward's business (ops.split_guard_submit examines what was handed out)
        ops._arena(gpu).take_unexamined()
        ops._GUARD_PENDING.clear()
    for y, yb in ((feat, fb), (attn, ab)):
        assert torch.isnan(y[1, :, 4, 11]).all() and torch.isnan(yb).all()
        assert torch.isfinite(y[0]).all() and torch.isnan(y[1]).sum().item() == y.shape[1]  # one pixel of one clip, every output channel


def test_tsa_front_ineligible_cases_run_the_three_launches(gpu):
    """functional.tsa_front outside the kernel's rule - gradients enabled, c = 12 (no multiple of 8) - is the old path, with its results."""
    from edvr_amd import functional as F_, ops
    b, t, c, h, w, co = 1, 5, 12, 4, 8, 32
    g = torch.Generator().manual_seed(21)
    emb, ref, al = (torch.randn(b, t, c, h, w, generator=g).to(gpu) * 0.3, torch.randn(b, c, h, w, generator=g).to(gpu) * 0.3,
                    torch.randn(b, t, c, h, w, generator=g).to(gpu))
    torch.manual_seed(3)
    mf, ma = torch.nn.Conv2d(t * c, co, 1).to(gpu), torch.nn.Conv2d(t * c, co, 1).to(gpu)
    ops.input_bound(al, al.flatten(0, 1))

    def old():
        mod = F_.tsa_temporal(emb, ref, al)
        mod = ops.carry_bound(mod.view(b, t * c, h, w), mod)
        return F_.conv(mf, mod, act=F_.ACT_LRELU), F_.conv(ma, mod, act=F_.ACT_LRELU)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            assert not F_.tsa_front_applies(mf, ma, emb, ref, al)
            (feat, attn), seen = _hooked(ops, lambda: F_.tsa_front(mf, ma, emb, ref, al))
            assert FUSED not in seen and 'tsa_temporal' in seen, seen
            want = old()
        assert torch.equal(feat.detach(), want[0].detach()) and torch.equal(attn.detach(), want[1].detach())
        assert feat.requires_grad == grad
    # ... and the same module pair at an eligible width takes the kernel without gradients, not with them
    c = 64
    emb, ref, al = (torch.randn(b, t, c, h, w, generator=g).to(gpu) * 0.3, torch.randn(b, c, h, w, generator=g).to(gpu) * 0.3,
                    torch.randn(b, t, c, h, w, generator=g).to(gpu))
    mf, ma = torch.nn.Conv2d(t * c, co, 1).to(gpu), torch.nn.Conv2d(t * c, co, 1).to(gpu)
    ops.input_bound(al, al.flatten(0, 1))
    assert not F_.tsa_front_applies(mf, ma, emb, ref, al)
    with torch.no_grad():
        assert F_.tsa_front_applies(mf, ma, emb, ref, al)
        (feat, attn), seen = _hooked(ops, lambda: F_.tsa_front(mf, ma, emb, ref, al))
        assert seen == [FUSED], seen
        prev = ops.set_tsa_front(False)
        try:
            assert not F_.tsa_front_applies(mf, ma, emb, ref, al)
            (f0, a0), seen = _hooked(ops, lambda: F_.tsa_front(mf, ma, emb, ref, al))
        finally:
            ops.set_tsa_front(prev)
        assert [k.split('<')[0] for k in seen] == ['tsa_temporal', 'conv1x1_split_kernel', 'conv1x1_split_kernel'], seen
        assert torch.equal(feat, f0) and torch.equal(attn, a0)
        assert _same_bits(ops.get_bound(feat), ops.get_bound(f0)) and _same_bits(ops.get_bound(attn), ops.get_bound(a0))
