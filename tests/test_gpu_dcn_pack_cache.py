"""-m gpu: the split tap-window DCN forward packs its weights once per parameter version (ops.pack_dcn_split_weight), not at every call:
launch counts through ops.LAUNCH_HOOK, and y bit-identical to the entry point that packs per call."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PACK, FWD = 'dcn_split_pack_weight', 'dcnv2_fwd[dcn_tapwin_split_fwd_kernel]'


def _hooked(ops, fn):
    seen = []
    ops.LAUNCH_HOOK = lambda name, flops, launch, *a: (seen.append(name), launch())
    try:
        out = fn()
    finally:
        ops.LAUNCH_HOOK = None
    return out, seen


@pytest.mark.parametrize('C,dg,h,w', [(16, 2, 8, 32), (64, 8, 16, 64)])
def test_dcn_split_weights_are_packed_once_per_version(gpu, C, dg, h, w):
    from edvr_amd import ops
    g = torch.Generator().manual_seed(C)
    B, Co = 2, C
    x = torch.randn(B, C, h, w, generator=g).to(gpu)
    offset = (torch.randn(B, dg * 18, h, w, generator=g) * 1.5).to(gpu)
    mask = torch.rand(B, dg * 9, h, w, generator=g).to(gpu)
    weight = torch.nn.Parameter((torch.randn(Co, C, 3, 3, generator=g) * 0.05).to(gpu))
    bias = torch.randn(Co, generator=g).to(gpu)
    xb = ops.amax(x)
    geo = (1, 1, 1, 1, dg)

    def run(cached):
        with torch.no_grad():
            return _hooked(ops, lambda: ops.dcnv2_forward(x, offset, mask, weight.detach(), bias, *geo, act=ops.ACT_LRELU, halo_hint=ops.DCN_HALO_TAPWIN,
                                                          xm_bound=xb, w_param=weight if cached else None).clone())
    ops.invalidate_packed_weights()
    y1, s1 = run(True)
    y2, s2 = run(True)
    ref, s0 = run(False)
    assert s1 == [PACK, FWD] and s2 == [FWD] and s0 == [FWD], (s1, s2, s0)  # (the per-call entry point packs inside its own call)
    assert torch.isfinite(ref).all() and torch.equal(y1, ref) and torch.equal(y2, ref)
    with torch.no_grad():
        weight.add_(0.01)
    ops.invalidate_packed_weights()
    y3, s3 = run(True)
    y4, s4 = run(True)
    ref3, _ = run(False)
    assert s3 == [PACK, FWD] and s4 == [FWD], (s3, s4)
    assert torch.equal(y3, ref3) and torch.equal(y4, ref3) and not torch.equal(ref3, ref)
    with torch.no_grad():  # an in-place write that moves the version counter needs no helper: the key follows it
        weight.mul_(0.5)
    y5, s5 = run(True)
    assert s5 == [PACK, FWD] and torch.equal(y5, run(False)[0])
