"""-m gpu: where the split F(4x4) conv (csrc/winograd_f4s.hip) and the split tap-window DCN forward (csrc/dcn_tapwin_s.hip) ISSUE their
LDS-DMA requests inside a step is a matter of speed only (profiles/dma_placement/README.md: which placements were tried, and that the
f4s staging wave now prepares its requests while its patch reads are in flight): the results are the ones of the fp64 reference at
the kernels' own tolerances (tests/test_gpu_conv_f4s.py: 3e-5 of max |ref|; tests/test_gpu_dcn.py: 2e-5), and every launch
repeated gives the same bits - a request that overtakes the read of the region it overwrites, or a piece that lands after its
reader, shows as a run-to-run difference.  The shapes put the request cursor of a staging wave in every state: an item boundary at
every step (one chunk per item), two chunks, padding channels (one-plane and empty buffers), the x1 / x2 switch between chunks,
more items than workgroups (second items, the last one re-staged), both instantiations, blocks with pieces outside the image; the
DCN cases take both channel-group instantiations, partial tiles, and fields that send lanes through the fix-up pass with the pieces
in flight.  Measured: f4s 2.6e-6 - 4.8e-6, DCN 0.9e-6 - 1.7e-6."""
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL_F4S = 3e-5  # tests/test_gpu_conv_f4.py RTOL_F4
RTOL_DCN = 2e-5  # tests/test_gpu_dcn.py FWD_RTOL


def _rel(a, ref):
    return ((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


F4S_CASES = [
    # n, c1, c2, h, w, co, act, add
    (2, 8, 0, 16, 64, 64, 'lrelu', None),      # one chunk per item: the cursor crosses an item boundary at every step
    (6, 8, 0, 40, 320, 128, 'none', None),     # ... and 300 items on 256 workgroups: the boundary leads to a real second item
    (2, 16, 0, 16, 64, 64, 'lrelu', None),     # two chunks
    (1, 33, 0, 16, 64, 64, 'none', None),      # padding channels: the last pair of the last chunk's first wave is a one-plane buffer
    (1, 34, 0, 16, 64, 64, 'none', None),      # ... and the pairs behind it are empty buffers
    (2, 8, 8, 16, 64, 64, 'lrelu', None),      # two inputs: the x1 / x2 switch between the chunks
    (6, 16, 0, 40, 320, 128, 'lrelu', None),   # kernel <4>, 300 items on 256 workgroups: second items, the last one re-staged
    (2, 16, 0, 48, 96, 64, 'lrelu', None),     # kernel <3>
    (2, 16, 0, 12, 68, 64, 'lrelu', None),     # edge blocks: pieces outside the image in x and y
    (2, 16, 0, 48, 96, 64, 'none', 'res1'),    # epilogue variants (the staging waves run them between two chunk loops)
    (2, 16, 0, 48, 96, 64, 'lrelu', 'pre'),
]


@pytest.mark.parametrize('case', F4S_CASES)
def test_f4s_request_placement_keeps_results(gpu, case):
    from edvr_amd import ops
    n, c1, c2, h, w, co, actn, add = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    x1 = torch.randn(n, c1, h, w, generator=g)
    x2 = torch.randn(n, c2, h, w, generator=g) if c2 else None
    wt = torch.randn(co, c1 + c2, 3, 3, generator=g) * 0.1
    b = torch.randn(co, generator=g)
    extra = torch.randn(n, co, h, w, generator=g) if add else None
    ref = F.conv2d((x1 if x2 is None else torch.cat([x1, x2], 1)).double(), wt.double(), b.double(), 1, 1)
    if add == 'pre':
        ref = ref + extra.double()
    if actn == 'lrelu':
        ref = F.leaky_relu(ref, 0.1)
    if add == 'res1':
        ref = ref + extra.double()
    wg, x1g = wt.to(gpu), x1.to(gpu)
    kw = dict(x2=None if x2 is None else x2.to(gpu), act=ops.ACT_LRELU if actn == 'lrelu' else ops.ACT_NONE,
              wpk_f4s=ops.pack_conv_weight(wg, f4s=True), algo=ops.CONV_WINOGRAD_F4S)
    if add == 'res1':
        kw['res1'] = extra.to(gpu)
    elif add == 'pre':
        kw['pre'] = extra.to(gpu)
    names = []
    ops.LAUNCH_HOOK = lambda name, flops, launch, nbytes, executed=None: (names.append(name), launch())
    try:
        y = ops.conv2d(x1g, ops.pack_conv_weight(wg), b.to(gpu), co, 3, **kw)
    finally:
        ops.LAUNCH_HOOK = None
    assert any('conv3x3_winograd_f4s_kernel' in nm for nm in names), names  # the request reached the split kernel
    bound = ops.get_bound(y)  # y_amax on: the epilogue's own statistic
    assert bound is not None
    again = ops.conv2d(x1g, ops.pack_conv_weight(wg), b.to(gpu), co, 3, **kw)
    torch.cuda.synchronize()
    err = _rel(y, ref)
    print(f'f4s {case}: rel err {err:.3e}')
    assert err < RTOL_F4S, err
    assert torch.equal(y, again)
    assert bound.item() >= y.abs().max().item()


def _field(kind, B, dg, H, W, g):
    planes = dg * 18
    if kind == 'subpixel':
        return (torch.randn(B, planes, H, W, generator=g) * 0.3).contiguous()
    if kind == 'per_tap':  # a constant ~ N(0, 4^2) per (group, tap, dy | dx), slow motion, white residual; a few pixels jump by 9 px: the fix-up pass
        bias = torch.randn(1, planes, 1, 1, generator=g) * 4.0
        coarse = torch.randn(B, planes, (H + 15) // 16 + 1, (W + 15) // 16 + 1, generator=g) * 0.5
        off = bias + F.interpolate(coarse, scale_factor=16, mode='bilinear', align_corners=False)[:, :, :H, :W]
        off = off + torch.randn(B, planes, H, W, generator=g) * 0.15
        for i in range(3):
            yy, xx = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
            off[:, :, yy, xx] += 9.0 * (1 if i % 2 else -1)
        return off.contiguous()
    # a step edge inside the first 8 x 32 tile (and every tile below it): two windows' worth of cells in one tile
    base = torch.randn(1, planes, 1, 1, generator=g) * 1.5
    step = (torch.rand(1, planes, 1, 1, generator=g) * 2 - 1) * 6.0
    side = (torch.arange(W) >= 13).float().view(1, 1, 1, W)
    return (base + side * step + torch.randn(B, planes, H, W, generator=g) * 0.05).contiguous()


DCN_GEOMS = [(16, 1), (32, 2), (64, 8)]  # (C, dg): 16 channels per group (9 steps / 18 steps), 8 channels per group
DCN_SIZES = [(16, 64), (9, 40)]          # whole tiles / partial tiles in both directions
DCN_FIELDS = ['subpixel', 'per_tap', 'step_edge']


@pytest.mark.parametrize('field', DCN_FIELDS)
@pytest.mark.parametrize('size', DCN_SIZES)
@pytest.mark.parametrize('geom', DCN_GEOMS)
def test_dcn_split_request_placement_keeps_results(gpu, geom, size, field):
    from edvr_amd import ops
    from oracle import dcn_oracle as O
    (C, dg), (H, W), B = geom, size, 2
    g = torch.Generator().manual_seed(zlib.crc32(repr((geom, size, field)).encode()))
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * 0.1
    b = torch.randn(C, generator=g)
    off = _field(field, B, dg, H, W, g)
    m = torch.rand(B, dg * 9, H, W, generator=g)
    ref = O.c_forward(x.double(), off.double(), m.double(), w.double(), b.double(), 1, 1, 1, 1, dg)
    dev = [t.to(gpu) for t in (x, off, m, w, b)]
    bound = ops.amax(dev[0])
    names = []
    ops.LAUNCH_HOOK = lambda name, flops, launch, nbytes, executed=None: (names.append(name), launch())
    try:
        y = ops.dcnv2_forward(*dev, 1, 1, 1, 1, dg, halo_hint=ops.DCN_HALO_TAPWIN, xm_bound=bound)
    finally:
        ops.LAUNCH_HOOK = None
    assert names == ['dcnv2_fwd[dcn_tapwin_split_fwd_kernel]'], names
    again = ops.dcnv2_forward(*dev, 1, 1, 1, 1, dg, halo_hint=ops.DCN_HALO_TAPWIN, xm_bound=bound)
    torch.cuda.synchronize()
    err = _rel(y, ref)
    print(f'dcn split C {C} dg {dg} {H}x{W} {field}: rel err {err:.3e}')
    assert err < RTOL_DCN, err
    assert torch.equal(y, again)
