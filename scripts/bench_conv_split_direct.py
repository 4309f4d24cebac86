"""Split-operand direct conv (csrc/conv2d_s.hip) beside the fp32 direct kernel on the eight launches of the EDVR-L x4 step
(T5, 180x320, batch 10) that ran on conv2d_mfma_kernel: 20 launches between two events, three repeats, median and spread.
The 1x1 layers are also timed with the streaming kernel's packing in `wpk_f4s`: in a library built with conv1x1_eligible's channel
threshold lowered that is conv1x1_split_kernel, in the committed one the same fp32 launch again (the kernel name printed says which)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from edvr_amd import ops

dev = torch.device('cuda')
g = torch.Generator(device=dev).manual_seed(0)
LAYERS = [  # (name, n, ci, h, w, co, ks, stride)
    ('pyramid L2 (stride 2)', 50, 128, 180, 320, 128, 3, 2),
    ('pyramid L3 (stride 2)', 50, 128, 90, 160, 128, 3, 2),
    ('conv_first', 50, 3, 180, 320, 128, 3, 1),
    ('spatial_attn2 1x1', 10, 256, 90, 160, 128, 1, 1),
    ('spatial_attn4 1x1', 10, 128, 90, 160, 128, 1, 1),
    ('spatial_attn_l1 1x1', 10, 128, 90, 160, 128, 1, 1),
    ('spatial_attn_add1 1x1', 10, 128, 180, 320, 128, 1, 1),
    ('spatial_attn_add2 1x1', 10, 128, 180, 320, 128, 1, 1),
]


def timed(run, launches=20, repeats=3):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / launches)
    ts.sort()
    return ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[len(ts) // 2]


for (name, n, ci, h, w, co, ks, stride) in LAYERS:
    x = torch.randn(n, ci, h, w, device=dev, generator=g)
    wt = torch.randn(co, ci, ks, ks, device=dev, generator=g) * 0.05
    b = torch.randn(co, device=dev, generator=g)
    wpk, bound = ops.pack_conv_weight(wt), ops.amax(x)
    variants = [('fp32', {}), ('split', {'wpk_ds': ops.pack_conv_weight(wt, ds=True), 'x_amax': bound})]
    if ks == 1 and ci % 8 == 0:
        variants.append(('stream', {'wpk_f4s': ops.pack_conv_weight(wt, f4s=True), 'x_amax': bound}))
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    y = torch.empty(n, co, ho, wo, device=dev)
    fl = 2.0 * ci * ks * ks * co * n * ho * wo
    out, ref = [], None
    for tag, kw in variants:
        seen = []
        ops.LAUNCH_HOOK = lambda kname, flops, launch, *a: (seen.append(kname), launch())
        ops.conv2d(x, wpk, b, co, ks, stride=stride, act=ops.ACT_LRELU, out=y, **kw)
        ops.LAUNCH_HOOK = None
        ms, spread = timed(lambda: ops.conv2d(x, wpk, b, co, ks, stride=stride, act=ops.ACT_LRELU, out=y, **kw))
        ref = y.clone() if ref is None else ref
        d = ((y - ref).abs().max() / ref.abs().max()).item()
        out.append(f'{tag} [{seen[-1]}] {ms:.4f} ms +-{100 * spread:.1f}% ({fl / ms / 1e9:.1f} TF/s) vs fp32 {d:.1e}')
    print(f'{name} {n}x{ci}x{h}x{w} -> {co}: ' + ' | '.join(out), flush=True)
