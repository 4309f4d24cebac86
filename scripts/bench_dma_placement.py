"""Per-layer times of the split F(4x4) conv and of the split tap-window DCN forward under several builds of the library (A/B of
where the kernels issue their LDS-DMA requests: profiles/dma_placement/README.md).

    python scripts/bench_dma_placement.py NAME=path/to/libedvr_amd.so [NAME=path ...] [--repeats 3] [--only f4s|dcn]

Every build runs in a process of its own (EDVR_AMD_LIB), one after the other, the builds interleaved within each repeat; a layer is
20 launches between two events.  Prints one line per (layer, build): the median over the repeats and their spread, in ms."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(only):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from edvr_amd import ops
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}

    def timed(run):
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 20

    if only in (None, 'f4s'):
        for (n, c, h, w, co) in [(50, 128, 180, 320, 128), (10, 128, 180, 320, 128), (10, 64, 720, 1280, 64)]:
            x = torch.randn(n, c, h, w, device=dev, generator=g)
            wt = torch.randn(co, c, 3, 3, device=dev, generator=g) * 0.05
            b = torch.randn(co, device=dev, generator=g)
            res = torch.randn(n, co, h, w, device=dev, generator=g)
            wpk, wf4s = ops.pack_conv_weight(wt), ops.pack_conv_weight(wt, f4s=True)
            bound = ops.amax(x)
            y = torch.empty(n, co, h, w, device=dev)
            for label, kw in (('lrelu', dict(act=ops.ACT_LRELU)), ('none + res1', dict(res1=res))):
                out[f'f4s {c}->{co} {h}x{w} n={n} {label}'] = timed(
                    lambda: ops.conv2d(x, wpk, b, co, 3, wpk_f4s=wf4s, x_amax=bound, algo=ops.CONV_WINOGRAD_F4S, out=y, **kw))
            del x, res, y
    if only in (None, 'dcn'):
        for (B, C, H, W) in [(50, 128, 180, 320), (160, 128, 64, 64)]:
            dg = 8
            x = torch.randn(B, C, H, W, device=dev, generator=g)
            w = torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05
            b = torch.randn(C, device=dev, generator=g)
            m = torch.rand(B, dg * 9, H, W, device=dev, generator=g)
            bound = ops.amax(x)
            y = torch.empty(B, C, H, W, device=dev)
            for label, sigma in (('sub-pixel', 0.3), ('sigma 4', 4.0)):  # (the field of scripts/bench_dcn_split.py, its per-tap constants scaled)
                bias = torch.randn(1, dg * 18, 1, 1, device=dev, generator=g) * sigma
                coarse = torch.randn(B, dg * 18, (H + 15) // 16 + 1, (W + 15) // 16 + 1, device=dev, generator=g) * (0.5 if sigma > 1 else 0.1)
                off = (bias + F.interpolate(coarse, scale_factor=16, mode='bilinear', align_corners=False)[:, :, :H, :W]
                       + torch.randn(B, dg * 18, H, W, device=dev, generator=g) * 0.15).contiguous()
                out[f'dcn {B}x{C}x{H}x{W} {label}'] = timed(
                    lambda: ops.dcnv2_forward(x, off, m, w, b, 1, 1, 1, 1, dg, act=ops.ACT_LRELU, halo_hint=ops.DCN_HALO_TAPWIN, out=y, xm_bound=bound))
                del off
            del x, y
    print('RESULT ' + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == '--child':
        return child(args[1] if len(args) > 1 and args[1] != 'all' else None)
    repeats, only, builds = 3, 'all', []
    i = 0
    while i < len(args):
        if args[i] == '--repeats':
            repeats, i = int(args[i + 1]), i + 2
        elif args[i] == '--only':
            only, i = args[i + 1], i + 2
        else:
            name, path = args[i].split('=', 1)
            builds.append((name, os.path.abspath(path)))
            i += 1
    times = {}
    for rep in range(repeats):
        for name, path in builds:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', only], env=dict(os.environ, EDVR_AMD_LIB=path),
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:  # a fault is a finding: nothing more is started on the device
                sys.exit(f'build {name} failed (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}')
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
            for layer, ms in res.items():
                times.setdefault(layer, {}).setdefault(name, []).append(ms)
            print(f'repeat {rep} {name}: ' + ', '.join(f'{ms:.4f}' for ms in res.values()), flush=True)
    base = builds[0][0]
    for layer, per in times.items():
        ref = statistics.median(per[base])
        for name, _ in builds:
            v = per[name]
            med = statistics.median(v)
            print(f'{layer:44s} {name:10s} median {med:8.4f} ms  spread {100 * (max(v) - min(v)) / med:5.2f} %  vs {base} {100 * (med / ref - 1):+6.2f} %  {v}')


if __name__ == '__main__':
    main()
