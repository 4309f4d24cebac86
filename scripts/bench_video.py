"""Whole-video restoration: the windowed path (metrics.validate_clip: every frame's features once per window it appears in) against
VideoRestorer (once per frame), same seeded video, same chunk / batch, one process, arms alternated.

    python scripts/bench_video.py --config L_T5            # EDVR-L, 5 frames, 100 frames of 180x320, chunk 10
    python scripts/bench_video.py --config L_T7
    python scripts/bench_video.py --config L_deblur        # hr_in + predeblur, 720x1280
    python scripts/bench_video.py --config L_T5 --out-dtype uint8

Per arm: frames/s (median over the repeats) with the spread, peak device memory, and the per-kernel table of ONE restore (events
around every launch through ops.LAUNCH_HOOK: the gather's and the uint8 tail's share is a number).  Prints one JSON line and merges
it into --json (default profiles/video/bench_video.json) under the configuration's name.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

CONFIGS = {
    # name: (EDVR keywords, (h, w), frames, chunk, per-frame share of the windowed FLOPs per output frame or None)
    'L_T5': (dict(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None), (180, 320), 100, 10, (905.0, 4231.0)),
    'L_T7': (dict(num_feat=128, num_frame=7, num_reconstruct_block=40, center_frame_idx=None), (180, 320), 100, 10, (1267.0, 5251.0)),
    'L_deblur': (dict(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None, hr_in=True, with_predeblur=True),
                 (720, 1280), 100, 4, None),
    'toy': (dict(num_feat=64, num_frame=5, num_reconstruct_block=4, center_frame_idx=None), (32, 48), 12, 4, None),
}


def kernel_table(run):
    from edvr_amd import ops
    records = []

    def hook(name, flops, launch, nbytes, executed=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        records.append((name, flops, e0, e1))

    ops.LAUNCH_HOOK = hook
    try:
        run()
        torch.cuda.synchronize()
    finally:
        ops.LAUNCH_HOOK = None
    per = {}
    for name, flops, e0, e1 in records:
        d = per.setdefault(name, [0, 0.0, 0.0])
        d[0] += 1
        d[1] += e0.elapsed_time(e1)
        d[2] += flops
    total = sum(d[1] for d in per.values())
    rows = sorted(per.items(), key=lambda kv: -kv[1][1])
    return {'kernel_ms': round(total, 3), 'gflop': round(sum(d[2] for d in per.values()) * 1e-9, 1),
            'kernels': [{'name': k, 'launches': d[0], 'ms': round(d[1], 3), 'share': round(d[1] / total, 4)} for k, d in rows]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='L_T5', choices=sorted(CONFIGS))
    ap.add_argument('--frames', type=int, default=None)
    ap.add_argument('--chunk', type=int, default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--padding', default='reflection_circle')
    ap.add_argument('--out-dtype', default='float32', choices=['float32', 'uint8'])
    ap.add_argument('--json', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'video', 'bench_video.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_video.py measures on the GPU: none found')
    from edvr_amd import EDVR, VideoRestorer, _lib, metrics
    from edvr_amd.build import source_hash
    kwargs, (h, w), frames, chunk, share = CONFIGS[args.config]
    frames, chunk = args.frames or frames, args.chunk or chunk
    dev = torch.device('cuda:0')
    torch.manual_seed(10)
    net = EDVR(**kwargs).eval()
    g = torch.Generator().manual_seed(123)
    with torch.no_grad():  # default init zeroes conv_offset: every tap on the integer grid; give the offsets sub-pixel values instead
        for name, p in net.named_parameters():
            if name.endswith('conv_offset.weight'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif name.endswith('conv_offset.bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    net = net.to(dev)
    lq = torch.rand(frames, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    t = kwargs['num_frame']
    out_dtype = getattr(torch, args.out_dtype)
    vr = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=out_dtype)

    def windowed():
        return metrics.validate_clip(net, lq, num_frame=t, padding=args.padding, batch=chunk)[0]

    def video():
        return vr.restore(lq)

    arms = {'windowed': windowed, 'video': video}
    res = {k: {'s': []} for k in arms}
    with torch.no_grad():
        outs = {}
        for k, fn in arms.items():  # warm-up: every shape of the timed window; peak memory of one restore
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            outs[k] = fn()
            torch.cuda.synchronize()
            res[k]['peak_mem_mb'] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        if out_dtype == torch.float32:
            diff = (outs['video'] - outs['windowed']).abs().max().item() / outs['windowed'].abs().max().item()
        else:
            ref = (outs['windowed'].clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
            diff = (outs['video'].int() - ref.int()).abs().max().item()
        del outs
        for _ in range(args.repeats):  # alternate the arms: drift of the shared machine hits both alike
            for k, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                res[k]['s'].append(e0.elapsed_time(e1) * 1e-3)
        net.check_offsets()
        for k, fn in arms.items():
            res[k]['table'] = kernel_table(fn)
        net.check_offsets()
    for k, r in res.items():
        s = r.pop('s')
        r['seconds'] = [round(v, 4) for v in s]
        r['frames_per_s'] = round(frames / statistics.median(s), 3)
        r['spread'] = round((max(s) - min(s)) / statistics.median(s), 4)  # (max - min) / median over the repeats
    ratio = res['video']['frames_per_s'] / res['windowed']['frames_per_s']
    tab = res['video']['table']
    glue = sum(k['ms'] for k in tab['kernels'] if k['name'] in ('gather_images', 'upsample4x_add_u8', 'f32_to_u8_hwc'))
    result = {'config': args.config, 'edvr': {k: v for k, v in kwargs.items()}, 'hw': [h, w], 'frames': frames, 'chunk': chunk,
              'padding': args.padding, 'out_dtype': args.out_dtype, 'repeats': args.repeats, 'speedup': round(ratio, 4),
              'flop_ceiling': round(share[1] / (share[1] - share[0] * (t - 1) / t), 4) if share else None,
              'measured_flop_ratio': round(res['windowed']['table']['gflop'] / max(tab['gflop'], 1e-9), 4),
              'faster_beyond_spread': bool(ratio - 1.0 > res['windowed']['spread']),
              'gather_and_u8_share_of_video_kernel_time': round(glue / tab['kernel_ms'], 5),
              'max_output_difference': diff, 'windowed': res['windowed'], 'video': res['video'],
              'csrc_sha16': source_hash(), 'library': _lib.lib().edvr_version().decode(), 'device': torch.cuda.get_device_name(0)}
    for r in (result['windowed'], result['video']):
        r['table']['kernels'] = r['table']['kernels'][:14]  # the table's head; the shares are of the whole
    path = os.path.abspath(args.json)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    merged = json.load(open(path)) if os.path.exists(path) else {}
    merged[args.config + ('' if args.out_dtype == 'float32' else '_' + args.out_dtype)] = result
    with open(path, 'w') as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
