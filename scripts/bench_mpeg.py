"""Times the device MPEG-style round trip (csrc/mpeg.hip, ops.mpeg_roundtrip).

  (a) ops.mpeg_roundtrip at qscale 8, gop 12, on one training batch of LQ crop clips (32 x 5 x 64 x 64), on 1 x 8 x 180 x 320 and on
      4 x 8 x 720 x 1280, each at search 7 and 15 and - the arm that tells what the search costs - at search 0: device events around
      one call (its t + 2 launches included) after warm-up, the median of `--iters` calls and their range, twice - `us_r*` is the lower
      of the two medians (the first run is on a colder device), `us_r*_runs` holds both; the share of the
      time that goes when the search goes; SAD candidates (one 16 x 16 block against one displacement) per second over the time the
      search adds;
  (b) samples/s of the training loader (32 clips x 5 frames, gt_size 256, LQ tree of 180 x 320 PNGs) with and without
      lq_mpeg = {'qscale': [2, 16]}, alternating, next to the samples/s the training step consumes.

    python scripts/bench_mpeg.py [--out profiles/mpeg/bench_mpeg.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

QSCALE, GOP = 8, 12
CASES = [('32x5x64x64', 32, 5, (64, 64)), ('1x8x180x320', 1, 8, (180, 320)), ('4x8x720x1280', 4, 8, (720, 1280))]
TRAINING_STEP_SAMPLES_PER_S = 293.0  # README: what the EDVR-L training step consumes on one GPU


def timed(fn, warmup, iters):
    """Median, min, max over `iters` of the device time of fn() in microseconds (events around each call, after `warmup` calls)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times), max(times)


def clips_like_video(b, t, H, W):
    """Smooth content that drifts by (1, -2) pixels a frame, with mild noise; the kernels' time does not depend on it."""
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    frames = []
    for i in range(t):
        y, x = yy + i, xx - 2 * i
        frames.append(torch.stack([128 + 100 * torch.sin(x / 23.0 + y / 31.0), 128 + 90 * torch.cos(x / 17.0), (x + y) % 256 * 1.0], -1))
    base = torch.stack(frames)
    return torch.stack([(base + 6 * torch.randn(t, H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8) for _ in range(b)])


def kernel_rows(args, dev):
    from edvr_amd import ops
    out = []
    for name, b, t, (H, W) in CASES:
        x = clips_like_video(b, t, H, W).to(dev)
        y = torch.empty_like(x)
        mbs = b * t * ((H + 15) // 16) * ((W + 15) // 16)
        predicted = sum(1 for i in range(t) if i % GOP) / t
        row = dict(case=name, clips=b, frames=t, size=[H, W], qscale=QSCALE, gop=GOP, launches=t + 2, macroblocks=mbs)
        for R in (0, 7, 15):
            fn = lambda: ops.mpeg_roundtrip(x, QSCALE, GOP, R, out=y)
            first, second = timed(fn, args.warmup, args.iters), timed(fn, 5, args.iters)
            row.update({f'us_r{R}': round(min(first[0], second[0]), 2), f'us_r{R}_runs': [round(first[0], 2), round(second[0], 2)],
                        f'us_r{R}_min_max': [round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)]})
        for R in (7, 15):
            extra = row[f'us_r{R}'] - row['us_r0']
            row[f'search_share_r{R}'] = round(extra / row[f'us_r{R}'], 3)
            cands = mbs * predicted * (2 * R + 1) ** 2
            row[f'sad_candidates_r{R}'] = int(cands)
            row[f'sad_candidates_per_s_r{R}'] = round(cands / (extra * 1e-6), 0) if extra > 0 else None
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def loader_rows(args):
    from bench_data import make_dataset
    from edvr_amd import data as D
    samples, t, P, s = 32, 5, 256, 4
    rates = {'plain': [], 'lq_mpeg': []}
    with tempfile.TemporaryDirectory() as root:
        meta = make_dataset(root, ['001'], 100)
        tree = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
                    io_backend=dict(type='disk'), gt_size=P, scale=s, num_frame=t, interval_list=[1], random_reverse=False,
                    use_flip=True, use_rot=True, val_partition='REDS4')
        arms = {'plain': tree, 'lq_mpeg': dict(tree, lq_mpeg={'qscale': [2, 16]})}
        for _ in range(args.loader_rounds):  # alternating
            for name, opt in arms.items():
                loader = D.REDSDeviceLoader(opt, samples, ratio=100, seed=0, num_threads=args.host_threads)
                loader.next()
                torch.cuda.synchronize()
                t0 = time.time()
                for _b in range(args.batches):
                    batch = loader.next()
                    assert batch['lq'].shape == (samples, t, 3, P // s, P // s)
                torch.cuda.synchronize()
                rates[name].append(args.batches * samples / (time.time() - t0))
                loader.close()
                print(f'{name}: {rates[name][-1]:.1f} samples/s', flush=True)
    out = {name: {'samples_per_s': round(statistics.median(v), 1), 'min_max': [round(min(v), 1), round(max(v), 1)]} for name, v in rates.items()}
    out.update(decode_threads=args.host_threads, batches_timed=args.batches, batch=samples, cpus=len(os.sched_getaffinity(0)),
               training_step_consumes_samples_per_s=TRAINING_STEP_SAMPLES_PER_S,
               tree='synthetic PNG, 720 x 1280 GT and 180 x 320 LQ (bench_data.make_dataset), page cache warm')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpeg', 'bench_mpeg.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--host-threads', type=int, default=16)
    ap.add_argument('--loader-rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, default=6)
    ap.add_argument('--skip-loader', action='store_true', help='kernel arms only')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_mpeg needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_mpeg', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(), device=torch.cuda.get_device_name(0),
                  warmup=args.warmup, iters=args.iters, kernel=kernel_rows(args, dev))
    if not args.skip_loader:
        record['loader'] = loader_rows(args)
        print(json.dumps(record['loader']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
