"""Times the device JPEG round trip (csrc/jpeg.hip, ops.jpeg_roundtrip) and what it replaces.

  (a) ops.jpeg_roundtrip at quality 75, '420' and '444', on one training batch of LQ crops (160 x 64 x 64: 32 clips x 5 frames), on
      8 x 180 x 320 and on 1 x 720 x 1280 - all three at most one wave of workgroups, i.e. at the floor of one launch - and on 32 x 720 x 1280
      (30 workgroups per CU), where the kernel's own rate shows: device events around one call (launch included) after warm-up, the median of `--iters` calls
      and their spread, twice; the bytes booked (3 n H W read and as many written) over that time as a share of the 6.29 TB/s measured HBM
      rate; the '420' / '444' ratio - where the ring of chroma blocks a '420' tile recomputes shows;
  (b) the same frames through PIL's JPEG writer and reader on 16 host threads (what a user without the operator does), wall clock;
  (c) samples/s of the training loader (32 clips x 5 frames, gt_size 256, LQ tree of 180 x 320 PNGs) with and without
      lq_jpeg = {'quality': [30, 90]}, alternating, next to the samples/s the training step consumes.

    python scripts/bench_jpeg.py [--out profiles/jpeg/bench_jpeg.json]
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_TBS = 6.29
QUALITY = 75
CASES = [('160x64x64', 160, (64, 64)), ('8x180x320', 8, (180, 320)), ('1x720x1280', 1, (720, 1280)), ('32x720x1280', 32, (720, 1280))]
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


def frames_like_video(n, H, W):
    """Smooth content with mild noise (white noise would be the codec's worst and least typical case); the kernel's time does not depend on it."""
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    base = torch.stack([128 + 100 * torch.sin(xx / 23.0 + yy / 31.0), 128 + 90 * torch.cos(xx / 17.0), (xx + yy) % 256 * 1.0], -1)
    return (base[None] + 6 * torch.randn(n, H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)


def pil_roundtrip(img, subsampling):
    import numpy as np
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=QUALITY, subsampling={'444': 0, '420': 2}[subsampling])
    buf.seek(0)
    return np.asarray(Image.open(buf).convert('RGB'))


def kernel_rows(args, dev):
    from edvr_amd import ops
    out = []
    with ThreadPoolExecutor(args.host_threads) as pool:
        for name, n, (H, W) in CASES:
            host = frames_like_video(n, H, W)
            x = host.to(dev)
            row = dict(case=name, frames=n, size=[H, W], quality=QUALITY, booked_bytes=6 * n * H * W)
            for sub in ('420', '444'):
                y = torch.empty_like(x)
                fn = lambda: ops.jpeg_roundtrip(x, QUALITY, sub, out=y)
                first, second = timed(fn, args.warmup, args.iters), timed(fn, 5, args.iters)
                med = min(first[0], second[0])  # twice: the first ran on a colder device
                imgs = list(host.numpy())
                got = list(pool.map(lambda im: pil_roundtrip(im, sub), imgs))  # (warm-up, and the check that both arms make the same bytes)
                assert all(torch.equal(torch.from_numpy(g.copy()), y[i].cpu()) for i, g in enumerate(got)), (name, sub)
                walls = []
                for _ in range(args.host_rounds):
                    t0 = time.perf_counter()
                    list(pool.map(lambda im: pil_roundtrip(im, sub), imgs))
                    walls.append((time.perf_counter() - t0) * 1e6)
                row.update({f'us_{sub}': round(med, 2), f'us_{sub}_runs': [round(first[0], 2), round(second[0], 2)],
                            f'us_{sub}_min_max': [round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)],
                            f'hbm_fraction_{sub}': round(6 * n * H * W / (med * 1e-6) / (HBM_TBS * 1e12), 5),
                            f'pil_{args.host_threads}_threads_us_{sub}': round(statistics.median(walls), 1),
                            f'pil_{args.host_threads}_threads_us_{sub}_min_max': [round(min(walls), 1), round(max(walls), 1)]})
                row[f'pil_over_device_{sub}'] = round(row[f'pil_{args.host_threads}_threads_us_{sub}'] / med, 1)
            row['ratio_420_over_444'] = round(row['us_420'] / row['us_444'], 3)
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def loader_rows(args):
    from bench_data import make_dataset
    from edvr_amd import data as D
    samples, t, P, s = 32, 5, 256, 4
    rates = {'plain': [], 'lq_jpeg': []}
    with tempfile.TemporaryDirectory() as root:
        meta = make_dataset(root, ['001'], 100)
        tree = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
                    io_backend=dict(type='disk'), gt_size=P, scale=s, num_frame=t, interval_list=[1], random_reverse=False,
                    use_flip=True, use_rot=True, val_partition='REDS4')
        arms = {'plain': tree, 'lq_jpeg': dict(tree, lq_jpeg={'quality': [30, 90]})}
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg', 'bench_jpeg.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--host-threads', type=int, default=16)
    ap.add_argument('--host-rounds', type=int, default=5)
    ap.add_argument('--loader-rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, default=6)
    ap.add_argument('--skip-loader', action='store_true', help='kernel and PIL arms only')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_jpeg needs the GPU: there is no CPU path to time'
    import PIL
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_jpeg', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(), device=torch.cuda.get_device_name(0),
                  hbm_tbs=HBM_TBS, warmup=args.warmup, iters=args.iters, pil=PIL.__version__, kernel=kernel_rows(args, dev))
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
