"""Times the device blur and noise degradations (csrc/degrade.hip, ops.degrade) and a stock arm of the same shape.

  (a) ops.degrade in its table form (nothing copied per call) at ksize 7 and 21, without and with noise (read sigma 10, shot 0.5), and
      noise alone, on one training batch of LQ crops (160 x 64 x 64: 32 clips x 5 frames), on 8 x 180 x 320 and on 32 x 720 x 1280: device
      events around one call (launch included) after warm-up, the median of `--iters` calls and their spread, twice; the bytes booked
      (3 n H W read and as many written) over that time as a share of the 6.29 TB/s measured HBM rate, and the integer multiply-adds
      (n H W 3 ksize^2) per second;
  (b) a stock arm for TIME only - its bytes differ: float32 frames through F.pad(mode='reflect'), one depthwise F.conv2d per image (the
      kernels are per image) and, with noise, x + sigma * torch.randn - the same events around the whole sequence;
  (c) samples/s of the training loader (32 clips x 5 frames, gt_size 256, LQ tree of 180 x 320 PNGs) with and without the default
      lq_degrade block, alternating, next to the samples/s the training step consumes.

    python scripts/bench_degrade.py [--out profiles/degrade/bench_degrade.json]
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

from bench_jpeg import HBM_TBS, TRAINING_STEP_SAMPLES_PER_S, frames_like_video, timed  # noqa: E402

CASES = [('160x64x64', 160, (64, 64)), ('8x180x320', 8, (180, 320)), ('32x720x1280', 32, (720, 1280))]
ARMS = [('k7', 7, None), ('k7_noise', 7, (10.0, 0.5, False)), ('k21', 21, None), ('k21_noise', 21, (10.0, 0.5, False)), ('noise', 0, (10.0, 0.5, False))]


def kernel_rows(args, dev):
    import torch.nn.functional as F
    from edvr_amd import ops
    from edvr_amd.data import gaussian_blur_kernel
    out = []
    for name, n, (H, W) in CASES:
        x = frames_like_video(n, H, W).to(dev)
        y = torch.empty_like(x)
        xf = x.permute(0, 3, 1, 2).float().contiguous()
        row = dict(case=name, frames=n, size=[H, W], booked_bytes=6 * n * H * W)
        for arm, ksize, noise in ARMS:
            kernel = gaussian_blur_kernel(ksize, 0.15 * ksize, 0.1 * ksize, 0.5) if ksize else None
            table, weights = ops.degrade_table(n, H, W, kernel, noise, seed=1)
            table = torch.from_numpy(table).to(dev)
            weights = None if weights is None else torch.from_numpy(weights).to(dev)
            fn = lambda: ops.degrade(x, table=table, weights=weights, out=y)
            first, second = timed(fn, args.warmup, args.iters), timed(fn, 5, args.iters)
            med = min(first[0], second[0])  # twice: the first ran on a colder device
            row.update({f'us_{arm}': round(med, 2), f'us_{arm}_runs': [round(first[0], 2), round(second[0], 2)],
                        f'us_{arm}_min_max': [round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)],
                        f'hbm_fraction_{arm}': round(6 * n * H * W / (med * 1e-6) / (HBM_TBS * 1e12), 5)})
            if ksize:
                row[f'tera_mads_per_s_{arm}'] = round(3.0 * n * H * W * ksize * ksize / (med * 1e-6) / 1e12, 3)
            # the stock arm: time only
            wf = None if kernel is None else (torch.from_numpy(kernel).float() / (1 << 20)).to(dev)[None, None].repeat(3, 1, 1, 1)
            r = ksize // 2

            def stock():
                z = xf
                if wf is not None:
                    padded = F.pad(z, (r, r, r, r), mode='reflect')
                    z = torch.cat([F.conv2d(padded[i:i + 1], wf, groups=3) for i in range(n)])
                if noise is not None:
                    z = z + noise[0] * torch.randn_like(z)
                return z
            s_med, s_min, s_max = timed(stock, 3, args.stock_iters)
            row.update({f'stock_us_{arm}': round(s_med, 1), f'stock_us_{arm}_min_max': [round(s_min, 1), round(s_max, 1)],
                        f'stock_over_device_{arm}': round(s_med / med, 1)})
            print(f'{name} {arm}: {med:.1f} us, stock {s_med:.1f} us', flush=True)
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def loader_rows(args):
    from bench_data import make_dataset
    from edvr_amd import data as D
    samples, t, P, s = 32, 5, 256, 4
    rates = {'plain': [], 'lq_degrade': []}
    with tempfile.TemporaryDirectory() as root:
        meta = make_dataset(root, ['001'], 100)
        tree = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
                    io_backend=dict(type='disk'), gt_size=P, scale=s, num_frame=t, interval_list=[1], random_reverse=False,
                    use_flip=True, use_rot=True, val_partition='REDS4')
        arms = {'plain': tree, 'lq_degrade': dict(tree, lq_degrade={k: dict(v) for k, v in D.LQ_DEGRADE_DEFAULTS.items()})}
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'degrade', 'bench_degrade.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--stock-iters', type=int, default=10)
    ap.add_argument('--host-threads', type=int, default=16)
    ap.add_argument('--loader-rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, default=6)
    ap.add_argument('--skip-loader', action='store_true', help='kernel and stock arms only')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_degrade needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_degrade', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(), device=torch.cuda.get_device_name(0),
                  hbm_tbs=HBM_TBS, warmup=args.warmup, iters=args.iters, stock_iters=args.stock_iters, kernel=kernel_rows(args, dev))
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
