"""Times the bicubic imresize kernel (csrc/resize.hip) on the three shapes of its users - the x4 reduction of a 4K-class GT frame, of a
720p frame (uint8 in, float32 out) and the x4 bicubic baseline of a 180 x 320 LQ frame (float32) - with device events after warm-up,
and beside each the same tensors through torch.nn.functional.interpolate(mode='bicubic', antialias=True) on float32 input.  The stock
op is the nearest existing op and a TIMING arm only: its boundary rule differs, it is no parity witness.

    python scripts/bench_resize.py [--out profiles/resize/bench_resize.json]

Records the median time, the algorithmic bytes (source + output, each element once) and the share of the 6.29 TB/s measured HBM rate
they amount to.  The bar: on the uint8 cases the kernel is not slower than the stock op (it reads a quarter of its source bytes).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

HBM_TBS = 6.29
CASES = [  # name, frames, (H, W), scale, uint8 source
    ('u8_2880x5120_to_720x1280', 1, (2880, 5120), 1 / 4, True),
    ('u8_720x1280_to_180x320', 8, (720, 1280), 1 / 4, True),
    ('f32_180x320_to_720x1280', 8, (180, 320), 4.0, False),
]


def timed(fn, warmup, iters):
    """Median over `iters` of the device time of fn() in microseconds (events around each call, after `warmup` calls)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'resize', 'bench_resize.json'))
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_resize needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib, ops
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    rows = []
    for name, n, (H, W), scale, u8 in CASES:
        g = torch.Generator().manual_seed(0)
        src_u8 = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        src_f = ops.frames_u8_to_f32(src_u8[None])[0]
        src = src_u8 if u8 else src_f
        out = ops.imresize(src, scale)
        nbytes = src.numel() * src.element_size() + out.numel() * 4
        ours = timed(lambda: ops.imresize(src, scale), args.warmup, args.iters)
        size = tuple(out.shape[-2:])
        stock = timed(lambda: torch.nn.functional.interpolate(src_f, size=size, mode='bicubic', align_corners=False, antialias=True),
                      args.warmup, args.iters)
        # alternate once more: the first arm ran on a colder device
        ours2 = timed(lambda: ops.imresize(src, scale), 5, args.iters)
        med = min(ours[0], ours2[0])
        row = dict(case=name, frames=n, source=[H, W], output=list(size), scale=scale, source_dtype='uint8' if u8 else 'float32',
                   algorithmic_bytes=nbytes, imresize_us=round(med, 2), imresize_us_runs=[round(ours[0], 2), round(ours2[0], 2)],
                   imresize_us_min_max=[round(min(ours[1], ours2[1]), 2), round(max(ours[2], ours2[2]), 2)],
                   hbm_fraction=round(nbytes / (med * 1e-6) / (HBM_TBS * 1e12), 4),
                   stock_interpolate_f32_us=round(stock[0], 2), stock_source_bytes=src_f.numel() * 4,
                   stock_over_imresize=round(stock[0] / med, 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    record = dict(bench='bench_resize', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(), device=torch.cuda.get_device_name(0),
                  hbm_tbs=HBM_TBS, warmup=args.warmup, iters=args.iters, cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
