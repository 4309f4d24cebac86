"""Times the BD downsampling kernel (csrc/bd.hip) on the three shapes of its users - the x4 reduction of a 4K-class GT frame and of
eight 720p frames from bytes, and of eight 720p frames from float32 - with device events around one call (launch included) after warm-up,
and beside each, in the same process:

  (b) ops.imresize at the same shape and 1 / scale: the bicubic kernel moves the same bytes with 18 taps per axis instead of 13 - the
      yardstick (the BD kernel should take no more than 1.1 x its time);
  (c) the stock composition the reference uses - F.pad(reflect) + F.conv2d(stride = scale) with the 13 x 13 float32 filter + crop - on
      float32 input through PyTorch.  Here the stock op is the same function, so this arm is also a parity witness (max abs difference).

    python scripts/bench_bd.py [--out profiles/bd/bench_bd.json]

Records the median time, the algorithmic bytes (source + output, each element once) and the share of the 6.29 TB/s measured HBM rate
they amount to.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

HBM_TBS = 6.29
SCALE = 4
CASES = [  # name, frames, (H, W), uint8 source
    ('u8_2880x5120_to_720x1280', 1, (2880, 5120), True),
    ('u8_8x720x1280_to_180x320', 8, (720, 1280), True),
    ('f32_8x720x1280_to_180x320', 8, (720, 1280), False),
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


def stock_bd(x, filt, scale):
    """duf_downsample as the reference writes it (data_util.py:299-331), on whatever device x lives."""
    n, c, h, w = x.shape
    pad = 6 + 2 * scale
    y = torch.nn.functional.pad(x.reshape(-1, 1, h, w), (pad, pad, pad, pad), mode='reflect')
    y = torch.nn.functional.conv2d(y, filt, stride=scale)[:, :, 2:-2, 2:-2]
    return y.reshape(n, c, y.shape[2], y.shape[3])


def git_head():
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=os.path.dirname(os.path.abspath(__file__)), stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'bd', 'bench_bd.json'))
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--head', default=None, help='commit to record where the tree is not a git checkout (default: git rev-parse HEAD)')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_bd needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib, ops
    from edvr_amd.build import source_hash
    from edvr_amd.data import bd_weights
    dev = torch.device('cuda:0')
    g = torch.from_numpy(bd_weights(SCALE))
    filt = torch.outer(g, g).float()[None, None].to(dev)
    rows = []
    for name, n, (H, W), u8 in CASES:
        gen = torch.Generator().manual_seed(0)
        src_u8 = torch.randint(0, 256, (n, H, W, 3), generator=gen, dtype=torch.uint8).to(dev)
        src_f = ops.frames_u8_to_f32(src_u8[None])[0]
        src = src_u8 if u8 else src_f
        out = ops.bd_downsample(src, SCALE)
        parity = (out - stock_bd(src_f, filt, SCALE)).abs().max().item()
        nbytes = src.numel() * src.element_size() + out.numel() * 4
        ours = timed(lambda: ops.bd_downsample(src, SCALE), args.warmup, args.iters)
        bicubic = timed(lambda: ops.imresize(src, 1 / SCALE), args.warmup, args.iters)
        stock = timed(lambda: stock_bd(src_f, filt, SCALE), args.warmup, max(20, args.iters // 4))
        # alternate once more: the first arms ran on a colder device
        ours2 = timed(lambda: ops.bd_downsample(src, SCALE), 5, args.iters)
        bicubic2 = timed(lambda: ops.imresize(src, 1 / SCALE), 5, args.iters)
        med, bic = min(ours[0], ours2[0]), min(bicubic[0], bicubic2[0])
        row = dict(case=name, frames=n, source=[H, W], output=list(out.shape[-2:]), scale=SCALE, source_dtype='uint8' if u8 else 'float32',
                   algorithmic_bytes=nbytes, bd_us=round(med, 2), bd_us_runs=[round(ours[0], 2), round(ours2[0], 2)],
                   bd_us_min_max=[round(min(ours[1], ours2[1]), 2), round(max(ours[2], ours2[2]), 2)],
                   hbm_fraction=round(nbytes / (med * 1e-6) / (HBM_TBS * 1e12), 4),
                   imresize_us=round(bic, 2), imresize_us_runs=[round(bicubic[0], 2), round(bicubic2[0], 2)], bd_over_imresize=round(med / bic, 3),
                   stock_pad_conv2d_f32_us=round(stock[0], 2), stock_source_bytes=src_f.numel() * 4, stock_over_bd=round(stock[0] / med, 2),
                   stock_max_abs_diff=parity)
        rows.append(row)
        print(json.dumps(row), flush=True)
    record = dict(bench='bench_bd', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(), git_head=args.head or git_head(),
                  device=torch.cuda.get_device_name(0), hbm_tbs=HBM_TBS, warmup=args.warmup, iters=args.iters, cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
