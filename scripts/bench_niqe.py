"""Times the device NIQE (csrc/niqe.hip, metrics.calculate_niqe) on 8 frames of 720 x 1280 and on one of 2880 x 5120.

  (a) metrics.niqe_moments - the one kernel launch - with device events around the call (launch included) after warm-up: the median, the
      source bytes (12 per pixel for float32 RGB, 3 for RGB bytes; each pixel of the kept rectangle is needed once per scale) over that
      time as a share of the 6.29 TB/s measured HBM rate - the kernel is arithmetic-bound (2 x 49 double multiply-adds per pixel and
      scale), the share says how far from the memory floor that leaves it;
  (b) metrics.calculate_niqe whole, host clock around the call (it ends in the copy of 50 doubles per block and the float64 finish on the
      host): the kernel's share of that time is (a) / (b);
  (c) the NumPy restatement of the same definition (tests/util_niqe.py + metrics.niqe_from_moments) on the host for ONE 720 x 1280 frame,
      as the host-side comparison - the reference itself (scipy + cv2) is not a dependency of this repository.

    python scripts/bench_niqe.py --params niqe_pris_params.npz [--out profiles/niqe/bench_niqe.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

HBM_TBS = 6.29
CASES = [('8x720x1280', 8, (720, 1280)), ('1x2880x5120', 1, (2880, 5120))]


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


def host_timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times), min(times), max(times)


def git_head():
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=os.path.dirname(os.path.abspath(__file__)), stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def rows(args, dev):
    from edvr_amd import metrics
    params = metrics.load_niqe_params(args.params)
    out = []
    for name, n, (H, W) in CASES:
        as_bytes = torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(dev)
        as_float = (as_bytes.permute(0, 3, 1, 2).float() / 255.).contiguous()
        assert torch.equal(metrics.niqe_moments(as_bytes), metrics.niqe_moments(as_float))
        nbh, nbw = metrics.niqe_grid(H, W)
        kept = n * nbh * nbw * metrics.NIQE_BLOCK ** 2
        row = dict(case=name, frames=n, size=[H, W], blocks=nbh * nbw)
        for arm, x, bpp in (('f32', as_float, 12), ('u8', as_bytes, 3)):
            first, second = timed(lambda: metrics.niqe_moments(x), args.warmup, args.iters), timed(lambda: metrics.niqe_moments(x), 5, args.iters)
            med = min(first[0], second[0])  # twice: the first ran on a colder device
            whole = host_timed(lambda: metrics.calculate_niqe(x, params=params), 3, max(10, args.iters // 10))
            row.update({f'moments_{arm}_us': round(med, 2), f'moments_{arm}_us_runs': [round(first[0], 2), round(second[0], 2)],
                        f'moments_{arm}_us_min_max': [round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)],
                        f'source_bytes_{arm}': kept * bpp, f'moments_{arm}_hbm_fraction': round(kept * bpp / (med * 1e-6) / (HBM_TBS * 1e12), 5),
                        f'calculate_niqe_{arm}_us': round(whole[0], 2), f'calculate_niqe_{arm}_us_min_max': [round(whole[1], 2), round(whole[2], 2)],
                        f'kernel_share_{arm}': round(med / whole[0], 4)})
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def host_row(args):
    """The NumPy restatement on the host, one 720 x 1280 frame."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import util_niqe
    from edvr_amd import metrics
    params = metrics.load_niqe_params(args.params)
    img = torch.randint(0, 256, (720, 1280, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).numpy()
    t0 = time.perf_counter()
    m, nbh, nbw = util_niqe.moments(img)
    t1 = time.perf_counter()
    value = metrics.niqe_from_moments(m[None], nbh, nbw, params)[0]
    t2 = time.perf_counter()
    row = dict(case='1x720x1280 NumPy restatement', moments_s=round(t1 - t0, 3), finish_s=round(t2 - t1, 4), niqe=value)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--params', required=True, help="BasicSR's basicsr/metrics/niqe_pris_params.npz")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'niqe', 'bench_niqe.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--skip-host', action='store_true', help='device arms only')
    ap.add_argument('--head', default=None, help='commit to record where the tree is not a git checkout (default: git rev-parse HEAD)')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_niqe needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_niqe', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(), git_head=args.head or git_head(),
                  device=torch.cuda.get_device_name(0), hbm_tbs=HBM_TBS, warmup=args.warmup, iters=args.iters, device_rows=rows(args, dev))
    if not args.skip_host:
        record['host'] = host_row(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(record, f, indent=1)
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
