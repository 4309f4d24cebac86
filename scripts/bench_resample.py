"""Times ops.resample (csrc/resample.hip) and the Y4M path with a delivery size in it.

  (a) ops.resample ('lanczos3') on float32 RGB: 8 frames of 1920 x 2880 -> 1080 x 1920 (a restored 720 x 480 DVD at 1080 rows, square
      pixels), 1 frame of 4320 x 7680 -> 2160 x 3840, 8 frames of 720 x 1280 -> 1080 x 1920 (an enlargement) and 8 frames of 1080 x 2880 ->
      1080 x 1920 (the rows are an identity axis): device events around one call after warm-up, the median of --iters calls and the range
      of single calls, the algorithmic bytes (source + output, each element once) and the share of the 6.29 TB/s measured HBM rate they
      amount to; beside each the same tensors through torch.nn.functional.interpolate(mode='bicubic', antialias=True) - the nearest
      stock op, a TIMING arm only: another kernel, another boundary rule, float32 sums;
  (b) restore_y4m on an in-memory telecined stream (`It`, 720 x 480 A32:27, F30000:1001; EDVR-L as trained, T = 5, deinterlace='film')
      with out_height=1080, square_pixels=True against no selector on the SAME stream, alternated, three runs each, host clock around the
      call ending in a synchronise: output frames/s of both arms and the bytes handed to the writer per frame.

    python scripts/bench_resample.py [--out profiles/resample/bench_resample.json] [--skip-video] [--video-frames 10]
"""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))

HBM_TBS = 6.29
CASES = [  # name, frames, (H, W), (Ho, Wo)
    ('dvd 8x3x1920x2880 -> 1080x1920', 8, (1920, 2880), (1080, 1920)),
    ('8k 1x3x4320x7680 -> 2160x3840', 1, (4320, 7680), (2160, 3840)),
    ('enlarge 8x3x720x1280 -> 1080x1920', 8, (720, 1280), (1080, 1920)),
    ('identity rows 8x3x1080x2880 -> 1080x1920', 8, (1080, 2880), (1080, 1920)),
]


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


def git_head(tree):
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=tree, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def kernel_rows(args, dev):
    from edvr_amd import ops
    from edvr_amd.resample import taps
    rows = []
    for name, n, (H, W), size in CASES:
        src = torch.rand((n, 3, H, W), generator=torch.Generator().manual_seed(0)).to(dev)
        out = torch.empty((n, 3) + size, dtype=torch.float32, device=dev)
        ops.resample(src, size, out=out)
        nbytes = 4 * (src.numel() + out.numel())
        first = timed(lambda: ops.resample(src, size, out=out), args.warmup, args.iters)
        stock = timed(lambda: torch.nn.functional.interpolate(src, size=size, mode='bicubic', align_corners=False, antialias=True),
                      min(args.warmup, 5), min(args.iters, 20))
        second = timed(lambda: ops.resample(src, size, out=out), 5, args.iters)  # alternate once more: the first arm ran on a colder device
        med = min(first[0], second[0])
        ty, tx = taps(H, size[0], 'lanczos3'), taps(W, size[1], 'lanczos3')
        row = dict(case=name, frames=n, source=[H, W], output=list(size), kernel='lanczos3', taps=[ty, tx], tile=list(ops.resample_tile(H, W, *size, ty, tx)),
                   algorithmic_bytes=nbytes, us=round(med, 2), us_runs=[round(first[0], 2), round(second[0], 2)],
                   us_min_max=[round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)],
                   hbm_fraction=round(nbytes / (med * 1e-6) / (HBM_TBS * 1e12), 4), stock_bicubic_antialias_us=round(stock[0], 2),
                   stock_us_min_max=[round(stock[1], 2), round(stock[2], 2)], stock_over_resample=round(stock[0] / med, 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del src, out
    return rows


def video_row(args, dev):
    """restore_y4m(deinterlace='film') on one resident telecined 480i stream, delivered at 1080 rows with square pixels against as it
    comes (2880 x 1920): EDVR-L, chunk 10 - the native arm is the film arm of scripts/bench_telecine.py."""
    from edvr_amd import EDVR, ops
    from edvr_amd.y4m import restore_y4m
    H, W, n, chunk = 480, 720, args.video_frames, 10
    torch.manual_seed(10)
    net = EDVR(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None).to(dev).eval()
    fs = ops.yuv420_frame_size(H, W)
    # smooth moving film frames (random samples would make the network's offsets run away) through 2:3 pulldown, top field first
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    fields = [j for j in range(n) for _ in range(3 if j % 2 else 2)][:2 * n]
    film = [((torch.sin((xx + 5 * t) / 17.0) * torch.cos(yy / 23.0) * 90 + 128).clamp(0, 255)).to(torch.uint8) for t in range(max(fields) + 1)]
    frames = torch.full((n, fs), 128, dtype=torch.uint8)
    for i in range(n):
        luma = film[fields[2 * i]].clone()
        luma[1::2] = film[fields[2 * i + 1]][1::2]
        frames[i, :H * W] = luma.reshape(-1)
    woven = f'YUV4MPEG2 W{W} H{H} F30000:1001 It A32:27 C420jpeg\n'.encode() + b''.join(b'FRAME\n' + f.numpy().tobytes() for f in frames)
    n_film = n - n // 5
    arms = {'native': {}, 'delivered': dict(out_height=1080, square_pixels=True)}

    def run(arm):
        src, dst = io.BytesIO(woven), io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = restore_y4m(net, src, dst, chunk=chunk, read_frames=chunk, deinterlace='film', **arms[arm])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert got == n_film
        data = dst.getvalue()
        head = data[:data.index(b'\n')]
        return got / dt, head.decode(), (len(data) - len(head) - 1) // got

    with torch.no_grad():
        for arm in arms:  # warm: weights packed, tables uploaded, the allocator filled
            run(arm)
        runs = {arm: [] for arm in arms}
        for _ in range(3):
            for arm in arms:
                runs[arm].append(run(arm))
    net.check_offsets()
    row = dict(case='EDVR-L T5 telecined 480i (720 x 480 A32:27), deinterlace=film', frames_in=n, frames_out=n_film, chunk=chunk)
    for arm in arms:
        row[arm] = dict(header=runs[arm][0][1], bytes_to_writer_per_frame=runs[arm][0][2], fps_runs=[round(r[0], 3) for r in runs[arm]],
                        fps=round(statistics.median(r[0] for r in runs[arm]), 4))
    row['delivered_over_native_fps'] = round(row['delivered']['fps'] / row['native']['fps'], 4)
    row['native_over_delivered_bytes'] = round(row['native']['bytes_to_writer_per_frame'] / row['delivered']['bytes_to_writer_per_frame'], 3)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'resample', 'bench_resample.json'))
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--video-frames', type=int, default=10, help='input frames of the restore_y4m arms')
    ap.add_argument('--skip-video', action='store_true', help='kernels only')
    ap.add_argument('--head', default=None, help='commit to record where the tree is not a git checkout (default: git rev-parse HEAD)')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_resample needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_resample', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(),
                  git_head=args.head or git_head(os.path.join(HERE, '..')), device=torch.cuda.get_device_name(0), hbm_tbs=HBM_TBS, warmup=args.warmup,
                  iters=args.iters, kernels=kernel_rows(args, dev))
    if not args.skip_video:
        record['restore_y4m'] = video_row(args, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
        print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
