"""Times ops.deinterlace (csrc/deint.hip) and the Y4M path with the stage in it.

  (a) ops.deinterlace in 'field' and 'frame' mode on 8 frames of 576 x 720 '420', 1080 x 1920 '420' and 1080 x 1920 '422p10', the input
      inside a Y4M buffer (stride framesize + 6, 6 bytes in: how restore_y4m calls it), the output dense: device events around one call
      (launch included) after warm-up, the median of --iters calls and their spread, the bytes the op books (n_out framesize (1 + 6.5):
      every row segment a lane reads, most of them from the cache) and the bytes that must cross HBM (every input frame and every output
      frame once) with the share of the 6.29 TB/s measured HBM rate each amounts to; beside it, in the same process at the same shape,
      ops.yuv_to_rgb (bilinear chroma) on the same buffer - the decode that follows it in the pipe - and the ratio of the two times;
  (b) restore_y4m on an in-memory 576i stream (`It`, 720 x 576, EDVR-L as trained, T = 5) with deinterlace='field' in output frames/s,
      host clock around the call ending in a synchronise, against the SAME output frames fed as an `Ip` stream at twice the rate,
      alternated, three runs each.

    python scripts/bench_deinterlace.py [--out profiles/deint/bench_deinterlace.json] [--skip-video] [--video-frames 10]
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
CASES = [('8x576x720 420', 8, 576, 720, '420'), ('8x1080x1920 420', 8, 1080, 1920, '420'), ('8x1080x1920 422p10', 8, 1080, 1920, '422p10')]


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
    rows = []
    for name, n, H, W, fmt in CASES:
        fs = ops.yuv_frame_size(H, W, fmt)
        depth = ops.yuv_format(fmt)[2]
        gen = torch.Generator().manual_seed(0)
        frames = torch.randint(0, 256, (n, fs), generator=gen, dtype=torch.uint8)
        if depth > 8:
            frames[:, 1::2] &= (1 << (depth - 8)) - 1  # little-endian words below 2^depth
        buf = torch.zeros((n, fs + 6), dtype=torch.uint8, device=dev)
        buf[:, 6:] = frames.to(dev)
        yuv = buf[:, 6:]
        decode_bytes = n * (fs + 12 * H * W)
        dec = timed(lambda: ops.yuv_to_rgb(yuv, H, W, fmt, 'bt709', 'limited'), args.warmup, args.iters)
        for mode in ('field', 'frame'):
            n_out = 2 * n if mode == 'field' else n
            out = torch.empty((n_out, fs), dtype=torch.uint8, device=dev)
            assert torch.equal(ops.deinterlace(yuv, H, W, fmt, mode=mode, out=out), ops.deinterlace(yuv.contiguous(), H, W, fmt, mode=mode))
            booked, hbm = n_out * fs * (1.0 + ops.DEINT_ROWS_READ), (n + n_out) * fs
            first = timed(lambda: ops.deinterlace(yuv, H, W, fmt, mode=mode, out=out), args.warmup, args.iters)
            second = timed(lambda: ops.deinterlace(yuv, H, W, fmt, mode=mode, out=out), 5, args.iters)  # twice: the first ran on a colder device
            med = min(first[0], second[0])
            row = dict(case=name, frames=n, size=[H, W], format=fmt, mode=mode, frames_out=n_out, us=round(med, 2),
                       us_runs=[round(first[0], 2), round(second[0], 2)], us_min_max=[round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)],
                       bytes_booked=booked, booked_hbm_fraction=round(booked / (med * 1e-6) / (HBM_TBS * 1e12), 4),
                       bytes_hbm=hbm, hbm_fraction=round(hbm / (med * 1e-6) / (HBM_TBS * 1e12), 4),
                       decode_us=round(dec[0], 2), decode_us_min_max=[round(dec[1], 2), round(dec[2], 2)], decode_bytes=decode_bytes,
                       decode_hbm_fraction=round(decode_bytes / (dec[0] * 1e-6) / (HBM_TBS * 1e12), 4), over_decode=round(med / dec[0], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def video_row(args, dev):
    """restore_y4m(deinterlace='field') on a resident 576i stream against the same output frames fed as Ip: EDVR-L, chunk 10."""
    from edvr_amd import EDVR, ops
    from edvr_amd.y4m import restore_y4m
    H, W, n, chunk = 576, 720, args.video_frames, 10
    torch.manual_seed(10)
    net = EDVR(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None).to(dev).eval()
    fs = ops.yuv420_frame_size(H, W)
    # a smooth moving picture, woven: random samples would make the network's offsets run away
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    fields = [((torch.sin((xx + 3 * t) / 17.0) * torch.cos(yy / 23.0) * 90 + 128).clamp(0, 255)).to(torch.uint8) for t in range(2 * n)]
    frames = torch.full((n, fs), 128, dtype=torch.uint8)
    for i in range(n):
        luma = fields[2 * i].clone()
        luma[1::2] = fields[2 * i + 1][1::2]
        frames[i, :H * W] = luma.reshape(-1)
    woven = f'YUV4MPEG2 W{W} H{H} F25:1 It A1:1 C420jpeg\n'.encode() + b''.join(b'FRAME\n' + f.numpy().tobytes() for f in frames)
    prog = ops.deinterlace(frames.to(dev), H, W, '420', mode='field').cpu()
    plain = f'YUV4MPEG2 W{W} H{H} F50:1 Ip A1:1 C420jpeg\n'.encode() + b''.join(b'FRAME\n' + f.numpy().tobytes() for f in prog)

    def run(data, **kw):
        src, dst = io.BytesIO(data), io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = restore_y4m(net, src, dst, chunk=chunk, read_frames=chunk, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert got == 2 * n
        return got / dt, dst.getvalue()

    with torch.no_grad():
        _, a = run(woven, deinterlace='field')
        _, b = run(plain)
        assert a == b, 'the two arms write the same stream'
        deint, prog_fps = [], []
        for _ in range(3):
            prog_fps.append(run(plain)[0])
            deint.append(run(woven, deinterlace='field')[0])
    net.check_offsets()
    row = dict(case='EDVR-L T5 576i (720 x 576) field rate', frames_in=n, frames_out=2 * n, chunk=chunk, progressive_fps_runs=[round(v, 3) for v in prog_fps],
               deinterlace_fps_runs=[round(v, 3) for v in deint], progressive_fps=round(statistics.median(prog_fps), 3),
               deinterlace_fps=round(statistics.median(deint), 3),
               progressive_spread=round((max(prog_fps) - min(prog_fps)) / statistics.median(prog_fps), 4),
               deinterlace_over_progressive=round(statistics.median(deint) / statistics.median(prog_fps), 4))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'deint', 'bench_deinterlace.json'))
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--video-frames', type=int, default=10, help='input frames of the restore_y4m arm (twice as many leave)')
    ap.add_argument('--skip-video', action='store_true', help='kernels only')
    ap.add_argument('--head', default=None, help='commit to record where the tree is not a git checkout (default: git rev-parse HEAD)')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_deinterlace needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_deinterlace', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(),
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
