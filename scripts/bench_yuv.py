"""Times the Y'CbCr <-> RGB kernels (csrc/yuv.hip) and the Y4M path built on them.

  (a) ops.yuv420_to_rgb (bilinear chroma) and ops.rgb_to_yuv420, float32 RGB and (the *_u8_* arms) uint8 RGB, on 8 frames of 180 x 320 and
      720 x 1280 and one of 2160 x 3840, each on a dense 16-byte-aligned batch and inside a Y4M buffer (stride framesize + 6, 6 bytes in:
      scalar accesses on the YUV side): device events around one call (launch included) after warm-up, the median, the bytes actually moved
      (frame bytes + RGB bytes, each once) and the share of the 6.29 TB/s measured HBM rate they amount to;
  (b) a stock-torch composition of the same definition on the device (slicing, repeat_interleave-free index arithmetic, separate mul /
      add, clamp, round) as a TIMING arm only;
  (c) restore_y4m on an in-memory Y4M of 100 frames of 180 x 320 (EDVR-L as trained, T = 5, chunk 10) in frames/s, host clock around the call
      ending in a synchronise, against VideoRestorer.restore on resident float32 frames - the parent's path - alternated, three runs each, so
      that the spread of the resident arm is known before the difference is read.

  (d) with --formats, INSTEAD of (a) - (c): ops.yuv_to_rgb (bilinear chroma) and ops.rgb_to_yuv for '420p10', '422p10', '444p10' and '420'
      on 8 frames of 720 x 1280 and one of 2160 x 3840 in a dense 16-byte-aligned batch, timed as (a); beside them, in the same process and
      at the same shapes, ops.yuv420_to_rgb / ops.rgb_to_yuv420, which reach the same kernels as the '420' row through the 8-bit 4:2:0
      entry points.  Printed, and written where --out names a file: profiles/yuv/bench_yuv_formats.json is the record of the commit that
      still had a kernel file per operator pair and is not overwritten by default.

  (e) with --siting, INSTEAD of (a) - (d): ops.yuv_to_rgb (bilinear chroma) and ops.rgb_to_yuv under every chroma siting ('center',
      'left', 'topleft') for '420', '420p10' and '422p10' at the shapes of (d), timed as (a), each siting's time beside
      'center' of the same process.  Written to profiles/yuv/bench_yuv_siting.json by default.

Legs (a) - (d): only public ops calls that every revision with both operator pairs has, so the same file times an older tree for a
comparison.

    python scripts/bench_yuv.py [--out profiles/yuv/bench_yuv.json] [--skip-video]
    python scripts/bench_yuv.py --formats [--out FILE]
    python scripts/bench_yuv.py --siting [--out profiles/yuv/bench_yuv_siting.json]
    python scripts/bench_yuv.py ... --tree DIR     the package of another checkout (built), for scripts/bench_yuv_compare.py
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

HBM_TBS = 6.29
CASES = [('8x180x320', 8, (180, 320)), ('8x720x1280', 8, (720, 1280)), ('1x2160x3840', 1, (2160, 3840))]


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


def stock_decode(yuv, H, W, mi, off):
    """The definition with stock torch ops on the device (bilinear chroma, float32 output): a timing arm."""
    n, hc, wc = yuv.shape[0], (H + 1) // 2, (W + 1) // 2
    y = yuv[:, :H * W].reshape(n, H, W).float()

    def up(c, dim, size):
        k = c.shape[dim]
        idx = torch.arange(k, device=c.device)
        prev, nxt = c.index_select(dim, (idx - 1).clamp(min=0)), c.index_select(dim, (idx + 1).clamp(max=k - 1))
        out = torch.stack([prev * 0.25 + c * 0.75, c * 0.75 + nxt * 0.25], dim + 1)
        shape = list(c.shape)
        shape[dim] = 2 * k
        return out.reshape(shape).narrow(dim, 0, size)
    d = [y - off[0]]
    for p in (0, 1):
        c = yuv[:, H * W + p * hc * wc:H * W + (p + 1) * hc * wc].reshape(n, hc, wc).float()
        d.append(up(up(c, 1, H), 2, W) - off[1 + p])
    v = torch.stack([(mi[k][0] * d[0] + mi[k][1] * d[1]) + mi[k][2] * d[2] for k in range(3)], 1)
    return v.clamp(0.0, 255.0) / 255.0


def stock_encode(rgb, m, off):
    n, _, H, W = rgb.shape
    x = rgb.clamp(0.0, 1.0) * 255.0
    p = [((m[k][0] * x[:, 0] + m[k][1] * x[:, 1]) + m[k][2] * x[:, 2]) + off[k] for k in range(3)]
    planes = [p[0].clamp(0.0, 255.0).round().to(torch.uint8).reshape(n, -1)]
    for k in (1, 2):
        q = torch.nn.functional.pad(p[k][:, None], (0, W % 2, 0, H % 2), mode='replicate')[:, 0]
        s = ((q[:, 0::2, 0::2] + q[:, 0::2, 1::2]) + (q[:, 1::2, 0::2] + q[:, 1::2, 1::2])) * 0.25
        planes.append(s.clamp(0.0, 255.0).round().to(torch.uint8).reshape(n, -1))
    return torch.cat(planes, 1)


def git_head(tree):
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=tree, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def kernel_rows(args, dev):
    from edvr_amd import ops
    m, mi, off = ops.yuv_coeffs('bt709', 'limited')
    rows = []
    for name, n, (H, W) in CASES:
        fs = ops.yuv420_frame_size(H, W)
        gen = torch.Generator().manual_seed(0)
        frames = torch.randint(0, 256, (n, fs), generator=gen, dtype=torch.uint8).to(dev)
        y4m = torch.zeros((n, fs + 6), dtype=torch.uint8, device=dev)
        y4m[:, 6:] = frames
        rgb = ops.yuv420_to_rgb(frames, H, W, 'bt709', 'limited')
        rgb8 = ops.yuv420_to_rgb(frames, H, W, 'bt709', 'limited', 'bilinear', torch.uint8)
        assert torch.equal(rgb, ops.yuv420_to_rgb(y4m[:, 6:], H, W, 'bt709', 'limited'))
        assert torch.equal(rgb8, ops.yuv420_to_rgb(y4m[:, 6:], H, W, 'bt709', 'limited', 'bilinear', torch.uint8))
        assert torch.equal(ops.rgb_to_yuv420(rgb8, 'bt709', 'limited'), ops.rgb_to_yuv420(rgb8, 'bt709', 'limited', out=y4m[:, 6:]))
        assert torch.equal(ops.rgb_to_yuv420(rgb, 'bt709', 'limited'), ops.rgb_to_yuv420(rgb, 'bt709', 'limited', out=y4m[:, 6:]))
        parity_dec = (rgb - stock_decode(frames, H, W, mi, off)).abs().max().item()
        parity_enc = (ops.rgb_to_yuv420(rgb, 'bt709', 'limited').int() - stock_encode(rgb, m, off).int()).abs().max().item()
        nbytes, nbytes_u8 = n * (fs + 12 * H * W), n * (fs + 3 * H * W)
        arms = {
            'decode_dense': lambda: ops.yuv420_to_rgb(frames, H, W, 'bt709', 'limited'),
            'decode_y4m': lambda: ops.yuv420_to_rgb(y4m[:, 6:], H, W, 'bt709', 'limited'),
            'encode_dense': lambda: ops.rgb_to_yuv420(rgb, 'bt709', 'limited', out=frames),
            'encode_y4m': lambda: ops.rgb_to_yuv420(rgb, 'bt709', 'limited', out=y4m[:, 6:]),
            'decode_u8_dense': lambda: ops.yuv420_to_rgb(frames, H, W, 'bt709', 'limited', 'bilinear', torch.uint8),
            'decode_u8_y4m': lambda: ops.yuv420_to_rgb(y4m[:, 6:], H, W, 'bt709', 'limited', 'bilinear', torch.uint8),
            'encode_u8_dense': lambda: ops.rgb_to_yuv420(rgb8, 'bt709', 'limited', out=frames),
            'encode_u8_y4m': lambda: ops.rgb_to_yuv420(rgb8, 'bt709', 'limited', out=y4m[:, 6:]),
        }
        row = dict(case=name, frames=n, size=[H, W], bytes_moved=nbytes, bytes_moved_u8=nbytes_u8, stock_decode_max_abs_diff=parity_dec,
                   stock_encode_max_abs_diff=parity_enc)
        for arm, fn in arms.items():
            moved = nbytes_u8 if '_u8_' in arm else nbytes
            first, second = timed(fn, args.warmup, args.iters), timed(fn, 5, args.iters)  # twice: the first ran on a colder device
            med = min(first[0], second[0])
            row[arm + '_us'] = round(med, 2)
            row[arm + '_us_runs'] = [round(first[0], 2), round(second[0], 2)]
            row[arm + '_us_min_max'] = [round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)]
            row[arm + '_hbm_fraction'] = round(moved / (med * 1e-6) / (HBM_TBS * 1e12), 4)
        row['stock_decode_us'] = round(timed(lambda: stock_decode(frames, H, W, mi, off), 5, max(20, args.iters // 4))[0], 2)
        row['stock_encode_us'] = round(timed(lambda: stock_encode(rgb, m, off), 5, max(20, args.iters // 4))[0], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


FORMAT_CASES = [('8x720x1280', 8, (720, 1280)), ('1x2160x3840', 1, (2160, 3840))]
FORMATS = ['420p10', '422p10', '444p10', '420']


def format_rows(args, dev):
    """Leg (d): one row per shape and format through ops.yuv_to_rgb / ops.rgb_to_yuv, and one per shape through ops.yuv420_to_rgb /
    ops.rgb_to_yuv420."""
    from edvr_amd import ops
    rows = []

    def measure(row, arms, nbytes):
        for arm, fn in arms.items():
            first, second = timed(fn, args.warmup, args.iters), timed(fn, 5, args.iters)  # twice: the first ran on a colder device
            med = min(first[0], second[0])
            row[arm + '_us'] = round(med, 2)
            row[arm + '_us_runs'] = [round(first[0], 2), round(second[0], 2)]
            row[arm + '_us_min_max'] = [round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)]
            row[arm + '_hbm_fraction'] = round(nbytes / (med * 1e-6) / (HBM_TBS * 1e12), 4)
        rows.append(row)
        print(json.dumps(row), flush=True)

    for name, n, (H, W) in FORMAT_CASES:
        gen = torch.Generator().manual_seed(0)
        rgb = torch.rand((n, 3, H, W), generator=gen).to(dev)
        frames8 = ops.rgb_to_yuv420(rgb, 'bt709', 'limited')
        fs8 = ops.yuv420_frame_size(H, W)
        measure(dict(case=name, frames=n, size=[H, W], ops='yuv420_to_rgb / rgb_to_yuv420', format='420', bytes_moved=n * (fs8 + 12 * H * W)),
                {'decode': lambda: ops.yuv420_to_rgb(frames8, H, W, 'bt709', 'limited'),
                 'encode': lambda: ops.rgb_to_yuv420(rgb, 'bt709', 'limited', out=frames8)}, n * (fs8 + 12 * H * W))
        for fmt in FORMATS:
            fs = ops.yuv_frame_size(H, W, fmt)
            frames = ops.rgb_to_yuv(rgb, fmt, 'bt709', 'limited')
            if fmt == '420':
                assert torch.equal(frames, frames8) and torch.equal(ops.yuv_to_rgb(frames, H, W, fmt, 'bt709', 'limited'),
                                                                    ops.yuv420_to_rgb(frames8, H, W, 'bt709', 'limited'))
            measure(dict(case=name, frames=n, size=[H, W], ops='yuv_to_rgb / rgb_to_yuv', format=fmt, bytes_moved=n * (fs + 12 * H * W)),
                    {'decode': lambda: ops.yuv_to_rgb(frames, H, W, fmt, 'bt709', 'limited'),
                     'encode': lambda: ops.rgb_to_yuv(rgb, fmt, 'bt709', 'limited', out=frames)}, n * (fs + 12 * H * W))
    return rows


SITING_FORMATS = ['420', '420p10', '422p10']
SITINGS = ['center', 'left', 'topleft']


def siting_rows(args, dev):
    """Leg (e): one row per shape, format and siting through ops.yuv_to_rgb / ops.rgb_to_yuv; `*_over_center` is the ratio to the
    'center' row of the same shape and format ('topleft' on 4:2:2 is 'left': the same launch, timed again)."""
    from edvr_amd import ops
    rows = []
    for name, n, (H, W) in FORMAT_CASES:
        rgb = torch.rand((n, 3, H, W), generator=torch.Generator().manual_seed(0)).to(dev)
        for fmt in SITING_FORMATS:
            fs = ops.yuv_frame_size(H, W, fmt)
            nbytes = n * (fs + 12 * H * W)
            frames = ops.rgb_to_yuv(rgb, fmt, 'bt709', 'limited')
            base = {}
            for siting in SITINGS:
                row = dict(case=name, frames=n, size=[H, W], format=fmt, siting=siting, bytes_moved=nbytes)
                arms = {'decode': lambda: ops.yuv_to_rgb(frames, H, W, fmt, 'bt709', 'limited', 'bilinear', siting),
                        'encode': lambda: ops.rgb_to_yuv(rgb, fmt, 'bt709', 'limited', out=frames, siting=siting)}
                for arm, fn in arms.items():
                    first, second = timed(fn, args.warmup, args.iters), timed(fn, 5, args.iters)  # twice: the first ran on a colder device
                    med = min(first[0], second[0])
                    row[arm + '_us'] = round(med, 2)
                    row[arm + '_us_runs'] = [round(first[0], 2), round(second[0], 2)]
                    row[arm + '_hbm_fraction'] = round(nbytes / (med * 1e-6) / (HBM_TBS * 1e12), 4)
                    base.setdefault(arm, med)
                    row[arm + '_over_center'] = round(med / base[arm], 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def video_row(args, dev):
    """restore_y4m against VideoRestorer.restore on resident frames: 100 frames of 180 x 320, EDVR-L, chunk 10."""
    from edvr_amd import EDVR, VideoRestorer, ops
    from edvr_amd.y4m import restore_y4m
    H, W, n, chunk = 180, 320, args.video_frames, 10
    torch.manual_seed(10)
    net = EDVR(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None).to(dev).eval()
    fs = ops.yuv420_frame_size(H, W)
    frames = torch.randint(0, 256, (n, fs), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    head = f'YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C420jpeg\n'.encode()
    data = head + b''.join(b'FRAME\n' + f.numpy().tobytes() for f in frames)
    resident = ops.yuv420_to_rgb(frames.to(dev), H, W)

    def run_resident():
        vr = VideoRestorer(net, chunk=chunk, out_dtype=torch.float32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = vr.restore(resident)
        torch.cuda.synchronize()
        del out
        return n / (time.perf_counter() - t0)

    def run_y4m():
        src, dst = io.BytesIO(data), io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = restore_y4m(net, src, dst, chunk=chunk, read_frames=chunk)
        torch.cuda.synchronize()
        assert got == n
        return n / (time.perf_counter() - t0)

    with torch.no_grad():
        run_resident(), run_y4m()  # warm-up of every shape
        res, y4m = [], []
        for _ in range(3):
            res.append(run_resident())
            y4m.append(run_y4m())
    net.check_offsets()
    row = dict(case='EDVR-L T5 180x320', frames=n, chunk=chunk, resident_fps_runs=[round(v, 2) for v in res], y4m_fps_runs=[round(v, 2) for v in y4m],
               resident_fps=round(statistics.median(res), 2), y4m_fps=round(statistics.median(y4m), 2),
               resident_spread=round((max(res) - min(res)) / statistics.median(res), 4),
               y4m_over_resident=round(statistics.median(y4m) / statistics.median(res), 4),
               copied_bytes_per_frame=fs + 6 + ops.yuv420_frame_size(4 * H, 4 * W) + 6)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='default: profiles/yuv/bench_yuv.json; with --formats none, the rows are only printed')
    ap.add_argument('--tree', default=os.path.join(HERE, '..'), help='the checkout whose edvr_amd package is timed (default: this one)')
    ap.add_argument('--formats', action='store_true', help='leg (d) alone: the operators that take a format beside the 8-bit 4:2:0 operators')
    ap.add_argument('--siting', action='store_true', help='leg (e) alone: decode and encode under every chroma siting')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--video-frames', type=int, default=100)
    ap.add_argument('--skip-video', action='store_true', help='kernels only')
    ap.add_argument('--head', default=None, help='commit to record where the tree is not a git checkout (default: git rev-parse HEAD)')
    args = ap.parse_args()
    if args.out is None and not args.formats:
        args.out = os.path.join(HERE, '..', 'profiles', 'yuv', 'bench_yuv_siting.json' if args.siting else 'bench_yuv.json')
    sys.path.insert(0, os.path.abspath(args.tree))
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_yuv needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_yuv', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(), git_head=args.head or git_head(os.path.abspath(args.tree)),
                  device=torch.cuda.get_device_name(0), hbm_tbs=HBM_TBS, warmup=args.warmup, iters=args.iters)
    if args.siting:
        record['bench'], record['sitings'] = 'bench_yuv_siting', siting_rows(args, dev)
    elif args.formats:
        record['bench'], record['formats'] = 'bench_yuv_formats', format_rows(args, dev)
    else:
        record['kernels'] = kernel_rows(args, dev)
    if not args.skip_video and not args.formats and not args.siting:
        record['restore_y4m'] = video_row(args, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
        print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
