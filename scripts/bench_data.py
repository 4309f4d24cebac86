"""Input-pipeline throughput on REDS-sized frames (180x320 LQ, 720x1280 GT PNGs): clips/s of plan + decode + byte crop into
staging for a number of decode threads (--host-only, runs without a GPU), or of the whole REDSDeviceLoader incl. the H2D copy
and edvr_frames_u8_to_f32 on the device.  The consumer to keep fed is the training step: 32 clips / 182 ms = 176 clips/s/GPU.

--lq-windows measures training from GT frames alone (opt lq_from_gt; ops.lq_crops_from_windows) and writes --out
(profiles/data/bench_lq_windows.json): (1) the windowed kernel on one EDVR-L training batch (32 samples x 5 frames, gt_size 256, x4) for
BI and BD against what the full-frame kernel offers for the same crops - the same 160 frames at 720 x 1280, then slicing - device events
around repeated calls, the two alternating; (2) samples/s of the device loader with an LQ tree and without one on the same PNG tree."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def make_dataset(root, clips, frames):
    from PIL import Image
    rs = np.random.RandomState(0)
    for kind, (h, w) in (('lq', (180, 320)), ('gt', (720, 1280))):
        yy, xx = np.mgrid[0:h, 0:w]
        for c in clips:
            d = os.path.join(root, kind, c)
            os.makedirs(d, exist_ok=True)
            for f in range(frames):
                if kind == 'gt' and f >= 8:  # 8 distinct 720p frames, hard-linked for the rest (encode time; decode cost is the same)
                    os.link(os.path.join(d, f'{f % 8:08d}.png'), os.path.join(d, f'{f:08d}.png'))
                    continue
                # smooth content + mild noise: PNG sizes (and decode cost) in the range of natural frames, not of white noise
                img = np.stack([(yy * 255 // h + f) % 256, (xx * 255 // w + 2 * f) % 256, ((yy + xx) // 4 + f) % 256], -1)
                img = (img + rs.randint(0, 6, img.shape)).clip(0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(d, f'{f:08d}.png'), compress_level=3)
    meta = os.path.join(root, 'meta_info.txt')
    with open(meta, 'w') as fh:
        fh.writelines(f'{c} {frames} (720,1280,3)\n' for c in clips)
    return meta


HBM_BYTES_PER_S = 6.29e12  # measured copy bandwidth of one MI355X, the denominator of every "fraction of HBM" here


def bench_lq_windows(a):
    import json
    import torch
    from edvr_amd import build, data as D, ops
    dev = torch.device('cuda')
    samples, t, P, s = 32, 5, 256, 4
    n, p, H, W = samples * t, P // s, 720, 1280
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    tops = torch.randint(0, H // s - p + 1, (n,), generator=g).tolist()
    lefts = torch.randint(0, W // s - p + 1, (n,), generator=g).tolist()
    report = {'shape': f'{samples} samples x {t} frames, gt_size {P}, x{s}: {n} crops of {p} x {p} from {H} x {W} frames', 'kernel': {}, 'loader': {},
              'csrc_sha16': build.source_hash(), 'device': torch.cuda.get_device_name(0)}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per call

    for degradation in D.DEGRADATIONS:
        e = D.lq_window_extent(p, s, degradation)
        pitch = D.lq_window_pitch(e)
        win = torch.zeros(n, e, pitch, dtype=torch.uint8, device=dev)
        tab = torch.zeros(n, D.LQ_WINDOW_RECORD_INTS, dtype=torch.int32)
        for i in range(n):
            y0 = D.lq_window_origin(D.lq_window(tops[i], p, H // s, s, degradation)[0], H, e)
            x0 = D.lq_window_origin(D.lq_window(lefts[i], p, W // s, s, degradation)[0], W, e)
            win[i, :, :3 * e] = frames[i, y0:y0 + e, x0:x0 + e].reshape(e, 3 * e)
            tab[i, :6] = torch.tensor([y0, x0, H, W, tops[i], lefts[i]], dtype=torch.int32)
        tab_d = tab.to(dev)
        whole = (lambda: ops.imresize(frames, 1 / s, out_dtype=torch.uint8)) if degradation == 'bi' else (lambda: ops.bd_downsample(frames, s, out_dtype=torch.uint8))

        def full_frame():
            lq = whole()
            return torch.stack([lq[i, tops[i]:tops[i] + p, lefts[i]:lefts[i] + p] for i in range(n)])

        windowed = lambda: ops.lq_crops_from_windows(win, tab_d, s, degradation, table_host=tab)
        assert torch.equal(windowed(), full_frame()), degradation  # the same bytes, at the size that is timed
        for _ in range(3):
            windowed(), whole()
        torch.cuda.synchronize()
        rounds = [(timed(windowed, 200), timed(whole, 5), timed(full_frame, 3)) for _ in range(a.rounds)]  # alternating
        w_us, f_us, fs_us = (sorted(r[k] for r in rounds) for k in range(3))
        med = lambda v: v[len(v) // 2]
        nbytes = 3.0 * n * (e * e + p * p) + 4.0 * tab.numel()
        report['kernel'][degradation] = {
            'window_extent': e, 'row_pitch_bytes': pitch, 'algorithmic_bytes': nbytes, 'staged_bytes': n * e * pitch + 4 * tab.numel(),
            'windowed_us': round(med(w_us), 2), 'windowed_us_min_max': [round(w_us[0], 2), round(w_us[-1], 2)],
            'full_frame_kernel_us': round(med(f_us), 1), 'full_frame_kernel_us_min_max': [round(f_us[0], 1), round(f_us[-1], 1)],
            'full_frame_then_slicing_us': round(med(fs_us), 1),
            'ratio_full_frame_kernel_over_windowed': round(med(f_us) / med(w_us), 1),
            'ratio_full_frame_then_slicing_over_windowed': round(med(fs_us) / med(w_us), 1),
            'windowed_fraction_of_hbm': round(nbytes / (med(w_us) * 1e-6) / HBM_BYTES_PER_S, 4),
            'note': 'events around repeated calls: host enqueue included; at this size the launch is expected to be launch- and latency-bound'}
        print(degradation, json.dumps(report['kernel'][degradation]), flush=True)
    del frames
    # ---- loader: the same PNG tree with its LQ folder and without
    consumer = None
    bench = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'BENCH_r06.json')
    if os.path.exists(bench):  # the training it/s is inside the recorded output line of bench.py
        import re
        m = re.search(r'train\\*":\s*\{\\*"iters_per_sec\\*":\s*([0-9.]+)', open(bench).read())
        consumer = 32 * float(m.group(1)) if m else None
    with tempfile.TemporaryDirectory() as root:
        meta = make_dataset(root, ['001'], 100)
        tree = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
                    io_backend=dict(type='disk'), gt_size=P, scale=s, num_frame=t, interval_list=[1], random_reverse=False,
                    use_flip=True, use_rot=True, val_partition='REDS4')
        arms = {'lq_tree': tree, 'gt_only_bi': dict(tree, dataroot_lq=None, lq_from_gt=dict(scale=s, degradation='bi')),
                'gt_only_bd': dict(tree, dataroot_lq=None, lq_from_gt=dict(scale=s, degradation='bd'))}
        rates = {k: [] for k in arms}
        for _ in range(a.rounds):  # alternating
            for name, opt in arms.items():
                loader = D.REDSDeviceLoader(opt, samples, ratio=100, seed=0, num_threads=a.threads[0])
                loader.next()
                torch.cuda.synchronize()
                t0 = time.time()
                for b in range(a.batches):
                    batch = loader.next()
                    assert batch['lq'].shape == (samples, t, 3, p, p)
                torch.cuda.synchronize()
                rates[name].append(a.batches * samples / (time.time() - t0))
                loader.close()
                print(f'{name}: {rates[name][-1]:.1f} samples/s', flush=True)
    for name, v in rates.items():
        v = sorted(v)
        report['loader'][name] = {'samples_per_s': round(v[len(v) // 2], 1), 'min_max': [round(v[0], 1), round(v[-1], 1)]}
    report['loader'].update(decode_threads=a.threads[0], batches_timed=a.batches, batch=samples, cpus=len(os.sched_getaffinity(0)),
                            training_step_consumes_samples_per_s=consumer and round(consumer, 1),
                            tree='synthetic PNG, 720 x 1280 GT and 180 x 320 LQ (make_dataset above), page cache warm')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(report, fh, indent=1)
        fh.write('\n')
    print(json.dumps(report['loader']), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--lq-windows', action='store_true', help='training from GT alone: windowed kernels and loader arms (needs a GPU)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'data', 'bench_lq_windows.json'))
    ap.add_argument('--threads', type=int, nargs='+', default=[1, 4, 8, 16, 32])
    ap.add_argument('--batches', type=int, default=6)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    if a.lq_windows:
        if a.threads == [1, 4, 8, 16, 32]:
            a.threads = [16]
        return bench_lq_windows(a)
    from edvr_amd import data as D
    import random
    from concurrent.futures import ThreadPoolExecutor
    with tempfile.TemporaryDirectory() as root:
        t0 = time.time()
        meta = make_dataset(root, ['001'], 100)
        gt_bytes = os.path.getsize(os.path.join(root, 'gt', '001', '00000000.png'))
        print(f'dataset written in {time.time() - t0:.1f}s; GT PNG {gt_bytes / 1e6:.2f} MB', flush=True)
        opt = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
                   io_backend=dict(type='disk'), gt_size=256, scale=4, num_frame=5, interval_list=[1], random_reverse=False,
                   use_flip=True, use_rot=True, val_partition='REDS4')
        for th in a.threads:
            if a.host_only:
                pl = D.REDSClipPlanner(opt)
                rng = random.Random(0)
                lq = np.empty((a.batch, 5, 64, 64, 3), np.uint8)
                gt = np.empty((a.batch, 1, 256, 256, 3), np.uint8)
                with ThreadPoolExecutor(th) as pool:
                    t0 = time.time()
                    for b in range(a.batches):
                        plans = [pl.plan(rng.randrange(len(pl)), rng) for _ in range(a.batch)]
                        list(pool.map(lambda q: pl.load(q[1], lq[q[0]], gt[q[0], 0]), enumerate(plans)))
                    dt = time.time() - t0
            else:
                import torch
                loader = D.REDSDeviceLoader(opt, a.batch, ratio=100, seed=0, num_threads=th)
                loader.next()
                torch.cuda.synchronize()
                t0 = time.time()
                for b in range(a.batches):
                    batch = loader.next()
                    assert batch['lq'].shape == (a.batch, 5, 3, 64, 64)
                torch.cuda.synchronize()
                dt = time.time() - t0
                loader.close()
            print(f'threads {th:3d}: {a.batches * a.batch / dt:8.1f} clips/s ({"host only" if a.host_only else "device loader"})', flush=True)


if __name__ == '__main__':
    main()
