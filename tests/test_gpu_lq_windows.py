"""-m gpu: LQ training crops made on the device from windows of the GT frames (ops.lq_crops_from_windows; csrc/resize.hip, csrc/bd.hip,
csrc/lq_window.h) - bit for bit the crops of the full-frame kernels, the reference's fixtures, the loader with and without an LQ tree,
scripts/train_reds.py --lq-from-gt, accounting and graph capture."""
import importlib.util
import math
import os
import shutil

import pytest
import torch

import util_bd
import util_imresize
from util_data import write_png_dataset, write_video_test_tree, write_vimeo_train_tree

pytestmark = pytest.mark.gpu
SCALES = (2, 3, 4)
# odd sizes, sizes whose rows leave the 16-byte load path of the full-frame kernels (3 W % 16 != 0 after the mod-crop), one that keeps it
FRAME_SIZES = [(37, 53), (57, 75), (101, 131), (277, 291), (272, 320)]


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bytes(h, w, seed):
    return torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _full_frame(frame, scale, degradation):
    """(H, W, 3) uint8 on the device -> the whole LQ frame's bytes, as scripts/make_lq.py makes them."""
    from edvr_amd import ops
    if degradation == 'bi':
        return ops.imresize(frame[None], 1 / scale, out_dtype=torch.uint8)[0]
    return ops.bd_downsample(frame[None], scale, out_dtype=torch.uint8)[0]


def _stage(frames, crops, p, scale, degradation, seed=0):
    """Host staging as the loader does it: crops = [(frame index, top, left)] -> windows (n, e, pitch) uint8 (row padding filled with
    noise: nothing may depend on it) and table (n, 8) int32, both on the host."""
    from edvr_amd import data as D
    e = D.lq_window_extent(p, scale, degradation)
    pitch = D.lq_window_pitch(e)
    win = torch.randint(0, 256, (len(crops), e, pitch), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    tab = torch.zeros(len(crops), D.LQ_WINDOW_RECORD_INTS, dtype=torch.int32)
    for i, (f, top, left) in enumerate(crops):
        H, W = frames[f].shape[:2]
        y0 = D.lq_window_origin(D.lq_window(top, p, H // scale, scale, degradation)[0], H, e)
        x0 = D.lq_window_origin(D.lq_window(left, p, W // scale, scale, degradation)[0], W, e)
        win[i, :, :3 * e] = frames[f][y0:y0 + e, x0:x0 + e].reshape(e, 3 * e)
        tab[i, :6] = torch.tensor([y0, x0, H, W, top, left], dtype=torch.int32)
    return win, tab


def _positions(n, p):
    """Crop origins along an axis of n LQ samples: both ends, next to them, and the interior."""
    return sorted({0, min(1, n - p), (n - p) // 2, max(n - p - 1, 0), n - p})


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('p', [8, 16, 64])
def test_equals_the_crop_of_the_full_frame_kernel_bit_for_bit(gpu, degradation, scale, p):
    """Random frames of several sizes (each mod-cropped to the scale, as the loader does; every listed size the window of p fits into),
    crops at the four corners, on each edge and inside, ALL in one launch with their different tables: equal to the slice of the
    full-frame result."""
    from edvr_amd import data as D, ops
    e = D.lq_window_extent(p, scale, degradation)
    frames = [_bytes(h - h % scale, w - w % scale, 100 * p + 10 * scale + k) for k, (h, w) in enumerate(FRAME_SIZES)]
    frames = [f for f in frames if min(f.shape[:2]) >= e]
    assert len(frames) >= 2, 'every (p, scale) must meet frames of different sizes'
    crops = [(k, top, left) for k, f in enumerate(frames)
             for top in _positions(f.shape[0] // scale, p) for left in _positions(f.shape[1] // scale, p)]
    assert len(crops) >= 8
    win, tab = _stage(frames, crops, p, scale, degradation)
    got = ops.lq_crops_from_windows(win.to(gpu), tab.to(gpu), scale, degradation, table_host=tab)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(crops), p, p, 3)
    whole = [_full_frame(f.to(gpu), scale, degradation) for f in frames]
    bad = [(k, top, left) for i, (k, top, left) in enumerate(crops) if not torch.equal(got[i], whole[k][top:top + p, left:left + p])]
    print(f'{degradation} x{scale} p {p}: window {e}, {len(frames)} frames, {len(crops)} crops in one launch, {len(bad)} differ')
    assert not bad, bad
    # without the host copy of the table the launch checks less and computes the same
    assert torch.equal(ops.lq_crops_from_windows(win.to(gpu), tab.to(gpu), scale, degradation), got)


def _golden_cases(degradation):
    """(input (n, H, W, 3) uint8, reference output (n, 3, h, w) float, scale, float64 restatement, tolerance of the existing comparison)
    of every fixture whose frame is a multiple of its integer scale - what a mod-cropped training frame is."""
    out = []
    if degradation == 'bi':
        for case in util_imresize.load_golden():
            s = round(1 / case['scale'])
            H, W = case['input'].shape[:2]
            if case['antialiasing'] and s in SCALES and abs(case['scale'] - 1 / s) < 1e-12 and H % s == 0 and W % s == 0:
                x = case['input'][None]
                f64 = util_imresize.imresize_f64((x.float() / 255).permute(0, 3, 1, 2), 1 / s)
                out.append((x, case['output'][None], s, f64, 1e-5))  # test_gpu_imresize.py: TOL
    else:
        for case in util_bd.load_golden():
            s = case['scale']
            H, W = case['input'].shape[1:3]
            if H % s == 0 and W % s == 0:
                f64 = util_bd.bd_f64((case['input'].float() / 255).permute(0, 3, 1, 2), s)
                out.append((case['input'], case['output'], s, f64, 5e-6))  # test_gpu_bd.py: TOL_REF
    return out


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_crops_of_the_reference_outputs(gpu, degradation):
    """Against the reference's own outputs (tests/golden): the condition test_gpu_bd.py::test_bytes_match_the_reference_rounded holds the
    full-frame bytes to, unchanged - a byte differs from tensor2img of the reference's float by at most 1, and only where 255 x (the
    float64 value) lies within 255 x (that test's tolerance) of a half-integer.  For imresize the tolerance is the one
    test_gpu_imresize.py::test_matches_the_reference holds the float output to."""
    from edvr_amd import ops
    cases = _golden_cases(degradation)
    assert len(cases) >= 3
    for x, ref, s, f64, tol in cases:
        p = 8
        frames = list(x)
        crops = [(k, top, left) for k, f in enumerate(frames) for top in _positions(f.shape[0] // s, p) for left in _positions(f.shape[1] // s, p)]
        win, tab = _stage(frames, crops, p, s, degradation)
        got = ops.lq_crops_from_windows(win.to(gpu), tab.to(gpu), s, degradation, table_host=tab).cpu()
        want = util_bd.to_u8(ref).permute(0, 2, 3, 1)
        exact = 255 * f64.permute(0, 2, 3, 1)
        near_tie = ((exact - exact.floor()) - 0.5).abs() <= 255 * tol
        differ = ties = 0
        for i, (k, top, left) in enumerate(crops):
            sl = (k, slice(top, top + p), slice(left, left + p))
            diff = (got[i].int() - want[sl].int()).abs()
            differ, ties = differ + int((diff != 0).sum()), ties + int(near_tie[sl].sum())
            assert diff.max().item() <= 1 and not bool((diff != 0)[~near_tie[sl]].any()), (tuple(x.shape), s, k, top, left)
        print(f'{degradation} {tuple(x.shape)} x{s}: {differ} bytes of {got.numel()} differ from the rounded reference, {ties} near a tie')


def test_refusals(gpu):
    from edvr_amd import _lib, data as D, ops
    e = D.lq_window_extent(8, 4, 'bd')
    pitch = D.lq_window_pitch(e)
    frame = _bytes(64, 80, 1)
    win, tab = _stage([frame], [(0, 3, 5)], 8, 4, 'bd')
    wd, td = win.to(gpu), tab.to(gpu)
    launches = []
    hook, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, lambda name, *a: launches.append(name)
    try:
        with pytest.raises(NotImplementedError):
            ops.lq_crops_from_windows(win, td, 4, 'bd')
        with pytest.raises(NotImplementedError):
            ops.lq_crops_from_windows(wd, tab, 4, 'bd')
        with pytest.raises(NotImplementedError):
            ops.lq_crops_from_windows(wd.float(), td, 4, 'bd')
        for scale, degradation in ((8, 'bd'), (1, 'bi'), (5, 'bi'), (4, 'blur'), (4, 'bi')):  # the last: no crop has this extent
            with pytest.raises(ValueError):
                ops.lq_crops_from_windows(wd, td, scale, degradation)
        with pytest.raises(ValueError):
            ops.lq_crops_from_windows(wd[:, :, :3 * e], td, 4, 'bd')  # rows off 16 bytes
        with pytest.raises(ValueError):
            ops.lq_crops_from_windows(wd, td[:, :6], 4, 'bd')
    finally:
        ops.LAUNCH_HOOK = hook
    assert launches == []  # refused before any launch
    # ... and the C entry points refuse on their own: the scale, the window, and - given the host copy - every record of the table
    lib = _lib.lib()
    out = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=gpu)

    def call(fn, table_host=None, p=8, wh=e, ww=e, pitch=pitch, scale=4):
        host = table_host.data_ptr() if table_host is not None else None
        return getattr(lib, fn)(wd.data_ptr(), td.data_ptr(), host, out.data_ptr(), 1, p, wh, ww, pitch, scale, None)

    for fn in ('edvr_bd_downsample_u8_windows', 'edvr_imresize_bicubic_u8_windows'):
        assert call(fn, scale=8) < 0 and b'not 2, 3 or 4' in lib.edvr_last_error()
        assert call(fn, scale=1) < 0 and b'not 2, 3 or 4' in lib.edvr_last_error()
        assert call(fn, wh=e + 1) < 0 and b'extent' in lib.edvr_last_error()
        assert call(fn, pitch=3 * e) < 0
    fn = 'edvr_bd_downsample_u8_windows'
    assert call(fn, pitch=pitch + 8) < 0 and b'16-byte' in lib.edvr_last_error()
    for col, value, why in ((2, 63, b'multiple of the scale'), (2, 40, b'smaller than the window'), (4, 9, b'crop leaves'), (5, -1, b'crop leaves'),
                            (0, 64 - e + 1, b'window leaves'), (1, -1, b'window leaves'), (0, int(tab[0, 0]) + 1, b'does not hold'),
                            (1, int(tab[0, 1]) - 1, b'does not hold')):
        bad = tab.clone()
        bad[0, col] = value
        assert call(fn, bad) < 0 and why in lib.edvr_last_error(), (col, value, lib.edvr_last_error())
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0  # nothing was launched
    assert call(fn, tab) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0], _full_frame(frame.to(gpu), 4, 'bd')[3:11, 5:13])


def test_launch_is_booked_with_algorithmic_bytes(gpu):
    from edvr_amd import data as D, ops
    seen = []

    def hook(name, flops, launch, nbytes, executed):
        seen.append((name, nbytes))
        launch()

    frames = [_bytes(64, 96, 1), _bytes(60, 80, 2)]
    crops = [(0, 0, 0), (1, 3, 4), (0, 8, 16)]
    prev, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, hook
    try:
        for degradation in ('bi', 'bd'):
            win, tab = _stage(frames, crops, 8, 4, degradation)
            ops.lq_crops_from_windows(win.to(gpu), tab.to(gpu), 4, degradation)
    finally:
        ops.LAUNCH_HOOK = prev
    e_bi, e_bd = D.lq_window_extent(8, 4, 'bi'), D.lq_window_extent(8, 4, 'bd')
    assert (e_bi, e_bd) == (44, 41)
    # window pixels and table read, crops written - not the padding of the rows
    assert seen == [('lq_crops_from_windows', 3 * (44 * 44 * 3 + 8 * 4 + 8 * 8 * 3.0)), ('lq_crops_from_windows', 3 * (41 * 41 * 3 + 8 * 4 + 8 * 8 * 3.0))]


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_graph_replay_equals_eager(gpu, degradation):
    """Captured once and replayed on new pixels and a new table in the same buffers: the bytes of the eager call."""
    from edvr_amd import ops
    frames = [_bytes(64, 96, 3), _bytes(72, 80, 4)]
    win_a, tab_a = _stage(frames, [(0, 0, 0), (1, 10, 12), (0, 8, 16), (1, 2, 0)], 8, 4, degradation)
    win_b, tab_b = _stage(frames, [(1, 9, 1), (0, 8, 7), (1, 0, 12), (0, 3, 3)], 8, 4, degradation, seed=1)
    win, tab = win_a.to(gpu), tab_a.to(gpu)
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(stream):
        ops.lq_crops_from_windows(win, tab, 4, degradation)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = ops.lq_crops_from_windows(win, tab, 4, degradation)
    win.copy_(win_b), tab.copy_(tab_b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.lq_crops_from_windows(win_b.to(gpu), tab_b.to(gpu), 4, degradation, table_host=tab_b))
    assert not torch.equal(out, ops.lq_crops_from_windows(win_a.to(gpu), tab_a.to(gpu), 4, degradation))


def _meta(path, clips, frames):
    with open(path, 'w') as fh:
        fh.writelines(f'{clip} {frames} (64,80,3)\n' for clip in clips)
    return str(path)


def _batches(opt, gpu, world, rank, epochs=2):
    from edvr_amd import data as D
    loader = D.REDSDeviceLoader(opt, 4, device=gpu, rank=rank, world_size=world, seed=7, num_threads=4, depth=2)
    out = []
    try:
        for epoch in range(epochs):
            if epoch:
                loader.reset(epoch)
            while True:
                b = loader.next()
                if b is None:
                    break
                out.append((b['lq'].clone(), b['gt'].clone(), list(b['key'])))
        torch.cuda.synchronize()
    finally:
        loader.close()
    return out


def _flags_seen(opt, world, rank, epochs=2):
    """The augmentation flags of the same epochs, from the planner, sampler and random stream the loader uses."""
    from edvr_amd import data as D
    planner = D.make_planner(opt)
    sampler = D.EnlargedSampler(planner, world, rank)
    flags = set()
    for epoch in range(epochs):
        sampler.set_epoch(epoch)
        rng = D.epoch_rng(7 + rank, epoch)
        if hasattr(planner, 'reset_epoch'):
            planner.reset_epoch()
        flags |= {planner.plan(i, rng).flags for i in sampler}
    return flags


def _assert_same_batches(with_tree, gt_only):
    assert len(with_tree) == len(gt_only) > 0
    for (lq_a, gt_a, key_a), (lq_b, gt_b, key_b) in zip(with_tree, gt_only):
        assert key_a == key_b
        assert lq_a.shape == lq_b.shape and torch.equal(lq_a, lq_b), key_a
        assert torch.equal(gt_a, gt_b), key_a


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_loader_equals_the_loader_on_a_stored_lq_tree(gpu, tmp_path, degradation):
    """The end-to-end witness: a GT tree, its x4 LQ tree written by scripts/make_lq.py's own function, and the device loader once on
    both trees and once on the GT tree alone - every batch of two epochs, for one rank and for each of two, is the same tensors."""
    make_lq = _load_script('make_lq')
    root = str(tmp_path)
    write_png_dataset(root, ['001', '002'], (16, 20), 4, frames=100)
    shutil.rmtree(os.path.join(root, 'lq'))
    assert make_lq.make_lq(os.path.join(root, 'gt'), os.path.join(root, 'lq'), scale=4, device=gpu, log=lambda *a: None, degradation=degradation) == 200
    meta = _meta(tmp_path / 'meta_train.txt', ['001', '002'], 24)
    tree = dict(dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), dataroot_flow=None, meta_info_file=meta,
                io_backend=dict(type='disk'), gt_size=32, scale=4, num_frame=5, interval_list=[1, 2], random_reverse=True, use_flip=True,
                use_rot=True, val_partition='REDS4')
    gt_only = dict(tree, dataroot_lq=None, lq_from_gt=dict(scale=4, degradation=degradation))
    flags = set()
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        _assert_same_batches(_batches(tree, gpu, world, rank), _batches(gt_only, gpu, world, rank))
        flags |= _flags_seen(gt_only, world, rank)
    assert flags == set(range(8)), flags  # every combination of hflip, vflip and rot90 occurred


def test_vimeo_loader_equals_the_loader_on_a_stored_lq_tree(gpu, tmp_path):
    make_lq = _load_script('make_lq')
    root = str(tmp_path)
    keys = [f'{c:05d}/{q:04d}' for c in (1, 2) for q in range(1, 13)]
    meta = write_vimeo_train_tree(root, keys, (16, 28), 4)
    shutil.rmtree(os.path.join(root, 'lq'))
    for clip in ('00001', '00002'):  # make_lq walks <clip>/<frame>: one call per first-level folder of <clip>/<seq>/im*.png
        make_lq.make_lq(os.path.join(root, 'gt', clip), os.path.join(root, 'lq', clip), scale=4, device=gpu, log=lambda *a: None, degradation='bd')
    tree = dict(type='Vimeo90KDataset', dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'), meta_info_file=meta,
                io_backend=dict(type='disk'), num_frame=7, gt_size=32, scale=4, random_reverse=True, use_flip=True, use_rot=True)
    gt_only = dict(tree, dataroot_lq=None, lq_from_gt=dict(scale=4, degradation='bd'))
    flags = set()
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        _assert_same_batches(_batches(tree, gpu, world, rank), _batches(gt_only, gpu, world, rank))
        flags |= _flags_seen(gt_only, world, rank)
    assert flags == set(range(8)), flags


@pytest.mark.parametrize('degradation', ['bi', 'bd'])
def test_training_loop_without_an_lq_tree(gpu, tmp_path, degradation):
    """scripts/train_reds.py --lq-from-gt 4 on a GT tree alone (modelled on test_gpu_data.py::test_training_loop_from_png_folders):
    a few iterations, finite losses, validation from the GT folder, a checkpoint."""
    tr = _load_script('train_reds')
    root = str(tmp_path)
    meta = write_png_dataset(root, ['001', '002'], (20, 24), 4, frames=100)
    write_video_test_tree(os.path.join(root, 'val'), dict(folders=['000'], frames=6, lq_hw=(16, 20), scale=4))
    shutil.rmtree(os.path.join(root, 'lq'))
    shutil.rmtree(os.path.join(root, 'val', 'lq'))
    args = tr.parse_args(['--gt', os.path.join(root, 'gt'), '--meta', meta, '--lq-from-gt', '4', '--degradation', degradation,
                          '--val-gt', os.path.join(root, 'val', 'gt'), '--num-feat', '64', '--num-reconstruct-block', '2', '--gt-size', '64',
                          '--batch', '2', '--threads', '4', '--enlarge-ratio', '1', '--iters', '4', '--dcn-lr-mul', '0.25', '--periods', '4', '4',
                          '--restart-weights', '1', '0.5', '--tsa-iter', '3', '--print-freq', '1', '--save-freq', '4', '--val-freq', '4',
                          '--val-batch', '3', '--save-dir', os.path.join(root, 'ckpt')])
    lines = []
    losses = tr.train(args, log=lines.append)
    assert len(losses) == 4 and all(math.isfinite(v) and v > 0 for v in losses)
    assert any('validation PSNR' in ln for ln in lines)
    assert os.path.exists(os.path.join(root, 'ckpt', 'net_g_4.pth')) and os.path.exists(os.path.join(root, 'ckpt', '4.state'))
