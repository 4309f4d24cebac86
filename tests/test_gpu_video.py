"""-m gpu: the whole-video path (edvr_amd/video.py, csrc/video.hip): every frame's features extracted once, windows gathered from
a bounded bank - against the fp64 oracle, against the windowed path (metrics.validate_clip) and kernel by kernel."""
import logging

import numpy as np
import pytest
import torch

from util_edvr import CONFIGS, oracle_kwargs, randomize_offsets

pytestmark = pytest.mark.gpu

INTERMEDIATE_RTOL = 2e-4   # the project's whole-network bound (tests/test_gpu_edvr.py): fp32 HIP vs fp64 oracle, relative to max |ref|
PSNR_TOL_DB = 1e-3         # ... and its PSNR bound
BATCH_COMPOSITION_TOL = 3e-5  # test_batch_composition_changes_a_clip_only_within_the_conv_tolerance: the split-operand scale is taken
#                               over a different batch of images


def _net(name, seed=10):
    from edvr_amd import EDVR
    kwargs, shape = CONFIGS[name]
    torch.manual_seed(seed)
    return randomize_offsets(EDVR(**kwargs)).eval(), kwargs, shape


def _video(n, h, w, seed=0):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


def _rel(a, ref):
    return ((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize('name,padding,hw', [('M_T5', 'reflection_circle', (32, 48)), ('L_T7', 'circle', (32, 48)),
                                             ('L_deblur_hr', 'reflection', (64, 64)), ('M_noTSA', 'replicate', (32, 48))])
def test_restore_matches_the_oracle_on_every_window(gpu, name, padding, hw):
    from edvr_amd import VideoRestorer, window_table
    from oracle import edvr_oracle as EO
    net, kwargs, _ = _net(name)
    t, n = kwargs['num_frame'], 9
    lq = _video(n, *hw)
    windows = lq[window_table(n, t, padding).long()]  # (n, t, 3, h, w)
    with torch.no_grad():
        ref = EO.edvr_forward({k: v.double() for k, v in net.state_dict().items()}, windows.double(), **oracle_kwargs(kwargs))
        net = net.to(gpu)
        out = VideoRestorer(net, padding=padding, chunk=4).restore(lq.to(gpu))  # 9 frames in chunks of 4, 4, 1
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    gt = torch.rand(ref.shape, generator=torch.Generator().manual_seed(1))
    for i in range(n):
        r = _rel(out[i], ref[i])
        p_ours, p_ref = EO.psnr(out[i:i + 1].cpu(), gt[i:i + 1]), EO.psnr(ref[i:i + 1].float(), gt[i:i + 1])
        print(f'{name} frame {i}: rel {r:.2e}, PSNR {p_ours:.5f} vs {p_ref:.5f} dB')
        assert r < INTERMEDIATE_RTOL, (i, r)
        assert abs(p_ours - p_ref) <= PSNR_TOL_DB, (i, p_ours, p_ref)


@pytest.mark.parametrize('f4s', [True, False])
@pytest.mark.parametrize('name,hw', [('M_T5', (32, 48)), ('L_deblur_hr', (64, 64))])
def test_restore_matches_the_windowed_path(gpu, name, hw, f4s):
    from edvr_amd import VideoRestorer, metrics, ops
    net, kwargs, _ = _net(name)
    net = net.to(gpu)
    lq = _video(9, *hw, seed=3).to(gpu)
    prev = ops.set_f4s(inference=f4s)
    try:
        with torch.no_grad():
            want, _ = metrics.validate_clip(net, lq, num_frame=kwargs['num_frame'], padding='reflection_circle', batch=4)
            got = VideoRestorer(net, padding='reflection_circle', chunk=4).restore(lq)
            also, _ = metrics.validate_video(net, lq, num_frame=kwargs['num_frame'], padding='reflection_circle', chunk=4)
        torch.cuda.synchronize()
    finally:
        ops.set_f4s(inference=prev[0])
    diff = (got - want).abs().max().item() / want.abs().max().item()
    same = torch.equal(got, want)
    print(f'{name} split kernels {"on" if f4s else "off"}: max |video - windowed| / scale = {diff:.2e}, bit-identical: {same}')
    assert torch.equal(also, got)
    assert diff < BATCH_COMPOSITION_TOL
    if not f4s:
        # without the split kernels nothing depends on which images share a launch: the same kernels see the same images
        assert same


def test_features_are_extracted_once_per_frame(gpu, monkeypatch):
    from edvr_amd import VideoRestorer, metrics, ops
    net, kwargs, _ = _net('M_T5')
    net = net.to(gpu)
    t, n = kwargs['num_frame'], 17
    lq = _video(n, 32, 48, seed=4).to(gpu)
    images, flops, inside = [], {'all': 0.0, 'extract': 0.0}, [False]
    real = net.extract_features

    def spy(frames, out=None):
        images.append(frames.shape[0])
        inside[0] = True
        try:
            return real(frames, out=out)
        finally:
            inside[0] = False

    def hook(name, fl, launch, nbytes, executed=None):
        flops['all'] += fl
        if inside[0]:
            flops['extract'] += fl
        launch()

    monkeypatch.setattr(net, 'extract_features', spy)
    monkeypatch.setattr(ops, 'LAUNCH_HOOK', hook)
    with torch.no_grad():
        metrics.validate_clip(net, lq, num_frame=t, padding='reflection_circle', batch=4)
        windowed, n_windowed = dict(flops), sum(images)
        images.clear()
        flops.update(all=0.0, extract=0.0)
        VideoRestorer(net, padding='reflection_circle', chunk=4).restore(lq)
    torch.cuda.synchronize()
    assert n_windowed == n * t and sum(images) == n
    assert windowed['extract'] > 0.15 * windowed['all']  # (the hook does see the per-frame stage)
    # the chunks have the windowed batches' shapes, so everything after the per-frame stage books the same work, and the per-frame
    # stage 1 / t of it: the difference IS (t - 1) / t of the windowed run's per-frame stage (rounding of the float sums aside)
    saved = windowed['all'] - flops['all']
    print(f'FLOPs windowed {windowed["all"]:.4e} (per-frame stage {windowed["extract"]:.4e}), video {flops["all"]:.4e}, saved {saved:.4e}')
    assert saved >= (t - 1) / t * windowed['extract'] * (1 - 1e-6)
    assert abs(flops['extract'] - windowed['extract'] / t) <= 1e-6 * windowed['extract']


@pytest.mark.parametrize('width', [44, 45, 6])
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_gather_images_is_index_select(gpu, width, levels):
    from edvr_amd import ops
    g = torch.Generator().manual_seed(width * 10 + levels)
    shapes = [(5, 7, width), (3, 4, (width + 1) // 2), (2, 2, 3)][:levels]
    n_src = 6
    banks = [torch.randn(n_src + 3, c + 1, h, w, generator=g).to(gpu) for c, h, w in shapes]
    srcs = [b[2:2 + n_src, 1:] for b in banks]  # a slice of a larger bank: images c * h * w dense, a larger image stride, odd offsets
    for i, s in enumerate(srcs):
        ops.set_bound(s, torch.full((1,), 10.0 + i, device=gpu))
    for idx in ([5, 4, 3, 2, 1, 0], [2, 2, 0, 5, 2, 5, 5, 1, 0], [3], list(torch.randint(0, n_src, (13,), generator=g))):
        table = torch.tensor([int(v) for v in idx], dtype=torch.int32, device=gpu)
        outs = ops.gather_images(srcs, table)
        for i, (o, s) in enumerate(zip(outs, srcs)):
            assert o.is_contiguous() and torch.equal(o, s.index_select(0, table.long()))
            assert ops.get_bound(o) is not None and float(ops.get_bound(o)) == 10.0 + i  # a gather cannot enlarge anything
    # an index outside the bank is never followed: that image comes out as NaN, its neighbours are right
    outs = ops.gather_images(srcs, torch.tensor([1, n_src, -1, 0], dtype=torch.int32, device=gpu))
    for o, s in zip(outs, srcs):
        assert torch.equal(o[0], s[1]) and torch.equal(o[3], s[0]) and torch.isnan(o[1:3]).all()
    with pytest.raises(NotImplementedError):
        ops.gather_images([s.cpu() for s in srcs], table)
    # no bound on the source -> none on the destination (not a stale one)
    plain = torch.randn(4, 2, 3, width, device=gpu)
    assert ops.get_bound(ops.gather_images([plain], table.clamp(max=3))[0]) is None


def _as_bytes(x):
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)


@pytest.mark.parametrize('name,hw', [('M_T5', (24, 44)), ('L_deblur_hr', (32, 48))])
def test_uint8_output_is_tensor2img_of_the_float_output(gpu, name, hw):
    from edvr_amd import VideoRestorer
    net, kwargs, _ = _net(name)
    with torch.no_grad():
        net.conv_last.weight.mul_(10.0)  # drives the outputs far outside [0, 1] on both sides: the clamp is exercised
    net = net.to(gpu)
    lq8 = torch.randint(0, 256, (7,) + hw + (3,), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).to(gpu)
    # (numpy's float32 division, which the input kernel reproduces exactly; torch divides by a scalar through its reciprocal)
    lq = torch.from_numpy(lq8.cpu().numpy().astype(np.float32) / np.float32(255)).permute(0, 3, 1, 2).contiguous().to(gpu)
    with torch.no_grad():
        f32 = VideoRestorer(net, chunk=3).restore(lq)
        u8 = VideoRestorer(net, chunk=3, out_dtype=torch.uint8).restore(lq)
        from_bytes = VideoRestorer(net, chunk=3).restore(lq8)
    torch.cuda.synchronize()
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (7, f32.shape[2], f32.shape[3], 3)
    assert (f32 < 0).any() and (f32 > 1).any() and ((f32 > 0) & (f32 < 1)).any()
    assert torch.equal(u8, _as_bytes(f32))
    assert torch.equal(from_bytes, f32)  # uint8 input = float input divided by 255


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (3, 3, 8, 12)])
def test_byte_kernels_on_their_own(gpu, shape):
    from edvr_amd import ops
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(shape, generator=g) * 0.8 + 0.5).to(gpu)
    x[0, 0, 0, :4] = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255])[:shape[3]][:4]  # ties: half to even
    assert torch.equal(ops.f32_to_u8_hwc(x), _as_bytes(x))
    big = torch.randn(shape[0], 5, shape[2], shape[3], generator=g).to(gpu)
    assert torch.equal(ops.f32_to_u8_hwc(big[:, 1:4]), _as_bytes(big[:, 1:4]))  # an image-strided view
    y = (torch.randn(shape[0], 3, 4 * shape[2], 4 * shape[3], generator=g) * 0.5).to(gpu)
    got = ops.upsample4x_add_u8(y, x)
    assert torch.equal(got, _as_bytes(ops.upsample4x_add_(y.clone(), x)))


def test_streaming_gives_the_same_frames_and_a_bounded_bank(gpu):
    from edvr_amd import VideoRestorer, ops
    net, kwargs, _ = _net('M_noTSA')
    net = net.to(gpu)
    lq = _video(11, 32, 32, seed=6).to(gpu)
    vr = VideoRestorer(net, padding='circle', chunk=4)
    with torch.no_grad():
        whole = vr.restore(lq)
        one_by_one = torch.stack(list(vr.restore_iter(iter(lq.unbind(0)))))
        uneven = torch.stack(list(vr.restore_iter([lq[:3], lq[3:4], lq[4:10], lq[10:]])))
    assert torch.equal(one_by_one, whole) and torch.equal(uneven, whole)

    def stream(n):
        g = torch.Generator().manual_seed(8)
        for _ in range(n):
            yield torch.rand(3, 32, 32, generator=g).to(gpu)

    peaks, checks = [], 0
    # (the magnitude-bound slots come in 8 KB blocks, a new one every 2048 launches, the old one alive until the next overflow check:
    # start a fresh block so that no such hand-over - which has nothing to do with the stream's length - falls into the window)
    ops.reserve_amax_slots(gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        for i, frame in enumerate(vr.restore_iter(stream(60))):
            checks += float(frame.sum()) == float(frame.sum())  # (consumed and dropped: the caller keeps nothing)
            peaks.append(torch.cuda.max_memory_allocated())
    assert len(peaks) == 60 and checks == 60
    assert peaks[-1] == peaks[20], (peaks[20], peaks[-1])  # the bank is a ring: no growth with the length of the stream
    assert vr.schedule.peak <= vr.capacity <= 4 + 2 * (kwargs['num_frame'] - 1)


def test_offset_bookkeeping_is_that_of_a_run_of_forwards(gpu, caplog):
    from edvr_amd import VideoRestorer, window_table
    net, kwargs, _ = _net('M_T5')
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith('cas_dcnpack.conv_offset.bias'):
                p.fill_(80.0)  # every offset of the cascade DCN ~80 px (tests/test_gpu_edvr.py::test_offset_check_never_waits_for_the_gpu)
    net = net.to(gpu)
    t, n = kwargs['num_frame'], 9
    lq = _video(n, 32, 32, seed=9).to(gpu)
    windows = lq[window_table(n, t, 'reflection_circle').long().to(gpu)]

    def warnings():
        return len([r for r in caplog.records if 'larger than 50' in r.getMessage()])

    with caplog.at_level(logging.WARNING, logger='basicsr'):
        with torch.no_grad():
            for s in range(0, n, 4):
                net(windows[s:s + 4])
        net.check_offsets()
        by_forwards = warnings()
        assert by_forwards == 3 * t  # per (DCN layer over the limit, window frame) of each of the three forwards
        caplog.clear()
        with torch.no_grad():
            out = VideoRestorer(net, chunk=4).restore(lq)
        assert net._pending_offset_stats  # nothing waited for the GPU: (at least) the last chunk's statistics are still on their way
        net.check_offsets()
        assert not net._pending_offset_stats
        assert warnings() == by_forwards
    assert torch.isfinite(out).all()
