"""-m gpu: temporal-reversal self-ensemble on the whole-video path (edvr_amd/video.py: time_reverse) - the attention kernel with two
outputs against the existing one, the whole network against the definition evaluated with the plain VideoRestorer on host-reversed (and
host-transformed) frames, the shared arm against the unshared one, streaming, validation and the offset bookkeeping."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_video import BATCH_COMPOSITION_TOL
from util_edvr import CONFIGS, randomize_offsets

pytestmark = pytest.mark.gpu


def _g(x, k):
    """The spatial elements of self_ensemble: k = 4 t + 2 v + h; transpose if t, then flip rows if v, then flip columns if h."""
    if k & 4:
        x = x.transpose(-1, -2)
    if k & 2:
        x = x.flip(-2)
    if k & 1:
        x = x.flip(-1)
    return x


def _g_inv(y, k):
    if k & 1:
        y = y.flip(-1)
    if k & 2:
        y = y.flip(-2)
    if k & 4:
        y = y.transpose(-1, -2)
    return y


def _up(v, m):
    return (v + m - 1) // m * m


def _video(n, h, w, seed=0):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('shape', [(2, 5, 8, 6, 10),    # hw = 60: the 16-byte path
                                   (1, 3, 4, 5, 7),     # hw = 35: the scalar path
                                   (2, 7, 16, 4, 4),
                                   (1, 1, 4, 4, 8)])    # t = 1: out_rev equals out
def test_pair_kernel_is_the_attention_kernel_with_a_reversed_second_store(gpu, shape):
    from edvr_amd import functional as F_, ops
    b, t, c, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    emb, ref, al = (torch.randn(s, generator=g).to(gpu) for s in (shape, (b, c, h, w), shape))
    with torch.no_grad():
        want = ops.tsa_temporal(emb, ref, al)
        out, out_rev = (torch.full(shape, float('nan'), device=gpu) for _ in range(2))  # NaN: an element no thread writes shows
        got, got_rev = ops.tsa_temporal_pair(emb, ref, al, out=out, out_rev=out_rev)
        assert got is out and got_rev is out_rev
        assert torch.equal(out, want)
        assert torch.equal(out_rev, out.flip(1))
        a, a_rev = F_.tsa_temporal_pair(emb, ref, al)                                   # ... and into outputs it allocates
        assert torch.equal(a, want) and torch.equal(a_rev, want.flip(1)) and a.data_ptr() != a_rev.data_ptr()
        # the magnitude bound travels to both outputs as with tsa_temporal
        ops.set_bound(al, ops.amax(al.view(b * t, c, h, w)))
        p, p_rev = ops.tsa_temporal_pair(emb, ref, al)
        assert ops.get_bound(p) is not None and torch.equal(ops.get_bound(p), ops.get_bound(al)) and torch.equal(ops.get_bound(p_rev), ops.get_bound(al))
        ops.void_bound(al)
        p, p_rev = ops.tsa_temporal_pair(emb, ref, al)
        assert ops.get_bound(p) is None and ops.get_bound(p_rev) is None
        # aliased buffers, CPU tensors
        for kw in (dict(out=out, out_rev=out), dict(out=al), dict(out_rev=al), dict(out=out, out_rev=out.view(-1)[:out.numel()].view(shape))):
            with pytest.raises(ValueError):
                ops.tsa_temporal_pair(emb, ref, al, **kw)
        two = torch.empty((2,) + shape, device=gpu)
        with pytest.raises(ValueError):                                                 # overlapping, not identical
            ops.tsa_temporal_pair(emb, ref, al, out=two.view(-1)[:out.numel()].view(shape), out_rev=two.view(-1)[1:out.numel() + 1].view(shape))
        with pytest.raises(NotImplementedError):
            ops.tsa_temporal_pair(emb.cpu(), ref.cpu(), al.cpu())
        with pytest.raises(NotImplementedError):
            ops.tsa_temporal_pair(emb, ref, al, out=out.cpu())
    with torch.enable_grad():                                                           # no backward: refused in grad mode
        with pytest.raises(RuntimeError):
            ops.tsa_temporal_pair(emb, ref, al)
        with pytest.raises(RuntimeError):
            F_.tsa_temporal_pair(emb, ref, al)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ whole path
# name, (H, W), pad_mode, tile, overlap.  M_T5 on the three sizes; L_deblur_hr (size multiple 16) on the one of them it admits: 24 x 40
# is no multiple of 16 and the overlap of 8 is no multiple of 2 x 16.  M_noTSA: the arm that reverses the aligned images by a gather.
CASES = {'M_24x40': ('M_T5', (24, 40), None, None, None),
         'M_30x46_reflect': ('M_T5', (30, 46), 'reflect', None, None),
         'M_62x90_tiles': ('M_T5', (62, 90), 'reflect', (32, 48), 8),
         'L_deblur_hr_30x46_reflect': ('L_deblur_hr', (30, 46), 'reflect', None, None),
         'noTSA_24x40': ('M_noTSA', (24, 40), None, None, None)}
ENSEMBLES = {'none': None, 'seq_5_0_2': (5, 0, 2)}
FRAMES, CHUNK = 9, 4    # the ring wraps, the last group is short, and the reversed video chunks differently (4 + 4 + 1 from the other end)
_NETS, _PLAIN = {}, {}  # the networks and the references R(g_k(crop)), R(rev(g_k(crop))) are computed once and shared


def _case(case, gpu):
    from edvr_amd import EDVR, tile_grid
    name, (H, W), pad_mode, tile, overlap = CASES[case]
    if name not in _NETS:
        kwargs, _ = CONFIGS[name]
        torch.manual_seed(10)
        _NETS[name] = (randomize_offsets(EDVR(**kwargs)).eval().to(gpu), kwargs)
    net, kwargs = _NETS[name]
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    lq = _video(FRAMES, H, W, seed=3).to(gpu)
    padded = F.pad(lq, (0, _up(W, m) - W, 0, _up(H, m) - H), mode=pad_mode) if pad_mode else lq
    return net, s, lq, padded, tile_grid(H, W, tile, overlap, m), dict(pad_mode=pad_mode, tile=tile, tile_overlap=overlap)


def _definition(case, gpu, f4s, elements):
    """The definition with the plain VideoRestorer: per tile, over the elements in order, g^-1(R(g(crop))) then g^-1(rev(R(rev(g(crop))))),
    added in float32 by torch in that order, times 1 / (2 n); the kept rectangles put together - float32 (FRAMES, 3, s H, s W)."""
    from edvr_amd import VideoRestorer
    net, s, lq, padded, grid, _ = _case(case, gpu)
    H, W = CASES[case][1]
    want = torch.empty(FRAMES, 3, s * H, s * W, device=gpu)
    for ti, ((y0, x0, th, tw), (ky, kx, kh, kw), (oy, ox)) in enumerate(grid):
        crop = padded[:, :, y0:y0 + th, x0:x0 + tw]
        acc = None
        for k in elements:
            for r in (0, 1):
                ck = (case, f4s, ti, k, r)
                if ck not in _PLAIN:
                    x = _g(crop, k).contiguous()
                    plain = VideoRestorer(net, chunk=CHUNK)
                    _PLAIN[ck] = plain.restore(x.flip(0).contiguous()).flip(0) if r else plain.restore(x)
                back = _g_inv(_PLAIN[ck], k)
                acc = back if acc is None else torch.add(acc, back)
        acc = torch.mul(acc, 1.0 / (2 * len(elements)))
        want[:, :, s * oy:s * (oy + kh), s * ox:s * (ox + kw)] = acc[:, :, s * ky:s * (ky + kh), s * kx:s * (kx + kw)]
    return want


@pytest.mark.parametrize('f4s', [True, False])
@pytest.mark.parametrize('ensemble', sorted(ENSEMBLES))
@pytest.mark.parametrize('case', sorted(CASES))
def test_time_reverse_is_the_definition(gpu, case, ensemble, f4s):
    """Split kernels off: bit for bit, float32 and bytes.  On: within BATCH_COMPOSITION_TOL - the reference's reversed video is cut into
    chunks from the other end, and the split scales depend on which images share a launch (tests/test_gpu_video.py)."""
    from edvr_amd import VideoRestorer, ops
    elements = ENSEMBLES[ensemble]
    net, s, lq, padded, grid, kw = _case(case, gpu)
    H, W = CASES[case][1]
    prev = ops.set_f4s(inference=f4s)
    try:
        with torch.no_grad():
            want = _definition(case, gpu, f4s, elements or (0,))
            want_u8 = ops.f32_to_u8_hwc(want)
            vr = VideoRestorer(net, chunk=CHUNK, self_ensemble=elements, time_reverse=True, **kw)
            got = vr.restore(lq)
            assert got.is_contiguous() and got.dtype == torch.float32 and tuple(got.shape) == (FRAMES, 3, s * H, s * W)
            assert len(vr.pairs) == len(grid) * len(elements or (0,)) and vr.share_alignment   # (tile x spatial element), as without it
            got8 = VideoRestorer(net, chunk=CHUNK, out_dtype=torch.uint8, self_ensemble=elements, time_reverse=True, **kw).restore(lq)
            assert got8.is_contiguous() and got8.dtype == torch.uint8 and tuple(got8.shape) == (FRAMES, s * H, s * W, 3)
            diff = (got - want).abs().max().item() / want.abs().max().item()
            diff8 = (got8.int() - want_u8.int()).abs().max().item()
            print(f'{case} {ensemble} f4s={f4s}: max |got - want| / max |want| = {diff:.3e}; bytes differ by at most {diff8}')
            if f4s:
                assert diff < BATCH_COMPOSITION_TOL
                assert diff8 <= 1  # (255 x 3e-5 x max |want| is far below 1: a byte moves only where the value sits on a rounding boundary)
            else:
                assert torch.equal(got, want), (case, ensemble, 'float32')
                assert torch.equal(got8, want_u8), (case, ensemble, 'uint8')
        torch.cuda.synchronize()
    finally:
        ops.set_f4s(inference=prev[0])
    net.check_offsets()


@pytest.mark.parametrize('f4s', [True, False])
@pytest.mark.parametrize('case,ensemble,blend', [('M_30x46_reflect', 'none', None), ('M_62x90_tiles', 'seq_5_0_2', None),
                                                 ('M_62x90_tiles', 'none', None), ('L_deblur_hr_30x46_reflect', 'seq_5_0_2', None),
                                                 ('noTSA_24x40', 'seq_5_0_2', None), ('M_62x90_tiles_blend', 'seq_5_0_2', 16)])
def test_shared_and_unshared_arms_are_bit_identical(gpu, case, ensemble, blend, f4s):
    """Both arms read the same bank under the same bounds in the same chunks, and every kernel between the gather and the fusion works
    image by image: the aligned (and modulated) images of the reversed windows are the forward ones at other positions, bit for bit - with
    the split kernels on as well, their scales being per launch and the launches holding the same images in another order."""
    from edvr_amd import VideoRestorer, ops
    elements = ENSEMBLES[ensemble]
    if blend:  # tiles (32, 64) at overlap 16 on 62 x 90: kept lengths that leave room for bands of 16
        net, s, lq, _, _, _ = _case('M_62x90_tiles', gpu)
        kw = dict(pad_mode='reflect', tile=(32, 64), tile_overlap=16, tile_blend=blend)
    else:
        net, s, lq, _, _, kw = _case(case, gpu)
    prev = ops.set_f4s(inference=f4s)
    try:
        with torch.no_grad():
            for dt in (torch.float32, torch.uint8):
                common = dict(chunk=CHUNK, out_dtype=dt, self_ensemble=elements, time_reverse=True, **kw)
                shared = VideoRestorer(net, share_alignment=True, **common).restore(lq)
                unshared = VideoRestorer(net, share_alignment=False, **common).restore(lq)
                d = (shared.float() - unshared.float()).abs().max().item()
                print(f'{case} {ensemble} blend={blend} f4s={f4s} {dt}: max |shared - unshared| = {d:.3e}')
                assert torch.equal(shared, unshared), (case, ensemble, dt)
        torch.cuda.synchronize()
    finally:
        ops.set_f4s(inference=prev[0])
    net.check_offsets()


def test_streaming_validation_and_offset_bookkeeping(gpu):
    from edvr_amd import VideoRestorer, metrics
    case = 'M_30x46_reflect'
    net, s, lq, _, grid, kw = _case(case, gpu)
    H, W = CASES[case][1]
    gt = torch.rand(FRAMES, 3, s * H, s * W, generator=torch.Generator().manual_seed(8)).to(gpu)
    net.check_offsets()
    arms = (('plain', {}), ('shared', dict(time_reverse=True)), ('unshared', dict(time_reverse=True, share_alignment=False)))
    with torch.no_grad():
        # the alignment ran once per (tile, element) and chunk: as many offset records as the plain tiled path queues, chunk by chunk - the
        # unshared arm, whose DCNs run twice, queues each twice
        launched = {}
        for key, extra in arms:
            seen = []
            orig = net._queue_offset_check
            net._queue_offset_check = lambda sink, b, t, _o=orig, _s=seen: (_s.append((len(sink), b, t)), _o(sink, b, t))[1]
            try:
                VideoRestorer(net, chunk=CHUNK, **kw, **extra).restore(lq)
            finally:
                del net._queue_offset_check
            launched[key] = seen
        assert launched['shared'] == launched['plain'] and len(launched['plain']) == 3 * len(grid)
        assert launched['unshared'] == [r for r in launched['plain'] for _ in (0, 1)]
        # frame by frame equals restore
        vr = VideoRestorer(net, chunk=CHUNK, time_reverse=True, **kw)
        want = vr.restore(lq)
        frames = list(vr.restore_iter(iter(lq.unbind(0))))
        assert torch.equal(torch.stack(frames), want)
        assert vr.banks is None and len(vr.pairs) == len(grid)
        # validate_video: the same tensor; its PSNRs are those of that tensor, not the plain path's
        out, psnr = metrics.validate_video(net, lq, gt, num_frame=5, chunk=CHUNK, pad_mode='reflect', time_reverse=True)
        plain, plain_psnr = metrics.validate_video(net, lq, gt, num_frame=5, chunk=CHUNK, pad_mode='reflect')
        assert torch.equal(out, want) and not torch.equal(out, plain)
        assert len(psnr) == FRAMES and psnr != plain_psnr
        assert psnr == [p for a in range(0, FRAMES, CHUNK) for p in metrics.calculate_psnr(want[a:a + CHUNK], gt[a:a + CHUNK], 0, False)]
    torch.cuda.synchronize()
    net.check_offsets()  # raises nothing
