"""GPU: the BD downsampling kernel (csrc/bd.hip, edvr_amd.ops.bd_downsample / edvr_amd.data.duf_downsample) against the reference's
duf_downsample (tests/golden/bd_downsample.pt, written by scripts/make_bd_golden.py), against a float64 restatement of the formula
(tests/util_bd.py) and against the stock F.pad + F.conv2d composition; its bit-for-bit identities, its properties, and the places it is
wired into (VideoTestClips, VideoTestDUFClips, scripts/eval_video.py).

Bounds, none of them taken from the kernel's output.  Against the float64 formula 3e-6: two float32 13-tap convex combinations of data in
[0, 1] err by at most about 2 * 14 * 2^-24 = 1.7e-6 in the worst case, the float32 weights add a few ulp.  Against the reference 5e-6:
the reference itself sits <= 7.2e-7 from float64 on the fixture (a 169-term float32 sum), added to the above and rounded up."""
import importlib.util
import os

import pytest
import torch

from util_bd import FIXTURE_CASES, bd_f64, gauss13, load_golden, to_u8
from util_data import png_bytes

pytestmark = pytest.mark.gpu
TOL_REF, TOL_F64 = 5e-6, 3e-6


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bytes(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _planes(u8):
    """(n, h, w, 3) uint8 -> (n, 3, h, w) float32 = byte / 255, correctly rounded (what edvr_frames_u8_to_f32 computes)."""
    return (u8.float() / 255).permute(0, 3, 1, 2).contiguous()


def _check(got, want64, what, tol):
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    err = (got.double().cpu() - want64).abs().max().item()
    print(f'{what}: max abs err {err:.3e}')
    assert err <= tol, (what, err)


@pytest.mark.parametrize('index', range(len(FIXTURE_CASES)))
def test_matches_the_reference(gpu, index):
    from edvr_amd import data
    case = load_golden()[index]
    (h, w), scale = FIXTURE_CASES[index]
    assert tuple(case['input'].shape) == (2, h, w, 3) and case['scale'] == scale
    want = case['output'].double()
    _check(data.duf_downsample(case['input'].to(gpu), scale=scale), want, f'uint8 {(h, w)} / {scale}', TOL_REF)
    _check(data.duf_downsample(_planes(case['input']).to(gpu), scale=scale), want, f'float {(h, w)} / {scale}', TOL_REF)
    _check(data.duf_downsample(_planes(case['input'])[None].to(gpu), 13, scale)[0], want, f'float (b, t, c, h, w) {(h, w)} / {scale}', TOL_REF)


@pytest.mark.parametrize('index', range(len(FIXTURE_CASES)))
def test_bytes_match_the_reference_rounded(gpu, index):
    """The uint8 output differs from tensor2img of the reference's output by at most 1, and only where 255 * (the float64 value) lies within
    255 * 5e-6 of a half-integer - a per-sample condition."""
    from edvr_amd import ops
    case = load_golden()[index]
    scale = case['scale']
    got = ops.bd_downsample(case['input'].to(gpu), scale, out_dtype=torch.uint8).cpu()
    want = to_u8(case['output']).permute(0, 2, 3, 1)
    exact = 255 * bd_f64(_planes(case['input']), scale).permute(0, 2, 3, 1)
    near_tie = ((exact - exact.floor()) - 0.5).abs() <= 255 * TOL_REF
    diff = (got.int() - want.int()).abs()
    print(f'{FIXTURE_CASES[index]}: {int((diff != 0).sum())} of {diff.numel()} bytes differ, {int(near_tie.sum())} near a tie')
    assert diff.max().item() <= 1 and not bool((diff != 0)[~near_tie].any())
    ref_diff = (want.int() - to_u8(exact / 255).int()).abs()  # the reference alone meets the same condition against float64
    assert ref_diff.max().item() <= 1 and not bool((ref_diff != 0)[~near_tie].any())


@pytest.mark.parametrize('n,hw,scale', [
    (1, (720, 1280), 4), (1, (720, 1280), 2), (1, (720, 1280), 3), (1, (2880, 5120), 4),  # real sizes
    (3, (64, 96), 4), (2, (37, 53), 4), (2, (37, 53), 2), (2, (45, 64), 3), (2, (41, 67), 3),  # n > 1; no multiples of the scale
    (2, (50, 48), 2), (2, (50, 16), 4), (1, (33, 52), 4), (1, (33, 50), 2),                # 3 W % 16 == 0 / W % 4 == 0 and neither
    (2, (130, 700), 4), (1, (300, 270), 2), (1, (100, 393), 3),                            # several tiles, ragged last tile
    (2, (7, 7), 2), (2, (7, 7), 3), (2, (7, 7), 4), (1, (8, 40), 2), (1, (40, 10), 2), (1, (9, 12), 3), (1, (12, 40), 3),  # 7 .. 6 + 2 s rows
    (1, (40, 14), 4), (1, (13, 14), 4), (1, (7, 100), 4), (1, (100, 7), 4),                # or columns: the reference cannot run these
])
def test_matches_the_float64_formula(gpu, n, hw, scale):
    from edvr_amd import ops
    u8 = _bytes(n, *hw, seed=1000 * n + hw[0] + scale)
    x = _planes(u8)
    want = bd_f64(x, scale)
    what = f'{n} x {hw} / {scale}'
    got_u8 = ops.bd_downsample(u8.to(gpu), scale)
    _check(got_u8, want, 'uint8 ' + what, TOL_F64)
    got_f = ops.bd_downsample(x.to(gpu), scale)
    _check(got_f, want, 'float ' + what, TOL_F64)
    assert torch.equal(got_u8, got_f)


def test_strided_batch_view(gpu):
    from edvr_amd import ops
    x = torch.rand(4, 6, 40, 52, generator=torch.Generator().manual_seed(3)).to(gpu)
    view = x[:, 3:]  # dense images, image stride 6 planes
    assert not view.is_contiguous()
    for scale in (2, 3, 4):
        got = ops.bd_downsample(view, scale)
        _check(got, bd_f64(view.cpu(), scale), f'strided view / {scale}', TOL_F64)
        assert torch.equal(got, ops.bd_downsample(view.contiguous(), scale))


@pytest.mark.parametrize('hw', [(64, 96), (37, 53), (45, 64), (30, 44), (50, 16)])
@pytest.mark.parametrize('scale', [2, 3, 4])
def test_byte_forms_are_the_float_form_bit_for_bit(gpu, hw, scale):
    """uint8 in == float in; uint8 out == tensor2img of the float out.  Widths with and without the 16-byte paths."""
    from edvr_amd import ops
    u8 = _bytes(2, *hw, seed=11).to(gpu)
    x = ops.frames_u8_to_f32(u8[None])[0]
    assert torch.equal(x.cpu(), _planes(u8.cpu()))
    f_from_u8, f_from_f = ops.bd_downsample(u8, scale), ops.bd_downsample(x, scale)
    assert torch.equal(f_from_u8, f_from_f)
    want_bytes = to_u8(f_from_f).permute(0, 2, 3, 1).contiguous()
    for src in (u8, x):
        got = ops.bd_downsample(src, scale, out_dtype=torch.uint8)
        assert got.dtype == torch.uint8 and torch.equal(got, want_bytes)
        assert torch.equal(got, ops.f32_to_u8_hwc(f_from_f))  # the network's byte tail agrees


@pytest.mark.parametrize('scale', [2, 3, 4])
def test_constant_image_stays_constant(gpu, scale):
    from edvr_amd import ops
    for value in (0.0, 0.37, 1.0):
        out = ops.bd_downsample(torch.full((1, 3, 48, 60), value, device=gpu), scale)
        assert (out - value).abs().max().item() <= 1e-6


@pytest.mark.parametrize('scale', [2, 3, 4])
def test_commutes_with_flips(gpu, scale):
    """bd(flip(x)) == flip(bd(x)) on an axis of n samples when (n - 1) % scale == 0: taps are centred on input sample i * scale, so the
    sampled positions 0, s, 2 s, .. map onto themselves under p -> n - 1 - p exactly then.  NOT when n is a multiple of the scale (the
    positions then sit off-centre: DUF's convention, unlike imresize's cell centres)."""
    from edvr_amd import ops
    h, w = 4 * scale + 1, 20 * scale + 1
    x = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(5)).to(gpu)
    base = ops.bd_downsample(x, scale)
    for dims in ((2,), (3,), (2, 3)):
        err = (ops.bd_downsample(x.flip(dims).contiguous(), scale) - base.flip(dims)).abs().max().item()
        assert err <= TOL_F64, (dims, err)
    y = torch.rand(1, 3, 4 * scale, 20 * scale, generator=torch.Generator().manual_seed(6)).to(gpu)
    assert (ops.bd_downsample(y.flip((3,)).contiguous(), scale) - ops.bd_downsample(y, scale).flip((3,))).abs().max().item() > 1e-3


@pytest.mark.parametrize('scale', [2, 3, 4])
def test_impulse_reproduces_the_kernel(gpu, scale):
    """An impulse at (i0 s + dy, j0 s + dx) puts g[6 - (a s - dy)] g[6 - (b s - dx)] at output (i0 + a, j0 + b): taps start at i s - 6."""
    from edvr_amd import ops
    g = torch.from_numpy(gauss13(scale))
    h, w = 20 * scale, 24 * scale
    for (dy, dx) in ((0, 0), (1, scale - 1)):
        i0, j0 = 9, 11
        x = torch.zeros(1, 3, h, w)
        x[0, 1, i0 * scale + dy, j0 * scale + dx] = 1.0
        out = ops.bd_downsample(x.to(gpu), scale).double().cpu()
        want = torch.zeros(h // scale, w // scale, dtype=torch.float64)
        for i in range(h // scale):
            for j in range(w // scale):
                a, b = i0 * scale + dy - (i * scale - 6), j0 * scale + dx - (j * scale - 6)  # the tap of output (i, j) on the impulse
                if 0 <= a <= 12 and 0 <= b <= 12:
                    want[i, j] = g[a] * g[b]
        assert want[i0, j0] == g[6 + dy] * g[6 + dx] and want.sum() > 0
        assert (out[0, 1] - want).abs().max().item() <= 1e-7 and out[0, 0].abs().max().item() == 0 and out[0, 2].abs().max().item() == 0


def test_refusals(gpu):
    from edvr_amd import data, ops
    with pytest.raises(NotImplementedError):
        data.duf_downsample(torch.rand(2, 3, 32, 32))
    with pytest.raises(NotImplementedError):
        ops.bd_downsample(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), 4)
    launches = []
    hook, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, lambda name, *a: launches.append(name)
    try:
        for shape, scale in (((1, 3, 6, 96), 4), ((1, 3, 64, 6), 2), ((1, 3, 1, 1), 3), ((1, 3, 64, 64), 1), ((1, 3, 64, 64), 5), ((1, 3, 64, 64), 2.5)):
            with pytest.raises(ValueError):
                ops.bd_downsample(torch.rand(*shape, device=gpu), scale)
        with pytest.raises(ValueError):
            ops.bd_downsample(torch.zeros(1, 6, 64, 3, dtype=torch.uint8, device=gpu), 4)
        with pytest.raises(ValueError):
            data.duf_downsample(torch.rand(2, 3, 32, 32, device=gpu), kernel_size=7)
        with pytest.raises(ValueError):
            ops.bd_downsample(torch.rand(1, 3, 32, 32, device=gpu), 4, out_dtype=torch.float16)
    finally:
        ops.LAUNCH_HOOK = hook
    assert launches == []  # refused before any launch
    # ... and the C entry point refuses the same calls on its own
    from edvr_amd import _lib
    lib = _lib.lib()
    x, out = torch.rand(1, 3, 6, 96, device=gpu), torch.zeros(1, 3, 24, 48, device=gpu)
    assert lib.edvr_bd_downsample_f32(x.data_ptr(), out.data_ptr(), 1, 6, 96, 3 * 6 * 96, 2, 24, 4, 0, None) != 0 and b'fewer than 7' in lib.edvr_last_error()
    x = torch.rand(1, 3, 32, 96, device=gpu)
    assert lib.edvr_bd_downsample_f32(x.data_ptr(), out.data_ptr(), 1, 32, 96, 3 * 32 * 96, 7, 20, 5, 0, None) != 0 and b'not 2, 3 or 4' in lib.edvr_last_error()
    assert lib.edvr_bd_downsample_f32(x.data_ptr(), out.data_ptr(), 1, 32, 96, 3 * 32 * 96, 8, 25, 4, 0, None) != 0 and b'is not ceil' in lib.edvr_last_error()
    u8 = torch.zeros(1, 32, 6, 3, dtype=torch.uint8, device=gpu)
    assert lib.edvr_bd_downsample_u8(u8.data_ptr(), out.data_ptr(), 1, 32, 6, 16, 3, 2, 0, None) != 0 and b'fewer than 7' in lib.edvr_last_error()
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0  # nothing was written


def test_launch_is_booked_with_algorithmic_bytes(gpu):
    from edvr_amd import ops
    seen = []

    def hook(name, flops, launch, nbytes, executed):
        seen.append((name, nbytes))
        launch()

    prev, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, hook
    try:
        ops.bd_downsample(_bytes(2, 64, 96, 1).to(gpu), 4)
        ops.bd_downsample(torch.rand(1, 3, 30, 44, device=gpu), 3, out_dtype=torch.uint8)
    finally:
        ops.LAUNCH_HOOK = prev
    assert seen == [('bd_downsample', 2 * 64 * 96 * 3 + 2 * 3 * 16 * 24 * 4.0), ('bd_downsample', 3 * 30 * 44 * 4.0 + 10 * 15 * 3)]


def test_stock_composition_agrees(gpu):
    """The reference's own formulation through PyTorch on the GPU - F.pad(reflect) by 6 + 2 s, F.conv2d with the float32 2-D filter at
    stride s, crop 2 per side - is the same function: a third witness, on a real size."""
    import torch.nn.functional as F
    from edvr_amd import data, ops
    scale = 4
    x = _planes(_bytes(2, 720, 1280, seed=21)).to(gpu)
    g = torch.from_numpy(data.bd_weights(scale))
    filt = torch.outer(g, g).float()[None, None].to(gpu)
    pad = 6 + 2 * scale
    stock = F.conv2d(F.pad(x.view(-1, 1, 720, 1280), (pad,) * 4, mode='reflect'), filt, stride=scale)[:, :, 2:-2, 2:-2].reshape(2, 3, 180, 320)
    got = ops.bd_downsample(x, scale)
    err = (got - stock).abs().max().item()
    print(f'stock composition: max abs diff {err:.3e}')
    assert err <= TOL_REF


def _write_gt_tree(root, folders, frames, hw):
    from oracle import data_oracle as DO
    for folder in folders:
        d = os.path.join(root, 'gt', folder)
        os.makedirs(d, exist_ok=True)
        for f in range(frames):
            with open(os.path.join(d, f'{f:08d}.png'), 'wb') as fh:
                fh.write(png_bytes(DO.synthetic_frame('gt', folder, f'{f:08d}', *hw)))


def test_video_clips_derive_bd_lq_from_gt(gpu, tmp_path):
    import json
    from edvr_amd import data, metrics, ops
    from util_edvr import build
    _write_gt_tree(str(tmp_path), ['000', '011'], 6, (66, 99))  # mod-cropped to 64 x 96
    opt = dict(name='Vid4', dataroot_gt=str(tmp_path / 'gt'), dataroot_lq=None, lq_from_gt={'scale': 4, 'degradation': 'bd'}, io_backend=dict(type='disk'),
               cache_data=True, num_frame=5, padding='reflection_circle')
    ds = data.VideoTestClips(opt, device=gpu)
    lq, gt = ds.clip('011')
    assert tuple(gt.shape) == (6, 3, 64, 96) and tuple(lq.shape) == (6, 3, 16, 24)
    full = data.read_img_seq(ds.imgs_gt['011'], gpu)
    assert torch.equal(gt, full[:, :, :64, :96])
    assert torch.equal(lq, ops.bd_downsample(gt, 4))  # not quantised: exactly the kernel's float output
    _check(lq, bd_f64(gt.cpu(), 4), 'clip LQ', TOL_F64)
    quant = data.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'degradation': 'bd', 'quantize': True}), device=gpu)
    assert torch.equal(quant.clip('011')[0], (to_u8(lq).cpu().float() / 255).to(gpu))

    # VideoTestDUFClips: the same frames under the reference's keys; windows and borders are VideoTestClips's
    duf = data.VideoTestDUFClips(dict(opt, lq_from_gt=None, dataroot_lq=str(tmp_path / 'BDx4'), use_duf_downsampling=True, scale=4), device=gpu)
    assert len(duf) == len(ds) == 12 and duf.data_info['border'] == ds.data_info['border'] and duf.data_info['idx'] == ds.data_info['idx']
    assert duf.data_info['lq_path'][6] == str(tmp_path / 'BDx4' / '011' / '00000000.png')
    for index in (0, 6, 11):
        a, b = duf[index], ds[index]
        assert torch.equal(a['lq'], b['lq']) and torch.equal(a['gt'], b['gt']) and (a['folder'], a['idx'], a['border']) == (b['folder'], b['idx'], b['border'])
    item = duf[len(duf) - 1]
    assert item['folder'] == '011' and item['border'] == 1 and torch.equal(item['gt'], gt[5]) and torch.equal(item['lq'][2], lq[5])
    window = metrics.generate_frame_indices(5, 6, 5, padding='reflection_circle')
    assert tuple(item['lq'].shape) == (5, 3, 16, 24) and all(torch.equal(item['lq'][k], lq[i]) for k, i in enumerate(window))
    lazy = data.VideoTestDUFClips(dict(opt, lq_from_gt=None, cache_data=False, use_duf_downsampling=True, scale=4), device=gpu)
    assert torch.equal(lazy[7]['lq'], duf[7]['lq']) and torch.equal(lazy[7]['gt'], duf[7]['gt'])

    net = build('M_T5')[0].to(gpu)
    with torch.no_grad():
        out, psnr = metrics.validate_video(net, lq, gt, num_frame=5, chunk=4)
    assert tuple(out.shape) == tuple(gt.shape) and len(psnr) == 6 and all(p == p for p in psnr)

    # scripts/eval_video.py --lq-from-gt 4 --degradation bd --bicubic-baseline: the report carries the degradation and a finite baseline
    ev = _load_script('eval_video')
    base = ev.bicubic_baseline(lq, gt, chunk=4)
    assert base == metrics.calculate_psnr(data.imresize(lq, 4), gt) and len(base) == 6 and all(0 < b < 100 for b in base)
    report = tmp_path / 'report.json'
    args = ev.parse_args(['--gt', str(tmp_path / 'gt'), '--lq-from-gt', '4', '--degradation', 'bd', '--bicubic-baseline', '--json', str(report),
                          '--name', 'Vid4', '--num-feat', '64', '--batch', '4'])
    args.num_feat, args.num_reconstruct_block = 64, 10  # EDVR-M
    summary = ev.evaluate(args, log=lambda s: None)
    record = json.loads(report.read_text())
    assert record['degradation'] == 'bd' and sorted(record['psnr']) == ['000', '011'] == sorted(summary)
    assert abs(record['bicubic_psnr']['011'] - sum(base) / 6) < 1e-9 and 0 < record['bicubic_average'] < 100
