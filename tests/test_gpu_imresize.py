"""GPU: the bicubic imresize kernel (csrc/resize.hip, edvr_amd.ops.imresize / edvr_amd.data.imresize) against the reference's imresize
(tests/golden/imresize.pt, written by scripts/make_imresize_golden.py) and against a float64 restatement of the formula
(tests/util_imresize.py), its bit-for-bit identities, and the places it is wired into (VideoTestClips, scripts/eval_video.py).

The 1e-5 bound on the float output: the reference itself sits <= 7e-7 from a float64 evaluation of the formula on the fixture cases
(its float32 `u` rounds at scale 0.3); a float32 dot product of <= 34 taps with sum |w| <= 1.3 on data in [0, 1] errs by under 3e-6
per pass; two passes plus the few ulp of the float32 weights stay below 1e-5.  A tap whose index flips between float32 and float64
floor() has a weight of ~0."""
import importlib.util
import os

import pytest
import torch

from util_data import png_bytes
from util_imresize import FIXTURE_CASES, imresize_f64, load_golden, to_u8

pytestmark = pytest.mark.gpu
TOL = 1e-5


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


def _check(got, want64, what):
    err = (got.double().cpu() - want64).abs().max().item()
    print(f'{what}: max abs err {err:.3e}')
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    assert err <= TOL, (what, err)


@pytest.mark.parametrize('index', range(len(FIXTURE_CASES)))
def test_matches_the_reference(gpu, index):
    from edvr_amd import data
    case = load_golden()[index]
    (h, w), scale = FIXTURE_CASES[index]
    assert tuple(case['input'].shape) == (h, w, 3) and case['scale'] == scale
    want = case['output'].double()
    u8 = case['input'][None].to(gpu)
    _check(data.imresize(u8, scale, case['antialiasing'])[0], want, f'uint8 {(h, w)} x {scale:.4g}')
    _check(data.imresize(_planes(case['input'][None])[0].to(gpu), scale, case['antialiasing']), want, f'float {(h, w)} x {scale:.4g}')


@pytest.mark.parametrize('n,hw,scale,antialiasing', [
    (1, (720, 1280), 1 / 4, True), (1, (180, 320), 4.0, True),          # real size, both directions
    (3, (64, 96), 1 / 4, True), (2, (37, 53), 1 / 4, True),             # n > 1; sizes that are no multiple of the scale
    (2, (45, 63), 1 / 3, True), (1, (50, 70), 0.3, True), (2, (31, 45), 2.0, True), (1, (41, 67), 2.5, True),
    (1, (64, 96), 1 / 4, False), (2, (37, 53), 1 / 4, False), (1, (48, 60), 1 / 2, False), (1, (50, 70), 0.3, False),  # antialiasing off: the
    (1, (30, 44), 4.0, False),                                          # first of these is a shape the reference cannot run
    (1, (128, 200), 1 / 8, True), (1, (16, 20), 8.0, True),             # the ends of the supported range
])
def test_matches_the_float64_formula(gpu, n, hw, scale, antialiasing):
    from edvr_amd import ops
    u8 = _bytes(n, *hw, seed=1000 * n + hw[0])
    x = _planes(u8)
    want = imresize_f64(x, scale, antialiasing)
    what = f'{n} x {hw} x {scale:.4g} aa={antialiasing}'
    _check(ops.imresize(u8.to(gpu), scale, antialiasing), want, 'uint8 ' + what)
    _check(ops.imresize(x.to(gpu), scale, antialiasing), want, 'float ' + what)


def test_strided_batch_view(gpu):
    from edvr_amd import ops
    x = torch.rand(4, 6, 40, 52, generator=torch.Generator().manual_seed(3)).to(gpu)
    view = x[:, 3:]  # dense images, image stride 6 planes
    assert not view.is_contiguous()
    got = ops.imresize(view, 1 / 4)
    _check(got, imresize_f64(view.cpu(), 1 / 4), 'strided view')
    assert torch.equal(got, ops.imresize(view.contiguous(), 1 / 4))


@pytest.mark.parametrize('hw,scale,antialiasing', [((64, 96), 1 / 4, True), ((37, 53), 1 / 4, True), ((45, 63), 1 / 3, False),
                                                  ((30, 44), 4.0, True), ((31, 45), 2.0, True), ((50, 70), 0.3, True)])
def test_byte_forms_are_the_float_form_bit_for_bit(gpu, hw, scale, antialiasing):
    """uint8 in == float in; uint8 out == tensor2img of the float out.  Widths with and without the 16-byte paths."""
    from edvr_amd import ops
    u8 = _bytes(2, *hw, seed=11).to(gpu)
    x = ops.frames_u8_to_f32(u8[None])[0]
    assert torch.equal(x.cpu(), _planes(u8.cpu()))
    f_from_u8, f_from_f = ops.imresize(u8, scale, antialiasing), ops.imresize(x, scale, antialiasing)
    assert torch.equal(f_from_u8, f_from_f)
    want_bytes = to_u8(f_from_f).permute(0, 2, 3, 1).contiguous()
    if scale > 1:
        assert f_from_f.max() > 1 and f_from_f.min() < 0  # an enlargement of noise overshoots: the float output is not clamped
    for src in (u8, x):
        got = ops.imresize(src, scale, antialiasing, out_dtype=torch.uint8)
        assert got.dtype == torch.uint8 and torch.equal(got, want_bytes)
        assert torch.equal(got, ops.f32_to_u8_hwc(f_from_f))  # the network's byte tail agrees


@pytest.mark.parametrize('scale', [1 / 4, 0.3, 2.0, 4.0])
def test_constant_image_stays_constant(gpu, scale):
    from edvr_amd import ops
    for value in (0.0, 0.37, 1.0):
        out = ops.imresize(torch.full((1, 3, 48, 60), value, device=gpu), scale)
        assert (out - value).abs().max().item() <= 1e-6


@pytest.mark.parametrize('hw,scale', [((64, 96), 1 / 4), ((48, 60), 1 / 2), ((30, 44), 4.0), ((45, 63), 1 / 3)])
def test_commutes_with_flips(gpu, hw, scale):
    """resize(flip(x)) == flip(resize(x)) on both axes when in * scale is an integer (the sampling grid is symmetric then)."""
    from edvr_amd import ops
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(5)).to(gpu)
    base = ops.imresize(x, scale)
    for dims in ((2,), (3,), (2, 3)):
        err = (ops.imresize(x.flip(dims).contiguous(), scale) - base.flip(dims)).abs().max().item()
        assert err <= TOL, (dims, err)


def test_refusals(gpu):
    from edvr_amd import data, ops
    with pytest.raises(NotImplementedError):
        data.imresize(torch.rand(3, 32, 32), 1 / 4)
    with pytest.raises(NotImplementedError):
        ops.imresize(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), 1 / 4)
    launches = []
    hook, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, lambda name, *a: launches.append(name)
    try:
        for shape, scale in (((1, 3, 5, 96), 1 / 4), ((1, 3, 64, 5), 1 / 4), ((1, 3, 1, 1), 4.0), ((1, 3, 64, 64), 1 / 16), ((1, 3, 8, 8), 9.0)):
            with pytest.raises(ValueError):
                ops.imresize(torch.rand(*shape, device=gpu), scale)
    finally:
        ops.LAUNCH_HOOK = hook
    assert launches == []  # refused before any launch
    # ... and the C entry point refuses the same frames on its own
    from edvr_amd import _lib
    x, out = torch.rand(1, 3, 5, 96, device=gpu), torch.empty(1, 3, 2, 24, device=gpu)
    rc = _lib.lib().edvr_imresize_bicubic_f32(x.data_ptr(), out.data_ptr(), 1, 5, 96, 3 * 5 * 96, 2, 24, 0.25, 1, 0, None)
    assert rc != 0 and b'symmetric extension' in _lib.lib().edvr_last_error()


def test_launch_is_booked_with_algorithmic_bytes(gpu):
    from edvr_amd import ops
    seen = []

    def hook(name, flops, launch, nbytes, executed):
        seen.append((name, nbytes))
        launch()

    prev, ops.LAUNCH_HOOK = ops.LAUNCH_HOOK, hook
    try:
        ops.imresize(_bytes(2, 64, 96, 1).to(gpu), 1 / 4)
        ops.imresize(torch.rand(1, 3, 30, 44, device=gpu), 2.0, out_dtype=torch.uint8)
    finally:
        ops.LAUNCH_HOOK = prev
    assert seen == [('imresize', 2 * 64 * 96 * 3 + 2 * 3 * 16 * 24 * 4.0), ('imresize', 3 * 30 * 44 * 4.0 + 60 * 88 * 3)]


def _write_gt_tree(root, folders, frames, hw):
    from oracle import data_oracle as DO
    for folder in folders:
        d = os.path.join(root, 'gt', folder)
        os.makedirs(d, exist_ok=True)
        for f in range(frames):
            with open(os.path.join(d, f'{f:08d}.png'), 'wb') as fh:
                fh.write(png_bytes(DO.synthetic_frame('gt', folder, f'{f:08d}', *hw)))


def test_video_clips_derive_lq_from_gt(gpu, tmp_path):
    from edvr_amd import data, metrics, ops
    from util_edvr import build
    _write_gt_tree(str(tmp_path), ['000', '011'], 6, (66, 99))  # mod-cropped to 64 x 96
    opt = dict(name='REDS4', dataroot_gt=str(tmp_path / 'gt'), dataroot_lq=None, lq_from_gt={'scale': 4}, io_backend=dict(type='disk'),
               cache_data=True, num_frame=5, padding='reflection_circle')
    ds = data.VideoTestClips(opt, device=gpu)
    lq, gt = ds.clip('011')
    assert tuple(gt.shape) == (6, 3, 64, 96) and tuple(lq.shape) == (6, 3, 16, 24)
    full = data.read_img_seq(ds.imgs_gt['011'], gpu)
    assert torch.equal(gt, full[:, :, :64, :96])
    want = (to_u8(ops.imresize(gt, 1 / 4)).cpu().float() / 255).to(gpu)
    assert torch.equal(lq, want)  # quantize defaults to True: exactly imresize(gt, 1/4) rounded to 8 bits
    item = ds[len(ds) - 1]
    assert item['folder'] == '011' and torch.equal(item['gt'], gt[5]) and torch.equal(item['lq'][2], lq[5]) and tuple(item['lq'].shape) == (5, 3, 16, 24)
    plain = data.VideoTestClips(dict(opt, lq_from_gt={'scale': 4, 'quantize': False}, cache_data=False), device=gpu)
    assert torch.equal(plain.clip('000')[0], ops.imresize(plain.clip('000')[1], 1 / 4))
    assert torch.equal(plain[0]['lq'][2], plain.clip('000')[0][0])
    net = build('M_T5')[0].to(gpu)
    with torch.no_grad():
        out, psnr = metrics.validate_video(net, lq, gt, num_frame=5, chunk=4)
    assert tuple(out.shape) == tuple(gt.shape) and len(psnr) == 6 and all(p == p for p in psnr)
    # the --bicubic-baseline number of scripts/eval_video.py
    ev = _load_script('eval_video')
    base = ev.bicubic_baseline(lq, gt, chunk=4)
    assert base == metrics.calculate_psnr(data.imresize(lq, 4), gt) and len(base) == 6
    assert ev.bicubic_baseline(lq, gt, crop_border=2, test_y_channel=True) == metrics.calculate_psnr(data.imresize(lq, 4), gt, 2, True)
    assert ev.bicubic_baseline(gt, gt, hr_in=True) == [float('inf')] * 6
