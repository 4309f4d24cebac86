"""-m gpu: every branch of the weight-gradient dispatch (wgrad_impl, csrc/wgrad.hip) through ops.conv2d_wgrad against an fp64 CPU
reference: the fp32 Winograd-domain kernel (what training runs on once the overflow guard has fallen back, or with the split kernels
switched off), its split-operand form on the same rows, every instantiation of the direct kernel (3x3 stride 1 / stride 2, 1x1), the
scalar reduction (co * ci * ks * ks not a multiple of 4), `into=` (dw += ...), a scale sweep of the split kernel and the opt-in
direct split kernel.  Every test asserts the kernel name it means to exercise before it compares numbers.

Tolerances are those of test_gpu_wgrad.py: dW within 2e-5 of max |dW_ref|, db within 2e-5 max(1, |db|max) + 1e-6 sqrt(n h w), and the
dW of the want_db call bit-equal to the dW of the call without."""
import ctypes
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WINO = 'conv3x3_winograd_wgrad_kernel'
WINO_SPLIT = 'conv3x3_winograd_wgrad_split_kernel'
DIRECT_SPLIT = 'conv3x3_wgrad_direct_split_kernel'
TOL = 2e-5

# n, c1, c2, h, w, co, x2_map, layout.  A chunk is 8 tiles (2 x 2 output pixels each) of one tile row; the kernels walk chunk PAIRS.
# layout: '' | 'alias' (x2 is the x1 buffer itself) | 'sliced' (x1 and dz are channel slices of wider tensors)
WINO_CASES = [
    (1, 64, 0, 2, 2, 64, None, ''),             # one tile, one chunk: the second chunk of the only pair is fully masked
    (5, 64, 0, 2, 4, 64, None, ''),             # 5 chunks = 5 images: pairs straddle images, the last pair is half masked
    (1, 64, 0, 4, 6, 64, None, ''),             # (test_gpu_wgrad.py)
    (2, 48, 0, 8, 8, 48, None, ''),             # (test_gpu_wgrad.py) partial ci and co blocks
    (3, 64, 64, 20, 36, 96, None, ''),          # (test_gpu_wgrad.py) concat input, 18 tiles per row, partial co block
    (6, 64, 64, 16, 16, 64, (3, 1, 0), ''),     # (test_gpu_wgrad.py) x2 is a broadcast reference frame
    (2, 64, 0, 6, 18, 64, None, ''),            # 9 tiles per row: the second chunk of a row holds one tile
    (1, 64, 0, 4, 34, 64, None, ''),            # 17 tiles per row: the third chunk holds one tile
    (2, 130, 0, 6, 10, 140, None, ''),          # 3 x 3 blocks, last ci block 2 channels wide, last co block 12
    (1, 51, 0, 8, 12, 49, None, ''),            # forced only; co * ci * 9 odd: scalar reduction + a launch for the bias partials
    (6, 64, 64, 8, 12, 64, (3, 3, 1), 'alias'),  # x2 = the 6-image x1 buffer, image (i // 3) * 3 + 1 (the PCD call site)
    (2, 64, 0, 6, 10, 64, None, 'sliced'),      # x1 = big[:, :64] of 96 channels, dz = bigz[:, 8:72] of 80: image strides != c h w
    # the two rows AUTO accepts (>= 64 chunk pairs; none of the rows above has enough work for its plan)
    (8, 64, 0, 16, 32, 64, None, ''),           # w % 4 == 0: the direct split kernel under EDVR_WGRAD_DIRECT_SPLIT=1
    (6, 64, 64, 16, 34, 64, (3, 1, 0), ''),     # w % 4 == 2: stays on the Winograd-domain kernels; concat + frame map, 17 tiles per row
]

# n, c1, c2, h, w, co, ks, stride, x2_map
DIRECT_CASES = [
    (1, 32, 0, 9, 11, 72, 3, 2, None),          # <3,2,4>, odd sizes
    (2, 20, 0, 16, 12, 20, 3, 2, None),         # <3,2,2> through the MW = 1 bump, partial ci block
    (1, 40, 24, 13, 70, 40, 3, 2, None),        # <3,2,2>, concat, wo = 35: ragged 32-column strips
    (2, 48, 0, 8, 8, 24, 3, 1, None),           # <3,1,1>
    (1, 32, 0, 2, 5, 24, 3, 1, None),           # one strip: units = splits = 1
    (2, 48, 0, 8, 8, 48, 3, 1, None),           # <3,1,2> (test_gpu_wgrad.py)
    (3, 64, 64, 20, 36, 96, 3, 1, None),        # <3,1,4> (test_gpu_wgrad.py)
    (2, 40, 24, 9, 13, 24, 1, 1, None),         # <1,1,1>
    (2, 40, 24, 9, 13, 48, 1, 1, None),         # <1,1,2>
    (4, 64, 64, 6, 10, 100, 1, 1, (2, 1, 0)),   # <1,1,4> with a frame map
    (1, 7, 0, 5, 3, 5, 1, 1, None),             # co * ci % 4 != 0: scalar reduction
]


def _id(c):
    return '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c if v not in (None, ''))


def _full(case):
    """(n, c1, c2, h, w, co, ks, stride, x2_map, layout) of a row of either table."""
    if len(case) == 8:
        n, c1, c2, h, w, co, x2_map, layout = case
        return n, c1, c2, h, w, co, 3, 1, x2_map, layout
    return tuple(case) + ('',)


@functools.lru_cache(maxsize=None)
def _tensors(case):
    """CPU inputs of a row and its fp64 reference (computed once, shared by every test of the row, never written)."""
    n, c1, c2, h, w, co, ks, stride, x2_map, layout = _full(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    pad = ks // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    big = bigz = x2 = None
    if layout == 'sliced':
        big, bigz = torch.randn(n, c1 + 32, h, w, generator=g), torch.randn(n, co + 16, ho, wo, generator=g)
        x1, dz = big[:, :c1], bigz[:, 8:8 + co]
    else:
        x1 = torch.randn(n, c1, h, w, generator=g)
        dz = torch.randn(n, co, ho, wo, generator=g)
    if layout == 'alias':
        x2 = x1
    elif c2:
        x2 = torch.randn(n if x2_map is None else n // x2_map[0], c2, h, w, generator=g)
    xcat = x1
    if c2:
        idx = torch.arange(n) if x2_map is None else (torch.arange(n) // x2_map[0]) * x2_map[1] + x2_map[2]
        xcat = torch.cat([x1, x2[idx]], 1)
    return dict(x1=x1, x2=x2, dz=dz, big=big, bigz=bigz, xcat=xcat)


@functools.lru_cache(maxsize=None)
def _reference(case, sx=1.0, sd=1.0):
    """fp64 weight.grad of F.conv2d(xcat, W) back-propagated with dz (the inputs scaled in fp32 first, as the kernel sees them), and db."""
    n, c1, c2, h, w, co, ks, stride, x2_map, layout = _full(case)
    t = _tensors(case)
    xcat, dz = (t['xcat'] * sx).double(), (t['dz'] * sd).double()
    wt = torch.zeros(co, c1 + c2, ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(xcat, wt, None, stride, ks // 2).backward(dz)
    return wt.grad.detach(), dz.sum((0, 2, 3))


def _algo_id(ops, algo):
    return {'winograd': ops.CONV_WINOGRAD, 'direct': ops.CONV_DIRECT, 'auto': ops.CONV_AUTO}[algo]


def _expected_name(case, algo, split):
    """The kernel the library resolves the row to under `algo` (edvr_conv2d_wgrad_kernel_name) with the renaming ops.conv2d_wgrad
    applies when the split-operand kernels take the call."""
    from edvr_amd import _lib, ops
    n, c1, c2, h, w, co, ks, stride, x2_map, layout = _full(case)
    L = _lib.lib()
    prev = ops.set_wgrad_algo(_algo_id(ops, algo))
    try:
        buf = ctypes.create_string_buffer(96)
        L.edvr_conv2d_wgrad_kernel_name(n, c1, c2, h, w, co, ks, stride, buf, 96)
        name = buf.value.decode()
        if split and name == WINO and L.edvr_conv2d_wgrad_split_applies(n, c1, c2, h, w, co, ks, stride):
            name = DIRECT_SPLIT if L.edvr_conv2d_wgrad_split_is_direct(h, w) else WINO_SPLIT
    finally:
        ops.set_wgrad_algo(prev)
    return name


def _wino_algos(case):
    """`winograd` (forced) and, where its plan accepts the row, `auto`."""
    return ['winograd'] + (['auto'] if _expected_name(case, 'auto', False) == WINO else [])


def _run(case, algo, split, want_db=True, into=None, scale=(1.0, 1.0), loose=False):
    """One ops.conv2d_wgrad call on the row under (algo, ops.F4S_TRAINING = split) -> (dw, db, names of the kernels launched)."""
    from edvr_amd import ops
    n, c1, c2, h, w, co, ks, stride, x2_map, layout = _full(case)
    t = _tensors(case)
    dev = torch.device('cuda:0')
    sx, sd = scale
    if layout == 'sliced':
        x1, dz = (t['big'] * sx).to(dev)[:, :c1], (t['bigz'] * sd).to(dev)[:, 8:8 + co]
        assert x1.stride(0) != c1 * h * w and dz.stride(0) != co * dz.shape[2] * dz.shape[3]
    else:
        x1, dz = (t['x1'] * sx).to(dev), (t['dz'] * sd).to(dev)
    x2 = x1 if layout == 'alias' else (t['x2'] * sx).to(dev) if c2 else None
    if loose:  # bounds 1000 x the true maxima are bounds too
        for v in (x1, dz) + ((x2,) if x2 is not None and x2 is not x1 else ()):
            ops.set_bound(v, ops.amax(v) * 1000.)
    names = []
    prev = ops.set_wgrad_algo(_algo_id(ops, algo))
    prev_f4s = ops.set_f4s(training=split)
    ops.LAUNCH_HOOK = lambda name, flops, launch, *a: (names.append(name), launch())
    try:
        r = ops.conv2d_wgrad(x1, x2, x2_map, dz, co, ks, stride, want_db=want_db, into=into)
    finally:
        ops.LAUNCH_HOOK = None
        ops.set_f4s(*prev_f4s)
        ops.set_wgrad_algo(prev)
    dw, db = r if want_db else (r, None)
    return dw, db, names


def _rel(dw, ref):
    return (dw.cpu().double() - ref).abs().max().item() / ref.abs().max().item()


def _check(case, algo, split, expect, note=''):
    """Kernel name first, then determinism, dW and db against the fp64 reference.  Returns dW's relative error."""
    n, c1, c2, h, w, co, ks, stride, x2_map, layout = _full(case)
    assert _expected_name(case, algo, split) == expect, (case, algo, _expected_name(case, algo, split))
    dw, db, names = _run(case, algo, split)
    dw2, _, names2 = _run(case, algo, split, want_db=False)
    assert expect in names and expect in names2, (expect, names, names2)
    ref, ref_db = _reference(case)
    assert tuple(dw.shape) == tuple(ref.shape)
    assert torch.equal(dw, dw2), 'the split-K reduction must be deterministic, with and without the bias gradient'
    err = _rel(dw, ref)
    print('%s %s %s: dW rel err %.3e%s' % (_id(case), algo, expect, err, note))
    assert err < TOL, (case, algo, expect, err, note)
    edb = (db.cpu().double() - ref_db).abs().max().item()
    assert edb <= TOL * max(1.0, ref_db.abs().max().item()) + 1e-6 * (n * h * w) ** 0.5, (case, algo, edb)
    return err


# ---------------------------------------------------------------------------------------------- (a) fp32 Winograd-domain kernel
@pytest.mark.parametrize('case', WINO_CASES, ids=_id)
def test_fp32_winograd_wgrad(gpu, case):
    for algo in _wino_algos(case):
        _check(case, algo, False, WINO)


# ---------------------------------------------------------------------------------------------- (b) split Winograd-domain kernel
@pytest.mark.parametrize('case', WINO_CASES, ids=_id)
def test_split_winograd_wgrad(gpu, case):
    """The same rows with ops.F4S_TRAINING on.  With EDVR_WGRAD_DIRECT_SPLIT=1 (test_direct_split_opt_in_child) the AUTO rows with
    w % 4 == 0 run on conv3x3_wgrad_direct_split_kernel: the expected name follows edvr_conv2d_wgrad_split_is_direct."""
    for algo in _wino_algos(case):
        expect = _expected_name(case, algo, True)
        assert expect in (WINO_SPLIT, DIRECT_SPLIT), expect
        dw32, _, names = _run(case, algo, False, want_db=False)
        assert WINO in names, names
        _check(case, algo, True, expect, note=' (fp32 kernel: %.3e)' % _rel(dw32, _reference(case)[0]))


# ---------------------------------------------------------------------------------------------- (c) direct kernel instantiations
def _mw(co, stride):
    mw = 4 if co > 64 else 2 if co > 32 else 1
    return 2 if (stride == 2 and mw == 1) else mw


@pytest.mark.parametrize('case', DIRECT_CASES, ids=_id)
def test_direct_wgrad_instantiations(gpu, case):
    n, c1, c2, h, w, co, ks, stride, x2_map = case
    expect = 'conv2d_wgrad_kernel<%d, %d, %d>' % (ks, stride, _mw(co, stride))
    _check(case, 'direct', True, expect)
    if ks == 1 and c2:  # the 1x1 GEMM needs c2 == 0: AUTO must route a concat input to the same direct kernel
        _check(case, 'auto', True, expect)


# ---------------------------------------------------------------------------------------------- (d) into=
INTO_CASES = [  # row, algo, split, kernel, vector reduction (co * ci * ks * ks % 4 == 0)
    ((2, 64, 0, 8, 36, 3, 3, 1, None), 'auto', True, 'wgrad3x3_smallco_kernel', True),
    ((2, 64, 0, 9, 7, 96, 1, 1, None), 'auto', True, 'gemm_nt_kernel', True),
    ((2, 64, 0, 8, 16, 64, 3, 1, None), 'winograd', False, WINO, True),
    ((2, 64, 0, 8, 16, 64, 3, 1, None), 'winograd', True, WINO_SPLIT, True),
    ((1, 32, 0, 9, 11, 72, 3, 2, None), 'direct', True, 'conv2d_wgrad_kernel<3, 2, 4>', True),
    ((1, 51, 0, 8, 12, 49, 3, 1, None), 'winograd', False, WINO, False),
]


@pytest.mark.parametrize('row', INTO_CASES, ids=lambda r: _id(r[0]) + '-' + r[3].split('<')[0] + ('' if r[4] else '-scalar'))
def test_into_accumulates(gpu, row):
    """into += dW within 2e-5 max |dW_ref| + 2e-7 max |into| (half an fp32 ulp of the addend, rounded up); the default still overwrites."""
    case, algo, split, expect, vector = row
    n, c1, c2, h, w, co, ks, stride, x2_map = case
    assert ((co * (c1 + c2) * ks * ks) % 4 == 0) == vector
    assert _expected_name(case, algo, split) == expect
    ref, ref_db = _reference(case)
    before = torch.randn(ref.shape, generator=torch.Generator().manual_seed(zlib.crc32(repr(row).encode())))
    into = before.to(gpu)
    dw, db, names = _run(case, algo, split, into=into)
    assert expect in names, names
    assert dw is into
    err = (into.cpu().double() - (before.double() + ref)).abs().max().item()
    assert err <= TOL * ref.abs().max().item() + 2e-7 * before.abs().max().item(), (err, ref.abs().max().item())
    assert (db.cpu().double() - ref_db).abs().max().item() <= TOL * max(1.0, ref_db.abs().max().item()) + 1e-6 * (n * h * w) ** 0.5
    dw2, _, names2 = _run(case, algo, split, want_db=False)  # default arguments: a fresh tensor, overwritten
    assert expect in names2 and dw2 is not into
    assert _rel(dw2, ref) < TOL


def test_into_is_checked(gpu):
    from edvr_amd import ops
    x, dz = torch.randn(1, 32, 4, 4, device=gpu), torch.randn(1, 32, 4, 4, device=gpu)
    with pytest.raises(AssertionError):
        ops.conv2d_wgrad(x, None, None, dz, 32, 3, 1, into=torch.zeros(32, 32, 1, 1, device=gpu))
    with pytest.raises(NotImplementedError):
        ops.conv2d_wgrad(x, None, None, dz, 32, 3, 1, into=torch.zeros(32, 32, 3, 3))


# ---------------------------------------------------------------------------------------------- (e) scale sweep of the split kernel
SWEEP_CASES = [(2, 64, 0, 12, 20, 64, None, ''),  # forced (AUTO's plan refuses it)
               (8, 64, 0, 16, 32, 64, None, '')]  # AUTO: the direct split kernel under EDVR_WGRAD_DIRECT_SPLIT=1
# inside the range where wgs_scale does not clamp (amax >= 2^-76 ~ 1.3e-23); the products stay normal in fp32
SCALES = [(1e-20, 1e12), (1e-3, 1.0), (1e4, 1e-9), (1e18, 1e-20), (1e-12, 1e-12)]


@pytest.mark.parametrize('scale', SCALES, ids=lambda s: '%g_%g' % s)
@pytest.mark.parametrize('case', SWEEP_CASES, ids=_id)
def test_split_wgrad_scale_sweep(gpu, case, scale):
    """Weight gradients move over many decades during training: the split kernels must hold 2e-5 wherever their power-of-two operand
    scales do not clamp, with the bounds the call measures itself and with bounds 1000 x too loose."""
    algo = _wino_algos(case)[-1]
    expect = _expected_name(case, algo, True)
    assert expect in (WINO_SPLIT, DIRECT_SPLIT), expect
    ref, _ = _reference(case, *scale)
    for loose in (False, True):
        dw, _, names = _run(case, algo, True, want_db=False, scale=scale, loose=loose)
        assert expect in names, names
        assert torch.isfinite(dw).all()
        err = _rel(dw, ref)
        print('%s %s scale %g x %g %s bounds: dW rel err %.3e' % (_id(case), expect, scale[0], scale[1], 'loose' if loose else 'measured', err))
        assert err < TOL, (scale, loose, err)


@pytest.mark.parametrize('case', SWEEP_CASES, ids=_id)
def test_split_wgrad_below_the_scale_clamp_is_finite(gpu, case):
    """max |dz| ~ 4e-30 is below the clamp of wgs_scale (2^-76): the operand scale stops at 2^88 and the f16 pairs lose low bits by
    design - only finiteness is asserted.  Measured on MI355X (relative to max |dW_ref|, not a bound): 9.3e-5 and 7.5e-5 on the
    Winograd-domain split kernel (the two shapes), 5.6e-5 on the direct split kernel (second shape, EDVR_WGRAD_DIRECT_SPLIT=1)."""
    algo = _wino_algos(case)[-1]
    expect = _expected_name(case, algo, True)
    scale = (1.0, 1e-30)
    dw, _, names = _run(case, algo, True, want_db=False, scale=scale)
    assert expect in (WINO_SPLIT, DIRECT_SPLIT) and expect in names, (expect, names)
    assert torch.isfinite(dw).all()
    print('%s %s below the clamp: dW rel err %.3e' % (_id(case), expect, _rel(dw, _reference(case, *scale)[0])))


# ---------------------------------------------------------------------------------------------- (f) the opt-in direct split kernel
def test_direct_split_opt_in_child(gpu):
    """EDVR_WGRAD_DIRECT_SPLIT=1 is read once per process: the split rows and the scale sweep of this file again in ONE child; the AUTO
    rows with w % 4 == 0 then run on conv3x3_wgrad_direct_split_kernel (csrc/wgrad_direct_s.hip), the others stay where they were."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, EDVR_WGRAD_DIRECT_SPLIT='1')
    code = ('import sys; sys.path.insert(0, "tests"); from edvr_amd import _lib; L = _lib.lib(); '
            'assert L.edvr_conv2d_wgrad_split_is_direct(16, 32) == 1 and L.edvr_conv2d_wgrad_split_is_direct(16, 34) == 0; '
            'import test_gpu_wgrad_branches as T; '
            'assert T._expected_name(T.WINO_CASES[-2], "auto", True) == T.DIRECT_SPLIT; '
            'assert T._expected_name(T.WINO_CASES[-1], "auto", True) == T.WINO_SPLIT; '
            'assert T._expected_name(T.WINO_CASES[-2], "winograd", True) == T.WINO_SPLIT; '
            'import pytest; sys.exit(pytest.main(["-q", "-x", "-s", "tests/test_gpu_wgrad_branches.py", "-k", '
            '"test_split_winograd_wgrad or test_split_wgrad_scale_sweep or test_split_wgrad_below"]))')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert ' passed' in r.stdout and 'skipped' not in r.stdout, r.stdout[-2000:]
    assert DIRECT_SPLIT + ':' in r.stdout and DIRECT_SPLIT + ' scale' in r.stdout, 'no row of the child ran on the direct split kernel'
    print('\n'.join(line for line in r.stdout.splitlines() if DIRECT_SPLIT in line))


# ---------------------------------------------------------------------------------------------- (g) coverage of the tables
def test_tables_cover_every_kernel(gpu):
    """The names tables (a)-(c) resolve to: a later edit cannot quietly drop a branch."""
    seen = set()
    for case in WINO_CASES:
        for algo in _wino_algos(case):
            seen.update({_expected_name(case, algo, False), _expected_name(case, algo, True)})
    for case in DIRECT_CASES:
        seen.add(_expected_name(case, 'direct', True))
    want = {WINO, WINO_SPLIT}
    want |= {'conv2d_wgrad_kernel<%d, %d, %d>' % k for k in [(3, 1, 1), (3, 1, 2), (3, 1, 4), (3, 2, 2), (3, 2, 4), (1, 1, 1), (1, 1, 2), (1, 1, 4)]}
    assert want <= seen, sorted(want - seen)
    assert any(_wino_algos(c) == ['winograd', 'auto'] for c in WINO_CASES), 'no row reaches the Winograd-domain kernels through AUTO'
    # the geometry the rows are there for (chunks of 8 tiles per tile row; 64-channel blocks)
    geo = set()
    for n, c1, c2, h, w, co, x2_map, layout in WINO_CASES:
        chunks = n * (h // 2) * -(-(w // 2) // 8)
        geo.update({('chunks', chunks) if chunks in (1, 5) else None, ('tail_tiles', (w // 2) % 8), ('ci_tail', (c1 + c2) % 64), ('co_tail', co % 64),
                    ('scalar', (co * (c1 + c2) * 9) % 4 != 0), ('map', x2_map), layout})
    assert {('chunks', 1), ('chunks', 5), ('tail_tiles', 1), ('ci_tail', 2), ('co_tail', 12), ('scalar', True), ('map', (3, 3, 1)), ('map', (3, 1, 0)),
            'alias', 'sliced'} <= geo
