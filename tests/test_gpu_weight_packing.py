"""-m gpu: the packed weight layouts every convolution reads, unpacked on the host against float64 restatements of the same
operation, and the multi-tensor launch of the training path (csrc/pack.hip, ops.prepack_conv_weights): bit for bit against the
per-tensor packers, its header across calls, and the ownership rules of its in-place rewrite.

A wrong packing neither faults nor makes a NaN - it gives a slightly or grossly wrong network - so the layouts are checked here
directly, with weights of a few hundred kilobytes at the most."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# rows of G of F(4x4, 3x3) (csrc/pack.h) and of F(2x2, 3x3)
G4 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                  dtype=torch.float64)
G2 = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)

# two 11-bit halves below a scaled magnitude of 2^15 (test_split_direct_packing's bound); test_the_split_bound_comes_from_the_reference
# shows the margin a plain fp32 emulation of the packing keeps under it
SPLIT_BOUND = 2.0 ** -21

SHAPES = [(70, 20), (64, 8), (130, 33)]  # (co, ci): both padded; exact blocks; three co blocks with ci % 8 == 1 and ci % 4 == 1


def _rup(v, m):
    return (v + m - 1) // m * m


def _weight(co, ci, k, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(co, ci, k, k, generator=g) * scale


def _src(wt, flip):
    """The kernel a packing stores, (o, c, kh, kw) in float64: the weight itself, or with transpose_flip w[c, o, kk - 1 - t]."""
    w = wt.double()
    return w.flip(2, 3).transpose(0, 1).contiguous() if flip else w


def _transform(G, g):
    return torch.einsum('ri,ocij,sj->ocrs', G, g, G)


def _halves(dwords):
    """int32 dwords -> (hi, lo) in float64: a dword is f16 hi | f16 lo << 16 (little-endian halves)."""
    h = dwords.contiguous().view(torch.float16).view(*dwords.shape, 2).double()
    return h[..., 0], h[..., 1]


def _assert_hi_lo_order(hi, lo):
    """hi is the f16 rounding of the scaled value and lo the f16 of the rest: |lo| is at most half a unit of hi's last place
    (2^-11 |hi| for a normal hi, 2^-25 below the normal range).  The sum alone would not notice the halves changing places."""
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    assert bool((lo.abs() <= torch.clamp(hi.abs() * 2.0 ** -11, min=2.0 ** -25)).all())


def _f4s_index(cop, cip):
    """dword (behind the 16-dword header) of U[o][c][r][cc] in the split F(4x4) layout."""
    o = torch.arange(cop).view(-1, 1, 1, 1)
    c = torch.arange(cip).view(1, -1, 1, 1)
    r = torch.arange(6).view(1, 1, -1, 1)
    cc = torch.arange(6).view(1, 1, 1, -1)
    blk0 = ((o >> 6) * (cip >> 3) + (c >> 3)) * 12 + ((o >> 5) & 1)
    ln = ((c >> 2) & 1) * 32 + (o & 31)
    return (blk0 + 2 * r) * 1536 + cc * 256 + ln * 4 + (c & 3)


def _check_f4s(buf, wt, flip):
    """One split F(4x4) buffer (int32, on the host) against U = G g G^T of `wt` in float64; returns (bits of s_U, worst error / max |w|)."""
    g = _src(wt, flip)
    co, ci = g.shape[:2]
    cop, cip = _rup(co, 64), _rup(ci, 8)
    assert buf.dtype == torch.int32 and buf.numel() == 16 + cop * cip * 36
    s_u, inv = buf[:2].view(torch.float32).tolist()
    top = wt.abs().max().item()
    assert math.frexp(s_u)[0] == 0.5 and s_u * inv == 1.0, (s_u, inv)
    assert 2.0 ** 14 <= top * s_u < 2.0 ** 15, (top, s_u)
    assert not buf[2:16].any()
    idx = _f4s_index(cop, cip)
    assert torch.equal(idx.flatten().sort().values, torch.arange(cop * cip * 36))  # every dword of the body is somebody's
    dwords = buf[16:][idx]                                                          # (cop, cip, 6, 6)
    hi, lo = _halves(dwords)
    _assert_hi_lo_order(hi, lo)
    val = (hi + lo) / s_u
    err = (val[:co, :ci] - _transform(G4, g)).abs().max().item()
    print(f'split F(4x4) {tuple(wt.shape)} flip={flip}: s_U = 2^{math.frexp(s_u)[1] - 1}, error {err / (SPLIT_BOUND * top):.3f} of the bound')
    assert err <= SPLIT_BOUND * top
    assert not dwords[co:].any() and not dwords[:, ci:].any()
    return buf[0].item(), err / top


# ----------------------------------------------------------------------------------------------- 1. host references
def test_the_split_bound_comes_from_the_reference():
    """No GPU: a plain emulation of the split packing (U = G g G^T in fp32, times a power of two s_U with max |w| s_U in
    [2^14, 2^15), two float16 casts) against the float64 U, for weights scaled from 2^-50 to 2^50.  Its worst error is a small
    fraction of 2^-21 max |w|: the bound the device tests assert is the reference's own, with room to spare."""
    worst = 0.0
    for co, ci in SHAPES:
        for e in (-50, -20, 0, 20, 50):
            wt = _weight(co, ci, 3, 100 + co) * 2.0 ** e
            top = wt.abs().max().item()
            s_u = 2.0 ** (14 - (math.frexp(top)[1] - 1))
            assert 2.0 ** 14 <= top * s_u < 2.0 ** 15
            u32 = torch.einsum('ri,ocij,sj->ocrs', G4.float(), wt, G4.float())
            xs = u32 * s_u
            hi = xs.half()
            lo = (xs - hi.float()).half()
            _assert_hi_lo_order(hi.double(), lo.double())
            err = ((hi.double() + lo.double()) / s_u - _transform(G4, wt.double())).abs().max().item()
            worst = max(worst, err / (SPLIT_BOUND * top))
    print(f'fp32 emulation of the split packing: worst error {worst:.3f} of 2^-21 max|w|')
    assert worst <= 0.5


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('co,ci', SHAPES)
def test_split_f4_layout_unpacked(gpu, co, ci, flip):
    """pack_conv_weight(w, f4s=True) of a 3x3 weight, copied to the host: header (s_U a power of two with max |w| s_U in [2^14, 2^15),
    its inverse, zeros), every element (hi + lo) / s_U at its dword within 2^-21 max |w| of G g G^T in float64, hi and lo in
    their halves, every padding dword zero."""
    from edvr_amd import ops
    wt = _weight(ci, co, 3, 11 * co + ci) if flip else _weight(co, ci, 3, 11 * co + ci)
    buf = ops.pack_conv_weight(wt.to(gpu), transpose_flip=flip, f4s=True).cpu()
    assert buf.numel() == 16 + _rup(co, 64) * _rup(ci, 8) * 36
    _check_f4s(buf, wt, flip)


def test_split_f4_layout_follows_the_weight_scale(gpu):
    """One weight set times 2^-50, 2^-20, 1 and 2^50 (inside the unclamped range of f4s_weight_scale_field): the same relative bound,
    s_U moves by exactly the exponent - and since a power of two changes no rounding, the body is the same dwords.  All-zero
    weights: a zero body behind a finite header."""
    from edvr_amd import ops
    base = _weight(70, 20, 3, 5)
    bufs = {}
    for e in (0, -50, -20, 50):
        wt = base * 2.0 ** e
        bufs[e] = ops.pack_conv_weight(wt.to(gpu), f4s=True).cpu()
        field, _ = _check_f4s(bufs[e], wt, False)
        assert field == bufs[0][0].item() - (e << 23), (e, field, bufs[0][0].item())
        assert torch.equal(bufs[e][16:], bufs[0][16:]), e
    z = ops.pack_conv_weight(torch.zeros(70, 20, 3, 3, device=gpu), f4s=True).cpu()
    s_u, inv = z[:2].view(torch.float32).tolist()
    assert math.isfinite(s_u) and math.isfinite(inv) and s_u > 0 and s_u * inv == 1.0
    assert not z[2:].any()


@pytest.mark.parametrize('co,ci', [(33, 136), (200, 640)])
def test_split_1x1_layout_unpacked(gpu, co, ci):
    """pack_conv_weight(w, f4s=True) of a 1x1 weight (the streaming 1x1 kernel's split form): header as the direct-split packer's, body
    [rup(ci, 64) / 4][rup(co, 128)][4] with (hi + lo) / s_W within 2^-21 max |w| of the weight, zero padding."""
    from edvr_amd import _lib, ops
    wt = _weight(co, ci, 1, 3 * co + ci)
    buf = ops.pack_conv_weight(wt.to(gpu), f4s=True).cpu()
    quads, cop = _rup(ci, 64) // 4, _rup(co, 128)
    assert buf.dtype == torch.int32 and buf.numel() == 16 + quads * cop * 4 == _lib.lib().edvr_conv2d_packed_weight_1x1s_elems(co, ci)
    s_w, inv = buf[:2].view(torch.float32).tolist()
    top = wt.abs().max().item()
    assert math.frexp(s_w)[0] == 0.5 and s_w * inv == 1.0 and 2.0 ** 14 <= top * s_w < 2.0 ** 15
    assert not buf[2:16].any()
    body = buf[16:].view(quads, cop, 4)
    hi, lo = _halves(body)
    _assert_hi_lo_order(hi, lo)
    full = ((hi + lo) / s_w).permute(1, 0, 2).reshape(cop, quads * 4)  # (co', channel)
    err = (full[:co, :ci] - wt.double().view(co, ci)).abs().max().item()
    print(f'split 1x1 {(co, ci)}: error {err / (SPLIT_BOUND * top):.3f} of the bound')
    assert err <= SPLIT_BOUND * top
    raw = body.permute(1, 0, 2).reshape(cop, quads * 4)
    assert not raw[co:].any() and not raw[:, ci:].any()


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('co,ci', SHAPES)
def test_direct_layout_and_its_f2_block_unpacked(gpu, co, ci, flip):
    """pack_conv_weight(w) of a 3x3 weight: the direct layout [rup(ci, 16)][9][rup(co, 32)] is the weight bit for bit, the block behind it
    [rup(ci, 16)][16][rup(co, 64)] is U = G2 g G2^T (entry 4 r + col) to 2e-7 max |U| - the tolerance the fp32 F(4x4) layout test uses
    for the same kind of transform - and both are zero in the padding."""
    from edvr_amd import _lib, ops
    wt = _weight(ci, co, 3, 7 * co + ci) if flip else _weight(co, ci, 3, 7 * co + ci)
    buf = ops.pack_conv_weight(wt.to(gpu), transpose_flip=flip).cpu()
    cip, cop32, cop64 = _rup(ci, 16), _rup(co, 32), _rup(co, 64)
    assert buf.dtype == torch.float32 and buf.numel() == cip * 9 * cop32 + cip * 16 * cop64 == _lib.lib().edvr_conv2d_packed_weight_elems(co, ci, 3)
    g = _src(wt, flip)
    want = torch.zeros(cip, 9, cop32)
    want[:ci, :, :co] = g.float().view(co, ci, 9).permute(1, 2, 0)
    assert torch.equal(buf[:cip * 9 * cop32].view(torch.int32), want.flatten().view(torch.int32))
    U = buf[cip * 9 * cop32:].view(cip, 16, cop64)
    ref = _transform(G2, g).view(co, ci, 16).permute(1, 2, 0)  # (c, 4 r + col, o)
    err = (U[:ci, :, :co].double() - ref).abs().max().item()
    print(f'F(2x2) block {tuple(wt.shape)} flip={flip}: error {err / ref.abs().max().item():.2e} of max |U|')
    assert err <= 2e-7 * ref.abs().max().item()
    assert not U[ci:].view(torch.int32).any() and not U[:, :, co:].view(torch.int32).any()


# ----------------------------------------------------------------------------------------------- 2. the multi-tensor launch
# 16 weights.  A job of a 3x3 weight asks for 64 workgroups (the cap) whenever its direct layout is packed; the 1x1 weights give
# 64, 24, 8 and 4, and four equal small jobs in a row make job_of_block's search step over equal sizes.
MULTI_SHAPES = [(128, 128, 3), (64, 3, 3), (3, 64, 3), (216, 128, 3), (70, 20, 3), (130, 33, 3), (48, 32, 3), (64, 640, 1), (48, 96, 1),
                (256, 256, 3), (48, 32, 3), (48, 32, 3), (48, 32, 3), (48, 32, 3), (16, 40, 1), (8, 8, 1)]
NO_FORWARD_F4, NO_DATA_GRADIENT = 0, 3  # the weights whose `meta` rules layouts out


def _cached(ops, w, flip, kind):
    """The buffer the cache holds for a layout, copied to the host - straight from the cache: pack_conv_weight would quietly pack a
    missing one."""
    return ops._PACKED[id(w)][1][(flip, kind)][1].cpu()


def _per_tensor(ops, w, flip, kind):
    """The per-tensor packing of a CLONE of `w` (a cache entry of its own), on the host."""
    c = w.detach().clone()
    return ops.pack_conv_weight(c, transpose_flip=flip, f4=kind is True, f4s=kind == 2).cpu()


def _expected_layouts(shapes, f4s):
    """(weight, flip, kind) the training step asks for: the direct layout always, an F(4x4) layout where f4_weight() gives one
    (3x3, at least 32 input and 48 output channels of the packed orientation), unless `meta` rules it out."""
    out = []
    for i, (co, ci, k) in enumerate(shapes):
        for flip in (False, True):
            if flip and i == NO_DATA_GRADIENT:
                continue
            o, c = (ci, co) if flip else (co, ci)
            out.append((i, flip, False))
            if k == 3 and c >= 32 and o >= 48 and not (i == NO_FORWARD_F4 and not flip):
                out.append((i, flip, 2 if f4s else True))
    return out


def _assert_multi_equals_per_tensor(ops, w, flip, kind, tag):
    got, ref = _cached(ops, w, flip, kind), _per_tensor(ops, w, flip, kind)
    assert got.dtype == ref.dtype and got.shape == ref.shape, tag
    if kind != 2:
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), tag
        return
    assert torch.equal(got[:2], ref[:2]) and torch.equal(got[16:], ref[16:]), tag
    slot = 2 + (ops._PACK_CALLS & 1)
    assert got[slot].item() == w.detach().abs().max().view(torch.int32).item(), (tag, got[:4].tolist())
    assert got[5 - slot].item() == 0 and not got[4:16].any(), (tag, got[:16].tolist())


@pytest.mark.parametrize('f4s', [True, False])
def test_multi_tensor_launch_equals_the_per_tensor_packers(gpu, f4s):
    """Every buffer ops.prepack_conv_weights fills (read from the cache, never through pack_conv_weight) against the per-tensor packing
    of a clone: the direct + F(2x2) and the fp32 F(4x4) layouts whole, the split F(4x4) layout in its scale and body, with max |w| in
    the header slot of the call's parity and zeros in the rest of the header; plus the bookkeeping - the number of jobs, layouts
    `meta` rules out stay absent, nothing to do on a second call, only the touched weight's jobs after an in-place update."""
    from edvr_amd import ops
    g = torch.Generator().manual_seed(123)
    ws = [torch.nn.Parameter((torch.randn(co, ci, k, k, generator=g) * 0.1).to(gpu)) for co, ci, k in MULTI_SHAPES]
    meta = [(i != NO_FORWARD_F4, i != NO_DATA_GRADIENT) for i in range(len(ws))]
    prev = ops.set_f4s(training=f4s)
    try:
        ops.invalidate_packed_weights()
        assert ops.prepack_conv_weights(ws, meta) == 2 * len(ws) - 1  # one job per weight and orientation
        expected = _expected_layouts(MULTI_SHAPES, f4s)
        assert len(expected) == 31 + 10  # a direct layout per job; F(4x4): 5 x (48, 32), (130, 33), (256, 256) twice, one each of the `meta` pair
        assert {(i, flip, kind) for i, w in enumerate(ws) for (flip, kind) in ops._PACKED[id(w)][1]} == set(expected)
        for i, flip, kind in expected:
            _assert_multi_equals_per_tensor(ops, ws[i], flip, kind, (MULTI_SHAPES[i], flip, kind))
        assert ops.prepack_conv_weights(ws, meta) == 0
        for k, n in ((5, 2), (NO_DATA_GRADIENT, 1), (8, 2)):
            with torch.no_grad():
                ws[k].mul_(2.0)  # the version moves, as after an optimizer step
            assert ops.prepack_conv_weights(ws, meta) == n
            for i, flip, kind in expected:
                if i == k:
                    _assert_multi_equals_per_tensor(ops, ws[i], flip, kind, ('after mul_', MULTI_SHAPES[i], flip, kind))
        assert ops.prepack_conv_weights(ws, meta) == 0
    finally:
        ops.set_f4s(training=prev[1])


# ----------------------------------------------------------------------------------------------- 3. the header across calls
@pytest.fixture
def split_training():
    from edvr_amd import ops
    prev = ops.set_f4s(training=True)
    ops.invalidate_packed_weights()
    yield ops
    ops.set_f4s(training=prev[1])


def _params(gpu):
    w = torch.nn.Parameter(_weight(64, 48, 3, 31, 0.1).to(gpu))   # both orientations have a split F(4x4) layout
    v = torch.nn.Parameter(_weight(48, 32, 3, 32, 0.1).to(gpu))   # only there to advance the call counter
    return w, v


def _ptr(ops, w, flip, kind):
    return ops._PACKED[id(w)][1][(flip, kind)][1].data_ptr()


def _assert_split_current(ops, w, tag):
    """Both split F(4x4) layouts of `w` in the cache represent its CURRENT values: unpacked against float64, and equal to a fresh
    per-tensor packing in the scale and the body."""
    for flip in (False, True):
        got, ref = _cached(ops, w, flip, 2), _per_tensor(ops, w, flip, 2)
        print(f'{tag} flip={flip}: header {[hex(x & 0xffffffff) for x in got[:4].tolist()]}, fresh {[hex(x & 0xffffffff) for x in ref[:2].tolist()]}, '
              f'{int((got[16:] != 0).sum())} non-zero body dwords of {int((ref[16:] != 0).sum())}')
        got_fresh_header = got.clone()
        got_fresh_header[2:16] = 0
        _check_f4s(got_fresh_header, w.detach().cpu(), flip)
        assert torch.equal(got[:2], ref[:2]) and torch.equal(got[16:], ref[16:]), (tag, flip)


def test_header_follows_the_weights_down_and_up(split_training, gpu):
    """A weight that takes part in every call: after w / 64 and after w * 192 the in-place rewritten split layout equals a fresh packing in
    scale and body - the maximum the scale is taken from follows the weights down as well as up."""
    ops = split_training
    w, _ = _params(gpu)
    assert ops.prepack_conv_weights([w]) == 2
    ptrs = [_ptr(ops, w, flip, 2) for flip in (False, True)]
    _assert_split_current(ops, w, 'first')
    for f in (1.0 / 64, 64.0 * 3):
        with torch.no_grad():
            w.mul_(f)
        assert ops.prepack_conv_weights([w]) == 2
        assert [_ptr(ops, w, flip, 2) for flip in (False, True)] == ptrs  # rewritten in place: the header is the one that has a history
        _assert_split_current(ops, w, f'x {f:g}')


def test_rejoin_on_the_same_parity(split_training, gpu):
    """prepack(w); prepack(v); w / 64; prepack(w): `w` sits out one call and re-enters on the header slot it used last, which no call
    zeroed for it.  Asserted: its buffers are rewritten in place, and they equal a fresh packing of the current weights in scale and
    body (so: values within 2^-21 of max |w|, a scale no larger and no smaller than a fresh one, nothing overflows) - the maximum
    of two calls ago, 64 times the current one, must not reach the scale."""
    ops = split_training
    w, v = _params(gpu)
    assert ops.prepack_conv_weights([w, v]) == 4
    ptrs = [_ptr(ops, w, flip, 2) for flip in (False, True)]
    with torch.no_grad():
        v.mul_(2.0)
    calls = ops._PACK_CALLS
    assert ops.prepack_conv_weights([v]) == 2
    with torch.no_grad():
        w.mul_(1.0 / 64)
    assert ops.prepack_conv_weights([w]) == 2
    assert ops._PACK_CALLS == calls + 2  # the parity of w's last call
    assert [_ptr(ops, w, flip, 2) for flip in (False, True)] == ptrs
    _assert_split_current(ops, w, 'rejoin')


def test_rejoin_on_the_same_parity_after_a_non_finite_weight(split_training, gpu):
    """One weight is +inf while `w` is packed; then the finite weights come back, one call passes without `w`, and `w` is packed again
    on the parity of the call that saw the inf.  The result must represent the finite weights within the 2^-21 bound - not the zeros
    a scale taken from a left-over infinite maximum gives - and equal a fresh packing in scale and body."""
    ops = split_training
    w, v = _params(gpu)
    w0 = w.detach().clone()
    assert ops.prepack_conv_weights([w, v]) == 4
    ptrs = [_ptr(ops, w, flip, 2) for flip in (False, True)]
    with torch.no_grad():
        w[5, 7, 1, 2] = float('inf')
    assert ops.prepack_conv_weights([w]) == 2
    assert [_ptr(ops, w, flip, 2) for flip in (False, True)] == ptrs
    print('header with the inf:', [hex(x & 0xffffffff) for x in _cached(ops, w, False, 2)[:4].tolist()])
    with torch.no_grad():
        w.copy_(w0)
        v.mul_(2.0)
    assert ops.prepack_conv_weights([v]) == 2
    assert ops.prepack_conv_weights([w]) == 2
    assert [_ptr(ops, w, flip, 2) for flip in (False, True)] == ptrs
    _assert_split_current(ops, w, 'after the inf')


# ----------------------------------------------------------------------------------------------- 4. ownership of the in-place rewrite
def _bump(w, f=2.0):
    with torch.no_grad():
        w.mul_(f)


def test_in_place_rewrite_only_of_buffers_the_cache_owns_alone(split_training, gpu):
    """prepack_conv_weights: the cache as sole owner keeps every buffer's address across an update; a buffer the caller holds, or one
    pinned with pin_packed_weights, is replaced by a new one and keeps its old contents bit for bit; once released, in-place reuse
    resumes."""
    ops = split_training
    w, _ = _params(gpu)
    keys = [(False, False), (False, 2), (True, False), (True, 2)]

    def ptrs():
        return {k: _ptr(ops, w, *k) for k in keys}

    assert ops.prepack_conv_weights([w]) == 2
    first = ptrs()
    _bump(w)
    assert ops.prepack_conv_weights([w]) == 2
    assert ptrs() == first
    # a reference somebody holds
    held = ops._PACKED[id(w)][1][(False, 2)][1]
    before = held.clone()
    _bump(w)
    assert ops.prepack_conv_weights([w]) == 2
    now = ptrs()
    assert now[(False, 2)] != held.data_ptr() and {k: p for k, p in now.items() if k != (False, 2)} == {k: p for k, p in first.items() if k != (False, 2)}
    assert torch.equal(held, before)
    _assert_split_current(ops, w, 'held')
    del held
    _bump(w)
    assert ops.prepack_conv_weights([w]) == 2
    assert ptrs() == now
    # pinned buffers
    pinned = ops.pin_packed_weights([w])
    assert {b.data_ptr() for b in pinned} == set(now.values())
    old = [b.clone() for b in pinned]
    _bump(w)
    assert ops.prepack_conv_weights([w]) == 2
    fresh = ptrs()
    assert not set(fresh.values()) & set(now.values())
    assert all(torch.equal(b, c) for b, c in zip(pinned, old))
    _assert_split_current(ops, w, 'pinned')
    ops.unpin_packed_weights(pinned)
    del pinned
    _bump(w)
    assert ops.prepack_conv_weights([w]) == 2
    assert ptrs() == fresh
    _assert_split_current(ops, w, 'released')


def test_split_1x1_layout_is_rewritten_in_place_under_the_same_rule(split_training, gpu):
    """pack_conv_weight(w, f4s=True) of a 1x1 weight (not part of the multi-tensor table): the stale buffer is rewritten in place when the
    cache owns it alone, replaced while the caller holds it or it is pinned - the old one keeping its contents."""
    ops = split_training
    w = torch.nn.Parameter(_weight(64, 320, 1, 41, 0.1).to(gpu))
    key = (False, 2)

    def pack():
        ops.pack_conv_weight(w, f4s=True)
        return _ptr(ops, w, *key)

    def current():
        assert torch.equal(_cached(ops, w, *key), _per_tensor(ops, w, *key))

    first = pack()
    _bump(w)
    assert pack() == first
    current()
    held = ops.pack_conv_weight(w, f4s=True)
    before = held.clone()
    _bump(w)
    second = pack()
    assert second != first and held.data_ptr() == first and torch.equal(held, before)
    current()
    del held
    _bump(w)
    assert pack() == second
    current()
    pinned = ops.pin_packed_weights([w])
    assert [b.data_ptr() for b in pinned] == [second]
    before = pinned[0].clone()
    _bump(w)
    third = pack()
    assert third != second and torch.equal(pinned[0], before)
    current()
    ops.unpin_packed_weights(pinned)
    del pinned
    _bump(w)
    assert pack() == third
    current()
