"""Tensor-level wrappers over the C ABI (no autograd here; see edvr_amd/functional.py).

PyTorch is plumbing only: it owns device memory and the current HIP stream.  Every
function launches hand-written HIP kernels from libedvr_amd.so on
``torch.cuda.current_stream()`` and never synchronises.
"""
import ctypes
import os
import weakref

import torch

from . import _lib
from .bars import check_rect
from ._lib import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, CONV_AUTO, CONV_DIRECT, CONV_WINOGRAD, CONV_WINOGRAD_F4, CONV_WINOGRAD_F4S, OUT_NCHW,  # noqa: F401
                   OUT_PIXEL_SHUFFLE2)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def require_gpu(*tensors, dtypes=(torch.float32,)):
    """Same refusal as the reference (deform_conv.py:133-134): no CPU path exists.  Everything is fp32 except the DCN operators,
    which also take float64 / float16 like the reference's dispatch (`dtypes`); the tensors of one call share one type."""
    seen = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
        if t.dtype not in dtypes:
            raise NotImplementedError(f'edvr_amd: {t.dtype} is not supported here (supported: {", ".join(map(str, dtypes))})')
        if seen is not None and t.dtype != seen:
            raise RuntimeError(f'expected every tensor of the call to be {seen}, got {t.dtype}')  # (the reference: "expected scalar type ...")
        seen = t.dtype
    return seen


DCN_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float64: _lib.DTYPE_F64, torch.float16: _lib.DTYPE_F16}


def _plane_contig(t):
    """(n, c, h, w) whose (c, h, w) block is dense; the image stride may be larger (channel-sliced view)."""
    n, c, h, w = t.shape
    return t.stride(3) == 1 and t.stride(2) == w and t.stride(1) == h * w and (n == 1 or t.stride(0) >= c * h * w)


def _as_planes(t):
    return t if _plane_contig(t) else t.contiguous()


def _img_stride(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2] * t.shape[3]


def _run(name, launch, flops=0.0, nbytes=0.0, executed=None):
    """Every launch of this module goes through here: LAUNCH_HOOK (bench.py's instrumented pass) brackets it with events on
    the launch stream and books `flops` / `nbytes` (ALGORITHMIC work of the call: each input / output element once) and
    `executed` (flops the matrix cores issue for it, padding included; None = not known here) under `name`."""
    if LAUNCH_HOOK is not None:
        LAUNCH_HOOK(name, float(flops), launch, float(nbytes), executed)
    else:
        launch()


def _nb(*ts):
    return 4.0 * sum(t.numel() for t in ts if t is not None)


# ------------------------------------------------------------------------------------------------ workspace
_WS = {}


def workspace(nbytes, device, tag=None):
    """Grow-only scratch buffer per (device, stream).  288 GB of HBM: keep it resident, never free per call.
    tag: a buffer of its own per tag, for state that must survive other launches (None: the kernels' scratch, rewritten by any call)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream) if tag is None else (device.index, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _WS.pop(key, None)
        buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


# ------------------------------------------------------------------------------------------------ weights
_PACKED = {}  # id(parameter) -> (weakref, {(transpose_flip, layout): (version, packed, data_ptr[, _PACK_CALLS of the multi launch that filled it])})


def pack_conv_weight(weight, transpose_flip=False, f4=False, f4s=False, ci_range=None, ds=False):
    """(co, ci, k, k) parameter -> MFMA-friendly [ci_pad][k*k][co_pad] array, cached per parameter version.
    ci_range = (lo, hi): the packing of weight[:, lo:hi] alone - one half of a two-input conv whose other half is convolved apart
    (conv2d's `pre`); cached in a slot of its own under the same parameter, version and pointer, so it is invalidated and pinned with the rest.
    f4: the F(4x4,3x3) Winograd weights of a 3x3 kernel instead (conv2d's `wpk_f4`), a separate buffer with its own cache slot.
    f4s: the same weights for the split-operand kernel (conv2d's `wpk_f4s`: scaled, split into f16 (hi, lo) pairs; int32 buffer); of a
    1x1 kernel: the split-operand packing of the streaming 1x1 kernel (csrc/conv1x1_s.hip), same field.
    ds: the split-operand packing of the DIRECT kernel (conv2d's `wpk_ds`, csrc/conv2d_s.hip: 3x3 or 1x1, forward orientation only; int32
    buffer), a cache slot of its own."""
    require_gpu(weight)
    assert not (ds and (f4 or f4s or transpose_flip)), 'ds is a layout of its own, of the forward orientation'
    key, wid, ver = (bool(transpose_flip), 3 if ds else (2 if f4s else bool(f4))), id(weight), weight._version
    if ci_range is not None:
        assert not transpose_flip, 'input-channel ranges serve forward convs'
        key = key + ((int(ci_range[0]), int(ci_range[1])),)
    ent = _PACKED.get(wid)
    if ent is not None and ent[0]() is weight:
        hit = ent[1].get(key)
        if hit is not None and hit[0] == ver and hit[2] == weight.data_ptr():
            return hit[1]
    else:
        ent = (weakref.ref(weight, lambda _r, wid=wid: _PACKED.pop(wid, None)), {})
        _PACKED[wid] = ent
    L = _lib.lib()
    w = weight.detach()
    if ci_range is not None:
        w = w[:, ci_range[0]:ci_range[1]]
    if not w.is_contiguous():
        w = w.contiguous()
    o, i, k, k2 = w.shape
    assert k == k2, 'square kernels only'
    co, ci = (i, o) if transpose_flip else (o, i)
    if ds:
        out = torch.empty(L.edvr_conv2d_packed_weight_ds_elems(co, ci, k), dtype=torch.int32, device=w.device)
        _lib.check(L.edvr_conv2d_pack_weight_ds_f32(_ptr(w), _ptr(out), co, ci, k, _stream()), 'edvr_conv2d_pack_weight_ds_f32')
    elif f4s and k == 1:  # the split-operand packing of a 1x1 conv (csrc/conv1x1_s.hip)
        assert not transpose_flip, 'the split 1x1 kernel serves forward convs'
        n_el = L.edvr_conv2d_packed_weight_1x1s_elems(co, ci)
        stale = ent[1].get(key)  # this layout is not part of prepack_conv_weights' table: rewritten in place here under the same rule
        if stale is not None and stale[1].numel() == n_el and stale[1].device == w.device and _sole_owner(stale):
            out = stale[1]
        else:
            out = torch.empty(n_el, dtype=torch.int32, device=w.device)
        _lib.check(L.edvr_conv2d_pack_weight_1x1s_f32(_ptr(w), _ptr(out), co, ci, _stream()), 'edvr_conv2d_pack_weight_1x1s_f32')
    elif f4s:
        assert k == 3, 'F(4x4,3x3) weights are for 3x3 kernels'
        out = torch.empty(L.edvr_conv2d_packed_weight_f4s_elems(co, ci), dtype=torch.int32, device=w.device)
        _lib.check(L.edvr_conv2d_pack_weight_f4s_f32(_ptr(w), _ptr(out), co, ci, 1 if transpose_flip else 0, _stream()),
                   'edvr_conv2d_pack_weight_f4s_f32')
    elif f4:
        assert k == 3, 'F(4x4,3x3) weights are for 3x3 kernels'
        out = torch.empty(L.edvr_conv2d_packed_weight_f4_elems(co, ci), dtype=torch.float32, device=w.device)
        _lib.check(L.edvr_conv2d_pack_weight_f4_f32(_ptr(w), _ptr(out), co, ci, 1 if transpose_flip else 0, _stream()),
                   'edvr_conv2d_pack_weight_f4_f32')
    else:
        out = torch.empty(L.edvr_conv2d_packed_weight_elems(co, ci, k), dtype=torch.float32, device=w.device)
        _lib.check(L.edvr_conv2d_pack_weight_f32(_ptr(w), _ptr(out), co, ci, k, 1 if transpose_flip else 0, _stream()),
                   'edvr_conv2d_pack_weight_f32')
    ent[1][key] = (ver, out, weight.data_ptr())
    return out


def pack_dcn_split_weight(weight):
    """The (Co, C, 3, 3) weight of a DCN layer in the layout of the split-operand tap-window kernel (csrc/dcn_tapwin_s.hip: scale pre-pass +
    packing, the two launches edvr_dcnv2_fwd_split_f32 issues at EVERY call), cached per parameter version like the conv layouts: same
    key (id, version, pointer) under a layout slot of its own, dropped by invalidate_packed_weights, pinned by pin_packed_weights.  int32
    buffer of edvr_dcnv2_split_packed_weight_elems(Co, C) dwords for dcnv2_forward's packed entry point."""
    require_gpu(weight)
    key, wid, ver = ('dcn_split',), id(weight), weight._version
    ent = _PACKED.get(wid)
    if ent is not None and ent[0]() is weight:
        hit = ent[1].get(key)
        if hit is not None and hit[0] == ver and hit[2] == weight.data_ptr():
            return hit[1]
    else:
        ent = (weakref.ref(weight, lambda _r, wid=wid: _PACKED.pop(wid, None)), {})
        _PACKED[wid] = ent
    L = _lib.lib()
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    co, c = w.shape[0], w.shape[1]
    n_el = L.edvr_dcnv2_split_packed_weight_elems(co, c)
    stale = ent[1].get(key)  # rewritten in place under the rule of the 1x1 split layout: only when the cache is the buffer's sole owner
    if stale is not None and stale[1].numel() == n_el and stale[1].device == w.device and _sole_owner(stale):
        out = stale[1]
    else:
        out = torch.empty(n_el, dtype=torch.int32, device=w.device)
    _run('dcn_split_pack_weight', lambda: _lib.check(L.edvr_dcnv2_split_pack_weight_f32(_ptr(w), _ptr(out), co, c, _stream()),
                                                     'edvr_dcnv2_split_pack_weight_f32'), 0, _nb(w) + 4.0 * n_el)
    ent[1][key] = (ver, out, weight.data_ptr())
    return out


_PACK_CALLS = 0   # edvr_conv2d_pack_weights_multi's split_parity counter
_PACK_TABLES = {}  # job signature -> (device table, total blocks): the table of a training iteration never changes


_PINNED_PACKED = set()  # data_ptr()s of packed buffers somebody outside the cache relies on (a captured hipGraph): never rewritten


def pin_packed_weights(weights):
    """Keep the CURRENT packed layouts of `weights` alive and unmodified: returns the list of buffers (hold it as long as they are
    needed - e.g. a captured hipGraph whose launches read them, edvr_amd/graphs.py) after registering them so that
    prepack_conv_weights allocates fresh buffers instead of rewriting these.  Release with unpin_packed_weights(list)."""
    bufs = []
    for w in weights:
        ent = _PACKED.get(id(w))
        if ent is not None and ent[0]() is w:
            bufs.extend(hit[1] for hit in ent[1].values())
    _PINNED_PACKED.update(b.data_ptr() for b in bufs)
    return bufs


def unpin_packed_weights(bufs):
    for b in bufs:
        _PINNED_PACKED.discard(b.data_ptr())


def _sole_owner(hit):
    """The cache entry `hit` = (version, buffer, pointer) is the only holder of its buffer: no other Python reference, no view, no
    C++ holder (autograd node, graph), not pinned.  Only then may the buffer be rewritten in place."""
    import sys
    return hit[1]._use_count() == 1 and sys.getrefcount(hit[1]) == 2 and hit[1].data_ptr() not in _PINNED_PACKED


def prepack_conv_weights(weights, meta=None):
    """Fill the packed-weight cache for a whole network in ONE launch (edvr_conv2d_pack_weights_multi): every (weight, orientation)
    the training step will ask pack_conv_weight / f4_weight for whose cached copy is stale - after an optimizer step: all of them,
    ~480 separate ~5 us launches otherwise.  `weights`: iterable of conv weight Parameters (3x3 or 1x1); `meta` (optional, same
    length): (forward_f4, data_gradient) per weight - False skips layouts the autograd path never requests (the F(4x4) forward
    layout of a stride-2 conv, the flipped layouts of a conv whose input needs no gradient).  Purely an optimisation: whatever is
    not packed here is packed lazily, one launch per request, as before.
    A stale buffer is REWRITTEN IN PLACE when the cache is its only owner (`_sole_owner`: nobody else holds the tensor, it is not
    pinned by a captured graph), so that the job table is built and uploaded once; otherwise a fresh buffer is allocated and the
    old one stays as it was for whoever holds it.  The rewrite is ordered behind the buffer's readers on the CURRENT stream only:
    work queued on another stream that still reads a packed layout must be synchronised with by the caller (single-stream
    assumption of the training loop; GraphedEDVR pins its layouts instead)."""
    import numpy as np
    global _PACK_CALLS
    L = _lib.lib()
    jobs, sig, filled = [], [], []
    meta = list(meta) if meta is not None else None
    for wi, w in enumerate(weights):
        fwd_f4, dgrad = meta[wi] if meta is not None else (True, True)
        if not w.is_cuda or w.dtype != torch.float32 or w.dim() != 4 or w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3) or not w.is_contiguous():
            continue
        wid, ver, k = id(w), w._version, w.shape[2]
        ent = _PACKED.get(wid)
        if ent is None or ent[0]() is not w:
            ent = (weakref.ref(w, lambda _r, wid=wid: _PACKED.pop(wid, None)), {})
            _PACKED[wid] = ent
        for flip in ((False, True) if dgrad else (False,)):
            co, ci = (w.shape[1], w.shape[0]) if flip else (w.shape[0], w.shape[1])
            want_f4 = F4_TRAINING and k == 3 and ci >= 32 and co >= 48 and (flip or fwd_f4)  # = f4_weight()
            # which layouts: the direct one always; of the two F(4x4) layouts the one the training convs will ask for (f4_kwargs)
            kinds = [False] + ([2 if F4S_TRAINING else True] if want_f4 else [])
            outs = []
            for f4 in kinds:
                hit = ent[1].get((flip, f4))
                if hit is not None and hit[0] == ver and hit[2] == w.data_ptr():
                    outs.append(None)  # current
                    continue
                if f4 == 2:
                    n, dt = L.edvr_conv2d_packed_weight_f4s_elems(co, ci), torch.int32
                else:
                    n, dt = (L.edvr_conv2d_packed_weight_f4_elems(co, ci) if f4 else L.edvr_conv2d_packed_weight_elems(co, ci, k)), torch.float32
                if hit is not None and hit[1].numel() == n and hit[1].dtype == dt and hit[1].device == w.device and _sole_owner(hit):
                    buf = hit[1]
                    if f4 == 2 and len(hit) > 3 and hit[3] != _PACK_CALLS:
                        # it sat out the last call(s): nobody zeroed the max |w| slot this call accumulates into, and after an odd number
                        # of them that is the slot of its own last call - an old, larger maximum would cost precision, an infinite one
                        # would scale every weight to zero.  (One tiny launch, only on this rare path.)
                        buf[2:4].zero_()
                else:
                    buf = torch.empty(n, dtype=dt, device=w.device)
                    if f4 == 2:
                        buf[:16].zero_()  # the header's max |w| slots start at zero (edvr_conv2d_pack_weights_multi)
                outs.append(buf)
                filled.append((ent, (flip, f4), ver, buf, w.data_ptr()))
            wpk = outs[0]
            wf4 = outs[1] if (want_f4 and not F4S_TRAINING) else None
            wf4s = outs[1] if (want_f4 and F4S_TRAINING) else None
            if wpk is None and wf4 is None and wf4s is None:
                continue
            wq = wf4 if wf4 is not None else wf4s
            work = max((wpk.numel() if wpk is not None else 0), (wq.numel() // 36 if wq is not None else 0))
            jobs.append((w.data_ptr(), wpk.data_ptr() if wpk is not None else 0, wf4.data_ptr() if wf4 is not None else 0, co, ci, k,
                         int(flip), max(1, min(64, (work + 255) // 256)), wf4s.data_ptr() if wf4s is not None else 0))
    if not jobs:
        return 0
    key = tuple(jobs)  # (device pointers inside: unique per device)
    tab = _PACK_TABLES.get(key)
    if tab is None:
        rec = np.zeros(len(jobs), dtype=np.dtype([('w', '<u8'), ('wpk', '<u8'), ('f4', '<u8'), ('co', '<i4'), ('ci', '<i4'), ('ks', '<i4'),
                                                  ('flip', '<i4'), ('first', '<i4'), ('nb', '<i4'), ('f4s', '<u8'), ('pad', '<i4', (2,))]))
        assert rec.dtype.itemsize == L.edvr_pack_job_bytes()
        first = 0
        for i, (pw, pk, pf, co, ci, k, flip, nb, ps) in enumerate(jobs):
            rec[i] = (pw, pk, pf, co, ci, k, flip, first, nb, ps, (0, 0))
            first += nb
        dev = filled[0][3].device
        tab = (torch.from_numpy(rec.view(np.uint8).copy()).to(dev), first)
        if len(_PACK_TABLES) > 8:
            _PACK_TABLES.clear()
        _PACK_TABLES[key] = tab
    _PACK_CALLS += 1
    parity = _PACK_CALLS if any(j[8] for j in jobs) else -1
    _lib.check(L.edvr_conv2d_pack_weights_multi(_ptr(tab[0]), len(jobs), tab[1], parity, _stream()), 'edvr_conv2d_pack_weights_multi')
    for ent, k2, ver, buf, ptr in filled:
        ent[1][k2] = (ver, buf, ptr, _PACK_CALLS)  # (the call it took part in: the header slots of a split layout alternate per call)
    return len(jobs)


def f4_weight(weight, ks, transpose_flip=False):
    """The F(4x4,3x3) packing of a 3x3 weight for the training path, or None when that path is off / the layer too small."""
    if not F4_TRAINING or ks != 3:
        return None
    co, ci = (weight.shape[1], weight.shape[0]) if transpose_flip else (weight.shape[0], weight.shape[1])
    return pack_conv_weight(weight, transpose_flip=transpose_flip, f4=True) if (ci >= 32 and co >= 48) else None


def f4_kwargs(weight, ks, transpose_flip=False):
    """The F(4x4) weights a training-path conv2d() call should get: {'wpk_f4s': ...} (split-operand kernel), {'wpk_f4': ...} (fp32
    kernel) or {} when the F(4x4) path is off / the layer too small."""
    if ks == 1 and F4S_TRAINING and not transpose_flip and weight.shape[1] >= 320 and weight.shape[1] % 8 == 0:
        return {'wpk_f4s': pack_conv_weight(weight, f4s=True)}  # the streaming 1x1 kernel's split form (csrc/conv1x1_s.hip; forward only)
    if not F4_TRAINING or ks != 3:
        return {}
    co, ci = (weight.shape[1], weight.shape[0]) if transpose_flip else (weight.shape[0], weight.shape[1])
    if not (ci >= 32 and co >= 48):
        return {}
    if F4S_TRAINING:
        return {'wpk_f4s': pack_conv_weight(weight, transpose_flip=transpose_flip, f4s=True)}
    return {'wpk_f4': pack_conv_weight(weight, transpose_flip=transpose_flip, f4=True)}


def invalidate_packed_weights():
    """Drop every cached packed weight.  The cache follows a parameter's autograd version and storage pointer, which in-place
    torch ops, optimizers and load_state_dict maintain; a write through `.data` (or through a raw pointer that does not call
    torch.autograd.graph.increment_version afterwards) does not - call this after such a write.  The cached weight norms behind
    linear_bound() (the magnitude bounds of the split-operand kernels) follow the same key and are dropped with them."""
    _PACKED.clear()
    _W_L1.clear()


# ------------------------------------------------------------------------------------------------ conv
DCN_SCATTER_AUTO, DCN_SCATTER_DEVICE, DCN_SCATTER_LDS, DCN_SCATTER_STRIP, DCN_SCATTER_LDS_WIDE = 0, 1, 2, 3, 4  # include/edvr_amd.h EDVR_DCN_SCATTER_*
_SCATTER_NAMES = {0: '[auto]', 1: '[device atomics]', 2: '[lds window]', 3: '[strip / fused]', 4: '[lds window]'}  # measurement label of dcnv2_backward's dX strategy
DCN_HALO_TAPWIN = _lib.DCN_HALO_TAPWIN  # halo_hint of dcnv2_forward: per-tap shifted windows (csrc/dcn_tapwin.hip)
LAUNCH_HOOK = None  # callable(kernel_name, algorithmic_flops, launch_fn, algorithmic_bytes) or None
CONV_ALGO = CONV_AUTO  # default algorithm request of conv2d(); tests flip it to cover both kernels on every shape
F4_INFERENCE = os.environ.get('EDVR_WINOGRAD_F4', '1') != '0'  # functional.conv hands the F(4x4,3x3) weights to no-grad convs
F4S_INFERENCE = os.environ.get('EDVR_WINOGRAD_F4S', '1') != '0'  # functional.conv hands the split-operand F(4x4) weights (csrc/winograd_f4s.hip) to no-grad convs
F4S_TRAINING = os.environ.get('EDVR_WINOGRAD_F4S_TRAIN', os.environ.get('EDVR_WINOGRAD_F4S', '1')) != '0'  # ... and to the forward / data-gradient convs of autograd.py
F4_TRAINING = os.environ.get('EDVR_WINOGRAD_F4_TRAIN', '1') != '0'  # autograd.py: forward and data-gradient convs too (-11 % per iteration;
#                                                                   the gradient parity tests hold at their 1e-5 bounds)


def set_f4(inference=None, training=None):
    """Switch the F(4x4,3x3) Winograd kernel on / off at run time for the no-grad path (`inference`) and for the forward / data-gradient
    convs of the training path (`training`); None leaves a setting alone.  Returns the previous (inference, training) pair.  The
    environment variables EDVR_WINOGRAD_F4 / EDVR_WINOGRAD_F4_TRAIN only give the initial values.  (F(4x4) rounds at ~1e-6 of the
    output scale, F(2x2) at ~2e-7.)"""
    global F4_INFERENCE, F4_TRAINING
    prev = (F4_INFERENCE, F4_TRAINING)
    if inference is not None:
        F4_INFERENCE = bool(inference)
    if training is not None:
        F4_TRAINING = bool(training)
    return prev


def set_f4s(inference=None, training=None):
    """Switch the SPLIT-OPERAND form of the F(4x4,3x3) kernel (csrc/winograd_f4s.hip) on / off at run time for the no-grad path and
    for the training path; with it off the fp32 F(4x4) kernel runs (set_f4).  Returns the previous pair.  EDVR_WINOGRAD_F4S /
    EDVR_WINOGRAD_F4S_TRAIN give the initial values."""
    global F4S_INFERENCE, F4S_TRAINING
    prev = (F4S_INFERENCE, F4S_TRAINING)
    if inference is not None:
        F4S_INFERENCE = bool(inference)
    if training is not None:
        F4S_TRAINING = bool(training)
    return prev


class _AmaxArena:
    """One-element device slots for the `y_amax` epilogue of the split-operand kernels and for the reduction passes: zeroed in blocks of
    2048, each slot handed out once.  A hipGraph capture (graphs.GraphedEDVR) takes a fresh block, zeroes it in its first node and
    keeps it to itself: every replay starts from zeroed slots, as an eager forward does.  One arena per (device, stream): a block is
    zero-filled on the stream that uses it.  The slots handed out since the last guard_submit() are what the overflow guard
    examines (a non-finite maximum = non-finite values left a split-operand kernel)."""

    BLOCK = 2048

    def __init__(self):
        self.buf, self.i, self.mark, self.retired = None, 0, 0, []

    def fresh(self, device):
        """Start a new block now (GraphedEDVR: BEFORE a capture, so that no allocation / zero-fill is recorded into the graph)."""
        if self.buf is not None and self.i > self.mark:
            self.retired.append(self.buf[self.mark:self.i])
        self.buf, self.i, self.mark = torch.zeros(self.BLOCK, dtype=torch.float32, device=device), 0, 0

    def slot(self, device):
        if self.buf is None or self.i >= self.buf.numel():
            if self.buf is not None and device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('edvr_amd: the magnitude-bound arena ran out of slots inside a hipGraph capture (more than '
                                   f'{self.BLOCK} split-operand launches in one captured region); capture a smaller region')
            self.fresh(device)
        self.i += 1
        return self.buf[self.i - 1:self.i]

    def take_unexamined(self):
        out, self.retired = self.retired, []
        if self.buf is not None and self.i > self.mark:
            out.append(self.buf[self.mark:self.i])
            self.mark = self.i
        return out


_AMAX_ARENAS = {}  # (device index, stream handle) -> _AmaxArena


def _arena(device):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    a = _AMAX_ARENAS.get(key)
    if a is None:
        a = _AMAX_ARENAS[key] = _AmaxArena()
    return a


def reserve_amax_slots(device):
    """A fresh, zero-filled block of bound slots for the current stream of `device`: call before a hipGraph capture."""
    _arena(device).fresh(device)


BOUND_CHECK = os.environ.get('EDVR_BOUND_CHECK', '0') == '1'  # verify every x_amax against the data (tests / debugging)
BOUND_CHECK_LOG = []  # (shape, bound / true maximum) of every checked conv input of the kernels that both paths have (a split conv of the
#                       no-grad path has a forward and a data-gradient twin in training: consumers compare the counts of the two)
BOUND_CHECK_LOG_DIRECT = []  # the same records for the split-operand DIRECT kernel (csrc/conv2d_s.hip), which the no-grad path alone launches
AMAX_LOG = None  # a list: every reduction pass of input_bound() is recorded there (shape, calling functions)
AMAX_PASSES = 0  # how often input_bound() had to run the reduction kernel (measurement: bench.py reports it per forward)


# ---- overflow guard of the split-operand path.  The split kernels place their operands in the f16 range from magnitude BOUNDS; a bound
# that is too small (a stale one: a raw-pointer write behind torch's back) overflows f16 to inf and the products to NaN - silently.
# Every split conv leaves max |y| in an arena slot with non-finite values STICKY (NaN bits order above every finite number), the
# reduction kernel does the same, so one 2048-element max per forward says whether anything non-finite passed through a split
# kernel.  It is read like the offset statistics: copy to pinned memory behind an event, examined when the next forward starts (or by
# split_guard_check(wait=True)); no forward waits for the GPU.
class SplitOperandOverflow(RuntimeError):
    pass


SPLIT_GUARD = os.environ.get('EDVR_SPLIT_GUARD', 'raise')  # 'raise' | 'fallback' (warn once, continue on the fp32 kernels) | 'off'
_GUARD_PENDING = []  # (pinned 1-element host tensor, copy-done event)
GUARD_TRIPS = 0


def split_guard_submit(device, parts=None):
    """Fold the bound slots handed out on the current stream since the last call (or `parts`: the slots of a replayed hipGraph) into
    one flag and send it to the host (no wait)."""
    if SPLIT_GUARD == 'off' or device.type != 'cuda' or torch.cuda.is_current_stream_capturing():
        return
    if parts is None:
        parts = _arena(device).take_unexamined()
    if not parts:
        return
    with torch.no_grad():
        worst = (parts[0] if len(parts) == 1 else torch.cat(parts)).max().reshape(1)  # torch.max propagates NaN
    host = torch.empty(1, dtype=torch.float32, pin_memory=True)
    host.copy_(worst, non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    _GUARD_PENDING.append((host, done))
    if len(_GUARD_PENDING) > 64:
        split_guard_check(wait=True)


def split_guard_check(wait=False):
    """Examine the flags that have arrived (wait=True: all of them, one synchronisation).  Non-finite -> SplitOperandOverflow, or with
    EDVR_SPLIT_GUARD=fallback a warning and the fp32 kernels from here on."""
    global GUARD_TRIPS
    while _GUARD_PENDING:
        host, done = _GUARD_PENDING[0]
        if wait:
            done.synchronize()
        elif not done.query():
            return
        _GUARD_PENDING.pop(0)
        v = float(host[0])
        if v != v or v == float('inf'):
            GUARD_TRIPS += 1
            msg = ('edvr_amd: non-finite values left a split-operand kernel (max |y| = %r): either the input holds inf / NaN, or a '
                   'magnitude bound was stale (a tensor rewritten through a raw pointer after its bound was taken: see '
                   'ops.void_bound).  EDVR_WINOGRAD_F4S=0 runs the fp32 kernels.' % v)
            if SPLIT_GUARD == 'fallback':
                import warnings
                warnings.warn(msg + '  Continuing on the fp32 kernels.')
                set_f4s(False, False)
            else:
                raise SplitOperandOverflow(msg)


def _ver(t):
    """The autograd version counter a bound is tied to; inference tensors (torch.inference_mode) do not have one - and cannot be
    written in place outside inference mode: None."""
    return None if t.is_inference() else t._version


def set_bound(t, bound, depth=0):
    """Remember `bound` (1-element device tensor >= max |t|) on the tensor object; valid while t is not written again.
    depth: 0 = measured (the split-operand kernel's y_amax epilogue, the reduction kernel), 1 = derived from a measured one through the
    weights' norms (linear_bound) - typically 10-50x the true maximum, which the split costs nothing (it has 2^18 of slack); a SECOND
    derivation on top would multiply the looseness (1e10 after a few layers), so it is refused and the consumer measures instead.
    Every function of this module that writes into a caller's tensor through a raw pointer replaces or voids its bound (void_bound):
    the version counter does not see those writes."""
    t._edvr_amax = (bound, _ver(t), depth)


def get_bound(t):
    b = getattr(t, '_edvr_amax', None)
    return b[0] if (b is not None and b[1] == _ver(t) and b[0].device == t.device) else None


def void_bound(*ts):
    """Forget the bounds of tensors a kernel has just rewritten through raw pointers (`out=` buffers, in-place kernels)."""
    for t in ts:
        if t is not None and hasattr(t, '_edvr_amax'):
            del t._edvr_amax


def _bound_depth(t):
    return t._edvr_amax[2]


def carry_bound(dst, *srcs, scale=1.0):
    """max |dst| <= scale * (sum of the sources' bounds) by construction of the op that made it (a gate, a convex combination, a
    permutation, a sum): hand the bound on without looking at the data.  Nothing happens when a source has none."""
    bs = [get_bound(t) for t in srcs]
    if not bs or any(b is None for b in bs):
        return dst
    b = bs[0]
    for o in bs[1:]:
        b = b + o
    set_bound(dst, b if scale == 1.0 else b * float(scale), max(_bound_depth(t) for t in srcs))
    return dst


_W_L1 = {}  # id(weight) -> (weakref, {transpose: (version, pointer, l1max)})


def weight_l1max(weight, transpose=False):
    """max over output channels of sum |w| (1-element device tensor), cached per parameter version: |conv(x, w)| <= that * max|x|.
    transpose: of the data-gradient kernel (sums over the output-channel axis of w)."""
    wid, ver = id(weight), weight._version
    ent = _W_L1.get(wid)
    if ent is None or ent[0]() is not weight:
        ent = (weakref.ref(weight, lambda _r, wid=wid: _W_L1.pop(wid, None)), {})
        _W_L1[wid] = ent
    hit = ent[1].get(bool(transpose))
    if hit is not None and hit[0] == ver and hit[1] == weight.data_ptr():
        return hit[2]
    w = weight.detach().abs()
    l1 = w.sum(dim=(0, 2, 3) if transpose else (1, 2, 3)).max().reshape(1)
    ent[1][bool(transpose)] = (ver, weight.data_ptr(), l1)
    return l1


def linear_bound(y, weight, bias, xs, extra=(), transpose=False, scale=1.0, floor=0.0):
    """Bound of y = scale * act(conv / deformable conv of xs with `weight` + bias) + extra tensors, for kernels without the y_amax
    epilogue: |y| <= |scale| (max_co sum|w| * max|x| + max|b|) + sum of the extras' bounds (1-Lipschitz activations through 0;
    `floor` = 1 for a sigmoid epilogue; deformable sampling and masks in [0, 1] are convex combinations of the input).  A few
    1-element torch ops; nothing happens when an input has no bound."""
    srcs = [t for t in xs if t is not None] + [t for t in extra if t is not None]
    bs = [get_bound(t) for t in srcs]
    if any(b is None for b in bs) or any(_bound_depth(t) > 0 for t in xs if t is not None):
        return y
    nx = sum(1 for t in xs if t is not None)
    bx = bs[0]
    for o in bs[1:nx]:
        bx = torch.maximum(bx, o)
    b = weight_l1max(weight, transpose) * bx
    if bias is not None:
        b = b + bias.detach().abs().max()
    if scale != 1.0:
        b = b * abs(float(scale))
    if floor:
        b = b.clamp_min(float(floor))
    for o in bs[nx:]:
        b = b + o
    set_bound(y, b, 1)
    return y


def input_bound(t_in, t_planes=None):
    """max |t| as a 1-element device tensor: the bound its producer left on it (set_bound), else one pass of the reduction kernel."""
    global AMAX_PASSES
    b = get_bound(t_in)
    if b is None:
        AMAX_PASSES += 1
        if AMAX_LOG is not None:  # measurement: who consumes a tensor whose producer left no bound
            import traceback
            AMAX_LOG.append((tuple(t_in.shape), [f.name for f in traceback.extract_stack()[-7:-2]]))
        b = amax(t_in if t_planes is None else t_planes)
        set_bound(t_in, b)
    return b


def amax(x, out=None):
    """max |x| of a (n, c, h, w) tensor (plane-contiguous images) as a 1-element device tensor: conv2d's `x_amax`.  `out`: an
    existing bound to fold this tensor into (max of both)."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    if out is None:
        out = _arena(x.device).slot(x.device)  # (zeroed; examined by the overflow guard: the kernel keeps non-finite values sticky)
    _run('amax', lambda: _lib.check(_lib.lib().edvr_amax_f32(_ptr(x), _ptr(out), n, c * h * w, _img_stride(x), _stream()), 'edvr_amax_f32'),
         0, _nb(x))
    return out


def conv2d(x1, wpk, bias, co, ks, *, x2=None, x2_map=None, stride=1, act=ACT_NONE, act_from=0, res1=None, res2=None,
           out_mode=OUT_NCHW, out=None, algo=None, gate=None, gate_slope=0.0, y_scale=1.0, wpk_f4=None, abs_sum_channels=0,
           wpk_f4s=None, x_amax=None, want_y_amax=True, pre=None, pre_map=None, wpk_ds=None):
    """y = y_scale * act(conv(cat(x1, x2)) + bias [+ pre]) + res1 + res2 on the fp32 MFMA kernel.
    pre (n_pre, co, h, w), pre_map = (div, mul, add) as x2_map: a pre-activation addend, image i of x1 takes image (i // div) * mul + add
    of it (edvr_conv2d_desc.pre: the F(4x4) Winograd kernels only, no gate / residuals / PixelShuffle - the C side rejects the rest).
    algo: CONV_AUTO (default; module-level CONV_ALGO overrides it, used by tests), CONV_DIRECT, CONV_WINOGRAD or CONV_WINOGRAD_F4.
    wpk_f4: pack_conv_weight(w, f4=True) - allows the F(4x4,3x3) Winograd kernel (inference; ~1e-6 relative rounding error).
    wpk_ds: pack_conv_weight(w, ds=True) - allows the split-operand direct kernel (csrc/conv2d_s.hip) where the launch would run on the
    fp32 direct kernel otherwise; like wpk_f4s it needs a bound of the inputs (x_amax, or the one travelling with them) and leaves one on y.

    x2_map = (div, mul, add): image i of x2 is (i // div) * mul + add (broadcast of a reference frame).
    gate (n, co, ho, wo): y *= gate > 0 ? 1 : gate_slope - the backward of a ReLU / LeakyReLU fused into the data-gradient conv
    (3x3 kernels; in the Winograd kernel's epilogue where that kernel applies, else in the direct kernel's).
    y_scale: ResidualBlockNoBN's res_scale (arch_util.py:95), 3x3 kernels only.
    abs_sum_channels > 0: returns (y, stats) with stats (2, n) = abs_stats_per_image(y[:, :abs_sum_channels]) (sums of |y| and of the
    horizontal neighbour differences) - the sums in the conv's own epilogue where the launch runs on the F(4x4) kernel
    (edvr_conv2d_desc.abs_sum), the differences estimated from the first image; by the separate reduction kernel otherwise.
    """
    require_gpu(x1, x2, wpk, bias, res1, res2)
    L = _lib.lib()
    x1_in, x2_in, y_bound = x1, x2, None
    x1 = _as_planes(x1)
    n, c1, h, w = x1.shape
    d = _lib.ConvDesc()
    d.x1, d.c1, d.x1_img_stride = _ptr(x1), c1, _img_stride(x1)
    if x2 is not None:
        x2 = _as_planes(x2)
        d.x2, d.c2, d.x2_img_stride = _ptr(x2), x2.shape[1], _img_stride(x2)
        assert x2.shape[2:] == x1.shape[2:]
        if x2_map is not None:
            d.x2_div, d.x2_mul, d.x2_add = x2_map
        else:
            assert x2.shape[0] == n
    d.n, d.h, d.w = n, h, w
    d.wpk, d.bias = _ptr(wpk), _ptr(bias)
    d.co, d.ks, d.stride = co, ks, stride
    d.act, d.act_from = act, act_from
    pad = ks // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    shape = (n, co // 4, 2 * ho, 2 * wo) if out_mode == OUT_PIXEL_SHUFFLE2 else (n, co, ho, wo)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x1.device)
    else:
        require_gpu(out)
        assert _plane_contig(out) and tuple(out.shape) == shape, f'out {tuple(out.shape)} / strides {out.stride()}: expected dense images of shape {shape}'
    for name, r in (('res1', res1), ('res2', res2)):
        if r is not None:
            r = _as_planes(r)
            assert tuple(r.shape) == (n, co, ho, wo), f'{name} shape {tuple(r.shape)}'
            setattr(d, name, _ptr(r))
            setattr(d, name + '_img_stride', _img_stride(r))
            if name == 'res1':
                res1 = r
            else:
                res2 = r
    if gate is not None:
        gate = _as_planes(gate)
        assert tuple(gate.shape) == (n, co, ho, wo), f'gate shape {tuple(gate.shape)}'
        d.gate, d.gate_img_stride, d.gate_slope = _ptr(gate), _img_stride(gate), float(gate_slope)
    if pre is not None:
        require_gpu(pre)
        pre = _as_planes(pre)
        if tuple(pre.shape[1:]) != (co, ho, wo):
            raise RuntimeError(f'pre shape {tuple(pre.shape)}: expected (n_pre, {co}, {ho}, {wo})')
        d.pre, d.pre_img_stride, d.pre_n = _ptr(pre), _img_stride(pre), pre.shape[0]
        if pre_map is not None:
            d.pre_div, d.pre_mul, d.pre_add = pre_map
    d.y, d.y_img_stride, d.out_mode = _ptr(out), _img_stride(out), out_mode
    d.y_scale = float(y_scale)
    if wpk_f4 is not None:
        require_gpu(wpk_f4)
        d.wpk_f4 = _ptr(wpk_f4)
    d.algo = CONV_ALGO if algo is None else algo
    split = False
    if wpk_f4s is not None or wpk_ds is not None:  # a split-operand kernel (F(4x4) / streaming 1x1; direct): its weights + a bound of the input's magnitude
        require_gpu(wpk_f4s, wpk_ds, dtypes=(torch.int32,))
        d.wpk_f4s, d.wpk_ds = _ptr(wpk_f4s), _ptr(wpk_ds)
        d.x_amax = _ptr(wpk_f4s if wpk_f4s is not None else wpk_ds)  # (any non-null pointer: only asks whether the launch would run on that kernel)
        split = bool(L.edvr_conv2d_y_amax_supported(ctypes.byref(d)))
        if split:
            if x_amax is None:
                x_amax = input_bound(x1_in, x1)
                if x2 is not None:
                    x_amax = torch.maximum(x_amax, input_bound(x2_in, x2))
            require_gpu(x_amax)
            if BOUND_CHECK:  # debugging / tests: every bound that reaches the kernel is compared with the data (synchronises)
                true = amax(x1).item() if x2 is None else max(amax(x1).item(), amax(x2).item())
                if not (x_amax.item() >= true):
                    raise AssertionError(f'magnitude bound {x_amax.item():.6g} < max |x| = {true:.6g} for a conv input of shape {tuple(x1.shape)}')
                direct = L.edvr_conv2d_kernel(ctypes.byref(d)) == _lib.CONV_KERNEL_DIRECT_SPLIT
                (BOUND_CHECK_LOG_DIRECT if direct else BOUND_CHECK_LOG).append((tuple(x1.shape), x_amax.item() / max(true, 1e-30)))
            d.x_amax = _ptr(x_amax)
            if want_y_amax:
                y_bound = _arena(x1.device).slot(x1.device)
                d.y_amax = _ptr(y_bound)
        else:
            d.wpk_f4s, d.wpk_ds, d.x_amax = None, None, None
    sums = None
    if abs_sum_channels > 0 and L.edvr_conv2d_abs_sum_supported(ctypes.byref(d)):
        sums = torch.zeros(2, n, dtype=torch.float32, device=x1.device)
        d.abs_sum, d.abs_sum_channels = _ptr(sums), int(abs_sum_channels)
    name, flops, nbytes, executed = 'conv2d', 0.0, 0.0, None
    if LAUNCH_HOOK is not None:  # measurement only (bench.py): brackets the launch with events on this stream
        buf = ctypes.create_string_buffer(96)
        L.edvr_conv2d_kernel_name(ctypes.byref(d), buf, 96)
        name = buf.value.decode()
        ex = ctypes.c_double(0.0)
        if L.edvr_conv2d_executed_flops(ctypes.byref(d), ctypes.byref(ex)) == 0:
            executed = ex.value
        flops = 2.0 * n * ho * wo * co * (c1 + d.c2) * ks * ks
        # algorithmic HBM bytes: every input / residual / gate / pre / output element once, plus the weights
        nbytes = 4.0 * (n * (c1 + d.c2) * h * w + n * co * ho * wo * (1 + (res1 is not None) + (res2 is not None) + (gate is not None) + (pre is not None))
                        + co * (c1 + d.c2) * ks * ks)
    _run(name, lambda: _lib.check(L.edvr_conv2d_f32(ctypes.byref(d), _stream()), 'edvr_conv2d_f32'), flops, nbytes, executed)
    if y_bound is not None:
        set_bound(out, y_bound)
    else:
        void_bound(out)  # a caller-provided buffer rewritten by a kernel without the epilogue: its old bound is void
    if abs_sum_channels > 0:
        if sums is None:
            return out, abs_stats_per_image(out[:, :abs_sum_channels])
        # the epilogue took the sums of |y|; the roughness statistic (row 1) is an ESTIMATE from up to four images spread over the batch
        # (one pass over ~4 x 30 MB on the L1 layer), each scaled to stand for its neighbours - one more accumulator in the F(4x4)
        # kernels' staging waves spills (128 registers) and slows every layer of the network by 4 %
        step = max(1, n // 4)
        sel = out[::step, :abs_sum_channels]
        r = abs_stats_per_image(sel)
        sums[1, ::step] = r[1] * (float(n) / sel.shape[0])
        return out, sums
    return out


def conv_pre_supported(n, c, h, w, co, f4s, algo=None):
    """Would conv2d(..., pre=...) of a 3x3 / stride-1 conv on (n, c, h, w) -> co channels run on a kernel whose epilogue takes the
    pre-activation addend?  f4s: the call would carry the split-operand weights (and a bound), else the fp32 F(4x4) ones.  (C-side rules:
    sizes, algorithm request, environment switches.)"""
    d = _lib.ConvDesc()
    d.c1, d.n, d.h, d.w, d.co, d.ks, d.stride = c, n, h, w, co, 3, 1
    d.algo = CONV_ALGO if algo is None else algo
    any_ptr = ctypes.addressof(d) & ~15  # (any non-null, 16-byte aligned value: only the eligibility rules are evaluated)
    if f4s:
        d.wpk_f4s = d.x_amax = any_ptr
    else:
        d.wpk_f4 = any_ptr
    return bool(_lib.lib().edvr_conv2d_pre_supported(ctypes.byref(d)))


def conv_gate_supported(n, c, h, w, co, algo=None):
    """Would conv2d(..., gate=...) of a 3x3 / stride-1 conv on (n, c, h, w) -> co channels run in a Winograd kernel's fused
    epilogue?  (C-side rules: sizes, algorithm request, EDVR_CONV_WINOGRAD=0 switch.  The direct kernel accepts a gate as well -
    also together with residuals - but the residual block only records the fused form where it is the fast one.)"""
    d = _lib.ConvDesc()
    d.c1, d.n, d.h, d.w, d.co, d.ks, d.stride = c, n, h, w, co, 3, 1
    d.algo = CONV_ALGO if algo is None else algo
    return bool(_lib.lib().edvr_conv2d_gate_supported(ctypes.byref(d)))


# ------------------------------------------------------------------------------------------------ DCNv1
def _ones_mask(offset):
    return torch.ones(offset.shape[0], offset.shape[1] // 2, offset.shape[2], offset.shape[3], dtype=offset.dtype, device=offset.device)


def dcnv1_forward(x, offset, weight, stride, pad, dil, groups, dg, halo_hint=0, out=None):
    """DeformConv forward (no mask, no bias): edvr_dcnv1_fwd_f32; float64 / float16: DCNv2 with an all-ones mask on edvr_dcnv2_fwd_any.
    out: optional preallocated contiguous output written in place."""
    if require_gpu(x, offset, weight, dtypes=tuple(DCN_DTYPES)) != torch.float32:
        return dcnv2_forward(x, offset, _ones_mask(offset), weight, None, stride, pad, dil, groups, dg, out=out)
    L = _lib.lib()
    offset = _as_planes(offset)
    dims = _dcn_dims(x, weight, stride, pad, dil, groups, dg)
    B, C, H, W, Co, kh, kw = dims[:7]
    ho, wo = offset.shape[2], offset.shape[3]
    if out is not None:
        if tuple(out.shape) != (B, Co, ho, wo) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
            raise RuntimeError(f'out must be a contiguous float32 tensor of shape {(B, Co, ho, wo)} on {x.device}')
        y = out
    else:
        y = torch.empty(B, Co, ho, wo, dtype=torch.float32, device=x.device)
    nbytes = L.edvr_dcnv1_fwd_ws_bytes(*dims)
    ws = workspace(nbytes, x.device)
    _run('dcnv1_fwd', lambda: _lib.check(L.edvr_dcnv1_fwd_f32(_ptr(x), _ptr(offset), _ptr(weight), _ptr(y), *dims, _bstride(offset), halo_hint, _ptr(ws), nbytes,
                                    _stream()),
                                       'edvr_dcnv1_fwd_f32'), 2.0 * B * Co * ho * wo * weight.shape[1] * kh * kw, _nb(x, offset, weight, y))
    void_bound(y)  # (a caller's `out` buffer: whatever bound it carried described its old contents)
    return y


def dcnv1_backward(x, offset, weight, dy, stride, pad, dil, groups, dg, scatter_hint=0):
    """Returns (dx, doffset, dweight) of DeformConv: edvr_dcnv1_bwd_f32 (float64 / float16: through edvr_dcnv2_bwd_any)."""
    if require_gpu(x, offset, weight, dy, dtypes=tuple(DCN_DTYPES)) != torch.float32:
        dx, doff, _, dw, _ = dcnv2_backward(x, offset, _ones_mask(offset), weight, dy, False, stride, pad, dil, groups, dg)
        return dx, doff, dw
    L = _lib.lib()
    offset = _as_planes(offset)
    dy = dy.contiguous()
    dims = _dcn_dims(x, weight, stride, pad, dil, groups, dg)
    dx = torch.empty_like(x)
    doff = torch.empty(offset.shape, dtype=torch.float32, device=x.device)
    dw = torch.empty_like(weight)
    nbytes = L.edvr_dcnv1_bwd_ws_bytes(*dims)
    ws = workspace(nbytes, x.device)
    _run('dcnv1_bwd', lambda: _lib.check(L.edvr_dcnv1_bwd_f32(_ptr(x), _ptr(offset), _ptr(weight), _ptr(dy), _ptr(dx), _ptr(doff), _ptr(dw), *dims,
                                    _bstride(offset), _bstride(doff), int(scatter_hint), _ptr(ws), nbytes, _stream()),
                                       'edvr_dcnv1_bwd_f32'), 4.0 * dy.numel() * weight[0].numel(),  # two GEMMs (dcol, dW)
                                       _nb(x, offset, weight, dy, dx, doff, dw))
    return dx, doff, dw


# ------------------------------------------------------------------------------------------------ DCNv2
def _hw(v):
    """int or (h, w) pair -> (h, w)"""
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _enc_hw(v):
    """EDVR_HW of include/edvr_amd.h: one int for an (h, w) pair; a square pair stays the plain value."""
    h, w = _hw(v)
    return h if h == w else (h | ((w + 1) << 16))


def _dcn_dims(x, weight, stride, pad, dil, groups, dg):
    B, C, H, W = x.shape
    Co, cig, kh, kw = weight.shape
    return [B, C, H, W, Co, kh, kw, _enc_hw(stride), _enc_hw(pad), _enc_hw(dil), groups, dg]


def _bstride(t):
    """offset/mask may be channel slices of one conv_offset output: pass their image stride."""
    return t.stride(0) if t.shape[0] > 1 else 0


def dcnv2_forward(x, offset, mask, weight, bias, stride, pad, dil, groups, dg, act=ACT_NONE, halo_hint=0, out=None, xm_bound=None, w_param=None):
    """out: optional preallocated (B, Co, Ho, Wo) contiguous tensor the kernels write in place (the reference's `output` argument,
    deform_conv_cuda.cpp:530-568).
    halo_hint: which kernel class runs (performance only).  The classes compute the same operator in different summation orders:
    their results agree to fp32 rounding (<= 2e-5 of the output scale, tests/test_gpu_dcn.py), NOT bit for bit.
    xm_bound: 1-element device tensor >= max |x| * max(1, max |mask|) (for sigmoid masks: a bound of |x|, `input_bound(x)`): allows the
    split-operand form of the tap-window kernel (csrc/dcn_tapwin_s.hip) where that kernel applies; None = the fp32 kernels.
    w_param (no-grad callers): the Parameter `weight` is the detached form of - where the split-operand kernel runs, its weight layout is
    then packed once per parameter version (pack_dcn_split_weight) instead of at every call; None packs per call.  Same bytes, same y."""
    dt = require_gpu(x, offset, mask, weight, bias, dtypes=tuple(DCN_DTYPES))
    L = _lib.lib()
    if not x.is_contiguous() or not weight.is_contiguous():
        raise RuntimeError('input tensor has to be contiguous')  # deform_conv_cuda.cpp:497-498
    offset, mask = _as_planes(offset), _as_planes(mask)
    dims = _dcn_dims(x, weight, stride, pad, dil, groups, dg)
    B, C, H, W, Co, kh, kw = dims[:7]
    if C != weight.shape[1] * groups:
        raise RuntimeError(f'Input shape and kernel channels wont match: ({C} vs {weight.shape[1] * groups}).')
    (sh, sw), (ph, pw), (dh, dw) = _hw(stride), _hw(pad), _hw(dil)
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f'convolution input is too small (output would be {Ho}x{Wo})')
    if tuple(offset.shape[1:]) != (dg * 2 * kh * kw, Ho, Wo):  # (RuntimeError like the reference's TORCH_CHECKs, deform_conv_cuda.cpp:64-66)
        raise RuntimeError(f'invalid spatial size / channels of offset: got {tuple(offset.shape)}, expected (B, {dg * 2 * kh * kw}, {Ho}, {Wo})')
    if tuple(mask.shape[1:]) != (dg * kh * kw, Ho, Wo):
        raise RuntimeError(f'invalid spatial size / channels of mask: got {tuple(mask.shape)}, expected (B, {dg * kh * kw}, {Ho}, {Wo})')
    if out is not None:
        if tuple(out.shape) != (B, Co, Ho, Wo) or out.dtype != dt or not out.is_contiguous() or out.device != x.device:
            raise RuntimeError(f'out must be a contiguous {dt} tensor of shape {(B, Co, Ho, Wo)} on {x.device}')
        y = out
    else:
        y = torch.empty(B, Co, Ho, Wo, dtype=dt, device=x.device)
    if dt != torch.float32:  # float64 / float16: the reference's other dispatch legs (csrc/dcn_any.hip); no fused activation there
        if act != ACT_NONE:
            raise NotImplementedError('the fused activation of dcnv2_forward exists in fp32 only')
        nbytes = L.edvr_dcnv2_any_ws_bytes(DCN_DTYPES[dt], *dims)
        ws = workspace(nbytes, x.device)
        _lib.check(L.edvr_dcnv2_fwd_any(DCN_DTYPES[dt], _ptr(x), _ptr(offset), _ptr(mask), _ptr(weight), _ptr(bias), _ptr(y), *dims,
                                        _bstride(offset), _bstride(mask), _ptr(ws), nbytes, _stream()), 'edvr_dcnv2_fwd_any')
        void_bound(y)
        return y
    nbytes = L.edvr_dcnv2_fwd_ws_bytes(*dims)
    ws = workspace(nbytes, x.device)
    name = 'dcnv2_fwd'
    split = xm_bound is not None and bool(L.edvr_dcnv2_fwd_split_applies(_ptr(x), *dims, int(halo_hint)))
    if LAUNCH_HOOK is not None:  # measurement only (bench.py): which kernel class this call runs on
        buf = ctypes.create_string_buffer(64)
        if L.edvr_dcnv2_fwd_kernel_name(_ptr(x), *dims, int(halo_hint), buf, 64) == 0:
            name = f'dcnv2_fwd[{"dcn_tapwin_split_fwd_kernel" if split else buf.value.decode()}]'
    common = (_ptr(x), _ptr(offset), _ptr(mask), _ptr(weight), _ptr(bias), _ptr(y), *dims, _bstride(offset), _bstride(mask), act, halo_hint, _ptr(ws), nbytes)
    if split and w_param is not None and w_param.data_ptr() == weight.data_ptr() and w_param.is_contiguous():
        require_gpu(xm_bound)
        wq = pack_dcn_split_weight(w_param)  # (a launch of its own under LAUNCH_HOOK, and only when the parameter has changed)
        launch = lambda: _lib.check(L.edvr_dcnv2_fwd_split_packed_f32(_ptr(x), _ptr(offset), _ptr(mask), _ptr(wq), _ptr(bias), _ptr(y), *dims, _bstride(offset),
                                                                      _bstride(mask), act, halo_hint, _ptr(xm_bound), _stream()),
                                    'edvr_dcnv2_fwd_split_packed_f32')
    elif split:
        require_gpu(xm_bound)
        launch = lambda: _lib.check(L.edvr_dcnv2_fwd_split_f32(*common, _ptr(xm_bound), _stream()), 'edvr_dcnv2_fwd_split_f32')
    else:
        launch = lambda: _lib.check(L.edvr_dcnv2_fwd_f32(*common, _stream()), 'edvr_dcnv2_fwd_f32')
    _run(name, launch, 2.0 * B * Co * Ho * Wo * weight.shape[1] * kh * kw, _nb(x, offset, mask, weight, y))
    void_bound(y)  # (a caller's `out` buffer: its old bound is void; the module path attaches the new one, dcn.py)
    return y


def dcnv2_backward(x, offset, mask, weight, dy, with_bias, stride, pad, dil, groups, dg, doffset=None, dmask=None,
                   scatter_hint=0, xm_bound=None, dy_bound=None):
    """Returns (dx, doffset, dmask, dweight, dbias).  `doffset` / `dmask` may be preallocated channel slices of one
    buffer (image-strided views): the kernels write them in place.
    xm_bound / dy_bound (both or neither): 1-element device tensors >= max |x| * max(1, max |mask|) and >= max |dy| - the dW product
    then runs in its split-operand form (csrc/gemm_nt_s.hip)."""
    dt = require_gpu(x, offset, mask, weight, dy, dtypes=tuple(DCN_DTYPES))
    L = _lib.lib()
    offset, mask = _as_planes(offset), _as_planes(mask)
    dy = dy.contiguous()
    dims = _dcn_dims(x, weight, stride, pad, dil, groups, dg)
    dx = torch.empty_like(x)
    doff = doffset if doffset is not None else torch.empty(offset.shape, dtype=dt, device=x.device)
    dmsk = dmask if dmask is not None else torch.empty(mask.shape, dtype=dt, device=x.device)
    assert _plane_contig(doff) and _plane_contig(dmsk)
    dw = torch.empty_like(weight)
    db = torch.empty(weight.shape[0], dtype=dt, device=x.device) if with_bias else None
    if dt != torch.float32:
        nbytes = L.edvr_dcnv2_any_ws_bytes(DCN_DTYPES[dt], *dims)
        ws = workspace(nbytes, x.device)
        _lib.check(L.edvr_dcnv2_bwd_any(DCN_DTYPES[dt], _ptr(x), _ptr(offset), _ptr(mask), _ptr(weight), _ptr(dy), _ptr(dx), _ptr(doff),
                                        _ptr(dmsk), _ptr(dw), _ptr(db), *dims, _bstride(offset), _bstride(mask), _bstride(doff),
                                        _bstride(dmsk), _ptr(ws), nbytes, _stream()), 'edvr_dcnv2_bwd_any')
        void_bound(doff, dmsk)
        return dx, doff, dmsk, dw, db
    nbytes = L.edvr_dcnv2_bwd_ws_bytes(*dims)
    ws = workspace(nbytes, x.device)
    common = (_ptr(x), _ptr(offset), _ptr(mask), _ptr(weight), _ptr(dy), _ptr(dx), _ptr(doff), _ptr(dmsk), _ptr(dw), _ptr(db), *dims,
              _bstride(offset), _bstride(mask), _bstride(doff), _bstride(dmsk), int(scatter_hint), _ptr(ws), nbytes)
    if xm_bound is not None and dy_bound is not None and L.edvr_dcnv2_bwd_split_applies():
        require_gpu(xm_bound, dy_bound)
        launch = lambda: _lib.check(L.edvr_dcnv2_bwd_split_f32(*common, _ptr(xm_bound), _ptr(dy_bound), _stream()), 'edvr_dcnv2_bwd_split_f32')
    else:
        launch = lambda: _lib.check(L.edvr_dcnv2_bwd_f32(*common, _stream()), 'edvr_dcnv2_bwd_f32')
    _run('dcnv2_bwd' + _SCATTER_NAMES.get(int(scatter_hint), ''), launch, 4.0 * dy.numel() * weight[0].numel(),
         _nb(x, offset, mask, weight, dy, dx, doff, dmsk, dw))
    void_bound(doff, dmsk)
    return dx, doff, dmsk, dw, db


def dcnv2_backward_kernel_name(x, weight, stride, pad, dil, groups, dg, scatter_hint=0):
    """The kernel dcnv2_backward's dX comes from for these shapes and this hint (float32 path): the launch's own decision, asked on
    the host - only the shapes of `x` and `weight` are read, no GPU is needed.  dcn_bwd_fused_kernel | dcn_bwd_dx_strip_kernel |
    dcn_bwd_coord_tile_kernel<3> | dcn_bwd_coord_tile_kernel<6> | dcn_bwd_coord_kernel."""
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.lib().edvr_dcnv2_bwd_kernel_name(*_dcn_dims(x, weight, stride, pad, dil, groups, dg), int(scatter_hint), buf, 64),
               'edvr_dcnv2_bwd_kernel_name')
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------ glue kernels
def tsa_temporal(emb, emb_ref, aligned, want_prob=False):
    """emb/aligned (b, t, c, h, w), emb_ref (b, c, h, w) -> aligned * sigmoid(<emb_t, emb_ref>) and optionally prob."""
    require_gpu(emb, emb_ref, aligned)
    b, t, c, h, w = aligned.shape
    al_in = aligned
    emb, emb_ref, aligned = emb.contiguous(), emb_ref.contiguous(), aligned.contiguous()
    out = torch.empty_like(aligned)
    prob = torch.empty(b, t, h, w, dtype=torch.float32, device=aligned.device) if want_prob else None
    _run('tsa_temporal', lambda: _lib.check(_lib.lib().edvr_tsa_temporal_f32(_ptr(emb), _ptr(emb_ref), _ptr(aligned), _ptr(out), _ptr(prob), b, t, c, h * w,
                                                _stream()),
                                       'edvr_tsa_temporal_f32'), 0, _nb(emb, emb_ref, aligned, out, prob))
    carry_bound(out, al_in)  # aligned * sigmoid(.)
    return (out, prob) if want_prob else out


TSA_FRONT = os.environ.get('EDVR_TSA_FRONT', '1') != '0'  # TSAFusion's no-grad path: temporal attention + both 1x1 heads in one kernel


def set_tsa_front(on=None):
    """Switch the one-pass head of TSA fusion (tsa_front, csrc/tsa_front_s.hip) on / off at run time; with it off the three launches
    run (tsa_temporal + two 1x1 convs: the same bits).  None leaves the setting alone.  Returns the previous value; EDVR_TSA_FRONT
    gives the initial one."""
    global TSA_FRONT
    prev = TSA_FRONT
    if on is not None:
        TSA_FRONT = bool(on)
    return prev


def _emb_ref_planes(emb_ref):
    """emb_ref (b, c, h, w) with dense images (a frame of a (b, t, c, h, w) tensor is one): no copy."""
    return emb_ref if _plane_contig(emb_ref) else emb_ref.contiguous()


def tsa_front_applies(emb, emb_ref, aligned, w_feat, w_attn, has_bias=(True, True), needs_grad=False, x_amax=None):
    """THE eligibility rule of tsa_front (edvr_tsa_front_applies, C side): no gradients, both convs 1x1 with bias and one co, a shape
    the kernel takes, and two convs that would each run on conv1x1_split_kernel - which needs a magnitude bound of `aligned` (x_amax or
    the one travelling with the tensor) and the split kernels switched on."""
    if not TSA_FRONT or not F4S_INFERENCE or needs_grad or aligned.dim() != 5 or w_feat.dim() != 4 or w_attn.dim() != 4:
        return False
    b, t, c, h, w = aligned.shape
    if tuple(emb.shape) != (b, t, c, h, w) or tuple(emb_ref.shape) != (b, c, h, w) or w_feat.shape[1] != t * c or w_attn.shape[1] != t * c:
        return False
    if x_amax is None and get_bound(aligned) is None:
        return False
    any_ptr = ctypes.c_void_p(16)  # (any non-null, 16-byte aligned value: the packed buffers are torch allocations)
    return bool(_lib.lib().edvr_tsa_front_applies(0, b, t, c, h, w, w_feat.shape[0], w_attn.shape[0], w_feat.shape[2], w_attn.shape[2],
                                                  int(bool(has_bias[0])), int(bool(has_bias[1])), any_ptr, any_ptr, any_ptr))


def tsa_front(emb, emb_ref, aligned, wq_feat, bias_feat, wq_attn, bias_attn, co, act_feat=ACT_LRELU, act_attn=ACT_LRELU, x_amax=None,
              want_y_amax=True):
    """(feat, attn) = the two 1x1 convs over mod = aligned * sigmoid(<emb_j, emb_ref>) viewed as (b, t * c, h, w), each with its bias and
    activation, in ONE kernel that never stores mod (edvr_tsa_front_f32): bit for bit tsa_temporal followed by two conv2d calls on the
    split-operand 1x1 kernel.  wq_*: pack_conv_weight(w, f4s=True) of the two (co, t * c, 1, 1) weights; x_amax: a bound of |aligned|
    (default: the one on the tensor, else one reduction pass).  No-grad only.  Both outputs carry their measured bound."""
    if torch.is_grad_enabled() and any(v.requires_grad for v in (emb, emb_ref, aligned)):
        raise RuntimeError('tsa_front has no backward: call it under torch.no_grad()')
    require_gpu(emb, emb_ref, aligned, bias_feat, bias_attn)
    require_gpu(wq_feat, wq_attn, dtypes=(torch.int32,))
    b, t, c, h, w = aligned.shape
    if tuple(emb.shape) != (b, t, c, h, w) or tuple(emb_ref.shape) != (b, c, h, w):
        raise ValueError(f'tsa_front: emb {tuple(emb.shape)} / emb_ref {tuple(emb_ref.shape)} do not match aligned {tuple(aligned.shape)}')
    L = _lib.lib()
    if not L.edvr_tsa_front_supported(b, t, c, h, w, co):
        raise NotImplementedError(f'tsa_front: the kernel takes t <= 16, c % 8 == 0, co <= 128; got t {t}, c {c}, co {co}')
    n_el = L.edvr_conv2d_packed_weight_1x1s_elems(co, t * c)
    if wq_feat.numel() != n_el or wq_attn.numel() != n_el or bias_feat.numel() != co or bias_attn.numel() != co:
        raise ValueError(f'tsa_front: packed weights of {n_el} dwords and biases of {co} elements expected')
    al_in = aligned
    emb, aligned, emb_ref = emb.contiguous(), aligned.contiguous(), _emb_ref_planes(emb_ref)
    if x_amax is None:
        x_amax = input_bound(al_in, aligned.view(b * t, c, h, w))
    require_gpu(x_amax)
    if BOUND_CHECK:  # debugging / tests, as in conv2d: the bound that reaches the kernel against the data (max |mod| <= max |aligned|; synchronises)
        true = amax(aligned.view(b * t, c, h, w)).item()
        if not (x_amax.item() >= true):
            raise AssertionError(f'magnitude bound {x_amax.item():.6g} < max |aligned| = {true:.6g} for the TSA head on {tuple(aligned.shape)}')
        BOUND_CHECK_LOG.extend([((b, t * c, h, w), x_amax.item() / max(true, 1e-30))] * 2)  # (one record per conv, as the three launches leave)
    feat = torch.empty(b, co, h, w, dtype=torch.float32, device=aligned.device)
    attn = torch.empty(b, co, h, w, dtype=torch.float32, device=aligned.device)
    yb = (_arena(aligned.device).slot(aligned.device), _arena(aligned.device).slot(aligned.device)) if want_y_amax else (None, None)
    ci = t * c
    _run('tsa_front_split_kernel',
         lambda: _lib.check(L.edvr_tsa_front_f32(_ptr(emb), _ptr(emb_ref), _img_stride(emb_ref), _ptr(aligned), _ptr(x_amax),
                                                 _ptr(wq_feat), _ptr(bias_feat), int(act_feat), _ptr(feat), _ptr(yb[0]),
                                                 _ptr(wq_attn), _ptr(bias_attn), int(act_attn), _ptr(attn), _ptr(yb[1]),
                                                 b, t, c, h, w, co, _stream()), 'edvr_tsa_front_f32'),
         2.0 * b * h * w * (t * c + 2 * co * ci), _nb(emb, emb_ref, aligned, feat, attn) + 8.0 * co * ci,
         16.0 * b * (-(-h * w // 128) * 128) * (-(-ci // 32) * 32) * (128 if co > 64 else 64))
    if want_y_amax:
        set_bound(feat, yb[0])
        set_bound(attn, yb[1])
    return feat, attn


def tsa_temporal_pair(emb, emb_ref, aligned, out=None, out_rev=None):
    """tsa_temporal with a second output from the same pass (edvr_tsa_temporal_pair_f32): returns (out, out_rev), out bit for bit
    tsa_temporal's and out_rev[:, j] = out[:, t - 1 - j] - the modulated features of every clip in reversed frame order (the
    temporal-reversal self-ensemble of edvr_amd/video.py).  No-grad only.  out / out_rev: contiguous (b, t, c, h, w) buffers to write
    (allocated when None); out, out_rev and aligned must not share memory.  Both outputs take `aligned`'s magnitude bound."""
    if torch.is_grad_enabled():
        raise RuntimeError('tsa_temporal_pair has no backward: call it under torch.no_grad()')
    require_gpu(emb, emb_ref, aligned, out, out_rev)
    b, t, c, h, w = aligned.shape
    al_in = aligned
    emb, emb_ref, aligned = emb.contiguous(), emb_ref.contiguous(), aligned.contiguous()
    if tuple(emb.shape) != (b, t, c, h, w) or tuple(emb_ref.shape) != (b, c, h, w):
        raise ValueError(f'tsa_temporal_pair: emb {tuple(emb.shape)} / emb_ref {tuple(emb_ref.shape)} do not match aligned {tuple(aligned.shape)}')
    out = torch.empty_like(aligned) if out is None else out
    out_rev = torch.empty_like(aligned) if out_rev is None else out_rev
    nbytes = 4 * aligned.numel()
    for o in (out, out_rev):
        if tuple(o.shape) != (b, t, c, h, w) or not o.is_contiguous():
            raise ValueError(f'tsa_temporal_pair: outputs are contiguous {(b, t, c, h, w)} tensors, got {tuple(o.shape)} / strides {o.stride()}')
    spans = [(v.data_ptr(), v.data_ptr() + nbytes) for v in (out, out_rev, aligned)]
    if any(a0 < b1 and b0 < a1 for i, (a0, a1) in enumerate(spans) for b0, b1 in spans[i + 1:]):
        raise ValueError('tsa_temporal_pair: out, out_rev and aligned must be distinct buffers (every frame is read and written at two places)')
    _run('tsa_temporal_pair', lambda: _lib.check(_lib.lib().edvr_tsa_temporal_pair_f32(_ptr(emb), _ptr(emb_ref), _ptr(aligned), _ptr(out), _ptr(out_rev), b, t, c,
                                                     h * w, _stream()),
                                            'edvr_tsa_temporal_pair_f32'), 0, _nb(emb, emb_ref, aligned, out, out_rev))
    void_bound(out, out_rev)
    carry_bound(out, al_in)  # aligned * sigmoid(.), and a permutation of it
    carry_bound(out_rev, al_in)
    return out, out_rev


def pool_maxavg(x):
    require_gpu(x)
    x_in, x = x, x.contiguous()
    n, c, h, w = x.shape
    y = torch.empty(n, 2 * c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, dtype=torch.float32, device=x.device)
    _run('pool_maxavg_3x3s2', lambda: _lib.check(_lib.lib().edvr_pool_maxavg_3x3s2_f32(_ptr(x), _ptr(y), n, c, h, w, _stream()),
                                       'edvr_pool_maxavg_3x3s2_f32'), 0, _nb(x, y))
    return carry_bound(y, x_in)


def upsample2x(x, scale=1.0):
    require_gpu(x)
    x_in, x = x, x.contiguous()
    n, c, h, w = x.shape
    y = torch.empty(n, c, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
    _run('upsample2x', lambda: _lib.check(_lib.lib().edvr_upsample2x_f32(_ptr(x), _ptr(y), n * c, h, w, float(scale), _stream()),
                                       'edvr_upsample2x_f32'), 0, _nb(x, y))
    return carry_bound(y, x_in, scale=abs(scale))  # bilinear weights sum to one


def tsa_combine(feat, attn, attn_add):
    require_gpu(feat, attn, attn_add)
    f_in, a_in = feat, attn_add
    feat, attn, attn_add = feat.contiguous(), attn.contiguous(), attn_add.contiguous()
    y = torch.empty_like(feat)
    _run('tsa_combine', lambda: _lib.check(_lib.lib().edvr_tsa_combine_f32(_ptr(feat), _ptr(attn), _ptr(attn_add), _ptr(y), feat.numel(), _stream()),
                                       'edvr_tsa_combine_f32'), 0, _nb(feat, attn, attn_add, y))
    bf, ba = get_bound(f_in), get_bound(a_in)
    if bf is not None and ba is not None:
        set_bound(y, bf * 2.0 + ba, max(_bound_depth(f_in), _bound_depth(a_in)))  # feat * sigmoid(attn) * 2 + attn_add
    return y


def upsample4x_add_(y, base):
    """y += bilinear_x4(base), in place."""
    require_gpu(y, base)
    base = base.contiguous()
    n, c, h, w = base.shape
    assert y.is_contiguous() and tuple(y.shape) == (n, c, 4 * h, 4 * w)
    by, bb = get_bound(y), get_bound(base)  # before the write: |y + up(base)| <= bound(y) + bound(base) (bilinear weights sum to one)
    depth = max(_bound_depth(y), _bound_depth(base)) if (by is not None and bb is not None) else 0
    _run('upsample4x_add', lambda: _lib.check(_lib.lib().edvr_upsample4x_add_f32(_ptr(base), _ptr(y), n * c, h, w, _stream()),
                                       'edvr_upsample4x_add_f32'), 0, _nb(base, y, y))
    void_bound(y)  # the raw-pointer write does not move y's version counter: the old bound must not survive it
    if by is not None and bb is not None:
        set_bound(y, by + bb, depth)
    return y


def add(a, b):
    require_gpu(a, b)
    a_in, b_in = a, b
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape
    y = torch.empty_like(a)
    _run('add', lambda: _lib.check(_lib.lib().edvr_add_f32(_ptr(a), _ptr(b), _ptr(y), a.numel(), _stream()),
                                       'edvr_add_f32'), 0, _nb(a, b, y))
    return carry_bound(y, a_in, b_in)


def act_backward(dy, y, act, act_from=0, res1=None, res2=None):
    """dz = dy * act'(.) computed from the activation output; y = act(z) + res1 + res2 as the fused conv wrote it.  (relu with both
    residuals: an output of 0 returns from y - res1 - res2 as rounding noise of either sign, so the kernel opens the gate only above
    2^-23 (|y| + |y - res1|); a positive output below that, ~1e-6 for residuals of order 1, gets the gradient 0 as well.)"""
    require_gpu(dy, y, res1, res2)
    dy_in = dy
    dy, y = dy.contiguous(), y.contiguous()
    res1 = res1.contiguous() if res1 is not None else None
    res2 = res2.contiguous() if res2 is not None else None
    n, c = y.shape[:2]
    dz = torch.empty_like(dy)
    _run('act_bwd', lambda: _lib.check(_lib.lib().edvr_act_bwd_f32(_ptr(dy), _ptr(y), _ptr(res1), _ptr(res2), _ptr(dz), n, c, y[0, 0].numel(), act, act_from,
                                           _stream()),
                                       'edvr_act_bwd_f32'), 0, _nb(dy, y, res1, res2, dz))
    return carry_bound(dz, dy_in)  # |act'| <= 1 for every epilogue activation


def set_wgrad_algo(algo):
    """Process-wide algorithm request of conv2d_wgrad (CONV_AUTO | CONV_DIRECT | CONV_WINOGRAD); returns the previous one."""
    prev = _lib.lib().edvr_conv2d_wgrad_algo(int(algo))
    if prev < 0:
        _lib.check(prev, 'edvr_conv2d_wgrad_algo')
    return prev


def conv2d_wgrad(x1, x2, x2_map, dz, co, ks, stride, want_db=False, into=None):
    """dW (co, c1+c2, ks, ks) of the fused conv: Winograd-domain GEMM over tiles (3x3 / stride 1) or fp32 MFMA implicit GEMM
    over the pixel axis.  want_db: also return db = sum of dz over (n, h, w) -> (dw, db); the Winograd-domain kernel produces it
    in the same two launches.  into: a contiguous fp32 (co, c1+c2, ks, ks) tensor the gradient is ADDED to (into += dW, the
    `accumulate` flag of the reduction pass) and that is returned in dW's place; db is never accumulated."""
    require_gpu(x1, x2, dz)
    L = _lib.lib()
    x1_in, x2_in, dz_in = x1, x2, dz
    x1, dz = _as_planes(x1), _as_planes(dz)
    n, c1, h, w = x1.shape
    c2 = 0
    if x2 is not None:
        x2 = _as_planes(x2)
        c2 = x2.shape[1]
    div, mul, add = x2_map if x2_map is not None else (0, 0, 0)
    if into is None:
        dw = torch.empty(co, c1 + c2, ks, ks, dtype=torch.float32, device=x1.device)
    else:
        require_gpu(into)
        assert into.is_contiguous() and tuple(into.shape) == (co, c1 + c2, ks, ks), \
            f'into {tuple(into.shape)} / strides {into.stride()}: expected a contiguous {(co, c1 + c2, ks, ks)}'
        dw = into
    nbytes = L.edvr_conv2d_wgrad_ws_bytes(n, c1 + c2, h, w, co, ks, stride)
    ws = workspace(nbytes, x1.device)
    db = torch.empty(co, dtype=torch.float32, device=x1.device) if want_db else None
    name = 'conv2d_wgrad'
    # the split-operand form of the Winograd-domain kernel needs bounds of both operands' magnitudes (they travel with the tensors)
    split = F4S_TRAINING and bool(L.edvr_conv2d_wgrad_split_applies(n, c1, c2, h, w, co, ks, stride))
    if LAUNCH_HOOK is not None:
        buf = ctypes.create_string_buffer(96)
        L.edvr_conv2d_wgrad_kernel_name(n, c1, c2, h, w, co, ks, stride, buf, 96)
        name = buf.value.decode()
        if split and name == 'conv3x3_winograd_wgrad_kernel':
            name = 'conv3x3_wgrad_direct_split_kernel' if L.edvr_conv2d_wgrad_split_is_direct(h, w) else 'conv3x3_winograd_wgrad_split_kernel'
    pad = ks // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    common = (_ptr(x1), _ptr(x2), _ptr(dz), _ptr(dw), c1, c2, n, h, w, co, ks, stride, _img_stride(x1), _img_stride(x2) if x2 is not None else 0,
              div, mul, add, _img_stride(dz), 0 if into is None else 1, _ptr(db), _ptr(ws), nbytes)
    if split and ks == 1:  # the 1x1 GEMM is too cheap to pay for a reduction pass: split only with both bounds at hand
        bx, bz = get_bound(x1_in), get_bound(dz_in)
        split = bx is not None and bz is not None
        if split and name == 'gemm_nt_kernel':
            name = 'gemm_nt_split_kernel'
    elif split:
        bx = input_bound(x1_in, x1)
        if x2 is not None:
            bx = torch.maximum(bx, input_bound(x2_in, x2))
        bz = input_bound(dz_in, dz)
    if split:
        launch = lambda: _lib.check(L.edvr_conv2d_wgrad_split_f32(*common, _ptr(bx), _ptr(bz), _stream()), 'edvr_conv2d_wgrad_split_f32')
    else:
        launch = lambda: _lib.check(L.edvr_conv2d_wgrad_f32(*common, _stream()), 'edvr_conv2d_wgrad_f32')
    _run(name, launch, 2.0 * n * ho * wo * co * (c1 + c2) * ks * ks, _nb(x1, dz, dw) + (4.0 * n * c2 * h * w if x2 is not None else 0.0))
    void_bound(into)  # (rewritten through a raw pointer)
    return (dw, db) if want_db else dw


def channel_sum(x):
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    out = torch.empty(c, dtype=torch.float32, device=x.device)
    nbytes = 64 * c * 4
    ws = workspace(nbytes, x.device)
    _run('channel_sum', lambda: _lib.check(_lib.lib().edvr_channel_sum_f32(_ptr(x), _ptr(out), n, c, h * w, _img_stride(x), _ptr(ws), nbytes, _stream()),
                                       'edvr_channel_sum_f32'), 0, _nb(x))
    return out


def pixel_unshuffle2(x):
    require_gpu(x)
    x_in, x = x, x.contiguous()
    n, c, h2, w2 = x.shape
    y = torch.empty(n, 4 * c, h2 // 2, w2 // 2, dtype=torch.float32, device=x.device)
    _run('pixel_unshuffle2', lambda: _lib.check(_lib.lib().edvr_pixel_unshuffle2_f32(_ptr(x), _ptr(y), n, c, h2 // 2, w2 // 2, _stream()),
                                       'edvr_pixel_unshuffle2_f32'), 0, _nb(x, y))
    return carry_bound(y, x_in)


def pixel_unshuffle2_act_backward(dy, y, act):
    """unshuffle(dy * act'(y)): the gradient of PixelShuffle(2)(act(z)) w.r.t. z in one launch (y = the shuffled activation output)."""
    require_gpu(dy)
    dy_in, dy = dy, dy.contiguous()
    n, c, h2, w2 = dy.shape
    if act != ACT_NONE:
        require_gpu(y)
        y = y.contiguous()
        if tuple(y.shape) != tuple(dy.shape):
            raise RuntimeError(f'pixel_unshuffle2_act_backward: y {tuple(y.shape)} vs dy {tuple(dy.shape)}')
    dz = torch.empty(n, 4 * c, h2 // 2, w2 // 2, dtype=torch.float32, device=dy.device)
    _run('pixel_unshuffle2_act_bwd', lambda: _lib.check(_lib.lib().edvr_pixel_unshuffle2_act_bwd_f32(
        _ptr(dy), _ptr(y) if act != ACT_NONE else None, _ptr(dz), n, c, h2 // 2, w2 // 2, int(act), _stream()), 'edvr_pixel_unshuffle2_act_bwd_f32'),
        0, _nb(dy, dz) + (_nb(y) if act != ACT_NONE else 0.0))
    return carry_bound(dz, dy_in)


def zero_stuff2(dz, H, W):
    require_gpu(dz)
    dz_in, dz = dz, dz.contiguous()
    n, c, ho, wo = dz.shape
    z = torch.empty(n, c, H, W, dtype=torch.float32, device=dz.device)
    _run('zero_stuff2', lambda: _lib.check(_lib.lib().edvr_zero_stuff2_f32(_ptr(dz), _ptr(z), n * c, H, W, ho, wo, _stream()),
                                       'edvr_zero_stuff2_f32'), 0, _nb(dz, z))
    return carry_bound(z, dz_in)


def frame_reduce_add_(src, dst, t, center):
    """dst[b, center] += sum_t src[b, t] for (b*t, c, h, w) tensors."""
    require_gpu(src, dst)
    src = src.contiguous()
    assert dst.is_contiguous() and src.shape == dst.shape and src.shape[0] % t == 0
    _run('frame_reduce_add', lambda: _lib.check(_lib.lib().edvr_frame_reduce_add_f32(_ptr(src), _ptr(dst), src.shape[0] // t, t, center, src[0].numel(), _stream()),
                                       'edvr_frame_reduce_add_f32'), 0, _nb(src) + 8.0 * src.numel() / t)
    void_bound(dst)  # rewritten in place through a raw pointer: the consumer measures
    return dst


def upsample2x_backward(dy, scale=1.0):
    require_gpu(dy)
    dy_in, dy = dy, dy.contiguous()
    n, c, h2, w2 = dy.shape
    dx = torch.empty(n, c, h2 // 2, w2 // 2, dtype=torch.float32, device=dy.device)
    _run('upsample2x_bwd', lambda: _lib.check(_lib.lib().edvr_upsample2x_bwd_f32(_ptr(dy), _ptr(dx), n * c, h2 // 2, w2 // 2, float(scale), _stream()),
                                       'edvr_upsample2x_bwd_f32'), 0, _nb(dy, dx))
    return carry_bound(dx, dy_in, scale=4.0 * abs(scale))  # adjoint of the interpolation: the weights into one coarse pixel sum to 4


def pool_maxavg_backward(x, dy):
    require_gpu(x, dy)
    dy_in = dy
    x, dy = x.contiguous(), dy.contiguous()
    n, c, h, w = x.shape
    dx = torch.empty_like(x)
    _run('pool_maxavg_3x3s2_bwd', lambda: _lib.check(_lib.lib().edvr_pool_maxavg_3x3s2_bwd_f32(_ptr(x), _ptr(dy), _ptr(dx), n, c, h, w, _stream()),
                                       'edvr_pool_maxavg_3x3s2_bwd_f32'), 0, _nb(x, dy, dx))
    return carry_bound(dx, dy_in, scale=8.0)  # a pixel sits in at most 4 windows of each of the two pooled halves


def tsa_temporal_backward(emb, emb_ref, aligned, dout):
    require_gpu(emb, emb_ref, aligned, dout)
    emb, emb_ref, aligned, dout = emb.contiguous(), emb_ref.contiguous(), aligned.contiguous(), dout.contiguous()
    b, t, c, h, w = aligned.shape
    d_emb, d_ref, d_al = torch.empty_like(emb), torch.empty_like(emb_ref), torch.empty_like(aligned)
    ws = torch.empty(b * t * h * w, dtype=torch.float32, device=emb.device)  # per-(clip, frame, pixel) scalar between the two passes
    _run('tsa_temporal_bwd', lambda: _lib.check(_lib.lib().edvr_tsa_temporal_bwd_f32(_ptr(emb), _ptr(emb_ref), _ptr(aligned), _ptr(dout), _ptr(d_emb), _ptr(d_ref),
                                                    _ptr(d_al), b, t, c, h * w, _ptr(ws), _stream()),
                                       'edvr_tsa_temporal_bwd_f32'), 0, _nb(emb, emb_ref, aligned, dout, d_emb, d_ref, d_al))
    return d_emb, d_ref, d_al


def tsa_combine_backward(feat, attn, dy):
    require_gpu(feat, attn, dy)
    feat, attn, dy = feat.contiguous(), attn.contiguous(), dy.contiguous()
    dfeat, dattn = torch.empty_like(feat), torch.empty_like(attn)
    _run('tsa_combine_bwd', lambda: _lib.check(_lib.lib().edvr_tsa_combine_bwd_f32(_ptr(feat), _ptr(attn), _ptr(dy), _ptr(dfeat), _ptr(dattn), feat.numel(), _stream()),
                                       'edvr_tsa_combine_bwd_f32'), 0, _nb(feat, attn, dy, dfeat, dattn))
    return dfeat, dattn


def charbonnier(pred, target, eps=1e-12, want_grad=True, grad_scale=1.0):
    """CharbonnierLoss(reduction='sum'): returns (loss (1,) device tensor, dloss/dpred or None) from one pass."""
    require_gpu(pred, target)
    pred, target = pred.contiguous(), target.contiguous()
    assert pred.shape == target.shape
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    _run('charbonnier', lambda: _lib.check(_lib.lib().edvr_charbonnier_f32(_ptr(pred), _ptr(target), _ptr(loss), _ptr(dpred), pred.numel(), float(eps),
                                               float(grad_scale), _stream()),
                                       'edvr_charbonnier_f32'), 0, _nb(pred, target, dpred))
    return loss, dpred


def note_abs_mean(x):
    """Start computing the offset statistics (mean |x| and the roughness, `offset_stats`) of a (n, c, h, w) float32 tensor without
    waiting for them: per-image sums -> pinned memory behind an event.  `abs_mean_if_ready` / `offset_stats_if_ready` return the
    values once they have arrived (None before) - how a backward picks up the statistic of its own forward without a host
    synchronisation.  EDVR_DCN_HINT_WAIT=1 makes the pick-up wait for the copy instead (deterministic kernel choice, for
    bisecting timings or rounding-level differences; costs one host synchronisation per backward)."""
    sums = abs_stats_per_image(x)
    host = torch.empty(sums.shape, dtype=sums.dtype, pin_memory=True)
    host.copy_(sums, non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    return host, done, x.numel()


HINT_WAIT = os.environ.get('EDVR_DCN_HINT_WAIT', '0') == '1'


def offset_stats_if_ready(rec):
    """(mean |x|, roughness or None) of a `note_abs_mean` record, or None while the copy has not landed."""
    if rec is None:
        return None
    if HINT_WAIT:
        rec[1].synchronize()
    elif not rec[1].query():
        return None
    return offset_stats(rec[0], rec[2])


def abs_mean_if_ready(rec):
    st = offset_stats_if_ready(rec)
    return None if st is None else st[0]


def offset_stats(stats, count):
    """(mean |offset|, mean |horizontal neighbour difference| or None) from the (2, n) sums of `abs_stats_per_image` over `count`
    elements in all.  The difference sum covers 3 of every 4 horizontal pairs (include/edvr_amd.h, edvr_abs_stats_f32)."""
    tot = stats.double().sum(-1).tolist() if stats.dim() == 2 else [float(stats.double().sum()), -1.0]
    return tot[0] / count, (tot[1] / (0.75 * count) if tot[1] >= 0 else None)


def abs_sum_per_image(x):
    """sum |x[i]| per image of a (n, c, h, w) tensor (image-strided views allowed)."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    _run('abs_sum', lambda: _lib.check(_lib.lib().edvr_abs_sum_f32(_ptr(x), _ptr(out), n, c * h * w, _img_stride(x), _stream()),
                                       'edvr_abs_sum_f32'), 0, _nb(x))
    return out


def abs_stats_per_image(x):
    """(2, n): row 0 = sum |x[i]| per image, row 1 = sum |x[i, c, r, col] - x[i, c, r, col + 1]| over 3 of every 4 horizontal
    neighbour pairs (edvr_abs_stats_f32; -1 where the rows are not whole 16-byte groups) of a (n, c, h, w) tensor."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    out = torch.empty(2, n, dtype=torch.float32, device=x.device)
    _run('abs_sum', lambda: _lib.check(_lib.lib().edvr_abs_stats_f32(_ptr(x), _ptr(out), n, c * h * w, w, _img_stride(x), _stream()),
                                       'edvr_abs_stats_f32'), 0, _nb(x))
    return out


# ------------------------------------------------------------------------------------------------ input pipeline
AUG_HFLIP, AUG_VFLIP, AUG_ROT90 = 1, 2, 4


def frames_u8_to_f32(frames_u8, flags=None, swap_rb=False):
    """uint8 device tensor (n_clips, frames, h, w, 3) -> float32 (n_clips, frames, 3, h', w') = bytes / 255, with the per-clip
    augmentation `flags` (bytes / sequence of n_clips OR-ed AUG_* values, host side) applied: hflip, vflip, then transpose, as
    transforms.augment does; the channel order is reversed when swap_rb (edvr_frames_u8_to_f32, csrc/data.hip)."""
    if not frames_u8.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 5 or frames_u8.shape[-1] != 3:
        raise ValueError(f'expected a uint8 (n_clips, frames, h, w, 3) tensor, got {frames_u8.dtype} {tuple(frames_u8.shape)}')
    frames_u8 = frames_u8.contiguous()
    n, f, h, w, _ = frames_u8.shape
    fl = None
    if flags is not None:
        fl = bytes(flags)
        if len(fl) != n:
            raise ValueError(f'{len(fl)} augmentation flags for {n} clips')
    rot = fl is not None and any(b & AUG_ROT90 for b in fl)
    out = torch.empty((n, f, 3, w, h) if rot else (n, f, 3, h, w), dtype=torch.float32, device=frames_u8.device)
    if n:
        _lib.check(_lib.lib().edvr_frames_u8_to_f32(_ptr(frames_u8), _ptr(out), n, f, h, w, fl, int(bool(swap_rb)), _stream()),
                   'edvr_frames_u8_to_f32')
    return out


# ------------------------------------------------------------------------------------------------ whole-video path (edvr_amd/video.py)
GATHER_MAX_LEVELS = 3  # EDVR_GATHER_MAX_LEVELS


def gather_images(srcs, table, outs=None):
    """outs[l][j] = srcs[l][table[j]] for up to three tensors in ONE launch (edvr_gather_images_f32): srcs[l] (n_src, c_l, h_l, w_l)
    with dense images and any image stride (slices / ring positions of a larger bank), table a DEVICE int32 vector (stream-ordered, no
    host synchronisation), outs[l] contiguous (len(table), c_l, h_l, w_l) - allocated when None.  A gather cannot enlarge anything:
    each destination takes its source's magnitude bound (set_bound on the bank tensor)."""
    srcs = list(srcs)
    require_gpu(*srcs)
    if not 1 <= len(srcs) <= GATHER_MAX_LEVELS:
        raise ValueError(f'gather_images takes 1..{GATHER_MAX_LEVELS} tensors, got {len(srcs)}')
    if not table.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if table.dtype != torch.int32 or table.dim() != 1 or not table.is_contiguous() or table.numel() == 0:
        raise ValueError(f'table must be a non-empty contiguous int32 vector, got {table.dtype} {tuple(table.shape)}')
    n_src, n_out = srcs[0].shape[0], table.numel()
    for s in srcs:
        if s.dim() != 4 or s.shape[0] != n_src or not _plane_contig(s):
            raise ValueError(f'gather_images: sources must be (n_src, c, h, w) tensors with dense images and one n_src, got {tuple(s.shape)} / strides {s.stride()}')
    if outs is None:
        outs = [torch.empty((n_out,) + tuple(s.shape[1:]), dtype=torch.float32, device=s.device) for s in srcs]
    else:
        outs = list(outs)
        require_gpu(*outs)
        assert len(outs) == len(srcs) and all(o.is_contiguous() and tuple(o.shape) == (n_out,) + tuple(s.shape[1:]) for o, s in zip(outs, srcs))
    k = len(srcs)
    P, I = ctypes.c_void_p * k, ctypes.c_int64 * k
    per = [s.shape[1] * s.shape[2] * s.shape[3] for s in srcs]
    a_src, a_dst = P(*[s.data_ptr() for s in srcs]), P(*[o.data_ptr() for o in outs])
    a_str, a_per = I(*[_img_stride(s) for s in srcs]), I(*per)
    _run('gather_images', lambda: _lib.check(_lib.lib().edvr_gather_images_f32(a_src, a_dst, a_str, a_per, k, _ptr(table), n_out, n_src, _stream()),
                                             'edvr_gather_images_f32'), 0, 8.0 * n_out * sum(per))
    for o, s in zip(outs, srcs):
        void_bound(o)
        carry_bound(o, s)
    return outs


def upsample4x_add_u8(y, base):
    """tensor2img(y + bilinear_x4(base)) as (n, 4h, 4w, 3) uint8: the bytes of upsample4x_add_'s float result, without storing it."""
    require_gpu(y, base)
    base = base.contiguous()
    n, c, h, w = base.shape
    if c != 3:
        raise NotImplementedError(f'the uint8 output is interleaved RGB: 3 channels, got {c}')
    assert y.is_contiguous() and tuple(y.shape) == (n, c, 4 * h, 4 * w)
    out = torch.empty(n, 4 * h, 4 * w, 3, dtype=torch.uint8, device=y.device)
    _run('upsample4x_add_u8', lambda: _lib.check(_lib.lib().edvr_upsample4x_add_u8(_ptr(y), _ptr(base), _ptr(out), n, h, w, _stream()),
                                                 'edvr_upsample4x_add_u8'), 0, _nb(base, y) + out.numel())
    return out


def f32_to_u8_hwc(x):
    """tensor2img semantics on the device: (n, 3, h, w) float32 -> (n, h, w, 3) uint8 = round-half-even(clamp(x, 0, 1) * 255)."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    if c != 3:
        raise NotImplementedError(f'the uint8 output is interleaved RGB: 3 channels, got {c}')
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=x.device)
    _run('f32_to_u8_hwc', lambda: _lib.check(_lib.lib().edvr_f32_to_u8_hwc(_ptr(x), _ptr(out), n, h, w, _img_stride(x), _stream()),
                                             'edvr_f32_to_u8_hwc'), 0, _nb(x) + out.numel())
    return out


PAD_MODES = {'reflect': 0, 'replicate': 1}  # EDVR_PAD_REFLECT, EDVR_PAD_REPLICATE


def crop_pad_frames(frames, y0, x0, th, tw, pad_mode=None):
    """The (th, tw) rectangle at (y0, x0) of `frames` extended at the bottom and right - F.pad(x, (0, .., 0, ..), mode=pad_mode) and a slice
    in one launch - as a dense float32 (n, 3, th, tw) tensor.  frames: uint8 (n, H, W, 3) (converted as frames_u8_to_f32 does: byte / 255)
    or float32 (n, 3, H, W) with dense images (a slice of a longer video works).  pad_mode 'reflect' | 'replicate'; None: the rectangle
    must lie inside the frames.  A rectangle the mode cannot fill ('reflect' reaches H - 1 rows beyond the frame) is a ValueError."""
    if not frames.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if pad_mode is not None and pad_mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be None, 'reflect' or 'replicate', got {pad_mode!r}")
    u8 = frames.dtype == torch.uint8
    if u8:
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f'uint8 frames are (n, H, W, 3), got {tuple(frames.shape)}')
        frames = frames.contiguous()
        n, H, W, _ = frames.shape
    else:
        require_gpu(frames)
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f'float32 frames are (n, 3, H, W), got {tuple(frames.shape)}')
        frames = _as_planes(frames)
        n, _, H, W = frames.shape
    y0, x0, th, tw = int(y0), int(x0), int(th), int(tw)
    if n == 0 or th <= 0 or tw <= 0 or not (0 <= y0 < H and 0 <= x0 < W):
        raise ValueError(f'crop_pad_frames: a {th} x {tw} rectangle at ({y0}, {x0}) of {n} frame(s) of {H} x {W}')
    reach = (H - 1, W - 1) if pad_mode is None else (2 * (H - 1), 2 * (W - 1)) if pad_mode == 'reflect' else None
    if reach is not None and (y0 + th - 1 > reach[0] or x0 + tw - 1 > reach[1]):
        raise ValueError(f'crop_pad_frames: a {th} x {tw} rectangle at ({y0}, {x0}) reaches beyond what pad_mode={pad_mode!r} makes of a {H} x {W} frame')
    mode = PAD_MODES[pad_mode or 'replicate']
    out = torch.empty(n, 3, th, tw, dtype=torch.float32, device=frames.device)
    if u8:
        _run('crop_pad_frames', lambda: _lib.check(_lib.lib().edvr_crop_pad_frames_u8(_ptr(frames), _ptr(out), n, H, W, y0, x0, th, tw, mode, _stream()),
                                                   'edvr_crop_pad_frames_u8'), 0, 5.0 * out.numel())
    else:
        _run('crop_pad_frames', lambda: _lib.check(_lib.lib().edvr_crop_pad_frames_f32(_ptr(frames), _ptr(out), n, H, W, _img_stride(frames), y0, x0, th, tw,
                                                                                       mode, _stream()), 'edvr_crop_pad_frames_f32'), 0, 8.0 * out.numel())
    return out


def _rect_dst(out, n, hy, wy, ky, kx, u8):
    """Checks a rectangle destination: `out` a view (n, 3, kh, kw) float32 / (n, kh, kw, 3) uint8 of a full-frame tensor (unit stride
    along a row, any row / plane / image strides) -> (kh, kw, row, plane, image strides in elements)."""
    if not out.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if out.dtype != (torch.uint8 if u8 else torch.float32) or out.dim() != 4 or out.shape[0] != n or out.shape[3 if u8 else 1] != 3:
        raise ValueError(f'rectangle destination: expected {"(n, kh, kw, 3) uint8" if u8 else "(n, 3, kh, kw) float32"} with n = {n}, got {out.dtype} {tuple(out.shape)}')
    kh, kw = (out.shape[1], out.shape[2]) if u8 else (out.shape[2], out.shape[3])
    ky, kx = int(ky), int(kx)
    if kh <= 0 or kw <= 0 or ky < 0 or kx < 0 or ky + kh > hy or kx + kw > wy:
        raise ValueError(f'a {kh} x {kw} rectangle at ({ky}, {kx}) does not lie inside a {hy} x {wy} result')
    st = out.stride()
    if u8:
        ok = st[3] == 1 and st[2] == 3 and st[1] >= 3 * kw and (n == 1 or st[0] >= (kh - 1) * st[1] + 3 * kw)
        row, plane, img = st[1], 0, st[0]
    else:
        ok = st[3] == 1 and st[2] >= kw and st[1] >= (kh - 1) * st[2] + kw and (n == 1 or st[0] >= 2 * st[1] + (kh - 1) * st[2] + kw)
        row, plane, img = st[2], st[1], st[0]
    if not ok:
        raise ValueError(f'rectangle destination: a view of a full-frame {"(N, H, W, 3)" if u8 else "(N, 3, H, W)"} tensor is expected, got strides {st}')
    if n == 1:
        img = max(img, (0 if u8 else 2 * plane) + (kh - 1) * row + (3 if u8 else 1) * kw)
    return kh, kw, row, plane, img


def upsample4x_add_rect(y, base, out, ky=0, kx=0):
    """out[...] = (y + bilinear_x4(base))[:, :, ky:ky + kh, kx:kx + kw] - the values upsample4x_add_ stores there - for a view `out`
    (n, 3, kh, kw) of a full-frame float32 tensor; y is left as it is.  Returns out."""
    require_gpu(y, base)
    base = base.contiguous()
    n, c, h, w = base.shape
    if c != 3:
        raise NotImplementedError(f'the rectangle stores are for RGB images: 3 channels, got {c}')
    assert y.is_contiguous() and tuple(y.shape) == (n, c, 4 * h, 4 * w)
    kh, kw, row, plane, img = _rect_dst(out, n, 4 * h, 4 * w, ky, kx, False)
    _run('upsample4x_add_rect', lambda: _lib.check(_lib.lib().edvr_upsample4x_add_rect_f32(_ptr(y), _ptr(base), _ptr(out), n, h, w, int(ky), int(kx), kh, kw,
                                                                                           row, plane, img, _stream()), 'edvr_upsample4x_add_rect_f32'),
         0, _nb(base) + 24.0 * n * kh * kw)
    void_bound(out)
    return out


def upsample4x_add_u8_rect(y, base, out, ky=0, kx=0):
    """out[...] = upsample4x_add_u8(y, base)[:, ky:ky + kh, kx:kx + kw] for a view `out` (n, kh, kw, 3) of a full-frame uint8 tensor."""
    require_gpu(y, base)
    base = base.contiguous()
    n, c, h, w = base.shape
    if c != 3:
        raise NotImplementedError(f'the uint8 output is interleaved RGB: 3 channels, got {c}')
    assert y.is_contiguous() and tuple(y.shape) == (n, c, 4 * h, 4 * w)
    kh, kw, row, _, img = _rect_dst(out, n, 4 * h, 4 * w, ky, kx, True)
    _run('upsample4x_add_u8_rect', lambda: _lib.check(_lib.lib().edvr_upsample4x_add_rect_u8(_ptr(y), _ptr(base), _ptr(out), n, h, w, int(ky), int(kx), kh, kw,
                                                                                             row, img, _stream()), 'edvr_upsample4x_add_rect_u8'),
         0, _nb(base) + 15.0 * n * kh * kw)
    return out


def f32_to_u8_hwc_rect(x, out, ky=0, kx=0):
    """out[...] = f32_to_u8_hwc(x)[:, ky:ky + kh, kx:kx + kw] for a view `out` (n, kh, kw, 3) of a full-frame uint8 tensor."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    if c != 3:
        raise NotImplementedError(f'the uint8 output is interleaved RGB: 3 channels, got {c}')
    kh, kw, row, _, img = _rect_dst(out, n, h, w, ky, kx, True)
    _run('f32_to_u8_hwc_rect', lambda: _lib.check(_lib.lib().edvr_f32_to_u8_hwc_rect(_ptr(x), _ptr(out), n, h, w, _img_stride(x), int(ky), int(kx), kh, kw,
                                                                                     row, img, _stream()), 'edvr_f32_to_u8_hwc_rect'), 0, 15.0 * n * kh * kw)
    return out


def copy_rect(x, out, ky=0, kx=0):
    """out[...] = x[:, :, ky:ky + kh, kx:kx + kw] for a view `out` (n, 3, kh, kw) of a full-frame float32 tensor (the hr_in float tail)."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    if c != 3:
        raise NotImplementedError(f'the rectangle stores are for RGB images: 3 channels, got {c}')
    kh, kw, row, plane, img = _rect_dst(out, n, h, w, ky, kx, False)
    _run('copy_rect', lambda: _lib.check(_lib.lib().edvr_copy_rect_f32(_ptr(x), _ptr(out), n, h, w, _img_stride(x), int(ky), int(kx), kh, kw,
                                                                       row, plane, img, _stream()), 'edvr_copy_rect_f32'), 0, 24.0 * n * kh * kw)
    void_bound(out)
    return out


# ------------------------------------------------------------------------------------------------ self-ensemble (csrc/ensemble.hip)
D4_FIRST, D4_LAST = 1, 2  # EDVR_D4_FIRST, EDVR_D4_LAST
D4_MODES = {'first': D4_FIRST, 'middle': 0, 'last': D4_LAST, 'only': D4_FIRST | D4_LAST}


def _d4_elem(elem):
    k = int(elem)
    if k != elem or not 0 <= k < 8:
        raise ValueError(f'a symmetry of the square is an element id 0 ... 7 (4 t + 2 v + h), got {elem!r}')
    return k


def d4_apply(x, elem):
    """g_k of a (..., H, W) tensor, k = 4 t + 2 v + h: transpose the last two axes if t, then flip rows if v, then flip columns if h
    (plain torch, any device: the definition the kernels of csrc/ensemble.hip are tested against)."""
    k = _d4_elem(elem)
    if k & 4:
        x = x.transpose(-1, -2)
    if k & 2:
        x = x.flip(-2)
    if k & 1:
        x = x.flip(-1)
    return x


def d4_invert(y, elem):
    """g_k^-1: flip columns if h, then flip rows if v, then transpose if t."""
    k = _d4_elem(elem)
    if k & 1:
        y = y.flip(-1)
    if k & 2:
        y = y.flip(-2)
    if k & 4:
        y = y.transpose(-1, -2)
    return y


def d4_index(elem, r, q, R, C):
    """The index map the kernels implement (frame_to_tile in csrc/ensemble.hip), pure Python: pixel (r, q) of the frame's orientation
    <-> (i, j) of the transformed (R, C) image - g_k(x)[i][j] = x[r][q] and g_k^-1(y)[r][q] = y[i][j]."""
    k = _d4_elem(elem)
    a, b = (q, r) if k & 4 else (r, q)
    return (R - 1 - a if k & 2 else a), (C - 1 - b if k & 1 else b)


def crop_pad_frames_d4(frames, y0, x0, th, tw, pad_mode=None, elem=0):
    """d4_apply(crop_pad_frames(frames, y0, x0, th, tw, pad_mode), elem) in one launch, dense: (n, 3, th, tw), or (n, 3, tw, th) for a
    transposing element (edvr_crop_pad_frames_d4_*).  The padding rule is applied in the frame's own orientation, before the symmetry."""
    if not frames.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    k = _d4_elem(elem)
    if pad_mode is not None and pad_mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be None, 'reflect' or 'replicate', got {pad_mode!r}")
    u8 = frames.dtype == torch.uint8
    if u8:
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f'uint8 frames are (n, H, W, 3), got {tuple(frames.shape)}')
        frames = frames.contiguous()
        n, H, W, _ = frames.shape
    else:
        require_gpu(frames)
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f'float32 frames are (n, 3, H, W), got {tuple(frames.shape)}')
        frames = _as_planes(frames)
        n, _, H, W = frames.shape
    y0, x0, th, tw = int(y0), int(x0), int(th), int(tw)
    if n == 0 or th <= 0 or tw <= 0 or not (0 <= y0 < H and 0 <= x0 < W):
        raise ValueError(f'crop_pad_frames_d4: a {th} x {tw} rectangle at ({y0}, {x0}) of {n} frame(s) of {H} x {W}')
    reach = (H - 1, W - 1) if pad_mode is None else (2 * (H - 1), 2 * (W - 1)) if pad_mode == 'reflect' else None
    if reach is not None and (y0 + th - 1 > reach[0] or x0 + tw - 1 > reach[1]):
        raise ValueError(f'crop_pad_frames_d4: a {th} x {tw} rectangle at ({y0}, {x0}) reaches beyond what pad_mode={pad_mode!r} makes of a {H} x {W} frame')
    mode = PAD_MODES[pad_mode or 'replicate']
    out = torch.empty((n, 3, tw, th) if k & 4 else (n, 3, th, tw), dtype=torch.float32, device=frames.device)
    if u8:
        _run('crop_pad_frames_d4', lambda: _lib.check(_lib.lib().edvr_crop_pad_frames_d4_u8(_ptr(frames), _ptr(out), n, H, W, y0, x0, th, tw, mode, k,
                                                                                            _stream()), 'edvr_crop_pad_frames_d4_u8'), 0, 5.0 * out.numel())
    else:
        _run('crop_pad_frames_d4', lambda: _lib.check(_lib.lib().edvr_crop_pad_frames_d4_f32(_ptr(frames), _ptr(out), n, H, W, _img_stride(frames), y0, x0,
                                                                                             th, tw, mode, k, _stream()), 'edvr_crop_pad_frames_d4_f32'),
             0, 8.0 * out.numel())
    return out


def _d4_tail(elem, mode, scale, hy, wy):
    """-> (element id, mode bits, scale, the result's size in the frame's orientation)"""
    k = _d4_elem(elem)
    if mode not in D4_MODES:
        raise ValueError(f'accumulate mode must be one of {sorted(D4_MODES)}, got {mode!r}')
    return k, D4_MODES[mode], float(scale), ((wy, hy) if k & 4 else (hy, wy))


def _d4_acc(acc, out, n, fh, fw, ky, kx):
    """The float32 accumulator rectangle that goes with the byte rectangle `out`: the same pixels of a (N, 3, H, W) scratch."""
    kh, kw, row, plane, img = _rect_dst(acc, n, fh, fw, ky, kx, False)
    if (kh, kw) != (out.shape[1], out.shape[2]):
        raise ValueError(f'the accumulator rectangle is {kh} x {kw}, the byte rectangle {out.shape[1]} x {out.shape[2]}')
    return row, plane, img


def upsample4x_add_rect_d4(y, base, out, ky=0, kx=0, elem=0, mode='only', scale=1.0):
    """upsample4x_add_rect under a symmetry, accumulating: value = d4_invert(y + bilinear_x4(base), elem)[:, :, ky:ky + kh, kx:kx + kw] with y
    and base in the tile's own, transformed orientation; `out` (a float32 rectangle view, the accumulator) takes value ('first'),
    out + value ('middle'), (out + value) * scale ('last') or value * scale ('only')."""
    require_gpu(y, base)
    base = base.contiguous()
    n, c, h, w = base.shape
    if c != 3:
        raise NotImplementedError(f'the rectangle stores are for RGB images: 3 channels, got {c}')
    assert y.is_contiguous() and tuple(y.shape) == (n, c, 4 * h, 4 * w)
    k, bits, scale, (fh, fw) = _d4_tail(elem, mode, scale, 4 * h, 4 * w)
    kh, kw, row, plane, img = _rect_dst(out, n, fh, fw, ky, kx, False)
    _run('upsample4x_add_rect_d4', lambda: _lib.check(_lib.lib().edvr_upsample4x_add_rect_d4_f32(
        _ptr(y), _ptr(base), _ptr(out), n, h, w, int(ky), int(kx), kh, kw, row, plane, img, k, bits, scale, _stream()), 'edvr_upsample4x_add_rect_d4_f32'),
         0, _nb(base) + 36.0 * n * kh * kw)
    void_bound(out)
    return out


def upsample4x_add_u8_rect_d4(y, base, out, acc, ky=0, kx=0, elem=0, mode='only', scale=1.0):
    """The byte form: `acc` (the float32 rectangle of a scratch that goes with the uint8 rectangle `out`) accumulates as in
    upsample4x_add_rect_d4; the 'last' / 'only' launch reads it and stores tensor2img bytes of the result into `out` instead."""
    require_gpu(y, base)
    base = base.contiguous()
    n, c, h, w = base.shape
    if c != 3:
        raise NotImplementedError(f'the uint8 output is interleaved RGB: 3 channels, got {c}')
    assert y.is_contiguous() and tuple(y.shape) == (n, c, 4 * h, 4 * w)
    k, bits, scale, (fh, fw) = _d4_tail(elem, mode, scale, 4 * h, 4 * w)
    kh, kw, row, _, img = _rect_dst(out, n, fh, fw, ky, kx, True)
    a_row, a_plane, a_img = _d4_acc(acc, out, n, fh, fw, ky, kx)
    _run('upsample4x_add_u8_rect_d4', lambda: _lib.check(_lib.lib().edvr_upsample4x_add_rect_d4_u8(
        _ptr(y), _ptr(base), _ptr(acc), _ptr(out), n, h, w, int(ky), int(kx), kh, kw, a_row, a_plane, a_img, row, img, k, bits, scale, _stream()),
        'edvr_upsample4x_add_rect_d4_u8'), 0, _nb(base) + 36.0 * n * kh * kw)
    return out


def f32_to_u8_hwc_rect_d4(x, out, acc, ky=0, kx=0, elem=0, mode='only', scale=1.0):
    """f32_to_u8_hwc_rect under a symmetry, accumulating in `acc` as upsample4x_add_u8_rect_d4 does (value = d4_invert(x, elem)[...])."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    if c != 3:
        raise NotImplementedError(f'the uint8 output is interleaved RGB: 3 channels, got {c}')
    k, bits, scale, (fh, fw) = _d4_tail(elem, mode, scale, h, w)
    kh, kw, row, _, img = _rect_dst(out, n, fh, fw, ky, kx, True)
    a_row, a_plane, a_img = _d4_acc(acc, out, n, fh, fw, ky, kx)
    _run('f32_to_u8_hwc_rect_d4', lambda: _lib.check(_lib.lib().edvr_f32_to_u8_hwc_rect_d4(
        _ptr(x), _ptr(acc), _ptr(out), n, h, w, _img_stride(x), int(ky), int(kx), kh, kw, a_row, a_plane, a_img, row, img, k, bits, scale, _stream()),
        'edvr_f32_to_u8_hwc_rect_d4'), 0, 36.0 * n * kh * kw)
    return out


def copy_rect_d4(x, out, ky=0, kx=0, elem=0, mode='only', scale=1.0):
    """copy_rect under a symmetry, accumulating in the float32 rectangle `out` (value = d4_invert(x, elem)[:, :, ky:ky + kh, kx:kx + kw])."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    if c != 3:
        raise NotImplementedError(f'the rectangle stores are for RGB images: 3 channels, got {c}')
    k, bits, scale, (fh, fw) = _d4_tail(elem, mode, scale, h, w)
    kh, kw, row, plane, img = _rect_dst(out, n, fh, fw, ky, kx, False)
    _run('copy_rect_d4', lambda: _lib.check(_lib.lib().edvr_copy_rect_d4_f32(
        _ptr(x), _ptr(out), n, h, w, _img_stride(x), int(ky), int(kx), kh, kw, row, plane, img, k, bits, scale, _stream()), 'edvr_copy_rect_d4_f32'),
         0, 36.0 * n * kh * kw)
    void_bound(out)
    return out


# ------------------------------------------------------------------------------------------------ tile blending (csrc/ensemble.hip)
def _bands(bands, kh, kw):
    """(low, high band lengths of the rows; low, high of the columns) of a rectangle, output pixels: each 0 or the one width B."""
    try:
        vals = tuple(bands)
    except TypeError:
        vals = ()
    if len(vals) != 4 or any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in vals):
        raise ValueError(f'bands are four non-negative integers (y low, y high, x low, x high), got {bands!r}')
    B = max(vals)
    if any(v not in (0, B) for v in vals):
        raise ValueError(f'every band has the same width: each of {vals} must be 0 or {B}')
    if vals[0] + vals[1] > kh or vals[2] + vals[3] > kw:
        raise ValueError(f'the bands {vals} of an axis overlap inside a {kh} x {kw} rectangle')
    return vals


def upsample4x_add_rect_blend(y, base, out, ky=0, kx=0, bands=(0, 0, 0, 0), elem=0, mode='only', scale=1.0):
    """upsample4x_add_rect_d4 with a weight per pixel: `out` (ky, kx, kh, kw) is a tile's extended rectangle, bands = (y low, y high, x
    low, x high) how many of its first / last rows / columns are a band of B output pixels shared with the neighbouring tile.  Weight of
    band pixel j: r(j) = float32(2 j + 1) / float32(2 B) in a low band, 1 - r(j) in a high band, 1 elsewhere; w = w_y * w_x.  A pixel in no
    low band with 'first' / 'only': out = w * value, else out = out + w * value; in no high band with 'last' / 'only': that times scale
    (include/edvr_amd.h: edvr_*_rect_blend_*)."""
    require_gpu(y, base)
    base = base.contiguous()
    n, c, h, w = base.shape
    if c != 3:
        raise NotImplementedError(f'the rectangle stores are for RGB images: 3 channels, got {c}')
    assert y.is_contiguous() and tuple(y.shape) == (n, c, 4 * h, 4 * w)
    k, bits, scale, (fh, fw) = _d4_tail(elem, mode, scale, 4 * h, 4 * w)
    kh, kw, row, plane, img = _rect_dst(out, n, fh, fw, ky, kx, False)
    bd = _bands(bands, kh, kw)
    _run('upsample4x_add_rect_blend', lambda: _lib.check(_lib.lib().edvr_upsample4x_add_rect_blend_f32(
        _ptr(y), _ptr(base), _ptr(out), n, h, w, int(ky), int(kx), kh, kw, row, plane, img, k, bits, scale, *bd, _stream()),
        'edvr_upsample4x_add_rect_blend_f32'), 0, _nb(base) + 36.0 * n * kh * kw)
    void_bound(out)
    return out


def upsample4x_add_u8_rect_blend(y, base, out, acc, ky=0, kx=0, bands=(0, 0, 0, 0), elem=0, mode='only', scale=1.0):
    """The byte form: `acc` (the float32 rectangle of a scratch that goes with the uint8 rectangle `out`) accumulates as in
    upsample4x_add_rect_blend; a pixel's last contributor stores the tensor2img bytes of its result into `out` instead."""
    require_gpu(y, base)
    base = base.contiguous()
    n, c, h, w = base.shape
    if c != 3:
        raise NotImplementedError(f'the uint8 output is interleaved RGB: 3 channels, got {c}')
    assert y.is_contiguous() and tuple(y.shape) == (n, c, 4 * h, 4 * w)
    k, bits, scale, (fh, fw) = _d4_tail(elem, mode, scale, 4 * h, 4 * w)
    kh, kw, row, _, img = _rect_dst(out, n, fh, fw, ky, kx, True)
    a_row, a_plane, a_img = _d4_acc(acc, out, n, fh, fw, ky, kx)
    bd = _bands(bands, kh, kw)
    _run('upsample4x_add_u8_rect_blend', lambda: _lib.check(_lib.lib().edvr_upsample4x_add_rect_blend_u8(
        _ptr(y), _ptr(base), _ptr(acc), _ptr(out), n, h, w, int(ky), int(kx), kh, kw, a_row, a_plane, a_img, row, img, k, bits, scale, *bd, _stream()),
        'edvr_upsample4x_add_rect_blend_u8'), 0, _nb(base) + 36.0 * n * kh * kw)
    return out


def f32_to_u8_hwc_rect_blend(x, out, acc, ky=0, kx=0, bands=(0, 0, 0, 0), elem=0, mode='only', scale=1.0):
    """f32_to_u8_hwc_rect_d4 with the weights of upsample4x_add_rect_blend, accumulating in `acc` as upsample4x_add_u8_rect_blend does."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    if c != 3:
        raise NotImplementedError(f'the uint8 output is interleaved RGB: 3 channels, got {c}')
    k, bits, scale, (fh, fw) = _d4_tail(elem, mode, scale, h, w)
    kh, kw, row, _, img = _rect_dst(out, n, fh, fw, ky, kx, True)
    a_row, a_plane, a_img = _d4_acc(acc, out, n, fh, fw, ky, kx)
    bd = _bands(bands, kh, kw)
    _run('f32_to_u8_hwc_rect_blend', lambda: _lib.check(_lib.lib().edvr_f32_to_u8_hwc_rect_blend(
        _ptr(x), _ptr(acc), _ptr(out), n, h, w, _img_stride(x), int(ky), int(kx), kh, kw, a_row, a_plane, a_img, row, img, k, bits, scale, *bd, _stream()),
        'edvr_f32_to_u8_hwc_rect_blend'), 0, 36.0 * n * kh * kw)
    return out


def copy_rect_blend(x, out, ky=0, kx=0, bands=(0, 0, 0, 0), elem=0, mode='only', scale=1.0):
    """copy_rect_d4 with the weights of upsample4x_add_rect_blend, accumulating in the float32 rectangle `out`."""
    require_gpu(x)
    x = _as_planes(x)
    n, c, h, w = x.shape
    if c != 3:
        raise NotImplementedError(f'the rectangle stores are for RGB images: 3 channels, got {c}')
    k, bits, scale, (fh, fw) = _d4_tail(elem, mode, scale, h, w)
    kh, kw, row, plane, img = _rect_dst(out, n, fh, fw, ky, kx, False)
    bd = _bands(bands, kh, kw)
    _run('copy_rect_blend', lambda: _lib.check(_lib.lib().edvr_copy_rect_blend_f32(
        _ptr(x), _ptr(out), n, h, w, _img_stride(x), int(ky), int(kx), kh, kw, row, plane, img, k, bits, scale, *bd, _stream()), 'edvr_copy_rect_blend_f32'),
         0, 36.0 * n * kh * kw)
    void_bound(out)
    return out


# ------------------------------------------------------------------------------------------------ bicubic imresize (csrc/resize.hip)
def imresize(frames, scale, antialiasing=True, out_dtype=torch.float32):
    """MATLAB-style bicubic imresize (basicsr/utils/matlab_functions.py:88-170) of a batch of frames in ONE launch, weights computed in
    the kernel: frames uint8 (n, H, W, 3) (byte / 255 as frames_u8_to_f32 rounds it) or float32 (n, 3, H, W) with dense images (a slice of
    a longer video works) -> out_dtype float32 (n, 3, H', W'), not clamped, or uint8 (n, H', W', 3) = tensor2img of that float, bit for
    bit; (H', W') = data.imresize_shape(H, W, scale, antialiasing), which also raises the ValueError for a scale outside [1/8, 8] and for
    frames shorter than the symmetric extension reaches - before anything is launched."""
    from .data import imresize_shape
    if not frames.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'out_dtype must be torch.float32 or torch.uint8, got {out_dtype}')
    u8 = frames.dtype == torch.uint8
    if u8:
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f'uint8 frames are (n, H, W, 3), got {tuple(frames.shape)}')
        frames = frames.contiguous()
        n, H, W, _ = frames.shape
    else:
        require_gpu(frames)
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f'float32 frames are (n, 3, H, W), got {tuple(frames.shape)}')
        frames = _as_planes(frames)
        n, _, H, W = frames.shape
    if not 0 < n <= 65535:
        raise ValueError(f'imresize takes 1..65535 frames per call, got {n}')
    scale = float(scale)
    ho, wo = imresize_shape(H, W, scale, antialiasing)
    u8out = out_dtype == torch.uint8
    out = torch.empty((n, ho, wo, 3) if u8out else (n, 3, ho, wo), dtype=out_dtype, device=frames.device)
    nbytes = 3.0 * n * (H * W * (1 if u8 else 4) + ho * wo * (1 if u8out else 4))  # source + output, each element once
    if u8:
        _run('imresize', lambda: _lib.check(_lib.lib().edvr_imresize_bicubic_u8(_ptr(frames), _ptr(out), n, H, W, ho, wo, scale, int(bool(antialiasing)),
                                                                                int(u8out), _stream()), 'edvr_imresize_bicubic_u8'), 0, nbytes)
    else:
        _run('imresize', lambda: _lib.check(_lib.lib().edvr_imresize_bicubic_f32(_ptr(frames), _ptr(out), n, H, W, _img_stride(frames), ho, wo, scale,
                                                                                 int(bool(antialiasing)), int(u8out), _stream()),
                                            'edvr_imresize_bicubic_f32'), 0, nbytes)
    return out


# ------------------------------------------------------------------------------------------------ resampling to a size (csrc/resample.hip)
def _resample_size(size):
    try:
        ho, wo = size
        ho, wo = int(ho), int(wo)
    except (TypeError, ValueError):
        raise ValueError(f'size is (Ho, Wo), got {size!r}') from None
    return ho, wo


def resample_tile(H, W, Ho, Wo, Ty, Tx):
    """(toh, tow): the output tile a workgroup of resample owns for (H, W) -> (Ho, Wo) with Ty / Tx taps (resample.taps) - tow is 64,
    toh falls from 32 as H / Ho grows toward 8.  Host arithmetic: no GPU needed."""
    toh, tow = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().edvr_resample_tile(int(H), int(W), int(Ho), int(Wo), int(Ty), int(Tx), ctypes.byref(toh), ctypes.byref(tow))
    if rc != 0:
        raise ValueError(_lib.lib().edvr_last_error().decode())
    return toh.value, tow.value


def resample(frames, size, kernel='lanczos3', out=None):
    """Frames at a stated size (the project's own definition) in ONE launch: frames float32 (n, c, H, W) with
    dense planes (a slice of a longer video works, any base alignment), size = (Ho, Wo), each axis with its own ratio, 1/8 <= I / O <= 8;
    kernel 'lanczos3' | 'bicubic' (Keys, -0.5) | 'bilinear', stretched by I / O when reducing.  Pixel centres are aligned, the edge
    sample repeats, columns first, then rows, every sum in float64 in tap order and rounded to float32 once per pass; an axis that keeps
    its length is the identity.  Nothing is clamped (Lanczos overshoots [0, 1]; the encoders saturate).  Returns float32 (n, c, Ho, Wo);
    out: such a tensor with dense planes to write into instead (a slice of a longer one works); it must not overlap frames.  The axis
    tables are made on the host once per (I, O, kernel, device) (resample.device_table): a later call allocates its output and
    nothing else, and waits for nothing.  NotImplementedError for a CPU tensor; ValueError - before anything is launched - for a wrong
    dtype, rank, kernel name or size, a ratio outside [1/8, 8], more than 65535 frames, a wrong `out`."""
    from . import resample as tables
    if not frames.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if frames.dtype != torch.float32:
        raise ValueError(f'resample takes float32 frames, got {frames.dtype}')
    if frames.dim() != 4:
        raise ValueError(f'frames are (n, c, H, W), got {tuple(frames.shape)}')
    if kernel not in tables.KERNELS:
        raise ValueError(f'kernel must be one of {sorted(tables.KERNELS)}, got {kernel!r}')
    ho, wo = _resample_size(size)
    n, c, H, W = frames.shape
    if not 0 < n <= 65535 or c < 1 or H < 1 or W < 1:
        raise ValueError(f'resample takes 1..65535 frames of at least one plane, got {tuple(frames.shape)}')
    tables.check_axis(H, ho, 'the row')
    tables.check_axis(W, wo, 'the column')
    if out is None:
        out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=frames.device)
    else:
        if not out.is_cuda or out.device != frames.device or out.dtype != torch.float32:
            raise ValueError(f'out is a float32 tensor on {frames.device}, got {out.dtype} on {out.device}')
        if tuple(out.shape) != (n, c, ho, wo) or not _plane_contig(out):
            raise ValueError(f'out is ({n}, {c}, {ho}, {wo}) with dense planes, got {tuple(out.shape)} with strides {tuple(out.stride())}')
        if _overlaps(out, frames):
            raise ValueError('out overlaps frames')
    frames = _as_planes(frames)
    fy, wy, ty = tables.device_table(H, ho, kernel, frames.device)
    fx, wx, tx = tables.device_table(W, wo, kernel, frames.device)
    _run('resample', lambda: _lib.check(_lib.lib().edvr_resample_f32(_ptr(frames), _ptr(out), n, c, H, W, _img_stride(frames), ho, wo, _img_stride(out),
                                                                     _ptr(fy), _ptr(wy), ty, _ptr(fx), _ptr(wx), tx, _stream()), 'edvr_resample_f32'),
         0, 4.0 * n * c * (H * W + ho * wo))  # source + output, each element once
    return out


# ------------------------------------------------------------------------------------------------ BD downsampling (csrc/bd.hip)
def bd_downsample(frames, scale=4, out_dtype=torch.float32):
    """DUF's "BD" degradation (duf_downsample, basicsr/data/data_util.py:281-331) of a batch of frames in ONE launch: the 13 x 13 Gaussian
    of sigma 0.4 * scale over the reflected frame, sampled at every scale-th input sample.  frames uint8 (n, H, W, 3) (byte / 255 as
    frames_u8_to_f32 rounds it) or float32 (n, 3, H, W) with dense images (a slice of a longer video works) -> out_dtype float32
    (n, 3, H', W'), not clamped, or uint8 (n, H', W', 3) = tensor2img of that float, bit for bit; (H', W') = data.bd_shape(H, W, scale),
    which also raises the ValueError for a scale outside {2, 3, 4} and for frames of fewer than 7 rows or columns - before anything is
    launched."""
    from .data import bd_shape
    if not frames.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'out_dtype must be torch.float32 or torch.uint8, got {out_dtype}')
    u8 = frames.dtype == torch.uint8
    if u8:
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f'uint8 frames are (n, H, W, 3), got {tuple(frames.shape)}')
        frames = frames.contiguous()
        n, H, W, _ = frames.shape
    else:
        require_gpu(frames)
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f'float32 frames are (n, 3, H, W), got {tuple(frames.shape)}')
        frames = _as_planes(frames)
        n, _, H, W = frames.shape
    if not 0 < n <= 65535:
        raise ValueError(f'bd_downsample takes 1..65535 frames per call, got {n}')
    ho, wo = bd_shape(H, W, scale)
    scale = int(scale)
    u8out = out_dtype == torch.uint8
    out = torch.empty((n, ho, wo, 3) if u8out else (n, 3, ho, wo), dtype=out_dtype, device=frames.device)
    nbytes = 3.0 * n * (H * W * (1 if u8 else 4) + ho * wo * (1 if u8out else 4))  # source + output, each element once
    if u8:
        _run('bd_downsample', lambda: _lib.check(_lib.lib().edvr_bd_downsample_u8(_ptr(frames), _ptr(out), n, H, W, ho, wo, scale, int(u8out), _stream()),
                                                 'edvr_bd_downsample_u8'), 0, nbytes)
    else:
        _run('bd_downsample', lambda: _lib.check(_lib.lib().edvr_bd_downsample_f32(_ptr(frames), _ptr(out), n, H, W, _img_stride(frames), ho, wo, scale,
                                                                                   int(u8out), _stream()), 'edvr_bd_downsample_f32'), 0, nbytes)
    return out


# ------------------------------------------------------------------------------------------------ LQ training crops from GT windows
def lq_crops_from_windows(windows, table, scale, degradation, table_host=None):
    """The LQ crops of a training batch from windows of their GT frames, in ONE launch of the imresize ('bi') or bd_downsample ('bd')
    kernel on another view of its source: windows uint8 (n, e, pitch) - n windows of e rows of e RGB pixels, rows `pitch` =
    data.lq_window_pitch(e) bytes apart, e = data.lq_window_extent(p, scale, degradation) - and table int32 (n, 8), both on the GPU (one
    record per window: its origin y0, x0 in the frame, the mod-cropped frame's H, W, the crop's origin top, left in the LQ frame) ->
    uint8 (n, p, p, 3): bit for bit imresize(frame, 1 / scale, out_dtype=uint8)[top:top + p, left:left + p] / the same of bd_downsample.
    table_host: the same table in host memory (the pinned slot it was copied from), which the launch checks record by record before it
    starts anything - without it only scale, extent and pitch are checked, and the kernel clamps every index into the window.
    ValueError for a scale outside {2, 3, 4}, an unknown degradation and an e no crop size has; there is no CPU fallback."""
    from .data import LQ_WINDOW_RECORD_INTS, lq_window_size
    require_gpu(windows, dtypes=(torch.uint8,))
    require_gpu(table, dtypes=(torch.int32,))
    if windows.dim() != 3 or table.dim() != 2 or table.shape != (windows.shape[0], LQ_WINDOW_RECORD_INTS):
        raise ValueError(f'windows are (n, e, pitch) uint8 with an (n, {LQ_WINDOW_RECORD_INTS}) int32 table, got {tuple(windows.shape)} and {tuple(table.shape)}')
    n, e, pitch = windows.shape
    if not 0 < n <= 65535:
        raise ValueError(f'lq_crops_from_windows takes 1..65535 windows per call, got {n}')
    p = lq_window_size(e, scale, degradation)  # ValueError: scale, degradation, extent
    scale = int(scale)
    if pitch % 16 or pitch < 3 * e:
        raise ValueError(f'window rows of {e} pixels are {pitch} bytes apart: not a multiple of 16 that holds {3 * e}')
    windows, table = windows.contiguous(), table.contiguous()
    if table_host is not None:
        if table_host.is_cuda or table_host.dtype != torch.int32 or table_host.shape != table.shape or not table_host.is_contiguous():
            raise ValueError('table_host is the table as a contiguous int32 host tensor')
    out = torch.empty((n, p, p, 3), dtype=torch.uint8, device=windows.device)
    nbytes = 3.0 * n * (e * e + p * p) + 4.0 * table.numel()  # window pixels + table read, crops written, each element once
    name = 'edvr_imresize_bicubic_u8_windows' if degradation == 'bi' else 'edvr_bd_downsample_u8_windows'
    _run('lq_crops_from_windows', lambda: _lib.check(getattr(_lib.lib(), name)(_ptr(windows), _ptr(table), _ptr(table_host), _ptr(out), n, p, e, e, pitch,
                                                                                scale, _stream()), name), 0, nbytes)
    return out


# ------------------------------------------------------------------------------------------------ planar Y'CbCr <-> RGB (csrc/yuv.hip)
# (Kr, Kb).  'bt2020nc' is BT.2020 non-constant luminance under the name ffmpeg's -colorspace gives it; a bare 'bt2020', which does not
# say which of the standard's two systems is meant, stays an unknown name
YUV_MATRICES = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722), 'bt2020nc': (0.2627, 0.0593)}
YUV_RANGES = {'limited': (219.0, 224.0, 16.0), 'full': (255.0, 255.0, 0.0)}     # luma scale, chroma scale, luma offset (chroma offset 128)
YUV_SUBSAMPLINGS = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}                    # (sx, sy): log2 of the chroma decimation per axis
_YUV_ALIASES = {'420jpeg': '420', '420mpeg2': '420', '420paldv': '420'}
# chroma siting -> (horizontal, vertical): 0 centre, 1 co-sited with the even luma samples; read along subsampled axes only
YUV_SITINGS = {'center': (0, 0), 'left': (1, 0), 'topleft': (1, 1)}


def _yuv_siting(siting, sx, sy):
    """A siting name -> (cx, cy) for a format of subsampling (sx, sy): an axis that is not subsampled has no siting (0)."""
    if not isinstance(siting, str) or siting not in YUV_SITINGS:
        raise ValueError(f'siting must be one of {sorted(YUV_SITINGS)}, got {siting!r}')
    cx, cy = YUV_SITINGS[siting]
    return cx & sx, cy & sy


def yuv_format(name):
    """A Y4M format name -> (sx, sy, depth, canonical): '420' | '422' | '444' (chroma planes ((H + sy) >> sy, (W + sx) >> sx)) with an
    optional suffix p9 ... p16 for the bit depth (none: 8 bits; p8 is not a Y4M tag).  '420jpeg', '420mpeg2' and '420paldv' are
    aliases of '420'.  canonical: '420', '422p10', '444p16' ...  ValueError for anything else."""
    if not isinstance(name, str):
        raise ValueError(f'a format is a name such as 420, 422p10 or 444p16, got {name!r}')
    base, sep, bits = _YUV_ALIASES.get(name, name).partition('p')
    depth = 8
    if sep:
        if not (bits.isascii() and bits.isdigit()) or bits != str(int(bits)) or not 9 <= int(bits) <= 16:
            raise ValueError(f'format {name!r}: the depth suffix is p9 ... p16')
        depth = int(bits)
    if base not in YUV_SUBSAMPLINGS:
        raise ValueError(f'format {name!r}: the subsampling is one of {sorted(YUV_SUBSAMPLINGS)} (mono, 4:1:1, 4:4:0 and alpha are not supported)')
    sx, sy = YUV_SUBSAMPLINGS[base]
    return sx, sy, depth, base + (f'p{depth}' if depth > 8 else '')


def yuv_frame_size(H, W, fmt='420'):
    """BYTES of one frame of (H, W) in format `fmt`: the luma plane and two chroma planes of ((H + sy) >> sy, (W + sx) >> sx), one
    byte per sample at 8 bits and two above."""
    sx, sy, depth, _ = yuv_format(fmt)
    return _yuv_frame_bytes(H, W, sx, sy, depth)


def _yuv_frame_bytes(H, W, sx, sy, depth):
    return (H * W + 2 * ((H + sy) >> sy) * ((W + sx) >> sx)) * (2 if depth > 8 else 1)


def yuv420_frame_size(H, W):
    """Bytes of one I420 frame of (H, W): the luma plane and two chroma planes of (ceil(H / 2), ceil(W / 2))."""
    return yuv_frame_size(H, W, '420')


def yuv_coeffs(matrix='bt601', range='limited', depth=8):
    """(M, Mi, off) in float64 (nested lists): M maps RGB in 0 ... 255 to (Y, Cb, Cr) before the offsets off = (yoff, coff, coff), Mi is its
    inverse (adjugate over determinant, every step one float64 operation).  The kernels get both rounded to float32.  depth 8 ... 16
    (DESIGN 4.14), k = 2^(depth - 8): 'limited' scales luma to 219 k and chroma to 224 k with offsets (16 k, 128 k), 'full' both to
    2^depth - 1 with offsets (0, 2^(depth - 1)); at depth 8 these are the 8-bit numbers, (yoff, 128, 128)."""
    if matrix not in YUV_MATRICES:
        raise ValueError(f'matrix must be one of {sorted(YUV_MATRICES)}, got {matrix!r}')
    if range not in YUV_RANGES:
        raise ValueError(f'range must be one of {sorted(YUV_RANGES)}, got {range!r}')
    if depth != int(depth) or not 8 <= depth <= 16:
        raise ValueError(f'depth must be 8 ... 16, got {depth!r}')
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    ys, cs, yoff = YUV_RANGES[range]
    k = float(1 << (int(depth) - 8))
    if range == 'full':
        ys = cs = float((1 << int(depth)) - 1)
    else:
        ys, cs, yoff = ys * k, cs * k, yoff * k
    sy, scb, scr = ys / 255.0, cs / 255.0 / (2.0 * (1.0 - kb)), cs / 255.0 / (2.0 * (1.0 - kr))
    m = [[sy * kr, sy * kg, sy * kb], [scb * -kr, scb * -kg, scb * (1.0 - kb)], [scr * (1.0 - kr), scr * -kg, scr * -kb]]
    (a, b, c), (d, e, f), (g, h, i) = m
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * adj[0][0] + b * adj[1][0] + c * adj[2][0]
    return m, [[v / det for v in row] for row in adj], [yoff, 128.0 * k, 128.0 * k]


def _yuv_coef_arg(mat, off):
    return (ctypes.c_float * 12)(*[v for row in mat for v in row], *off)


def _yuv_batch(yuv, H, W, fmt, what):
    """Checks a (n, >= framesize) byte batch of frames, fmt = yuv_format(name) -> (n, framesize, bytes between frames)."""
    if yuv.dim() != 2:
        raise ValueError(f'{what} is a 2-D uint8 batch (n, >= framesize), got {tuple(yuv.shape)}')
    if H < 1 or W < 1:
        raise ValueError(f'a frame has at least one row and column, got {H} x {W}')
    sx, sy, depth, canonical = fmt
    fs = _yuv_frame_bytes(H, W, sx, sy, depth)
    if yuv.shape[1] < fs:
        raise ValueError(f'{what}: rows of {yuv.shape[1]} bytes are shorter than the {fs} bytes of a {H} x {W} {canonical} frame')
    if yuv.stride(1) != 1:
        raise ValueError(f'{what}: the bytes of a frame must be contiguous (stride(1) == 1), got stride {yuv.stride(1)}')
    n = yuv.shape[0]
    if n < 1:
        raise ValueError(f'{what}: no frames')
    if n > 1 and yuv.stride(0) < fs:
        raise ValueError(f'{what}: frames {yuv.stride(0)} bytes apart overlap')
    if depth > 8 and (yuv.data_ptr() % 2 or (n > 1 and yuv.stride(0) % 2)):
        raise ValueError(f'{what}: the 16-bit samples of {canonical} need an even base address and an even row stride, got address '
                         f'{yuv.data_ptr():#x}, stride {yuv.stride(0)}')
    return n, fs, (yuv.stride(0) if n > 1 else fs)


_YUV420 = (1, 1, 8, '420')  # yuv_format('420')


def _yuv_decode(op, yuv, H, W, fmt, matrix, range, chroma, out_dtype, siting='center'):
    """Both decodes, fmt = yuv_format(name); uint8 RGB (n, H, W, 3) exists for 8-bit 4:2:0 alone, through edvr_yuv420_to_rgb_u8.  A siting
    that co-sites an axis the format subsamples goes through the _sited entry points; everything else through the ones it always did."""
    if chroma not in ('bilinear', 'nearest'):
        raise ValueError(f"chroma must be 'bilinear' or 'nearest', got {chroma!r}")
    sx, sy, depth, _ = fmt
    cx = cy = 0
    if siting != 'center':  # (the default pays this comparison and nothing else)
        cx, cy = _yuv_siting(siting, sx, sy)
        if chroma == 'nearest':
            cx = cy = 0  # replication has no siting
    _, mi, off = yuv_coeffs(matrix, range, depth)
    require_gpu(yuv, dtypes=(torch.uint8,))
    H, W = int(H), int(W)
    n, fs, stride = _yuv_batch(yuv, H, W, fmt, 'yuv')
    u8 = out_dtype == torch.uint8
    out = torch.empty((n, H, W, 3) if u8 else (n, 3, H, W), dtype=out_dtype, device=yuv.device)
    coef, bil = _yuv_coef_arg(mi, off), int(chroma == 'bilinear')
    if cx and u8:
        call = lambda: _lib.check(_lib.lib().edvr_yuv420_to_rgb_sited_u8(_ptr(yuv), _ptr(out), n, H, W, stride, coef, bil, cx, cy, _stream()),
                                  'edvr_yuv420_to_rgb_sited_u8')
    elif cx:
        call = lambda: _lib.check(_lib.lib().edvr_yuv_to_rgb_sited_f32(_ptr(yuv), _ptr(out), n, H, W, sx, sy, depth, stride, 3 * H * W, coef, bil, cx, cy,
                                                                        _stream()), 'edvr_yuv_to_rgb_sited_f32')
    elif u8:
        call = lambda: _lib.check(_lib.lib().edvr_yuv420_to_rgb_u8(_ptr(yuv), _ptr(out), n, H, W, stride, coef, bil, _stream()), 'edvr_yuv420_to_rgb_u8')
    else:
        call = lambda: _lib.check(_lib.lib().edvr_yuv_to_rgb_f32(_ptr(yuv), _ptr(out), n, H, W, sx, sy, depth, stride, 3 * H * W, coef, bil, _stream()),
                                  'edvr_yuv_to_rgb_f32')
    _run(op, call, 0, float(n) * (fs + 3 * H * W * (1 if u8 else 4)))
    return out


def yuv420_to_rgb(yuv, H, W, matrix='bt601', range='limited', chroma='bilinear', out_dtype=torch.float32, siting='center'):
    """8-bit I420 frames -> RGB in ONE launch.  yuv: uint8 (n, >= framesize) on the GPU with stride(1) == 1 and ANY row stride and base
    offset - each row starts with the H W luma bytes, then the (ceil(H / 2), ceil(W / 2)) Cb and Cr planes, i.e. the payload of a Y4M
    frame (`buf[:, 6:]` of a Y4MReader buffer works as it is).  matrix: a name of YUV_MATRICES, range 'limited' | 'full' (`yuv_coeffs`), chroma
    'bilinear' (the two-tap filter of the siting, vertical then horizontal, indices clamped) | 'nearest'.  siting (YUV_SITINGS, DESIGN
    4.15): where the chroma samples lie - 'center' (JPEG / MPEG-1: the 1/4 - 3/4 filter), 'left' (H.264 / HEVC / AV1: co-sited with the even
    luma columns - even columns take c[k], odd ones 0.5 c[k] + 0.5 c[k + 1]), 'topleft' (BT.2020 / UHD: rows likewise); 'nearest' ignores
    it.  Returns float32 (n, 3, H, W) in [0, 1] or uint8 (n, H, W, 3); the definition, operation by operation, is DESIGN 4.11.  ValueError
    for bad names and layouts."""
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'out_dtype must be torch.float32 or torch.uint8, got {out_dtype}')
    return _yuv_decode('yuv420_to_rgb', yuv, H, W, _YUV420, matrix, range, chroma, out_dtype, siting)


def yuv_to_rgb(yuv, H, W, fmt='420', matrix='bt601', range='limited', chroma='bilinear', siting='center'):
    """Planar Y'CbCr frames of any Y4M format -> float32 RGB (n, 3, H, W) in [0, 1], in ONE launch.  fmt: `yuv_format` - 4:2:0, 4:2:2 or
    4:4:4 at 8 ... 16 bits.  yuv: uint8 (n, >= yuv_frame_size(H, W, fmt)) on the GPU with stride(1) == 1 and any row stride and base
    offset (`buf[:, 6:]` of a Y4MReader buffer works as it is); above 8 bits a sample is a little-endian 16-bit word, whose bits above
    the depth are NOT masked, and the base address and row stride are even.  matrix, range: `yuv_coeffs` at the format's depth; chroma:
    'bilinear' (the two-tap filter of the siting along each subsampled axis, vertical then horizontal, indices clamped) | 'nearest'.
    siting: as yuv420_to_rgb takes it, per SUBSAMPLED axis - 'topleft' on 4:2:2 is 'left', any siting on 4:4:4 changes nothing.
    The definition is DESIGN 4.14 (siting: 4.15); at '420' it is that of yuv420_to_rgb, bit for bit.  ValueError for bad names and layouts."""
    return _yuv_decode('yuv_to_rgb', yuv, H, W, yuv_format(fmt), matrix, range, chroma, torch.float32, siting)


def _byte_span(t):
    """[first, last) byte addresses a tensor's elements lie in."""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    last = sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def _yuv_encode(op, rgb, fmt, matrix, range, out, u8_too, siting='center'):
    """Both encodes, fmt = yuv_format(name); uint8 RGB (n, H, W, 3) is read for 8-bit 4:2:0 alone (`u8_too`), through edvr_rgb_to_yuv420_u8.
    A siting that co-sites an axis the format subsamples goes through the _sited entry points."""
    sx, sy, depth, _ = fmt
    cx = cy = 0
    if siting != 'center':
        cx, cy = _yuv_siting(siting, sx, sy)
    m, _, off = yuv_coeffs(matrix, range, depth)
    if not rgb.is_cuda:
        raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    u8 = u8_too and rgb.dtype == torch.uint8
    if u8:
        if rgb.dim() != 4 or rgb.shape[-1] != 3:
            raise ValueError(f'uint8 frames are (n, H, W, 3), got {tuple(rgb.shape)}')
        rgb = rgb.contiguous()
        n, H, W, _ = rgb.shape
    else:
        require_gpu(rgb)
        if rgb.dim() != 4 or rgb.shape[1] != 3:
            raise ValueError(f'float32 frames are (n, 3, H, W), got {tuple(rgb.shape)}')
        rgb = _as_planes(rgb)
        n, _, H, W = rgb.shape
    if out is None:
        out = torch.empty((n, _yuv_frame_bytes(H, W, sx, sy, depth)), dtype=torch.uint8, device=rgb.device)
    else:
        require_gpu(out, dtypes=(torch.uint8,))
        if out.dim() == 2 and out.shape[0] != n:
            raise ValueError(f'out holds {out.shape[0]} frames, the input {n}')
    n, fs, stride = _yuv_batch(out, H, W, fmt, 'out')
    (a0, a1), (b0, b1) = _byte_span(rgb), _byte_span(out)
    if a0 < b1 and b0 < a1:
        raise ValueError('out overlaps the input')
    coef = _yuv_coef_arg(m, off)
    if cx and u8:
        call = lambda: _lib.check(_lib.lib().edvr_rgb_to_yuv420_sited_u8(_ptr(rgb), _ptr(out), n, H, W, stride, coef, cx, cy, _stream()),
                                  'edvr_rgb_to_yuv420_sited_u8')
    elif cx:
        call = lambda: _lib.check(_lib.lib().edvr_rgb_to_yuv_sited_f32(_ptr(rgb), _ptr(out), n, H, W, sx, sy, depth, _img_stride(rgb), stride, coef, cx, cy,
                                                                        _stream()), 'edvr_rgb_to_yuv_sited_f32')
    elif u8:
        call = lambda: _lib.check(_lib.lib().edvr_rgb_to_yuv420_u8(_ptr(rgb), _ptr(out), n, H, W, stride, coef, _stream()), 'edvr_rgb_to_yuv420_u8')
    else:
        call = lambda: _lib.check(_lib.lib().edvr_rgb_to_yuv_f32(_ptr(rgb), _ptr(out), n, H, W, sx, sy, depth, _img_stride(rgb), stride, coef, _stream()),
                                  'edvr_rgb_to_yuv_f32')
    _run(op, call, 0, float(n) * (fs + 3 * H * W * (1 if u8 else 4)))
    return out


def rgb_to_yuv420(rgb, matrix='bt601', range='limited', out=None, siting='center'):
    """RGB frames -> 8-bit I420 in ONE launch: rgb float32 (n, 3, H, W) (clamped to [0, 1], x 255, NOT rounded before the matrix: the
    only quantisation is the one to YUV bytes; dense images, a slice of a longer video works) or uint8 (n, H, W, 3).  Returns uint8
    (n, framesize), framesize = yuv420_frame_size(H, W): luma, then Cb and Cr, each the mean of its 2 x 2 block (an odd edge replicates).
    out: a uint8 (n, >= framesize) batch to write into instead, stride(1) == 1, any row stride and base offset (`buf[:, 6:]` of a Y4M
    write buffer); bytes past a frame's end are left alone and `out` is returned.  siting (YUV_SITINGS): where the chroma
    samples are to lie - 'center' (the mean above), 'left' ([1 2 1] / 4 over the columns around the even one, the mean of the two rows),
    'topleft' ([1 2 1] / 4 along both axes, around the even row and column); indices clamped to the frame.  ValueError for bad names,
    layouts and an `out` that overlaps the input."""
    return _yuv_encode('rgb_to_yuv420', rgb, _YUV420, matrix, range, out, True, siting)


def rgb_to_yuv(rgb, fmt='420', matrix='bt601', range='limited', out=None, siting='center'):
    """float32 RGB (n, 3, H, W) -> planar Y'CbCr frames of any Y4M format in ONE launch (clamped to [0, 1], x 255, NOT rounded before
    the matrix: the only quantisation is the one to samples of the format's depth; dense images, a slice of a longer video works).
    Returns uint8 (n, yuv_frame_size(H, W, fmt)): luma, then Cb and Cr - the mean of a 2 x 2 block (4:2:0) or of a pair of columns
    (4:2:2), an odd edge replicating, or the sample itself (4:4:4) - clamped to [0, 2^depth - 1] and rounded half to even, a byte or a
    little-endian 16-bit word each.  out: a uint8 (n, >= framesize) batch to write into instead, stride(1) == 1, any row stride and base
    offset (even ones above 8 bits; `buf[:, 6:]` of a Y4M write buffer); bytes past a frame's end are left alone and `out` is returned.
    uint8 RGB stays with rgb_to_yuv420.  siting: as rgb_to_yuv420 takes it, per SUBSAMPLED axis ('topleft' on 4:2:2 is 'left', 4:4:4 has
    none).  The definition is DESIGN 4.14 (siting: 4.15).  ValueError for bad names, layouts and an `out` that overlaps the input."""
    return _yuv_encode('rgb_to_yuv', rgb, yuv_format(fmt), matrix, range, out, False, siting)


# ------------------------------------------------------------------------------------------------ deinterlacing (csrc/deint.hip)
DEINT_FIRST = {'top': 0, 'bottom': 1}   # which field of a frame is the earlier one: its even rows ('top', Y4M It) or its odd rows (Ib)
DEINT_MODES = {'field': 1, 'frame': 0}  # a frame per field (2 n out of n) or per frame (from its first field)
DEINT_ROWS_READ = 12 / 2 + 1 / 2        # row segments read per output row on average: 12 for a predicted row, 1 for a copied one


def _deint_context(t, fs, depth, what):
    """`prev` / `next` of deinterlace: one frame, uint8 (>= framesize,) or with a leading 1, dense."""
    if t is None:
        return None
    require_gpu(t, dtypes=(torch.uint8,))
    if t.dim() == 2 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 1 or t.shape[0] < fs:
        raise ValueError(f'{what} is one frame, uint8 ({fs},) or (1, {fs}), got {tuple(t.shape)}')
    if t.stride(0) != 1:
        t = t.contiguous()
    if depth > 8 and t.data_ptr() % 2:
        raise ValueError(f'{what}: 16-bit samples need an even base address, got {t.data_ptr():#x}')
    return t


def deinterlace(yuv, H, W, format='420', *, first='top', mode='field', prev=None, next=None, out=None):
    """Interlaced planar Y'CbCr frames -> progressive ones, on the samples as decoded, in ONE launch (integers
    only).  yuv: uint8 (n, >= yuv_frame_size(H, W, format)) on the GPU, as yuv_to_rgb takes it - stride(1) == 1, any row stride and base
    offset (`buf[:, 6:]` of a Y4MReader buffer), even ones above 8 bits.  Each frame weaves two fields, on its even and odd rows in every
    plane alike; first: 'top' - the even rows are the earlier field (Y4M `It`) - or 'bottom' (`Ib`).  mode 'field': every field becomes
    a frame - uint8 (2 n, framesize), frame 2 i + s from the s-th field in time of input frame i: a 25i clip is 50 pictures per second;
    'frame': the first field of every frame does, (n, framesize).  A field's own rows are copied; each missing sample is predicted along
    the least-different of five edge directions between the rows above and below it and clamped to a band around the mean of the
    fields before and after, as wide as the fields around it differ.  prev / next: the frame before / after the batch, uint8
    (framesize,) or with a leading 1: with them a batch inside a longer video gets exactly what the whole video would give
    (y4m.deinterlaced does that); on a side without one the field index reflects about the batch's end.  out: a uint8 (2 n | n, >=
    framesize) batch to write into instead, stride(1) == 1, any row stride and base offset (`buf[:, 6:]`); it must not overlap an input.
    H >= 4 (every plane needs two rows), any W.  Bytes booked: every output sample is written once and 12 / 2 + 1 / 2 row segments are
    read per output row on average (12 for a predicted row, 1 for a copied one): n_out framesize (1 + 6.5), most of it from the cache.
    NotImplementedError for CPU tensors, ValueError for bad names, shapes and layouts."""
    fmt = yuv_format(format)
    if first not in DEINT_FIRST:
        raise ValueError(f'first must be one of {sorted(DEINT_FIRST)}, got {first!r}')
    if mode not in DEINT_MODES:
        raise ValueError(f'mode must be one of {sorted(DEINT_MODES)}, got {mode!r}')
    require_gpu(yuv, dtypes=(torch.uint8,))
    H, W = int(H), int(W)
    if H < 4:
        raise ValueError(f'deinterlace: a frame needs at least 4 rows, so that every plane has 2, got {H} x {W}')
    sx, sy, depth, _ = fmt
    n, fs, stride = _yuv_batch(yuv, H, W, fmt, 'yuv')
    prev, next = _deint_context(prev, fs, depth, 'prev'), _deint_context(next, fs, depth, 'next')
    n_out = 2 * n if DEINT_MODES[mode] else n
    if out is None:
        out = torch.empty((n_out, fs), dtype=torch.uint8, device=yuv.device)
    else:
        require_gpu(out, dtypes=(torch.uint8,))
        if out.dim() == 2 and out.shape[0] != n_out:
            raise ValueError(f'out holds {out.shape[0]} frames, mode {mode!r} makes {n_out} of {n}')
    _, _, out_stride = _yuv_batch(out, H, W, fmt, 'out')
    b0, b1 = _byte_span(out)
    for t in (yuv, prev, next):
        if t is not None:
            a0, a1 = _byte_span(t)
            if a0 < b1 and b0 < a1:
                raise ValueError('out overlaps an input')
    _run('deinterlace', lambda: _lib.check(_lib.lib().edvr_deinterlace(_ptr(yuv), _ptr(prev), _ptr(next), _ptr(out), n, H, W, sx, sy, depth, stride,
                                                                       out_stride, DEINT_FIRST[first], DEINT_MODES[mode], _stream()),
                                           'edvr_deinterlace'), 0, float(n_out) * fs * (1.0 + DEINT_ROWS_READ))
    return out


# ------------------------------------------------------------------------------------------------ inverse telecine (csrc/telecine.hip)
FIELD_MATCH_COLUMNS = ('S_c', 'S_p', 'mic_c', 'mic_p', 'A', 'B', 'C')  # the columns of field_match's table
FIELD_MATCHES = {'c': 0, 'p': 1}  # field_weave's `matches`: the second field comes from the frame itself or from the frame before


def _film_level(v, what):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255:
        raise ValueError(f'{what} is an 8-bit level, an integer in 0 ... 255, got {v!r}')
    return v


def _overlaps(out, *inputs):
    b0, b1 = _byte_span(out)
    for t in inputs:
        if t is not None:
            a0, a1 = _byte_span(t)
            if a0 < b1 and b0 < a1:
                return True
    return False


def field_match(yuv, H, W, format='420', *, first='top', prev=None, prev2=None, nt=2, ct=9, out=None):
    """The measurements inverse telecine decides on (integers only), for all n frames in ONE kernel launch behind
    a clear of the table.  yuv: uint8 (n, >= yuv_frame_size(H, W, format)) on the GPU, as deinterlace takes it - stride(1) == 1, any
    row stride and base offset (`buf[:, 6:]` of a Y4MReader buffer), even ones above 8 bits; first: 'top' | 'bottom', the field that is
    earlier in time.  Only luma is read.  Returns int64 (n, 7) on the device, columns FIELD_MATCH_COLUMNS: for frame i, the comb sums
    S_c, S_p and the largest 16 x 16 block counts mic_c, mic_p of the two candidates - the frame as it is (c) and its first field woven
    with the second field of the frame before (p) - and the field differences A (first field against frame i - 1's), B (second field
    against frame i - 1's), C (second field against frame i - 2's).  prev / prev2: frame -1 / frame -2, uint8 (framesize,) or with a
    leading 1; where an earlier frame does not exist p is c and the differences are 0.  nt, ct: the comb thresholds in 8-bit levels
    (shifted by depth - 8).  Exact: a row does not depend on the batch it was computed in.  out: an int64 (n, 7) contiguous tensor
    to write into instead.  Bytes booked: the luma plane of every frame once, and the table.  H >= 4, any W.  NotImplementedError for
    CPU tensors, ValueError for bad names, shapes and layouts."""
    fmt = yuv_format(format)
    if first not in DEINT_FIRST:
        raise ValueError(f'first must be one of {sorted(DEINT_FIRST)}, got {first!r}')
    nt, ct = _film_level(nt, 'nt'), _film_level(ct, 'ct')
    require_gpu(yuv, dtypes=(torch.uint8,))
    H, W = int(H), int(W)
    if H < 4:
        raise ValueError(f'field_match: a frame needs at least 4 rows, so that every plane has 2, got {H} x {W}')
    sx, sy, depth, _ = fmt
    n, fs, stride = _yuv_batch(yuv, H, W, fmt, 'yuv')
    prev, prev2 = _deint_context(prev, fs, depth, 'prev'), _deint_context(prev2, fs, depth, 'prev2')
    if out is None:
        out = torch.empty((n, len(FIELD_MATCH_COLUMNS)), dtype=torch.int64, device=yuv.device)
    else:
        require_gpu(out, dtypes=(torch.int64,))
        if tuple(out.shape) != (n, len(FIELD_MATCH_COLUMNS)) or not out.is_contiguous():
            raise ValueError(f'out is a contiguous int64 ({n}, {len(FIELD_MATCH_COLUMNS)}) tensor, got {tuple(out.shape)}')
        if _overlaps(out, yuv, prev, prev2):
            raise ValueError('out overlaps an input')
    _run('field_match', lambda: _lib.check(_lib.lib().edvr_field_match(_ptr(yuv), _ptr(prev), _ptr(prev2), _ptr(out), n, H, W, sx, sy, depth, stride,
                                                                       DEINT_FIRST[first], nt, ct, _stream()), 'edvr_field_match'),
         0, float(n) * (H * W * (2 if depth > 8 else 1) + 8 * len(FIELD_MATCH_COLUMNS)))
    return out


def field_weave(yuv, H, W, format='420', *, first='top', frames, matches, prev=None, out=None):
    """Film frames put back together from their fields, all three planes, in ONE launch.  yuv: uint8 (n, >= framesize)
    on the GPU, as field_match takes it.  frames, matches: host sequences of equal length k >= 1 - output frame j takes its rows of
    `first`'s parity (the first field) from input frame frames[j] and its other rows from the same frame (matches[j] == 0, 'c') or from
    frame frames[j] - 1 (1, 'p'); frame -1 is `prev`, uint8 (framesize,) or with a leading 1.  Returns uint8 (k, framesize).  out: a
    uint8 (k, >= framesize) batch to write into instead, stride(1) == 1, any row stride and base offset (`buf[:, 6:]`); bytes outside the
    frames are left alone; it must not overlap an input.  The (frame, match) table travels to the device as one small int32 tensor.
    Bytes booked: every output byte read once and written once.  NotImplementedError for CPU tensors; ValueError for bad names,
    shapes and layouts, an index outside [0, n), a match other than 0 / 1, and a 'p' match of frame 0 without prev."""
    fmt = yuv_format(format)
    if first not in DEINT_FIRST:
        raise ValueError(f'first must be one of {sorted(DEINT_FIRST)}, got {first!r}')
    require_gpu(yuv, dtypes=(torch.uint8,))
    H, W = int(H), int(W)
    if H < 4:
        raise ValueError(f'field_weave: a frame needs at least 4 rows, so that every plane has 2, got {H} x {W}')
    sx, sy, depth, _ = fmt
    n, fs, stride = _yuv_batch(yuv, H, W, fmt, 'yuv')
    prev = _deint_context(prev, fs, depth, 'prev')
    try:
        frames, matches = list(frames), list(matches)
    except TypeError:
        raise ValueError('frames and matches are sequences of integers') from None
    if not frames or len(frames) != len(matches):
        raise ValueError(f'frames and matches are of one length, at least 1: got {len(frames)} and {len(matches)}')
    for f, m in zip(frames, matches):
        if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f < n:
            raise ValueError(f'frames are indices into the {n} input frames, got {f!r}')
        if isinstance(m, bool) or m not in (0, 1):
            raise ValueError(f"matches are 0 ('c') or 1 ('p'), got {m!r}")
        if m == 1 and f == 0 and prev is None:
            raise ValueError("a 'p' match of frame 0 needs prev: its second field lies in the frame before the batch")
    k = len(frames)
    if out is None:
        out = torch.empty((k, fs), dtype=torch.uint8, device=yuv.device)
    else:
        require_gpu(out, dtypes=(torch.uint8,))
        if out.dim() == 2 and out.shape[0] != k:
            raise ValueError(f'out holds {out.shape[0]} frames, the list names {k}')
    _, _, out_stride = _yuv_batch(out, H, W, fmt, 'out')
    if _overlaps(out, yuv, prev):
        raise ValueError('out overlaps an input')
    table = torch.tensor([v for pair in zip(frames, matches) for v in pair], dtype=torch.int32).to(yuv.device, non_blocking=True)
    _run('field_weave', lambda: _lib.check(_lib.lib().edvr_field_weave(_ptr(yuv), _ptr(prev), _ptr(out), _ptr(table), n, k, H, W, sx, sy, depth, stride,
                                                                       out_stride, DEINT_FIRST[first], _stream()), 'edvr_field_weave'),
         0, 2.0 * k * fs)
    return out


# ------------------------------------------------------------------------------------------------ bars (csrc/bars.hip)
def bar_profile(yuv, H, W, format='420', *, out=None):
    """How dark every row and column of every frame is, for letterbox / pillarbox detection (integers only), for all n
    frames in ONE kernel launch behind a clear of the table.  yuv: uint8 (n, >= yuv_frame_size(H, W, format)) on the GPU, as field_match
    takes it - stride(1) == 1, any row stride and base offset (`buf[:, 6:]` of a Y4MReader buffer), even ones above 8 bits.  Only luma
    is read, every sample once.  Returns int64 (n, H + W) on the device: [:, :H] the row sums P (row y: the sum of its W samples, as
    integers), [:, H:] the column sums Q.  Exact: a row does not depend on the batch it was computed in.  out: an int64 (n, H + W)
    contiguous tensor to write into instead.  What the sums mean is host arithmetic: edvr_amd/bars.py (B2 - B6).  Bytes booked: the
    luma plane of every frame once, and the table.  NotImplementedError for CPU tensors, ValueError for bad names, shapes and
    layouts."""
    fmt = yuv_format(format)
    require_gpu(yuv, dtypes=(torch.uint8,))
    H, W = int(H), int(W)
    sx, sy, depth, _ = fmt
    n, fs, stride = _yuv_batch(yuv, H, W, fmt, 'yuv')
    if out is None:
        out = torch.empty((n, H + W), dtype=torch.int64, device=yuv.device)
    else:
        require_gpu(out, dtypes=(torch.int64,))
        if tuple(out.shape) != (n, H + W) or not out.is_contiguous():
            raise ValueError(f'out is a contiguous int64 ({n}, {H + W}) tensor, got {tuple(out.shape)}')
        if _overlaps(out, yuv):
            raise ValueError('out overlaps the input')
    _run('bar_profile', lambda: _lib.check(_lib.lib().edvr_bar_profile(_ptr(yuv), _ptr(out), n, H, W, sx, sy, depth, stride, _stream()),
                                           'edvr_bar_profile'), 0, float(n) * (H * W * (2 if depth > 8 else 1) + 8 * (H + W)))
    return out


def yuv_crop(yuv, H, W, format='420', *, rect, out=None):
    """The rect (y0, x0, h, w) of every frame, all three planes, in ONE launch: luma [y0, y0 + h) x [x0, x0 + w) and
    the chroma rects (y0 >> sy, x0 >> sx, h >> sy, w >> sx), as frames of yuv_frame_size(h, w, format) bytes.  yuv: uint8 (n, >=
    yuv_frame_size(H, W, format)) on the GPU, as bar_profile takes it.  The rect lies inside the frame, on the chroma steps (rows in
    multiples of 1 << sy, columns of 1 << sx: chroma siting and field parity survive exactly) and is not empty.  Returns uint8
    (n, yuv_frame_size(h, w, format)).  out: a uint8 (n, >= that) batch to write into instead, stride(1) == 1, any row stride and base
    offset (`buf[:, 6:]`), even ones above 8 bits; bytes outside the frames are left alone; it must not overlap the input.  Bytes booked:
    every output byte read once and written once.  NotImplementedError for CPU tensors; ValueError for bad names, shapes and layouts,
    a rect outside the frame, off the chroma steps or empty, and an `out` that overlaps the input."""
    fmt = yuv_format(format)
    require_gpu(yuv, dtypes=(torch.uint8,))
    H, W = int(H), int(W)
    sx, sy, depth, _ = fmt
    n, fs, stride = _yuv_batch(yuv, H, W, fmt, 'yuv')
    y0, x0, h, w = check_rect(rect, H, W, (1 << sy, 1 << sx))
    if out is None:
        out = torch.empty((n, _yuv_frame_bytes(h, w, sx, sy, depth)), dtype=torch.uint8, device=yuv.device)
    else:
        require_gpu(out, dtypes=(torch.uint8,))
        if out.dim() == 2 and out.shape[0] != n:
            raise ValueError(f'out holds {out.shape[0]} frames, the input {n}')
    _, out_fs, out_stride = _yuv_batch(out, h, w, fmt, 'out')
    if _overlaps(out, yuv):
        raise ValueError('out overlaps the input')
    _run('yuv_crop', lambda: _lib.check(_lib.lib().edvr_yuv_crop(_ptr(yuv), _ptr(out), n, H, W, sx, sy, depth, stride, out_stride, y0, x0, h, w,
                                                                 _stream()), 'edvr_yuv_crop'), 0, 2.0 * n * out_fs)
    return out


# ------------------------------------------------------------------------------------------------ scene cuts
def frame_sad(frames, prev=None, out=None):
    """How much consecutive frames differ, for scene-cut detection (edvr_amd/shots.py), in ONE kernel launch.
    frames: uint8 (n, H, W, 3) or float32 (n, 3, H, W) RGB on the GPU - each frame dense, the frames any distance apart at any base
    address (a slice of a longer video works as it is).  Per pixel, in integers, Y8 = ((66 R + 129 G + 25 B + 128) >> 8) + 16 of the
    bytes - a float frame's are its tensor2img bytes rint(clamp(x, 0, 1) * 255), NaN -> 0, so a frame holding byte / 255 gives what the
    bytes give.  Returns int64 (n,) on the device: [j] = sum over the pixels of |Y8 of frame j - Y8 of frame j - 1|, [0] against `prev`
    (one frame of the same type and size, (H, W, 3) / (3, H, W) or with a leading 1: the last frame of the batch before) or 0 without
    one.  Exact (at most 219 H W), whatever the batching.  out: an int64 (n,) contiguous tensor to write into instead."""
    for t in (frames, prev, out):
        if t is not None and not t.is_cuda:
            raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    u8 = frames.dtype == torch.uint8
    if not u8 and frames.dtype != torch.float32:
        raise NotImplementedError(f'edvr_amd: {frames.dtype} frames are not supported here (float32 CHW in [0, 1] or uint8 HWC)')
    if frames.dim() != 4 or frames.shape[-1 if u8 else 1] != 3:
        raise ValueError(f'frames are uint8 (n, H, W, 3) or float32 (n, 3, H, W), got {frames.dtype} {tuple(frames.shape)}')
    n = frames.shape[0]
    H, W = (frames.shape[1], frames.shape[2]) if u8 else (frames.shape[2], frames.shape[3])
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f'frame_sad: no frames or empty frames, got {tuple(frames.shape)}')
    if not (frames[0].is_contiguous() and (n == 1 or frames.stride(0) >= 3 * H * W)):
        frames = frames.contiguous()
    if prev is not None:
        if prev.dim() == 4 and prev.shape[0] == 1:
            prev = prev[0]
        if prev.dtype != frames.dtype or tuple(prev.shape) != tuple(frames.shape[1:]):
            raise ValueError(f'prev is one frame like those of `frames` ({frames.dtype} {tuple(frames.shape[1:])}), got {prev.dtype} {tuple(prev.shape)}')
        prev = prev.contiguous()
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=frames.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (n,) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f'out is a contiguous int64 ({n},) tensor on the GPU, got {out.dtype} {tuple(out.shape)}')
    stride = frames.stride(0) if n > 1 else 3 * H * W
    name = 'edvr_frame_sad_rgb_u8' if u8 else 'edvr_frame_sad_rgb_f32'
    nbytes = float(n + (prev is not None)) * 3 * H * W * frames.element_size() + 8.0 * n  # each frame once
    _run('frame_sad', lambda: _lib.check(getattr(_lib.lib(), name)(_ptr(frames), _ptr(prev), _ptr(out), n, H, W, stride, _stream()), name), 0, nbytes)
    return out


# ------------------------------------------------------------------------------------------------ JPEG round trip (csrc/jpeg.hip)
JPEG_SUBSAMPLINGS = tuple(_lib.JPEG_SUBSAMPLINGS)


def jpeg_quality(quality, what='quality', allow_zero=False):
    """One host-side JPEG quality as an int: 1 .. 100 (0 = no compression where `allow_zero`); ValueError otherwise."""
    import operator
    try:
        q = operator.index(quality) if not isinstance(quality, bool) else None
    except TypeError:
        q = None
    if q is None:
        raise ValueError(f'{what} must be an int in 1 .. 100, got {quality!r}')
    if not (1 <= q <= 100 or (allow_zero and q == 0)):
        raise ValueError(f'{what} {q} is outside 1 .. 100')
    return q


def jpeg_roundtrip(frames, quality, subsampling='420', out=None):
    """What a baseline JPEG encoder followed by a decoder makes of a batch of frames, in ONE launch: libjpeg's integer
    pipeline - colour conversion, edge padding to the MCU, 2 x 2 chroma mean ('420'), 13-bit DCT, Annex K tables scaled by the quality
    and back - byte for byte what PIL's Image.save(format='JPEG', quality=q, subsampling=2 | 0) and Image.open(...).convert('RGB')
    return.  Entropy coding is lossless and is not performed.  frames: uint8 (n, H, W, 3) RGB on the GPU, 1 <= n <= 65535, each image
    dense, the images any distance apart (a slice of a longer batch works as it is) -> uint8 (n, H, W, 3).  quality: an int 1 .. 100 for
    every image, a sequence of n ints, or an int32 (n,) device tensor (which the kernel clamps to 0 .. 100); an entry 0 copies that
    image through unchanged.  subsampling: '420' (16 x 16 MCUs) or '444' (8 x 8).  out: a uint8 (n, H, W, 3) tensor of dense images to
    write into, which must not overlap `frames` (a workgroup reads pixels of its neighbours' tiles).  ValueError for bad qualities,
    names, layouts and an overlapping `out`; CPU tensors raise NotImplementedError: there is no fallback."""
    for t in (frames, out, quality if torch.is_tensor(quality) else None):
        if t is not None and not t.is_cuda:
            raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if subsampling not in _lib.JPEG_SUBSAMPLINGS:
        raise ValueError(f'subsampling must be one of {JPEG_SUBSAMPLINGS}, got {subsampling!r}')
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f'frames are uint8 (n, H, W, 3), got {frames.dtype} {tuple(frames.shape)}')
    n, H, W, _ = frames.shape
    if not 0 < n <= 65535 or H < 1 or W < 1:
        raise ValueError(f'jpeg_roundtrip takes 1..65535 non-empty frames per call, got {tuple(frames.shape)}')

    def dense(t):
        return t[0].is_contiguous() and (n == 1 or t.stride(0) >= 3 * H * W)
    if not dense(frames):
        frames = frames.contiguous()
    table, q_all = None, 0
    if torch.is_tensor(quality):
        if quality.dtype != torch.int32 or tuple(quality.shape) != (n,):
            raise ValueError(f'a quality table is an int32 ({n},) device tensor, got {quality.dtype} {tuple(quality.shape)}')
        table = quality.contiguous()
    elif isinstance(quality, (list, tuple)):
        if len(quality) != n:
            raise ValueError(f'{len(quality)} qualities for {n} frames')
        table = torch.tensor([jpeg_quality(q, allow_zero=True) for q in quality], dtype=torch.int32).to(frames.device, non_blocking=True)
    else:
        q_all = jpeg_quality(quality, allow_zero=True)
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=frames.device)
    else:
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not dense(out):
            raise ValueError(f'out is a uint8 {(n, H, W, 3)} tensor of dense images, got {out.dtype} {tuple(out.shape)}')
        (a0, a1), (b0, b1) = _byte_span(frames), _byte_span(out)
        if a0 < b1 and b0 < a1:
            raise ValueError('out overlaps the input')
    stride = lambda t: t.stride(0) if n > 1 else 3 * H * W
    nbytes = 6.0 * n * H * W + (4.0 * n if table is not None else 0.0)  # each pixel read and written once, plus the table
    _run('jpeg_roundtrip', lambda: _lib.check(_lib.lib().edvr_jpeg_roundtrip_u8(_ptr(frames), _ptr(out), _ptr(table), q_all, n, H, W, stride(frames),
                                                                                 stride(out), _lib.JPEG_SUBSAMPLINGS[subsampling], _stream()),
                                              'edvr_jpeg_roundtrip_u8'), 0, nbytes)
    return out


# ------------------------------------------------------------------------------------------------ MPEG-style round trip (csrc/mpeg.hip)
MPEG_MAX_QSCALE, MPEG_MAX_SEARCH = 31, 15


def _mpeg_int(v, lo, hi, what):
    import operator
    try:
        i = operator.index(v) if not isinstance(v, bool) else None
    except TypeError:
        i = None
    if i is None:
        raise ValueError(f'{what} must be an int in {lo} .. {hi}, got {v!r}')
    if not lo <= i <= hi:
        raise ValueError(f'{what} {i} is outside {lo} .. {hi}')
    return i


def mpeg_qscale(qscale, what='qscale', allow_zero=False):
    """One host-side quantiser scale as an int: 1 .. 31 (0 = no compression where `allow_zero`); ValueError otherwise."""
    return _mpeg_int(qscale, 0 if allow_zero else 1, MPEG_MAX_QSCALE, what)


def mpeg_gop(gop, what='gop'):
    """The distance between intra frames as an int: positive, or 0 for frame 0 alone; ValueError otherwise."""
    return _mpeg_int(gop, 0, 1 << 30, what)


def mpeg_search(search, what='search'):
    """The motion search range R as an int: 0 .. 15; ValueError otherwise."""
    return _mpeg_int(search, 0, MPEG_MAX_SEARCH, what)


def mpeg_roundtrip(frames, qscale, gop=12, search=7, out=None):
    """What an MPEG-2 / MPEG-4-SP shaped I / P video encoder followed by a decoder makes of clips of frames, in t + 2 launches (DESIGN
    4.18, M1 - M7): 4:2:0 planes, frame i intra (the MPEG-2 default matrix scaled by qscale) if i == 0 or gop > 0 and i % gop == 0, else
    predicted from the reconstruction of frame i - 1 by a full search over [-search, search]^2 per 16 x 16 macroblock, with a half-sample
    chroma vector and a flat dead-zone quantiser on the residual.  All integers; entropy coding is not performed and no stream
    compatibility is claimed.  frames: uint8 (b, t, H, W, 3), or (t, H, W, 3) for one clip, RGB in display order on the GPU, b t <= 65535,
    H, W <= 16384, each frame dense, frames at least a frame and clips at least a clip apart (any other view is gathered first) -> the same shape.  qscale: an int 1 .. 31 for every clip, a
    sequence of b ints, or an int32 (b,) device tensor (which the kernels clamp to 0 .. 31); an entry 0 copies that clip through unchanged.
    out: a uint8 tensor of the same shape under the same layout rule (no two frames share a byte), which must not overlap `frames`.  ValueError for values out of range, wrong
    dtypes or shapes and an overlapping `out`; CPU tensors raise NotImplementedError: there is no fallback."""
    for t_ in (frames, out, qscale if torch.is_tensor(qscale) else None):
        if t_ is not None and not t_.is_cuda:
            raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    gop, search = mpeg_gop(gop), mpeg_search(search)
    if frames.dtype != torch.uint8 or frames.dim() not in (4, 5) or frames.shape[-1] != 3:
        raise ValueError(f'frames are uint8 (b, t, H, W, 3) or (t, H, W, 3), got {frames.dtype} {tuple(frames.shape)}')
    one = frames.dim() == 4
    if one:
        frames = frames[None]
        if out is not None and out.dim() == 4:
            out = out[None]
    b, t, H, W, _ = frames.shape
    if b < 1 or t < 1 or b * t > 65535 or not 1 <= H <= 16384 or not 1 <= W <= 16384:
        raise ValueError(f'mpeg_roundtrip takes 1..65535 non-empty frames of at most 16384 x 16384 per call, got {tuple(frames.shape)}')
    fb = 3 * H * W

    def dense(x):
        fs_ = x.stride(1) if t > 1 else fb  # no two frames share a byte: a frame stride of at least a frame, a clip stride of at least a clip
        return x[0, 0].is_contiguous() and fs_ >= fb and (b == 1 or x.stride(0) >= (t - 1) * fs_ + fb)
    if not dense(frames):
        frames = frames.contiguous()
    table, q_all = None, 0
    if torch.is_tensor(qscale):
        if qscale.dtype != torch.int32 or tuple(qscale.shape) != (b,):
            raise ValueError(f'a qscale table is an int32 ({b},) device tensor, got {qscale.dtype} {tuple(qscale.shape)}')
        table = qscale.contiguous()
    elif isinstance(qscale, (list, tuple)):
        if len(qscale) != b:
            raise ValueError(f'{len(qscale)} qscales for {b} clips')
        table = torch.tensor([mpeg_qscale(q, allow_zero=True) for q in qscale], dtype=torch.int32).to(frames.device, non_blocking=True)
    else:
        q_all = mpeg_qscale(qscale, allow_zero=True)
    if out is None:
        out = torch.empty((b, t, H, W, 3), dtype=torch.uint8, device=frames.device)
    else:
        if out.dtype != torch.uint8 or tuple(out.shape) != (b, t, H, W, 3) or not dense(out):
            raise ValueError(f'out is a uint8 {(b, t, H, W, 3)} tensor of dense frames, got {out.dtype} {tuple(out.shape)}')
        (a0, a1), (b0, b1) = _byte_span(frames), _byte_span(out)
        if a0 < b1 and b0 < a1:
            raise ValueError('out overlaps the input')
    nbytes = int(_lib.lib().edvr_mpeg_roundtrip_workspace(b, t, H, W))
    ws = workspace(nbytes, frames.device)
    fs = lambda x: x.stride(1) if t > 1 else fb
    cs = lambda x: x.stride(0) if b > 1 else t * fs(x)
    booked = 6.0 * b * t * H * W + 2.0 * nbytes + (4.0 * b if table is not None else 0.0)  # pixels in and out, the planes written and read
    _run('mpeg_roundtrip', lambda: _lib.check(_lib.lib().edvr_mpeg_roundtrip_u8(_ptr(frames), _ptr(out), _ptr(table), q_all, b, t, H, W, cs(frames), fs(frames),
                                                                                 cs(out), fs(out), gop, search, _ptr(ws), nbytes, _stream()),
                                              'edvr_mpeg_roundtrip_u8'), 0, booked)
    return out[0] if one else out


# ------------------------------------------------------------------------------------------------ blur and noise (csrc/degrade.hip)
DEGRADE_TILE, DEGRADE_MAX_KSIZE, DEGRADE_RECORD_INTS = _lib.DEGRADE_TILE, _lib.DEGRADE_MAX_KSIZE, _lib.DEGRADE_RECORD_INTS
DEGRADE_ONE = 1 << 20  # what the Q20 weights of a blur kernel sum to


def degrade_ksize(ksize, what='ksize'):
    """One blur kernel size as an int: odd, 3 .. 21; ValueError otherwise."""
    import operator
    try:
        k = operator.index(ksize) if not isinstance(ksize, bool) else None
    except TypeError:
        k = None
    if k is None:
        raise ValueError(f'{what} must be an odd int in 3 .. {DEGRADE_MAX_KSIZE}, got {ksize!r}')
    if not 3 <= k <= DEGRADE_MAX_KSIZE or k % 2 == 0:
        raise ValueError(f'{what} {k} is not an odd size in 3 .. {DEGRADE_MAX_KSIZE}')
    return k


def degrade_blur(kernel, H=None, W=None):
    """One blur kernel of ops.degrade as a contiguous int32 (k, k) NumPy array: k odd in 3 .. 21, every weight in 0 .. 2^20, the sum exactly
    2^20 (data.gaussian_blur_kernel makes such kernels), and - given the frame - H, W > k // 2, so that one reflection covers the ring.
    ValueError otherwise."""
    import numpy as np
    k = kernel.cpu().numpy() if torch.is_tensor(kernel) else np.asarray(kernel)
    if k.dtype != np.int32 or k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise ValueError(f'a blur kernel is an int32 (k, k) array of Q20 weights, got {k.dtype} {k.shape}')
    degrade_ksize(k.shape[0], 'the blur kernel: ksize')
    if int(k.min()) < 0 or int(k.sum(dtype=np.int64)) != DEGRADE_ONE:
        raise ValueError(f'the weights of a blur kernel are >= 0 and sum to 1 << 20, got a minimum of {int(k.min())} and a sum of {int(k.sum(dtype=np.int64))}')
    if H is not None and min(H, W) <= k.shape[0] // 2:
        raise ValueError(f'a {H} x {W} frame is not larger than the radius {k.shape[0] // 2} of its blur kernel: one reflection must cover the ring')
    return np.ascontiguousarray(k)


def degrade_noise(noise):
    """One noise setting (read_sigma, shot, gray) of ops.degrade with both numbers as float32 values: read_sigma >= 0 in levels of 0 .. 255,
    shot >= 0 the variance per level; ValueError for anything negative, NaN or infinite (as float32).  None is (0, 0, False): no noise."""
    import numpy as np
    if noise is None:
        return 0.0, 0.0, False
    try:
        read, shot, gray = noise
        with np.errstate(over='ignore'):
            read, shot = float(np.float32(read)), float(np.float32(shot))
    except (TypeError, ValueError):
        raise ValueError(f'noise is (read_sigma, shot, gray), got {noise!r}') from None
    if not (0 <= read < float('inf') and 0 <= shot < float('inf')):
        raise ValueError(f'noise: read_sigma and shot are finite numbers >= 0, got {noise!r}')
    return read + 0.0, shot + 0.0, bool(gray)


def degrade_record(ksize, weight_offset, read_sigma, shot, gray, key, ctr_t):
    """The eight int32 words of one image's record (include/edvr_amd.h: edvr_degrade_u8), from checked values."""
    import struct
    bits = lambda f: struct.unpack('<i', struct.pack('<f', f))[0]
    s32 = lambda u: (u & 0xffffffff) - ((u & 0x80000000) << 1)
    return [ksize, weight_offset, bits(read_sigma), bits(shot), int(bool(gray)), s32(key), s32(key >> 32), s32(ctr_t)]


def degrade_table(n, H, W, blur=None, noise=None, seed=0, frame_index=None):
    """The host side of ops.degrade: (table int32 (n, 8), weights int32 (m,) or None) as NumPy arrays, every argument checked (ValueError)
    - one record per image, the distinct blur kernels once each in `weights`.  Arguments as ops.degrade takes them."""
    import numpy as np
    import operator

    def per_image(v, single, what):
        if single(v):
            return [v] * n
        v = list(v)
        if len(v) != n:
            raise ValueError(f'{len(v)} {what} for {n} frames')
        return v
    blurs = per_image(blur, lambda v: v is None or ((torch.is_tensor(v) or isinstance(v, np.ndarray)) and v.ndim == 2), 'blur kernels')
    noises = per_image(noise, lambda v: v is None or (isinstance(v, (tuple, list)) and len(v) == 3 and not any(e is None or isinstance(e, (tuple, list)) for e in v)), 'noise settings')
    try:
        seeds = [operator.index(s) for s in per_image(seed, lambda v: not isinstance(v, (tuple, list, np.ndarray)) and not torch.is_tensor(v), 'seeds')]
        frame_index = list(range(n)) if frame_index is None else [operator.index(t) for t in per_image(frame_index, lambda v: False, 'frame indices')]
    except TypeError:
        raise ValueError('seed and frame_index are ints') from None
    if any(not -(1 << 63) <= s < 1 << 64 for s in seeds) or any(not 0 <= t < 1 << 32 for t in frame_index):
        raise ValueError('a seed is a 64-bit key, a frame index lies in 0 .. 2^32 - 1')
    table, parts, where, offset = np.zeros((n, DEGRADE_RECORD_INTS), np.int32), [], {}, 0
    for i in range(n):
        ksize = off = 0
        if blurs[i] is not None:
            if id(blurs[i]) not in where:
                k = degrade_blur(blurs[i], H, W)
                where[id(blurs[i])] = (k.shape[0], offset)
                parts.append(k.ravel())
                offset += k.size
            ksize, off = where[id(blurs[i])]
        table[i] = degrade_record(ksize, off, *degrade_noise(noises[i]), seeds[i], frame_index[i])
    return table, (np.concatenate(parts) if parts else None)


def check_degrade_table(table_host, n_weights, H, W, weights_host=None):
    """What a launch of ops.degrade's table form checks on the host copy of its table (int32 (n, 8) NumPy array or CPU tensor): every
    ksize, that the frame is larger than its radius, that the weights lie inside the buffer of n_weights words, the noise numbers - and,
    given the host copy of the weights, their range and sum.  ValueError otherwise."""
    import numpy as np
    t = table_host.numpy() if torch.is_tensor(table_host) else np.asarray(table_host)
    if t.dtype != np.int32 or t.ndim != 2 or t.shape[1] != DEGRADE_RECORD_INTS:
        raise ValueError(f'table_host is the table as an int32 (n, {DEGRADE_RECORD_INTS}) host array')
    w = None if weights_host is None else (weights_host.numpy() if torch.is_tensor(weights_host) else np.asarray(weights_host))
    for i, (ksize, off) in enumerate(t[:, :2].tolist()):
        if ksize == 0:
            continue
        degrade_ksize(ksize, f'record {i}: ksize')
        if min(H, W) <= ksize // 2:
            raise ValueError(f'record {i}: a {H} x {W} frame is not larger than the radius {ksize // 2} of its blur kernel')
        if off < 0 or off + ksize * ksize > n_weights:
            raise ValueError(f'record {i}: weights {off} .. {off + ksize * ksize} leave the buffer of {n_weights}')
        if w is not None:
            degrade_blur(w[off:off + ksize * ksize].reshape(ksize, ksize))
    f = np.ascontiguousarray(t[:, 2:4]).view(np.float32)
    if not np.all(np.isfinite(f)) or np.any(np.signbit(f)):
        raise ValueError('a record has a negative, NaN or infinite read sigma or shot')


def degrade(frames, blur=None, noise=None, seed=0, frame_index=None, out=None, table=None, weights=None, table_host=None, weights_host=None):
    """Blur, then noise, on a batch of frames in ONE launch: the two steps of the first-order degradation model that come
    before compression (jpeg_roundtrip).  frames: uint8 (n, H, W, 3) RGB on the GPU, 1 <= n <= 65535, each image dense, the images any
    distance apart -> uint8 (n, H, W, 3).
    blur: an int32 (k, k) kernel of Q20 weights (data.gaussian_blur_kernel; k odd in 3 .. 21, weights >= 0 that sum to 1 << 20) for every
    image, or a sequence of n kernels / None (no blur).  The sum runs over the frame extended by the reflection that does not repeat the
    edge sample and is exact: (acc + 2^19) >> 20 where there is no noise.
    noise: (read_sigma, shot, gray) for every image or a sequence of n such tuples / None: Gaussian noise of standard deviation
    sqrt(shot v + read_sigma^2) levels at a blurred value v, independent per channel or - gray - one draw for the three.
    seed: one 64-bit key or n keys; frame_index: the third word of the Philox counter per image, default range(n) - a frame's noise
    field is a function of (key, frame_index, x, y) alone.
    The second form, degrade(frames, table=, weights=), takes the records and the weight buffer as int32 DEVICE tensors ((n, 8) and (m,);
    degrade_table makes them on the host) and copies nothing: capturable in a graph.  table_host / weights_host: their host copies,
    which are then checked before the launch; without them the caller vouches for the records.
    out: a uint8 (n, H, W, 3) tensor of dense images to write into, which must not overlap `frames`.  ValueError for bad kernels, noise
    numbers, layouts and an overlapping `out`; CPU tensors raise NotImplementedError: there is no fallback."""
    for t in (frames, out, table, weights):
        if t is not None and not t.is_cuda:
            raise NotImplementedError('edvr_amd ops run on the GPU only (HIP/gfx950); got a CPU tensor')
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f'frames are uint8 (n, H, W, 3), got {frames.dtype} {tuple(frames.shape)}')
    n, H, W, _ = frames.shape
    if not 0 < n <= 65535 or H < 1 or W < 1:
        raise ValueError(f'degrade takes 1..65535 non-empty frames per call, got {tuple(frames.shape)}')

    def dense(t):
        return t[0].is_contiguous() and (n == 1 or t.stride(0) >= 3 * H * W)
    if not dense(frames):
        frames = frames.contiguous()
    if table is None:
        if weights is not None:
            raise ValueError('weights go with a table')
        table_np, weights_np = degrade_table(n, H, W, blur, noise, seed, frame_index)
        table = torch.from_numpy(table_np).to(frames.device, non_blocking=True)
        weights = None if weights_np is None else torch.from_numpy(weights_np).to(frames.device, non_blocking=True)
    else:
        if blur is not None or noise is not None or frame_index is not None:
            raise ValueError('a table holds the blur, the noise and the frame indices: give one or the other')
        if table.dtype != torch.int32 or tuple(table.shape) != (n, DEGRADE_RECORD_INTS) or not table.is_contiguous():
            raise ValueError(f'a table is a contiguous int32 ({n}, {DEGRADE_RECORD_INTS}) device tensor, got {table.dtype} {tuple(table.shape)}')
        if weights is not None and (weights.dtype != torch.int32 or weights.dim() != 1 or not weights.is_contiguous()):
            raise ValueError(f'weights are a contiguous int32 (m,) device tensor, got {weights.dtype} {tuple(weights.shape)}')
        if table_host is not None:
            check_degrade_table(table_host, 0 if weights is None else weights.numel(), H, W, weights_host)
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=frames.device)
    else:
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not dense(out):
            raise ValueError(f'out is a uint8 {(n, H, W, 3)} tensor of dense images, got {out.dtype} {tuple(out.shape)}')
        (a0, a1), (b0, b1) = _byte_span(frames), _byte_span(out)
        if a0 < b1 and b0 < a1:
            raise ValueError('out overlaps the input')
    stride = lambda t: t.stride(0) if n > 1 else 3 * H * W
    nbytes = 6.0 * n * H * W + 4.0 * table.numel() + (4.0 * weights.numel() if weights is not None else 0.0)  # pixels in and out, table, weights
    _run('degrade', lambda: _lib.check(_lib.lib().edvr_degrade_u8(_ptr(frames), _ptr(out), _ptr(table), _ptr(weights), n, H, W, stride(frames), stride(out),
                                                                  _stream()), 'edvr_degrade_u8'), 0, nbytes)
    return out


def philox_words(key, ctr_t, H, W, device='cuda'):
    """The generator of ops.degrade on its own: int32 (H, W, 4) on the GPU holding the BIT PATTERNS of the four uint32 words of
    Philox4x32-10 (Random123) at counter (x, y, ctr_t, 0) and the 64-bit key `key` (low word first) - .view(numpy.uint32) on the host gives
    the words.  ValueError for a key, ctr_t or size out of range."""
    import operator
    key, ctr_t, H, W = (operator.index(v) for v in (key, ctr_t, H, W))
    if not -(1 << 63) <= key < 1 << 64 or not 0 <= ctr_t < 1 << 32 or H < 1 or W < 1 or H * W > 1 << 29:
        raise ValueError(f'philox_words: key {key}, ctr_t {ctr_t} or size {H} x {W} out of range')
    out = torch.empty((H, W, 4), dtype=torch.int32, device=device)
    _run('philox_words', lambda: _lib.check(_lib.lib().edvr_philox_words_u32(_ptr(out), key & 0xffffffff, (key >> 32) & 0xffffffff, ctr_t, H, W, _stream()),
                                            'edvr_philox_words_u32'), 0, 16.0 * H * W)
    return out
