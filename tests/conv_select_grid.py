"""The descriptor grid of test_conv_select_cpu.py and its evaluation.  No GPU: the queries are host code and nothing is dereferenced.

    python tests/conv_select_grid.py            prints {"outcomes": [...], "index": [...], "kernels": [...]} as one JSON line
    python tests/conv_select_grid.py --record   rewrites conv_select_fixture.json from the library in the tree

Run in a fresh interpreter without the EDVR_* switches (CLEAN_ENV): the C side reads them once into statics.
"""
import base64
import ctypes
import itertools
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'conv_select_fixture.json')
CLEAN_ENV = ('EDVR_CONV_WINOGRAD', 'EDVR_WINOGRAD_F4', 'EDVR_WINOGRAD_F4S', 'EDVR_CONV1X1_STREAM', 'EDVR_CONV1X1_SPLIT', 'EDVR_F4S_LEAN')

SHAPES = [(2, 64, 0, 16, 64), (1, 3, 0, 20, 36), (1, 64, 64, 8, 32), (2, 16, 0, 12, 20), (1, 320, 0, 8, 16), (1, 128, 192, 8, 16),
          (1, 6, 2, 9, 33), (1, 64, 0, 16, 30)]  # (n, c1, c2, h, w)
COS = [3, 4, 32, 64, 130]
KS_STRIDE = [(3, 1), (3, 2), (1, 1)]
ALGOS = [0, 1, 2, 3, 4]  # EDVR_CONV_AUTO, _DIRECT, _WINOGRAD, _WINOGRAD_F4, _WINOGRAD_F4S
PACKINGS = ['none', 'f4', 'f4s', 'ds', 'all']  # f4s / ds / all come with x_amax
EPILOGUES = ['none', 'res1', 'res1+res2', 'gate', 'pre', 'y_scale', 'sigmoid']
OUT_MODES = [0, 1]  # EDVR_OUT_NCHW, EDVR_OUT_PIXEL_SHUFFLE2
FIELDS = ('name', 'flops', 'abs_sum_supported', 'pre_supported', 'y_amax_supported', 'gate_supported', 'lean_items')
PTR = 4096  # a 16-byte aligned address


def rows():
    return list(itertools.product(SHAPES, COS, KS_STRIDE, ALGOS, PACKINGS, EPILOGUES, OUT_MODES))


def describe(row):
    (n, c1, c2, h, w), co, (ks, stride), algo, packing, epilogue, out_mode = row
    return f'n={n} c1={c1} c2={c2} h={h} w={w} co={co} ks={ks} stride={stride} algo={algo} packing={packing} epilogue={epilogue} out_mode={out_mode}'


def desc(row):
    from edvr_amd import _lib
    (n, c1, c2, h, w), co, (ks, stride), algo, packing, epilogue, out_mode = row
    pad = ks // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    d = _lib.ConvDesc()
    d.n, d.c1, d.c2, d.h, d.w, d.co, d.ks, d.stride, d.algo, d.out_mode = n, c1, c2, h, w, co, ks, stride, algo, out_mode
    d.x1, d.wpk, d.y = PTR, PTR, PTR
    d.x1_img_stride, d.y_img_stride = c1 * h * w, co * ho * wo
    if c2 > 0:
        d.x2, d.x2_img_stride = PTR, c2 * h * w
    if packing in ('f4', 'all'):
        d.wpk_f4 = PTR
    if packing in ('f4s', 'all'):
        d.wpk_f4s = PTR
    if packing in ('ds', 'all'):
        d.wpk_ds = PTR
    if packing in ('f4s', 'ds', 'all'):
        d.x_amax = PTR
    if epilogue in ('res1', 'res1+res2'):
        d.res1, d.res1_img_stride = PTR, co * ho * wo
    if epilogue == 'res1+res2':
        d.res2, d.res2_img_stride = PTR, co * ho * wo
    if epilogue == 'gate':
        d.gate, d.gate_img_stride, d.gate_slope = PTR, co * ho * wo, 0.1
    if epilogue == 'pre':
        d.pre, d.pre_img_stride, d.pre_n = PTR, co * ho * wo, n
    if epilogue == 'y_scale':
        d.y_scale = 0.2
    if epilogue == 'sigmoid':
        d.act = _lib.ACT_SIGMOID
    return d


def evaluate(with_kernel=True):
    """-> (distinct outcome tuples in FIELDS order, one index into them per grid row, edvr_conv2d_kernel per grid row)"""
    sys.path.insert(0, os.path.dirname(HERE))
    from edvr_amd import _lib
    L = _lib.lib()
    buf, ex = ctypes.create_string_buffer(96), ctypes.c_double(0.0)
    outcomes, index, kernels = {}, [], []
    for row in rows():
        d = desc(row)
        p = ctypes.byref(d)
        assert L.edvr_conv2d_kernel_name(p, buf, 96) == 0 and L.edvr_conv2d_executed_flops(p, ctypes.byref(ex)) == 0, describe(row)
        out = (buf.value.decode(), ex.value, L.edvr_conv2d_abs_sum_supported(p), L.edvr_conv2d_pre_supported(p),
               L.edvr_conv2d_y_amax_supported(p), L.edvr_conv2d_gate_supported(p), L.edvr_conv2d_f4s_lean_items(p))
        index.append(outcomes.setdefault(out, len(outcomes)))
        if with_kernel:
            kernels.append(L.edvr_conv2d_kernel(p))
    return [list(o) for o in outcomes], index, kernels


def load_fixture():
    """-> (outcomes, index): the index is stored as base64(zlib(little-endian uint16 per grid row))"""
    fx = json.load(open(FIXTURE))
    raw = zlib.decompress(base64.b64decode(fx['index_u16le_zlib_b64']))
    return fx['outcomes'], [int.from_bytes(raw[i:i + 2], 'little') for i in range(0, len(raw), 2)]


def record():
    outcomes, index, _ = evaluate(with_kernel=False)
    raw = b''.join(i.to_bytes(2, 'little') for i in index)
    with open(FIXTURE, 'w') as f:
        json.dump({'fields': FIELDS, 'rows': len(index), 'index_u16le_zlib_b64': base64.b64encode(zlib.compress(raw, 9)).decode(),
                   'outcomes': outcomes}, f, indent=0)
        f.write('\n')
    print(f'{len(index)} rows, {len(outcomes)} distinct outcomes -> {FIXTURE}')


if __name__ == '__main__':
    if '--record' in sys.argv:
        record()
    else:
        outcomes, index, kernels = evaluate()
        print(json.dumps({'outcomes': outcomes, 'index': index, 'kernels': kernels}))
