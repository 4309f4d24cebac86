"""No GPU: which kernel takes a conv2d descriptor, and what every query says about it (csrc/conv2d.hip: conv2d_select and its table).

conv_select_fixture.json holds, for the 42 000 descriptors of conv_select_grid.py, what edvr_conv2d_kernel_name, _executed_flops, the
four _supported queries and _f4s_lean_items answered BEFORE the selection moved into one function, recorded from the library as it was.
One rule of it was corrected afterwards, the label fault the move fixed: a descriptor the small-co kernel would take (3x3 / stride 1,
co <= 4, EDVR_CONV_AUTO, NCHW) that carries a gate or a y_scale runs on conv2d_mfma_kernel<3, 1, 1, ..> - the small-co kernel has
neither epilogue - and is now named so; it used to be reported as conv3x3_smallco_kernel.  Only the name of those rows changed.
"""
import json
import os
import subprocess
import sys

import pytest

import conv_select_grid as G

# EDVR_CONV_KERNEL_* -> (kernel name, has y_amax, has abs_sum, has pre): the table beside conv2d_select
KERNELS = [
    ('conv3x3_smallco_kernel', 0, 0, 0),
    ('conv3x3_winograd_f4s_kernel', 1, 1, 1),
    ('conv3x3_winograd_f4_kernel', 0, 1, 1),
    ('conv3x3_winograd_kernel', 0, 0, 0),
    ('conv1x1_split_kernel', 1, 0, 0),
    ('conv1x1_stream_kernel', 0, 0, 0),
    ('conv2d_split_kernel', 1, 0, 0),
    ('conv2d_mfma_kernel', 0, 0, 0),
]


@pytest.fixture(scope='module')
def evaluated():
    """The grid in a fresh interpreter without the EDVR_* switches: the C side reads them once into statics."""
    env = {k: v for k, v in os.environ.items() if k not in G.CLEAN_ENV}
    r = subprocess.run([sys.executable, os.path.join(G.HERE, 'conv_select_grid.py')], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_every_query_answers_as_recorded(evaluated):
    want_outcomes, want_index = G.load_fixture()
    rows = G.rows()
    assert len(rows) == len(want_index) == len(evaluated['index']) == 42000
    for row, w, g in zip(rows, want_index, evaluated['index']):
        want, got = want_outcomes[w], evaluated['outcomes'][g]
        assert got == want, f'{G.describe(row)}: {dict(zip(G.FIELDS, got))}, recorded {dict(zip(G.FIELDS, want))}'
    names = {o[0].split('<')[0] for o in want_outcomes}
    assert names == {k[0] for k in KERNELS}  # the grid reaches all eight kernels


def test_the_kernel_export_agrees_with_the_name_and_the_table(evaluated):
    for row, g, kernel in zip(G.rows(), evaluated['index'], evaluated['kernels']):
        out = dict(zip(G.FIELDS, evaluated['outcomes'][g]))
        (n, c1, c2, h, w), co, (ks, stride), algo, packing, epilogue, out_mode = row
        name, y_amax, abs_sum, pre = KERNELS[kernel]
        what = f'{G.describe(row)}: kernel {kernel}, {out}'
        direct = name in ('conv2d_split_kernel', 'conv2d_mfma_kernel')  # (these print their template arguments)
        assert out['name'].startswith(name + f'<{ks}, {stride}, ') if direct else out['name'] == name, what
        assert out['y_amax_supported'] == y_amax, what
        assert out['abs_sum_supported'] == (abs_sum and out_mode == 0), what  # (the PixelShuffle store has no such sum)
        # `pre` rides in the registers of the gate / residuals of the NCHW epilogue
        assert out['pre_supported'] == (pre and out_mode == 0 and epilogue not in ('gate', 'res1', 'res1+res2')), what
        assert (out['lean_items'] > 0) <= (kernel == 1), what
