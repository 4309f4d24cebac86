"""CPU: the definition of NIQE this package computes - the NumPy restatement of the device part (tests/util_niqe.py) finished by
metrics.niqe_from_moments - against the reference's calculate_niqe recorded in tests/golden/niqe.pt (scripts/make_niqe_golden.py); the
block order, the NaN rules, the parameter file, and the --niqe options of scripts/restore_video.py and scripts/eval_video.py.

Tolerance: the fixture's `tol` = 4 x max |ref - ref64| over its frames, the reference's own float32 noise."""
import argparse
import importlib.util
import io
import json
import os

import numpy as np
import pytest
import torch

import util_niqe as N
from util_data import write_video_test_tree

PARAMS = os.path.join(N.GOLDEN, 'niqe_pris_params.npz')
ALPHAS = [a + 18 * s for s in (0, 1) for a in (0, 2, 6, 10, 14)]  # where the 36 features hold a grid value
_CACHE = {}


def _data():
    if not _CACHE:
        from edvr_amd import metrics
        d = N.load_cases()
        _CACHE.update(tol=d['tol'], cases={c['name']: c for c in d['cases']}, params=metrics.load_niqe_params(PARAMS), restated={})
    return _CACHE


def _restated(name):
    d = _data()
    if name not in d['restated']:
        c = d['cases'][name]
        per_frame = [N.moments(img, c['crop_border']) for img in c['img'].numpy()]
        d['restated'][name] = (np.stack([m for m, _, _ in per_frame]), per_frame[0][1], per_frame[0][2])
    return d['restated'][name]


NAMES = ['noise', 'smooth', 'cropped', 'grey']


def test_fixture_is_what_the_issue_describes():
    d = _data()
    shapes = {k: (tuple(c['img'].shape), c['crop_border']) for k, c in d['cases'].items()}
    assert shapes == {'noise': ((2, 96, 192, 3), 0), 'smooth': ((1, 192, 288, 3), 0), 'cropped': ((1, 203, 301, 3), 4), 'grey': ((1, 96, 192), 0)}
    assert torch.equal(d['cases']['grey']['img'][0], d['cases']['noise']['img'][0, :, :, 0])
    worst = max(abs(a - b) for c in d['cases'].values() for a, b in zip(c['ref'], c['ref64']))
    assert d['tol'] == 4 * worst and 0 < d['tol'] < 1e-4  # the reference's float32 noise on values of 14 .. 75
    assert all(c['img'].dtype == torch.uint8 and np.isfinite(c['ref']).all() for c in d['cases'].values())


@pytest.mark.parametrize('name', NAMES)
def test_restatement_matches_the_reference(name):
    from edvr_amd import metrics
    d = _data()
    m, nbh, nbw = _restated(name)
    got = metrics.niqe_from_moments(m, nbh, nbw, d['params'])
    ref = d['cases'][name]['ref']
    err = [abs(g - r) for g, r in zip(got, ref)]
    print(f'{name}: {got} ref {ref} |d| {err} tol {d["tol"]:.3e}')
    assert len(got) == len(ref) and max(err) <= d['tol']
    assert metrics.niqe_from_moments(torch.from_numpy(m), nbh, nbw, d['params']) == got  # a tensor or an array


@pytest.mark.parametrize('name', NAMES)
def test_feature_table_matches_the_reference(name):
    from edvr_amd import metrics
    m, nbh, nbw = _restated(name)
    got, ref = metrics.niqe_features(m), _data()['cases'][name]['feat'].numpy()
    assert got.shape == ref.shape == (m.shape[0], nbh * nbw, 36)
    others = [k for k in range(36) if k not in ALPHAS]
    assert np.abs(got[..., ALPHAS] - ref[..., ALPHAS]).max() <= 0.001 + 1e-12  # one step of the arange(0.2, 10.001, 0.001) grid
    assert (np.abs(got[..., others] - ref[..., others]) / np.abs(ref[..., others])).max() <= 1e-4


def test_block_order_is_column_major():
    """2 x 3 blocks: row k of the table is block (k % 2, k // 2), the reference's idx_w-outer loop - not the row-major order."""
    from edvr_amd import metrics
    m, nbh, nbw = _restated('smooth')
    assert (nbh, nbw) == (2, 3)
    ref = _data()['cases']['smooth']['feat'].numpy()[0]
    x = N.kept(N.y_plane(_data()['cases']['smooth']['img'][0].numpy()))[0]
    z = N.mscn(x)
    for k, (ih, iw) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]):
        one = N.block_moments(z[ih * 96:(ih + 1) * 96, iw * 96:(iw + 1) * 96])
        assert np.array_equal(one, m[0, 0, k])
    got = metrics.niqe_features(m)[0]
    row_major = got.reshape(3, 2, 36).transpose(1, 0, 2).reshape(6, 36)
    assert np.abs(got[:, 1] - ref[:, 1]).max() < 1e-4 * np.abs(ref[:, 1]).max() < np.abs(row_major[:, 1] - ref[:, 1]).max()


def _flattened(img, ih, iw, margin=8):
    """Block (ih, iw) and `margin` pixels around it set to one grey level: every 7 x 7 neighbourhood of the block is constant at both scales."""
    img = img.copy()
    img[max(ih * 96 - margin, 0):(ih + 1) * 96 + margin, max(iw * 96 - margin, 0):(iw + 1) * 96 + margin] = 128
    return img


def test_constant_block_is_a_nan_row_dropped_from_the_covariance():
    from edvr_amd import metrics
    d = _data()
    img = _flattened(d['cases']['smooth']['img'][0].numpy(), 1, 1)
    m, nbh, nbw = N.moments(img)
    k = 1 * nbh + 1  # block (1, 1)
    assert not m[:, k].any()  # z == 0 exactly on the whole block: it counts on neither side, all five sums are empty
    feat = metrics.niqe_features(m)
    assert np.isnan(feat[k, [1, 3, 4, 5, 19, 21]]).all() and (feat[k, ALPHAS] == 0.2).all()  # argmin of an all-NaN row is 0
    good = [j for j in range(6) if j != k]
    assert np.isfinite(feat[good]).all()
    # niqe.py:142-153 by hand: nanmean over all rows, covariance of the NaN-free rows
    mu_pris, cov_pris = d['params']
    diff = mu_pris - np.nanmean(feat, axis=0)
    want = float(np.sqrt(diff @ np.linalg.pinv((cov_pris + np.cov(feat[good], rowvar=False)) / 2) @ diff.T)[0, 0])
    got = metrics.niqe_from_moments(m[None], nbh, nbw, d['params'])
    assert np.isfinite(want) and got == [want]
    assert got[0] != metrics.niqe_from_moments(_restated('smooth')[0], nbh, nbw, d['params'])[0]


def test_fewer_than_two_nan_free_blocks_give_nan():
    from edvr_amd import metrics
    d = _data()
    m = _restated('noise')[0][:1].copy()
    assert np.isfinite(metrics.niqe_from_moments(m, 1, 2, d['params'])[0])
    m[0, :, 0] = 0.0  # block 0 constant at both scales: one NaN-free block is left, np.cov has nothing to estimate
    assert np.isnan(metrics.niqe_from_moments(m, 1, 2, d['params'])[0])
    one_sided = _restated('noise')[0][:1].copy()
    one_sided[0, 0, 1, 2, :2] = 0.0  # a map without negative values: the mean of an empty selection
    assert np.isnan(metrics.niqe_features(one_sided)[0, 1, 7]) and np.isnan(metrics.niqe_from_moments(one_sided, 1, 2, d['params'])[0])


def test_no_block_fits_is_a_value_error():
    from edvr_amd import metrics
    assert metrics.niqe_grid(96, 192) == (1, 2) and metrics.niqe_grid(203, 301, 4) == (2, 3) and metrics.niqe_grid(200, 301, 4) == (2, 3)
    for h, w, crop in ((95, 400, 0), (400, 95, 0), (96, 96, 1), (97, 97, 1)):
        with pytest.raises(ValueError, match='96x96'):
            metrics.niqe_grid(h, w, crop)
    with pytest.raises(ValueError):
        metrics.niqe_from_moments(_restated('noise')[0], 2, 2, _data()['params'])  # moments of 2 blocks, a grid of 4
    with pytest.raises(NotImplementedError):
        metrics.calculate_niqe(torch.zeros(1, 3, 96, 96), params=_data()['params'])  # a CPU tensor, like its neighbours
    with pytest.raises(NotImplementedError, match='gray'):
        metrics.calculate_niqe(torch.zeros(1, 3, 96, 96), params=_data()['params'], convert_to='gray')


def test_load_niqe_params(tmp_path):
    from edvr_amd import metrics
    mu, cov = metrics.load_niqe_params(PARAMS)
    assert mu.shape == (1, 36) and cov.shape == (36, 36) and mu.dtype == cov.dtype == np.float64
    assert np.array_equal(cov, cov.T) and np.isfinite(mu).all() and 2.0 < mu[0, 0] < 3.5  # the pristine shape parameter
    np.savez(tmp_path / 'bad.npz', mu_pris_param=np.zeros((1, 18)), cov_pris_param=np.zeros((18, 18)))
    with pytest.raises(ValueError, match='36'):
        metrics.load_niqe_params(tmp_path / 'bad.npz')


def test_window_is_the_parameter_files_window():
    from edvr_amd import metrics
    win = metrics.niqe_window()
    assert win.shape == (7, 7) and win.dtype == np.float64 and np.array_equal(win, win.T) and np.array_equal(win, win[::-1, ::-1])
    assert np.abs(win - np.load(PARAMS)['gaussian_window']).max() <= 1e-16
    assert abs(win.sum() - 1.0) < 1e-15


def test_argmin_shortcut_is_the_full_argmin():
    from edvr_amd import metrics
    gam, r_gam, increasing = metrics._niqe_table()
    assert increasing and len(gam) == 9801
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(r_gam[0] - 0.05, r_gam[-1] + 0.05, 300), r_gam[[0, 1, 4000, -1]], (r_gam[10:14] + r_gam[11:15]) / 2, [np.nan]])
    with np.errstate(invalid='ignore'):
        want = [int(np.argmin((r_gam - v) ** 2)) for v in x]
    assert metrics._niqe_argmin(x).tolist() == want


# ------------------------------------------------------------------------------------------------ scripts
def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), '..', 'scripts', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Net(torch.nn.Module):
    def __init__(self, *a, **k):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def to(self, device):
        return self

    def check_offsets(self):
        pass


def test_restore_video_niqe_options(tmp_path, monkeypatch, capsys):
    import edvr_amd
    from edvr_amd import metrics as M, y4m
    mod = _load('restore_video')
    a = mod.parse_args(['-', '-'])
    assert a.niqe is None and a.niqe_json is None
    a = mod.parse_args(['in.y4m', 'out.y4m', '--niqe', 'p.npz', '--niqe-json', 'n.json'])
    assert (a.niqe, a.niqe_json) == ('p.npz', 'n.json')
    with pytest.raises(SystemExit) as e:
        mod.parse_args(['-', '-', '--niqe-json', 'n.json'])
    assert e.value.code == 2
    capsys.readouterr()

    seen = {}

    def restore_y4m(net, reader, dst, on_chunk=None, **kw):
        seen['hook'] = on_chunk
        for k in (3, 1):
            on_chunk(torch.zeros(k, 3, 96, 192))
        return 4

    def niqe(img, crop_border=0, params=None, convert_to='y'):
        assert params == 'PARAMS'
        seen.setdefault('n', 0)
        seen['n'] += img.shape[0]
        return [float(seen['n'] - img.shape[0] + i) for i in range(img.shape[0])]

    monkeypatch.setattr(edvr_amd, 'EDVR', _Net)
    monkeypatch.setattr(y4m, 'restore_y4m', restore_y4m)
    monkeypatch.setattr(M, 'calculate_niqe', niqe)
    monkeypatch.setattr(M, 'load_niqe_params', lambda path: 'PARAMS')
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: None)
    src = tmp_path / 'in.y4m'
    src.write_bytes(b'YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420jpeg\n')
    args = mod.parse_args([str(src), str(tmp_path / 'out.y4m'), '--num-feat', '8', '--niqe', 'p.npz', '--niqe-json', str(tmp_path / 'n.json')])
    lines = []
    assert mod.restore(args, log=lines.append) == 4
    assert callable(seen['hook']) and seen['n'] == 4
    assert any('NIQE 1.5000 over 4 frames' in ln and '0.000 1.000 2.000 3.000' in ln for ln in lines)
    assert any('not scored' in ln for ln in lines)  # a 16 x 24 input holds no two blocks
    rec = json.load(open(tmp_path / 'n.json'))
    assert rec == {'output': {'niqe': [0.0, 1.0, 2.0, 3.0], 'average': 1.5}, 'input': None}
    # without --niqe the hook is not installed
    seen.clear()
    monkeypatch.setattr(y4m, 'restore_y4m', lambda net, reader, dst, **kw: seen.update(kw) or 0)
    mod.restore(mod.parse_args([str(src), str(tmp_path / 'out.y4m'), '--num-feat', '8']), log=lines.append)
    assert 'on_chunk' not in seen
    buf = io.StringIO()
    mod.report_niqe(argparse.Namespace(input='a', output='b'), [2.0], [4.0, 6.0], log=lambda s: buf.write(s + '\n'))
    assert 'b: NIQE 2.0000 over 1 frames' in buf.getvalue() and 'a: NIQE 5.0000 over 2 frames' in buf.getvalue()


def test_eval_video_niqe_option(tmp_path, monkeypatch):
    import edvr_amd
    from edvr_amd import data as D, metrics as M
    ev = _load('eval_video')
    assert ev.parse_args(['--gt', 'g', '--lq', 'l']).niqe is None
    assert ev.parse_args(['--gt', 'g', '--lq', 'l', '--niqe', 'p.npz']).niqe == 'p.npz'
    write_video_test_tree(str(tmp_path), dict(folders=['000', '011'], frames=7, lq_hw=(8, 12), scale=4))

    def read_img_seq(paths, device='cpu', **k):
        return torch.stack([torch.from_numpy(D.decode_image(open(p, 'rb').read()).transpose(2, 0, 1).copy()).float() / 255 for p in paths])

    def validate_video(net, lq, gt=None, num_frame=5, padding='reflection_circle', chunk=8, crop_border=0, test_y_channel=False,
                       self_ensemble=None, time_reverse=False):
        return torch.full((lq.shape[0], 3, 32, 48), 0.5 if self_ensemble else 0.25), [31.0 if self_ensemble else 30.0] * lq.shape[0]

    calls = []

    def niqe(img, crop_border=0, params=None, convert_to='y'):  # tells the three sources apart by their content
        assert params == 'PARAMS' and crop_border == 2 and img.shape[0] <= 3
        calls.append(img.shape[0])
        v = float(img[0, 0, 0, 0])
        return [{0.25: 5.0, 0.5: 4.0}.get(v, 7.0)] * img.shape[0]

    monkeypatch.setattr(edvr_amd, 'EDVR', _Net)
    monkeypatch.setattr(D, 'read_img_seq', read_img_seq)
    monkeypatch.setattr(D, 'imresize', lambda x, s: torch.full((x.shape[0], 3, 32, 48), 0.75))
    monkeypatch.setattr(M, 'validate_video', validate_video)
    monkeypatch.setattr(M, 'calculate_niqe', niqe)
    monkeypatch.setattr(M, 'calculate_psnr', lambda a, b, crop_border=0, test_y_channel=False: [20.0] * a.shape[0])
    monkeypatch.setattr(M, 'load_niqe_params', lambda path: 'PARAMS')
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    base = dict(lq=str(tmp_path / 'lq'), gt=str(tmp_path / 'gt'), weights=None, name='REDS4', num_feat=64, num_reconstruct_block=2, num_frame=5,
                hr_in=False, with_predeblur=False, no_tsa=False, padding='reflection', crop_border=2, test_y_channel=False, batch=3)
    lines = []
    out_json = tmp_path / 'r.json'
    summary = ev.evaluate(argparse.Namespace(**base, niqe='p.npz', self_ensemble='flip4', bicubic_baseline=True, json=str(out_json)), log=lines.append)
    assert summary == {'000': 30.0, '011': 30.0}
    assert calls == [3, 3, 1] * 6  # model, second pass, baseline for each folder, `batch` frames per launch
    assert len(lines) == 3 and all('; NIQE 5.0000, self-ensemble flip4 4.0000 (bicubic 7.0000)' in ln and 'PSNR' in ln or 'average' in ln for ln in lines)
    assert lines[-1].endswith('; NIQE 5.0000, self-ensemble flip4 4.0000 (bicubic 7.0000)')
    rec = json.load(open(out_json))
    assert rec['niqe'] == {'000': 5.0, '011': 5.0} and rec['niqe_average'] == 5.0
    assert rec['self_ensemble_niqe'] == {'000': 4.0, '011': 4.0} and rec['self_ensemble_niqe_average'] == 4.0
    assert rec['bicubic_niqe'] == {'000': 7.0, '011': 7.0} and rec['bicubic_niqe_average'] == 7.0
    assert rec['average'] == 30.0 and rec['bicubic_average'] == 20.0
    # without the option: no NIQE call, no NIQE in the report
    del calls[:], lines[:]
    ev.evaluate(argparse.Namespace(**base, json=str(out_json)), log=lines.append)
    assert not calls and not any('NIQE' in ln for ln in lines) and 'niqe' not in json.load(open(out_json))
    # the model alone
    ev.evaluate(argparse.Namespace(**base, niqe='p.npz', json=str(out_json)), log=lines.append)
    assert lines[-1].endswith('; NIQE 5.0000') and set(k for k in json.load(open(out_json)) if 'niqe' in k) == {'niqe', 'niqe_average'}
