"""CPU: the definition of inverse telecine on the designed clip - the NumPy restatement (tests/telecine_ref.py) finds every
film partner, drops true duplicates, flags exactly the orphans and returns the film frames bit for bit - and the host side that decides
on the device's table (edvr_amd/telecine.py): the batch functions against the restatement, PulldownDetector against the batch functions for
every piece pattern, film_rate and resolve_field_order."""
import math

import numpy as np
import pytest

import telecine_ref as T
import util_telecine as U

H, W, FMT = U.FILM_H, U.FILM_W, '420'


def _case(first, phase, noise):
    video, src = U.telecine(U.film_clip(), first, phase)
    video = U.add_noise(video, H, W, FMT, noise, seed=10 * phase + noise)
    info = {}
    out = T.inverse_telecine(video, H, W, FMT, first, info=info)
    return video, src, out, info


@pytest.mark.parametrize('noise', [0, 2])
@pytest.mark.parametrize('first', ['top', 'bottom'])
@pytest.mark.parametrize('phase', range(6))
def test_the_designed_clip(phase, first, noise):
    """14 film frames telecined into 16 - 17 video frames: every frame is matched to its film partner, combed is set on exactly the orphan
    first fields a truncated start leaves (mic 240 / 256 there, 80 - the three static lines, not more than mi: the comparison is strict
    - everywhere else), a dropped frame repeats the frame before it wherever the start is orphan-free, and without noise phases 0 - 3
    return film frames bit for bit."""
    film = U.film_clip()
    video, src, out, info = _case(first, phase, noise)
    assert video.shape[0] in (16, 17)
    partner, shown = U.partners(src), [src[2 * v] for v in range(video.shape[0])]
    for v, (want, got) in enumerate(zip(partner, info['matches'])):
        either = v > 0 and src[2 * v - 1] == src[2 * v] == src[2 * v + 1]  # three fields of one film frame: both candidates are it
        assert want is None or got == want or either, (v, want, got)
        if noise == 0 and either:
            assert got == 0  # the tie goes to c
    orphans = [v for v, p in enumerate(partner) if p is None]
    assert orphans == ([] if phase in U.ORPHAN_FREE else [0])
    assert [v for v, c in enumerate(info['combed']) if c] == orphans
    mic = [int(r[3] if m else r[2]) for r, m in zip(info['table'], info['matches'])]
    assert all((m >= 240) if v in orphans else (m == 80) for v, m in enumerate(mic)), mic
    assert len(info['dropped']) == video.shape[0] // 5 and info['scores'][0] == math.inf
    if phase in U.ORPHAN_FREE:
        assert all(shown[d] == shown[d - 1] for d in info['dropped']), info['dropped']
    kept = [v for v in range(video.shape[0]) if v not in info['dropped']]
    assert out.shape[0] == len(kept)
    if noise == 0:
        for j, v in enumerate(kept):
            if v not in orphans:
                assert np.array_equal(out[j], film[shown[v]]), (j, v)
        if phase in U.ORPHAN_FREE:  # and no film frame is lost: they come out in order, each once (a trailing partial cycle keeps its repeat)
            films = [shown[v] for v in kept]
            assert sorted(set(films)) == list(range(films[0], films[-1] + 1))


def test_the_fallback_is_the_frame_rate_deinterlacer():
    import deint_ref as D
    video, src, out, info = _case('top', 4, 0)
    assert info['combed'][0] and 0 not in info['dropped']
    assert np.array_equal(out[0], D.deinterlace(video[:1], H, W, FMT, 'top', 'frame', nxt=video[1])[0])


def test_decimate_off_keeps_every_frame():
    video, src = U.telecine(U.film_clip(), 'top', 0)
    info = {}
    out = T.inverse_telecine(video, H, W, FMT, 'top', decimate=False, info=info)
    assert out.shape[0] == video.shape[0] and info['dropped'] == []


def _tables():
    """Tables of 17 rows: the designed clip's, at a clean and an orphan phase, and random ones with many ties."""
    out = [T.field_match(U.telecine(U.film_clip(), 'top', p)[0], H, W, FMT, 'top') for p in (0, 3, 4)]
    rng = np.random.default_rng(5)
    out += [rng.integers(0, 4, size=(17, 7)) * np.array([1, 1, 40, 40, 1, 1, 1]) for _ in range(3)]
    return out


def test_batch_functions_equal_the_restatement():
    from edvr_amd import telecine
    for table in _tables():
        for mi in (80, 79, 0):
            matches, combed, scores, dropped = T.decide(table, mi)
            assert telecine.match_fields(table, mi) == (matches, combed)
            assert telecine.duplicate_scores(table, matches) == scores
            for n in (0, 4, 5, 9, 10, 17):
                assert telecine.select_drops(scores, n) == [d for d in dropped if d < 5 * (n // 5)]
    with pytest.raises(ValueError):
        telecine.select_drops([1.0] * 4, 5)
    with pytest.raises(ValueError):
        telecine.duplicate_scores(table, [0] * 3)
    with pytest.raises(ValueError):
        telecine.match_fields([[0] * 6])
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            telecine.match_fields(table, mi=bad)


def test_pulldown_detector_equals_the_batch_functions_for_every_split():
    """Every composition of 17 into pieces (2^16 of them), on a clip table, plus both decimate settings on a table with ties."""
    from edvr_amd import telecine
    tables = _tables()
    for table, decimate, every in ((tables[2], True, True), (tables[3], True, False), (tables[4], False, False)):
        n = len(table)
        rows = table.tolist()
        matches, combed = telecine.match_fields(table)
        scores = telecine.duplicate_scores(table, matches)
        drops = telecine.select_drops(scores, n) if decimate else []
        want = [(i, matches[i], combed[i], i not in drops) for i in range(n)]
        for cuts in range(0, 1 << (n - 1), 1 if every else 257):
            edges = [0] + [i + 1 for i in range(n - 1) if cuts >> i & 1] + [n]
            det = telecine.PulldownDetector(decimate=decimate)
            got = []
            for a, b in zip(edges, edges[1:]):
                new = det.push(rows[a:b])
                assert all(i < b for i, *_ in new)
                if decimate:
                    assert det.released == 5 * (b // 5)  # a frame leaves as soon as its cycle is whole
                got += new
            got += det.finish()
            assert got == want, edges
            assert det.dropped == drops and det.scores == scores and det.matches == matches
        with pytest.raises(RuntimeError):
            det.push(rows[:1])


def test_film_rate():
    from edvr_amd.y4m import film_rate
    assert film_rate('30000:1001') == '24000:1001'
    assert film_rate('60000:1001') == '48000:1001'
    assert film_rate('30:1') == '24:1'
    assert film_rate('25:1') == '20:1'
    assert film_rate('2997:100') == '2997:125'
    assert film_rate(None) is None
    for bad in ('30', '30000/1001', 'a:b', '30:', ':1', '30:0', '-30:1', '3.0:1'):
        with pytest.raises(ValueError):
            film_rate(bad)


def test_resolve_field_order_with_film():
    from edvr_amd.y4m import resolve_field_order

    class Reader:
        def __init__(self, interlace):
            self.interlace = interlace

    assert resolve_field_order('film', 'auto', Reader('t')) == ('top', 'film')
    assert resolve_field_order('film', 'auto', Reader('b')) == ('bottom', 'film')
    for tag in ('p', '?', None):
        assert resolve_field_order('film', 'auto', Reader(tag)) == (None, 'film')  # progressive: passed through, no launch
    assert resolve_field_order('film', 'bff', Reader('p')) == ('bottom', 'film')
    assert resolve_field_order('field', 'auto', Reader('t')) == ('top', 'field')
    assert resolve_field_order(None, 'auto', Reader('t')) == (None, None)
    with pytest.raises(ValueError, match='film'):
        resolve_field_order('ivtc', 'auto', Reader('t'))
    with pytest.raises(ValueError):
        resolve_field_order('film', 'top', Reader('t'))


# ---------------------------------------------------------------------------------------------------------------- the generator
def _numpy_ops(monkeypatch, log=None):
    """ops.field_match / field_weave / deinterlace restated in NumPy on CPU tensors, so that y4m.inverse_telecined runs here."""
    import deint_ref as D
    import torch
    from edvr_amd import ops
    arr = lambda t: None if t is None else t.numpy().reshape(-1)

    def match(yuv, h, w, fmt='420', *, first='top', prev=None, prev2=None, nt=2, ct=9, out=None):
        if log is not None:
            log.append(('match', yuv.shape[0]))
        return torch.from_numpy(T.field_match(yuv.numpy(), h, w, fmt, first, arr(prev), arr(prev2), nt, ct))

    def weave(yuv, h, w, fmt='420', *, first='top', frames, matches, prev=None, out=None):
        assert prev is not None or (0, 1) not in zip(frames, matches)
        return out.copy_(torch.from_numpy(T.field_weave(yuv.numpy(), h, w, fmt, first, frames, matches, arr(prev))))

    def deint(yuv, h, w, fmt='420', *, first='top', mode='field', prev=None, next=None, out=None):
        if log is not None:
            log.append(('deinterlace', yuv.shape[0]))
        return out.copy_(torch.from_numpy(D.deinterlace(yuv.numpy(), h, w, fmt, first, mode, prev=arr(prev), nxt=arr(next))))

    monkeypatch.setattr(ops, 'field_match', match)
    monkeypatch.setattr(ops, 'field_weave', weave)
    monkeypatch.setattr(ops, 'deinterlace', deint)


def _compositions(n, sizes=(1, 2, 3, 4)):
    if n == 0:
        yield []
    for s in sizes:
        if s <= n:
            for rest in _compositions(n - s, sizes):
                yield [s] + rest


@pytest.mark.parametrize('phase, first', [(0, 'top'), (3, 'bottom'), (4, 'top'), (5, 'bottom')])
def test_inverse_telecined_gives_the_whole_clip_for_every_piece_pattern(monkeypatch, phase, first):
    """The generator's own logic - what it holds, when a frame leaves, which frame is a weave's prev and a fallback's neighbours - on the
    CPU with the ops restated: every composition of the first 7 frames into pieces of 1 ... 4, and pieces of 1, 2, 3, 4, 5 and all on
    the whole clip, with and without decimation; the stats are the restatement's decisions."""
    import torch
    from edvr_amd import y4m
    _numpy_ops(monkeypatch)
    video, _ = U.telecine(U.film_clip(), first, phase)
    n = video.shape[0]
    for frames, patterns, decimate in ((video[:7], list(_compositions(7)), True), (video, [[s] * (n // s) + [n % s] * (n % s > 0) for s in (1, 2, 3, 4, 5, n)], True),
                                       (video[:7], list(_compositions(7))[::5], False)):
        info = {}
        want = T.inverse_telecine(frames, H, W, FMT, first, decimate=decimate, info=info)
        clip = torch.from_numpy(frames)
        for pattern in patterns:
            edges = np.cumsum([0] + pattern)
            stats = {}
            got = list(y4m.inverse_telecined((clip[a:b] for a, b in zip(edges, edges[1:])), H, W, FMT, first, decimate, stats=stats))
            assert all(g.shape[0] for g in got) and np.array_equal(torch.cat(got).numpy(), want), pattern
            assert stats == dict(film_matches=info['matches'], film_combed=[i for i, c in enumerate(info['combed']) if c], film_dropped=info['dropped'],
                                 film_dropped_scores=[info['scores'][d] for d in info['dropped']])


def test_inverse_telecined_measures_the_next_piece_before_it_decides(monkeypatch):
    """Pieces of one frame, nothing dropped: piece k + 1 is fetched and measured before the frame of piece k leaves - the host's wait for
    a table lies behind the next launch - and the orphan first frame (phase 4) waits for the frame after it, then leaves deinterlaced."""
    import torch
    from edvr_amd import y4m
    log = []
    _numpy_ops(monkeypatch, log)
    video, _ = U.telecine(U.film_clip(), 'top', 4)
    clip = torch.from_numpy(video[:4])

    def pieces():
        for i in range(4):
            log.append(('read', i))
            yield clip[i:i + 1]

    for out in y4m.inverse_telecined(pieces(), H, W, FMT, 'top', decimate=False):
        log.append(('out', out.shape[0]))
    assert log == [('read', 0), ('match', 1), ('read', 1), ('match', 1), ('deinterlace', 1), ('out', 1), ('read', 2), ('match', 1), ('out', 1),
                   ('read', 3), ('match', 1), ('out', 1), ('out', 1)]
    assert list(y4m.inverse_telecined(iter(()), H, W, FMT)) == []


@pytest.mark.parametrize('decimate', [True, False])
def test_restore_y4m_film_between_the_copy_and_the_decode(monkeypatch, decimate):
    import io
    import torch
    import util_yuv  # noqa: F401  (what the stand-ins decode and encode with)
    from test_deinterlace_cpu import _Nearest4, _stand_ins
    from edvr_amd import y4m
    calls = []
    Y = _stand_ins(monkeypatch, calls)
    _numpy_ops(monkeypatch)
    h, w = 12, 32
    video, _ = U.telecine(U.film_clip(7, h, w), 'bottom', 0, h, w)
    n = video.shape[0]
    info = {}
    want = T.inverse_telecine(video, h, w, FMT, 'bottom', decimate=decimate, info=info)
    out, stats = io.BytesIO(), {}
    got = y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(video, h, w, 'F30000:1001 Ib A1:1 C420jpeg')), out, read_frames=3, deinterlace='film',
                          film_decimate=decimate, chunk=3, stats=stats)
    assert got == want.shape[0] == (n - n // 5 if decimate else n)
    assert _Nearest4.made[-1].kwargs == dict(chunk=3)  # the restorer sees none of the arguments
    head = out.getvalue().split(b'\n')[0].split()
    assert b'Ip' in head and (b'F24000:1001' if decimate else b'F30000:1001') in head
    rgb = Y.decode_def(torch.from_numpy(want), h, w, 'bt601', 'limited', 'bilinear').repeat_interleave(4, 2).repeat_interleave(4, 3)
    assert torch.equal(y4m.Y4MReader(io.BytesIO(out.getvalue())).read(n + 1)[:, 6:], Y.encode_def(rgb, 'bt601', 'limited'))
    assert stats['frames'] == got and stats['film_matches'] == info['matches'] and stats['film_dropped'] == info['dropped']
    assert stats['film_combed'] == [i for i, c in enumerate(info['combed']) if c]  # (at 12 rows the lines and the box do comb: the fallback runs too)
    # a progressive stream passes through, with the calls it always made and its rate
    calls.clear()
    out = io.BytesIO()
    assert y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(video, h, w, 'F24:1 Ip C420jpeg')), out, read_frames=5, deinterlace='film') == n
    assert calls == [('yuv420_to_rgb', 5), ('rgb_to_yuv420', 5), ('yuv420_to_rgb', n - 5), ('rgb_to_yuv420', n - 5)] and b'F24:1' in out.getvalue().split(b'\n')[0].split()
    with pytest.raises(ValueError, match='film_params'):
        y4m.restore_y4m(torch.nn.Linear(1, 1), io.BytesIO(U.y4m_bytes(video, h, w, 'F24:1 It C420jpeg')), io.BytesIO(), deinterlace='film', film_params={'cycle': 5})


def test_restore_video_command_line_takes_film(capsys):
    from test_deinterlace_cpu import _script
    mod = _script()
    args = mod.parse_args(['-', '-', '--deinterlace', 'film'])
    assert (args.deinterlace, args.field_order, args.no_decimate, args.film_json) == ('film', 'auto', False, None)
    args = mod.parse_args(['in.y4m', 'out.y4m', '--deinterlace', 'film', '--no-decimate', '--film-json', 'f.json', '--field-order', 'bff'])
    assert (args.deinterlace, args.field_order, args.no_decimate, args.film_json) == ('film', 'bff', True, 'f.json')
    args = mod.parse_args(['-', '-'])
    assert (args.deinterlace, args.no_decimate, args.film_json) == (None, False, None)
    for bad in (['-', '-', '--no-decimate'], ['-', '-', '--deinterlace', '--film-json', 'f.json'], ['-', '-', '--deinterlace', 'frame', '--no-decimate']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
