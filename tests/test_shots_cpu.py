"""CPU: scene cuts (edvr_amd/shots.py) - the cut rule on hand-written tables, the streaming detector against it, the
restorer's per-shot schedule with CPU stand-ins for the device primitives, argument errors and the command line.  The device side is
tests/test_gpu_shots.py."""
import importlib.util
import json
import os
import random

import pytest
import torch

import util_shots as S
from test_video_cpu import PADDINGS, _StubNet, _batches, _stub_restorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_select_cuts_on_hand_written_tables():
    from edvr_amd.shots import select_cuts
    hi, lo = 50.0, 1.0

    def table(n, *at):
        return [hi if i in at else lo for i in range(n)]

    for fn in (select_cuts, S.select_cuts):
        assert fn(table(20, 5, 12), 20, 10.0, 3) == [5, 12]
        assert fn(table(20, 5, 7, 12), 20, 10.0, 3) == [5, 12]          # 7 lies inside min_shot of the cut at 5: dropped
        assert fn(table(20, 5, 8), 20, 10.0, 3) == [5, 8]               # ... 8 does not
        assert fn(table(20, 5, 18), 20, 10.0, 3) == [5]                 # 18 lies inside min_shot of the end
        assert fn(table(20, 5, 17), 20, 10.0, 3) == [5, 17]             # ... 17 leaves exactly min_shot frames
        assert fn(table(20, 9, 10), 20, 10.0, 3) == [9]                 # two adjacent candidates: the first wins
        assert fn(table(20, 1, 2, 3, 4), 20, 10.0, 3) == [3]            # 1, 2 too close to the start; 4 too close to the cut at 3
        assert fn(table(20, 1, 2, 3, 4), 20, 10.0, 1) == [1, 2, 3, 4]
        assert fn(table(5, 1, 2, 3, 4), 5, 10.0, 3) == []               # n < 2 min_shot: no place for a cut
        assert fn(table(6, 3), 6, 10.0, 3) == [3]                       # n = 2 min_shot: exactly one place
        assert fn(table(6, 2, 4), 6, 10.0, 3) == []
        assert fn([0.0, 10.0, 0.0, 0.0, 9.999999, 0.0, 10.0, 0.0, 0.0], 9, 10.0, 2) == [6]   # equality counts; frame 1 is too early
        assert fn([0.0, 0.0, 10.0, 0.0, 0.0], 5, 10.0, 2) == [2]
        assert fn([99.0], 1, 10.0, 2) == [] and fn([], 0, 10.0, 2) == []
        assert fn([99.0, 99.0], 2, 10.0, 1) == [1]                      # scores[0] is never looked at
    with pytest.raises(ValueError):
        select_cuts([0.0, 1.0], 3)
    with pytest.raises(ValueError):
        select_cuts([0.0, 1.0], 2, 10.0, 0)


def test_cut_scores_is_the_definition():
    from edvr_amd.shots import cut_scores
    sads = [0, 300, 330, 4000, 360, 0, 7]
    mafd, score = cut_scores(sads, 100)
    assert (mafd, score) == S.scores(sads, 100)
    assert mafd == [0.0, 3.0, 3.3, 40.0, 3.6, 0.0, 0.07]
    assert score[1] == 3.0 and score[3] == 40.0 - 3.3 and score[4] == 3.6 and score[5] == 0.0   # mafd runs on across the cut at 3
    # chained pieces give the same lists: the number before a piece is all that crosses
    m1, s1 = cut_scores(torch.tensor(sads[:3]), 100)
    m2, s2 = cut_scores(sads[3:], 100, prev_mafd=m1[-1])
    assert (m1 + m2, s1 + s2) == (mafd, score)


def test_shot_detector_is_select_cuts_for_every_piece_pattern():
    from edvr_amd.shots import ShotDetector, select_cuts
    rng = random.Random(1234)
    checked = with_cuts = 0
    for _ in range(200):
        n, min_shot = rng.randint(1, 40), rng.randint(2, 7)
        scores = [rng.choice((0.5, 3.0, 9.99, 10.0, 25.0, 60.0)) if rng.random() < 0.35 else rng.random() * 4 for _ in range(n)]
        want = select_cuts(scores, n, 10.0, min_shot)
        assert want == S.select_cuts(scores, n, 10.0, min_shot)
        for size in (1, 2, 3, 4, 5, n):
            det = ShotDetector(10.0, min_shot)
            seen = []
            for a in range(0, n, size):
                new = det.push(scores[a:a + size])
                arrived = min(a + size, n)
                assert det.arrived == arrived and 0 <= arrived - det.released < min_shot
                for c in new:
                    assert arrived >= c + min_shot and det.confirmed_at[c] == arrived  # frame c + min_shot - 1 is here
                    assert c < det.released
                seen += new
            seen += det.finish()
            assert det.released == n
            assert seen == det.cuts == want, (scores, min_shot, size)
            assert det.scores == scores
            assert all(b - a >= min_shot for a, b in S.shot_bounds(det.cuts, n)) or n < min_shot
            checked += 1
        with_cuts += bool(want)
    assert checked == 1200 and with_cuts >= 50
    det = ShotDetector(10.0, 2)
    det.finish()
    with pytest.raises(RuntimeError):
        det.push([1.0])


def test_shot_detector_from_sads():
    from edvr_amd.shots import ShotDetector
    sads = [0, 300, 330, 4000, 360, 340, 9000, 100, 120]
    mafd, score = S.scores(sads, 100)
    det = ShotDetector(10.0, 2)
    assert det.push_sad(sads[:2], 100) == [] and det.push_sad(sads[2:5], 100) == [3] and det.push_sad(sads[5:], 100) == [6]
    assert det.finish() == [] and det.cuts == [3, 6] == S.select_cuts(score, 9, 10.0, 2)
    assert det.mafd == mafd and det.scores == score


# ---------------------------------------------------------------------------------------------------------------- the restorer's schedule
def _cut_restorer(num_frame, padding, chunk, **kwargs):
    """test_video_cpu's CPU restorer with scene-cut arguments; every extract / restore step is recorded with the shot it ran in."""
    from edvr_amd import VideoRestorer

    class CpuRestorer(VideoRestorer):
        def _check_input(self, t):
            pass

        def _slot_table(self, slots, device):
            return torch.tensor(slots, dtype=torch.int32)

        def _gather(self, srcs, table):
            return [s[table.long()] for s in srcs]

        def _begin_shot(self):
            super()._begin_shot()
            self.steps.append(('shot',))

        def _run(self, steps, length):
            def recorded():
                for step in steps:
                    self.steps.append(step)
                    yield step
            return super()._run(recorded(), length)

    net = _StubNet(num_frame).eval()
    vr = CpuRestorer(net, num_frame=num_frame, padding=padding, chunk=chunk, **kwargs)
    vr.steps = []
    net.restorer = vr
    return net, vr


@pytest.mark.parametrize('padding', PADDINGS)
@pytest.mark.parametrize('chunk', (3, 8))
@pytest.mark.parametrize('pattern', ((1,), (3, 1, 7, 2), (22,)))
def test_schedule_with_explicit_cuts(padding, chunk, pattern):
    from edvr_amd import window_table
    t, n, cuts = 5, 22, [7, 16]
    net, vr = _cut_restorer(t, padding, chunk, cuts=cuts)
    with torch.no_grad():
        got = [int(f[0, 0, 0]) for f in vr.restore_iter(_batches(n, pattern))]
    assert got == list(range(n)) and vr.cuts_found == cuts and vr.cut_scores is None
    assert net.extracted == list(range(n))  # every frame through the extraction stage exactly once, in order
    shots, bounds = [], S.shot_bounds(cuts, n)
    for step in vr.steps:
        if step[0] == 'shot':
            shots.append([])
        else:
            shots[-1].append(step)
    assert len(shots) == 3
    rows_seen = []
    for (a, b), steps in zip(bounds, shots):
        table = window_table(b - a, t, padding).tolist()
        ext = out = 0
        for kind, first, arg in steps:  # indices are the shot's own: no step can name a frame of another shot
            if kind == 'extract':
                assert first == ext and first + arg <= b - a
                ext += arg
            else:
                assert first == out and len(arg) <= chunk and arg == table[first:first + len(arg)]
                out += len(arg)
                rows_seen += [[a + f for f in r] for r in arg]
        assert ext == out == b - a
    # what the network gathered: each shot's own window_table shifted by the shot's start
    assert net.windows == rows_seen == [[a + f for f in r] for a, b in bounds for r in window_table(b - a, t, padding).tolist()]
    for r, i in zip(net.windows, range(n)):
        a, b = next(s for s in bounds if s[0] <= i < s[1])
        assert all(a <= f < b for f in r)


def test_restore_with_explicit_cuts_on_the_stub():
    net, vr = _cut_restorer(5, 'reflection_circle', 4, cuts=[7, 16])
    lq = torch.arange(22, dtype=torch.float32).view(22, 1, 1, 1).expand(22, 3, 4, 4).contiguous()
    with torch.no_grad():
        out = vr.restore(lq)
    assert torch.equal(out, lq) and net.extracted == list(range(22)) and vr.cuts_found == [7, 16]
    sizes = [len(s[2]) for s in vr.steps if s[0] == 'restore']
    assert sizes == [4, 3, 4, 4, 1, 4, 2]  # chunks of 4 inside every shot, short at its end


def test_cuts_none_runs_the_parents_steps():
    """Without the argument nothing changes: one shot, the schedule's own step sequence for the arrival pattern."""
    from edvr_amd import WindowSchedule
    for padding in PADDINGS:
        for pattern in ((1,), (3, 1, 7, 2)):
            net, vr = _cut_restorer(5, padding, 4)
            assert vr.cuts is None and vr.min_shot == 5
            with torch.no_grad():
                list(vr.restore_chunks(_batches(17, pattern)))
            want, sched = [('shot',)], WindowSchedule(5, padding, 4, _probe=False)
            for item in _batches(17, pattern):
                want += list(sched.push(1 if item.dim() == 3 else item.shape[0]))
            want += list(sched.finish())
            assert vr.steps == want and vr.cuts_found is None


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_argument_errors():
    from edvr_amd import VideoRestorer
    net = _StubNet(5).eval()

    def make(**kw):
        return VideoRestorer(net, num_frame=5, **kw)

    for bad in ([16, 7], [7, 7], [0, 7], [-3], [7, 16.0], [True, 9], 'scene', 7, [3], [7, 10]):
        with pytest.raises(ValueError):
            make(cuts=bad)
    assert make(cuts=(7, 16)).cuts == [7, 16] and make(cuts=[]).cuts == [] and make(cuts=[5, 10]).cuts == [5, 10]
    with pytest.raises(ValueError, match='min_shot'):
        make(cuts='auto', min_shot=4)          # below max(num_frame, 2)
    with pytest.raises(ValueError, match='min_shot'):
        make(cuts='auto', min_shot=5.0)
    assert make(cuts='auto', min_shot=9).min_shot == 9 and make(cuts='auto').min_shot == 5 and make(cuts='auto').cut_threshold == 10.0
    assert VideoRestorer(_StubNet(1).eval(), num_frame=1, cuts='auto').min_shot == 2
    for kw in (dict(cut_threshold=12.0), dict(min_shot=6), dict(cuts=[7], cut_threshold=12.0), dict(cuts=[7], min_shot=6)):
        with pytest.raises(ValueError, match="cuts='auto'"):
            make(**kw)
    with pytest.raises(ValueError):
        make(cuts='auto', cut_threshold=float('nan'))

    # the last shot is checked where the length becomes known: restore() before any launch, a stream at its end
    lq = torch.zeros(20, 3, 4, 4)
    for cuts in ([7, 16], [7, 20], [7, 25]):
        net, vr = _cut_restorer(5, 'replicate', 4, cuts=cuts)
        with torch.no_grad(), pytest.raises(ValueError, match='shot'):
            vr.restore(lq)
        assert net.extracted == []
        net, vr = _cut_restorer(5, 'replicate', 4, cuts=cuts)
        with torch.no_grad(), pytest.raises(ValueError, match='shot'):
            list(vr.restore_iter(lq.unbind(0)))
    net, vr = _cut_restorer(5, 'replicate', 4, cuts=[7, 15])
    with torch.no_grad():
        assert len(list(vr.restore_iter(lq.unbind(0)))) == 20


def test_cpu_frames_are_refused_with_cuts():
    from edvr_amd import VideoRestorer, ops
    vr = VideoRestorer(_StubNet(5).eval(), num_frame=5, cuts='auto')
    with torch.no_grad(), pytest.raises(NotImplementedError):
        vr.restore(torch.zeros(12, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        ops.frame_sad(torch.zeros(2, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        ops.frame_sad(torch.zeros(2, 4, 4, 3, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- the synthetic video
def test_synthetic_video_has_its_two_cuts():
    for H, W in ((36, 52), (20, 28)):
        v = S.synthetic_video(H, W)
        assert v.shape == (22, 3, H, W) and float(v.min()) >= 0.0 and float(v.max()) <= 1.0
        cuts, mafd, score = S.cuts_of(v)
        assert cuts == S.CUTS
        inside = [i for i in range(1, 22) if i not in S.CUTS]
        assert all(1.5 <= mafd[i] <= 4.2 for i in inside) and all(score[i] <= 4.2 for i in inside)
        assert all(score[c] >= 15.0 for c in S.CUTS)
        u8 = S.synthetic_video(H, W, torch.uint8)
        assert torch.equal(S.sad(u8), S.sad(v)) and torch.equal(S.sad(u8), S.sad(u8.permute(0, 3, 1, 2).float() / 255.0))


# ---------------------------------------------------------------------------------------------------------------- the script
def _script():
    spec = importlib.util.spec_from_file_location('restore_video', os.path.join(ROOT, 'scripts', 'restore_video.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restore_video_scene_cut_options(capsys, tmp_path):
    mod = _script()
    with pytest.raises(SystemExit) as e:
        mod.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--scene-cuts', '--min-shot', '--cuts', '--cuts-json'):
        assert opt in text, opt
    args = mod.parse_args(['-', '-'])
    assert (args.scene_cuts, args.min_shot, args.cuts, args.cuts_json) == (None, None, None, None) and mod.cut_kwargs(args) == {}
    args = mod.parse_args(['-', '-', '--scene-cuts'])
    assert args.scene_cuts == 10.0 and mod.cut_kwargs(args) == dict(cuts='auto', cut_threshold=10.0)
    args = mod.parse_args(['in.y4m', 'out.y4m', '--scene-cuts', '14.5', '--min-shot', '8', '--cuts-json', 'c.json'])
    assert mod.cut_kwargs(args) == dict(cuts='auto', cut_threshold=14.5, min_shot=8) and args.cuts_json == 'c.json'
    args = mod.parse_args(['-', '-', '--cuts', '7', '16'])
    assert args.cuts == [7, 16] and mod.cut_kwargs(args) == dict(cuts=[7, 16])
    for bad in (['-', '-', '--min-shot', '8'], ['-', '-', '--cuts-json', 'c.json'], ['-', '-', '--cuts', '7', '--scene-cuts'],
                ['-', '-', '--cuts'], ['-', '-', '--cuts', '9', '7'], ['-', '-', '--cuts', '0'], ['-', '-', '--scene-cuts', 'high'],
                ['-', '-', '--scene-cuts', '--min-shot', '4'], ['-', '-', '--num-frame', '7', '--scene-cuts', '--min-shot', '6']):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    # --cuts-json: the cuts, every frame's mafd and score, the threshold and min_shot
    args = mod.parse_args(['-', '-', '--scene-cuts', '12', '--cuts-json', str(tmp_path / 'c.json')])
    lines = []
    mod.report_cuts(args, dict(frames=4, cuts=[2], cut_scores=[0.0, 1.0, 30.0, 1.5], cut_mafd=[0.0, 1.0, 31.0, 1.5]), lines.append)
    rec = json.load(open(tmp_path / 'c.json'))
    assert rec == dict(frames=4, cuts=[2], mafd=[0.0, 1.0, 31.0, 1.5], score=[0.0, 1.0, 30.0, 1.5], threshold=12.0, min_shot=5)
    assert 'cuts at [2]' in lines[0]
