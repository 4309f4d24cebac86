"""CPU: the whole-video path's index table and schedule (edvr_amd/video.py) - no kernels.  The device side is tests/test_gpu_video.py."""
import json
import os

import pytest
import torch

PADDINGS = ('replicate', 'reflection', 'reflection_circle', 'circle')


def test_window_table_is_generate_frame_indices_row_by_row():
    from edvr_amd import window_table
    from edvr_amd.metrics import generate_frame_indices
    for pad in PADDINGS:
        for t in (3, 5, 7):
            for n in range(t, 21):
                tab = window_table(n, t, pad)
                assert tab.dtype == torch.int32 and tuple(tab.shape) == (n, t) and not tab.is_cuda
                assert tab.tolist() == [generate_frame_indices(i, n, t, pad) for i in range(n)], (pad, t, n)
                assert int(tab.min()) >= 0 and int(tab.max()) < n
    with pytest.raises(ValueError):
        window_table(3, 5, 'reflection_circle')  # reaches frame 4 of a 3-frame video
    with pytest.raises(AssertionError):
        window_table(10, 4, 'reflection')


def test_window_table_reproduces_the_reference_fixture():
    from edvr_amd import window_table
    gold = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'frame_indices.json')))
    assert len(gold) >= 24
    for key, want in gold.items():
        pad, t, n = key.split('/')
        assert window_table(int(n), int(t), pad).tolist() == want, key


class _StubNet(torch.nn.Module):
    """Stands in for the two stages: a frame's "features" are its index (the test's frames are filled with theirs), the "restored"
    frame is the centre frame; every call is recorded."""

    def __init__(self, num_frame):
        super().__init__()
        self.conv_l2_1 = torch.nn.Conv2d(2, 2, 3, 2, 1)
        self.hr_in = self.with_predeblur = False
        self.center_frame_idx = num_frame // 2
        self.extracted, self.windows, self.bank_at_extract, self.restorer = [], [], [], None

    def check_offsets(self, wait=True):
        pass

    def extract_features(self, frames, out=None):
        ids = frames[:, 0, 0, 0]
        self.extracted += [int(v) for v in ids]
        self.bank_at_extract.append(self.restorer.bank_frames)
        for o in out:
            assert o.shape[0] == frames.shape[0]
            o[:] = ids.view(-1, 1, 1, 1)
        return list(out)

    def restore_from_features(self, pyr, x_center, b, t, out_dtype=torch.float32):
        assert all(f.shape[0] == b * t for f in pyr) and x_center.shape[0] == b
        levels = [f[:, 0, 0, 0].view(b, t).to(torch.int64).tolist() for f in pyr]
        assert levels[0] == levels[1] == levels[2]
        self.windows += levels[0]
        return x_center.clone()


def _stub_restorer(num_frame, padding, chunk):
    from edvr_amd import VideoRestorer

    class CpuRestorer(VideoRestorer):  # CPU stand-ins for the device primitives
        def _check_input(self, t):
            pass

        def _slot_table(self, slots, device):
            return torch.tensor(slots, dtype=torch.int32)

        def _gather(self, srcs, table):
            return [s[table.long()] for s in srcs]

    net = _StubNet(num_frame).eval()
    vr = CpuRestorer(net, num_frame=num_frame, padding=padding, chunk=chunk)
    net.restorer = vr
    return net, vr


def _batches(n, pattern):
    """frame i is filled with i; pattern: sizes of the arriving batches, cycled (1 = single (3, h, w) frames)"""
    frames = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 3, 4, 8).contiguous()
    i = k = 0
    while i < n:
        m = min(pattern[k % len(pattern)], n - i)
        yield frames[i] if pattern == (1,) else frames[i:i + m]
        i, k = i + m, k + 1


@pytest.mark.parametrize('padding', PADDINGS)
@pytest.mark.parametrize('chunk', (1, 4, 8))
@pytest.mark.parametrize('n', (5, 6, 17, 40))
@pytest.mark.parametrize('pattern', ((1,), (3, 1, 7, 2)))
def test_schedule(padding, chunk, n, pattern):
    from edvr_amd import window_table
    t = 5
    net, vr = _stub_restorer(t, padding, chunk)
    table = window_table(n, t, padding).tolist()
    arrived, got = [0], []

    def counted(batches):
        for item in batches:
            arrived[0] += 1 if item.dim() == 3 else item.shape[0]
            yield item

    with torch.no_grad():
        for frame in vr.restore_iter(counted(_batches(n, pattern))):
            i = len(got)
            # none before its window is complete: everything its row names has arrived (and with it the frame num_frame // 2 ahead,
            # without which the row would not be known)
            assert max(table[i]) < arrived[0] and min(i + t // 2, n - 1) < arrived[0], (i, arrived[0])
            got.append(int(frame[0, 0, 0]))
    assert got == list(range(n))                       # in order, every frame
    assert net.extracted == list(range(n))             # every frame through the extraction stage exactly once
    assert net.windows == table                        # every output frame's gathered window is its table row
    limit = chunk + 2 * (t - 1)
    assert max(net.bank_at_extract) <= vr.capacity <= limit and vr.slots <= limit  # the bank: bounded whatever n is


def test_restore_is_restore_iter_over_the_tensor():
    net, vr = _stub_restorer(7, 'reflection_circle', 4)
    lq = torch.arange(19, dtype=torch.float32).view(19, 1, 1, 1).expand(19, 3, 4, 4).contiguous()
    with torch.no_grad():
        out = vr.restore(lq)
    assert torch.equal(out, lq) and net.extracted == list(range(19))


def test_cpu_input_and_training_mode_are_refused():
    from edvr_amd import EDVR, VideoRestorer
    net = EDVR(num_feat=16, num_frame=3, num_extract_block=1, num_reconstruct_block=1, center_frame_idx=1, deformable_groups=2).eval()
    vr = VideoRestorer(net, padding='replicate', chunk=2)
    assert vr.num_frame == 3
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            vr.restore(torch.rand(4, 3, 8, 8))
        with pytest.raises(NotImplementedError):
            list(vr.restore_iter([torch.zeros(8, 8, 3, dtype=torch.uint8)]))
    with pytest.raises(RuntimeError, match='no_grad'):
        vr.restore(torch.rand(4, 3, 8, 8))
    net.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match='eval'):
        vr.restore(torch.rand(4, 3, 8, 8))
    with pytest.raises(ValueError):
        VideoRestorer(EDVR(num_feat=16, num_frame=5, num_extract_block=1, num_reconstruct_block=1, center_frame_idx=1, deformable_groups=2))
