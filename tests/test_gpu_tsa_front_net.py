"""-m gpu: the one-pass head of TSA fusion inside EDVR - the network's output with it equals, bit for bit, the output with it switched off
(ops.set_tsa_front / EDVR_TSA_FRONT=0: tsa_temporal + two 1x1 convs), eagerly and through GraphedEDVR replays."""
import pytest
import torch

from util_edvr import build

pytestmark = pytest.mark.gpu

FUSED = 'tsa_front_split_kernel'


def _net(name, gpu):
    net, x, _ = build(name)
    if name == 'M_T5':  # at 32 x 48 like L_T7: 1536 pixels = 12 blocks of 128
        x = torch.rand(1, 5, 3, 32, 48, generator=torch.Generator().manual_seed(0))
    return net.to(gpu), x.to(gpu)


def _forward(ops, net, xg, on):
    seen = []
    prev = ops.set_tsa_front(on)
    ops.LAUNCH_HOOK = lambda name, flops, launch, *a: (seen.append(name), launch())
    try:
        with torch.no_grad():
            y = net(xg).clone()
    finally:
        ops.LAUNCH_HOOK = None
        ops.set_tsa_front(prev)
    return y, seen


@pytest.mark.parametrize('name', ['L_T7', 'M_T5'])
def test_network_output_is_the_same_bits_with_and_without_the_fused_head(gpu, name):
    from edvr_amd import ops
    from edvr_amd.graphs import GraphedEDVR
    net, xg = _net(name, gpu)
    _forward(ops, net, xg, True)  # (packs every weight layout, settles the DCNs' offset statistics)
    net.check_offsets(wait=True)
    y_off, seen_off = _forward(ops, net, xg, False)
    y_on, seen_on = _forward(ops, net, xg, True)
    assert FUSED not in seen_off and seen_off.count('tsa_temporal') == 1, seen_off
    assert seen_on.count(FUSED) == 1 and 'tsa_temporal' not in seen_on, seen_on
    assert len(seen_on) == len(seen_off) - 2  # one launch where there were three, everything else as it was
    assert torch.isfinite(y_on).all() and torch.equal(y_on, y_off)
    net.check_offsets()
    ops.split_guard_check(wait=True)
    g = GraphedEDVR(net, xg)  # (captured with the head on: the module default)
    assert ops.TSA_FRONT
    assert torch.equal(g(xg), y_off)
    assert torch.equal(g(xg), y_off)  # a second replay: same slots, same bits
    del g


def test_public_pieces_keep_their_meaning(gpu):
    """temporal() still returns the modulated tensor, spatial() takes it, align_windows() hands out tensors: callers that pass `mod`
    explicitly (the temporal-reversal ensemble, the tests) see what they saw."""
    from edvr_amd import ops
    net, xg = _net('M_T5', gpu)
    with torch.no_grad():
        y = net(xg)
        b, t = xg.shape[:2]
        pyr = net.extract_features(xg.view(b * t, *xg.shape[2:]))
        operand, sink = net.align_windows(pyr, b, t)
        assert torch.is_tensor(operand) and operand.shape[1] == t * 64
        assert torch.equal(net.restore_from_aligned(operand, xg[:, 2], b, t, sink=sink), y)
        al = operand.new_empty(0)
        net.taps = {}
        try:
            assert torch.equal(net(xg), y)  # taps collection: the three launches, the same bits
            al = net.taps['aligned']
        finally:
            net.taps = None
        mod = net.fusion.temporal(al)
        assert torch.is_tensor(mod) and torch.equal(mod, operand)
        assert torch.equal(net.fusion(al), net.fusion.spatial(mod))
    net.check_offsets()
    ops.split_guard_check(wait=True)
