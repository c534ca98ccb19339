"""fuse_irchain (planning option, off by default): which runs of stride-1 inverted residuals the planner puts in one launch (no GPU)."""
import subprocess
import sys

import numpy as np
import pytest

from f8net_amd import synth, topology
from f8net_amd.net import F8Net, build_net

CHAIN14 = ['stage_3_layer_1', 'stage_3_layer_2', 'stage_3_layer_3', 'stage_4_layer_0', 'stage_4_layer_1', 'stage_4_layer_2']
CHAIN7 = ['stage_5_layer_1', 'stage_5_layer_2', 'stage_6_layer_0']


@pytest.fixture(scope='module')
def mbv2():
    spec = topology.get('mobilenet_v2')
    return spec, synth.make_params(spec, 1)


def _chains(net):
    return [ln.split()[1] for ln in net.describe().splitlines() if 'ir_chain_x' in ln]


def _ops(net, n):
    return sum(net.launch_info(i, n)[2] for i in range(net.num_launches))


def test_mobilenet_v2_224_two_chains(mbv2):
    spec, params = mbv2
    off = build_net(spec, params, max_batch=128, hw=224)
    on = build_net(spec, params, max_batch=128, hw=224, options={'fuse_irchain': 1})
    assert off.num_launches == 28 and on.num_launches == 15
    assert _chains(on) == ['ir_chain_x6:' + '+'.join(CHAIN14), 'ir_chain_x3:' + '+'.join(CHAIN7)]
    idx = [i for i in range(on.num_launches) if 'ir_chain_x' in on.launch_info(i, 1)[0]]
    assert len(idx) == 2 and all(on.launch_kernel(i).startswith('f8::irchain_kernel<') for i in idx)
    assert _ops(on, 128) == pytest.approx(_ops(off, 128), rel=1e-12)
    assert on.arena_bytes <= off.arena_bytes
    for i in idx:
        assert on.launch_valu(i, 128) > 0


def test_option_off_is_todays_plan(mbv2):
    spec, params = mbv2
    plain = build_net(spec, params, max_batch=128, hw=224)
    off = build_net(spec, params, max_batch=128, hw=224, options={'fuse_irchain': 0})
    assert plain.get_option('fuse_irchain') == 0
    assert plain.describe() == off.describe() and plain.num_launches == 28 and not _chains(plain)


def test_environment_seeds_a_new_handle():
    code = ('from f8net_amd import synth, topology; from f8net_amd.net import build_net; s = topology.get("mobilenet_v2"); '
            'n = build_net(s, synth.make_params(s, 1), max_batch=4, hw=224); print(n.get_option("fuse_irchain"), n.num_launches)')
    import os
    env = dict(os.environ, F8_FUSE_IRCHAIN='1')
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))).stdout.split()
    assert out == ['1', '15']


def test_320_chains_the_10x10_run_only(mbv2):
    spec, params = mbv2
    net = build_net(spec, params, max_batch=2, hw=320, options={'fuse_irchain': 1})
    assert _chains(net) == ['ir_chain_x3:' + '+'.join(CHAIN7)], net.describe()


def test_64_chains_the_8x8_pair(mbv2):
    spec, params = mbv2
    net = build_net(spec, params, max_batch=2, hw=64, options={'fuse_irchain': 1})
    assert _chains(net) == ['ir_chain_x2:stage_2_layer_1+stage_2_layer_2', 'ir_chain_x6:' + '+'.join(CHAIN14), 'ir_chain_x3:' + '+'.join(CHAIN7)]


def _graph(n_blocks, second_reader=None, output_at=None, hw=6, stride2_at=None):
    """A pre conv, then n_blocks residual inverted residuals (32 channels, E 96) on hw x hw; second_reader = index of a block whose output a 1x1
    also reads; output_at = index of the block whose output is the net output (the blocks after it are built too: nothing reads their result);
    stride2_at = index of a block whose depthwise conv has stride 2 (and which therefore has no join)."""
    rng = np.random.default_rng(0)
    w = lambda *s: rng.integers(-20, 20, s).astype(np.int32)
    net = F8Net()
    t = net.input(32, hw, hw, 5)
    t = net.conv(t, w(32, 32, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=5, input_signed=True, quant_input=True, relu=False)
    outs = []
    for i in range(n_blocks):
        e = net.conv(t, w(96, 32, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=True, quant_input=True, relu=True)
        d = net.conv(e, w(96, 1, 3, 3), None, stride=2 if i == stride2_at else 1, pad=1, groups=96, weight_fl=6, input_fl=6, input_signed=False, quant_input=True, relu=True)
        p = net.conv(d, w(32, 96, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=5, input_signed=False, quant_input=True, relu=False)
        t = p if i == stride2_at else net.add(p, t)
        outs.append(t)
    last = outs[-1]
    if second_reader is not None:
        x = net.conv(outs[second_reader], w(32, 32, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=True, quant_input=True, relu=False)
        last = net.add(last, x)
    net.output(outs[output_at] if output_at is not None else last, as_float=False)
    net.set_option('fuse_irchain', 1)
    return net.finalize(2)


def test_graph_cut_at_a_second_reader():
    assert [c.split(':')[0] for c in _chains(_graph(5))] == ['ir_chain_x5']
    assert [c.split(':')[0] for c in _chains(_graph(5, second_reader=1))] == ['ir_chain_x2', 'ir_chain_x3']
    assert [c.split(':')[0] for c in _chains(_graph(5, second_reader=2))] == ['ir_chain_x3', 'ir_chain_x2']


def test_a_stride_2_block_ends_the_run():
    """The launch keeps ONE map in LDS: a stride-2 inverted residual is no block of a run — neither in its middle nor as its first —, the runs on
    either side of it are (12x12, then 6x6)."""
    assert [c.split(':')[0] for c in _chains(_graph(5, hw=12, stride2_at=2))] == ['ir_chain_x2', 'ir_chain_x2']
    assert [c.split(':')[0] for c in _chains(_graph(3, hw=12, stride2_at=0))] == ['ir_chain_x2']


def test_graph_cut_at_the_net_output():
    """An intermediate block output that is the net output ends the run there; the blocks behind it (whose results nothing reads) form a
    run of their own, or stay per-block launches when only one is left."""
    assert [c.split(':')[0] for c in _chains(_graph(4, output_at=1))] == ['ir_chain_x2', 'ir_chain_x2']
    assert [c.split(':')[0] for c in _chains(_graph(4, output_at=2))] == ['ir_chain_x3']
    assert [c.split(':')[0] for c in _chains(_graph(4, output_at=0))] == ['ir_chain_x3']
    assert [c.split(':')[0] for c in _chains(_graph(4, output_at=3))] == ['ir_chain_x4']       # (the run's own end)
