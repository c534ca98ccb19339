"""fuse_dws7 (planning option, off by default): which depthwise-separable blocks on 7x7 output maps the planner runs as one launch, and where
the average pool behind the last one is summed in it (no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

# the 13 blocks of MobileNet-V1 in order; at 224x224 their output maps are 112, 56, 56, 28, 28, 14 (x6), 7, 7 wide
BLOCKS = ['stage_0_layer_0', 'stage_1_layer_0', 'stage_1_layer_1', 'stage_2_layer_0', 'stage_2_layer_1'] + \
         [f'stage_3_layer_{i}' for i in range(6)] + ['stage_4_layer_0', 'stage_4_layer_1']


@pytest.fixture(scope='module')
def mbv1():
    spec = topology.get('mobilenet_v1')
    return spec, synth.make_params(spec, 1)


def _fused7(net):
    return [ln.split()[1] for ln in net.describe().splitlines() if 'fused_dws7:' in ln]


def _fused(net):
    return [ln.split()[1] for ln in net.describe().splitlines() if 'fused_dws:' in ln]


def _lines7(blocks, pool_on_last=False):
    out = [f'fused_dws7:{b}.body.0+{b}.body.2' for b in blocks]
    if pool_on_last:
        out[-1] += '+avgpool'
    return out


def _ops(net, n):
    return sum(net.launch_info(i, n)[2] for i in range(net.num_launches))


def test_option_off_is_todays_plan(mbv1):
    spec, params = mbv1
    plain = build_net(spec, params, max_batch=128, hw=224)
    off = build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws7': 0})
    assert plain.get_option('fuse_dws7') == 0
    assert plain.num_launches == 30 and off.num_launches == 30
    assert plain.describe() == off.describe() and 'fused_dws7:' not in plain.describe()
    # ... and fuse_dws alone is fuse_dws' plan
    dws = build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws': 1})
    assert dws.describe() == build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws': 1, 'fuse_dws7': 0}).describe()
    assert 'fused_dws7:' not in dws.describe()


@pytest.mark.parametrize('both', [False, True], ids=['alone', 'with_fuse_dws'])
def test_mobilenet_v1_224(mbv1, both):
    spec, params = mbv1
    base = {'fuse_dws': 1} if both else {}
    off = build_net(spec, params, max_batch=128, hw=224, options=base)
    on = build_net(spec, params, max_batch=128, hw=224, options=dict(base, fuse_dws7=1))
    assert off.num_launches == (19 if both else 30) and on.num_launches == (16 if both else 27)
    assert _fused7(on) == _lines7(BLOCKS[11:], pool_on_last=True)
    assert _fused(on) == _fused(off) and len(_fused(on)) == (11 if both else 0)      # stage_3_layer_5, read by a dws7 block, stays fused
    assert 'avgpool_sum:' in off.describe() and 'avgpool_sum:' not in on.describe()
    # everything in front of the 7x7 blocks keeps its lines
    head = lambda net: [ln.split(None, 1)[1] for ln in net.describe().splitlines() if 'stage_' in ln and 'stage_4_layer_' not in ln]
    assert head(on) == head(off)
    idx = [i for i in range(on.num_launches) if on.launch_info(i, 1)[0].startswith('fused_dws7:')]
    assert len(idx) == 2 and all(on.launch_kernel(i).startswith('f8::dws7_kernel<') for i in idx)
    assert on.launch_kernel(idx[0]).endswith('false>') and on.launch_kernel(idx[1]).endswith('true>')       # POOL
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    for i in idx:
        assert f'void {on.launch_kernel(i)}(f8::Dws7Args)' in syms, on.launch_kernel(i)
    assert _ops(on, 128) == pytest.approx(_ops(off, 128), rel=1e-12)
    assert on.arena_bytes <= off.arena_bytes
    for i in idx:
        assert on.launch_valu(i, 128) > 0


def test_other_sizes(mbv1):
    """112: the six blocks of stage 3 sit on 7x7 maps (the 4x4 blocks behind them and their pool stay); 64: no 7x7 map at all."""
    spec, params = mbv1
    off = build_net(spec, params, max_batch=8, hw=112)
    on = build_net(spec, params, max_batch=8, hw=112, options={'fuse_dws7': 1})
    assert _fused7(on) == _lines7(BLOCKS[5:11])
    assert on.num_launches == off.num_launches - 6
    keep = lambda net: [ln.split(None, 1)[1] for ln in net.describe().splitlines() if 'stage_4_layer_' in ln or 'avgpool' in ln]
    assert len(keep(on)) == 5 and keep(on) == keep(off)
    off = build_net(spec, params, max_batch=8, hw=64)
    on = build_net(spec, params, max_batch=8, hw=64, options={'fuse_dws7': 1})
    assert not _fused7(on) and on.describe() == off.describe()


@pytest.mark.parametrize('arch', ['mobilenet_v2', 'resnet18', 'resnet50'])
def test_other_nets_keep_their_plans(arch):
    spec = topology.get(arch)
    params = synth.make_params(spec, 1)
    off = build_net(spec, params, max_batch=8, hw=224)
    on = build_net(spec, params, max_batch=8, hw=224, options={'fuse_dws7': 1})
    assert on.describe() == off.describe()


def test_environment_seeds_a_new_handle():
    code = ('from f8net_amd import synth, topology; from f8net_amd.net import build_net; s = topology.get("mobilenet_v1"); '
            'n = build_net(s, synth.make_params(s, 1), max_batch=4, hw=224); print(n.get_option("fuse_dws7"), n.get_option("fuse_dws"), n.num_launches)')
    env = dict(os.environ, F8_FUSE_DWS7='1')
    env.pop('F8_FUSE_DWS', None)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))).stdout.split()
    assert out == ['1', '0', '27']


def _graph(hw=7, cout=32, cin=32, second_reader=False, join=False, block_is_output=False, pool=False, pool_is_output=False, pool_and_conv=False,
           finalize=True):
    """pre 1x1 -> depthwise 3x3 -> 1x1 -> [average pool -> linear | a 1x1 reader]; the last int32 result is the net output.  32 channels
    (cin: those of the depthwise conv)."""
    rng = np.random.default_rng(0)
    w = lambda *s: rng.integers(-20, 20, s).astype(np.int32)
    conv = lambda net, t, cin, co, fl, sgn, relu: net.conv(t, w(co, cin, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=fl,
                                                           input_signed=sgn, quant_input=True, relu=relu)
    net = F8Net()
    t = net.input(32, hw, hw, 5)
    t = conv(net, t, 32, cin, 5, True, True)
    d = net.conv(t, w(cin, 1, 3, 3), None, stride=1, pad=1, groups=cin, weight_fl=6, input_fl=6, input_signed=False, quant_input=True, relu=True)
    p = conv(net, d, cin, cout, 6, False, not join)
    if join:
        p = net.add(p, t)
    out = p
    if pool or pool_is_output or pool_and_conv:
        out = net.avgpool_sum(p, 6, label='pool')
        if not pool_is_output:
            out = net.linear(out, w(32, cout), None, weight_fl=6, input_fl=4, input_signed=False)
        if pool_and_conv:
            out = net.add(net.avgpool_sum(conv(net, p, cout, 32, 4, False, False), 6), out)
    elif not block_is_output:
        out = conv(net, p, cout, 32, 4, join, False)
    if second_reader:
        x = conv(net, d, cin, 32, 5, False, False)
        out = net.add(out, x)
    net.output(out, as_float=False)
    net.set_option('fuse_dws7', 1)
    return net.finalize(2) if finalize else net


def test_graph_cuts():
    assert _fused7(_graph()) == ['fused_dws7:t2+t3']
    assert len(_fused7(_graph(cout=48))) == 1                      # an output channel count that is no multiple of 32 is padded like any conv's
    assert not _fused7(_graph(second_reader=True))                 # the depthwise result has a second reader
    assert not _fused7(_graph(join=True))                          # the 1x1 carries a residual join
    assert not _fused7(_graph(block_is_output=True))               # the block output is the net output (int32)
    assert not _fused7(_graph(hw=8))                               # an 8x8 map
    assert not _fused7(_graph(hw=14)) and not _fused7(_graph(hw=28))      # (fuse_dws' maps)


def test_a_depthwise_conv_of_48_channels_stays_two_launches():
    """Pass 1k asks for whole 32-channel slices of real channels on the depthwise side.  The 48-channel block input has a 64-channel form, which
    the launch's shape check (asked with the padded count) would take: only the planner's own term keeps the block two launches."""
    net = _graph(cin=48)
    assert not _fused7(net)
    assert 'dwconv3x3s1:' in net.describe(), net.describe()
    assert len(_fused7(_graph(cin=64))) == 1


def test_pool_fold_and_its_cuts():
    net = _graph(pool=True)
    assert _fused7(net) == ['fused_dws7:t2+t3+pool'] and 'avgpool_sum:' not in net.describe()
    assert any(net.launch_kernel(i).startswith('f8::dws7_kernel<1, ') and net.launch_kernel(i).endswith(', true>') for i in range(net.num_launches))
    # the pooled tensor is the net output: the pool stays a launch of its own, and the block — whose int32 result it reads — two launches
    net = _graph(pool_is_output=True)
    assert not _fused7(net) and 'avgpool_sum:' in net.describe() and 'dwconv3x3s1:' in net.describe()
    # the pool is not the only reader: it needs the int32 form, which this launch does not write — not fused at all
    net = _graph(pool_and_conv=True)
    assert not _fused7(net) and 'avgpool_sum:' in net.describe() and 'dwconv3x3s1:' in net.describe()


def test_option_is_fixed_at_finalize_and_range_checked():
    net = _graph(finalize=False)
    with pytest.raises(Exception):
        net.set_option('fuse_dws7', 2)
    net.finalize(2)
    with pytest.raises(Exception):
        net.set_option('fuse_dws7', 0)
    L = _lib.lib()
    assert L.f8_net_set_option(net._h, b'fuse_dws7', 1) == -5         # F8_ERR_STATE
    fresh = F8Net()
    assert L.f8_net_set_option(fresh._h, b'fuse_dws7', 2) == -1       # F8_ERR_INVALID
    assert L.f8_net_set_option(fresh._h, b'fuse_dws7', 1) == 0
