"""fuse_dws (planning option, off by default): which MobileNet-V1 depthwise-separable blocks the planner runs as one launch (no GPU)."""
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


def _fused(net):
    return [ln.split()[1] for ln in net.describe().splitlines() if 'fused_dws:' in ln]


def _lines(blocks):
    return [f'fused_dws:{b}.body.0+{b}.body.2' for b in blocks]


def _ops(net, n):
    return sum(net.launch_info(i, n)[2] for i in range(net.num_launches))


def test_option_off_is_todays_plan(mbv1):
    spec, params = mbv1
    plain = build_net(spec, params, max_batch=128, hw=224)
    off = build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws': 0})
    assert plain.get_option('fuse_dws') == 0
    assert plain.num_launches == 30 and off.num_launches == 30
    assert plain.describe() == off.describe() and 'fused_dws:' not in plain.describe()


def test_mobilenet_v1_224_eleven_blocks(mbv1):
    spec, params = mbv1
    off = build_net(spec, params, max_batch=128, hw=224)
    on = build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws': 1})
    assert off.num_launches == 30 and on.num_launches == 19
    assert _fused(on) == _lines(BLOCKS[:11])
    # the two blocks on 7-wide maps keep today's lines
    keep = lambda net: [ln.split(None, 1)[1] for ln in net.describe().splitlines() if 'stage_4_layer_' in ln]
    assert len(keep(on)) == 4 and keep(on) == keep(off)
    idx = [i for i in range(on.num_launches) if on.launch_info(i, 1)[0].startswith('fused_dws:')]
    assert len(idx) == 11 and all(on.launch_kernel(i).startswith('f8::dws_kernel<') for i in idx)
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    for i in idx:
        assert f'void {on.launch_kernel(i)}(f8::DwsArgs)' in syms, on.launch_kernel(i)
    assert _ops(on, 128) == pytest.approx(_ops(off, 128), rel=1e-12)
    assert on.arena_bytes <= off.arena_bytes
    for i in idx:
        assert on.launch_valu(i, 128) > 0


@pytest.mark.parametrize('hw,blocks', [(112, [BLOCKS[i] for i in (0, 1, 2, 3, 4)]), (64, [BLOCKS[0]])])
def test_other_sizes(mbv1, hw, blocks):
    """112: output maps 56, 28, 28, 14, 14 (then 7 and narrower); 64: 32 (then 16, 8, ...: neither >= 28 nor 14)."""
    spec, params = mbv1
    off = build_net(spec, params, max_batch=8, hw=hw)
    on = build_net(spec, params, max_batch=8, hw=hw, options={'fuse_dws': 1})
    assert _fused(on) == _lines(blocks)
    assert on.num_launches == off.num_launches - len(blocks)


@pytest.mark.parametrize('arch', ['mobilenet_v2', 'resnet18', 'resnet50'])
def test_other_nets_keep_their_plans(arch):
    spec = topology.get(arch)
    params = synth.make_params(spec, 1)
    off = build_net(spec, params, max_batch=8, hw=224)
    on = build_net(spec, params, max_batch=8, hw=224, options={'fuse_dws': 1})
    assert on.describe() == off.describe()


def test_environment_seeds_a_new_handle():
    code = ('from f8net_amd import synth, topology; from f8net_amd.net import build_net; s = topology.get("mobilenet_v1"); '
            'n = build_net(s, synth.make_params(s, 1), max_batch=4, hw=224); print(n.get_option("fuse_dws"), n.num_launches)')
    env = dict(os.environ, F8_FUSE_DWS='1')
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))).stdout.split()
    assert out == ['1', '19']


def _graph(hw=28, cout=32, cin=32, second_reader=False, dw_is_output=False, join=False, int32_output=False, finalize=True):
    """pre 1x1 -> depthwise 3x3 -> 1x1 (-> a 1x1 reader whose int32 result is the net output), 32 channels (cin: those of the depthwise conv)."""
    rng = np.random.default_rng(0)
    w = lambda *s: rng.integers(-20, 20, s).astype(np.int32)
    net = F8Net()
    t = net.input(32, hw, hw, 5)
    t = net.conv(t, w(cin, 32, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=5, input_signed=True, quant_input=True, relu=True)
    d = net.conv(t, w(cin, 1, 3, 3), None, stride=1, pad=1, groups=cin, weight_fl=6, input_fl=6, input_signed=False, quant_input=True, relu=True)
    p = net.conv(d, w(cout, cin, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=6, input_signed=False, quant_input=True, relu=not join)
    if join:
        p = net.add(p, t)
    out = p
    if not int32_output:
        out = net.conv(p, w(32, cout, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=join, quant_input=True, relu=False)
    if second_reader:
        x = net.conv(d, w(32, cin, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=5, input_signed=False, quant_input=True, relu=False)
        out = net.add(out, x)
    net.output(d if dw_is_output else out, as_float=False)
    net.set_option('fuse_dws', 1)
    return net.finalize(2) if finalize else net


def test_graph_cuts():
    assert len(_fused(_graph())) == 1
    assert len(_fused(_graph(cout=48))) == 1                       # an output channel count that is no multiple of 32 is padded like any conv's
    assert not _fused(_graph(second_reader=True))                  # the depthwise result has a second reader
    assert not _fused(_graph(dw_is_output=True))                   # ... is the net output
    assert not _fused(_graph(join=True))                           # the 1x1 carries a residual join
    assert not _fused(_graph(hw=7))                                # a 7-wide map
    assert len(_fused(_graph(hw=14))) == 1


def test_a_depthwise_conv_of_48_channels_stays_two_launches():
    """Pass 1j asks for whole 32-channel slices of real channels on the depthwise side.  The 48-channel block input has a 64-channel form, which
    the launch's shape check (asked with the padded count) would take: only the planner's own term keeps the block two launches."""
    net = _graph(hw=14, cin=48)
    assert not _fused(net)
    assert 'dwconv3x3s1:' in net.describe(), net.describe()
    assert len(_fused(_graph(hw=14, cin=64))) == 1


def test_int32_net_output_stays_two_launches():
    net = _graph(int32_output=True)
    plan = net.describe()
    assert not _fused(net)
    assert 'dwconv3x3s1:' in plan and 'conv1x1' in plan, plan


def test_option_is_fixed_at_finalize_and_range_checked():
    net = _graph(finalize=False)
    with pytest.raises(Exception):
        net.set_option('fuse_dws', 2)
    net.finalize(2)
    with pytest.raises(Exception):
        net.set_option('fuse_dws', 0)
    L = _lib.lib()
    assert L.f8_net_set_option(net._h, b'fuse_dws', 1) == -5          # F8_ERR_STATE
    fresh = F8Net()
    assert L.f8_net_set_option(fresh._h, b'fuse_dws', 2) == -1        # F8_ERR_INVALID
    assert L.f8_net_set_option(fresh._h, b'fuse_dws', 1) == 0
