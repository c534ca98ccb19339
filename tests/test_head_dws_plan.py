"""fuse_head_dws (planning option, off by default): MobileNet-V1's head conv and first depthwise-separable block as one launch (no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

HEAD = 'conv3x3s2_t128x32x32_stem:head.0'
FUSED = 'head3x3s2+dw3x3+1x1:head.0+stage_0_layer_0.body.0+stage_0_layer_0.body.2'
RAW_INPUT = 'input(read by the stem launch)'
BLOCKS = ['stage_0_layer_0', 'stage_1_layer_0', 'stage_1_layer_1', 'stage_2_layer_0', 'stage_2_layer_1'] + \
         [f'stage_3_layer_{i}' for i in range(6)] + ['stage_4_layer_0', 'stage_4_layer_1']


@pytest.fixture(scope='module')
def mbv1():
    spec = topology.get('mobilenet_v1')
    return spec, synth.make_params(spec, 1)


def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _kernel_launches(net):
    """Steps that start a kernel: the input step launches nothing when the head launch reads the caller's buffer itself."""
    return sum(1 for n in _names(net) if n != RAW_INPUT)


def _ops(net, n):
    return sum(net.launch_info(i, n)[2] for i in range(net.num_launches))


def test_option_off_is_todays_plan(mbv1):
    spec, params = mbv1
    plain = build_net(spec, params, max_batch=128, hw=224)
    off = build_net(spec, params, max_batch=128, hw=224, options={'fuse_head_dws': 0})
    assert plain.get_option('fuse_head_dws') == 0
    assert plain.describe() == off.describe()
    assert plain.num_launches == 30 and off.num_launches == 30
    assert HEAD in _names(plain) and 'head3x3s2+dw3x3+1x1' not in plain.describe()


def test_mobilenet_v1_224(mbv1):
    spec, params = mbv1
    off = build_net(spec, params, max_batch=128, hw=224, options={'fuse_head_dws': 0})
    on = build_net(spec, params, max_batch=128, hw=224, options={'fuse_head_dws': 1})
    assert on.num_launches == 28
    names = _names(on)
    assert names.count(FUSED) == 1 and sum('head3x3s2+dw3x3+1x1:' in ln for ln in on.describe().splitlines()) == 1
    assert names[0] == RAW_INPUT and HEAD not in names
    i = names.index(FUSED)
    sym = on.launch_kernel(i)
    assert sym == 'f8::head_dws_kernel'
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    # the template arguments are the kind of the run's raw input and the 1x1's output tiles: chosen where the launch starts
    for kind in (-1, 0, 1, 2):
        for nt in (1, 2):
            assert f'void {sym}<{kind}, {nt}>(f8::StemPoolArgs)' in syms, (kind, nt)
    assert _ops(on, 128) == pytest.approx(_ops(off, 128), rel=1e-12)
    assert on.arena_bytes <= off.arena_bytes
    assert on.launch_valu(i, 128) > 0
    # every other step is the option-0 plan's
    rest = lambda net: [ln.split(None, 1)[1] for ln in net.describe().splitlines()[:-2] if 'stage_0_layer_0' not in ln and 'head.0' not in ln and 'input' not in ln]
    assert rest(on) == rest(off)


def _fused_dws(net):
    return [ln.split()[1] for ln in net.describe().splitlines() if 'fused_dws:' in ln]


def test_with_fuse_dws_block_0_belongs_to_the_head(mbv1):
    """Pass 1h runs before 1j: block 0 is the head launch's.  The head conv and block 0 become one step instead of two (head.0, fused_dws), and
    the input step launches nothing any more: two kernel launches fewer than fuse_dws alone."""
    spec, params = mbv1
    dws = build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws': 1})
    both = build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws': 1, 'fuse_head_dws': 1})
    assert _kernel_launches(dws) == dws.num_launches == 19
    assert _kernel_launches(both) == _kernel_launches(dws) - 2 and both.num_launches == 18
    assert _names(both).count(FUSED) == 1 and _names(both)[0] == RAW_INPUT
    assert _fused_dws(both) == [f'fused_dws:{b}.body.0+{b}.body.2' for b in BLOCKS[1:11]]
    assert _ops(both, 128) == pytest.approx(_ops(dws, 128), rel=1e-12)


def test_with_fuse_dws_and_fuse_dws7(mbv1):
    spec, params = mbv1
    two = build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws': 1, 'fuse_dws7': 1})
    three = build_net(spec, params, max_batch=128, hw=224, options={'fuse_dws': 1, 'fuse_dws7': 1, 'fuse_head_dws': 1})
    assert _kernel_launches(three) == _kernel_launches(two) - 2
    assert _names(three).count(FUSED) == 1 and len(_fused_dws(three)) == 10
    assert _ops(three, 128) == pytest.approx(_ops(two, 128), rel=1e-12)


@pytest.mark.parametrize('arch', ['mobilenet_v2', 'resnet18', 'resnet50'])
def test_other_nets_keep_their_plans(arch):
    spec = topology.get(arch)
    params = synth.make_params(spec, 1)
    off = build_net(spec, params, max_batch=8, hw=224, options={'fuse_head_dws': 0})
    on = build_net(spec, params, max_batch=8, hw=224, options={'fuse_head_dws': 1})
    assert on.describe() == off.describe()
    if arch == 'mobilenet_v2':                                      # claimed by the existing matcher, run by the existing kernel
        i = [k for k, n in enumerate(_names(on)) if n.startswith('head3x3s2+dw3x3+1x1:')]
        assert len(i) == 1 and on.launch_kernel(i[0]) == 'f8::stem_rows_kernel'


@pytest.mark.parametrize('hw,taken', [(64, True), (112, True), (226, False), (456, False)])
def test_other_sizes(mbv1, hw, taken):
    """226: no multiple of 4; 456: 228 output columns, more than four strips of 28."""
    spec, params = mbv1
    off = build_net(spec, params, max_batch=4, hw=hw, options={'fuse_head_dws': 0})
    on = build_net(spec, params, max_batch=4, hw=hw, options={'fuse_head_dws': 1})
    if taken:
        assert _names(on).count(FUSED) == 1 and on.num_launches == off.num_launches - 2 and _names(on)[0] == RAW_INPUT
    else:
        assert on.describe() == off.describe() and HEAD.split(':')[1] in off.describe()


def test_environment_seeds_a_new_handle():
    code = ('from f8net_amd import synth, topology; from f8net_amd.net import build_net; s = topology.get("mobilenet_v1"); '
            'n = build_net(s, synth.make_params(s, 1), max_batch=4, hw=224); print(n.get_option("fuse_head_dws"), n.num_launches)')
    env = dict(os.environ, F8_FUSE_HEAD_DWS='1')
    for k in ('F8_FUSE_DWS', 'F8_FUSE_DWS7'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))).stdout.split()
    assert out == ['1', '28']


def _graph(on, hw=32, cout=64, relu=True, head_cout=32, dw_stride=1, head_reader=False, dw_reader=False, is_output=False, join=False,
           dw_signed=False, head_w_fl=6, readers=((6, False),)):
    """input (3 channels, unsigned fraclen 8) -> 3x3 / 2 head conv (ReLU) -> depthwise 3x3 (ReLU) -> 1x1 -> one 1x1 reader per format, summed."""
    rng = np.random.default_rng(0)
    w = lambda *s: rng.integers(-20, 20, s).astype(np.int32)
    net = F8Net()
    t = net.input(3, hw, hw, 8)
    h = net.conv(t, w(head_cout, 3, 3, 3), None, stride=2, pad=1, groups=1, weight_fl=head_w_fl, input_fl=8, input_signed=False, quant_input=True, relu=True)
    d = net.conv(h, w(head_cout, 1, 3, 3), None, stride=dw_stride, pad=1, groups=head_cout, weight_fl=6, input_fl=6, input_signed=dw_signed,
                 quant_input=True, relu=True)
    p = net.conv(d, w(cout, head_cout, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=6, input_signed=False, quant_input=True, relu=relu)
    out = None
    if join:                                                        # the block output is an operand of an add: an int32 form
        y = net.conv(p, w(cout, cout, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=6, input_signed=False, quant_input=True, relu=False)
        out = net.add(p, y)
    elif is_output:
        out = p
    else:
        for fl, sgn in readers:
            c = net.conv(p, w(32, cout, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, quant_input=True, relu=False)
            out = c if out is None else net.add(out, c)
    for src in ([h] if head_reader else []) + ([d] if dw_reader else []):      # a second reader: a 1x1 on the same map, summed into the output
        x = net.conv(src, w(32, head_cout, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=5, input_signed=False, quant_input=True, relu=False)
        out = net.add(out, x)
    net.output(out, as_float=False)
    net.set_option('fuse_head_dws', on)
    return net.finalize(2)


def _taken(**kw):
    on, off = _graph(1, **kw), _graph(0, **kw)
    n = sum(1 for ln in _names(on) if ln.startswith('head3x3s2+dw3x3+1x1:'))
    if n == 0:
        assert on.describe() == off.describe()                      # the parent's steps
    else:
        assert 'head3x3s2+dw3x3+1x1:' not in off.describe()
    return n


def test_graphs_the_option_takes():
    assert _taken() == 1
    assert _taken(cout=48) == 1                                     # padded to 64 like any conv's
    assert _taken(cout=32) == 1                                     # one output tile with a ReLU
    assert _taken(cout=64, relu=False) == 1
    assert _taken(readers=((6, False), (5, True))) == 1
    on = _graph(1)
    i = [k for k, n in enumerate(_names(on)) if n.startswith('head3x3s2+dw3x3+1x1:')][0]
    assert on.launch_kernel(i) == 'f8::head_dws_kernel' and on.launch_valu(i, 2) > 0
    # 32 outputs without a ReLU: the existing matcher's form, on the existing kernel, with the option on or off
    v2 = _graph(1, cout=32, relu=False)
    assert v2.describe() == _graph(0, cout=32, relu=False).describe()
    i = [k for k, n in enumerate(_names(v2)) if n.startswith('head3x3s2+dw3x3+1x1:')][0]
    assert v2.launch_kernel(i) == 'f8::stem_rows_kernel'


@pytest.mark.parametrize('why,kw', [
    ('1x1 with 96 outputs', dict(cout=96)),
    ('depthwise stride 2', dict(dw_stride=2)),
    ('head conv with 16 outputs', dict(head_cout=16)),
    ('second reader of the head conv', dict(head_reader=True)),
    ('second reader of the depthwise output', dict(dw_reader=True)),
    ('block output is the net output', dict(is_output=True)),
    ('block output feeds an add', dict(join=True)),
    ('signed depthwise input', dict(dw_signed=True)),
    ('inner shift 17', dict(head_w_fl=15)),
    ('three reader formats', dict(readers=((6, False), (5, False), (5, True)))),
], ids=lambda v: v.replace(' ', '_') if isinstance(v, str) else '')
def test_refusals(why, kw):
    assert _taken(**kw) == 0, why


def test_option_is_fixed_at_finalize_and_range_checked():
    net = _graph(1)
    with pytest.raises(Exception):
        net.set_option('fuse_head_dws', 0)
    fresh = F8Net()
    L = _lib.lib()
    assert L.f8_net_set_option(fresh._h, b'fuse_head_dws', 2) == -1      # F8_ERR_INVALID
    assert L.f8_net_set_option(fresh._h, b'fuse_head_dws', 1) == 0
