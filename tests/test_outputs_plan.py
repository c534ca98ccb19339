"""Several network outputs (f8_net_output called more than once; net.record_net `taps=`): the builder's rules, the queries, where the planner
puts the copy-out launches and what they cost in arena.  No GPU: f8_net_finalize touches no device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net, record_net

from outputs_cases import bottleneck_chain, case_data, record_blocks, stage_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'f8net_amd', 'libf8net.so')
F8_ERR_INVALID, F8_ERR_UNSUPPORTED, F8_ERR_STATE = -1, -2, -5


def _chain_of_convs(n, C=32, hw=4):
    """input -> n 1x1 convs in a row; returns (net, [tensor ids of the convs])."""
    net = F8Net()
    t = net.input(C, hw, hw, 6)
    w = np.eye(C, dtype=np.int32).reshape(C, C, 1, 1)
    ts = []
    for _ in range(n):
        t = net.conv(t, w, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=6, input_signed=True)
        ts.append(t)
    return net, ts


def test_indices_duplicates_and_the_limit():
    net, ts = _chain_of_convs(10)
    assert [net.output(ts[9]), net.output(ts[0], as_float=False), net.output(ts[1])] == [0, 1, 2]
    L, h = net._L, net._h
    assert L.f8_net_num_outputs(h) == 3
    assert L.f8_net_output(h, ts[0], 0) == F8_ERR_INVALID            # the same tensor twice
    assert L.f8_net_output(h, ts[9], 1) == F8_ERR_INVALID
    for k in range(2, 7):
        assert net.output(ts[k]) == k + 1
    assert L.f8_net_num_outputs(h) == 8
    assert L.f8_net_output(h, ts[7], 0) == F8_ERR_UNSUPPORTED        # a ninth output
    assert L.f8_net_num_outputs(h) == 8
    net.finalize(2)
    assert L.f8_net_output(h, ts[8], 0) == F8_ERR_STATE              # after finalize
    assert len(net.outputs) == 8 and net.outputs[0][4] is True and net.outputs[1][4] is False
    with pytest.raises(_lib.F8Error):
        net.output_info(8)


def test_set_output_buffers_wants_every_further_output():
    net, ts = _chain_of_convs(3)
    net.output(ts[2]), net.output(ts[0]), net.output(ts[1])
    L, h = net._L, net._h
    bufs = (ctypes.c_void_p * 3)(4096, 8192, 12288)                  # never dereferenced: nothing runs here
    assert L.f8_net_set_output_buffers(h, bufs, 2) == F8_ERR_STATE   # not finalized yet
    net.finalize(2)
    for n in (0, 1, 3):
        assert L.f8_net_set_output_buffers(h, bufs, n) == F8_ERR_INVALID
    bufs[1] = None
    assert L.f8_net_set_output_buffers(h, bufs, 2) == F8_ERR_INVALID    # a NULL buffer
    single, ts = _chain_of_convs(1)
    single.output(ts[0])
    single.finalize(2)
    assert L.f8_net_set_output_buffers(single._h, None, 0) == 0
    assert L.f8_net_set_output_buffers(single._h, bufs, 1) == F8_ERR_INVALID


@pytest.fixture(scope='module')
def r18():
    spec = topology.get('resnet18')
    return spec, synth.make_params(spec, 1)


def test_output_info_of_a_conv_a_join_and_the_pooled_vector(r18):
    spec, params = r18
    taps = ('stage_1_layer_0.body.0', 'stage_1_layer_1', 'avgpool', 'head.maxpool')
    net = build_net(spec, params, max_batch=2, hw=64, taps=taps)
    assert net.taps == taps and net._L.f8_net_num_outputs(net._h) == 5
    fl = lambda key: int(params[key + '.weight_fraclen']) + int(params[key + '.input_fraclen'][0])
    assert net.outputs[0][:3] == (1000, 1, 1) and net.outputs[0][4] is True and net.outputs[0][3] == net.output_fraclen
    assert net.outputs[1] == (128, 8, 8, fl('stage_1_layer_0.body.0'), False)
    join_fl = net.outputs[2][3]
    assert net.outputs[2][:3] == (128, 8, 8) and join_fl >= fl('stage_1_layer_1.body.2')        # an align-add keeps the larger fraclen
    last = net.output_info(0)
    assert last == net.outputs[0]
    C, H, W, pooled_fl, f = net.outputs[3]
    assert (C, H, W, f) == (512, 1, 1, False)
    feat = build_net(spec, params, max_batch=2, hw=64, taps=('stage_3_layer_1',))
    assert pooled_fl == feat.outputs[1][3] + 6                                                   # FXQAvgPool2d(7): fraclen + 6
    assert net.outputs[4] == (64, 16, 16, fl('head.0'), False)
    # out-pointers may be NULL
    c = ctypes.c_int(0)
    assert net._L.f8_net_output_info(net._h, 1, ctypes.byref(c), None, None, None, None) == 0 and c.value == 128


def test_unknown_tap_name_lists_the_valid_ones(r18):
    spec, params = r18
    with pytest.raises(ValueError) as e:
        record_net(spec, params, 64, taps=('stage_1_layer_1', 'stage_9_layer_0'))
    msg = str(e.value)
    assert 'stage_9_layer_0' in msg and 'stage_1_layer_1.body.0' in msg and 'head.maxpool' in msg and 'avgpool' in msg
    net = record_net(spec, params, 64)
    assert net.tap_ids['avgpool'] > net.tap_ids['stage_3_layer_1'] > net.tap_ids['head.0']


def _tap_steps(net):
    lines = [ln for ln in net.describe().splitlines() if ln[:3].strip().isdigit()]
    names = [ln.split()[1] for ln in lines]
    return names, [i for i, n in enumerate(names) if n.startswith('tap:')]


@pytest.mark.parametrize('arch, hw', [('resnet18', 64), ('resnet50', 224), ('mobilenet_v2', 224), ('mobilenet_v1', 224)])
def test_every_tap_step_follows_its_producer(arch, hw):
    spec = topology.get(arch)
    params = synth.make_params(spec, 1)
    taps = stage_taps(spec)[-4:] + ['avgpool', spec.blocks[1].body[0].key] + (['head.maxpool'] if spec.head_maxpool else [])      # (at most 7 further outputs)
    net = build_net(spec, params, max_batch=8, hw=hw, taps=taps)
    names, at = _tap_steps(net)
    # a step is named by its tensor's label: a block that ends in no join shares its output tensor — and the label — with its last conv
    label = lambda n: next(k for k, t in net.tap_ids.items() if t == net.tap_ids[n])
    assert sorted(names[i][4:] for i in at) == sorted(label(n) for n in taps), net.describe()
    for i in at:
        what = names[i][4:]
        assert i > 0 and not names[i - 1].startswith('tap:') and what in names[i - 1], net.describe()    # e.g. 'stage_chain_x4_tail:..stage_1_layer_3.body.4' / 'requant:<name>'
    assert names[-1].startswith('linear_dense:') and 'output:' not in net.describe()                      # output 0 keeps what it had
    for i in at:
        assert net.launch_kernel(i) == 'f8::tap_kernel<false>'
        assert net.step_launches(i, 8) == net.num_parts(8)                                                # never chunked
    slow = build_net(spec, params, max_batch=8, hw=hw, taps=taps, options={'tap_tiled': 0})
    assert slow.describe() == net.describe()
    for i in at:
        assert slow.launch_kernel(i) == 'f8::output_kernel'


def test_float_tap_names_its_instance_and_output_0_stays_on_output_kernel():
    net, ts = _chain_of_convs(3)
    net.output(ts[2], as_float=False), net.output(ts[0], as_float=True), net.output(ts[1], as_float=False)
    net.finalize(4)
    names, at = _tap_steps(net)
    assert len(at) == 2 and names[-1].startswith('output:')
    assert [net.launch_kernel(i) for i in at] == ['f8::tap_kernel<true>', 'f8::tap_kernel<false>']
    assert net.launch_kernel(len(names) - 1) == 'f8::output_kernel'
    assert net.get_option('tap_tiled') == 1


def test_env_sets_the_default_of_tap_tiled(monkeypatch):
    monkeypatch.setenv('F8_TAP_TILED', '0')
    assert F8Net().get_option('tap_tiled') == 0


def test_a_tap_inside_a_stage_chain_cuts_it():
    case = bottleneck_chain()
    params, _ = case_data(case)
    plain = record_blocks(case['blocks'], params, case['cin'], case['hw'], case['x_fl'], tail=case['tail']).finalize(case['N'])
    assert 'stage_chain_x3' in plain.describe()
    net = record_blocks(case['blocks'], params, case['cin'], case['hw'], case['x_fl'], tail=case['tail'], taps=case['taps']).finalize(case['N'])
    plan = net.describe()
    assert 'stage_chain_x3' not in plan and 'stage_chain_x2:s.1.body.0..s.2.body.4' in plan, plan
    names, at = _tap_steps(net)
    assert [names[i] for i in at] == ['tap:s.0', 'tap:s.2'] and 's.0.body.4' in names[at[0] - 1] and names[at[1] - 1].startswith('stage_chain_x2')


@pytest.mark.parametrize('arch', ['resnet50', 'mobilenet_v2'])
def test_tapped_maps_give_their_arena_back(arch):
    """The int32 form of a tapped map dies at its tap step unless the net reads it again, so the first-fit arena reuses its space: the plan grows by
    less than the tapped forms add up to."""
    spec = topology.get(arch)
    params = synth.make_params(spec, 1)
    bs = 64
    taps = stage_taps(spec)
    plain = build_net(spec, params, max_batch=bs, hw=224)
    net = build_net(spec, params, max_batch=bs, hw=224, taps=taps)
    forms = sum(bs * H * W * ((C + 31) // 32 * 32) * 4 for C, H, W, _, _ in net.outputs[1:])
    assert len(net.outputs) == 1 + len(taps)
    assert plain.arena_bytes <= net.arena_bytes < plain.arena_bytes + forms, (plain.arena_bytes, net.arena_bytes, forms)


@pytest.mark.skipif(shutil.which('gcc') is None, reason='needs gcc')
def test_c99_host_builds_a_two_output_net(tmp_path):
    assert os.path.exists(LIB), 'build libf8net.so first (__graft_entry__.build())'
    exe = str(tmp_path / 'host_outputs')
    cmd = ['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'),
           os.path.join(ROOT, 'examples', 'host_outputs.c'), '-L' + os.path.dirname(LIB), '-lf8net',
           '-Wl,-rpath,' + os.path.dirname(LIB), '-o', exe]
    subprocess.check_call(cmd)
    out = subprocess.check_output([exe], text=True, env=dict(os.environ, LD_LIBRARY_PATH='/opt/rocm/lib:' + os.environ.get('LD_LIBRARY_PATH', '')))
    assert 'output indices 0 1' in out
    assert 'output 0: 32 x 8 x 8 fraclen 11 int32' in out and 'output 1: 32 x 8 x 8 fraclen 11 float32' in out, out
    lines = out.splitlines()
    tap = [i for i, ln in enumerate(lines) if ' tap:' in ln]
    assert len(tap) == 1 and 'conv3x3' in lines[tap[0] - 1] and 'output:' in out, out
