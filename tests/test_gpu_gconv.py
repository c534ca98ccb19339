"""Grouped convolutions (1 < groups < cin) on the device, bit for bit against the reference of tests/gconv_cases.py (the CPU oracle per group): every
case with `grouped = 1` (f8::gconv3x3_kernel<S>, f8_gconv.hip, where the shape is in its set) and, on the same graph and input, with `grouped = 2`
(the dense expansion on conv_igemm_kernel); the two legs also against each other; one handle at several batch sizes; bench.py's pipelined schedule; a
tap on the grouped result and the profiled run; the op-level drop-in; a ResNeXt-style net recorded as an IntGraph and ResNeXt-50 through build_net.
tests/test_gconv_plan.py checks on the CPU that every case is live on the reference's values."""
import numpy as np
import pytest
import torch

import gconv_cases
from f8net_amd import synth, topology
from f8net_amd.net import build_net
from f8net_amd.onnx_import import IntGraph, IntOp
from oracle import oracle
from ref_ops import grouped_conv2d

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _both_legs(name, case, dev, batches=None, x=None):
    x = gconv_cases.make_input(name, case) if x is None else x
    xt = torch.from_numpy(x).to(dev)
    outs = {}
    for leg in gconv_cases.LEGS:
        g, out, _ = gconv_cases.plan(name, case, x, leg)
        assert gconv_cases.lines_match(gconv_cases.g_lines(g.net), gconv_cases.expect(case, leg)), g.net.describe()
        want = g.v[out][0]
        for n in batches or [x.shape[0]]:
            got = g.net.run(xt[:n]).cpu().numpy().reshape((n,) + want.shape[1:])
            np.testing.assert_array_equal(got, want[:n], err_msg=f'{name} grouped={leg} n={n}')
            outs[leg] = got
        g.net.check()
    np.testing.assert_array_equal(outs[1], outs[2], err_msg=name)
    return outs


@pytest.mark.parametrize('name', sorted(gconv_cases.GEOMETRY))
def test_geometry(name, dev):
    _both_legs(name, gconv_cases.GEOMETRY[name], dev)


@pytest.mark.parametrize('name', sorted(gconv_cases.CHANNELS))
def test_channels(name, dev):
    _both_legs(name, gconv_cases.CHANNELS[name], dev)


@pytest.mark.parametrize('name', sorted(gconv_cases.DENSE))
def test_dense_expansion_outside_the_kernels_set(name, dev):
    _both_legs(name, gconv_cases.DENSE[name], dev)


@pytest.mark.parametrize('name', sorted(gconv_cases.XTALK))
def test_no_cross_talk_between_groups(name, dev):
    """A signed input that is zero outside one group: every output channel outside that group is its bias, exactly."""
    case = gconv_cases.XTALK[name]
    outs = _both_legs(name, case, dev)
    cg, gi = case['cg'], case['only_group']
    outside = np.ones(case['C'], bool)
    outside[gi * cg:(gi + 1) * cg] = False
    b = gconv_cases.biases(case)
    for leg in gconv_cases.LEGS:
        assert (outs[leg][:, outside] == b[outside][None, :, None, None]).all(), leg


@pytest.mark.parametrize('name', sorted(gconv_cases.FORMATS))
def test_formats(name, dev):
    _both_legs(name, gconv_cases.FORMATS[name], dev)


@pytest.mark.parametrize('s', [1, 2])
def test_requant_float_changes_nothing(s, dev):
    """requant_float = 1: the same kernel symbol (the kernel requantises in the integer form) and the same values as the default plan."""
    x = gconv_cases.make_input(f's{s}_9x11', gconv_cases.GEOMETRY[f's{s}_9x11'])
    a = _both_legs(f's{s}_9x11', gconv_cases.GEOMETRY[f's{s}_9x11'], dev, x=x)
    b = _both_legs(f'f_rq1_s{s}', gconv_cases.FORMATS[f'f_rq1_s{s}'], dev, x=x)
    np.testing.assert_array_equal(a[1], b[1])


def test_fewer_images_than_max_batch(dev):
    """Planned for 8 images; 3 images (sub-batches of 2 and 1), then 8 from the same handle."""
    _both_legs('max_batch', gconv_cases.MAX_BATCH_CASE, dev, batches=[3, 8])


@pytest.mark.parametrize('leg', gconv_cases.LEGS)
def test_pipelined_schedule(leg, dev):
    """bench.py's schedule on grouped 3x3 / 1 -> 1x1 -> grouped 3x3 / 2: whole-batch launches, three arena copies, runs in flight
    (set_pipelined(2)), three inputs rotating over nine runs; every output against the reference."""
    case = gconv_cases.PIPELINED_CASE
    xs = [gconv_cases.make_input(f'pipelined{i}', case) for i in range(3)]
    g, out, _ = gconv_cases.plan('pipelined', case, xs[0], leg)
    assert gconv_cases.lines_match(gconv_cases.g_lines(g.net), gconv_cases.expect(case, leg)), g.net.describe()
    wants = [g.v[out][0]] + [gconv_cases.build_graph(case, x)[0].v[out][0] for x in xs[1:]]
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=outs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(outs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    g.net.check()


@pytest.mark.parametrize('leg', gconv_cases.LEGS)
def test_tap_on_the_grouped_result_and_the_profiled_run(leg, dev):
    """f8_net_output on the grouped conv's own tensor (the launch then writes int32 next to its int8 form) and f8_net_run_profiled."""
    name, case = 's2_9x11', gconv_cases.GEOMETRY['s2_9x11']
    x = gconv_cases.make_input(name, case)
    g, out, ids = gconv_cases.build_graph(case, x, leg)
    assert g.net.output(ids[0], as_float=False) == 1
    g.net.finalize(3)
    xt = torch.from_numpy(x).to(dev)
    y, tap = g.net.run(xt)
    np.testing.assert_array_equal(y.cpu().numpy().reshape(g.v[out][0].shape), g.v[out][0])
    np.testing.assert_array_equal(tap.cpu().numpy(), g.v[ids[0]][0])
    (y2, tap2), ms = g.net.run_profiled(xt)
    assert torch.equal(y2, y) and torch.equal(tap2, tap)
    assert len(ms) == g.net.num_launches and all(m >= 0.0 for m in ms)
    g.net.check()


@pytest.mark.parametrize('C, G, stride', [(40, 5, 2), (64, 2, 1)])
def test_op_level_conv2d(dev, C, G, stride):
    """F8Conv2d / torch.ops.f8net.conv2d on int32 NCHW device tensors: the op accepts the groups by itself and returns the int32 result."""
    from f8net_amd import ops
    N, H, W = 3, 9, 11
    x = synth.rand_uniform_int(11, f'gop_x{C}', (N, C, H, W), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(12, f'gop_w{C}', (C, C // G, 3, 3), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(13, f'gop_b{C}', (C,), 3e5).astype(np.int32)
    conv = ops.F8Conv2d(C, C, 3, stride=stride, padding=1, groups=G)
    conv.weight.data, conv.bias.data = torch.from_numpy(w), torch.from_numpy(b)
    conv.input_fraclen.fill_(5)
    conv.weight_fraclen.fill_(6)
    got = conv(torch.from_numpy(x).to(dev)).cpu().numpy()
    want = grouped_conv2d(x, w, b, stride, 1, G)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


# ---- net level: a ResNeXt-style net recorded op by op as an IntGraph (what the ONNX importer hands to build_net)

def _w(key, shape, sig):
    return np.clip(synth.rand_normal_int(7, f'rx_w_{key}', shape, sig), -127, 127).astype(np.int32)


def _b(key, n, sig, mean):
    return (synth.rand_normal_int(8, f'rx_b_{key}', (n,), sig) + int(mean)).astype(np.int32)


def resnext_graph():
    """head 3x3 / 2 on 3 x 32 x 32 -> max-pool -> an opening bottleneck around a grouped 3x3 / 1 (32 -> mid 64 in 8 groups -> 128, 1x1 shortcut) -> an
    identity bottleneck -> a stride-2 opening bottleneck around a grouped 3x3 / 2 (mid 128 in 8 groups -> 256) -> average pool -> linear to 10 classes.
    Every conv requantises its input to unsigned 8 bits by a right shift chosen from the spread of the weights."""
    ops = [IntOp('input', shape=(3, 32, 32))]

    def conv(src, key, cout, cin, k, stride, shift, w_sig, b_mean, groups=1, relu=True):
        ops.append(IntOp('conv', src=src, weight=_w(key, (cout, cin // groups, k, k), w_sig), bias=_b(key, cout, abs(b_mean) / 4 + 16, b_mean),
                         stride=stride, pad=k // 2, groups=groups, kernel=k, shift=shift, signed=False, relu=relu, key=key))
        return len(ops) - 1

    def block(x, name, cin, mid, cout, stride, groups, shortcut):
        t = conv(x, f'{name}.body.0', mid, cin, 1, 1, 7, 12.0 * (32.0 / cin) ** 0.5, 2.0 ** 11)
        t = conv(t, f'{name}.body.2', mid, mid, 3, stride, 7, 14.0 * (8.0 * groups / mid) ** 0.5, 2.0 ** 11, groups=groups)
        t = conv(t, f'{name}.body.4', cout, mid, 1, 1, 7, 8.0 * (64.0 / mid) ** 0.5, 0.0, relu=False)
        s = conv(x, f'{name}.shortcut.0', cout, cin, 1, stride, 7, 12.0 * (32.0 / cin) ** 0.5, 0.0, relu=False) if shortcut else x
        ops.append(IntOp('add', src=t, src2=s, shift=0, relu=True))
        return len(ops) - 1

    t = conv(0, 'head.0', 32, 3, 3, 2, None, 16.0, 2.0 ** 11)
    ops.append(IntOp('maxpool', src=t, kernel=3, stride=2, pad=1))
    t = len(ops) - 1
    t = block(t, 'stage_0_layer_0', 32, 64, 128, 1, 8, True)
    t = block(t, 'stage_0_layer_1', 128, 64, 128, 1, 8, False)
    t = block(t, 'stage_1_layer_0', 128, 128, 256, 2, 8, True)
    ops.append(IntOp('avgpool', src=t))
    t = len(ops) - 1
    ops.append(IntOp('linear', src=t, weight=_w('fc', (10, 256), 30.0), bias=_b('fc', 10, 2.0 ** 10, 0.0), shift=12, signed=False, key='classifier.1'))
    return IntGraph(ops=ops, output=len(ops) - 1, output_float=False, input_signed=False)


def test_resnext_style_net_through_build_net(dev):
    ig = resnext_graph()
    x = synth.rand_uniform_int(9, 'rx_x', (3, 3, 32, 32), 0, 255).astype(np.int32)
    with gconv_cases.grouped_oracle():
        want = oracle.graph_forward(ig, x)
    assert np.unique(want).size > 8
    xt = torch.from_numpy(x).to(dev)
    for options, toks in ((None, ('gconv3x3s1:', 'gconv3x3s2:')), ({'grouped': 2}, ('gconv3x3s1_dense:', 'gconv3x3s2_dense:'))):
        net = ig.build_net(4, options=options)
        plan = net.describe()
        assert all(t in plan for t in toks), plan
        got = net.run(xt).cpu().numpy()
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=str(options))
        net.check()


def test_resnext50_through_build_net(dev):
    """ResNeXt-50 32x4d at 64 x 64, two images: all sixteen grouped layers on the new kernel, against net_forward on the per-group reference."""
    spec = topology.get('resnext50_32x4d')
    params = synth.make_params(spec, seed=31)
    x, x_fl = synth.make_input(spec, params, 2, 64, seed=3)
    with gconv_cases.grouped_oracle():
        want = oracle.net_forward(spec, params, x, x_fl)
    assert np.unique(want).size > 8
    net = build_net(spec, params, 2, hw=64)
    assert sum(net.launch_info(i, 1)[0].startswith('gconv3x3s') and '_dense' not in net.launch_info(i, 1)[0] for i in range(net.num_launches)) == 16
    xt = torch.from_numpy(x).to(dev)
    for _ in range(2):
        got = net.run(xt).cpu().numpy()
        net.check()
        np.testing.assert_array_equal(got, want)
