"""Large depthwise convs (kernel 8 .. 31, option dw_large) on the device, bit for bit against the CPU oracle: every case of tests/dwlk_cases.py on
dwlk_kernel (f8_dwlk.hip, dw_large = 1) and on dwconvk_kernel (dw_large = 2), the two legs against each other; the op-level drop-in; a RepLKNet-style
net recorded as an IntGraph.  tests/test_dwlk_plan.py checks on the CPU that every case is live on the oracle's values."""
import numpy as np
import pytest
import torch

import dwlk_cases as lc
from f8net_amd import synth
from f8net_amd.onnx_import import IntGraph, IntOp
from ir_cases import _b, _w
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _all_legs(name, case, dev, batches=None):
    x = lc.make_input(name, case)
    xt = torch.from_numpy(x).to(dev)
    outs = {}
    for leg in lc.LEGS:
        g, out, _ = lc.plan(case, x, leg)
        assert [ln[1:] for ln in lc.dw_lines(g.net)] == lc.expect(case, leg), g.net.describe()
        want = g.v[out][0]
        for n in batches or [x.shape[0]]:
            outs[leg] = g.net.run(xt[:n]).cpu().numpy().reshape((n,) + want.shape[1:])
            np.testing.assert_array_equal(outs[leg], want[:n], err_msg=f'{name} leg={leg} n={n}')
        g.net.check()
    np.testing.assert_array_equal(outs['own'], outs['generic'])


@pytest.mark.parametrize('name', sorted(lc.CASES))
def test_case(name, dev):
    _all_legs(name, lc.CASES[name], dev)


def test_fewer_images_than_max_batch(dev):
    """Planned for 8 images; 3 images, then 8 from the same handle."""
    _all_legs('max_batch', lc.MAX_BATCH_CASE, dev, batches=[3, 8])


def test_pipelined_schedule(dev):
    """bench.py's schedule on depthwise 13x13 -> 1x1 -> depthwise 9x9: whole-batch launches, three arena copies, runs in flight, three inputs
    rotating over nine runs; every output against the oracle."""
    case = lc.PIPELINED_CASE
    xs = [lc.make_input(f'pipelined{i}', case) for i in range(3)]
    g, out, _ = lc.plan(case, xs[0])
    assert [ln[1:] for ln in lc.dw_lines(g.net)] == lc.expect(case), g.net.describe()
    wants = [g.v[out][0]] + [lc.build_graph(case, x)[0].v[out][0] for x in xs[1:]]
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=outs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(outs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')


def test_op_level_conv2d(dev):
    """F8Conv2d on int32 NCHW device tensors opts in by itself; the op returns the int32 result."""
    from f8net_amd import ops
    C, N, K = 40, 3, 13
    x = synth.rand_uniform_int(11, 'dwlkop_x', (N, C, 14, 14), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(12, 'dwlkop_w', (C, 1, K, K), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(13, 'dwlkop_b', (C,), 3e5).astype(np.int32)
    conv = ops.F8Conv2d(C, C, K, padding=6, groups=C)
    conv.weight.data, conv.bias.data = torch.from_numpy(w), torch.from_numpy(b)
    conv.input_fraclen.fill_(5)
    conv.weight_fraclen.fill_(6)
    got = conv(torch.from_numpy(x).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.conv2d(x, w, b, 1, 6, C))


def replk_graph():
    """stem 3x3 / 2 on 3 x 32 x 32 -> [1x1 -> depthwise 13x13 -> 1x1, + the block input] -> transition 3x3 / 2 -> [1x1 -> depthwise 9x9 -> 1x1, + input]
    -> average pool -> linear to 10 classes.  Every conv requantises its input to unsigned 8 bits by a right shift chosen from the spread of the
    weights (a sum over T taps of w * x has a spread near sqrt(T) * sigma_w * |x|)."""
    ops = [IntOp('input', shape=(3, 32, 32))]

    def conv(src, key, cout, cin, k, stride, shift, w_sig, b_mean, groups=1, relu=True):
        ops.append(IntOp('conv', src=src, weight=_w(2 * len(ops), (cout, cin // groups, k, k), w_sig), bias=_b(2 * len(ops) + 1, cout, abs(b_mean) / 4 + 16, b_mean),
                         stride=stride, pad=k // 2, groups=groups, kernel=k, shift=shift, signed=False, relu=relu, key=key))
        return len(ops) - 1

    def block(src, key, C, k):
        t = conv(src, f'{key}.pw1', C, C, 1, 1, 7, 12.0, 2.0 ** 11)
        t = conv(t, f'{key}.dw', C, C, k, 1, 7, 36.0 / k, 2.0 ** 12, groups=C)
        t = conv(t, f'{key}.pw2', C, C, 1, 1, 7, 8.0, 0.0, relu=False)
        ops.append(IntOp('add', src=t, src2=src, shift=0))
        return len(ops) - 1

    t = conv(0, 'stem', 48, 3, 3, 2, None, 16.0, 2.0 ** 11)
    t = block(t, 'b0', 48, 13)
    t = conv(t, 'trans', 96, 48, 3, 2, 7, 6.0, 2.0 ** 11)
    t = block(t, 'b1', 96, 9)
    ops.append(IntOp('avgpool', src=t))
    ops.append(IntOp('linear', src=len(ops) - 1, weight=_w(98, (10, 96), 30.0), bias=_b(99, 10, 2.0 ** 10, 0.0), shift=12, signed=False, key='classifier.1'))
    return IntGraph(ops=ops, output=len(ops) - 1, output_float=False, input_signed=False)


def test_replknet_style_net_through_build_net(dev):
    ig = replk_graph()
    x = synth.rand_uniform_int(9, 'lk_x', (3, 3, 32, 32), 0, 255).astype(np.int32)
    want = oracle.graph_forward(ig, x)
    assert np.unique(want).size > 8
    net = ig.build_net(4, options=None)
    plan = net.describe()
    assert 'dwconv13x13s1:' in plan and 'dwconv9x9s1:' in plan and net.get_option('dw_large') == 1, plan
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got.reshape(want.shape), want)
    net.check()
