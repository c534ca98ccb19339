"""The general depthwise launches (f8_dwk.hip: kernel 3 / 5 / 7, stride 1 / 2, pad 0 .. kernel / 2 — everything depthwise but 3x3 / pad 1) on the
device, bit for bit against the CPU oracle: every case of tests/dwk_cases.py with its own plan (dwconvk_dot4_kernel<K, S>) and, on the same graph and
input, with dwk_dot4 = 0 (dwconvk_kernel); the op-level drop-in; a MnasNet-style net recorded as an IntGraph.  tests/test_dwk_plan.py checks on
the CPU that every case is live on the oracle's values."""
import numpy as np
import pytest
import torch

import dwk_cases
from f8net_amd import synth
from f8net_amd.onnx_import import IntGraph, IntOp
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _legs(case):
    """The legs that run a kernel no earlier leg of the case runs (an int32 output keeps the generic kernel on both)."""
    seen, legs = [], []
    for leg in dwk_cases.LEGS:
        k = dwk_cases.leg_kernels(case, leg)
        if k not in seen:
            seen.append(k)
            legs.append(leg)
    return legs


def _all_legs(name, case, dev, batches=None, x=None, legs=None):
    x = dwk_cases.make_input(name, case) if x is None else x
    xt = torch.from_numpy(x).to(dev)
    outs = {}
    for leg in legs or _legs(case):
        g, out, _ = dwk_cases.plan(name, case, x, leg)
        assert [ln[1:] for ln in dwk_cases.dw_lines(g.net)] == dwk_cases.expect(case, leg), g.net.describe()
        want = g.v[out][0]
        for n in batches or [x.shape[0]]:
            got = g.net.run(xt[:n]).cpu().numpy().reshape((n,) + want.shape[1:])
            np.testing.assert_array_equal(got, want[:n], err_msg=f'{name} leg={leg} n={n}')
            outs[leg] = got
        g.net.check()
        assert [ln[1:] for ln in dwk_cases.dw_lines(g.net)] == dwk_cases.expect(case, leg)
    return outs


@pytest.mark.parametrize('name', sorted(dwk_cases.GEOMETRY))
def test_geometry(name, dev):
    _all_legs(name, dwk_cases.GEOMETRY[name], dev)


@pytest.mark.parametrize('name', sorted(dwk_cases.PADS))
def test_pads(name, dev):
    _all_legs(name, dwk_cases.PADS[name], dev)


@pytest.mark.parametrize('name', sorted(dwk_cases.CHANNELS))
def test_channels(name, dev):
    _all_legs(name, dwk_cases.CHANNELS[name], dev)


@pytest.mark.parametrize('name', sorted(dwk_cases.FORMATS))
def test_formats(name, dev):
    _all_legs(name, dwk_cases.FORMATS[name], dev)


def test_both_legs_agree_and_requant_float_changes_nothing(dev):
    """One input through dwconvk_dot4_kernel<5, 1>, through dwconvk_kernel and through the plan with requant_float = 1 (the same kernel symbol: the
    general depthwise kernels requantise in the integer form): one value."""
    x = dwk_cases.make_input('k5s1_9x11', dwk_cases.GEOMETRY['k5s1_9x11'])
    a = _all_legs('k5s1_9x11', dwk_cases.GEOMETRY['k5s1_9x11'], dev, x=x, legs=list(dwk_cases.LEGS))
    b = _all_legs('f_rq1_k5s1', dwk_cases.FORMATS['f_rq1_k5s1'], dev, x=x, legs=['own'])
    np.testing.assert_array_equal(a['own'], a['generic'])
    np.testing.assert_array_equal(a['own'], b['own'])


def test_fewer_images_than_max_batch(dev):
    """Planned for 8 images; 3 images (sub-batches of 2 and 1), then 8 from the same handle."""
    _all_legs('max_batch', dwk_cases.MAX_BATCH_CASE, dev, batches=[3, 8])


def test_pipelined_schedule(dev):
    """bench.py's schedule on depthwise 5x5 / 1 -> 1x1 -> depthwise 7x7 / 2: whole-batch launches, three arena copies, runs in flight
    (set_pipelined(2)), three inputs rotating over nine runs; every output against the oracle."""
    case = dwk_cases.PIPELINED_CASE
    xs = [dwk_cases.make_input(f'pipelined{i}', case) for i in range(3)]
    g, out, _ = dwk_cases.plan('pipelined', case, xs[0])
    assert [ln[1:] for ln in dwk_cases.dw_lines(g.net)] == dwk_cases.expect(case), g.net.describe()
    wants = [g.v[out][0]] + [dwk_cases.build_graph(case, x)[0].v[out][0] for x in xs[1:]]
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=outs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(outs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    assert [ln[1:] for ln in dwk_cases.dw_lines(g.net)] == dwk_cases.expect(case)


@pytest.mark.parametrize('K, stride, H, W', [(5, 2, 9, 11), (7, 1, 8, 10)])
def test_op_level_conv2d(dev, K, stride, H, W):
    """F8Conv2d / torch.ops.f8net.conv2d on int32 NCHW device tensors: the op returns the int32 result (dwconvk_kernel)."""
    from f8net_amd import ops
    C, N = 40, 3
    x = synth.rand_uniform_int(11, f'dwkop_x{K}', (N, C, H, W), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(12, f'dwkop_w{K}', (C, 1, K, K), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(13, f'dwkop_b{K}', (C,), 3e5).astype(np.int32)
    conv = ops.F8Conv2d(C, C, K, stride=stride, padding=K // 2, groups=C)
    conv.weight.data, conv.bias.data = torch.from_numpy(w), torch.from_numpy(b)
    conv.input_fraclen.fill_(5)
    conv.weight_fraclen.fill_(6)
    got = conv(torch.from_numpy(x).to(dev)).cpu().numpy()
    want = oracle.conv2d(x, w, b, stride, K // 2, C)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


# ---- net level: a MnasNet-style net recorded op by op as an IntGraph (what the ONNX importer hands to build_net)

def _w(key, shape, sig):
    return np.clip(synth.rand_normal_int(7, f'mnas_w_{key}', shape, sig), -127, 127).astype(np.int32)


def _b(key, n, sig, mean):
    return (synth.rand_normal_int(8, f'mnas_b_{key}', (n,), sig) + int(mean)).astype(np.int32)


def mnas_graph():
    """head 3x3 / 2 on 3 x 32 x 32 -> depthwise-separable 3x3 -> inverted residuals with a 5x5 / 2, a 5x5 / 1 (+ residual) and a 7x7 / 1 depthwise
    conv -> 1x1 tail -> average pool -> linear to 10 classes.  Every conv requantises its input to unsigned 8 bits by a right shift chosen from the
    spread of the weights (sum over T taps of w * x has a spread near sqrt(T) * sigma_w * |x|)."""
    ops = [IntOp('input', shape=(3, 32, 32))]

    def conv(src, key, cout, cin, k, stride, shift, w_sig, b_mean, groups=1, relu=True):
        ops.append(IntOp('conv', src=src, weight=_w(key, (cout, cin // groups, k, k), w_sig), bias=_b(key, cout, abs(b_mean) / 4 + 16, b_mean),
                         stride=stride, pad=k // 2, groups=groups, kernel=k, shift=shift, signed=False, relu=relu, key=key))
        return len(ops) - 1

    t = conv(0, 'head.0', 32, 3, 3, 2, None, 16.0, 2.0 ** 11)
    t = conv(t, 'dws.dw', 32, 32, 3, 1, 8, 24.0, 2.0 ** 11, groups=32)
    b0 = conv(t, 'dws.pw', 24, 32, 1, 1, 7, 12.0, 0.0, relu=False)
    t = conv(b0, 'ir0.expand', 72, 24, 1, 1, 7, 16.0, 2.0 ** 11)
    t = conv(t, 'ir0.dw', 72, 72, 5, 2, 7, 14.0, 2.0 ** 11, groups=72)
    b1 = conv(t, 'ir0.project', 40, 72, 1, 1, 7, 10.0, 0.0, relu=False)
    t = conv(b1, 'ir1.expand', 120, 40, 1, 1, 7, 12.0, 2.0 ** 11)
    t = conv(t, 'ir1.dw', 120, 120, 5, 1, 7, 14.0, 2.0 ** 11, groups=120)
    t = conv(t, 'ir1.project', 40, 120, 1, 1, 7, 8.0, 0.0, relu=False)
    ops.append(IntOp('add', src=t, src2=b1, shift=0))
    b2 = len(ops) - 1
    t = conv(b2, 'ir2.expand', 144, 40, 1, 1, 7, 12.0, 2.0 ** 11)
    t = conv(t, 'ir2.dw', 144, 144, 7, 1, 7, 10.0, 2.0 ** 11, groups=144)
    t = conv(t, 'ir2.project', 64, 144, 1, 1, 7, 8.0, 0.0, relu=False)
    t = conv(t, 'tail', 128, 64, 1, 1, 7, 12.0, 2.0 ** 10)
    ops.append(IntOp('avgpool', src=t))
    t = len(ops) - 1
    ops.append(IntOp('linear', src=t, weight=_w('fc', (10, 128), 30.0), bias=_b('fc', 10, 2.0 ** 10, 0.0), shift=12, signed=False, key='classifier.1'))
    return IntGraph(ops=ops, output=len(ops) - 1, output_float=False, input_signed=False)


def test_mnasnet_style_net_through_build_net(dev):
    ig = mnas_graph()
    x = synth.rand_uniform_int(9, 'mnas_x', (3, 3, 32, 32), 0, 255).astype(np.int32)
    want = oracle.graph_forward(ig, x)
    assert np.unique(want).size > 8
    net = ig.build_net(4)
    plan = net.describe()
    assert 'dwconv5x5s2:' in plan and 'dwconv5x5s1:' in plan and 'dwconv7x7s1:' in plan, plan
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got.reshape(want.shape), want)
    net.check()
