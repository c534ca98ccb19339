"""Depthwise transposed convs (option dw_deconv) on the device, bit for bit against ref_ops.deconv_ref on the diagonal-expanded dense weights: every case
of tests/dwdeconv_cases.py on dwdeconv_dot4_kernel<T> where dw_deconv = 1 plans it and on dwdeconv_kernel (dw_deconv = 2), the op-level drop-in, and one DLA
IDAUp step imported from ONNX."""
import numpy as np
import pytest
import torch

import dwdeconv_cases as dd
from concat_cases import producer
from f8net_amd import onnx_export, onnx_import, ops, synth
from ir_cases import _b, _w
from oracle import oracle
from ref_ops import deconv_ref
from refgraph import record_int_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', sorted(dd.CASES))
def test_case(name, dev):
    c = dd.CASES[name]
    for mode in (1, 2):
        g, x, outs = dd.plan(name, mode)
        assert [ln[1:] for ln in dd.deconv_lines(g.net)] == [(dd.token(c), dd.symbol(c, mode))], g.net.describe()
        got = g.net.run(torch.from_numpy(x).to(dev))
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == len(outs)
        for y, o in zip(got, outs):
            want = g.v[o][0]
            np.testing.assert_array_equal(y.cpu().numpy().reshape(want.shape), want, err_msg=f'{name} dw_deconv={mode}')
        g.net.check()


@pytest.mark.parametrize('C, k, s, pad, op, signed', [(40, 4, 2, 1, 0, False), (8, 3, 2, 1, 1, True)])
def test_op_level_drop_in(C, k, s, pad, op, signed, dev):
    m = ops.F8ConvTranspose2d(C, C, k, stride=s, padding=pad, output_padding=op, input_symmetric=signed, groups=C)
    assert tuple(m.weight.shape) == (C, 1, k, k)
    w = synth.rand_uniform_int(3, f'dwdw{k}{s}', (C, 1, k, k), -127, 127).astype(np.int32)
    b = synth.rand_uniform_int(4, f'dwdb{k}{s}', (C,), -2 ** 20, 2 ** 20).astype(np.int32)
    x = synth.rand_uniform_int(5, f'dwdx{k}{s}', (2, C, 3, 5), -127 if signed else 0, 127 if signed else 255).astype(np.int32)
    m.weight.data, m.bias.data = torch.from_numpy(w), torch.from_numpy(b)
    m.weight_fraclen.fill_(6)
    m.input_fraclen.fill_(4)
    got = m.to(dev)(torch.from_numpy(x).to(dev))
    want = deconv_ref(x, dd.dense(w), b, s, pad, op)
    assert tuple(got.shape) == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def _ida_up(g, x0):
    """One IDAUp step of DLA: the coarse level (the input max-pooled by 2) projected to 40 channels, upsampled by a depthwise 4x4 / 2 transposed conv
    (fraclen 10), added to a lateral 1x1 conv of the fine level (fraclen 9), a 3x3 node conv behind the sum.  The transposed conv's IntOp is appended by
    hand: RefGraph.conv_transpose knows no groups."""
    c = dd.CASES['g_4210']
    lateral = producer(g, x0, 1, 40, 5, w_fl=1, relu=False)
    top = producer(g, g.maxpool(x0, 2, 2, 0), 0, 40, 9, w_fl=5, relu=True)
    w, b = dd.weights(c)
    x, fl = g.v[top]
    y = deconv_ref(oracle.requant(x, 4, fl, False), dd.dense(w), b, 2, 1, 0)
    up = g._put(g._id(None), (oracle.relu(y), 10), 'deconv', src=g._src(top), weight=w, bias=b, stride=2, pad=1, groups=40, kernel=4, shift=fl - 4, signed=False,
                relu=True, key='up', output_padding=0)
    return g.conv(g.add(up, lateral), _w(70, (32, 40, 3, 3), 3.0), _b(71, 32, 2.0 ** 11), pad=1, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=True)


def test_dla_ida_up_step_from_onnx(dev):
    x = synth.rand_uniform_int(9, 'dwd_ida', (2, 8, 6, 10), 0, 255).astype(np.int32)
    ig, g, out = record_int_graph(x, 8, _ida_up)
    want = g.v[out][0]
    assert np.unique(want).size > 100
    net = onnx_import.import_graph(onnx_export.export_graph(ig)).build_net(2, input_fraclen=8)
    names = [net.launch_info(i, 1)[0].split(':')[0] for i in range(net.num_launches)]
    # (the join reads the int32 form, so the launch is the anchor kernel's: a join in the transposed conv's epilogue is not built)
    assert net.get_option('dw_deconv') == 1 and 'dwdeconv4x4s2' in names and net.launch_kernel(names.index('dwdeconv4x4s2')) == 'f8::dwdeconv_kernel<false>', net.describe()
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got.reshape(want.shape), want)
    net.check()
