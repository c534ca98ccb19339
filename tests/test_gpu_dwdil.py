"""Dilated depthwise 5x5 / 7x7 convs (option dw_dilated) on the device, bit for bit against the zero-stuffed reference (tests/dil_cases.py describes it):
dwconvk_dil_dot4_kernel<K, ROWS> (f8_dwk.hip, dw_dilated = 1: ROWS = 1 by the measured rule, ROWS = 2 under dwdil_rows = 2) and dwconvk_kernel
(dw_dilated = 2), the legs against each other; a MobileNet-V3
LR-ASPP-style tail recorded as an IntGraph.  Graph: input -> the conv (quant_input = False) -> one 32-output 1x1 reader per (fraclen, signed), summed."""
import numpy as np
import pytest
import torch

from dwk_cases import dw_lines, generic
from f8net_amd import synth
from ir_cases import _b, _w
from mul_cases import _cv
from refgraph import RefGraph, graph_forward, record_int_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


# own: dwconvk_dil_dot4_kernel on the dw_dilated = 1 legs (WRITTEN BY HAND from dwk_inst: stride 1, int8 forms only); else dwconvk_kernel there too
def _case(C, H, W, K, d, pad, own=True, **kw):
    return dict(dict(C=C, H=H, W=W, K=K, d=d, pad=pad, own=own, stride=1, N=3, max_batch=None, in_fl=8, in_signed=False, relu=True, readers=[(4, False)],
                     bias_big=False, b_mean=2.0 ** 13, b_sig=2.0 ** 9), **kw)


_SGN = dict(in_fl=7, in_signed=True, relu=False, readers=[(4, True)], b_mean=0.0, b_sig=2.0 ** 11)      # the pad value is a real 0
CASES = {
    'c32_9x3_k5_d2_p4': _case(32, 9, 3, 5, 2, 4),                       # W < DWK_PIX d: residue classes of 2 and 1 pixels
    'c32_9x3_k5_d4_p8': _case(32, 9, 3, 5, 4, 8),                       # W < d: residue 3 is empty; ceil(P / d) = 3: a ROWS = 2 thread without a partner row
    'c40_7x7_k7_d3_p9': _case(40, 7, 7, 7, 3, 9),                       # every window loses taps on both sides; channels padded to 64
    'c96_14x14_k5_d2_p4': _case(96, 14, 14, 5, 2, 4),                   # MobileNet-V3 os16's geometry
    'c96_14x14_k7_d2_p6': _case(96, 14, 14, 7, 2, 6),
    'c32_14x14_k5_d3_p0': _case(32, 14, 14, 5, 3, 0),                   # -> 2 x 2, P < d: no ROWS = 2 thread has a partner row
    'c40_13x15_k7_d2_p1': _case(40, 13, 15, 7, 2, 1),                   # pad < d: -> 3 x 5
    'c32_5x35_k5_d2_p3': _case(32, 5, 35, 5, 2, 3),                     # pad no multiple of d; Q = 33: residues of 17 and 16 pixels, four groups + 1
    'c32_5x11_k7_d9_p27': _case(32, 5, 11, 7, 9, 27),                   # d > H: the extent is 55
    'signed_in_no_relu': _case(40, 9, 11, 5, 2, 4, **_SGN),
    'two_forms': _case(32, 9, 11, 7, 2, 6, readers=[(4, False), (3, True)]),
    'bias_big': _case(32, 9, 11, 5, 3, 6, bias_big=True),               # the int32 wrap in the rounding add
    'stride2': _case(40, 9, 11, 5, 2, 4, False, stride=2),
    'int32_out': _case(32, 9, 11, 7, 2, 6, False, readers=None),
    'max_batch': _case(40, 9, 11, 5, 2, 4, N=8, max_batch=8, **_SGN),   # planned for 8 images; 3, then 8 from one handle
}


def _plan(c, x, dw_dilated, rows):
    g = RefGraph(x, c['in_fl'])
    g.net.set_option('dw_dilated', dw_dilated).set_option('dwdil_rows', rows)
    C, K = c['C'], c['K']
    bd = _b(40, C, c['b_sig'], c['b_mean'])
    if c['bias_big']:
        bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
    t = out = g.conv(next(iter(g.v)), _w(30, (C, 1, K, K), 120.0 / K), bd, stride=c['stride'], pad=c['pad'], groups=C, weight_fl=5, input_fl=c['in_fl'],
                     input_signed=c['in_signed'], relu=c['relu'], quant_input=False, dilation=c['d'])
    for k, (fl, sgn) in enumerate(c['readers'] or []):
        r = g.conv(t, _w(90 + k, (32, C, 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, relu=False)
        out = r if k == 0 else g.add(out, r)
    g.net.output(out, as_float=False)
    g.net.finalize(c['max_batch'] or x.shape[0])
    return g.net, g.v[out][0]


@pytest.mark.parametrize('name', sorted(CASES))
def test_case(name, dev):
    c = CASES[name]
    hi = 127 if c['in_signed'] else 255
    x = synth.rand_uniform_int(5, f'dwdil{name}', (c['N'], c['C'], c['H'], c['W']), -hi if c['in_signed'] else 0, hi).astype(np.int32)
    xt = torch.from_numpy(x).to(dev)
    got = {}
    for leg, (dw_dilated, rows, sym_rows) in enumerate(((1, 0, 1), (1, 2, 2), (2, 0, None))):
        sym = f'f8::dwconvk_dil_dot4_kernel<{c["K"]}, {sym_rows}>' if c['own'] and sym_rows else generic(c['in_signed'])
        net, want = _plan(c, x, dw_dilated, rows)
        assert [ln[1:] for ln in dw_lines(net)] == [(f'dwconv{c["K"]}x{c["K"]}s{c["stride"]}d{c["d"]}:', sym)], net.describe()
        assert np.unique(want).size > 16
        for n in ([3, 8] if c['max_batch'] else [c['N']]):
            got[leg] = net.run(xt[:n]).cpu().numpy().reshape((n,) + want.shape[1:])
            np.testing.assert_array_equal(got[leg], want[:n], err_msg=f'{name} {sym} n={n}')
        net.check()
    np.testing.assert_array_equal(got[0], got[2])
    np.testing.assert_array_equal(got[1], got[2])


def _lraspp_tail(g, x0):
    """mul_cases.mbv3_block with its depthwise 5x5 at dilation 2, pad 4, and a classifier behind it: 1x1 to 24 (the block input) -> 1x1 expand to 72 + hard-swish
    -> the depthwise conv + hard-swish -> SE (pool -> fc to 24 -> fc to 72 -> hard gate -> channel gate) -> 1x1 project to 24 + the block input ->
    average pool -> linear to 10 classes."""
    t = _cv(g, x0, 0, 24, 9, relu=False, in_fl=8, in_signed=False, quant_input=False, label='stem')                    # fraclen 13
    e = _cv(g, t, 1, 72, 8, relu=False, in_fl=4, in_signed=True, label='expand')                                       # 9
    h1 = g.hard_swish(e, x_fl=3, x_signed=True, g_fl=5, label='hs1')                                                  # 8
    d = g.conv(h1, _w(714, (72, 1, 5, 5), 40.0), _b(814, 72, 2.0 ** 8 * 20), pad=4, groups=72, weight_fl=7, input_fl=2, input_signed=True, relu=False,
               dilation=2, label='dw')                                                                                 # 9
    h2 = g.hard_swish(d, x_fl=3, x_signed=True, g_fl=5, label='hs2')                                                  # 8
    f1 = g.linear(g.avgpool_sum(h2), _w(901, (24, 72), 6.0), _b(902, 24, 2.0 ** 8), weight_fl=5, input_fl=2, input_signed=True, label='se.fc1')
    f2 = g.linear(f1, _w(903, (72, 24), 10.0), _b(904, 72, 2.0 ** 9), weight_fl=6, input_fl=3, input_signed=True, label='se.fc2')
    s = g.mul(h2, g.hard_gate(f2, label='se.gate'), a_fl=2, a_signed=True, b_fl=5, b_signed=False, label='se.scale')   # 7
    j = g.add(_cv(g, s, 3, 24, 6, relu=False, in_fl=1, in_signed=True, w_fl=6, label='project'), t)                    # 13
    return g.linear(g.avgpool_sum(j), _w(98, (10, 24), 30.0), _b(99, 10, 2.0 ** 10), weight_fl=5, input_fl=4, input_signed=True, label='classifier')


def test_mobilenet_v3_tail_through_build_net(dev):
    x = synth.rand_uniform_int(9, 'dwdil_net', (3, 8, 14, 14), 0, 255).astype(np.int32)
    ig, _, _ = record_int_graph(x, 8, _lraspp_tail)
    want = graph_forward(ig, x, 8)
    assert np.unique(want).size > 8
    net = ig.build_net(4, input_fraclen=8, options=None)
    assert net.get_option('dw_dilated') == 1 and 'dwconv5x5s1d2:' in net.describe(), net.describe()
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got.reshape(want.shape), want)
    net.check()
