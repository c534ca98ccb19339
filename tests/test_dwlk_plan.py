"""Large depthwise convs (kernel 8 .. 31, option dw_large; dwlk_kernel of f8_dwlk.hip and dwconvk_kernel of f8_dwk.hip) without a GPU: what the builder
accepts and refuses, the plan of every case of tests/dwlk_cases.py against its hand-written table on both legs, the kernels 3 / 5 / 7 left as they were,
an ONNX round trip, and the liveness of every case on the oracle's values."""
import functools

import numpy as np
import pytest

import dwk_cases
import dwlk_cases as lc
from f8net_amd import _lib, onnx_export, onnx_import
from f8net_amd.net import F8Net
from refgraph import record_int_graph

F8_ERR_UNSUPPORTED = -2


@functools.lru_cache(maxsize=None)
def _planned(name):
    return lc.plan(lc.ALL[name], lc.make_input(name, lc.ALL[name]))


def _dw_net(K, stride, pad, dw_large, dilation=1, hw=40):
    net = F8Net().set_option('dw_large', dw_large)
    t = net.input(16, hw, hw, 8)
    t = net.conv(t, np.ones((16, 1, K, K), np.int32), None, stride=stride, pad=pad, groups=16, weight_fl=4, input_fl=8, input_signed=False,
                 quant_input=False, relu=True, dilation=dilation)
    net.output(t, as_float=False)
    return net


@pytest.mark.parametrize('K', [8, 9, 13, 16, 31])
def test_acceptance_follows_the_option(K):
    assert F8Net().get_option('dw_large') == 0
    with pytest.raises(_lib.F8Error) as e:
        _dw_net(K, 1, K // 2, 0)
    assert e.value.status == F8_ERR_UNSUPPORTED and 'kernel 3, 5 or 7, stride 1 or 2' in str(e.value)
    for dw_large in (1, 2):
        for stride, pad in ((1, K // 2), (2, 0), (1, 1)):
            net = _dw_net(K, stride, pad, dw_large).finalize(2)
            assert f'dwconv{K}x{K}s{stride}:' in net.describe(), net.describe()


@pytest.mark.parametrize('K, stride, pad, dilation', [(4, 1, 1, 1), (6, 1, 3, 1), (9, 3, 4, 1), (9, 1, 5, 1), (32, 1, 16, 1), (9, 1, 4, 2)])
def test_what_stays_refused_with_the_option_on(K, stride, pad, dilation):
    with pytest.raises(_lib.F8Error) as e:
        _dw_net(K, stride, pad, 1, dilation, hw=64)
    assert e.value.status == F8_ERR_UNSUPPORTED
    assert dilation > 1 or '8 .. 31' in str(e.value)


@pytest.mark.parametrize('name', sorted(lc.ALL))
def test_plan(name):
    case = lc.ALL[name]
    for leg in lc.LEGS:
        g, _, ids = _planned(name) if leg == 'own' else lc.plan(case, lc.make_input(name, case), leg)
        lines = lc.dw_lines(g.net)
        assert [ln[1:] for ln in lines] == lc.expect(case, leg), (leg, g.net.describe())
        assert len(lines) == len(ids)
        P, Q = lc.out_hw(case)
        assert g.net.launch_info(lines[0][0], case['N'])[2] == 2.0 * case['K'] ** 2 * case['C'] * P * Q * case['N']


@pytest.mark.parametrize('name', ['k5s1_9x11', 'k7s2_8x10', 'p_k3s1_pad0', 'f_two_unsigned_k5s1', 'f_i32_k7s2'])
def test_kernels_3_5_7_plan_as_before(name):
    case = dwk_cases.CASES[name]
    x = dwk_cases.make_input(name, case)
    texts = []
    for dw_large in (0, 1, 2):
        g, _, _ = dwk_cases.build_graph(case, x)
        texts.append(g.net.set_option('dw_large', dw_large).finalize(3).describe())
        assert [ln[1:] for ln in dwk_cases.dw_lines(g.net)] == dwk_cases.expect(case)
    assert texts[0] == texts[1] == texts[2]


def test_onnx_round_trip_opts_in_by_itself():
    case = lc.CASES['k13_7x7_p6_c40']
    x = lc.make_input('rt', case)
    w, b = lc._dw_weight(30, case['C'], 13, case['w_sig']), lc._b(40, case['C'], case['b_sig'], case['b_mean'])
    ig, g, out = record_int_graph(x, 8, lambda g, t: g.conv(t, w, b, pad=6, groups=case['C'], weight_fl=5, input_fl=8, input_signed=False, relu=True,
                                                           quant_input=False))
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    net = back.build_net(3, input_fraclen=8)
    assert net.get_option('dw_large') == 1 and [ln[1:] for ln in lc.dw_lines(net)] == [('dwconv13x13s1:', lc.generic(False))], net.describe()     # (its result is the int32 output)
    assert 'dwconv13x13s1:' in back.build_net(3, input_fraclen=8, options={'dw_large': 2}).describe()
    with pytest.raises(_lib.F8Error):
        back.build_net(3, input_fraclen=8, options={'dw_large': 0})


@pytest.mark.parametrize('name', sorted(lc.ALL))
def test_liveness_on_the_oracle(name):
    """Conditions on the case table, not measurements: the depthwise result's first int8 form has more than 16 distinct values and fewer than a quarter
    of its values at a clamp bound; the final value is not constant; the wrap case wraps."""
    case = lc.ALL[name]
    g, out, ids = _planned(name)
    assert np.unique(g.v[out][0]).size > 16
    if g.taps:
        _, xq, sgn = g.taps[0]
        lo, hi = (-127, 127) if sgn else (0, 255)
        assert np.unique(xq).size > 16 and ((xq == lo) | (xq == hi)).mean() < 0.25, name
    else:
        assert case['readers'] is None
    if case['bias_big']:
        assert (g.raw[ids[0]].astype(np.int64) > 2 ** 31 - 2 ** 13).any()
