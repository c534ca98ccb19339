"""Grouped 3x3 convolutions at group widths 24 .. 64 (f8_gconvw.hip) without a GPU: the planning key `gconv_wide`, what it routes and what keeps its route, the
launch's counts, the forwarding through build_net on ResNeXt-101 32x8d, the plan and liveness of every case of tests/gconv_wide_cases.py on the reference."""
import numpy as np
import pytest

import gconv_cases
import gconv_wide_cases as wc
from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

F8_ERR_INVALID, F8_ERR_STATE = -1, -5


def _net(wide, grouped=1, C=48, cg=24, K=3, stride=1, pad=1, cout=None, dilation=1, hw=12):
    net = F8Net().set_option('grouped', grouped)
    if wide is not None:
        net.set_option('gconv_wide', wide)
    t = net.conv(net.input(C, hw, hw, 8), np.ones((cout or C, cg, K, K), np.int32), None, stride=stride, pad=pad, groups=C // cg, weight_fl=4,
                 input_fl=8, input_signed=False, quant_input=False, relu=True, dilation=dilation)
    net.output(t, as_float=False)
    return net.finalize(2)


def test_the_option_is_a_planning_key(monkeypatch):
    assert F8Net().get_option('gconv_wide') == 0 and F8Net().set_option('gconv_wide', 1).get_option('gconv_wide') == 1
    for net, bad, status in ((F8Net(), 2, F8_ERR_INVALID), (F8Net(), -1, F8_ERR_INVALID), (_net(1), 0, F8_ERR_STATE)):      # (refused after finalize)
        with pytest.raises(_lib.F8Error) as e:
            net.set_option('gconv_wide', bad)
        assert e.value.status == status
    monkeypatch.setenv('F8_GCONV_WIDE', '1')
    assert F8Net().get_option('gconv_wide') == 1


@pytest.mark.parametrize('C, cg', wc.SHAPES + ((120, 24), (192, 64)))
def test_the_shape_set_plans_one_launch_and_counts_the_grouped_work(C, cg):
    for stride, pad in ((1, 1), (1, 0), (2, 1), (2, 0)):
        net = _net(1, C=C, cg=cg, stride=stride, pad=pad)
        (i, tok, kern), = gconv_cases.g_lines(net)
        assert (tok, kern) == (f'gconvw3x3s{stride}:', f'f8::gconvw3x3_kernel<{stride}, {(cg + 31) // 32}>'), net.describe()
        P, Cs = (12 + 2 * pad - 3) // stride + 1, (C + 31) // 32 * 32
        assert net.launch_info(i, 2)[1:] == (2 * (12 * 12 * Cs + P * P * Cs * 4) + C * (9 * cg + 4), 2.0 * 9 * cg * C * P * P * 2)    # bytes: input once, int32 out, the groups' weights
        assert net.launch_valu(i, 2) == 0.0                                # no int8 form produced (3 per int8 value: below)
        for wide in (None, 0):                                             # the key off: the parent's plan
            (_, tok, kern), = gconv_cases.g_lines(_net(wide, C=C, cg=cg, stride=stride, pad=pad))
            assert tok == f'gconv3x3s{stride}_dense:' and kern.startswith(gconv_cases.DENSE_KERNEL)


@pytest.mark.parametrize('kw, tok', [(dict(C=64, cg=32), 'gconv3x3s1:'), (dict(C=144, cg=72), 'gconv3x3s1_dense:'), (dict(cout=96), 'gconv3x3s1_dense:'),
                                     (dict(K=5, pad=2), 'gconv5x5s1_dense:'), (dict(grouped=2), 'gconv3x3s1_dense:'),
                                     (dict(dilation=2, pad=2), 'gconv3x3s1d2_dense:')], ids=lambda v: v if isinstance(v, str) else '_'.join(map(str, v)))
def test_everything_else_keeps_its_route(kw, tok):
    nets = [_net(wide, **kw) for wide in (0, 1)]
    assert [[ln[1] for ln in gconv_cases.g_lines(n)] for n in nets] == [[tok], [tok]] and nets[0].describe() == nets[1].describe(), nets[1].describe()


def test_build_net_forwards_the_key_on_resnext101_32x8d():
    spec = topology.get('resnext101_32x8d')
    params = synth.make_params(spec, seed=31)
    nets = [build_net(spec, params, 2, hw=64, options=o) for o in (None, {'gconv_wide': 1})]
    old, toks = [[n.launch_info(i, 1)[0] for i in range(n.num_launches)] for n in nets]
    new = [t for t in toks if t.startswith('gconvw')]
    assert new == ['gconvw3x3s2:stage_3_layer_0.body.2', 'gconvw3x3s1:stage_3_layer_1.body.2', 'gconvw3x3s1:stage_3_layer_2.body.2']
    assert [t.replace('gconvw3x3', 'gconv3x3').replace(':', '_dense:', 1) if t in new else t for t in toks] == old      # (hence no gconvw token in `old`)


@pytest.mark.parametrize('name', sorted(wc.CASES))
def test_plan_and_liveness_on_the_reference(name):
    """The plan of both legs and the conditions of test_gconv_plan.test_liveness_on_the_reference (values spread, under half of an int8 form at a clamp bound)."""
    case = wc.CASES[name]
    x = gconv_cases.make_input(name, case)
    g, out, ids = wc.plan(name, case, x)
    lines = gconv_cases.g_lines(g.net)
    assert [ln[1:] for ln in lines] == wc.expect(case), g.net.describe()
    assert g.net.launch_valu(lines[0][0], 1) == 3.0 * len(case['readers'] or []) * np.prod(gconv_cases.out_hw(case)) * ((case['C'] + 31) // 32 * 32)
    assert not case.get('tap') or 'out[i32=1 i8=1' in [ln for ln in g.net.describe().splitlines() if 'gconvw' in ln][0], g.net.describe()
    y = g.v[out][0]
    assert np.unique(y).size > 8 and ((y == y.max()) | (y == y.min())).mean() < 0.5 and len(g.taps) == len(case['readers'] or []) + (2 if case.get('second') else 0)
    for label, xq, sgn in g.taps:
        assert np.unique(xq).size >= 16 and ((xq == (-127 if sgn else 0)) | (xq == (127 if sgn else 255))).mean() < 0.5, label
    raw, b = g.raw[ids[0]], gconv_cases.biases(case)
    if case['only_group'] is not None:
        inside = np.arange(case['C']) // case['cg'] == case['only_group']
        assert (raw[:, ~inside] == b[~inside][None, :, None, None]).all() and (raw[:, inside] != b[inside][None, :, None, None]).mean() > 0.9
    if case['bias_big']:
        assert (raw.astype(np.int64) > 2 ** 31 - 2 ** 13).any() and (g.taps[0][1][:, 3] == 0).any()
