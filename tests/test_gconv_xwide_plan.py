"""Grouped 3x3 convolutions at group widths 72 .. 256 (f8_gconvx.hip) without a GPU: the planning key `gconv_xwide`, what it routes and what keeps its route,
the launch's counts, the forwarding through build_net, the plan and liveness of every case of tests/gconv_xwide_cases.py on the reference."""
import numpy as np
import pytest

import gconv_cases
import gconv_wide_cases as wc
import gconv_xwide_cases as xc
from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

F8_ERR_INVALID, F8_ERR_STATE = -1, -5


def _net(xwide, grouped=1, C=144, cg=72, K=3, stride=1, pad=1, cout=None, dilation=1, hw=12, wide=None):
    net = F8Net().set_option('grouped', grouped)
    for key, v in (('gconv_xwide', xwide), ('gconv_wide', wide)):
        if v is not None:
            net.set_option(key, v)
    t = net.conv(net.input(C, hw, hw, 8), np.ones((cout or C, cg, K, K), np.int32), None, stride=stride, pad=pad, groups=C // cg, weight_fl=4,
                 input_fl=8, input_signed=False, quant_input=False, relu=True, dilation=dilation)
    net.output(t, as_float=False)
    return net.finalize(2)


def test_the_option_is_a_planning_key(monkeypatch):
    assert F8Net().get_option('gconv_xwide') == 0 and F8Net().set_option('gconv_xwide', 1).get_option('gconv_xwide') == 1
    for net, bad, status in ((F8Net(), 2, F8_ERR_INVALID), (F8Net(), -1, F8_ERR_INVALID), (_net(1), 0, F8_ERR_STATE)):      # (refused after finalize)
        with pytest.raises(_lib.F8Error) as e:
            net.set_option('gconv_xwide', bad)
        assert e.value.status == status
    monkeypatch.setenv('F8_GCONV_XWIDE', '1')
    assert F8Net().get_option('gconv_xwide') == 1 and F8Net().get_option('gconv_wide') == 0


@pytest.mark.parametrize('C, cg', xc.SHAPES + ((360, 72), (384, 128)))
def test_the_shape_set_plans_one_launch_and_counts_the_grouped_work(C, cg):
    # 12 x 12 in, by hand (gconvx_tile): / 1 pad 1: 144 outputs in one tile, five groups: <1, 8>; pad 0: 100 outputs, two images a tile up to cg 128 (7 groups),
    # one above (4 groups); / 2: always <2, 4>
    for stride, pad, npg in ((1, 1, 8), (1, 0, 8 if cg <= 128 else 4), (2, 1, 4), (2, 0, 4)):
        net = _net(1, C=C, cg=cg, stride=stride, pad=pad)
        (i, tok, kern), = gconv_cases.g_lines(net)
        assert (tok, kern) == (f'gconvx3x3s{stride}:', f'f8::gconvx3x3_kernel<{stride}, {npg}>'), net.describe()
        P, Cs = (12 + 2 * pad - 3) // stride + 1, (C + 31) // 32 * 32
        assert net.launch_info(i, 2)[1:] == (2 * (12 * 12 * Cs + P * P * Cs * 4) + C * (9 * cg + 4), 2.0 * 9 * cg * C * P * P * 2)    # bytes: input once, int32 out, the groups' weights
        assert net.launch_valu(i, 2) == 0.0                                # no int8 form produced (3 per int8 value: below)
        for xwide in (None, 0):                                            # the key off: the parent's plan
            (_, tok, kern), = gconv_cases.g_lines(_net(xwide, C=C, cg=cg, stride=stride, pad=pad))
            assert tok == f'gconv3x3s{stride}_dense:' and kern.startswith(gconv_cases.DENSE_KERNEL)


@pytest.mark.parametrize('kw, tok', [(dict(C=152, cg=76), 'gconv3x3s1_dense:'), (dict(C=528, cg=264), 'gconv3x3s1_dense:'), (dict(cout=288), 'gconv3x3s1_dense:'),
                                     (dict(K=5, pad=2), 'gconv5x5s1_dense:'), (dict(dilation=2, pad=2), 'gconv3x3s1d2_dense:'),
                                     (dict(grouped=2), 'gconv3x3s1_dense:'), (dict(C=128, cg=64, wide=0), 'gconv3x3s1_dense:'),
                                     (dict(C=128, cg=64, wide=1), 'gconvw3x3s1:'),
                                     (dict(C=240, cg=120, stride=2, hw=32), 'gconv3x3s2_dense:')],      # (two groups / 2 on 16 x 16 outputs, more than one tile: measured slower)
                         ids=lambda v: v if isinstance(v, str) else '_'.join(map(str, v)))
def test_everything_else_keeps_its_route(kw, tok):
    nets = [_net(xwide, **kw) for xwide in (0, 1)]
    assert [[ln[1] for ln in gconv_cases.g_lines(n)] for n in nets] == [[tok], [tok]] and nets[0].describe() == nets[1].describe(), nets[1].describe()


def test_build_net_forwards_the_key():
    """The first stage of a ResNeXt-50 of two groups, 128 wide (group width 128, three blocks), classifier on its 256 channels."""
    spec = topology.resnext(50, 2, 128, num_classes=10)
    spec.blocks, spec.fc_in = spec.blocks[:3], 256
    params = synth.make_params(spec, seed=31)
    nets = [build_net(spec, params, 2, hw=64, options=o) for o in (None, {'gconv_xwide': 1})]
    old, toks = [[n.launch_info(i, 1)[0] for i in range(n.num_launches)] for n in nets]
    new = [t for t in toks if t.startswith('gconvx')]
    assert new == [f'gconvx3x3s1:stage_0_layer_{k}.body.2' for k in range(3)] and [n.get_option('gconv_xwide') for n in nets] == [0, 1]
    assert [t.replace('gconvx3x3', 'gconv3x3').replace(':', '_dense:', 1) if t in new else t for t in toks] == old      # (hence no gconvx token in `old`)


@pytest.mark.parametrize('name', sorted(xc.CASES))
def test_plan_and_liveness_on_the_reference(name):
    """The plan of both legs and the conditions of test_gconv_plan.test_liveness_on_the_reference (values spread, under half of an int8 form at a clamp bound)."""
    case = xc.CASES[name]
    x = gconv_cases.make_input(name, case)
    g, out, ids = wc.plan(name, case, x)
    lines = gconv_cases.g_lines(g.net)
    assert gconv_cases.lines_match(lines, xc.expect(case)), g.net.describe()
    assert g.net.launch_valu(lines[0][0], 1) == 3.0 * len(case['readers'] or []) * np.prod(gconv_cases.out_hw(case)) * ((case['C'] + 31) // 32 * 32)
    assert not case.get('tap') or 'out[i32=1 i8=1' in [ln for ln in g.net.describe().splitlines() if 'gconv' in ln][0], g.net.describe()
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
