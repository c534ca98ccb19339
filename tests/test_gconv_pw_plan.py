"""Grouped 1x1 convs with cin != cout (f8_gconvp.hip) without a GPU: the planning key `gconv_pw`, its routes, counts and forwarding, every case's plan and liveness."""
import numpy as np
import pytest

import gconv_cases
import gconv_pw_cases as pc
import gconv_wide_cases as wc
from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

def _net(pw, grouped=1, cin=96, cout=384, groups=8, K=1, stride=1, pad=0, hw=6):
    net = F8Net().set_option('grouped', grouped)
    if pw is not None:
        net.set_option('gconv_pw', pw)
    t = net.conv(net.input(cin, hw, hw, 8), np.ones((cout, cin // groups, K, K), np.int32), None, stride=stride, pad=pad, groups=groups, weight_fl=4,
                 input_fl=8, input_signed=False, quant_input=False, relu=True)
    net.output(t, as_float=False)
    return net.finalize(2)


def test_the_option_is_a_planning_key(monkeypatch):
    assert F8Net().get_option('gconv_pw') == 0 and [F8Net().set_option('gconv_pw', v).get_option('gconv_pw') for v in (1, 2)] == [1, 2]
    for net, bad, status in ((F8Net(), 3, -1), (F8Net(), -1, -1), (_net(1), 0, -5)):      # F8_ERR_INVALID, F8_ERR_STATE (refused after finalize)
        with pytest.raises(_lib.F8Error) as e:
            net.set_option('gconv_pw', bad)
        assert e.value.status == status
    monkeypatch.setenv('F8_GCONV_PW', '2')
    assert F8Net().get_option('gconv_pw') == 2 and F8Net().get_option('gconv_xwide') == 0


@pytest.mark.parametrize('cin, cout, groups, inst, rule', [(96, 384, 8, (4, 1), False), (384, 192, 8, (16, 2), False), (768, 192, 8, (16, 4), True),
                                                          (240, 480, 3, (16, 4), False), (720, 240, 2, (16, 16), False)])      # rule: gconvp_rule by hand, what gconv_pw = 1 routes
def test_the_set_plans_one_launch_and_counts_the_grouped_work(cin, cout, groups, inst, rule):
    kw = dict(cin=cin, cout=cout, groups=groups)
    net = _net(2, **kw)
    (i, tok, kern), = gconv_cases.g_lines(net)
    assert (tok, kern) == ('gconvp1x1s1:', 'f8::gconvp1x1_kernel<%d, %d>' % inst), net.describe()
    ci, co = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32      # bytes: input once, int32 out, the groups' weights and biases; operations: 2 cgi cout P Q an image
    assert net.launch_info(i, 2)[1:] == (2 * 36 * (ci + co * 4) + cout * (cin // groups + 4), 2.0 * (cin // groups) * cout * 36 * 2)
    assert _net(1, **kw).describe() == _net(2 if rule else 0, **kw).describe()
    for pw in (None, 0):                                            # the key off: the parent's plan
        (_, tok, kern), = gconv_cases.g_lines(_net(pw, **kw))
        assert tok == 'gconv1x1s1_dense:' and kern.startswith(gconv_cases.DENSE_KERNEL)


def test_build_net_forwards_the_key():
    spec = topology.resnext(50, 32, 4, num_classes=10)      # its first block: no grouped 1x1 in it, so the key changes no launch; it arrives on the handle
    spec.blocks, spec.fc_in = spec.blocks[:1], 256
    params = synth.make_params(spec, seed=31)
    nets = [build_net(spec, params, 2, hw=64, options=o) for o in (None, {'gconv_pw': 2})]
    assert [n.get_option('gconv_pw') for n in nets] == [0, 2] and nets[0].describe() == nets[1].describe()


def _live(g, out):
    y = g.v[out][0]      # test_gconv_xwide_plan's conditions: values spread, under half of any int8 form at a clamp bound
    assert np.unique(y).size > 8 and ((y == y.max()) | (y == y.min())).mean() < 0.5
    for label, xq, sgn in g.taps:
        assert np.unique(xq).size >= 16 and ((xq == (-127 if sgn else 0)) | (xq == (127 if sgn else 255))).mean() < 0.5, label


@pytest.mark.parametrize('name', sorted(pc.CASES))
def test_plan_and_liveness_on_the_reference(name):
    case = pc.CASES[name]
    x = gconv_cases.make_input(name, case)
    g, out, ids = wc.plan(name, case, x)
    lines = gconv_cases.g_lines(g.net)
    assert gconv_cases.lines_match(lines, pc.expect(case)), g.net.describe()
    off = wc.plan(name, dict(case, opts={'gconv_pw': 0}), x)[0].net      # the key off: the parent's plan; outside the set the key changes nothing
    assert gconv_cases.lines_match(gconv_cases.g_lines(off), gconv_cases.expect(case, leg=2)) and (case['inst'] is not None or off.describe() == g.net.describe())
    assert not case.get('tap') or 'out[i32=1 i8=1' in [ln for ln in g.net.describe().splitlines() if 'gconv' in ln][0], g.net.describe()
    _live(g, out)
    raw, b = g.raw[ids[0]], gconv_cases.biases(case)
    if case['only_group'] is not None:
        o = pc.outside(case)
        assert (raw[:, o] == b[o][None, :, None, None]).all() and (raw[:, ~o] != b[~o][None, :, None, None]).mean() > 0.9
    if case['bias_big']:
        assert (raw.astype(np.int64) > 2 ** 31 - 2 ** 13).any() and (g.taps[0][1][:, 3] == 0).any()


def test_the_unit_plans_two_launches_and_an_add():
    g, out, _ = pc.unit(1)
    toks = [g.net.launch_info(i, 1)[0].split(':')[0] for i in range(g.net.num_launches)]
    assert gconv_cases.lines_match(gconv_cases.g_lines(g.net), pc.UNIT_EXPECT) and toks.count('add') == 1, g.net.describe()
    assert all(tok == 'gconv1x1s1_dense:' for _, tok, _ in gconv_cases.g_lines(pc.unit(1, {})[0].net))
    _live(g, out)
