"""Grouped 1x1 convs with cin != cout on the device, bit for bit against the CPU oracle per group: every case of tests/gconv_pw_cases.py and one ShuffleNet-V1
unit with `grouped = 1, gconv_pw = 2` (f8::gconvp1x1_kernel<SB, KSM>, f8_gconvp.hip) and with `grouped = 2` (the dense expansion), and the legs against each other."""
import numpy as np
import pytest
import torch

import gconv_cases
import gconv_pw_cases as pc
import gconv_wide_cases as wc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(pc.CASES))
def test_case(name):
    case = pc.CASES[name]
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    x = gconv_cases.make_input(name, case)
    xt = torch.from_numpy(x).to('cuda:0')
    outs = {}
    for leg in gconv_cases.LEGS:
        g, out, ids = wc.plan(name, case, x, leg)
        lines = gconv_cases.g_lines(g.net)
        assert gconv_cases.lines_match(lines, pc.expect(case)) if leg == 1 else all(tok.endswith('_dense:') for _, tok, _ in lines), g.net.describe()
        wants = [g.v[out][0]] + ([g.v[ids[0]][0]] if case.get('tap') else [])          # (a `tap` case: the grouped conv's own int32 result is output 1)
        for n in case.get('batches') or [x.shape[0]]:
            got = g.net.run(xt[:n])
            got = [o.cpu().numpy() for o in (got if case.get('tap') else [got])]
            for o, want in zip(got, wants):
                np.testing.assert_array_equal(o.reshape((n,) + want.shape[1:]), want[:n], err_msg=f'{name} grouped={leg} n={n}')
        outs[leg] = got[0]
        g.net.check()
    np.testing.assert_array_equal(outs[1], outs[2], err_msg=name)
    if case['only_group'] is not None:                  # no cross-talk: every output channel outside the live group is its bias, exactly
        for leg in gconv_cases.LEGS:
            assert (outs[leg].reshape(case['N'], case['cout'], -1)[:, pc.outside(case)] == gconv_cases.biases(case)[pc.outside(case)][None, :, None]).all(), leg


def test_shufflenet_v1_unit():
    outs = {}
    for leg in gconv_cases.LEGS:
        g, out, x = pc.unit(leg)
        lines = gconv_cases.g_lines(g.net)
        assert gconv_cases.lines_match(lines, pc.UNIT_EXPECT) if leg == 1 else all(tok.endswith('_dense:') for _, tok, _ in lines), g.net.describe()
        outs[leg] = g.net.run(torch.from_numpy(x).to('cuda:0')).cpu().numpy()
        np.testing.assert_array_equal(outs[leg].reshape(g.v[out][0].shape), g.v[out][0], err_msg=f'grouped={leg}')
        g.net.check()
    np.testing.assert_array_equal(outs[1], outs[2])
