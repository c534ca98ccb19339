"""Grouped 3x3 convolutions at group widths 72 .. 256 on the device, bit for bit against the reference of tests/gconv_cases.py (the CPU oracle per group):
every case of tests/gconv_xwide_cases.py with `grouped = 1, gconv_xwide = 1` (f8::gconvx3x3_kernel<S, NPG>, f8_gconvx.hip) and, on the same graph and
input, with `grouped = 2` (the dense expansion); the two legs against each other; case `batches`: one handle at 1, 2 and 3 images."""
import numpy as np
import pytest
import torch

import gconv_cases
import gconv_wide_cases as wc
import gconv_xwide_cases as xc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(xc.CASES))
def test_case(name):
    case = xc.CASES[name]
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    x = gconv_cases.make_input(name, case)
    xt = torch.from_numpy(x).to('cuda:0')
    outs = {}
    for leg in gconv_cases.LEGS:
        g, out, ids = wc.plan(name, case, x, leg)
        lines = gconv_cases.g_lines(g.net)
        assert gconv_cases.lines_match(lines, xc.expect(case)) if leg == 1 else all(tok.endswith('_dense:') for _, tok, _ in lines), g.net.describe()
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
        outside = np.arange(case['C']) // case['cg'] != case['only_group']
        for leg in gconv_cases.LEGS:
            assert (outs[leg].reshape(case['N'], case['C'], -1)[:, outside] == gconv_cases.biases(case)[outside][None, :, None]).all(), leg
