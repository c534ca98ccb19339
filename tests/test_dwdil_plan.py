"""Dilated depthwise 5x5 / 7x7 convs (option dw_dilated) without a GPU: what the builder accepts and refuses, an ONNX round trip, and the zero-stuffed
reference of tests/test_gpu_dwdil.py pinned to torch's dilated conv."""
import numpy as np
import pytest
import torch

from dwk_cases import dw_lines
from f8net_amd import _lib, onnx_export, onnx_import, synth
from f8net_amd.net import F8Net
from ir_cases import _b, _w
from oracle import oracle
from ref_ops import stuffed
from refgraph import record_int_graph

F8_ERR_UNSUPPORTED = -2


def _dw_net(K, stride, pad, d, hw=64, **opts):
    net = F8Net()
    for k, v in opts.items():
        net.set_option(k, v)
    t = net.input(16, hw, hw, 8)
    t = net.conv(t, np.ones((16, 1, K, K), np.int32), None, stride=stride, pad=pad, groups=16, weight_fl=4, input_fl=8, input_signed=False,
                 quant_input=False, relu=True, dilation=d)
    net.output(t, as_float=False)
    return net


@pytest.mark.parametrize('K', [5, 7])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('d', [2, 4])
def test_acceptance_follows_the_option(K, stride, d):
    assert F8Net().get_option('dw_dilated') == 0
    for pad in (0, d, d * (K // 2)):
        with pytest.raises(_lib.F8Error) as e:
            _dw_net(K, stride, pad, d)
        assert e.value.status == F8_ERR_UNSUPPORTED and 'dilated depthwise is built for kernel 3, stride 1 or 2' in str(e.value)
        for dw_dilated in (1, 2):
            net = _dw_net(K, stride, pad, d, dw_dilated=dw_dilated).finalize(2)
            assert f'dwconv{K}x{K}s{stride}d{d}:' in net.describe(), net.describe()


@pytest.mark.parametrize('K, stride, pad, d, opts', [(9, 1, 8, 2, dict(dw_large=1)), (5, 1, 5, 2, {}), (7, 1, 10, 3, {}), (5, 3, 4, 2, {})])
def test_what_stays_refused_with_the_option_on(K, stride, pad, d, opts):
    with pytest.raises(_lib.F8Error) as e:
        _dw_net(K, stride, pad, d, dw_dilated=1, **opts)
    assert e.value.status == F8_ERR_UNSUPPORTED
    assert f'kernel {K}, stride {stride}, pad {pad}, dilation {d}' in str(e.value) and 'pad 0 .. dilation * (kernel / 2)' in str(e.value)


def test_onnx_round_trip_opts_in_by_itself():
    """96 x 14 x 14, 5x5 at dilation 2, pad 4 (MobileNet-V3 at output stride 16)."""
    x = synth.rand_uniform_int(5, 'dwdil_rt', (2, 96, 14, 14), 0, 255).astype(np.int32)
    ig, g, out = record_int_graph(x, 8, lambda g, t: g.conv(t, _w(30, (96, 1, 5, 5), 24.0), _b(40, 96, 2.0 ** 9, 2.0 ** 13), pad=4, groups=96, weight_fl=5,
                                                           input_fl=8, input_signed=False, relu=True, quant_input=False, dilation=2))
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    net = back.build_net(2, input_fraclen=8)
    assert net.get_option('dw_dilated') == 1 and [ln[1] for ln in dw_lines(net)] == ['dwconv5x5s1d2:'], net.describe()
    assert 'dwconv5x5s1d2:' in back.build_net(2, input_fraclen=8, options={'dw_dilated': 2}).describe()
    with pytest.raises(_lib.F8Error):
        back.build_net(2, input_fraclen=8, options={'dw_dilated': 0})


@pytest.mark.parametrize('K, d, stride, pad', [(5, 2, 1, 4), (5, 4, 2, 3), (7, 3, 1, 9), (7, 2, 2, 1)])
def test_stuffed_reference_is_torchs_dilated_conv(K, d, stride, pad):
    """float64 is exact here: |acc| < 49 * 255 * 127 + 2^14 << 2^53."""
    C = 8
    x = synth.rand_uniform_int(5, f'dwdil_pin{K}{d}', (2, C, 15, 17), 0, 255).astype(np.int32)
    w, b = _w(30, (C, 1, K, K), 40.0), _b(40, C, 2.0 ** 9, 2.0 ** 13)
    want = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=stride, padding=pad,
                                      dilation=d, groups=C).numpy()
    np.testing.assert_array_equal(oracle.conv2d(x, stuffed(w, d), b, stride, pad, C), want)
