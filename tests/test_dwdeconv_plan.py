"""Depthwise transposed convs (option dw_deconv, f8_dwdeconv.hip) without a GPU: the option, what every case of tests/dwdeconv_cases.py plans, the stride-1
route, the accepted range and what stays refused, an ONNX round trip, and the reference pinned to torch in float64.  tests/test_gpu_dwdeconv.py runs the
cases on the device."""
import os
import subprocess

import numpy as np
import pytest
import torch

import dwdeconv_cases as dd
from f8net_amd import _lib, onnx_export, onnx_import, onnx_io, synth
from f8net_amd.net import F8Net
from f8net_amd.onnx_import import IntGraph, IntOp
from ref_ops import deconv_ref

UNSUPPORTED = -2


def _net(k, s, pad, op=0, C=8, cout=None, groups=None, hw=(3, 5), **opts):
    net = F8Net()
    for key, v in opts.items():
        net.set_option(key, v)
    groups = C if groups is None else groups
    cout = C if cout is None else cout
    t = net.conv_transpose(net.input(C, hw[0], hw[1], 4), np.ones((C, cout // groups, k, k), np.int32), None, stride=s, pad=pad, output_padding=op, weight_fl=6,
                           input_fl=4, input_signed=False, quant_input=False, groups=groups, label='up')
    net.output(t, as_float=False)
    return net.finalize(2)


def test_the_option_is_a_planning_key(monkeypatch):
    assert F8Net().get_option('dw_deconv') == 0 and [F8Net().set_option('dw_deconv', v).get_option('dw_deconv') for v in (1, 2)] == [1, 2]
    with pytest.raises(_lib.F8Error):
        F8Net().set_option('dw_deconv', 3)
    monkeypatch.setenv('F8_DW_DECONV', '2')
    assert F8Net().get_option('dw_deconv') == 2


@pytest.mark.parametrize('name', sorted(dd.CASES))
def test_token_and_symbol_of_every_case(name):
    c = dd.CASES[name]
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    for mode in (1, 2):
        g, _, outs = dd.plan(name, mode)
        (i, tok, sym), = dd.deconv_lines(g.net)
        assert (tok, sym) == (dd.token(c), dd.symbol(c, mode)), g.net.describe()
        assert f'void {sym}(f8::DwDeconvArgs)' in syms
        assert f'out[i32={int(c["out"])} i8={len(c["fmts"] or ())} ' in g.net.describe().splitlines()[i], g.net.describe()
        assert all(np.unique(g.v[o][0]).size > 16 for o in outs)


def test_stride_1_is_recorded_as_the_flipped_depthwise_conv():
    net = _net(3, 1, 1, dw_deconv=1)
    (_, tok, sym), = dd.deconv_lines(net)
    assert tok.startswith('dwconv3x3s1') and 'deconv' not in net.describe(), net.describe()
    with pytest.raises(_lib.F8Error):                               # the depthwise conv's own rule: kernel 4 is not built
        _net(4, 1, 1, dw_deconv=1)


@pytest.mark.parametrize('k, s, pad, op', [(1, 2, 0, 1), (16, 8, 15, 7), (16, 2, 0, 0), (9, 5, 3, 4), (2, 8, 1, 0)])
def test_accepted_range(k, s, pad, op):
    for mode in (1, 2):
        net = _net(k, s, pad, op, dw_deconv=mode)
        assert net.output_info(0)[:3] == (8, dd.out_size(3, k, s, pad, op), dd.out_size(5, k, s, pad, op)) and f'dwdeconv{k}x{k}s{s}:up' in net.describe()


@pytest.mark.parametrize('kw, words', [
    (dict(k=17, s=2, pad=1), 'kernel 17 > 16'), (dict(k=4, s=9, pad=1), 'stride 9 > 8'), (dict(k=4, s=2, pad=4), 'pad 4 > kernel - 1'),
    (dict(k=4, s=2, pad=1, op=2), 'output_padding 2'), (dict(k=4, s=2, pad=1, groups=2), 'groups 2: only groups == 1 is built'),
    (dict(k=4, s=2, pad=1, groups=8, cout=16), 'groups 8: only groups == 1 is built')])
def test_what_stays_refused_with_the_option_on(kw, words):
    with pytest.raises(_lib.F8Error) as e:
        _net(dw_deconv=1, **kw)
    assert words in str(e.value)


def test_a_default_handle_refuses_the_depthwise_form_in_the_parents_words():
    with pytest.raises(_lib.F8Error) as e:
        _net(4, 2, 1)
    assert e.value.status == UNSUPPORTED and 'f8_net_conv_transpose: groups 8: only groups == 1 is built (' in str(e.value)


def test_onnx_round_trip_opts_in_by_itself():
    c = dd.CASES['g_4210']
    w, b = dd.weights(c)
    ig = IntGraph(ops=[IntOp('input', shape=(40, 3, 5)), IntOp('deconv', src=0, weight=w, bias=b, stride=2, pad=1, groups=40, kernel=4, shift=None, key='up')],
                  output=1, output_float=False)
    data = onnx_export.export_graph(ig)
    (ct,) = [n for n in onnx_io.load_graph(data).nodes if n.op == 'ConvTranspose']
    assert ct.attrs['group'] == 40
    back = onnx_import.import_graph(data)
    assert back.ops[1].groups == 40 and back.ops[1].weight.shape == (40, 1, 4, 4)
    net = back.build_net(2, input_fraclen=4)
    assert net.get_option('dw_deconv') == 1 and net.output_info(0)[:3] == (40, 6, 10) and 'dwdeconv4x4s2:' in net.describe()
    assert 'f8::dwdeconv_kernel' in back.build_net(2, input_fraclen=4, options={'dw_deconv': 2}).launch_kernel(1)
    with pytest.raises(_lib.F8Error):
        back.build_net(2, input_fraclen=4, options={'dw_deconv': 0})


@pytest.mark.parametrize('k, s, pad, op', [(4, 2, 1, 0), (3, 2, 1, 1), (2, 3, 0, 1), (16, 8, 4, 0)])
def test_reference_on_expanded_weights_is_torchs_grouped_deconv(k, s, pad, op):
    """float64 is exact here: |acc| < 256 * 255 * 127 + 2^20 << 2^53."""
    x = synth.rand_uniform_int(9, f'dwdpin{k}{s}', (2, 4, 3, 5), -127, 255)
    w = synth.rand_uniform_int(10, f'dwdpin{k}{s}', (4, 1, k, k), -127, 127)
    b = synth.rand_uniform_int(11, 'dwdpin', (4,), -2 ** 20, 2 ** 20)
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=s, padding=pad,
                                                output_padding=op, groups=4).numpy()
    np.testing.assert_array_equal(deconv_ref(x, dd.dense(w), b, s, pad, op).astype(np.float64), want)
