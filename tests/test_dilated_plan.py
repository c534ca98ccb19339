"""Dilated convolutions (f8_net_conv_dilated) without a GPU: the stuffed reference of tests/dil_cases.py pinned to torch's float64 dilated conv; what
the builder accepts and refuses, each with its status; dilation 1 through the new entry point = f8_net_conv; the plan token and kernel symbol of every
case against the hand-written table; the bias classes of the largest case; liveness of every case on the reference; `topology.dilate` against strides /
dilations / pads listed by hand; no fused or chain launch takes a dilated conv in; the ONNX round trip."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import dil_cases
from f8net_amd import _lib, onnx_export, onnx_import, onnx_io, synth, topology
from f8net_amd.net import F8Net, build_net, record_net
from oracle import oracle
from ref_ops import stuffed
from refgraph import graph_forward

F8_ERR_INVALID, F8_ERR_UNSUPPORTED = -1, -2
ALL = dil_cases.ALL
FUSE_ALL = dil_cases.FUSE_ALL


# ---- the reference
@pytest.mark.parametrize('d, stride, pad, groups', [(2, 1, 2, 1), (4, 1, 4, 1), (2, 2, 2, 1), (3, 1, 0, 1), (2, 1, 1, 1), (4, 1, 2, 1), (2, 1, 2, 8), (3, 2, 1, 8)])
def test_the_stuffed_integer_conv_is_torchs_float64_dilated_conv(d, stride, pad, groups):
    """float64 is exact here: |acc| <= 9 * 8 * 255 * 127 + 2^20 << 2^53."""
    C = 8
    x = synth.rand_uniform_int(1, f'pin_x{d}{stride}{pad}', (2, C, 11, 13), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(2, f'pin_w{d}{groups}', (C, C // groups, 3, 3), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(3, 'pin_b', (C,), 3e5).astype(np.int32)
    got = oracle.conv2d(x, stuffed(w, d), b, stride, pad, groups)
    want = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=stride, padding=pad,
                                      dilation=d, groups=groups).numpy()
    assert got.shape == want.shape == (2, C, dil_cases.out_size(11, 3, stride, pad, d), dil_cases.out_size(13, 3, stride, pad, d))
    np.testing.assert_array_equal(got.astype(np.float64), want)


# ---- the builder
def _net(K=3, stride=1, pad=2, dilation=2, groups=1, C=16, hw=16, grouped=None):
    net = F8Net()
    if grouped is not None:
        net.set_option('grouped', grouped)
    t = net.input(C, hw, hw, 8)
    t = net.conv(t, np.ones((C, C // groups, K, K), np.int32), None, stride=stride, pad=pad, groups=groups, weight_fl=4, input_fl=8, input_signed=False,
                 quant_input=False, relu=True, dilation=dilation)
    net.output(t, as_float=False)
    return net


def _tokens(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


@pytest.mark.parametrize('K, stride, pad, d', [(3, 1, 2, 2), (3, 2, 0, 3), (3, 1, 7, 4), (5, 1, 4, 2), (7, 2, 3, 2), (3, 3, 1, 64), (2, 1, 1, 5)])
def test_plain_convs_of_any_geometry_are_accepted(K, stride, pad, d):
    net = _net(K, stride, pad, d, hw=16 if d < 64 else 140).finalize(2)
    tok = [t for t in _tokens(net) if t.startswith('conv')]
    assert len(tok) == 1 and tok[0].startswith(f'conv{K}x{K}s{stride}d{d}_t'), net.describe()
    hw = 16 if d < 64 else 140
    P = (hw + 2 * pad - d * (K - 1) - 1) // stride + 1
    assert net.outputs[0][:3] == (16, P, P)


def test_kernel_1_normalises_dilation_to_1():
    a, b = _net(1, 1, 0, 5).finalize(2), _net(1, 1, 0, 1).finalize(2)
    assert a.describe() == b.describe() and 'd5' not in a.describe()


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('d, pad', [(2, 0), (2, 1), (2, 2), (4, 3), (7, 7), (64, 64)])
def test_depthwise_kernel_3_with_pad_up_to_the_dilation_is_accepted(stride, d, pad):
    hw = 16 if d < 64 else 8
    net = _net(3, stride, pad, d, groups=16, hw=hw).finalize(2)
    tok = [t for t in _tokens(net) if t.startswith('dwconv')]
    assert len(tok) == 1 and tok[0].startswith(f'dwconv3x3s{stride}d{d}:'), net.describe()


def test_grouped_convs_are_always_the_dense_expansion():
    for grouped in (1, 2):
        net = _net(3, 1, 2, 2, groups=4, C=32, grouped=grouped).finalize(2)
        tok = [t for t in _tokens(net) if t.startswith('gconv')]
        assert len(tok) == 1 and tok[0].startswith('gconv3x3s1d2_dense:'), net.describe()
    with pytest.raises(_lib.F8Error) as e:                          # grouped = 0 refuses them, dilated or not
        _net(3, 1, 2, 2, groups=4, C=32)
    assert e.value.status == F8_ERR_UNSUPPORTED


@pytest.mark.parametrize('kw, status, words', [
    (dict(dilation=0), F8_ERR_INVALID, ('dilation 0', 'kernel 3')),
    (dict(dilation=-2), F8_ERR_INVALID, ('dilation -2',)),
    (dict(dilation=65, pad=65, hw=140), F8_ERR_UNSUPPORTED, ('dilation 65', '64')),
    (dict(K=5, dilation=2, pad=2, groups=16), F8_ERR_UNSUPPORTED, ('kernel 5', 'dilation 2', 'depthwise')),
    (dict(K=7, dilation=3, pad=3, groups=16, hw=32), F8_ERR_UNSUPPORTED, ('kernel 7', 'dilation 3', 'depthwise')),
    (dict(dilation=2, pad=3, groups=16), F8_ERR_UNSUPPORTED, ('pad 3', 'dilation 2', 'depthwise')),
    (dict(dilation=2, pad=2, stride=3, groups=16), F8_ERR_UNSUPPORTED, ('stride 3', 'depthwise')),
    (dict(dilation=8, pad=0), F8_ERR_INVALID, ('empty output', 'dilation 8', 'spans 17')),
    (dict(dilation=9, pad=1, groups=16), F8_ERR_INVALID, ('empty output', 'dilation 9')),
])
def test_refusals_name_the_geometry(kw, status, words):
    with pytest.raises(_lib.F8Error) as e:
        _net(**kw)
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert 'f8_net_conv_dilated' in str(e.value)


def test_a_null_desc_is_invalid():
    net = F8Net()
    t = net.input(16, 8, 8, 8)
    w = np.ones((16, 16, 3, 3), np.int32)
    assert net._L.f8_net_conv_dilated(net._h, t, None, 2, w.ctypes.data, None) == F8_ERR_INVALID


@pytest.mark.parametrize('groups, pad', [(1, 1), (1, 0), (16, 1), (16, 0)])
def test_dilation_1_through_the_new_entry_point_is_f8_net_conv(groups, pad):
    def build(dilated):
        net = F8Net()
        t = net.input(16, 12, 12, 8)
        w = (np.arange(16 * (16 // groups) * 9, dtype=np.int32).reshape(16, 16 // groups, 3, 3) % 13) - 6
        d = _lib.ConvDesc(cin=16, cout=16, kernel=3, stride=1, pad=pad, groups=groups, weight_fl=4, input_fl=8, input_signed=0, quant_input=0, relu=1)
        if dilated:
            t = _lib.check(net._L.f8_net_conv_dilated(net._h, t, ctypes.byref(d), 1, w.ctypes.data, None))
        else:
            t = _lib.check(net._L.f8_net_conv(net._h, t, ctypes.byref(d), w.ctypes.data, None))
        net.output(t, as_float=False)
        return net.finalize(4)
    a, b = build(True), build(False)
    assert a.describe() == b.describe()
    assert [a.launch_kernel(i) for i in range(a.num_launches)] == [b.launch_kernel(i) for i in range(b.num_launches)]
    assert a.weight_bytes == b.weight_bytes and a.arena_bytes == b.arena_bytes


# ---- plans of the case table
@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    return dil_cases.plan(name, case, dil_cases.make_input(name, case))


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    g, _, ids = _planned(name)
    assert dil_cases.d_lines(g.net) == dil_cases.expect(case), g.net.describe()
    assert len(dil_cases.d_lines(g.net)) == len(ids)                 # one launch per dilated conv, the residual join and an int32 form included
    if case['kind'] == 'dw':                                         # the dwk_dot4 = 0 leg: the generic kernel everywhere
        g0, _, _ = dil_cases.plan(name, case, dil_cases.make_input(name, case), dwk_dot4=0)
        assert dil_cases.d_lines(g0.net) == dil_cases.expect(case, dot4=False), g0.net.describe()
    if case['join_i32']:
        line = [ln for ln in g.net.describe().splitlines() if f"d{case['d']}" in ln.split(':')[0]][0]
        assert 'out[i32=1 i8=1' in line, g.net.describe()
    if case['res']:
        assert not any(t.startswith('add:') for t in _tokens(g.net)), g.net.describe()      # the join rides in the dilated conv's epilogue


@pytest.mark.parametrize('name', ['p_14x14_d2_pad2', 'p_9x11_d2_pad2_s2', 'd_c96_14x14_d2_pad2', 'dg_s2_d2', 'g_c32_cg4_d2'])
def test_launch_info_and_valu_count_the_nine_real_taps(name):
    case = ALL[name]
    g, _, _ = _planned(name)
    i = [k for k in range(g.net.num_launches) if g.net.launch_info(k, 1)[0].split(':')[0] + ':' == dil_cases.expect(case)[0][0]][0]
    P, Q = dil_cases.out_size(case['H'], 3, case['stride'], case['pad'], case['d']), dil_cases.out_size(case['W'], 3, case['stride'], case['pad'], case['d'])
    N, cin_g = case['N'], case['C'] // dil_cases.groups_of(case)
    assert g.net.launch_info(i, N)[2] == 2.0 * 9 * cin_g * case['cout'] * P * Q * N
    if case['kind'] == 'dw':                                         # one v_dot4 per four taps + three operations per requantised value
        assert g.net.launch_valu(i, N) == (9 * P * Q * case['C'] / 4.0 + 3.0 * P * Q * dil_cases._cs(case['C'])) * N


@pytest.mark.parametrize('tile', sorted(dil_cases.TILES))
def test_igemm_tile_forces_the_tile_of_a_dilated_conv(tile):
    name = dil_cases.TILE_CASE
    g, _, _ = dil_cases.plan(name, ALL[name], dil_cases.make_input(name, ALL[name]), igemm_tile=tile)
    assert dil_cases.d_lines(g.net) == dil_cases.expect(ALL[name], tile=dil_cases.TILES[tile]), g.net.describe()


def test_every_expected_kernel_is_an_exported_symbol():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    names = {k for c in ALL.values() for dot4 in (True, False) for _, k in dil_cases.expect(c, dot4)}
    names |= {k for t in dil_cases.TILES.values() for _, k in dil_cases.expect(ALL[dil_cases.TILE_CASE], tile=t)}
    assert 'f8::dwconv3x3_dil_dot4_kernel' in names and 'f8::dwconvk_kernel<true>' in names and 'f8::dwconvk_kernel<false>' in names
    for k in sorted(names):
        arg = 'f8::DwArgs' if 'dwconv' in k else 'f8::ConvArgs'
        assert (f'void {k}({arg})' if '<' in k else f' {k}({arg})') in syms, k      # (nm prints the return type of template instances only)


def test_bias_classes_of_the_case_whose_rows_lose_both_outer_taps():
    """7 x 7, d = 4, pad = 4, unsigned: output p reads rows p - 4, p, p + 4.  p = 0 .. 2: masks 110; p = 3: 010; p = 4 .. 6: 011 — three classes a side,
    nine bias vectors.  The table is not visible through the ABI; its effect is: with weights of one and a zero bias, an all-zero unsigned input
    (stored biased) must give exactly 0 at every pixel, which only the right 128 * sum(w over the in-image taps) per class does — and the reference's
    count of in-image taps, per pixel, with an input of ones."""
    net = F8Net()
    t = net.input(32, 7, 7, 8)
    t = net.conv(t, np.ones((32, 32, 3, 3), np.int32), None, stride=1, pad=4, groups=1, weight_fl=0, input_fl=8, input_signed=False, quant_input=False,
                 relu=False, dilation=4)
    net.output(t, as_float=False)
    net.finalize(1)
    want = oracle.conv2d(np.ones((1, 32, 7, 7), np.int32), stuffed(np.ones((32, 32, 3, 3), np.int32), 4), None, 1, 4, 1)
    rows = [2, 2, 2, 1, 2, 2, 2]                                     # in-image taps of an output row / column
    assert (want[0, 0] == 32 * np.outer(rows, rows)).all()
    # the weight image grows by the eight further bias vectors (32 int32 each) and the two class tables, against the one vector of a signed input
    signed = F8Net()
    t = signed.input(32, 7, 7, 7)
    t = signed.conv(t, np.ones((32, 32, 3, 3), np.int32), None, stride=1, pad=4, groups=1, weight_fl=0, input_fl=7, input_signed=True, quant_input=False,
                    relu=False, dilation=4)
    signed.output(t, as_float=False)
    signed.finalize(1)
    grown = net.weight_bytes - signed.weight_bytes
    assert 8 * 128 + 14 <= grown <= 8 * 128 + 14 + 3 * 256, grown   # (each table starts on a 256-byte boundary)


# ---- liveness on the reference
@pytest.mark.parametrize('name', sorted(ALL))
def test_every_case_is_live_on_the_reference(name):
    case = ALL[name]
    g, out, ids = dil_cases.reference(name)
    gc, outc, _ = dil_cases.reference(name, centre=True)
    y = g.v[out][0]
    assert np.unique(y).size > 16, name
    assert (y != gc.v[outc][0]).mean() > 0.25, name                 # the outer taps matter: not the same as the centre tap alone
    for t in ids:                                                    # the dilated conv's own result: neither all zero behind its ReLU nor constant
        v = g.v[t][0]
        assert (v != 0).mean() > 0.25 and np.unique(v).size > 16, name
    for label, xq, signed in g.taps:                                 # what the readers (and a second conv) read: 8 bits in use, not pinned at the clamps
        lo, hi = (-127, 127) if signed else (0, 255)
        assert ((xq == lo) | (xq == hi)).mean() < 0.6 and np.unique(xq).size > 16, (name, label)
    if case['bias_big']:
        assert (np.abs(g.raw[ids[0]].astype(np.int64)) > 2 ** 30).any(), name


# ---- topology.dilate
def _geo(spec):
    return {c.key: (c.stride, c.dilation, c.pad) for c in spec.convs() if c.k > 1}


def test_dilate_resnet50():
    os16, os8 = _geo(topology.get('resnet50_os16')), _geo(topology.get('resnet50_os8'))
    base = _geo(topology.get('resnet50'))
    want16, want8 = dict(base), dict(base)
    want16.update({'stage_3_layer_0.body.2': (1, 1, 1), 'stage_3_layer_1.body.2': (1, 2, 2), 'stage_3_layer_2.body.2': (1, 2, 2)})
    want8.update({'stage_2_layer_0.body.2': (1, 1, 1), **{f'stage_2_layer_{i}.body.2': (1, 2, 2) for i in range(1, 6)},
                  'stage_3_layer_0.body.2': (1, 2, 2), 'stage_3_layer_1.body.2': (1, 4, 4), 'stage_3_layer_2.body.2': (1, 4, 4)})
    assert os16 == want16 and os8 == want8
    assert base['stage_1_layer_0.body.2'] == os8['stage_1_layer_0.body.2'] == (2, 1, 1)
    for arch, shortcuts in (('resnet50_os16', {'stage_3_layer_0': 1, 'stage_2_layer_0': 2}), ('resnet50_os8', {'stage_3_layer_0': 1, 'stage_2_layer_0': 1, 'stage_1_layer_0': 2})):
        spec = topology.get(arch)
        assert spec.arch == arch
        for b in spec.blocks:
            if b.name in shortcuts:
                assert b.shortcut.stride == shortcuts[b.name] and b.shortcut.dilation == 1, (arch, b.name)
    r101 = _geo(topology.get('resnet101_os16'))
    assert r101['stage_3_layer_0.body.2'] == (1, 1, 1) and r101['stage_3_layer_2.body.2'] == (1, 2, 2) and r101['stage_2_layer_22.body.2'] == (1, 1, 1)


def test_dilate_mobilenet_v2():
    got, base = _geo(topology.get('mobilenet_v2_os16')), _geo(topology.get('mobilenet_v2'))
    want = dict(base)
    want.update({'stage_5_layer_0.body.2': (1, 1, 1), 'stage_5_layer_1.body.2': (1, 2, 2), 'stage_5_layer_2.body.2': (1, 2, 2), 'stage_6_layer_0.body.2': (1, 2, 2)})
    assert got == want
    assert base['stage_5_layer_0.body.2'] == (2, 1, 1) and got['stage_3_layer_0.body.2'] == (2, 1, 1)


def test_dilate_refuses_other_output_strides_and_leaves_its_argument_alone():
    spec = topology.get('resnet50')
    with pytest.raises(ValueError):
        topology.dilate(spec, 4)
    topology.dilate(spec, 8)
    assert _geo(spec) == _geo(topology.get('resnet50')) and spec.arch == 'resnet50'
    assert topology.ConvSpec('k', 1, 1, 3, 1, 1).dilation == 1
    assert [f.name for f in topology.ConvSpec.__dataclass_fields__.values()][-1] == 'dilation'


@pytest.mark.parametrize('arch, last', [('resnet50_os16', 14), ('resnet50_os8', 28), ('mobilenet_v2_os16', 14)])
def test_the_final_map_at_224(arch, last):
    spec = topology.get(arch)
    net = record_net(spec, synth.make_params(spec, 1), 224, taps=[spec.blocks[-1].name]).finalize(2)
    assert net.outputs[1][1:3] == (last, last)


# ---- no fused launch takes a dilated conv in
def _dilated_keys(spec):
    return [c.key for c in spec.convs() if c.dilation > 1]


@pytest.mark.parametrize('arch', ['resnet50_os16', 'resnet50_os8', 'mobilenet_v2_os16'])
@pytest.mark.parametrize('opts', [{}, FUSE_ALL], ids=['default', 'all_fusions'])
def test_every_dilated_conv_is_a_launch_of_its_own(arch, opts):
    spec = topology.get(arch)
    net = build_net(spec, synth.make_params(spec, 1), 2, hw=224, options=opts)
    toks = _tokens(net)
    for key in _dilated_keys(spec):
        mine = [t for t in toks if key in t]
        assert len(mine) == 1, (key, mine)
        head, names = mine[0].split(':', 1)
        assert names == key and (head.startswith('conv3x3s1d') or head.startswith('dwconv3x3s1d')), mine
    assert len(_dilated_keys(spec)) == {'resnet50_os16': 2, 'resnet50_os8': 8, 'mobilenet_v2_os16': 3}[arch]


@pytest.mark.parametrize('opts', [{}, FUSE_ALL], ids=['default', 'all_fusions'])
def test_the_undilated_stages_of_resnet50_os16_plan_as_those_of_resnet50(opts):
    """Stages 0 .. 2 are the same convs on the same maps: the same launches, token for token and symbol for symbol, up to the first launch of stage 3."""
    plans = []
    for arch in ('resnet50', 'resnet50_os16'):
        spec = topology.get(arch)
        net = build_net(spec, synth.make_params(spec, 1), 2, hw=224, options=opts)
        lines = [(net.launch_info(i, 2), net.launch_kernel(i)) for i in range(net.num_launches)]
        cut = min(i for i, (info, _) in enumerate(lines) if 'stage_3' in info[0])
        plans.append(lines[:cut])
    assert plans[0] == plans[1] and len(plans[0]) >= 4


# ---- ONNX
def test_the_onnx_round_trip_preserves_dilation():
    spec = topology.get('mobilenet_v2_os16')
    params = synth.make_params(spec, 5)
    ig = onnx_export.graph_from_params(spec, params, 64)
    assert sorted(o.key for o in ig.ops if o.kind == 'conv' and o.dilation == 2) == sorted(_dilated_keys(spec))
    model = onnx_export.export_graph(ig)
    convs = [n for n in onnx_io.load_graph(model).nodes if n.op == 'Conv']
    assert sorted({tuple(n.attrs['dilations']) for n in convs}) == [(1, 1), (2, 2)]
    back = onnx_import.import_graph(model, input_signed=spec.normalize)
    assert [(o.key, o.dilation, o.pad, o.stride) for o in back.ops if o.kind == 'conv'] == [(o.key, o.dilation, o.pad, o.stride) for o in ig.ops if o.kind == 'conv']
    a, b = ig.build_net(2), back.build_net(2)
    assert a.describe() == b.describe() and 'dwconv3x3s1d2:' in a.describe()
    x = synth.rand_uniform_int(6, 'onnx_x', (1, 3, 64, 64), 0, 255).astype(np.int32)
    np.testing.assert_array_equal(graph_forward(back, x), graph_forward(ig, x))
    # unequal dilations are refused
    bad = onnx_io.load_graph(model)
    next(n for n in bad.nodes if n.op == 'Conv' and tuple(n.attrs['dilations']) == (2, 2)).attrs['dilations'] = [2, 1]
    with pytest.raises(onnx_import.OnnxImportError, match='equal dilations'):
        onnx_import.import_graph(bad)


@pytest.mark.parametrize('arch', ['mobilenet_v2_os16', 'resnet50_os8'])
def test_the_importer_names_a_dilated_net_and_builds_its_module_tree(arch):
    """detect_arch: the `_os` form whose strides, pads and dilations the graph has — an IntModel built from the undilated entry would compute another net."""
    spec = topology.get(arch)
    model = onnx_export.export_graph(onnx_export.graph_from_params(spec, synth.make_params(spec, 5), 64))
    assert onnx_import.detect_arch(onnx_import.import_graph(model)) == arch
    m = onnx_import.int_model_from_onnx(model)
    got = {n: (c.stride[0], c.dilation[0], c.padding[0]) for n, c in m.named_modules() if isinstance(c, torch.nn.Conv2d) and c.kernel_size[0] > 1}
    assert got == _geo(spec)
    odd = onnx_import.import_graph(model)
    next(o for o in odd.ops if o.kind == 'conv' and o.dilation > 1).dilation = 3      # no table entry has this geometry
    assert onnx_import.detect_arch(odd) is None
