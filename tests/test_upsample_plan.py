"""Upsampling on the CPU: f8_net_upsample's acceptance and refusals, shapes and fraclens, the mode token and kernel symbol every case of
tests/upsample_cases.py plans on both legs of option upsample_i8 — written by hand there —, the forms asked of the source, launch_info / launch_valu,
where an upsample cuts the fused launches of ResNet-50 and MobileNet-V2 (exactly where an output tap does), the ONNX Resize in both directions with
its refusals, the reference pinned to torch in float64, the option key.  tests/test_gpu_upsample.py runs every case on the device."""
import numpy as np
import pytest

import ref_ops
import upsample_cases as uc
from f8net_amd import onnx_export, onnx_import, onnx_io, synth, topology
from f8net_amd._lib import F8Error
from f8net_amd.net import F8Net, build_net, record_net
from graph_cases import same_ops
from refgraph import graph_forward

INVALID, UNSUPPORTED, STATE = -1, -2, -5


def _w(cout, cin, k=1):
    return np.ones((cout, cin, k, k), np.int32)


def _one(C=40, H=3, W=5, fl=8, w_fl=5):
    """input (8 channels, H x W) -> a 1x1 conv; returns (net, input id, conv id)."""
    net = F8Net()
    x = net.input(8, H, W, fl)
    t = net.conv(x, _w(C, 8), None, stride=1, pad=0, groups=1, weight_fl=w_fl, input_fl=fl, input_signed=False, quant_input=False)
    return net, x, t


# ---- the C ABI
@pytest.mark.parametrize('mode, scale, shape', [('nearest', (3, 5), (40, 9, 25, 13)), ('nearest', 2, (40, 6, 10, 13)), ('nearest', (1, 4), (40, 3, 20, 13)),
                                                ('nearest', (256, 1), (40, 768, 5, 13)), ('bilinear', 2, (40, 6, 10, 17)), ('bilinear', 4, (40, 12, 20, 19)),
                                                ('bilinear', 8, (40, 24, 40, 21)), ('bilinear', (16, 16), (40, 48, 80, 23))])
def test_acceptance_shape_and_fraclen(mode, scale, shape):
    net, x, t = _one()
    u = net.upsample(t, scale, mode, label='up')
    net.output(u, as_float=False)
    net.finalize(2)
    assert net.output_info(0) == shape + (False,)
    assert ('upsample_nearest_i32:up' if mode == 'nearest' else 'upsample_bilinear_i32:up') in net.describe()


def test_bilinear_up_to_fraclen_32_is_accepted():
    net, x, t = _one(fl=8, w_fl=22)                                # fraclen 30
    with pytest.raises(F8Error) as e:
        net.upsample(t, 2, 'bilinear')                            # 34
    assert e.value.status == INVALID
    net, x, t = _one(fl=8, w_fl=20)                                # 28 + 4 = 32
    assert net.upsample(t, 2, 'bilinear') >= 0
    assert net.upsample(t, 256, 'nearest') >= 0                    # nearest keeps the fraclen: no bound


@pytest.mark.parametrize('what, status', [
    ('bad_id', INVALID), ('negative_id', INVALID), ('scale0', INVALID), ('scale_neg', INVALID), ('both1', INVALID), ('both1_bilinear', INVALID),
    ('mode2', INVALID), ('mode_neg', INVALID), ('fraclen', INVALID),
    ('nearest257', UNSUPPORTED), ('nearest_w257', UNSUPPORTED), ('bilinear_unequal', UNSUPPORTED), ('bilinear3', UNSUPPORTED), ('bilinear32', UNSUPPORTED),
    ('bilinear_1_2', UNSUPPORTED), ('finalized', STATE)])
def test_refusals(what, status):
    net, x, t = _one(w_fl=22 if what == 'fraclen' else 5)
    args = {'bad_id': (99, 0, 2, 2), 'negative_id': (-1, 0, 2, 2), 'scale0': (t, 0, 0, 2), 'scale_neg': (t, 0, 2, -1), 'both1': (t, 0, 1, 1),
            'both1_bilinear': (t, 1, 1, 1), 'mode2': (t, 2, 2, 2), 'mode_neg': (t, -1, 2, 2), 'fraclen': (t, 1, 4, 4), 'nearest257': (t, 0, 257, 1),
            'nearest_w257': (t, 0, 2, 257), 'bilinear_unequal': (t, 1, 2, 4), 'bilinear3': (t, 1, 3, 3), 'bilinear32': (t, 1, 32, 32),
            'bilinear_1_2': (t, 1, 1, 2), 'finalized': (t, 0, 2, 2)}[what]
    if what == 'finalized':
        net.output(t, as_float=False)
        net.finalize(1)
    from f8net_amd._lib import lib
    assert lib().f8_net_upsample(net._h, *args) == status


def test_python_wrapper_refuses_an_unknown_mode_name():
    net, x, t = _one()
    with pytest.raises(ValueError, match='bicubic'):
        net.upsample(t, 2, 'bicubic')


# ---- modes and kernels
@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_mode_and_kernel_of_every_case(name):
    c = uc.CASES[name]
    x = uc.make_input(name)
    for opts in ({}, uc.FUSE_ALL):
        g, _, ups = uc.plan(name, x, max_batch=c['N'] + 1, **opts)
        assert [(t, k) for _, t, k in uc.upsample_lines(g.net)] == [(c['tok'], uc.SYMBOL[c['tok']])] * len(ups), g.net.describe()
    g, _, ups = uc.plan(name, x, upsample_i8=0)
    assert [(t, k) for _, t, k in uc.upsample_lines(g.net)] == [(c['tok_off'], uc.SYMBOL[c['tok_off']])] * len(ups), g.net.describe()
    ref, outs, rups = uc.reference(name)                           # the case carries values
    assert all(np.unique(ref.v[o][0]).size > 8 for o in outs + rups)                # (b_1x1_k1: 8 channels x 3 images of one pixel)


def _line(net, i):
    return net.describe().splitlines()[i]


@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_forms_written_by_the_launch_and_asked_of_the_source(name):
    """describe() shows per launch which forms it writes.  The upsample writes the case's hand-written forms; its source's producer (the launch in
    front of it, or of the lateral / skip in between) writes int8 forms only in the i8 mode and the int32 form in the int32 mode."""
    c = uc.CASES[name]
    g, _, _ = uc.plan(name, uc.make_input(name))
    (i, tok, _), = uc.upsample_lines(g.net)
    o32, o8 = c['forms']
    assert f'out[i32={o32} i8={o8} ' in _line(g.net, i), g.net.describe()
    src = max(j for j in range(i) if _line(g.net, j).split()[1].startswith('conv'))
    if tok == uc.I8:
        assert f'out[i32=0 i8={o8} ' in _line(g.net, src), g.net.describe()
        assert all('requant:' not in l for l in g.net.describe().splitlines()[:i + 1])
    else:
        assert 'out[i32=1 i8=0 ' in _line(g.net, src), g.net.describe()
    extra = sum('requant:up' in l for l in g.net.describe().splitlines())
    assert extra == (1 if name.endswith('three') else 0)


# (the launch's bytes and essential vector work by hand: C real channels, Cs padded, in / out pixels per image)
@pytest.mark.parametrize('name, C, Cs, ipx, opx', [('n_3x5_two', 40, 64, 15, 60), ('n_7x7_three', 64, 64, 49, 196), ('b_out_reader', 64, 64, 15, 60),
                                                    ('n_bcast33', 32, 32, 1, 1089), ('b_3x5_k4', 8, 32, 15, 3840)])
def test_launch_info_and_valu_by_hand(name, C, Cs, ipx, opx):
    g, _, _ = uc.plan(name, uc.make_input(name))
    (i, tok, _), = uc.upsample_lines(g.net)
    o32, o8 = uc.CASES[name]['forms']
    for N in (1, 5):
        _, nbytes, ops = g.net.launch_info(i, N)
        assert ops == 0
        if tok == uc.I8:                                           # every real byte read once and written once, per form
            assert nbytes == N * (ipx + opx) * C * o8
            assert g.net.launch_valu(i, N) == 0
        else:
            assert nbytes == N * (ipx * C * 4 + opx * Cs * (4 * o32 + o8))
            assert g.net.launch_valu(i, N) == N * opx * C * ((4 if tok == uc.B32 else 0) + 3 * o8)
    if name == 'n_3x5_two':
        assert g.net.launch_info(i, 1)[1] == 75 * 40 * 2
        g, _, _ = uc.plan(name, uc.make_input(name), upsample_i8=0)
        (i, _, _), = uc.upsample_lines(g.net)
        assert g.net.launch_info(i, 1)[1] == 15 * 40 * 4 + 60 * 64 * 2 and g.net.launch_valu(i, 1) == 60 * 40 * 6


# ---- an upsample cuts fused launches where a tap does
def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _backbone(net):
    return [n for n in _names(net) if not n.startswith(('tap:', 'upsample_'))]


# (MobileNet-V2: a block output inside the 14 x 14 run that fuse_irchain makes one launch of)
@pytest.mark.parametrize('arch, name', [('resnet50', 'stage_1_layer_1'), ('mobilenet_v2', 'stage_3_layer_2')])
@pytest.mark.parametrize('mode', ['nearest', 'bilinear'])
def test_an_upsample_cuts_the_chain_where_a_tap_does(arch, name, mode):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=7)
    plain = build_net(spec, params, 8, options=uc.FUSE_ALL)
    tapped = build_net(spec, params, 8, options=uc.FUSE_ALL, taps=(name,))
    net = record_net(spec, params, options=uc.FUSE_ALL)
    up = net.upsample(net.tap_ids[name], 2, mode, label='up')
    assert net.output(up, as_float=False) == 1
    for k, v in uc.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(8)
    assert _backbone(net) == _backbone(tapped)
    assert net.num_launches == tapped.num_launches + 1             # one tap there; here the upsample and the tap on it
    assert _backbone(plain) != _backbone(tapped), 'the tensor does not cut any fused launch: the comparison shows nothing'
    assert [n for n in _names(net) if n.startswith('upsample_')] == [f'upsample_{mode}_i32:up']


# ---- ONNX
@pytest.mark.parametrize('name', ['n_3x5_s35', 'n_unet_i8', 'b_3x5_k4', 'b_fpn'])
def test_onnx_round_trip(name):
    c = uc.CASES[name]
    ig, g, out = uc.int_graph(name)
    assert sum(o.kind == 'upsample' for o in ig.ops) == 1
    data = onnx_export.export_graph(ig)
    (rs,) = [n for n in onnx_io.load_graph(data).nodes if n.op == 'Resize']
    if c['mode'] == 'nearest':
        assert (rs.attrs['mode'], rs.attrs['coordinate_transformation_mode'], rs.attrs['nearest_mode']) == (b'nearest', b'asymmetric', b'floor')
    else:
        assert (rs.attrs['mode'], rs.attrs['coordinate_transformation_mode']) == (b'linear', b'half_pixel')
    back = onnx_import.import_graph(data)
    same_ops(ig, back)
    assert back.solve_fraclens(uc.X_FL) == ig.solve_fraclens(uc.X_FL)
    x = uc.make_input(name)
    np.testing.assert_array_equal(graph_forward(back, x, uc.X_FL), g.v[out][0])      # the walker against RefGraph's values
    net = back.build_net(2, input_fraclen=uc.X_FL)
    assert [(t, k) for _, t, k in uc.upsample_lines(net)] == [(c['tok'], uc.SYMBOL[c['tok']])]


def _model(name, edit):
    ig, _, _ = uc.int_graph(name)
    g = onnx_io.load_graph(onnx_export.export_graph(ig))
    rs = next(n for n in g.nodes if n.op == 'Resize')
    edit(g, rs)
    return g


def _const(g, name, value):
    g.nodes.insert(0, onnx_io.Node('Constant', [], [name], name=name, attrs={'value': value}))
    return name


def _drop_mul(g, rs):
    mul = next(n for n in g.nodes if n.op == 'Mul' and n.inputs[0] == rs.outputs[0])
    for n in g.nodes:
        n.inputs = [rs.outputs[0] if s == mul.outputs[0] else s for s in n.inputs]
    g.nodes.remove(mul)


def _wrong_mul(g, rs):
    mul = next(n for n in g.nodes if n.op == 'Mul' and n.inputs[0] == rs.outputs[0])
    mul.inputs[1] = _const(g, 'eight', np.array(8.0, np.float32))


def _scales_from_input(g, rs):
    rs.inputs[2] = rs.inputs[0]


@pytest.mark.parametrize('name, edit, match', [
    ('b_3x5_k1', _drop_mul, 'without the Mul'),
    ('b_3x5_k1', _wrong_mul, 'Mul by 2\\^4 = 16'),
    ('b_3x5_k1', lambda g, rs: rs.attrs.__setitem__('coordinate_transformation_mode', b'align_corners'), "align_corners"),
    ('b_3x5_k1', lambda g, rs: rs.attrs.__setitem__('coordinate_transformation_mode', b'asymmetric'), 'asymmetric'),
    ('b_3x5_k1', lambda g, rs: rs.attrs.__setitem__('mode', b'cubic'), 'cubic'),
    ('b_3x5_k1', lambda g, rs: rs.inputs.__setitem__(2, _const(g, 'sc3', np.array([1, 1, 3, 3], np.float32))), 'equal scales of 2, 4, 8 or 16'),
    ('n_3x5_s35', lambda g, rs: rs.attrs.__setitem__('coordinate_transformation_mode', b'half_pixel'), 'half_pixel'),
    ('n_3x5_s35', lambda g, rs: rs.attrs.__setitem__('nearest_mode', b'round_prefer_floor'), 'round_prefer_floor'),
    ('n_3x5_s35', lambda g, rs: rs.inputs.append(_const(g, 'sizes', np.array([2, 40, 9, 25], np.int64))), 'sizes'),
    ('n_3x5_s35', _scales_from_input, 'not a constant'),
    ('n_3x5_s35', lambda g, rs: rs.inputs.__setitem__(2, _const(g, 'sc', np.array([1, 1, 1.5, 2], np.float32))), 'integer sh, sw'),
    ('n_3x5_s35', lambda g, rs: rs.inputs.__setitem__(2, _const(g, 'sc', np.array([1, 2, 2, 2], np.float32))), 'expected \\[1, 1, sh, sw\\]'),
])
def test_onnx_import_refusals(name, edit, match):
    with pytest.raises(onnx_import.OnnxImportError, match=match):
        onnx_import.import_graph(_model(name, edit))


def test_onnx_pytorch_half_pixel_is_accepted():
    ig, _, _ = uc.int_graph('b_3x5_k1')
    same_ops(ig, onnx_import.import_graph(_model('b_3x5_k1', lambda g, rs: rs.attrs.__setitem__('coordinate_transformation_mode', b'pytorch_half_pixel'))))


# ---- the reference
@pytest.mark.parametrize('k', [1, 2, 3, 4])
@pytest.mark.parametrize('hw', [(1, 1), (1, 3), (3, 1), (2, 2), (3, 5), (7, 7)])
def test_bilinear_reference_is_torch_float64_times_4s2(k, hw):
    x = synth.rand_uniform_int(9, f'pin{k}{hw}', (2, 3) + hw, -2 ** 30, 2 ** 30)
    uc.pin_to_torch(x, k)
    y, fl = ref_ops.upsample_ref(x.astype(np.int32), 5, 1 << k, 'bilinear')
    assert fl == 5 + 2 * k + 2 and y.dtype == np.int32 and y.shape == (2, 3, hw[0] << k, hw[1] << k)
    np.testing.assert_array_equal(y, ref_ops.wrap32(ref_ops.bilinear_exact(x, k)))


def test_nearest_reference_is_torch_nearest():
    import torch
    x = synth.rand_uniform_int(9, 'pinn', (2, 3, 3, 5), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    y, fl = ref_ops.upsample_ref(x, 5, (3, 2), 'nearest')
    want = torch.nn.functional.interpolate(torch.from_numpy(x.astype(np.float64)), scale_factor=(3, 2), mode='nearest').numpy()
    assert fl == 5
    np.testing.assert_array_equal(y.astype(np.float64), want)


def test_wrap_case_leaves_the_int32_range_before_wrapping():
    ref, _, (up,) = uc.reference('b_wrap')
    g, _, _ = uc.build_graph('b_wrap', uc.make_input('b_wrap', uc.CASES['b_wrap']['N'] + 1), record=False)     # (the builder asserts it as well)
    exact = ref_ops.bilinear_exact(next(v for t, (v, fl) in ref.v.items() if t not in (0, up)), 4)
    assert (np.abs(exact) >= 2 ** 31).sum() > 1000 and (exact != ref.v[up][0]).sum() > 1000
    np.testing.assert_array_equal(ref.v[up][0], ref_ops.wrap32(exact))


# ---- the option key
def test_option_key():
    net, x, t = _one()
    assert net.get_option('upsample_i8') == 1
    net.set_option('upsample_i8', 0)
    assert net.get_option('upsample_i8') == 0
    for bad in (2, -1):
        with pytest.raises(F8Error) as e:
            net.set_option('upsample_i8', bad)
        assert e.value.status == INVALID
    net.output(net.upsample(t, 2), as_float=False)
    net.finalize(1)
    with pytest.raises(F8Error) as e:
        net.set_option('upsample_i8', 1)                          # a planning key: not after finalize
    assert e.value.status == STATE


def test_option_default_comes_from_the_environment(monkeypatch):
    monkeypatch.setenv('F8_UPSAMPLE_I8', '0')
    assert F8Net().get_option('upsample_i8') == 0
    monkeypatch.delenv('F8_UPSAMPLE_I8')
    assert F8Net().get_option('upsample_i8') == 1
