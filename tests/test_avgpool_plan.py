"""Windowed average pooling on the CPU: f8_net_avgpool_window's acceptance and every refusal with its status and message, shapes and fraclens, the
global window recorded as the avgpool_sum node (ResNet-18's tail plans the same text), the plan token and kernel symbol every case of
tests/avgpool_cases.py plans on the three legs of option sumpool_wide — written by hand there —, the forms written, launch_info / launch_valu by
hand, where a pool cuts the fused launches of ResNet-50 and MobileNet-V2 (exactly where an output tap does), the reference pinned to torch in
float64 and to the oracle's depthwise conv, adaptive_avgpool, ONNX AveragePool in both directions with its refusals, the torch op's meta shape, the
option key, the shipped nets' plan digests, and examples/avgpool_host.c with the host code under ASan / UBSan as a stand-alone program.
tests/test_gpu_avgpool.py runs every case on the device."""
import numpy as np
import pytest

import avgpool_cases as ac
import ref_ops
from f8net_amd import onnx_export, onnx_import, onnx_io, synth, topology
from f8net_amd._lib import F8Error, lib
from f8net_amd.net import F8Net, build_net, record_net
from graph_cases import plan_digest_tool, same_ops, sanitized_host_program, shipped_digest_membership
from refgraph import RefGraph, graph_forward

INVALID, UNSUPPORTED, STATE = -1, -2, -5


def _w(cout, cin, k=1):
    return np.ones((cout, cin, k, k), np.int32)


def _one(C=40, H=7, W=9, fl=8, w_fl=5):
    """input (8 channels, H x W) -> a 1x1 conv; returns (net, input id, conv id)."""
    net = F8Net()
    x = net.input(8, H, W, fl)
    t = net.conv(x, _w(C, 8), None, stride=1, pad=0, groups=1, weight_fl=w_fl, input_fl=fl, input_signed=False, quant_input=False)
    return net, x, t


# ---- the C ABI
@pytest.mark.parametrize('k, s, pad, shift, shape', [
    (2, None, 0, None, (40, 3, 4, 15)), (3, 1, 1, None, (40, 7, 9, 16)), (3, 2, 1, None, (40, 4, 5, 16)), (3, 2, 0, None, (40, 3, 4, 16)),
    (2, 3, 1, None, (40, 3, 4, 15)), (4, 2, 2, None, (40, 4, 5, 17)), (1, 2, 0, None, (40, 4, 5, 13)), (7, 7, 0, None, (40, 1, 1, 19)),
    (7, 1, 0, 0, (40, 1, 3, 13)), (2, 64, 0, 5, (40, 1, 1, 18)), (5, 1, 2, 19, (40, 7, 9, 32))])
def test_acceptance_shape_and_fraclen(k, s, pad, shift, shape):
    net, x, t = _one()
    p = net.avgpool(t, k, s, pad, shift, label='pool')
    assert net.tensor_info(p) == shape
    net.output(p, as_float=False)
    net.finalize(2)
    assert net.output_info(0) == shape + (False,)
    assert f'sumpool{k}x{k}s{k if s is None else s}:pool' in net.describe()


def test_default_shift_is_the_references():
    assert [ref_ops.default_shift(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 15, 30, 64)] == [0, 2, 3, 4, 5, 5, 6, 6, 8, 10, 12]
    import torch
    for k in (2, 3, 5, 7, 11, 15):                                 # FXQAvgPool2d.__init__ (fix_quant_ops.py:121-122)
        assert ref_ops.default_shift(k) == int(torch.round(torch.log2(torch.tensor(float(k ** 2)))).item())


@pytest.mark.parametrize('what, status, match', [
    ('bad_id', INVALID, 'tensor'), ('negative_id', INVALID, 'tensor'), ('kernel0', INVALID, 'bad geometry'), ('stride0', INVALID, 'bad geometry'),
    ('pad_neg', INVALID, 'bad geometry'), ('pad_above_half', INVALID, 'bad geometry'), ('identity', INVALID, 'identity'),
    ('window_too_large', INVALID, 'larger than the padded'), ('window_too_wide', INVALID, 'larger than the padded'), ('shift_neg', INVALID, 'shift -1'),
    ('fraclen', INVALID, 'fraclen 33 > 32'), ('kernel65', UNSUPPORTED, 'above 64'), ('stride65', UNSUPPORTED, 'above 64'),
    ('finalized', STATE, 'finalized')])
def test_refusals(what, status, match):
    net, x, t = _one()
    args = {'bad_id': (99, 2, 2, 0, 2), 'negative_id': (-1, 2, 2, 0, 2), 'kernel0': (t, 0, 1, 0, 0), 'stride0': (t, 2, 0, 0, 2), 'pad_neg': (t, 2, 2, -1, 2),
            'pad_above_half': (t, 3, 1, 2, 3), 'identity': (t, 1, 1, 0, 0), 'window_too_large': (t, 8, 8, 0, 6), 'window_too_wide': (t, 10, 1, 1, 7),
            'shift_neg': (t, 2, 2, 0, -1), 'fraclen': (t, 2, 2, 0, 20), 'kernel65': (t, 65, 1, 32, 12), 'stride65': (t, 2, 65, 0, 2),
            'finalized': (t, 2, 2, 0, 2)}[what]
    if what == 'finalized':
        net.output(t, as_float=False)
        net.finalize(1)
    assert lib().f8_net_avgpool_window(net._h, *args) == status
    assert match in lib().f8_last_error().decode(), lib().f8_last_error()


def test_null_net_is_refused():
    assert lib().f8_net_avgpool_window(None, 0, 2, 2, 0, 2) == INVALID


def test_fraclen_32_is_accepted():
    net, x, t = _one()
    assert net.avgpool(t, 2, 2, 0, 19) >= 0                        # 13 + 19


# ---- the global window is the avgpool_sum node
def test_global_window_records_the_avgpool_sum_node():
    for H, W, k, pad, glob_ in ((7, 7, 7, 0, True), (7, 9, 7, 0, False), (8, 8, 4, 0, False), (6, 6, 6, 3, False), (1, 1, 1, 0, None)):
        net, x, t = _one(H=H, W=W)
        if glob_ is None:                                          # kernel 1 on a 1 x 1 map needs stride 2 to be accepted; then it is the global window
            p = net.avgpool(t, 1, 2, 0, 0, label='pool')
        else:
            p = net.avgpool(t, k, k, pad, label='pool')
        net.output(p, as_float=False)
        net.finalize(2)
        text = net.describe()
        assert ('avgpool_sum:pool' in text) == (glob_ is not False) and ('sumpool' in text) == (glob_ is False), text
    a, b = _one(H=7, W=7), _one(H=7, W=7)
    a[0].output(a[0].avgpool(a[2], 7, 3, 0, 6), as_float=False)    # (the stride does not matter: one window)
    b[0].output(b[0].avgpool_sum(b[2], 6), as_float=False)
    a[0].finalize(3), b[0].finalize(3)
    assert a[0].describe() == b[0].describe() and a[0].output_info(0) == b[0].output_info(0) == (40, 1, 1, 19, False)


@pytest.mark.parametrize('fuse_pool', [1, 0])
def test_resnet18_tail_plans_the_same_through_the_window_call(fuse_pool, monkeypatch):
    spec = topology.get('resnet18')
    params = synth.make_params(spec, seed=7)
    opts = dict(ac.FUSE_ALL, fuse_pool=fuse_pool)
    want = build_net(spec, params, 8, options=opts).describe()
    assert ('+avgpool' in want) == bool(fuse_pool) and ('avgpool_sum:' in want) == (not fuse_pool), want
    monkeypatch.setattr(F8Net, 'avgpool_sum', lambda self, src, shift=6, label=None: self.avgpool(src, 7, 7, 0, shift, label=label))
    assert build_net(spec, params, 8, options=opts).describe() == want


# ---- tokens, kernels, forms
@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_token_and_kernel_of_every_case_on_every_leg(name):
    c = ac.CASES[name]
    x = ac.make_input(name)
    for leg in (0, 1, 2):
        for opts in ({}, ac.FUSE_ALL):
            g, _, pools = ac.plan(name, x, max_batch=c['N'] + 1, sumpool_wide=leg, **opts)
            want = [] if c['forms'] is None else [(ac.token(c), ac.symbol(c, leg))]
            assert [(t, k) for _, t, k in ac.pool_lines(g.net)] == want, g.net.describe()
    if c['forms'] is None:
        assert sum('avgpool_sum:pool' in l for l in g.net.describe().splitlines()) == 1
    ref, outs, rpools = ac.reference(name)                         # the case carries values
    assert all(np.unique(ref.v[o][0]).size > 8 for o in outs + rpools)


def test_the_legs_differ_where_the_table_says():
    """The table exercises every instance: the walker's three and the wide kernel, and the default leg takes both sides of the crossover."""
    per_leg = {leg: {ac.symbol(c, leg) for c in ac.CASES.values() if c['forms'] is not None} for leg in (0, 1, 2)}
    walkers = {'f8::sumpool_i32_kernel<0>', 'f8::sumpool_i32_kernel<2>', 'f8::sumpool_i32_kernel<3>'}
    assert per_leg[0] == walkers and per_leg[1] == walkers | {'f8::sumpool_wide_kernel'}
    assert per_leg[2] == {'f8::sumpool_wide_kernel', 'f8::sumpool_i32_kernel<0>'}                # (kernel 1 stays on the walker)
    assert ac.symbol(ac.CASES['g_15s15_15x30'], 1) == 'f8::sumpool_wide_kernel'


def _line(net, i):
    return net.describe().splitlines()[i]


@pytest.mark.parametrize('name', ac.POOLED)
def test_forms_written_by_the_launch_and_asked_of_the_source(name):
    """describe() shows per launch which forms it writes: the pool writes the case's hand-written forms, its source's producer the int32 form (and
    nothing else unless something else reads it), and a third int8 format is a `requant:` step."""
    c = ac.CASES[name]
    g, _, _ = ac.plan(name, ac.make_input(name))
    (i, tok, _), = ac.pool_lines(g.net)
    o32, o8 = c['forms']
    assert f'out[i32={o32} i8={o8} ' in _line(g.net, i), g.net.describe()
    src = max(j for j in range(i) if _line(g.net, j).split()[1].startswith('conv'))
    assert 'out[i32=1 i8=0 ' in _line(g.net, src), g.net.describe()
    assert sum('requant:pool' in l for l in g.net.describe().splitlines()) == (1 if name == 'r_three' else 0)


# (the launch's bytes and essential vector work by hand: C real channels, Cs padded, source / output pixels per image, kernel)
@pytest.mark.parametrize('name, C, Cs, ipx, opx, k', [('g_2s2_7x9', 40, 64, 63, 12, 2), ('g_3s1p1_5x7', 64, 64, 35, 35, 3), ('r_three', 64, 64, 63, 12, 2),
                                                       ('r_out_reader', 64, 64, 63, 20, 3), ('g_15s15_15x30', 64, 64, 450, 2, 15), ('g_1s2_7x9', 24, 32, 63, 20, 1)])
def test_launch_info_and_valu_by_hand(name, C, Cs, ipx, opx, k):
    o32, o8 = ac.CASES[name]['forms']
    for leg in (0, 2):
        g, _, _ = ac.plan(name, ac.make_input(name), sumpool_wide=leg)
        (i, tok, _), = ac.pool_lines(g.net)
        for N in (1, 5):
            _, nbytes, ops = g.net.launch_info(i, N)
            assert ops == 0
            assert nbytes == N * (ipx * Cs * 4 + opx * Cs * (4 * o32 + o8))
            assert g.net.launch_valu(i, N) == N * opx * C * (k * k - 1 + 3 * o8)


# ---- a pool cuts fused launches where a tap does
def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _backbone(net):
    return [n for n in _names(net) if not n.startswith(('tap:', 'sumpool'))]


# (MobileNet-V2: a block output inside the 14 x 14 run that fuse_irchain makes one launch of)
@pytest.mark.parametrize('arch, name', [('resnet50', 'stage_1_layer_1'), ('mobilenet_v2', 'stage_3_layer_2')])
def test_a_pool_cuts_the_chain_where_a_tap_does(arch, name):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=7)
    plain = build_net(spec, params, 8, options=ac.FUSE_ALL)
    tapped = build_net(spec, params, 8, options=ac.FUSE_ALL, taps=(name,))
    net = record_net(spec, params, options=ac.FUSE_ALL)
    pl = net.avgpool(net.tap_ids[name], 2, label='pool')
    assert net.output(pl, as_float=False) == 1
    for k, v in ac.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(8)
    assert _backbone(net) == _backbone(tapped)
    assert net.num_launches == tapped.num_launches + 1             # one tap there; here the pool and the tap on it
    assert _backbone(plain) != _backbone(tapped), 'the tensor does not cut any fused launch: the comparison shows nothing'
    assert [n for n in _names(net) if n.startswith('sumpool')] == ['sumpool2x2s2:pool']


@pytest.mark.parametrize('name', sorted(ac.NETS))
def test_small_nets_plan(name):
    build, _, pools = ac.NETS[name]
    x = ac.net_input(name)
    for opts in ({}, ac.FUSE_ALL):
        g = RefGraph(x, ac.X_FL)
        build(g, next(iter(g.v)))
        for k, v in opts.items():
            g.net.set_option(k, v)
        g.net.finalize(2)
        assert [t for _, t, _ in ac.pool_lines(g.net)] == pools, g.net.describe()


# ---- the reference
GRID = [(k, s, pad) for k in (1, 2, 3, 4, 5, 7) for s in (1, 2, 3, 7) for pad in range(k // 2 + 1) if not (k == 1 and s == 1)]


@pytest.mark.parametrize('hw', [(7, 9), (8, 8), (15, 30)])
def test_reference_is_torch_float64_with_divisor_1(hw):
    x = synth.rand_uniform_int(9, f'pin{hw}', (2, 3) + hw, -2 ** 27 + 1, 2 ** 27 - 1)
    small = synth.rand_uniform_int(10, f'pin8{hw}', (2, 3) + hw, -127, 255)
    for k, s, pad in GRID + [(15, 15, 0), (6, 6, 3)]:
        if hw[0] + 2 * pad < k:
            continue
        ac.pin_to_torch(x, k, s, pad)
        ac.pin_to_oracle(small, k, s, pad)
        y, fl = ref_ops.sumpool_ref(x.astype(np.int32), 5, k, s, pad)
        assert fl == 5 + ref_ops.default_shift(k) and y.dtype == np.int32 and y.shape == (2, 3, ac.out_size(hw[0], k, s, pad), ac.out_size(hw[1], k, s, pad))


def test_the_issues_six_geometries_on_7x9():
    x = synth.rand_uniform_int(9, 'pin6', (2, 3, 7, 9), -2 ** 27 + 1, 2 ** 27 - 1)
    for k, s, pad in ((2, 2, 0), (3, 1, 1), (2, 3, 1), (3, 2, 0), (7, 7, 0), (4, 2, 2)):
        ac.pin_to_torch(x, k, s, pad)


def test_wrap_case_leaves_the_int32_range_before_wrapping():
    c = ac.CASES['w_wrap']
    ref, _, (pl,) = ac.reference('w_wrap')
    src = next(v for t, (v, fl) in ref.v.items() if t not in (0, pl))
    exact = ref_ops.sumpool_exact(src, c['k'], c['s'], c['pad'])
    assert (np.abs(exact) >= 2 ** 31).sum() > 1000 and (exact != ref.v[pl][0]).sum() > 1000
    np.testing.assert_array_equal(ref.v[pl][0], ref_ops.wrap32(exact))


# ---- adaptive pooling
def test_adaptive_avgpool_on_the_psp_bins():
    for bins, k, sh in ((1, 12, 7), (2, 6, 5), (3, 4, 4), (6, 2, 2)):
        net, x, t = _one(H=12, W=12)
        p = net.adaptive_avgpool(t, bins, label='pool')
        assert net.tensor_info(p) == (40, bins, bins, 13 + sh)
        net.output(p, as_float=False)
        net.finalize(2)
        assert ('avgpool_sum:pool' if bins == 1 else f'sumpool{k}x{k}s{k}:pool') in net.describe()
    net, x, t = _one(H=12, W=12)
    for bins in (5, 7, 0, 12):                                     # uneven bins; the identity
        with pytest.raises(ValueError, match='adaptive_avgpool'):
            net.adaptive_avgpool(t, bins)
    net, x, t = _one(H=12, W=24)
    with pytest.raises(ValueError, match='square'):
        net.adaptive_avgpool(t, 2)


# ---- ONNX
def _plan_but_labels(net):
    """Per launch (plan token, kernel symbol, bytes, the forms and epilogue flags describe() prints): the plan, but for the tensor labels."""
    text = [l.split()[2:] for l in net.describe().splitlines() if l.strip() and l.split()[0].isdigit()]
    return [(net.launch_info(i, 3)[0].split(':')[0], net.launch_kernel(i), net.launch_info(i, 3)[1], text[i]) for i in range(net.num_launches)]


@pytest.mark.parametrize('name', ['g_2s2_7x9', 'g_3s1p1_5x7', 'g_4s2p2_8x10', 'g_15s15_15x30', 'g_12_12x12_global', 'r_two', 'r_join', 'r_concat_i8', 'r_psp'])
def test_onnx_round_trip(name):
    c = ac.CASES[name]
    ig, g, out = ac.int_graph(name)
    assert sum(o.kind == 'avgpool2d' for o in ig.ops) == 1
    data = onnx_export.export_graph(ig)
    nodes = onnx_io.load_graph(data).nodes
    (ap,) = [n for n in nodes if n.op == 'AveragePool']
    assert (ap.attrs['count_include_pad'], ap.attrs['ceil_mode'], list(ap.attrs['kernel_shape']), list(ap.attrs['strides']), list(ap.attrs['pads'])) == \
        (1, 0, [c['k']] * 2, [c['s']] * 2, [c['pad']] * 4)
    (mul,) = [n for n in nodes if n.op == 'Mul' and n.inputs[0] == ap.outputs[0]]
    back = onnx_import.import_graph(data)
    same_ops(ig, back)
    assert back.solve_fraclens(ac.X_FL) == ig.solve_fraclens(ac.X_FL)
    x = ac.make_input(name)
    np.testing.assert_array_equal(graph_forward(back, x, ac.X_FL), g.v[out][0])      # the walker against RefGraph's values
    net = back.build_net(3, input_fraclen=ac.X_FL, options=c['opts'])
    direct, _, _ = ac.plan(name, x)
    assert [(t, k) for _, t, k in ac.pool_lines(net)] == ([] if c['forms'] is None else [(ac.token(c), ac.symbol(c, 1))])
    assert _plan_but_labels(net) == _plan_but_labels(direct.net)


def _model(name, edit):
    ig, _, _ = ac.int_graph(name)
    g = onnx_io.load_graph(onnx_export.export_graph(ig))
    ap = next(n for n in g.nodes if n.op == 'AveragePool')
    edit(g, ap)
    return g


def _const(g, name, value):
    g.nodes.insert(0, onnx_io.Node('Constant', [], [name], name=name, attrs={'value': value}))
    return name


def _drop_mul(g, ap):
    mul = next(n for n in g.nodes if n.op == 'Mul' and n.inputs[0] == ap.outputs[0])
    for n in g.nodes:
        n.inputs = [ap.outputs[0] if s == mul.outputs[0] else s for s in n.inputs]
    g.nodes.remove(mul)


def _wrong_mul(g, ap):
    mul = next(n for n in g.nodes if n.op == 'Mul' and n.inputs[0] == ap.outputs[0])
    mul.inputs[1] = _const(g, 'eight', np.array(8.0, np.float32))


def _set(key, value):
    return lambda g, ap: ap.attrs.__setitem__(key, value)


@pytest.mark.parametrize('name, edit, match', [
    ('g_3s1p1_5x7', _drop_mul, 'without the Mul by 9'),
    ('g_3s1p1_5x7', _wrong_mul, 'Mul by 3\\^2 = 9'),
    ('g_3s1p1_5x7', _set('ceil_mode', 1), 'ceil_mode=1'),
    ('g_3s1p1_5x7', _set('count_include_pad', 0), 'count_include_pad=0 with pad 1'),
    ('g_3s1p1_5x7', _set('kernel_shape', [3, 2]), 'non-square kernel \\[3, 2\\]'),
    ('g_3s1p1_5x7', _set('strides', [1, 2]), 'non-square strides \\[1, 2\\]'),
    ('g_3s1p1_5x7', _set('pads', [1, 1, 0, 0]), 'asymmetric pads \\[1, 1, 0, 0\\]'),
    ('g_3s1p1_5x7', _set('auto_pad', b'SAME_UPPER'), 'auto_pad'),
])
def test_onnx_import_refusals(name, edit, match):
    with pytest.raises(onnx_import.OnnxImportError, match=match):
        onnx_import.import_graph(_model(name, edit))


def test_onnx_count_include_pad_0_without_padding_is_accepted():
    ig, _, _ = ac.int_graph('g_2s2_7x9')
    same_ops(ig, onnx_import.import_graph(_model('g_2s2_7x9', _set('count_include_pad', 0))))


def test_onnx_reduce_sum_pair_stays_the_global_pool():
    spec = topology.get('resnet18')
    ig = onnx_export.graph_from_params(spec, synth.make_params(spec, seed=1), hw=64)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert [o.kind for o in back.ops if 'pool' in o.kind] == ['maxpool', 'avgpool']


# ---- the torch op
def test_torch_op_meta_shape():
    import torch
    import f8net_amd.torch_ops  # noqa: F401
    x = torch.empty((3, 40, 7, 9), dtype=torch.int32, device='meta')
    for k, s, pad, hw in ((2, 2, 0, (3, 4)), (3, 1, 1, (7, 9)), (4, 2, 2, (4, 5)), (7, 7, 0, (1, 1)), (2, 3, 1, (3, 4))):
        y = torch.ops.f8net.avgpool2d_sum(x, k, s, pad)
        assert y.device.type == 'meta' and y.dtype == torch.int32 and tuple(y.shape) == (3, 40) + hw


def test_module_defaults():
    from f8net_amd import ops
    m = ops.F8AvgPool2d(3)
    assert (m.kernel_size, m.stride, m.padding, m.shiftnum) == (3, 3, 0, 3)
    m = ops.F8AvgPool2d(2, stride=1, padding=1)
    assert (m.kernel_size, m.stride, m.padding, m.shiftnum) == (2, 1, 1, 2)


# ---- the option key
def test_option_key():
    net, x, t = _one()
    assert net.get_option('sumpool_wide') == 1
    for v in (0, 2):
        net.set_option('sumpool_wide', v)
        assert net.get_option('sumpool_wide') == v
    for bad in (3, -1):
        with pytest.raises(F8Error) as e:
            net.set_option('sumpool_wide', bad)
        assert e.value.status == INVALID
    net.output(net.avgpool(t, 2), as_float=False)
    net.finalize(1)
    with pytest.raises(F8Error) as e:
        net.set_option('sumpool_wide', 1)                          # a planning key: not after finalize
    assert e.value.status == STATE


def test_option_default_comes_from_the_environment(monkeypatch):
    monkeypatch.setenv('F8_SUMPOOL_WIDE', '0')
    assert F8Net().get_option('sumpool_wide') == 0
    monkeypatch.delenv('F8_SUMPOOL_WIDE')
    assert F8Net().get_option('sumpool_wide') == 1


def test_plan_digests_of_the_shipped_nets_are_the_parents():
    """tools/plan_digest.py's DEFAULT option column (tests/golden/plan_digest_default.txt, recorded before f8_net_concat existed) at batch 128 for the
    nets whose tail is the global pool in its three plans (a launch of its own, fused behind a conv, the end of a chain): f8_net_avgpool_window
    changes no matcher, and its option key moves no shipped plan.  (tests/test_concat_plan.py plans the whole column.)"""
    plan_digest = plan_digest_tool()
    assert plan_digest.LATER['sumpool_wide'] == (0, 2)
    jobs = [(a, 224, 128, False, 'default') for a in plan_digest.ARCHS if a in ('resnet18', 'resnet50', 'mobilenet_v1', 'mobilenet_v2')]
    assert len(jobs) == 4
    shipped_digest_membership(jobs)


# ---- host code under the sanitizers
def test_host_code_under_asan_and_ubsan():
    """examples/avgpool_host.c records a DenseNet transition and a PSP pyramid (bins 1 / 2 / 3 / 6 -> 1x1 -> nearest upsample -> concat) through the C
    ABI, walks every refusal, finalizes, describes and destroys.  f8_net.cpp's host side is compiled with AddressSanitizer and
    UndefinedBehaviorSanitizer and linked with the library's other objects into that stand-alone program."""
    out = sanitized_host_program('avgpool_host.c')
    assert out.rstrip().endswith('ok')
    assert out.count('sumpool2x2s2:transition.pool') == 1 and out.count('avgpool_sum:psp.pool1') == 1
    assert all(out.count(f'sumpool{k}x{k}s{k}:psp.pool{b}') == 1 for k, b in ((6, 2), (4, 3), (2, 6)))
    assert out.count('upsample_nearest_i8:psp.up') == 4 and out.count('concat_i8:psp.cat') == 1
