"""Channel concatenation on the CPU: f8_net_concat's acceptance and refusals, the mode (concat_i8: / concat_i32:) and kernel instance every case of
tests/concat_cases.py plans — written by hand there —, the forms of an i8-mode plan, launch_info, where a concat cuts the fused launches of
ResNet-50 and MobileNet-V2 (exactly where an output tap does), the ONNX Concat in both directions, the shipped nets' plans against the digests of
the library before this entry point existed, and the host code under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program.
tests/test_gpu_concat.py runs every case on the device."""
import numpy as np
import pytest

import concat_cases as cc
from f8net_amd import onnx_export, onnx_import, onnx_io, synth, topology
from f8net_amd._lib import F8Error
from f8net_amd.net import F8Net, build_net, record_net
from graph_cases import all_shipped_jobs, same_ops, sanitized_host_program, shipped_digest_membership
from oracle import oracle
from ref_ops import stuffed
from refgraph import RefGraph, graph_forward

INVALID, UNSUPPORTED, STATE = -1, -2, -5


def _w(cout, cin, k=1):
    return np.ones((cout, cin, k, k), np.int32)


def _two(C=(32, 32), fl=8, w_fl=(5, 5), stride=(1, 1)):
    """input (8 channels, 8 x 8) -> two 1x1 convs; returns (net, input id, [conv ids])."""
    net = F8Net()
    x = net.input(8, 8, 8, fl)
    ts = [net.conv(x, _w(c, 8), None, stride=s, pad=0, groups=1, weight_fl=wf, input_fl=fl, input_signed=False, quant_input=False)
          for c, wf, s in zip(C, w_fl, stride)]
    return net, x, ts


# ---- the C ABI
def test_acceptance_shape_and_fraclen():
    net, x, (a, b) = _two(C=(24, 40), w_fl=(5, 2))
    t = net.concat([a, b, x], label='cat')                        # fraclens 13, 10, 8
    r = net.conv(t, _w(32, 72), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False)
    net.output(r, as_float=False)
    assert net.output(t, as_float=False) == 1
    net.finalize(2)
    assert net.output_info(1) == (72, 8, 8, 13, False)
    assert 'concat_i32:cat' in net.describe()


@pytest.mark.parametrize('what, status', [('one', INVALID), ('none', INVALID), ('bad_id', INVALID), ('negative_id', INVALID), ('size', INVALID), ('gap', INVALID),
                                          ('nine', UNSUPPORTED), ('twice', UNSUPPORTED), ('finalized', STATE)])
def test_refusals(what, status):
    net, x, (a, b) = _two(stride=(1, 2) if what == 'size' else (1, 1))
    srcs = {'one': [a], 'none': [], 'bad_id': [a, 99], 'negative_id': [-1, a], 'size': [a, b], 'nine': [a, b] + [x] * 7, 'twice': [a, b, a],
            'finalized': [a, b]}.get(what)
    if what == 'gap':                                              # fraclens 0 and 39
        net = F8Net()
        x = net.input(8, 8, 8, 0)
        a = net.conv(x, _w(8, 8), None, stride=1, pad=0, groups=1, weight_fl=31, input_fl=0, input_signed=False, quant_input=False)
        b = net.conv(a, _w(8, 8), None, stride=1, pad=0, groups=1, weight_fl=31, input_fl=8, input_signed=False)
        assert net.concat([x, a]) >= 0                             # a gap of 31 is the residual join's limit too
        srcs = [x, b]
    if what == 'finalized':
        net.output(a, as_float=False)
        net.finalize(1)
    with pytest.raises(F8Error) as e:
        net.concat(srcs)
    assert e.value.status == status, str(e.value)


def test_eight_operands_are_accepted():
    net = F8Net()
    x = net.input(8, 4, 4, 8)
    ts = [net.conv(x, _w(16, 8), None, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False) for _ in range(8)]
    assert net.concat(ts) >= 0


# ---- modes and kernels
@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_mode_and_kernel_of_every_case(name):
    c = cc.CASES[name]
    x = cc.make_input(name)
    for opts in ({}, cc.FUSE_ALL):
        g, _, cats = cc.plan(name, x, max_batch=c['N'] + 1, **opts)
        lines = cc.concat_lines(g.net)
        assert len(lines) == len(cats)
        assert [(t, k) for _, t, k in lines] == [(c['mode'], cc.symbol(c['mode'], c['aligned']))] * len(cats), g.net.describe()
    g, _, cats = cc.plan(name, x, concat_i8=0)
    assert [(t, k) for _, t, k in cc.concat_lines(g.net)] == [(cc.I32, 'f8::concat_i32_kernel')] * len(cats), g.net.describe()
    _live(name)


def _live(name):
    """The case's reference carries values: outputs and concats, and in every 8-channel stretch of a concat most channels (a ReLU leaves some at 0)."""
    ref, outs, cats = cc.reference(name)
    assert all(np.unique(ref.v[o][0]).size > 100 for o in outs + cats)
    for t in cats:
        v = ref.v[t][0]
        live = np.array([np.unique(v[:, ch]).size > 4 for ch in range(v.shape[1])])
        assert all(live[i:i + 8].mean() >= 0.5 for i in range(0, live.size, 8)), live


def test_raw_case_wraps_and_clamps_in_the_alignment_and_plans_the_int32_mode():
    g, _, _ = cc.plan('raw', cc.make_input('raw'))
    assert [t for _, t, _ in cc.concat_lines(g.net)] == [cc.I32]
    ref, _, (cat,) = cc.reference('raw')
    x = cc.make_input('raw', cc.CASES['raw']['N'] + 1)
    got = ref.v[cat][0][:, :8]
    exact = x.astype(np.int64) << 7
    assert (np.abs(exact) >= 2 ** 31).sum() > 100 and (got == -(2 ** 31 - 1)).any()      # wrapped values, and -2^31 moved by the clamp
    wrapped = ((exact + 2 ** 31) % 2 ** 32 - 2 ** 31)
    np.testing.assert_array_equal(got, np.maximum(wrapped, -(2 ** 31 - 1)))


@pytest.mark.parametrize('name', [n for n in cc.I8_CASES if n not in ('vec', 'gapneg', 'gapneg0')])
def test_an_i8_plan_holds_no_int32_form_up_to_its_last_concat(name):
    """Neither the sources nor the concat exist in int32, and no stand-alone requant stands in for a missing form.  (`vec` pools the int32 input; the
    `gapneg` producers read the input at lower fraclens, which the input launch serves from its int32 form.)"""
    g, _, _ = cc.plan(name, cc.make_input(name))
    last = cc.concat_lines(g.net)[-1][0]
    lines = g.net.describe().splitlines()[:last + 1]
    assert all('i32=0' in l and 'requant:' not in l for l in lines), g.net.describe()


# (forms written by the launch, by hand: int8 forms per concat in launch order; int32 mode: (int32 written, int8 forms written))
I8_FORMS = {'twoforms': [2], 'nested': [2, 2, 2, 1], 'shared': [1, 1]}
I32_FORMS = {'threeforms': (1, 2), 'to_add': (1, 0), 'to_out': (1, 0), 'to_out_f32': (1, 0), 'to_pool': (1, 1), 'raw': (0, 1)}


@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_launch_info_bytes(name):
    c = cc.CASES[name]
    ref, _, cats = cc.reference(name)
    g, _, _ = cc.plan(name, cc.make_input(name))
    for k, ((i, tok, _), t) in enumerate(zip(cc.concat_lines(g.net), cats)):
        _, C, H, W = ref.v[t][0].shape
        for N in (1, 5):
            _, nbytes, ops = g.net.launch_info(i, N)
            assert ops == 0
            if tok == cc.I8:                                       # every real byte read once and written once, per form
                assert nbytes == 2 * N * H * W * C * I8_FORMS.get(name, [1])[k]
                assert g.net.launch_valu(i, N) == 0
            else:
                o32, o8 = I32_FORMS[name]
                Cs = -(-C // 32) * 32
                assert nbytes == N * H * W * (C * 4 + Cs * (4 * o32 + o8))
                assert g.net.launch_valu(i, N) == N * H * W * C * (2 + 3 * o8)
    if name == 'aligned2':
        g, _, _ = cc.plan(name, cc.make_input(name), concat_i8=0)
        (i, _, _), = cc.concat_lines(g.net)
        assert g.net.launch_info(i, 2)[1] == 2 * 64 * (96 * 4 + 96)


# ---- a concat cuts fused launches where a tap does
def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _backbone(net):
    return [n for n in _names(net) if not n.startswith(('tap:', 'concat_'))]


# (MobileNet-V2: a block output and its input inside the 14 x 14 run that fuse_irchain makes one launch of)
@pytest.mark.parametrize('arch, pair', [('resnet50', ('stage_1_layer_1', 'stage_1_layer_3')), ('mobilenet_v2', ('stage_3_layer_2', 'stage_3_layer_1'))])
def test_a_concat_cuts_the_chain_where_a_tap_does(arch, pair):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=7)
    plain = build_net(spec, params, 8, options=cc.FUSE_ALL)
    tapped = build_net(spec, params, 8, options=cc.FUSE_ALL, taps=pair)
    net = record_net(spec, params, options=cc.FUSE_ALL)
    cat = net.concat([net.tap_ids[pair[0]], net.tap_ids[pair[1]]], label='cat')
    assert net.output(cat, as_float=False) == 1
    for k, v in cc.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(8)
    assert _backbone(net) == _backbone(tapped)
    assert net.num_launches == tapped.num_launches                 # two taps there; here the concat and the tap on it
    assert _backbone(plain) != _backbone(tapped), 'the pair does not cut any fused launch: the comparison shows nothing'
    assert [n for n in _names(net) if n.startswith('concat_')] == ['concat_i32:cat']


# ---- ONNX
@pytest.mark.parametrize('name', ['gap', 'nested', 'inception'])
def test_onnx_round_trip(name):
    ig, g, out = cc.int_graph(name)
    assert sum(o.kind == 'concat' for o in ig.ops) == len(cc.reference(name)[2])
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    same_ops(ig, back)
    assert back.solve_fraclens(cc.X_FL) == ig.solve_fraclens(cc.X_FL)
    if name == 'gap':
        assert [o.shifts for o in back.ops if o.kind == 'concat'] == [[0, 3, 6]]
    x = cc.make_input(name)
    np.testing.assert_array_equal(graph_forward(back, x, cc.X_FL), g.v[out][0])      # the walker against RefGraph's values
    net = back.build_net(2, input_fraclen=cc.X_FL)
    c = cc.CASES[name]
    assert {(t, k) for _, t, k in cc.concat_lines(net)} == {(c['mode'], cc.symbol(c['mode'], c['aligned']))}


def _concat_model(edit):
    ig, _, _ = cc.int_graph('gap')
    g = onnx_io.load_graph(onnx_export.export_graph(ig))
    cat = next(n for n in g.nodes if n.op == 'Concat' and n.attrs.get('axis') == 1)
    edit(g, cat)
    return g


@pytest.mark.parametrize('axis', [0, 2, -1])
def test_onnx_concat_on_another_axis_is_refused(axis):
    with pytest.raises(onnx_import.OnnxImportError, match='axis'):
        onnx_import.import_graph(_concat_model(lambda g, cat: cat.attrs.__setitem__('axis', axis)))


def test_onnx_concat_axis_minus_3_is_the_channel_axis():
    ig, _, _ = cc.int_graph('gap')
    same_ops(ig, onnx_import.import_graph(_concat_model(lambda g, cat: cat.attrs.__setitem__('axis', -3))))


def test_onnx_concat_operand_scaled_by_three_is_refused():
    def edit(g, cat):
        mul = next(n for n in g.nodes if n.op == 'Mul' and n.outputs[0] in cat.inputs)
        g.nodes.insert(0, onnx_io.Node('Constant', [], ['three'], name='three', attrs={'value': np.array(3, np.int32)}))
        mul.inputs[1] = 'three'
    with pytest.raises(onnx_import.OnnxImportError, match='power of two'):
        onnx_import.import_graph(_concat_model(edit))


def test_a_shipped_net_exports_and_imports_as_before():
    """ResNet-18's file still holds the `x.view(x.size(0), -1)` Concat of shape arithmetic, which stays plumbing."""
    spec = topology.get('resnet18')
    ig = onnx_export.graph_from_params(spec, synth.make_params(spec, seed=5), 64)
    data = onnx_export.export_graph(ig)
    assert sum(n.op == 'Concat' for n in onnx_io.load_graph(data).nodes) == 1
    back = onnx_import.import_graph(data)
    assert all(o.kind != 'concat' for o in back.ops)
    same_ops(ig, back)


def test_cropped_stuffed_kernel_is_the_same_conv():
    """The identity RefGraph.conv evaluates ASPP's large dilations with, on the graph of two such convs and their concat as the handle records it."""
    x = synth.rand_uniform_int(3, 'cropx', (2, 4, 5, 6), 0, 255).astype(np.int32)
    g = RefGraph(x, 8)
    ws = [synth.rand_uniform_int(4 + d, 'cropw', (16, 4, 3, 3), -127, 127).astype(np.int32) for d in (7, 9)]
    os_ = [g.conv(0, w, None, pad=d, groups=1, weight_fl=5, input_fl=8, input_signed=False, relu=False, quant_input=True, dilation=d) for w, d in zip(ws, (7, 9))]
    cat = g.concat(os_)
    g.output(cat)
    g.net.finalize(2)
    assert [n.split(':')[0] for n in _names(g.net)][1:4] == ['conv3x3s1d7_t128x32x32', 'conv3x3s1d9_t128x32x32', 'concat_i32']
    want = [oracle.conv2d(x, stuffed(w, d), None, 1, d, 1) for w, d in zip(ws, (7, 9))]
    np.testing.assert_array_equal(g.v[cat][0], np.concatenate(want, axis=1))


# ---- the shipped nets plan as before
def test_plan_digests_of_the_shipped_nets_are_the_parents():
    """tools/plan_digest.py's DEFAULT option column only: the lines recorded from the library before f8_net_concat existed
    (tests/golden/plan_digest_default.txt), of which a subset is planned here.  The other option sets of the tool's matrix are not checked by the suite."""
    shipped_digest_membership(all_shipped_jobs())


# ---- host code under the sanitizers
def test_host_code_under_asan_and_ubsan():
    """examples/concat_host.c records `bytes`, `raw` and `nested` through the C ABI, finalizes, describes and destroys them.  f8_net.cpp's host side is
    compiled with AddressSanitizer and UndefinedBehaviorSanitizer and linked with the library's other objects into that stand-alone program."""
    out = sanitized_host_program('concat_host.c')
    assert out.rstrip().endswith('ok')
    assert out.count('concat_i8:') == 5 and out.count('concat_i32:') == 1
