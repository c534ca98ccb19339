"""Channel slice and channel shuffle on the CPU: acceptance and refusals of f8_net_slice / f8_net_channel_shuffle, the reference of
tests/chanmap_cases.py pinned to torch, the plan tokens and kernel instances every case plans on both legs of option chanmap_i8, with every fusing
pass on and with fuse_shuffle = 0 — written by hand there —, launch_info / launch_valu by hand, where the ops cut the fused launches of ResNet-50 and
MobileNet-V2 (exactly where an output tap does), ONNX Split / Slice / Reshape-Transpose-Reshape in both directions and the import refusals, the
shipped nets' default plans against the recorded digests, and the host code under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone
program.  tests/test_gpu_chanmap.py runs every case on the device."""
import numpy as np
import pytest
import torch

import chanmap_cases as cm
import ref_ops
from f8net_amd import onnx_export, onnx_import, onnx_io, synth, topology
from f8net_amd._lib import F8Error
from f8net_amd.net import F8Net, build_net, record_net
from graph_cases import all_shipped_jobs, plan_digest_tool, same_ops, sanitized_host_program, shipped_digest_membership
from refgraph import graph_forward

INVALID, UNSUPPORTED, STATE = -1, -2, -5


def _w(cout, cin, k=1):
    return np.ones((cout, cin, k, k), np.int32)


def _src(C=24, fl=8, w_fl=5):
    """input (8 channels, 8 x 8) -> a 1x1 conv to C channels; returns (net, input id, conv id)."""
    net = F8Net()
    x = net.input(8, 8, 8, fl)
    return net, x, net.conv(x, _w(C, 8), None, stride=1, pad=0, groups=1, weight_fl=w_fl, input_fl=fl, input_signed=False, quant_input=False)


# ---- the C ABI
def test_acceptance_shape_and_fraclen():
    net, x, a = _src(C=24)
    s = net.slice(a, 5, 17, label='part')
    h = net.channel_shuffle(a, 3, label='mixed')
    parts = net.split(a, [4, 12, 8])
    assert net.tensor_info(s) == (12, 8, 8, 13) and net.tensor_info(h) == (24, 8, 8, 13)
    assert [net.tensor_info(p)[0] for p in parts] == [4, 12, 8]
    assert net.tensor_info(net.slice(x, 7, 8)) == (1, 8, 8, 8)
    r = net.conv(h, _w(32, 24), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False)
    net.output(r, as_float=False)
    assert net.output(s, as_float=False) == 1
    net.finalize(2)
    assert net.output_info(1) == (12, 8, 8, 13, False)
    assert 'slice_i32:part' in net.describe() and 'shuffle3_i8:mixed' in net.describe()


@pytest.mark.parametrize('what, status', [('bad_id', INVALID), ('negative_id', INVALID), ('first_negative', INVALID), ('no_channels', INVALID),
                                          ('negative_channels', INVALID), ('past_the_end', INVALID), ('first_past_the_end', INVALID), ('whole', INVALID),
                                          ('finalized', STATE)])
def test_slice_refusals(what, status):
    net, x, a = _src(C=24)
    args = {'bad_id': (99, 0, 4), 'negative_id': (-1, 0, 4), 'first_negative': (a, -1, 4), 'no_channels': (a, 3, 3), 'negative_channels': (a, 8, 4),
            'past_the_end': (a, 20, 25), 'first_past_the_end': (a, 30, 31), 'whole': (a, 0, 24), 'finalized': (a, 0, 4)}[what]
    if what == 'finalized':
        net.output(a, as_float=False)
        net.finalize(1)
    with pytest.raises(F8Error) as e:
        net.slice(*args)
    assert e.value.status == status, str(e.value)


@pytest.mark.parametrize('what, status', [('bad_id', INVALID), ('negative_id', INVALID), ('one_group', INVALID), ('no_groups', INVALID), ('negative_groups', INVALID),
                                          ('not_dividing', INVALID), ('identity', INVALID), ('twelve', UNSUPPORTED), ('finalized', STATE)])
def test_shuffle_refusals(what, status):
    net, x, a = _src(C=24)
    args = {'bad_id': (99, 2), 'negative_id': (-1, 2), 'one_group': (a, 1), 'no_groups': (a, 0), 'negative_groups': (a, -2), 'not_dividing': (a, 5),
            'identity': (a, 24), 'twelve': (a, 12), 'finalized': (a, 2)}[what]
    if what == 'finalized':
        net.output(a, as_float=False)
        net.finalize(1)
    with pytest.raises(F8Error) as e:
        net.channel_shuffle(*args)
    assert e.value.status == status, str(e.value)


def test_eight_groups_are_accepted_and_the_identity_of_eight_channels_is_not():
    net, x, a = _src(C=24)
    assert net.channel_shuffle(a, 8) >= 0
    with pytest.raises(F8Error) as e:
        net.channel_shuffle(x, 8)                                  # the input has 8 channels
    assert e.value.status == INVALID


def test_options():
    net = F8Net()
    for key in ('chanmap_i8', 'fuse_shuffle'):
        assert net.get_option(key) == 1
        net.set_option(key, 0)
        assert net.get_option(key) == 0
        for bad in (-1, 2):
            with pytest.raises(F8Error):
                net.set_option(key, bad)
    later = plan_digest_tool().LATER
    assert later['chanmap_i8'] == (0, 1) and later['fuse_shuffle'] == (0, 1)


# ---- the reference
@pytest.mark.parametrize('groups, C', cm.SHUFFLES)
def test_shuffle_reference_is_torchs(groups, C):
    x = np.random.default_rng(C * 10 + groups).integers(-2 ** 31, 2 ** 31, (2, C, 3, 2), dtype=np.int64).astype(np.int32)
    y = ref_ops.channel_shuffle(x, groups)
    np.testing.assert_array_equal(y, torch.nn.functional.channel_shuffle(torch.from_numpy(x), groups).numpy())
    assert sorted(ref_ops.shuffle_index(C, groups).tolist()) == list(range(C))
    assert not np.array_equal(y, x)
    if groups != C // groups:                                      # (4, 16) is its own inverse; every other entry tells the transpose done the wrong way round
        assert not np.array_equal(y, ref_ops.channel_shuffle(x, C // groups))


@pytest.mark.parametrize('first, channels, C', cm.SLICES)
def test_slice_reference_is_torchs(first, channels, C):
    x = np.random.default_rng(C * 100 + first).integers(-2 ** 31, 2 ** 31, (2, C, 3, 2), dtype=np.int64).astype(np.int32)
    sizes = [s for s in (first, channels, C - first - channels) if s]
    parts = torch.split(torch.from_numpy(x), sizes, dim=1)
    np.testing.assert_array_equal(ref_ops.channel_slice(x, first, channels), parts[1 if first else 0].numpy())
    np.testing.assert_array_equal(ref_ops.channel_slice(x, first, channels), x[:, first:first + channels])


@pytest.mark.parametrize('name', sorted(cm.CASES))
def test_the_reference_of_every_case_carries_values(name):
    """Outputs and op results carry values, no two channels of an op result are equal, and every shuffle result differs from its source and from the
    shuffle done the wrong way round (by C / groups) — except the one self-inverse entry of the table."""
    ref, outs, ops = cm.reference(name)
    c = cm.CASES[name]
    assert all(np.unique(ref.v[o][0]).size > (20 if c.get('vec') else 100) for o in outs)
    for t in ops:
        v = ref.v[t][0]
        flat = v.transpose(1, 0, 2, 3).reshape(v.shape[1], -1)
        live = [r.tobytes() for r in flat if r.any()]              # (a ReLU leaves a few channels of the wide producers at 0 throughout)
        assert len(set(live)) == len(live), 'two channels carry the same values'
        assert len(live) >= v.shape[1] - v.shape[1] // 16, f'{v.shape[1] - len(live)} of {v.shape[1]} channels are dead'
    if c['build'] in (cm._shuffle, cm._shuffle_join, cm._shuffle_input, cm._cat_shuffle):
        (t,) = ops
        y, g = ref.v[t][0], c['groups']
        src = ref_ops.channel_shuffle(y, y.shape[1] // g)               # the inverse permutation gives the source back
        assert not np.array_equal(y, src)
        if g != y.shape[1] // g:
            assert not np.array_equal(y, ref_ops.channel_shuffle(src, y.shape[1] // g))


# ---- tokens and kernels
@pytest.mark.parametrize('name', sorted(cm.CASES))
def test_tokens_and_kernels_of_every_case(name):
    c = cm.CASES[name]
    x = cm.make_input(name)
    for opts in ({}, cm.FUSE_ALL, dict(chanmap_i8=0), dict(fuse_shuffle=0), dict(chanmap_i8=0, fuse_shuffle=0)):
        g, _, _ = cm.plan(name, x, max_batch=c['N'] + 1, **opts)
        assert [(t, k) for _, t, k in cm.lines(g.net)] == cm.expected(name, **opts), (opts, g.net.describe())


def test_the_third_int8_format_is_a_requant_step():
    g, _, _ = cm.plan('sh_threeforms', cm.make_input('sh_threeforms'))
    names = [g.net.launch_info(i, 1)[0] for i in range(g.net.num_launches)]
    assert [n for n in names if n.startswith(('shuffle', 'requant:'))] == ['shuffle2_i32:op', 'requant:op']


@pytest.mark.parametrize('name', ['sh2_64', 'sh_twice', 'sl_58_58', 'sl_two', 'f_58', 'f_16x4', 'f_twoforms'])
def test_an_i8_plan_holds_no_int32_form_up_to_its_last_op(name):
    g, _, _ = cm.plan(name, cm.make_input(name))
    last = cm.lines(g.net)[-1][0]
    rows = g.net.describe().splitlines()[:last + 1]
    assert all('i32=0' in r and 'requant:' not in r for r in rows), g.net.describe()


def test_a_fused_concat_emits_no_launch_and_fuse_shuffle_0_brings_it_back():
    x = cm.make_input('f_32')
    fused, _, _ = cm.plan('f_32', x)
    two, _, _ = cm.plan('f_32', x, fuse_shuffle=0)
    assert two.net.num_launches == fused.net.num_launches + 1
    assert 'concat_' not in fused.net.describe() and 'concat_i8:cat' in two.net.describe()


# (bytes / essential vector operations by hand: i8 — every real byte read once and written once, per form; i32 — the source's real int32 values read,
#  the padded output forms written, 3 operations per int8 value produced)
@pytest.mark.parametrize('name, per_image, valu', [
    ('sh2_116', 2 * 49 * 116, 0),
    ('sh_twoforms', 2 * 49 * 64 * 2, 0),
    ('f_58', 2 * 49 * 116, 0),
    ('sl_29_29', 2 * 49 * 29, 0),
    ('sl_to_out', 49 * (30 * 4 + 32 * 4), 0),                                   # int32 in, the int32 form (32 padded channels) out
    ('sh_threeforms', 49 * (64 * 4 + 64 * (4 + 2)), 49 * 64 * 3 * 2),           # int32 in; the int32 form and two int8 forms out
])
def test_launch_info_and_valu_by_hand(name, per_image, valu):
    g, _, _ = cm.plan(name, cm.make_input(name))
    (i, _, _), = cm.lines(g.net)
    for N in (1, 3):
        _, nbytes, ops = g.net.launch_info(i, N)
        assert (nbytes, ops) == (N * per_image, 0)
        assert g.net.launch_valu(i, N) == N * valu


# ---- a slice / a shuffle cuts fused launches where a tap does
def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _backbone(net):
    return [n for n in _names(net) if not n.startswith(('tap:', 'slice_', 'shuffle'))]


# (ResNet-50: a block output inside the stage chain; MobileNet-V2: a block output inside the 14 x 14 run that fuse_irchain makes one launch of)
@pytest.mark.parametrize('op', ['slice', 'shuffle'])
@pytest.mark.parametrize('arch, name', [('resnet50', 'stage_1_layer_1'), ('mobilenet_v2', 'stage_3_layer_1')])
def test_the_op_cuts_the_chain_where_a_tap_does(arch, name, op):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=7)
    plain = build_net(spec, params, 8, options=cm.FUSE_ALL)
    tapped = build_net(spec, params, 8, options=cm.FUSE_ALL, taps=(name,))
    net = record_net(spec, params, options=cm.FUSE_ALL)
    t = net.slice(net.tap_ids[name], 3, 19, label='op') if op == 'slice' else net.channel_shuffle(net.tap_ids[name], 2, label='op')
    assert net.output(t, as_float=False) == 1
    for k, v in cm.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(8)
    assert _backbone(net) == _backbone(tapped)
    assert net.num_launches == tapped.num_launches + 1             # the tap there; here the op and the tap on it
    assert _backbone(plain) != _backbone(tapped), 'the tensor does not cut any fused launch: the comparison shows nothing'
    assert [n for n in _names(net) if n.startswith(('slice_', 'shuffle'))] == ['slice_i32:op' if op == 'slice' else 'shuffle2_i32:op']


# ---- ONNX
def test_onnx_round_trip_of_the_stage():
    ig, g, out = cm.stage_int_graph()
    assert [o.kind for o in ig.ops].count('slice') == 4 and [o.kind for o in ig.ops].count('shuffle') == 3
    data = onnx_export.export_graph(ig)
    nodes = onnx_io.load_graph(data).nodes
    assert sum(n.op == 'Slice' for n in nodes) == 4 and sum(n.op == 'Transpose' for n in nodes) == 3
    back = onnx_import.import_graph(data)
    same_ops(ig, back)
    assert back.solve_fraclens(cm.X_FL) == ig.solve_fraclens(cm.X_FL)
    x = cm.stage_input()
    np.testing.assert_array_equal(graph_forward(back, x, cm.X_FL), g.v[out][0])      # the walker against RefGraph's values
    net = back.build_net(2, input_fraclen=cm.X_FL)
    assert [t for _, t, _ in cm.lines(net)] == ['concat+shuffle2_i8:', 'slice_i8:', 'slice_i8:'] * 2 + ['concat+shuffle2_i8:']


def _const_of(g, name):
    return next(n for n in g.nodes if n.op == 'Constant' and n.outputs[0] == name)


def _reshapes_to(g, rank):
    """The Reshape nodes whose shape operand is a constant of this length (the classifier's is computed: Shape / Gather / Concat)."""
    consts = {n.outputs[0]: n for n in g.nodes if n.op == 'Constant'}
    return [n for n in g.nodes if n.op == 'Reshape' and n.inputs[1] in consts and len(consts[n.inputs[1]].attrs['value']) == rank]


def _set_const(g, name, values):
    _const_of(g, name).attrs['value'] = np.array(values, np.int64)


def _stage_model(edit=None, torch_style=True):
    """The stage's file, rewritten by hand the way torch.onnx writes a ShuffleNet: each pair of Slice nodes of one tensor becomes one
    Split(axis=1, split=[58, 58]) with two outputs, and the shuffle's first Reshape names the batch as 0."""
    ig, _, _ = cm.stage_int_graph()
    g = onnx_io.load_graph(onnx_export.export_graph(ig))
    if torch_style:
        by_src = {}
        for n in [n for n in g.nodes if n.op == 'Slice']:
            by_src.setdefault(n.inputs[0], []).append(n)
        for src, pair in by_src.items():
            assert len(pair) == 2
            at = g.nodes.index(pair[0])
            g.nodes[at] = onnx_io.Node('Split', [src], [pair[0].outputs[0], pair[1].outputs[0]], name=f'/Split_{at}', attrs={'axis': 1, 'split': [58, 58]})
            g.nodes.remove(pair[1])
        for n in _reshapes_to(g, 5):
            _set_const(g, n.inputs[1], [0] + list(_const_of(g, n.inputs[1]).attrs['value'][1:]))
    if edit:
        edit(g)
    return ig, g


def test_onnx_split_and_the_reshape_transpose_reshape_triple_import_as_slices_and_shuffles():
    ig, g = _stage_model()
    assert sum(n.op == 'Split' for n in g.nodes) == 2 and not any(n.op == 'Slice' for n in g.nodes)
    same_ops(ig, onnx_import.import_graph(onnx_io.model_proto(g)))


def test_onnx_split_without_sizes_is_an_equal_split():
    def edit(g):
        for n in g.nodes:
            if n.op == 'Split':
                del n.attrs['split']
    ig, g = _stage_model(edit)
    same_ops(ig, onnx_import.import_graph(onnx_io.model_proto(g)))


def test_the_classifiers_reshape_stays_plumbing():
    ig, g = _stage_model()
    back = onnx_import.import_graph(onnx_io.model_proto(g))
    assert sum(n.op == 'Reshape' for n in g.nodes) == 7 and [o.kind for o in back.ops].count('shuffle') == 3      # two per shuffle, one in front of the Gemm


def _first(g, op):
    return next(n for n in g.nodes if n.op == op)


@pytest.mark.parametrize('what, match', [('split_axis', 'axis 2'), ('split_sizes', 'do not cover'), ('slice_axis', 'axes'), ('slice_step', 'steps'),
                                         ('perm', 'perm'), ('factor', 'groups x'), ('map', 'groups x'), ('back', 'behind the shuffle')])
def test_onnx_import_refusals(what, match):
    def edit(g):
        if what == 'split_axis':
            _first(g, 'Split').attrs['axis'] = 2
        elif what == 'split_sizes':
            _first(g, 'Split').attrs['split'] = [58, 57]
        elif what == 'slice_axis':
            _set_const(g, _first(g, 'Slice').inputs[3], [2])
        elif what == 'slice_step':
            _set_const(g, _first(g, 'Slice').inputs[4], [2])
        elif what == 'perm':
            _first(g, 'Transpose').attrs['perm'] = [0, 2, 1, 4, 3]
        elif what in ('factor', 'map'):
            r = _reshapes_to(g, 5)[0]
            _set_const(g, r.inputs[1], [-1, 3, 39, 7, 7] if what == 'factor' else [-1, 2, 58, 49, 1])
        elif what == 'back':
            r = _reshapes_to(g, 4)[0]
            _set_const(g, r.inputs[1], [-1, 58, 14, 7])
    _, g = _stage_model(edit, torch_style=what.startswith('split'))
    with pytest.raises(onnx_import.OnnxImportError, match=match):
        onnx_import.import_graph(onnx_io.model_proto(g))


def test_a_shipped_net_exports_and_imports_as_before():
    spec = topology.get('resnet18')
    ig = onnx_export.graph_from_params(spec, synth.make_params(spec, seed=5), 64)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert all(o.kind not in ('slice', 'shuffle') for o in back.ops)
    same_ops(ig, back)


# ---- the shipped nets plan as before
def test_plan_digests_of_the_shipped_nets_are_the_recorded_ones():
    """tools/plan_digest.py's DEFAULT option column: the lines recorded before these entry points existed (tests/golden/plan_digest_default.txt), of
    which a subset is planned here.  The other option sets of the tool's matrix are not checked by the suite."""
    shipped_digest_membership(all_shipped_jobs())


# ---- host code under the sanitizers
def test_host_code_under_asan_and_ubsan():
    """examples/shuffle_host.c records `unit`, `unequal` and `output` through the C ABI, finalizes, describes and destroys them.  f8_net.cpp's host side
    is compiled with AddressSanitizer and UndefinedBehaviorSanitizer and linked with the library's other objects into that stand-alone program."""
    out = sanitized_host_program('shuffle_host.c')
    assert out.rstrip().endswith('ok')
    assert out.count('slice_i8:') == 2 and out.count('concat+shuffle2_i8:') == 1 and out.count('concat_i8:') == 1
    assert out.count('shuffle2_i8:') == 2 and out.count('shuffle3_i32:') == 1
