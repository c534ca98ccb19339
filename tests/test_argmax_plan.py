"""Channel argmax outputs on the CPU: f8_net_output_argmax's acceptance and refusals, what the output queries report, the plan token and kernel
symbol every case of tests/argmax_cases.py plans on every leg — written by hand there —, the fusion conditions (a second reader, a value output on
the upsampled tensor or fuse_argmax = 0 each give two launches), the arena a fused plan saves, where an argmax cuts ResNet-50's stage chain (exactly
where an output tap does), launch_info / launch_valu by hand, the reference pinned to torch, the shipped nets' digests, the C host example under the
sanitizers.  tests/test_gpu_argmax.py runs every case on the device."""
import numpy as np
import pytest

import argmax_cases as ac
import graph_cases
from f8net_amd import synth, topology
from f8net_amd._lib import F8Error, lib
from f8net_amd.net import F8Net, record_net

INVALID, UNSUPPORTED, STATE = -1, -2, -5
U8, I32 = 1, 4


def _net(C=21, H=5, W=3):
    net = F8Net()
    return net, net.input(C, H, W, 8)


# ---- the C ABI
@pytest.mark.parametrize('what, status', [('bad_id', INVALID), ('negative_id', INVALID), ('bytes2', INVALID), ('bytes0', INVALID), ('bytes8', INVALID),
                                          ('one_channel', INVALID), ('twice', INVALID), ('twice_other_type', INVALID), ('u8_256', UNSUPPORTED),
                                          ('ninth', UNSUPPORTED), ('finalized', STATE)])
def test_refusals(what, status):
    C = {'one_channel': 1, 'u8_256': 256}.get(what, 21)
    net, x = _net(C)
    args = {'bad_id': (99, U8), 'negative_id': (-1, U8), 'bytes2': (x, 2), 'bytes0': (x, 0), 'bytes8': (x, 8)}.get(what, (x, U8))
    L = lib()
    if what.startswith('twice'):
        assert L.f8_net_output_argmax(net._h, x, U8) == 0
        args = (x, I32 if what == 'twice_other_type' else U8)
    if what == 'ninth':
        for k in range(8):
            assert net.output_argmax(net.upsample(x, 2, 'nearest'), 'u8') == k
    if what == 'finalized':
        net.output(x, as_float=False)
        net.finalize(1)
    assert L.f8_net_output_argmax(net._h, *args) == status
    assert L.f8_last_error()


def test_null_handle_and_kind_out_of_range():
    L = lib()
    assert L.f8_net_output_argmax(None, 0, U8) == INVALID
    net, x = _net()
    assert L.f8_net_output_kind(net._h, 0) == INVALID and L.f8_net_output_kind(None, 0) == INVALID
    net.output_argmax(x, 'u8')
    assert L.f8_net_output_kind(net._h, 0) == 2 and L.f8_net_output_kind(net._h, 1) == INVALID and L.f8_net_output_kind(net._h, -1) == INVALID


def test_acceptance_limits():
    net, x = _net(255)
    assert net.output_argmax(x, 'u8') == 0                         # 255 classes: indices 0 .. 254, 255 stays the poison value
    net, x = _net(256)
    assert net.output_argmax(x, 'i32') == 0
    net, x = _net(2, 1, 1)
    assert net.output_argmax(x, 'u8') == 0
    with pytest.raises(ValueError, match='i64'):
        net.output_argmax(x, 'i64')


def test_both_marks_on_one_tensor_in_either_order():
    for first in ('value', 'argmax'):
        net, x = _net()
        ks = [net.output(x, as_float=False), net.output_argmax(x, 'i32')] if first == 'value' else [net.output_argmax(x, 'i32'), net.output(x, as_float=False)]
        assert ks == [0, 1]
        with pytest.raises(F8Error) as e:
            net.output(x, as_float=True)                           # a second VALUE mark stays refused
        assert e.value.status == INVALID
        net.finalize(2)
        assert sorted(net.output_kinds) == [0, 3]


def test_output_queries():
    net, x = _net(21, 5, 3)
    up = net.upsample(x, 4, 'bilinear', label='up')
    assert net.output(x, as_float=True) == 0 and net.output_argmax(up, 'u8') == 1 and net.output_argmax(x, 'i32') == 2
    net.finalize(3)
    assert net.outputs == [(21, 5, 3, 8, True), (1, 20, 12, 0, False), (1, 5, 3, 0, False)]
    assert net.output_kinds == [1, 2, 3]
    assert net.out_elems == 21 * 15 and net.output_fraclen == 8    # output 0 is the value output: as before
    net, x = _net(21, 5, 3)
    net.output_argmax(net.upsample(x, (2, 3), 'nearest'), 'i32')
    net.finalize(2)
    assert net.out_elems == 10 * 9 and net.output_fraclen == 0 and net.outputs == [(1, 10, 9, 0, False)] and net.output_kinds == [3]
    net, x = _net(1000, 1, 1)                                      # a classifier's predicted class: [N]
    net.output_argmax(x, 'i32')
    net.finalize(2)
    assert net.out_elems == 1 and net.outputs == [(1, 1, 1, 0, False)]


def test_option_key():
    net, x = _net()
    assert net.get_option('fuse_argmax') == 1
    net.set_option('fuse_argmax', 0)
    assert net.get_option('fuse_argmax') == 0
    for bad in (-1, 2):
        with pytest.raises(F8Error) as e:
            net.set_option('fuse_argmax', bad)
        assert e.value.status == INVALID
    net.output_argmax(x)
    net.finalize(1)
    with pytest.raises(F8Error) as e:
        net.set_option('fuse_argmax', 1)
    assert e.value.status == STATE


# ---- tokens and kernels
@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_token_and_kernel_of_every_case_on_every_leg(name):
    c = ac.CASES[name]
    data = ac.data_kinds(name)[-1]
    x = ac.make_input(name, data, c['N'] + 1)
    for leg, opts in ac.LEGS.items():
        g, _ = ac.plan(name, data, x, **opts)
        tok = ac.expected_token(name, opts)
        assert [(t, k) for _, t, k in ac.argmax_lines(g.net)] == [(tok, ac.SYMBOL[tok])], (leg, g.net.describe())
        ups = ac.upsample_lines(g.net)
        if tok.startswith('upsample_'):                            # fused: the upsample emits no launch
            assert not ups, (leg, g.net.describe())
        elif ac.is_upsampled(c):                                   # two launches: the upsample in int32 mode directly in front of the argmax
            (i, t, _), = ups
            assert t == f'upsample_{c["mode"]}_i32:' and ac.argmax_lines(g.net)[0][0] > i, (leg, g.net.describe())
        assert g.net.output_kinds == [0 if o[0] == 'value' else 2 if o[2] == 'u8' else 3 for o in g.outs]


@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_the_data_of_every_case_holds_what_it_promises(name):
    for data in ac.data_kinds(name):
        ac.reference(name, data)                                   # asserts _check_data


def test_the_argmax_launch_stands_directly_behind_its_producer():
    """As an output tap: behind the launch that writes what it reads, whatever its output index — output 0 included, which has no launch at the end."""
    net, x = _net(8, 4, 4)
    w = np.ones((21, 8, 1, 1), np.int32)
    a = net.conv(x, w, None, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, label='a')
    b = net.conv(a, np.ones((16, 21, 1, 1), np.int32), None, stride=1, pad=0, groups=1, weight_fl=5, input_fl=4, input_signed=False, label='b')
    assert net.output_argmax(a, 'u8') == 0 and net.output(b, as_float=False) == 1
    net.finalize(2)
    toks = [net.launch_info(i, 1)[0] for i in range(net.num_launches)]
    assert toks[1].endswith(':a') and toks[2] == 'argmax_u8:a' and toks[-1] == 'tap:b' and not any(t.startswith('output:') for t in toks), toks


def test_a_marked_classifier_writes_its_int32_form():
    """fuse_fc: the classifier writes the caller's buffer itself (dense) — unless its result carries an argmax mark, which reads the int32 form."""
    def fc(mark):
        net, x = _net(512, 1, 1)
        t = net.linear(x, np.ones((1000, 512), np.int32), None, weight_fl=5, input_fl=8, input_signed=False, label='fc')
        net.output(t, as_float=True)
        if mark:
            net.output_argmax(t, 'i32')
        return net.finalize(2).describe()
    assert 'dense=1' in fc(False) and 'output:' not in fc(False)
    plan = fc(True)
    assert 'dense=1' not in plan and 'argmax_i32:fc' in plan and 'output:fc' in plan, plan


# ---- the arena, the launch's accounting
@pytest.mark.parametrize('name', ['b16_21x2x2_u8', 'b4_19x3x3_i32', 'n23_21x3x2_u8'])
def test_a_fused_plan_lays_out_no_form_of_the_upsampled_tensor(name):
    c = ac.CASES[name]
    M = c['N'] + 1
    x = ac.make_input(name, 'random', M)
    fused, _ = ac.plan(name, 'random', x)
    two, t = ac.plan(name, 'random', x, fuse_argmax=0)
    _, _, P, Q = two.v[t][0].shape
    assert two.net.arena_bytes - fused.net.arena_bytes >= M * P * Q * 32 * 4      # the upsampled int32 form: 32 padded channels


def test_launch_info_and_valu_by_hand():
    # 21 real / 32 padded channels, source 5 x 3, output 10 x 6, u8: the source's blocks once + one byte a pixel; bilinear 4 + compare / select 3 per value
    g, _ = ac.plan('b2_21x5x3_u8', 'random', ac.make_input('b2_21x5x3_u8', 'random', 3))
    (i, _, _), = ac.argmax_lines(g.net)
    assert g.net.launch_info(i, 3)[1:] == (3 * (15 * 32 * 4 + 60 * 1), 0.0) and g.net.launch_valu(i, 3) == 3 * 60 * 21 * 7
    # unfused, int32 indices: 49 pixels x 32 padded channels read, 4 bytes a pixel written; 3 per value
    g, _ = ac.plan('c21_7x7_i32', 'random', ac.make_input('c21_7x7_i32', 'random', 4))
    (i, _, _), = ac.argmax_lines(g.net)
    assert g.net.launch_info(i, 2)[1:] == (2 * (49 * 32 * 4 + 49 * 4), 0.0) and g.net.launch_valu(i, 2) == 2 * 49 * 21 * 3
    assert g.net.step_launches(i, 2) == g.net.num_parts(2)


# ---- whole nets
def test_an_argmax_cuts_the_stage_chain_where_an_output_tap_does():
    """ResNet-50 at 224 x 224: stage_1_layer_1's output sits in the middle of what the stage chain runs as one launch.  Marked as an argmax output it cuts
    the chain exactly as a value tap does: the same launches, `argmax_i32:` where the tap plan has `tap:`."""
    name = 'stage_1_layer_1'
    spec = topology.get('resnet50')
    params = synth.make_params(spec, seed=17)
    plain = record_net(spec, params, 224).finalize(2)
    tapped = record_net(spec, params, 224, taps=(name,)).finalize(2)
    net = record_net(spec, params, 224)
    assert net.output_argmax(net.tap_ids[name], 'i32') == 1        # 512 channels: int32 indices
    net.finalize(2)
    names = lambda n: [n.launch_info(i, 1)[0] for i in range(n.num_launches)]
    assert names(net) == [s.replace('tap:', 'argmax_i32:') for s in names(tapped)] and names(net) != names(plain)
    assert sum(s.startswith('stage_chain') for s in names(net)) == sum(s.startswith('stage_chain') for s in names(plain)) + 1, names(net)
    assert net.outputs[1] == (1, 28, 28, 0, False) and net.output_kinds == [1, 3]


def test_a_net_without_an_argmax_output_plans_as_before():
    """The shipped nets, planned now, are in the recorded digests (the whole matrix: tests/test_plan_digest.py)."""
    graph_cases.shipped_digest_membership(graph_cases.all_shipped_jobs())


# ---- the reference
def test_reference_pinned_to_torch_ties_included():
    for name in ('c21_7x7', 'c33_6x6', 'c150_3x3', 'b8_33x2x3_u8'):
        for data in ac.data_kinds(name):
            g, t, _ = ac.reference(name, data)
            ac.pin_to_torch(g.v[t][0])
    v = np.zeros((2, 40, 3, 3), np.int32)                          # all equal: the first index
    v[1, 5] = v[1, 37] = 9
    ac.pin_to_torch(v)
    assert (ac.argmax_ref(v)[0] == 0).all() and (ac.argmax_ref(v)[1] == 5).all()


# ---- the C ABI from C, under the sanitizers
def test_host_example_under_the_sanitizers():
    out = graph_cases.sanitized_host_program('argmax_host.c')
    assert out.rstrip().endswith('ok')
    fused, both = out.split('== logits and classes')
    assert 'upsample_bilinear+argmax_u8:seg' in fused and 'upsample_bilinear_i32' not in fused and 'output 0: kind 2, 1 x 64 x 64, fraclen 0' in fused
    assert 'output 0: 4096 elements an image' in fused
    assert 'argmax_i32:' in both and 'output 1: kind 3, 1 x 16 x 16, fraclen 0' in both and 'output 0: kind 0, 21 x 16 x 16' in both


# ---- the torch op
def test_torch_op_meta_impl_and_module_arguments():
    import torch
    from f8net_amd import ops, torch_ops  # noqa: F401  (registers the op)
    x = torch.empty((2, 21, 5, 3), dtype=torch.int32, device='meta')
    for u8, dt in ((True, torch.uint8), (False, torch.int32)):
        y = torch.ops.f8net.argmax_channels(x, u8)
        assert tuple(y.shape) == (2, 5, 3) and y.dtype == dt and y.device.type == 'meta'
    with pytest.raises(ValueError, match='i64'):
        ops.F8ArgMax('i64')
    with pytest.raises(NotImplementedError):
        torch.ops.f8net.argmax_channels(torch.zeros((1, 3, 2, 2), dtype=torch.int32), True)      # there is no CPU implementation


# ---- ONNX
def _exported(dtype='u8'):
    from f8net_amd import onnx_export, onnx_io
    ig, x, want = ac.seg_tail_int_graph(dtype)
    return ig, onnx_io.load_graph(onnx_export.export_graph(ig))


@pytest.mark.parametrize('dtype', ['u8', 'i32'])
def test_onnx_round_trip(dtype):
    """Export -> import gives the same ops and the same output kind; build_net of both gives the same plan: the fused launch, no upsample launch."""
    from f8net_amd import onnx_import, onnx_io
    ig, g = _exported(dtype)
    assert [nd.op for nd in g.nodes[-2:]] == ['ArgMax', 'Cast'] and g.nodes[-2].attrs == {'axis': 1, 'keepdims': 0, 'select_last_index': 0}
    assert g.outputs[0][1] == (onnx_io.UINT8 if dtype == 'u8' else onnx_io.INT32)
    back = onnx_import.import_graph(g)
    graph_cases.same_ops(ig, back)
    assert back.output_argmax == dtype and not back.output_float
    a, b = ig.build_net(3, input_fraclen=ac.X_FL), back.build_net(3, input_fraclen=ac.X_FL)
    tok = f'upsample_bilinear+argmax_{dtype}:'
    assert a.describe() == b.describe() and [(t, k) for _, t, k in ac.argmax_lines(b)] == [(tok, ac.SYMBOL[tok])] and not ac.upsample_lines(b)
    assert b.output_kinds == [2 if dtype == 'u8' else 3] and b.outputs == [(1, 20, 12, 0, False)]
    assert onnx_import.IntGraph().output_argmax is None            # the default: a value output, as before


@pytest.mark.parametrize('form, dtype', [('alone', 'i32'), ('int64', 'i32'), ('keepdims', 'u8')])
def test_onnx_accepted_forms(form, dtype):
    """ArgMax alone (int64) and ArgMax + Cast(INT64) are returned as int32; keepdims = 1 is the same map."""
    from f8net_amd import onnx_import, onnx_io
    ig, g = _exported('u8')
    if form == 'alone':
        g.nodes.pop()
        g.nodes[-1].outputs[0] = 'output'
    elif form == 'int64':
        g.nodes[-1].attrs['to'] = onnx_io.INT64
    else:
        g.nodes[-2].attrs['keepdims'] = 1
    back = onnx_import.import_graph(g)
    assert back.output_argmax == dtype and back.output == ig.output


@pytest.mark.parametrize('what, says', [('axis', 'axis 2'), ('last_index', 'select_last_index'), ('feeds', 'feeds something other'), ('topk', 'TopK'),
                                        ('softmax', 'Softmax'), ('cast_float', 'Cast of an ArgMax')])
def test_onnx_import_errors_say_which(what, says):
    from f8net_amd import onnx_import, onnx_io
    ig, g = _exported('u8')
    amax, cast = g.nodes[-2], g.nodes[-1]
    if what == 'axis':
        amax.attrs['axis'] = 2
    elif what == 'last_index':
        amax.attrs['select_last_index'] = 1
    elif what == 'feeds':                                          # the Cast behind the ArgMax is not the output: a Relu reads it
        cast.outputs[0] = 'mid'
        g.nodes.append(onnx_io.Node('Relu', ['mid'], ['output'], name='/Relu_tail', attrs={}))
    elif what == 'topk':
        amax.op = 'TopK'
    elif what == 'softmax':
        amax.op = 'Softmax'
    else:
        cast.attrs['to'] = onnx_io.FLOAT
    with pytest.raises(onnx_import.OnnxImportError, match=says):
        onnx_import.import_graph(g)
