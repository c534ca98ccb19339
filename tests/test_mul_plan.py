"""The fixed-point multiply and the hard gate on the CPU: the references of tests/mul_cases.py pinned to torch in float64 for every format pair of
the table, acceptance and refusals of f8_net_mul / f8_net_hard_gate, the plan tokens and kernel instances every case plans — by default, with every
fusing pass on and with fuse_hgate = 0, written by hand there —, launch_info / launch_valu by hand, tensor_amax behind a mul (a concat_i8: launch),
where the ops cut the fused launches of ResNet-50 and MobileNet-V2 (exactly where an output tap does), the IntOp round trip through ONNX with the
exported file evaluated by the oracle's ONNX walker, the importer's refusals, the shipped nets' default plans against the recorded digests, and the
host code under AddressSanitizer / UndefinedBehaviorSanitizer as a stand-alone program.  tests/test_gpu_mul.py runs every case on the device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mul_cases as mc
import ref_ops
from f8net_amd import onnx_export, onnx_import, onnx_io, synth, topology
from f8net_amd._lib import F8Error
from f8net_amd.net import F8Net, build_net, record_net
from f8net_amd.onnx_import import IntGraph, IntOp, OnnxImportError
from graph_cases import all_shipped_jobs, plan_digest_tool, same_ops, sanitized_host_program, shipped_digest_membership
from oracle import onnx_eval
from refgraph import RefGraph, graph_forward

INVALID, STATE = -1, -5


def _w(cout, cin, k=1):
    return np.ones((cout, cin, k, k), np.int32)


def _src(C=24, fl=8, w_fl=5, H=8, W=8):
    """input (8 channels) -> a 1x1 conv to C channels at fraclen fl + w_fl; returns (net, input id, conv id)."""
    net = F8Net()
    x = net.input(8, H, W, fl)
    return net, x, net.conv(x, _w(C, 8), None, stride=1, pad=0, groups=1, weight_fl=w_fl, input_fl=fl, input_signed=False, quant_input=False)


def _vec(net, x, C=24, w_fl=5):
    return net.linear(net.avgpool_sum(x), np.ones((C, 8), np.int32), None, weight_fl=w_fl, input_fl=8, input_signed=False, quant_input=True)


# ---- the references are torch's, in float64 (every value below 2^53: exact)
@pytest.mark.parametrize('a, b', mc.FORMATS)
def test_mul_reference_is_the_real_product(a, b):
    """A / 2^a_fl * B / 2^b_fl == out / 2^(a_fl + b_fl), for the element-wise product and the channel gate, with and without the ReLU."""
    rng = np.random.default_rng(a[0] * 100 + b[0] * 10 + a[1] * 2 + b[1])
    xa = rng.integers(-2 ** 11, 2 ** 11, (2, 5, 3, 4), dtype=np.int64).astype(np.int32)      # a shift by 3 leaves +-256: the clamps act
    for shape in ((2, 5, 3, 4), (2, 5, 1, 1)):
        xb = rng.integers(-2 ** 10, 2 ** 10, shape, dtype=np.int64).astype(np.int32)
        fa, fb = a[0] + 3, b[0] + 2
        A, B = ref_ops.mul_operands(xa, fa, xb, fb, a[0], a[1], b[0], b[1])
        assert A.min() >= (-127 if a[1] else 0) and A.max() <= (127 if a[1] else 255) and np.unique(A).size > 20
        for relu in (False, True):
            y, fl = ref_ops.mul_ref(xa, fa, xb, fb, a_fl=a[0], a_signed=a[1], b_fl=b[0], b_signed=b[1], relu=relu)
            assert fl == a[0] + b[0] and y.dtype == np.int32 and y.shape == xa.shape
            want = torch.from_numpy(A).double() / 2 ** a[0] * (torch.from_numpy(B).double() / 2 ** b[0])
            if relu:
                want = F.relu(want)
            assert torch.equal(torch.from_numpy(y).double() / 2 ** fl, want.expand(xa.shape))


@pytest.mark.parametrize('fl', [0, 2, 10, 13, 28])
def test_hard_gate_reference_is_relu6_of_x_plus_3(fl):
    x = np.random.default_rng(fl).integers(-5 * 2 ** fl - 3, 5 * 2 ** fl + 3, 4000, dtype=np.int64)
    x = np.concatenate([x, [-2 ** 31, 2 ** 31 - 1, 3 * 2 ** fl, -3 * 2 ** fl, 3 * 2 ** fl + 1, -3 * 2 ** fl - 1, 0]]).astype(np.int32)
    g = ref_ops.hard_gate_ref(x, fl)
    xr = torch.from_numpy(x).double() / 2 ** fl
    assert torch.equal(torch.from_numpy(g).double() / 2 ** fl, F.relu6(xr + 3))
    assert torch.equal(torch.from_numpy(g).double() / 2 ** fl, F.hardsigmoid(xr) * 6) or fl > 20      # (hardsigmoid divides and multiplies back: exact on small fraclens)
    assert g.min() == 0 and g.max() == 6 * 2 ** fl


def test_hard_swish_reference_is_six_times_torchs():
    """x_q * relu6(x + 3) with x read in its own format: six times hardswish of the value the format holds, up to the gate's own rounding —
    here the gate is read at its full fraclen (no rounding) and x at a format that holds it exactly."""
    fl = 4
    x = np.arange(-127, 128, dtype=np.int32).reshape(1, 5, 51, 1)                 # every signed 8-bit value at fraclen 4: -7.9 .. 7.9
    y, out_fl = ref_ops.mul_ref(x, fl, ref_ops.hard_gate_ref(x, fl), fl, a_fl=fl, a_signed=True, b_fl=fl, b_signed=False)
    xr = torch.from_numpy(x).double() / 2 ** fl
    want = xr * F.relu6(xr + 3)
    assert torch.equal(torch.from_numpy(y).double() / 2 ** out_fl, want)
    assert torch.allclose(want / 6, F.hardswish(xr), rtol=0, atol=1e-12)


# ---- the C ABI
def test_acceptance_shape_and_fraclen():
    net, x, a = _src(C=24)
    b = net.conv(x, _w(24, 8), None, stride=1, pad=0, groups=1, weight_fl=3, input_fl=8, input_signed=False, quant_input=False)
    v = _vec(net, x)
    m = net.mul(a, b, a_fl=4, a_signed=True, b_fl=3, label='prod')
    c = net.mul(a, v, a_fl=8, a_signed=False, b_fl=0, b_signed=True, relu=True, label='gated')
    sq = net.mul(a, a, a_fl=7, a_signed=True, b_fl=2)
    g = net.hard_gate(a, label='gate')
    hs = net.hard_swish(a, x_fl=4, x_signed=True, g_fl=5, label='hs')
    assert net.tensor_info(m) == (24, 8, 8, 7) and net.tensor_info(c) == (24, 8, 8, 8) and net.tensor_info(sq) == (24, 8, 8, 9)
    assert net.tensor_info(g) == (24, 8, 8, 13) and net.tensor_info(hs) == (24, 8, 8, 9)
    assert net.tensor_info(net.hard_gate(v)) == (24, 1, 1, net.tensor_info(v)[3])
    net.output(m, as_float=False)
    for t in (c, sq, g, hs):
        assert net.output(t, as_float=False) >= 1
    net.finalize(2)
    d = net.describe()
    assert 'mul_i32:prod' in d and 'chmul_i32:gated' in d and 'hgate:gate' in d and 'hgate+mul_i32:hs' in d


@pytest.mark.parametrize('what', ['bad_a', 'bad_b', 'negative_id', 'channels', 'map', 'vector_is_a', 'spatial_broadcast', 'a_fl_high', 'a_fl_signed_high',
                                  'b_fl_high', 'b_fl_negative', 'shift_low', 'finalized'])
def test_mul_refusals(what):
    net, x, a = _src(C=24)
    other = net.conv(x, _w(16, 8), None, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False)
    small = net.maxpool(a, 2, 2, 0)
    v = _vec(net, x)
    fmt = dict(a_fl=4, a_signed=False, b_fl=4, b_signed=False)
    args = {'bad_a': (99, a, fmt), 'bad_b': (a, 99, fmt), 'negative_id': (-1, a, fmt), 'channels': (a, other, fmt), 'map': (a, small, fmt),
            'vector_is_a': (v, a, fmt), 'spatial_broadcast': (a, small, fmt),
            'a_fl_high': (a, a, dict(fmt, a_fl=9)), 'a_fl_signed_high': (a, a, dict(fmt, a_fl=8, a_signed=True)),
            'b_fl_high': (a, v, dict(fmt, b_fl=8, b_signed=True)), 'b_fl_negative': (a, v, dict(fmt, b_fl=-1)),
            'shift_low': (x, x, dict(fmt, a_fl=8, b_fl=8)), 'finalized': (a, a, fmt)}[what]
    status = INVALID
    if what == 'finalized':
        net.output(a, as_float=False)
        net.finalize(1)
        status = STATE
    if what == 'shift_low':                                        # the input at fraclen 8 read at fraclen 8 is shift 0: accepted; the refusal needs a far source
        net2 = F8Net()
        far = net2.input(8, 4, 4, 40)
        with pytest.raises(F8Error) as e:
            net2.mul(far, far, a_fl=8, a_signed=False, b_fl=8, b_signed=False)    # shift 32
        assert e.value.status == INVALID and 'shift' in str(e.value)
        return
    with pytest.raises(F8Error) as e:
        net.mul(args[0], args[1], **args[2])
    assert e.value.status == status, str(e.value)


@pytest.mark.parametrize('what, status', [('bad_id', INVALID), ('negative_id', INVALID), ('fraclen_29', INVALID), ('finalized', STATE)])
def test_hard_gate_refusals(what, status):
    net, x, a = _src(C=24, w_fl=5)
    deep = net.conv(x, _w(24, 8), None, stride=1, pad=0, groups=1, weight_fl=21, input_fl=8, input_signed=False, quant_input=False)      # fraclen 29
    ok = net.conv(x, _w(24, 8), None, stride=1, pad=0, groups=1, weight_fl=20, input_fl=8, input_signed=False, quant_input=False)        # fraclen 28
    assert net.hard_gate(ok) >= 0
    arg = {'bad_id': 99, 'negative_id': -1, 'fraclen_29': deep, 'finalized': a}[what]
    if what == 'finalized':
        net.output(a, as_float=False)
        net.finalize(1)
    with pytest.raises(F8Error) as e:
        net.hard_gate(arg)
    assert e.value.status == status, str(e.value)


def test_option():
    net = F8Net()
    assert net.get_option('fuse_hgate') == 1
    net.set_option('fuse_hgate', 0)
    assert net.get_option('fuse_hgate') == 0
    for bad in (-1, 2):
        with pytest.raises(F8Error):
            net.set_option('fuse_hgate', bad)
    assert plan_digest_tool().LATER['fuse_hgate'] == (0, 1)


# ---- tokens and kernels
@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_the_reference_of_every_case_carries_what_the_table_promises(name):
    ref, outs, ops = mc.reference(name)                           # (asserts the extreme pairs, the ties and that values vary)
    assert all(np.unique(ref.v[o][0]).size > 5 for o in outs)


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_tokens_and_kernels_of_every_case(name):
    c = mc.CASES[name]
    x = mc.make_input(name)
    for opts in ({}, mc.FUSE_ALL, dict(fuse_hgate=0)):
        g, _, _ = mc.plan(name, x, max_batch=c['N'] + 1, **opts)
        assert [(t, k) for _, t, k in mc.lines(g.net)] == mc.expected(name, **opts), (opts, g.net.describe())


def test_the_third_int8_format_is_a_requant_step():
    g, _, _ = mc.plan('mul_threeforms', mc.make_input('mul_threeforms'))
    names = [g.net.launch_info(i, 1)[0] for i in range(g.net.num_launches)]
    assert [n for n in names if n.startswith(('mul_', 'requant:op'))] == ['mul_i32:op', 'requant:op']


@pytest.mark.parametrize('name', ['mul_uu_64', 'mul_twoforms', 'sq_two', 'ch_su_20', 'se_64', 'se_twoforms'])
def test_an_i8_plan_writes_no_int32_form_of_the_product(name):
    g, _, _ = mc.plan(name, mc.make_input(name))
    i = mc.lines(g.net)[-1][0]
    assert 'i32=0' in g.net.describe().splitlines()[i], g.net.describe()


def test_a_fused_gate_emits_no_launch_and_fuse_hgate_0_brings_it_back():
    for name in ('se_64', 'hsw_64'):
        x = mc.make_input(name)
        fused, _, _ = mc.plan(name, x)
        two, _, _ = mc.plan(name, x, fuse_hgate=0)
        assert two.net.num_launches == fused.net.num_launches + 1
        assert 'hgate:gate' not in fused.net.describe() and 'hgate:gate' in two.net.describe()
        assert two.net.arena_bytes >= fused.net.arena_bytes


def test_a_square_in_two_formats_reads_two_forms_of_one_tensor():
    g, _, _ = mc.plan('sq_two', mc.make_input('sq_two'))
    row = next(r for r in g.net.describe().splitlines() if 'conv1x1' in r)
    assert 'i8=2' in row and 'i32=0' in row, g.net.describe()


# (bytes / essential vector operations by hand.  Bytes: the real channels of a in int8, of b in int8 — int32 where the gate is fused —, of each output
#  form, each once.  Operations per product: the multiply, the ReLU where set, 3 per int8 value produced; a fused gate: 5 per gate value (clamp, offset, 3);
#  the stand-alone gate: 2 + 3 per int8 value)
@pytest.mark.parametrize('name, which, per_image, valu', [
    ('mul_uu_64', -1, 49 * 64 * (1 + 1 + 1), 49 * 64 * (1 + 3)),
    ('mul_twoforms', -1, 49 * 64 * (1 + 1 + 2), 49 * 64 * (1 + 3 * 2)),
    ('mul_ss_relu', -1, 49 * 20 * 3, 49 * 20 * (1 + 1 + 3)),
    ('mul_to_out', -1, 49 * 48 * (1 + 1 + 4), 49 * 48),
    ('mul_threeforms', 0, 49 * 64 * (1 + 1 + 4 + 2), 49 * 64 * (1 + 6)),
    ('ch_uu_64', -1, 49 * 64 * 2 + 64, 49 * 64 * 4),
    ('se_64', -1, 49 * 64 * 2 + 64 * 4, 49 * 64 * 4 + 64 * 5),
    ('hsw_64', -1, 49 * 64 * (1 + 4 + 1), 49 * 64 * (4 + 5)),
    ('hg_input_fl2', -1, 49 * 8 * (4 + 4), 49 * 8 * 2),
    ('hg_input_read', -1, 49 * 8 * (4 + 2), 49 * 8 * (2 + 6)),
])
def test_launch_info_and_valu_by_hand(name, which, per_image, valu):
    g, _, _ = mc.plan(name, mc.make_input(name))
    i = mc.lines(g.net)[which][0]
    for N in (1, 3):
        _, nbytes, ops = g.net.launch_info(i, N)
        assert (nbytes, ops) == (N * per_image, 0)
        assert g.net.launch_valu(i, N) == N * valu


# ---- tensor_amax: a product is bounded by its formats, a gate by 6 * 2^fl — a concat behind them qualifies for the byte mode
@pytest.mark.parametrize('what', ['mul', 'hgate'])
def test_a_concat_behind_the_op_moves_bytes(what):
    net, x, a = _src(C=32, H=7, W=7)
    if what == 'mul':
        t = net.mul(a, net.hard_gate(_vec(net, x, C=32)), a_fl=4, a_signed=False, b_fl=5)      # fraclen 9
    else:
        t = net.hard_gate(x)                                       # the raw input: unbounded by itself; its gate is 0 .. 6 * 2^8
    other = net.conv(x, _w(32, 8) if what == 'mul' else _w(8, 8), None, stride=1, pad=0, groups=1, weight_fl=2, input_fl=8, input_signed=False,
                     quant_input=False)                           # fraclen 10: the op's result is shifted by 1 / 2
    cat = net.concat([t, other], label='cat')
    C = 64 if what == 'mul' else 16
    net.output(net.conv(cat, _w(32, C), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(2)
    assert 'concat_i8:cat' in net.describe(), net.describe()


def test_a_concat_of_the_raw_input_itself_does_not():
    """The counterpart: without the gate nothing bounds the input, and the concat stays in int32."""
    net, x, a = _src(C=32, H=7, W=7)
    other = net.conv(x, _w(8, 8), None, stride=1, pad=0, groups=1, weight_fl=2, input_fl=8, input_signed=False, quant_input=False)
    cat = net.concat([x, other], label='cat')
    net.output(net.conv(cat, _w(32, 16), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(2)
    assert 'concat_i32:cat' in net.describe(), net.describe()


# ---- the ops cut fused launches where a tap does
def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _backbone(net):
    """The launches of the net itself: without the taps, the ops under test and the SE branch in front of them (labelled se.*)."""
    return [n for n in _names(net) if not n.startswith(('tap:', 'mul_', 'chmul_', 'hgate')) and ':se.' not in n]


@pytest.mark.parametrize('op', ['hswish', 'hgate', 'se'])
@pytest.mark.parametrize('arch, name', [('resnet50', 'stage_1_layer_1'), ('mobilenet_v2', 'stage_3_layer_1')])
def test_the_op_cuts_the_chain_where_a_tap_does(arch, name, op):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=7)
    plain = build_net(spec, params, 8, options=mc.FUSE_ALL)
    tapped = build_net(spec, params, 8, options=mc.FUSE_ALL, taps=(name,))
    net = record_net(spec, params, options=mc.FUSE_ALL)
    src = net.tap_ids[name]
    C, H, W, fl = net.tensor_info(src)
    if op == 'hswish':
        t, want = net.hard_swish(src, x_fl=4, x_signed=True, g_fl=5, label='op'), ['hgate+mul_i32:op']
    elif op == 'hgate':
        t, want = net.hard_gate(src, label='op'), ['hgate:op']
    else:
        v = net.linear(net.avgpool_sum(src, 6, label='se.pool'), np.ones((C, C), np.int32), None, weight_fl=0, input_fl=4, input_signed=True,
                       quant_input=True, label='se.fc')
        t, want = net.mul(src, net.hard_gate(v), a_fl=4, a_signed=True, b_fl=5, label='op'), ['hgate+chmul_i32:op']
    assert net.output(t, as_float=False) == 1
    for k, v in mc.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(8)
    assert _backbone(net) == _backbone(tapped), (net.describe(), tapped.describe())
    assert _backbone(plain) != _backbone(tapped), 'the tensor does not cut any fused launch: the comparison shows nothing'
    assert [n for n in _names(net) if n.startswith(('mul_', 'chmul_', 'hgate'))] == want


# ---- the two small nets
def test_tokens_of_the_mobilenet_v3_block_and_the_se_net():
    for build, x, fl, tokens, nofuse in ((lambda g, x0: mc.mbv3_block(g, x0)[0], mc.mbv3_input(), mc.X_FL, mc.MBV3_TOKENS, mc.MBV3_NOFUSE),
                                         (mc.se_net, mc.se_input(), mc.X_FL, mc.SE_TOKENS, None)):
        for opts in ({}, mc.FUSE_ALL, dict(fuse_hgate=0)):
            g = RefGraph(x, fl)
            build(g, next(iter(g.v)))
            for k, v in opts.items():
                g.net.set_option(k, v)
            g.net.finalize(x.shape[0])
            got = [(t, k) for _, t, k in mc.lines(g.net)]
            if 'fuse_hgate' not in opts:
                assert got == tokens, g.net.describe()
            elif nofuse:
                assert got == nofuse, g.net.describe()
            else:
                assert [t for t, _ in got].count('hgate:') == 2, g.net.describe()


# ---- ONNX
def test_onnx_round_trip_of_the_se_net_and_the_file_evaluates_to_the_reference():
    seen = {}
    ig, g, out = mc.se_int_graph(seen)
    assert seen['fc1'].min() > 0, 'a negative value in front of a requantisation: the file as ONNX truncates it where the reference floors'
    assert [o.kind for o in ig.ops].count('mul') == 2 and [o.kind for o in ig.ops].count('hgate') == 2
    data = onnx_export.export_graph(ig)
    graph = onnx_io.load_graph(data)
    assert sum(n.op == 'Unsqueeze' and n.attrs.get('axes') == [2, 3] for n in graph.nodes) == 1      # the [N, C] gate in front of its Mul
    back = onnx_import.import_graph(data)
    same_ops(ig, back)
    assert back.solve_fraclens(mc.X_FL) == ig.solve_fraclens(mc.X_FL)
    x = mc.se_input()
    np.testing.assert_array_equal(graph_forward(back, x, mc.X_FL), g.v[out][0])      # the walker against RefGraph's values
    V, _ = ig.solve_fraclens(mc.X_FL)
    gates = [t for t, o in enumerate(ig.ops) if o.kind == 'hgate']
    assert [V[t] for t in gates] == [ig.ops[t].shift for t in gates] == [9, 9]      # pinned absolutely
    net = back.build_net(3, input_fraclen=mc.X_FL)
    assert [(t, k) for _, t, k in mc.lines(net)] == mc.SE_TOKENS, net.describe()
    want = g.v[out][0]
    assert np.unique(want).size > 100
    y = onnx_eval.run(graph, mc.se_input())
    np.testing.assert_array_equal(np.asarray(y).astype(np.int64), want)


def _se_model(edit):
    ig, _, _ = mc.se_int_graph()
    g = onnx_io.load_graph(onnx_export.export_graph(ig))
    edit(g)
    return onnx_io.model_proto(g)


def _const_of(g, name):
    while True:
        n = next(n for n in g.nodes if n.outputs[0] == name)
        if n.op == 'Constant':
            return n
        name = n.inputs[0]                                         # (through a Cast)


def _gate_nodes(g):
    """(Clip, Add) of the first hard gate: the Clip whose upper bound is 3 * 2^9 (every requant's is 127 or 255), and the Add that reads it."""
    clip = next(n for n in g.nodes if n.op == 'Clip' and float(_const_of(g, n.inputs[2]).attrs['value']) == 3 << 9)
    names = {clip.outputs[0]}
    for n in g.nodes:                                              # (through the Cast behind the Clip)
        if n.op == 'Cast' and n.inputs[0] in names:
            names.add(n.outputs[0])
    return clip, next(n for n in g.nodes if n.op == 'Add' and names & set(n.inputs))


@pytest.mark.parametrize('what, match', [('unequal', 'equal constants'), ('offset', 'equal constants'), ('not_3_2k', 'is not')])
def test_onnx_import_refuses_a_malformed_gate(what, match):
    def edit(g):
        clip, add = _gate_nodes(g)
        lim = 3 << 9
        if what == 'unequal':
            _const_of(g, clip.inputs[2]).attrs['value'] = np.array(float(lim * 2), np.float32)
        elif what == 'offset':
            c = next(i for i in add.inputs if any(n.op == 'Constant' and n.outputs[0] == i for n in g.nodes))
            _const_of(g, c).attrs['value'] = np.array(lim + 1, np.int32)
        else:
            c = next(i for i in add.inputs if any(n.op == 'Constant' and n.outputs[0] == i for n in g.nodes))
            for name, v, dt in ((clip.inputs[1], -5.0 * 512, np.float32), (clip.inputs[2], 5.0 * 512, np.float32), (c, 5 * 512, np.int32)):
                _const_of(g, name).attrs['value'] = np.array(v, dt)
    with pytest.raises(OnnxImportError, match=match):
        onnx_import.import_graph(_se_model(edit))


def test_onnx_import_refuses_an_unanchored_mul():
    """Mul(requant(a), requant(b)) with b a conv result, not a hard gate's: V[out] = a_fl + b_fl is no difference constraint."""
    ig = IntGraph(input_signed=False)
    ig.ops.append(IntOp('input', shape=(8, 5, 5)))
    for k in range(2):
        ig.ops.append(IntOp('conv', src=0, weight=np.ones((8, 8, 1, 1), np.int32), bias=np.zeros(8, np.int32), kernel=1, shift=None, key=f'c{k}'))
    ig.ops.append(IntOp('mul', src=1, src2=2, shifts=[5, 5], signed=False, signed2=False))
    ig.output, ig.output_float = 3, False
    with pytest.raises(OnnxImportError, match='not anchored'):
        ig.solve_fraclens(8)
    with pytest.raises(OnnxImportError, match='anchored'):
        onnx_import.import_graph(onnx_export.export_graph(ig))


def test_a_shipped_net_exports_and_imports_as_before():
    spec = topology.get('resnet18')
    ig = onnx_export.graph_from_params(spec, synth.make_params(spec, seed=5), 64)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert all(o.kind not in ('mul', 'hgate') for o in back.ops)
    same_ops(ig, back)


# ---- the shipped nets plan as before
def test_plan_digests_of_the_shipped_nets_are_the_recorded_ones():
    """tools/plan_digest.py's DEFAULT option column: the lines recorded before these entry points existed (tests/golden/plan_digest_default.txt), of
    which a subset is planned here; and the op cases' digests (tests/golden/plan_digest_cases.txt): the tool's case modules are the ones they were."""
    assert 'mul_cases' not in plan_digest_tool().CASE_MODULES
    shipped_digest_membership(all_shipped_jobs())


# ---- host code under the sanitizers
def test_host_code_under_asan_and_ubsan():
    """examples/se_host.c records `se`, `hswish` and `shared` through the C ABI, finalizes, describes and destroys them.  f8_net.cpp's host side
    is compiled with AddressSanitizer and UndefinedBehaviorSanitizer and linked with the library's other objects into that stand-alone program."""
    out = sanitized_host_program('se_host.c')
    assert out.rstrip().endswith('ok')
    assert out.count('hgate+chmul_i8:') == 1 and out.count('hgate+mul_i32:') == 1 and out.count('hgate:') == 1 and out.count(' chmul_i8:') == 1
