"""The 256-entry table op on the CPU: f8net_amd.tables against its definition and the rounding bound, acceptance and every refusal of f8_net_table,
the plan tokens and kernel instances every case of tests/table_cases.py plans — by default, with every fusing pass on, with table_i8 = 0 and with
fuse_table = 0, written by hand there —, the host-composed byte tables' effect on the plan's value bound (a concat behind a table moves bytes), where
the op cuts the fused launches of ResNet-50 and MobileNet-V2 (exactly where an output tap does), the shipped nets' default plans against the
recorded digests, and the host code — table composition, value bound, argument checks — under AddressSanitizer / UndefinedBehaviorSanitizer as a
stand-alone program.  tests/test_gpu_table.py runs every case on the device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mul_cases as mc
import ref_ops
import table_cases as tc
from f8net_amd import onnx_export, onnx_import, onnx_io, synth, tables, topology
from f8net_amd._lib import F8Error
from f8net_amd.net import F8Net, build_net, record_net
from f8net_amd.onnx_import import OnnxImportError
from graph_cases import all_shipped_jobs, plan_digest_tool, same_ops, sanitized_host_program, shipped_digest_membership
from oracle import onnx_eval
from oracle import oracle
from refgraph import RefGraph, graph_forward

INVALID, STATE = -1, -5
FORMATS = [(8, False), (5, False), (0, False), (7, True), (4, True), (0, True)]


def _w(cout, cin, k=1):
    return np.ones((cout, cin, k, k), np.int32)


def _src(C=24, fl=8, w_fl=5, H=8, W=8):
    """input (8 channels) -> a 1x1 conv to C channels at fraclen fl + w_fl; returns (net, input id, conv id)."""
    net = F8Net()
    x = net.input(8, H, W, fl)
    return net, x, net.conv(x, _w(C, 8), None, stride=1, pad=0, groups=1, weight_fl=w_fl, input_fl=fl, input_signed=False, quant_input=False)


def _vec(net, x, C=24, w_fl=5):
    return net.linear(net.avgpool_sum(x), np.ones((C, 8), np.int32), None, weight_fl=w_fl, input_fl=8, input_signed=False, quant_input=True)


# ---- f8net_amd.tables against the definition
FUNCTIONS = {'sigmoid': (tables.sigmoid, torch.sigmoid), 'tanh': (tables.tanh, torch.tanh), 'swish': (tables.swish, lambda x: x * torch.sigmoid(x)),
             'mish': (tables.mish, lambda x: x * torch.tanh(F.softplus(x))), 'gelu': (tables.gelu, lambda x: 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))),
             'leaky_relu': (lambda *a: tables.leaky_relu(0.1, *a), lambda x: torch.where(x < 0, 0.1 * x, x)),
             'hard_sigmoid': (tables.hard_sigmoid, lambda x: torch.clamp(x + 3, 0, 6) / 6)}


@pytest.mark.parametrize('fn', sorted(FUNCTIONS))
@pytest.mark.parametrize('in_fl, in_signed', FORMATS)
def test_tables_are_the_function_on_the_grid_rounded_half_to_even(fn, in_fl, in_signed):
    make, f = FUNCTIONS[fn]
    q = torch.arange(256, dtype=torch.float64) - (128 if in_signed else 0)
    assert torch.equal(tables.grid(in_fl, in_signed), q / 2 ** in_fl)
    for out_fl in (0, 7, 12, 24, 38):
        t = make(in_fl, in_signed, out_fl)
        assert t.dtype == np.int32 and t.shape == (256,)
        real = f(q / 2 ** in_fl)                                                       # the definition, written out independently of torch's fused forms
        free = (real.abs() * 2.0 ** out_fl < 2 ** 31 - 1)                              # where the int32 clamp does not act
        err = (torch.from_numpy(t.astype(np.int64)).double() / 2.0 ** out_fl - real).abs()
        # the rounding bound, plus what float64 itself contributes to f and to the product (a few ulps of the value)
        assert bool((err[free] <= 2.0 ** -(out_fl + 1) + 8 * 2.0 ** -52 * (1 + real[free].abs())).all()), (fn, out_fl, float(err[free].max()))
        assert np.all(t[~free.numpy()] == np.where(real[~free].numpy() > 0, 2 ** 31 - 1, -2 ** 31))


def test_from_function_rounds_half_to_even_and_clamps():
    t = tables.from_function(lambda x: x / 2, 0, True, 0)                              # q / 2: every odd q is an exact tie
    q = np.arange(-128, 128)
    assert np.array_equal(t, np.where(q % 2 == 0, q // 2, np.where((q // 2) % 2 == 0, q // 2, q // 2 + 1)))
    big = tables.from_function(lambda x: x * 2.0 ** 31, 0, True, 1)
    assert big[0] == -2 ** 31 and big[255] == 2 ** 31 - 1 and big[128] == 0


def test_the_wrappers_record_their_table():
    for name in ('sigmoid', 'swish', 'tanh'):
        net, x, a = _src()
        t = getattr(net, name)(a, in_fl=4, in_signed=True, out_fl=10, label='op')
        assert net.tensor_info(t) == (24, 8, 8, 10)
        net.output(t, as_float=False)
        net.finalize(1)
        assert 'table_i32:op' in net.describe()


# ---- the reference is the definition
@pytest.mark.parametrize('in_fl, in_signed', FORMATS)
def test_reference_indexes_by_the_requantised_source(in_fl, in_signed):
    rng = np.random.default_rng(in_fl * 2 + in_signed)
    fl = in_fl + 3
    x = rng.integers(-2 ** 11, 2 ** 11, (2, 5, 3, 40), dtype=np.int64).astype(np.int32)
    table = rng.integers(-2 ** 31, 2 ** 31, 256, dtype=np.int64).astype(np.int32)
    y = ref_ops.table_ref(x, fl, table, in_fl=in_fl, in_signed=in_signed)
    q = oracle.requant_py(x, in_fl, fl, in_signed)                                     # the second, independent statement of the shift
    want = np.array([table[v + 128] if in_signed else table[v] for v in q.reshape(-1).tolist()], np.int32).reshape(x.shape)
    assert np.array_equal(y, want) and y.dtype == np.int32
    assert q.min() == (-127 if in_signed else 0) and q.max() == (127 if in_signed else 255)


# ---- the C ABI
def test_acceptance_shape_and_fraclen():
    net, x, a = _src(C=24)
    v = _vec(net, x)
    t = net.table(a, np.arange(256), in_fl=4, in_signed=True, out_fl=0, label='ramp')
    u = net.table(v, tables.sigmoid(8, False, 38), in_fl=8, in_signed=False, out_fl=38, label='deep')
    w = net.table(x, np.full(256, -2 ** 31), in_fl=8, in_signed=False, out_fl=5, label='raw')      # the net input, shift 0
    assert net.tensor_info(t) == (24, 8, 8, 0) and net.tensor_info(u) == (24, 1, 1, 38) and net.tensor_info(w) == (8, 8, 8, 5)
    net.output(t, as_float=False)
    for o in (u, w):
        assert net.output(o, as_float=False) >= 1
    net.finalize(2)
    d = net.describe()
    assert 'table_i32:ramp' in d and 'table_i32:deep' in d and 'table_i32:raw' in d


def test_the_table_is_copied_at_the_call():
    net, x, a = _src(C=32, H=7, W=7)
    tab = np.zeros(256, np.int32)
    t = net.table(a, tab, in_fl=4, in_signed=False, out_fl=4, label='op')
    other = net.conv(x, _w(32, 8), None, stride=1, pad=0, groups=1, weight_fl=2, input_fl=8, input_signed=False, quant_input=False)
    tab[:] = 2 ** 31 - 1                                                               # after the call: must not reach the plan's value bound
    cat = net.concat([t, other], label='cat')
    net.output(net.conv(cat, _w(32, 64), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(2)
    assert 'concat_i8:cat' in net.describe(), net.describe()


@pytest.mark.parametrize('what', ['bad_id', 'negative_id', 'in_fl_high', 'in_fl_signed_high', 'in_fl_negative', 'out_fl_high', 'out_fl_negative',
                                  'shift_high', 'short_table', 'float_table', 'finalized'])
def test_refusals(what):
    net, x, a = _src(C=24)
    tab = np.arange(256, dtype=np.int32)
    fmt = dict(in_fl=4, in_signed=False, out_fl=7)
    if what == 'shift_high':
        net2 = F8Net()
        far = net2.input(8, 4, 4, 39)
        with pytest.raises(F8Error) as e:
            net2.table(far, tab, in_fl=8, in_signed=False, out_fl=7)                   # shift 31
        assert e.value.status == INVALID and 'shift' in str(e.value)
        return
    if what in ('short_table', 'float_table'):
        with pytest.raises(ValueError):
            net.table(a, tab[:255] if what == 'short_table' else tab + 0.5, **fmt)
        return
    args = {'bad_id': (99, fmt), 'negative_id': (-1, fmt), 'in_fl_high': (a, dict(fmt, in_fl=9)), 'in_fl_signed_high': (a, dict(fmt, in_fl=8, in_signed=True)),
            'in_fl_negative': (a, dict(fmt, in_fl=-1)), 'out_fl_high': (a, dict(fmt, out_fl=39)), 'out_fl_negative': (a, dict(fmt, out_fl=-1)),
            'finalized': (a, fmt)}[what]
    status = INVALID
    if what == 'finalized':
        net.output(a, as_float=False)
        net.finalize(1)
        status = STATE
    with pytest.raises(F8Error) as e:
        net.table(args[0], tab, **args[1])
    assert e.value.status == status, str(e.value)
    if what.startswith('out_fl'):
        assert '[0, 38]' in str(e.value)


def test_null_desc_and_null_table_through_the_raw_abi():
    import ctypes
    from f8net_amd import _lib
    net, x, a = _src()
    L = _lib.lib()
    d = _lib.TableDesc(in_fl=4, in_signed=0, out_fl=7)
    tab = (ctypes.c_int32 * 256)()
    assert L.f8_net_table(net._h, a, None, tab) == INVALID
    assert L.f8_net_table(net._h, a, ctypes.byref(d), None) == INVALID
    assert L.f8_net_table(None, a, ctypes.byref(d), tab) == INVALID
    assert L.f8_net_table(net._h, a, ctypes.byref(d), tab) >= 0


def test_options():
    net = F8Net()
    for key, hi in (('table_i8', 1), ('fuse_table', 2)):
        assert net.get_option(key) == 1
        for v in range(hi + 1):
            net.set_option(key, v)
            assert net.get_option(key) == v
        for bad in (-1, hi + 1):
            with pytest.raises(F8Error):
                net.set_option(key, bad)
    later = plan_digest_tool().LATER
    assert later['table_i8'] == (0, 1) and later['fuse_table'] == (0, 2)


def test_the_torch_op_has_a_meta_impl_and_refuses_what_no_format_holds():
    from f8net_amd import ops  # noqa: F401  (registers torch.ops.f8net)
    x = torch.empty((2, 5, 3, 4), dtype=torch.int32, device='meta')
    t = torch.empty(256, dtype=torch.int32, device='meta')
    y = torch.ops.f8net.table_q(x, t, 13, 4, True, 10)
    assert y.shape == x.shape and y.dtype == torch.int32 and y.device.type == 'meta'
    from f8net_amd.torch_ops import _table_q
    xi = torch.zeros((1, 4, 2, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        _table_q(xi, torch.zeros(255, dtype=torch.int32), 13, 4, True, 10)
    with pytest.raises(ValueError):
        _table_q(xi, torch.zeros(256, dtype=torch.int32), 0, 8, True, 10)         # a left shift by 8 into a signed format: fraclen 8 > 7
    with pytest.raises(TypeError):
        _table_q(xi.float(), torch.zeros(256, dtype=torch.int32), 13, 4, True, 10)


# ---- tokens and kernels
@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_the_reference_of_every_case_carries_what_the_table_promises(name):
    """reference() asserts it: every reachable index within the first N and the first N - 1 images, ties of the index shift, both clamps."""
    ref, outs, ops = tc.reference(name)
    assert all(np.unique(ref.v[o][0]).size > 5 for o in outs)
    if tc.CASES[name]['table'] == 'ext':
        y = ref.v[ops[0]][0]
        assert (y == -2 ** 31).any() and (y == 2 ** 31 - 1).any() and (y == 0).any()


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_tokens_and_kernels_of_every_case(name):
    c = tc.CASES[name]
    x = tc.make_input(name)
    for opts in ({}, tc.FUSE_ALL, dict(table_i8=0), dict(fuse_table=0), dict(table_i8=0, fuse_table=0)):
        g, _, _ = tc.plan(name, x, max_batch=c['N'] + 1, **opts)
        assert [(t, k) for _, t, k in tc.lines(g.net)] == tc.expected(name, **opts), (opts, g.net.describe())


def test_tokens_of_the_mbconv_block():
    for opts in ({}, tc.FUSE_ALL, dict(table_i8=0), dict(fuse_table=0)):
        g = RefGraph(tc.mbconv_input(), tc.X_FL)
        tc.mbconv_block(g, next(iter(g.v)))
        for k, v in opts.items():
            g.net.set_option(k, v)
        g.net.finalize(2)
        assert [(t, k) for _, t, k in tc.lines(g.net)] == tc.expected_of(tc.MBCONV_TOKENS, tc.MBCONV_NOFUSE, **opts), (opts, g.net.describe())


def test_the_third_int8_format_is_a_requant_step():
    g, _, _ = tc.plan('rnd_s_8_three', tc.make_input('rnd_s_8_three'))
    names = [g.net.launch_info(i, 1)[0] for i in range(g.net.num_launches)]
    assert [n for n in names if n.startswith(('table', 'requant:op'))] == ['table_i32:op', 'requant:op']


@pytest.mark.parametrize('name', ['rnd_u_8', 'rnd_u_48_9x11', 'ext_u_20', 'sig_u_64', 'se_64', 'se_48_9x11'])
def test_an_i8_plan_writes_no_int32_form_of_the_result(name):
    g, _, _ = tc.plan(name, tc.make_input(name))
    i = tc.lines(g.net)[-1][0]
    assert 'i32=0' in g.net.describe().splitlines()[i], g.net.describe()


def test_a_fused_table_emits_no_launch_and_fuse_table_0_brings_it_back():
    x = tc.make_input('se_64')
    fused, _, _ = tc.plan('se_64', x)
    two, _, _ = tc.plan('se_64', x, fuse_table=0)
    assert two.net.num_launches == fused.net.num_launches + 1
    assert 'table_i8:gate' not in fused.net.describe() and 'table_i8:gate' in two.net.describe()


@pytest.mark.parametrize('C, H, fused', [(32, 112, True), (144, 56, True), (96, 112, False), (64, 128, False), (63, 128, True)])
def test_the_default_fuses_below_2_to_the_20_values_an_image(C, H, fused):
    """The measured rule (profiles/table_r15.md): fused on every measured shape up to 144 x 56 x 56, two launches on 96 x 112 x 112, where the fused
    launch came out slower; the threshold 2^20 = 64 x 128 x 128 itself is not fused.  fuse_table = 2 fuses every size, 0 none."""
    for opt, want in ((1, fused), (2, True), (0, False)):
        net, x, a = _src(C=C, H=H, W=H)
        gate = net.sigmoid(_vec(net, x, C=C), in_fl=4, in_signed=False, out_fl=12, label='gate')
        net.output(net.conv(net.mul(a, gate, a_fl=4, a_signed=False, b_fl=8, label='op'), _w(32, C), None, stride=1, pad=0, groups=1, weight_fl=6,
                            input_fl=4, input_signed=False), as_float=False)
        net.set_option('fuse_table', opt)
        net.finalize(1)
        d = net.describe()
        assert ('table+chmul_i8:op' in d) == want and ('table_i8:gate' in d) == (not want), (opt, d)


def test_an_element_wise_mul_and_an_output_table_do_not_fuse():
    net, x, a = _src(C=32, H=7, W=7)
    t = net.table(a, tables.sigmoid(4, False, 12), in_fl=4, in_signed=False, out_fl=12, label='gate')        # a's shape: element-wise
    net.output(net.mul(a, t, a_fl=4, a_signed=False, b_fl=8, label='op'), as_float=False)
    v = net.table(_vec(net, x, C=32), tables.sigmoid(4, False, 12), in_fl=4, in_signed=False, out_fl=12, label='vgate')
    net.output(net.mul(a, v, a_fl=4, a_signed=False, b_fl=8, label='op2'), as_float=False)
    net.output(v, as_float=False)                                                      # the vector gate is an output too
    net.finalize(2)
    d = net.describe()
    assert 'table_i8:gate' in d and 'mul_i32:op' in d and 'table_i32:vgate' in d and 'chmul_i32:op2' in d and 'table+' not in d, d


# (bytes / essential vector operations by hand.  Bytes: the real channels of the source in int8 and of each output form, each once; a fused table: the
#  mul's, its b one byte per image and channel.  Operations: a byte gather has none; the int32 mode 3 per int8 value produced)
@pytest.mark.parametrize('name, which, per_image, valu', [
    ('rnd_u_8', -1, 49 * 8 * (1 + 1), 0),
    ('ext_u_20', -1, 49 * 20 * (1 + 2), 0),
    ('rnd_u_64_out', -1, 49 * 64 * (1 + 4), 0),
    ('rnd_s_8_three', 0, 49 * 8 * (1 + 4 + 2), 49 * 8 * 6),
    ('se_64', -1, 49 * 64 * 2 + 64, 49 * 64 * 4),
])
def test_launch_info_and_valu_by_hand(name, which, per_image, valu):
    g, _, _ = tc.plan(name, tc.make_input(name))
    i = tc.lines(g.net)[which][0]
    for N in (1, 3):
        _, nbytes, ops = g.net.launch_info(i, N)
        const = 0 if name == 'se_64' else 1024 if 'i32' in tc.lines(g.net)[which][1] else 256 * (2 if name == 'ext_u_20' else 1)
        assert (nbytes, ops) == (N * per_image + const, 0)
        assert g.net.launch_valu(i, N) == N * valu


# ---- the value bound: the largest reachable entry
@pytest.mark.parametrize('signed, bounded', [(False, False), (True, True)])
def test_the_value_bound_is_over_the_reachable_entries(signed, bounded):
    """Entry 0 holds INT32_MIN, every other entry is small.  A signed table never reads entry 0: the result is bounded and a concat behind it
    moves bytes; the same table indexed unsigned reaches it and the concat stays in int32."""
    net, x, a = _src(C=32, H=7, W=7)
    tab = np.arange(256, dtype=np.int64) * 16
    tab[0] = -2 ** 31
    t = net.table(a, tab, in_fl=4, in_signed=signed, out_fl=9)
    other = net.conv(x, _w(32, 8), None, stride=1, pad=0, groups=1, weight_fl=2, input_fl=8, input_signed=False, quant_input=False)      # fraclen 10
    cat = net.concat([t, other], label='cat')
    net.output(net.conv(cat, _w(32, 64), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(2)
    assert ('concat_i8:cat' if bounded else 'concat_i32:cat') in net.describe(), net.describe()


# ---- the op cuts fused launches where a tap does
def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _backbone(net):
    return [n for n in _names(net) if not n.startswith(('tap:', 'table', 'mul_', 'chmul_')) and ':se.' not in n]


@pytest.mark.parametrize('op', ['swish', 'se'])
@pytest.mark.parametrize('arch, name', [('resnet50', 'stage_1_layer_1'), ('mobilenet_v2', 'stage_3_layer_1')])
def test_the_op_cuts_the_chain_where_a_tap_does(arch, name, op):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=7)
    plain = build_net(spec, params, 8, options=tc.FUSE_ALL)
    tapped = build_net(spec, params, 8, options=tc.FUSE_ALL, taps=(name,))
    net = record_net(spec, params, options=tc.FUSE_ALL)
    src = net.tap_ids[name]
    C, H, W, fl = net.tensor_info(src)
    if op == 'swish':
        t, want = net.swish(src, in_fl=4, in_signed=True, out_fl=8, label='op'), ['table_i32:op']
    else:
        v = net.linear(net.avgpool_sum(src, 6, label='se.pool'), np.ones((C, C), np.int32), None, weight_fl=0, input_fl=4, input_signed=True,
                       quant_input=True, label='se.fc')
        gate = net.sigmoid(v, in_fl=4, in_signed=True, out_fl=12, label='gate')
        t, want = net.mul(src, gate, a_fl=4, a_signed=True, b_fl=8, label='op'), ['table+chmul_i32:op']
    assert net.output(t, as_float=False) == 1
    for k, v in tc.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(8)
    assert _backbone(net) == _backbone(tapped), (net.describe(), tapped.describe())
    assert _backbone(plain) != _backbone(tapped), 'the tensor does not cut any fused launch: the comparison shows nothing'
    assert [n for n in _names(net) if n.startswith(('table', 'mul_', 'chmul_'))] == want


# ---- the shipped nets plan as before
def test_plan_digests_of_the_shipped_nets_are_the_recorded_ones():
    """tools/plan_digest.py's DEFAULT option column of a subset of the jobs: each planned line must be one of the recorded lines
    (tests/golden/plan_digest_default.txt).  Membership, not file equality: tests/test_plan_digest.py compares the whole file and the whole matrix."""
    assert 'table_cases' not in plan_digest_tool().CASE_MODULES
    shipped_digest_membership(all_shipped_jobs())


# ---- host code under the sanitizers
def test_host_code_under_asan_and_ubsan():
    """examples/table_host.c records `se`, `extreme` and `output` through the C ABI — argument checks, the value bound, byte tables composed from
    INT32_MIN / INT32_MAX entries by right and left shifts — finalizes, describes and destroys them.  f8_net.cpp's host side is compiled with
    AddressSanitizer and UndefinedBehaviorSanitizer and linked with the library's other objects into that stand-alone program."""
    out = sanitized_host_program('table_host.c', libs=['-lm'])
    assert out.rstrip().endswith('ok')
    assert out.count('table+chmul_i8:') == 1 and out.count(' table_i8:') == 2 and out.count(' table_i32:') == 1 and out.count('requant:') == 1


# ---- IntOp(kind='table'), the fraction-length solver's pins, ONNX in both directions
def test_onnx_round_trip_of_the_mbconv_block():
    """Export: per table the mul's requant subgraph, Add(128) for the signed index, Gather(axis=0) on a 256-entry int32 initializer; the importer maps
    each back to ONE op, and the imported graph plans the tokens of the recorded one (the sigmoid gate anchors the channel gate's b as a hard gate does)."""
    ig, g, out = tc.mbconv_int_graph()
    assert [o.kind for o in ig.ops].count('table') == 4 and [o.kind for o in ig.ops].count('mul') == 1
    data = onnx_export.export_graph(ig)
    graph = onnx_io.load_graph(data)
    gathers = [n for n in graph.nodes if n.op == 'Gather' and n.inputs[0] in graph.initializers]
    assert len(gathers) == 4 and all(n.attrs['axis'] == 0 for n in gathers)
    for n in gathers:
        arr = graph.initializers[n.inputs[0]]
        assert arr.shape == (256,) and arr.dtype == np.int32
    back = onnx_import.import_graph(data)
    same_ops(ig, back)
    assert back.solve_fraclens(tc.X_FL) == ig.solve_fraclens(tc.X_FL)
    x = tc.mbconv_input()
    np.testing.assert_array_equal(graph_forward(back, x, tc.X_FL), g.v[out][0])      # the walker against RefGraph's values
    net = back.build_net(2, input_fraclen=tc.X_FL)
    assert [(t, k) for _, t, k in tc.lines(net)] == tc.MBCONV_TOKENS, net.describe()


def test_onnx_file_with_an_unsigned_index_evaluates_to_the_reference():
    """An unsigned index has no offset node; every requantised value of this graph is non-negative (the file's integer Div truncates where the
    reference's shift floors: oracle/onnx_eval.py), so the exported file evaluated AS ONNX equals the reference."""
    ig, g, out = tc.unsigned_int_graph()
    data = onnx_export.export_graph(ig)
    graph = onnx_io.load_graph(data)
    (gather,) = [n for n in graph.nodes if n.op == 'Gather' and n.inputs[0] in graph.initializers]
    producer = {n.outputs[0]: n for n in graph.nodes}
    assert producer[gather.inputs[1]].op == 'Cast'                                     # straight from the requant's Clip / Cast: no Add(128)
    back = onnx_import.import_graph(data)
    same_ops(ig, back)
    x = mc.se_input()
    np.testing.assert_array_equal(graph_forward(back, x, tc.X_FL), g.v[out][0])      # the walker against RefGraph's values
    want = g.v[out][0]
    assert np.unique(want).size > 100 and all(v[0].min() >= 0 for k, v in g.v.items() if k != out)
    y = onnx_eval.run(graph, mc.se_input())
    np.testing.assert_array_equal(np.asarray(y).astype(np.int64).reshape(want.shape), want)


def test_the_solver_pins_a_tables_source_and_result_absolutely():
    ig, g, out = tc.mbconv_int_graph()
    V, _ = ig.solve_fraclens(tc.X_FL)
    tabs = [t for t, o in enumerate(ig.ops) if o.kind == 'table']
    assert [V[t] for t in tabs] == [ig.ops[t].out_fl for t in tabs] == [8, 8, 8, 12]
    assert [V[ig.ops[t].src] for t in tabs] == [ig.ops[t].in_fl + ig.ops[t].shift for t in tabs] == [9, 9, 9, 9]
    m = next(o for o in ig.ops if o.kind == 'mul')                                     # b = the sigmoid table: b_fl = out_fl - n_b is a constant
    assert V[ig.ops.index(m)] == (V[m.src] - m.shifts[0]) + (12 - m.shifts[1]) == 12
    # a second table on the same source that reads it at another absolute fraction length contradicts the first
    import copy
    bad, _, _ = tc.mbconv_int_graph()
    t0 = next(t for t, o in enumerate(bad.ops) if o.kind == 'table')
    bad.ops[t0].in_fl += 1                                                             # alone: the (otherwise free) source moves with it
    assert bad.solve_fraclens(tc.X_FL)[0][bad.ops[t0].src] == 10
    second = copy.copy(bad.ops[t0])
    second.in_fl -= 1                                                                  # same shift, another format: the source at 9 AND at 10
    bad.ops.append(second)
    with pytest.raises(OnnxImportError, match='no fraction-length assignment'):
        bad.solve_fraclens(tc.X_FL)
    for field, value, msg in (('out_fl', 39, '0 .. 38'), ('out_fl', -1, '0 .. 38'), ('in_fl', 8, '8-bit formats'), ('in_fl', -1, '8-bit formats')):
        bad, _, _ = tc.mbconv_int_graph()
        setattr(bad.ops[t0], field, value)
        with pytest.raises(OnnxImportError, match=msg):
            bad.solve_fraclens(tc.X_FL)


def _model(edit, make=tc.unsigned_int_graph):
    ig, _, _ = make()
    g = onnx_io.load_graph(onnx_export.export_graph(ig))
    edit(g, next(n for n in g.nodes if n.op == 'Gather' and n.inputs[0] in g.initializers))
    return onnx_io.model_proto(g)


def _rename(g, n, new, arr=None):
    old = g.initializers.pop(n.inputs[0])
    g.initializers[new] = old if arr is None else arr
    n.inputs[0] = new


@pytest.mark.parametrize('what, msg', [
    ('axis', 'along axis 1'), ('short', r'shape \(255,\)'), ('matrix', r'shape \(16, 16\)'), ('int64', 'type int64'), ('name', 'in_fl_<i>.out_fl_<o>'),
    ('raw_index', 'not a requantised activation'), ('offset_on_unsigned', 'offset 128 on a unsigned'), ('no_offset_on_signed', 'offset 0 on a signed'),
    ('activation', 'Gather of an activation'), ('sigmoid', 'Sigmoid')])
def test_importer_refusals(what, msg):
    make = tc.unsigned_int_graph
    if what == 'axis':
        def edit(g, n): n.attrs['axis'] = 1
    elif what in ('short', 'matrix', 'int64'):
        def edit(g, n):
            a = g.initializers[n.inputs[0]]
            _rename(g, n, n.inputs[0], {'short': a[:255].copy(), 'matrix': a.reshape(16, 16).copy(), 'int64': a.astype(np.int64)}[what])
    elif what == 'name':
        def edit(g, n): _rename(g, n, 'lookup')
    elif what == 'raw_index':
        def edit(g, n): n.inputs[1] = next(m for m in g.nodes if m.op == 'Mod').inputs[0]      # the stem's result itself, not requantised
    elif what == 'offset_on_unsigned':
        def edit(g, n):
            i = g.nodes.index(n)
            c = onnx_io.Node('Constant', [], ['/c128'], name='/c128', attrs={'value': np.array(128, np.int32)})
            add = onnx_io.Node('Add', [n.inputs[1], '/c128'], ['/idx128'], name='/idx128', attrs={})
            g.nodes[i:i] = [c, add]
            n.inputs[1] = '/idx128'
    elif what == 'no_offset_on_signed':
        make = tc.mbconv_int_graph

        def edit(g, n):
            add = next(m for m in g.nodes if m.outputs[0] == n.inputs[1])
            assert add.op == 'Add'
            n.inputs[1] = add.inputs[0]
    elif what == 'activation':
        def edit(g, n): n.inputs[0] = next(m for m in g.nodes if m.op == 'Mod').inputs[0]
    else:
        def edit(g, n):                                                                # a raw float Sigmoid stays refused
            n.op, n.inputs, n.attrs = 'Sigmoid', [n.inputs[1]], {}
    with pytest.raises(OnnxImportError, match=msg):
        onnx_import.import_graph(_model(edit, make))


def test_a_shipped_net_exports_and_imports_as_before():
    spec = topology.get('resnet18')
    ig = onnx_export.graph_from_params(spec, synth.make_params(spec, seed=5), 64)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert all(o.kind != 'table' for o in back.ops)
    same_ops(ig, back)
