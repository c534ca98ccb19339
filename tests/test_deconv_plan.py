"""Transposed convolutions on the CPU: f8_net_conv_transpose's acceptance and every refusal with its status, output shapes, the plan token, kernel
symbol and forms every case of tests/deconv_cases.py plans — written by hand there —, launch_info by hand, stride 1 recorded as a plain conv, where a
transposed conv cuts the fused launches of ResNet-50 (exactly where an output tap does), ONNX ConvTranspose and IntGraph round trips with the import
errors, the reference pinned to torch in float64 and to the oracle's conv over the zero-stuffed input for 314 geometries, the liveness of every
kernel tap of every case, the default plan digests of the shipped nets, the host code under the sanitizers as a stand-alone C program.
tests/test_gpu_deconv.py runs every case on the device."""
import itertools

import numpy as np
import pytest

import deconv_cases as dc
import ref_ops
from f8net_amd import onnx_export, onnx_import, onnx_io, synth, topology
from f8net_amd._lib import ConvDesc, F8Error, lib
from f8net_amd.net import F8Net, build_net, record_net
from graph_cases import all_shipped_jobs, same_ops, sanitized_host_program, shipped_digest_membership
from refgraph import graph_forward

INVALID, UNSUPPORTED, STATE = -1, -2, -5


def _one(C=40, H=3, W=5, fl=8, w_fl=5):
    """input (8 channels, H x W) -> a 1x1 conv with ReLU; returns (net, input id, conv id)."""
    net = F8Net()
    x = net.input(8, H, W, fl)
    t = net.conv(x, np.ones((C, 8, 1, 1), np.int32), None, stride=1, pad=0, groups=1, weight_fl=w_fl, input_fl=fl, input_signed=False, quant_input=False, relu=True)
    return net, x, t


def _deconv(net, t, k, s, pad, op, cin=40, cout=21, label='up', **kw):
    fmt = dict(weight_fl=6, input_fl=4, input_signed=False)
    fmt.update(kw)
    return net.conv_transpose(t, np.ones((cin, cout, k, k), np.int32), None, stride=s, pad=pad, output_padding=op, label=label, **fmt)


# ---- the C ABI
@pytest.mark.parametrize('k, s, pad, op, hw', [(2, 2, 0, 0, (6, 10)), (4, 2, 1, 0, (6, 10)), (3, 2, 1, 1, (6, 10)), (3, 2, 0, 0, (7, 11)), (4, 4, 0, 0, (12, 20)),
                                               (5, 3, 2, 1, (8, 14)), (8, 4, 2, 0, (12, 20)), (7, 2, 3, 1, (6, 10)), (1, 2, 0, 1, (6, 10)), (2, 3, 0, 0, (8, 14)),
                                               (3, 4, 1, 2, (11, 19)), (8, 4, 7, 3, (5, 13)), (1, 4, 0, 3, (12, 20))])
def test_acceptance_shape_fraclen_and_token(k, s, pad, op, hw):
    net, x, t = _one()
    u = _deconv(net, t, k, s, pad, op)
    net.output(u, as_float=False)
    net.finalize(2)
    assert net.output_info(0) == (21,) + hw + (10, False)
    assert hw == (dc.out_size(3, k, s, pad, op), dc.out_size(5, k, s, pad, op))
    (i, tok, sym), = dc.deconv_lines(net)
    assert (tok, sym) == (f'deconv{k}x{k}s{s}:', 'f8::deconv_kernel<1>'), net.describe()


@pytest.mark.parametrize('k, pad, hw', [(3, 1, (3, 5)), (3, 0, (5, 7)), (1, 0, (3, 5)), (4, 2, (0, 0)), (8, 4, (0, 0)), (2, 0, (4, 6))])
def test_stride_1_is_recorded_as_a_plain_conv(k, pad, hw):
    """flipped, swapped weights at pad' = k - 1 - pad: a conv token on a conv kernel, nothing of the transposed conv's in the plan."""
    net, x, t = _one()
    hw = hw if hw != (0, 0) else (dc.out_size(3, k, 1, pad, 0), dc.out_size(5, k, 1, pad, 0))
    u = _deconv(net, t, k, 1, pad, 0)
    net.output(u, as_float=False)
    net.finalize(2)
    assert net.output_info(0) == (21,) + hw + (10, False)
    (i, tok, sym), = dc.deconv_lines(net)
    assert tok.startswith(f'conv{k}x{k}s1') and sym.startswith('f8::conv') and 'deconv' not in net.describe(), net.describe()


REFUSALS = {
    # what: (source, (cin, cout, k, s, pad, groups, input_fl, weight_fl), output_padding, weight value, status, words its message names)
    'op_negative': ('t', (40, 21, 4, 2, 1, 1, 4, 6), -1, 1, INVALID, ('output_padding -1', 'stride 2')),
    'op_eq_stride': ('t', (40, 21, 4, 2, 1, 1, 4, 6), 2, 1, INVALID, ('output_padding 2', 'stride 2')),
    'op_at_stride_1': ('t', (40, 21, 3, 1, 1, 1, 4, 6), 1, 1, INVALID, ('output_padding 1', 'stride 1')),
    'empty_output': ('v', (40, 21, 2, 2, 1, 1, 4, 6), 0, 1, INVALID, ('empty output', '1 x 1', 'pad 1')),
    'weight_128': ('t', (40, 21, 4, 2, 1, 1, 4, 6), 0, 128, INVALID, ('128', 'int8')),
    'weight_m129': ('t', (40, 21, 4, 2, 1, 1, 4, 6), 0, -129, INVALID, ('-129', 'int8')),
    'cin': ('t', (32, 21, 4, 2, 1, 1, 4, 6), 0, 1, INVALID, ('cin 32', '40')),
    'input_fl': ('t', (40, 21, 4, 2, 1, 1, 9, 6), 0, 1, INVALID, ('input_fl 9',)),
    'bad_id': (99, (40, 21, 4, 2, 1, 1, 4, 6), 0, 1, INVALID, ('99',)),
    'stride0': ('t', (40, 21, 4, 0, 1, 1, 4, 6), 0, 1, INVALID, ('stride 0',)),
    'kernel9': ('t', (40, 21, 9, 2, 1, 1, 4, 6), 0, 1, UNSUPPORTED, ('kernel 9',)),
    'stride5': ('t', (40, 21, 4, 5, 1, 1, 4, 6), 0, 1, UNSUPPORTED, ('stride 5',)),
    'pad_k': ('t', (40, 21, 4, 2, 4, 1, 4, 6), 0, 1, UNSUPPORTED, ('pad 4', '3')),
    'groups2': ('t', (40, 20, 4, 2, 1, 2, 4, 6), 0, 1, UNSUPPORTED, ('groups 2',)),
    'depthwise': ('t', (40, 40, 4, 2, 1, 40, 4, 6), 0, 1, UNSUPPORTED, ('groups 40',)),
    'two_gib': ('big', (8, 64, 4, 4, 0, 1, 4, 6), 0, 1, UNSUPPORTED, ('2 GiB', '64')),
    'finalized': ('t', (40, 21, 4, 2, 1, 1, 4, 6), 0, 1, STATE, ('finalized',)),
}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refusals(what):
    src, (cin, cout, k, s, pad, groups, in_fl, w_fl), op, wv, status, words = REFUSALS[what]
    net, x, t = _one()
    if src == 'v':                                                  # a [40, 1, 1] tensor
        t = net.avgpool_sum(t, 4)
    elif src == 'big':                                              # 8 channels at 4096 x 4096: times (4, 4) and 64 channels it passes the bound
        net = F8Net()
        t = net.input(8, 4096, 4096, 4)
    if what == 'finalized':
        net.output(t, as_float=False)
        net.finalize(1)
    d = ConvDesc(cin=cin, cout=cout, kernel=k, stride=s, pad=pad, groups=groups, weight_fl=w_fl, input_fl=in_fl, input_signed=0, quant_input=1, relu=0)
    w = np.full((cin, cout, min(k, 9), min(k, 9)), 1, np.int32)
    w.reshape(-1)[-1] = wv
    import ctypes
    L = lib()
    assert L.f8_net_conv_transpose(net._h, t if isinstance(src, str) else src, ctypes.byref(d), op, w.ctypes.data, None) == status
    msg = L.f8_last_error().decode()
    assert msg.startswith('f8_net_conv_transpose') and all(wd in msg for wd in words), msg


def test_null_arguments_are_refused():
    import ctypes
    net, x, t = _one()
    L = lib()
    d = ConvDesc(cin=40, cout=21, kernel=2, stride=2, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=0, quant_input=1, relu=0)
    w = np.ones((40, 21, 2, 2), np.int32)
    assert L.f8_net_conv_transpose(None, t, ctypes.byref(d), 0, w.ctypes.data, None) == INVALID
    assert L.f8_net_conv_transpose(net._h, t, None, 0, w.ctypes.data, None) == INVALID
    assert L.f8_net_conv_transpose(net._h, t, ctypes.byref(d), 0, None, None) == INVALID
    assert L.f8_net_conv_transpose(net._h, t, ctypes.byref(d), 0, w.ctypes.data, None) >= 0


# ---- what every case plans
@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_token_kernel_and_forms_of_every_case(name):
    """The launch's token and symbol, the forms it writes (describe()), and — its source being a conv — that the source's producer writes the int8 form
    it reads in its own epilogue: no `requant:` step in front of the transposed conv."""
    c = dc.CASES[name]
    x = dc.make_input(name)
    for opts in ({}, dc.FUSE_ALL):
        g, _, ups = dc.plan(name, x, **opts)
        lines = dc.deconv_lines(g.net)
        dc.check_lines(c, lines, g.net.describe())
        (i, tok, _), = lines
        rows = g.net.describe().splitlines()
        o32, o8 = c['forms']
        assert f'out[i32={o32} i8={o8} ' in rows[i], g.net.describe()
        assert all('requant:' not in r for r in rows[:i + 1])
        assert sum('requant:up' in r for r in rows) == (1 if o32 + o8 == 3 else 0)
        if c['src'] != 'input':
            assert 'out[i32=0 i8=1 ' in rows[i - 1] and rows[i - 1].split()[1].startswith('conv1x1'), g.net.describe()
    ref, outs, rups = dc.reference(name)                            # the case carries values
    assert all(np.unique(ref.v[o][0]).size > 20 for o in outs + rups)


def test_join_behind_a_transposed_conv_stays_an_add_launch():
    g, _, _ = dc.plan('f_fcn', dc.make_input('f_fcn'), **dc.FUSE_ALL)
    names = [g.net.launch_info(i, 1)[0] for i in range(g.net.num_launches)]
    (i, _, _), = dc.deconv_lines(g.net)
    assert names[i + 1].startswith('add:') and not any('_res' in n for n in names), g.net.describe()


def test_two_concat_modes_ask_the_transposed_conv_for_different_forms():
    for name, tok in (('f_unet_i8', 'concat_i8:'), ('f_unet_i32', 'concat_i32:')):
        g, _, _ = dc.plan(name, dc.make_input(name))
        assert any(g.net.launch_info(i, 1)[0].startswith(tok) for i in range(g.net.num_launches)), g.net.describe()


# (the launch's algorithmic bytes and ops by hand: real / padded channels, in / out pixels per image)
@pytest.mark.parametrize('name, cin, cinS, cout, coutS, ipx, opx, kk', [
    ('g_2200', 8, 32, 8, 32, 15, 60, 4), ('g_3211', 64, 64, 130, 160, 15, 60, 9), ('g_5321', 160, 160, 21, 32, 15, 112, 25),
    ('g_7231_3x5', 96, 96, 8, 32, 15, 60, 49), ('f_out_reader', 64, 64, 64, 64, 15, 60, 16), ('e_3412', 8, 32, 64, 64, 49, 729, 9)])
def test_launch_info_and_valu_by_hand(name, cin, cinS, cout, coutS, ipx, opx, kk):
    g, _, _ = dc.plan(name, dc.make_input(name))
    (i, _, _), = dc.deconv_lines(g.net)
    o32, o8 = dc.CASES[name]['forms']
    for N in (1, 5):
        _, nbytes, nops = g.net.launch_info(i, N)
        assert nops == N * 2 * ipx * kk * cin * cout                # H W k^2 cin cout multiply-adds
        assert nbytes == N * (ipx * cinS + opx * coutS * (4 * o32 + o8)) + coutS * (kk * cinS + 4)      # input once + output forms; weights + bias once
        assert g.net.launch_valu(i, N) == N * 3 * opx * coutS * o8
    if name == 'g_2200':
        assert g.net.launch_info(i, 1)[1:] == (15 * 32 + 60 * 32 + 32 * 132, 2 * 15 * 4 * 64)


# ---- a transposed conv cuts fused launches where a tap does
def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _backbone(net):
    return [n for n in _names(net) if not n.startswith(('tap:', 'deconv', 'requant:'))]


@pytest.mark.parametrize('signed, in_fl', [(False, 4), (True, 3)])
def test_a_transposed_conv_cuts_the_chain_where_a_tap_does(signed, in_fl):
    """ResNet-50 stage_1_layer_1 sits inside the stage chain with all fusions on.  Read by a transposed conv it cuts the chain exactly where an output
    tap on it does; the transposed conv's int8 form is one more format of that tensor (a `requant:` step where the cut launch already writes two)."""
    spec = topology.get('resnet50')
    name = 'stage_1_layer_1'
    params = synth.make_params(spec, seed=7)
    plain = build_net(spec, params, 8, options=dc.FUSE_ALL)
    tapped = build_net(spec, params, 8, options=dc.FUSE_ALL, taps=(name,))
    net = record_net(spec, params, options=dc.FUSE_ALL)
    up = _deconv(net, net.tap_ids[name], 2, 2, 0, 0, cin=512, cout=64, input_fl=in_fl, input_signed=signed)
    assert net.output(up, as_float=False) == 1
    for k, v in dc.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(8)
    assert _backbone(net) == _backbone(tapped)
    assert _backbone(plain) != _backbone(tapped), 'the tensor does not cut any fused launch: the comparison shows nothing'
    assert [n for n in _names(net) if n.startswith('deconv')] == ['deconv2x2s2:up']
    assert sum(n.startswith('tap:') for n in _names(net)) == 1 and net.output_info(1)[:3] == (64, 56, 56)


# ---- ONNX and IntGraph
@pytest.mark.parametrize('name', ['g_2200', 'g_5321', 'g_7231', 'e_1201', 's_3110', 'f_fcn', 'f_unet_i8'])
def test_onnx_and_intgraph_round_trip(name):
    c = dc.CASES[name]
    ig, g, out = dc.int_graph(name)
    (op,) = [o for o in ig.ops if o.kind == 'deconv']
    assert 'up' in ig.layer_keys() and tuple(ig.state_dict(dc.X_FL)['up.weight'].shape) == (c['cin'], c['cout'], c['k'], c['k'])
    assert {'up.bias', 'up.weight_fraclen', 'up.input_fraclen'} <= set(ig.state_dict(dc.X_FL))
    data = onnx_export.export_graph(ig)
    (ct,) = [n for n in onnx_io.load_graph(data).nodes if n.op == 'ConvTranspose']
    assert (list(ct.attrs['strides']), list(ct.attrs['pads']), list(ct.attrs['output_padding']), list(ct.attrs['kernel_shape']), ct.attrs['group'],
            list(ct.attrs['dilations'])) == ([c['s']] * 2, [c['pad']] * 4, [c['op']] * 2, [c['k']] * 2, 1, [1, 1])
    back = onnx_import.import_graph(data)
    same_ops(ig, back)
    assert back.solve_fraclens(dc.X_FL) == ig.solve_fraclens(dc.X_FL)
    x = dc.make_input(name)
    np.testing.assert_array_equal(graph_forward(back, x, dc.X_FL), g.v[out][0])      # the walker against RefGraph's values
    net = back.build_net(2, input_fraclen=dc.X_FL)
    dc.check_lines(c, dc.deconv_lines(net), net.describe())


def _model(edit, name='g_5321'):
    ig, _, _ = dc.int_graph(name)
    g = onnx_io.load_graph(onnx_export.export_graph(ig))
    ct = next(n for n in g.nodes if n.op == 'ConvTranspose')
    edit(g, ct)
    return g


def _nonsquare(g, ct):
    w = g.initializers[ct.inputs[1]]
    g.initializers[ct.inputs[1]] = np.ascontiguousarray(w[:, :, :, :3])
    ct.attrs['kernel_shape'] = [5, 3]


@pytest.mark.parametrize('edit, match', [
    (_nonsquare, 'non-square kernel'),
    (lambda g, ct: ct.attrs.__setitem__('pads', [2, 2, 1, 1]), 'asymmetric pads'),
    (lambda g, ct: ct.attrs.__setitem__('auto_pad', b'SAME_UPPER'), 'auto_pad'),
    (lambda g, ct: ct.attrs.__setitem__('output_shape', [8, 14]), 'output_shape'),
    (lambda g, ct: ct.attrs.__setitem__('group', 2), 'group 2'),
    (lambda g, ct: ct.attrs.__setitem__('dilations', [2, 2]), 'dilations'),
    (lambda g, ct: ct.attrs.__setitem__('strides', [3, 2]), 'unequal strides'),
    (lambda g, ct: ct.attrs.__setitem__('output_padding', [1, 0]), 'output_padding'),
])
def test_onnx_import_errors_say_which(edit, match):
    with pytest.raises(onnx_import.OnnxImportError, match=match):
        onnx_import.import_graph(_model(edit))


def test_intgraph_refuses_what_the_library_refuses():
    ig, _, _ = dc.int_graph('g_5321')
    next(o for o in ig.ops if o.kind == 'deconv').output_padding = 3
    with pytest.raises(F8Error) as e:
        ig.build_net(2, input_fraclen=dc.X_FL)
    assert e.value.status == INVALID


# ---- the reference
GEOMETRIES = [(k, s, pad, op) for k in range(1, 9) for s in range(1, 5) for pad in range(k) for op in range(s)]


def test_reference_is_torch_float64_and_the_oracle_conv_over_the_stuffed_input():
    """Every accepted (k, s, pad, output_padding) on 3 x 2 maps — 360 tuples, 314 of them with an output — exact equality both ways."""
    assert len(GEOMETRIES) == 360
    n = 0
    for k, s, pad, op in GEOMETRIES:
        if dc.out_size(3, k, s, pad, op) < 1 or dc.out_size(2, k, s, pad, op) < 1:
            continue
        n += 1
        x = synth.rand_uniform_int(9, f'pinx{k}{s}', (2, 3, 3, 2), -127, 255)
        w = synth.rand_uniform_int(10, f'pinw{k}{s}', (3, 4, k, k), -127, 127)
        b = synth.rand_uniform_int(11, 'pinb', (4,), -2 ** 20, 2 ** 20).astype(np.int32)
        dc.pin_to_torch(x, w, b, s, pad, op)
        dc.pin_to_oracle(x, w, b, s, pad, op)
    assert n == 314


def test_wrap_cases_leave_the_int32_range_before_wrapping():
    for name in ('f_wrap', 'f_wrap_u8'):
        c = dc.CASES[name]
        ref, _, (up,) = dc.reference(name)
        w, b = dc.weights(c)
        src = ref.v[0][0] if c['src'] == 'input' else oracle_requant(ref, up)
        exact = ref_ops.deconv_exact(src, w, b, c['s'], c['pad'], c['op'])
        assert (np.abs(exact) >= 2 ** 31).sum() > 100 and (exact != ref.v[up][0]).sum() > 100
        np.testing.assert_array_equal(ref.v[up][0], ref_ops.wrap32(exact))


def oracle_requant(ref, up):
    from oracle import oracle
    (t,) = [t for t in ref.v if t not in (0, up) and t < up]        # the producer in front of the transposed conv
    return oracle.requant(ref.v[t][0], 4, ref.v[t][1], False)


@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_every_kernel_tap_of_every_case_is_live(name):
    """Zeroing any single tap (kh, kw) of the transposed conv's weights changes the case's reference outputs: no case can pass with a dead tap."""
    c = dc.CASES[name]
    x = dc.make_input(name)
    ref, outs, _ = dc.reference(name)
    w, _ = dc.weights(c)
    for kh, kw in itertools.product(range(c['k']), repeat=2):
        w0 = w.copy()
        w0[:, :, kh, kw] = 0
        assert (w0 != w).any()
        g, o2, _ = dc.build_graph(name, x, record=False, w_eval=w0)
        assert all((g.v[a][0] != ref.v[b][0]).any() for a, b in zip(o2, outs)), (name, kh, kw)


# ---- the shipped nets plan as before
def test_plan_digests_of_the_shipped_nets_are_the_parents():
    """tools/plan_digest.py's DEFAULT option column (tests/golden/plan_digest_default.txt, recorded before f8_net_concat existed), the subset
    tests/test_concat_plan.py plans: f8_net_conv_transpose adds no option key and changes no matcher."""
    shipped_digest_membership(all_shipped_jobs())


# ---- host code under the sanitizers
def test_host_code_under_asan_and_ubsan():
    """examples/deconv_host.c records a U-Net step (conv / 2 -> conv -> deconv 2x2 / 2 -> concat with the skip -> conv) and every phase shape of the
    packer through the C ABI, walks the refusals, finalizes, describes and destroys.  f8_net.cpp's host side is compiled with AddressSanitizer and
    UndefinedBehaviorSanitizer and linked with the library's other objects into that stand-alone program."""
    out = sanitized_host_program('deconv_host.c')
    assert out.rstrip().endswith('ok')
    assert out.count('deconv2x2s2:') == 1 and out.count('concat_i8:') == 1 and out.count('deconv') >= 5
