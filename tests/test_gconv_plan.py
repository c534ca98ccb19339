"""Grouped convolutions (1 < groups < cin) without a GPU: what the builder accepts and refuses with the option `grouped` at 0 / 1 / 2, the plan of
every case of tests/gconv_cases.py against the hand-written table on both legs, the kernel instances as exported symbols, depthwise plans left as
they were, the reference helper against torch, the liveness of every case on the reference's values, the ResNeXt topology tables, the exporter's
refusal and the ONNX round trip of `group`."""
import functools
import os
import subprocess

import numpy as np
import pytest

import dw_cases
import gconv_cases
from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net
from oracle import oracle
from ref_ops import grouped_conv2d

ALL = dict(gconv_cases.CASES, max_batch=gconv_cases.MAX_BATCH_CASE, pipelined=gconv_cases.PIPELINED_CASE)
F8_ERR_INVALID, F8_ERR_UNSUPPORTED, F8_ERR_STATE = -1, -2, -5


def test_status_codes_are_the_headers():
    L = _lib.lib()
    assert L.f8_status_string(F8_ERR_INVALID) == b'invalid argument' and L.f8_status_string(F8_ERR_UNSUPPORTED) == b'unsupported' and \
        L.f8_status_string(F8_ERR_STATE) == b'bad state'


@functools.lru_cache(maxsize=None)
def _planned(name, leg=1):
    case = ALL[name]
    return gconv_cases.plan(name, case, gconv_cases.make_input(name, case), leg)


def _g_net(grouped, C=32, groups=8, K=3, stride=1, pad=1, cout=None, hw=12):
    net = F8Net()
    if grouped is not None:
        net.set_option('grouped', grouped)
    t = net.input(C, hw, hw, 8)
    t = net.conv(t, np.ones((cout or C, C // groups, K, K), np.int32), None, stride=stride, pad=pad, groups=groups, weight_fl=4, input_fl=8,
                 input_signed=False, quant_input=False, relu=True)
    net.output(t, as_float=False)
    return net


def test_a_default_handle_still_refuses_with_the_old_message():
    assert F8Net().get_option('grouped') == 0
    for grouped in (None, 0):
        with pytest.raises(_lib.F8Error) as e:
            _g_net(grouped)
        assert e.value.status == F8_ERR_UNSUPPORTED and 'groups must be 1 or cin (depthwise)' in str(e.value)


@pytest.mark.parametrize('cg', [2, 4, 8, 16, 32])
def test_the_kernels_set_is_accepted_and_plans_one_launch(cg):
    for C in (64, 96):
        for stride in (1, 2):
            for pad in (0, 1):
                net = _g_net(1, C=C, groups=C // cg, stride=stride, pad=pad).finalize(2)
                lines = gconv_cases.g_lines(net)
                assert [ln[1:] for ln in lines] == [(f'gconv3x3s{stride}:', gconv_cases.kernel(stride))], net.describe()
                P = (12 + 2 * pad - 3) // stride + 1
                name, nbytes, ops = net.launch_info(lines[0][0], 2)
                assert ops == 2.0 * 9 * cg * C * P * P * 2                     # the grouped multiply-adds, not the expanded ones
                Cs = (C + 31) // 32 * 32
                assert nbytes == 2 * (12 * 12 * Cs + P * P * Cs * 4) + C * (9 * cg + 4)      # input once, the int32 output, the groups' weights
                assert net.launch_valu(lines[0][0], 2) == 0.0                  # no int8 form produced


def test_valu_counts_three_per_int8_value():
    g, _, _ = _planned('f_two_unsigned_s1')
    (i, _, _), = gconv_cases.g_lines(g.net)
    assert g.net.launch_valu(i, 3) == 3.0 * 2 * 9 * 11 * 32 * 3


@pytest.mark.parametrize('kw', [dict(C=48, groups=2), dict(C=32, groups=8, cout=64), dict(C=32, groups=4, K=1, pad=0), dict(C=32, groups=8, K=5, pad=2),
                                dict(C=32, groups=8, K=7, pad=3, stride=2), dict(C=32, groups=8, stride=3), dict(C=128, groups=2), dict(C=32, groups=8, pad=2)],
                         ids=lambda kw: '_'.join(f'{k}{v}' for k, v in kw.items()))
def test_everything_else_is_the_dense_expansion(kw):
    """cg = 24, cin != cout, kernel 1 / 5 / 7, stride 3, cg = 64, pad 2: accepted, planned as the plain conv over block-diagonal weights."""
    K, s = kw.get('K', 3), kw.get('stride', 1)
    for grouped in (1, 2):
        net = _g_net(grouped, **kw).finalize(2)
        lines = gconv_cases.g_lines(net)
        assert len(lines) == 1 and lines[0][1] == f'gconv{K}x{K}s{s}_dense:' and lines[0][2].startswith(gconv_cases.DENSE_KERNEL), net.describe()
        C, cout, G = kw['C'], kw.get('cout', kw['C']), kw['groups']
        P = (12 + 2 * kw.get('pad', 1) - K) // s + 1
        assert net.launch_info(lines[0][0], 2)[2] == 2.0 * K * K * (C // G) * cout * P * P * 2


def test_grouped_2_plans_the_kernels_set_as_the_expansion_too():
    net = _g_net(2).finalize(2)
    (_, tok, kern), = gconv_cases.g_lines(net)
    assert tok == 'gconv3x3s1_dense:' and kern.startswith(gconv_cases.DENSE_KERNEL)


@pytest.mark.parametrize('grouped', [1, 2])
def test_groups_that_do_not_divide_the_channels_are_invalid(grouped):
    for C, cout, groups in ((32, 32, 5), (30, 32, 3), (32, 30, 4)):
        net = F8Net().set_option('grouped', grouped)
        t = net.input(C, 8, 8, 8)
        with pytest.raises(_lib.F8Error) as e:
            w = np.ones((cout, max(1, C // groups), 3, 3), np.int32)
            d = _lib.ConvDesc(cin=C, cout=cout, kernel=3, stride=1, pad=1, groups=groups, weight_fl=4, input_fl=8, input_signed=0, quant_input=0, relu=0)
            import ctypes
            _lib.check(net._L.f8_net_conv(net._h, t, ctypes.byref(d), w.ctypes.data, None))
        assert e.value.status == F8_ERR_INVALID and 'must divide' in str(e.value)


def test_the_option_is_a_planning_key():
    net = _g_net(1)
    assert net.get_option('grouped') == 1
    net.finalize(2)
    with pytest.raises(_lib.F8Error) as e:
        net.set_option('grouped', 2)
    assert e.value.status == F8_ERR_STATE
    with pytest.raises(_lib.F8Error) as e:
        F8Net().set_option('grouped', 3)
    assert e.value.status == F8_ERR_INVALID


def test_the_environment_seeds_the_option(monkeypatch):
    monkeypatch.setenv('F8_GROUPED', '2')
    assert F8Net().get_option('grouped') == 2


@pytest.mark.parametrize('name', ['s_12x29', 'u_14x14', 'd_7x13_s2', 'f_gen_i32_and_i8'])
def test_depthwise_plans_do_not_change_with_the_option(name):
    case = dw_cases.CASES[name]
    x = dw_cases.make_input(name, case)
    texts = []
    for grouped in (0, 1, 2):
        g, _, _ = dw_cases.build_graph(case, x)
        for k, v in dict(case['opts'], grouped=grouped).items():
            g.net.set_option(k, v)
        g.net.finalize(x.shape[0])
        assert [ln[1:] for ln in dw_cases.dw_lines(g.net)] == dw_cases.expect(case, 'own'), (grouped, g.net.describe())
        texts.append((g.net.describe(), [g.net.launch_kernel(i) for i in range(g.net.num_launches)], g.net.weight_bytes, g.net.arena_bytes))
    assert texts[0] == texts[1] == texts[2]


def test_depthwise_keeps_its_own_rules_whatever_the_option_says():
    for grouped in (1, 2):
        net = _g_net(grouped, C=16, groups=16).finalize(2)                  # groups == cin == cout: depthwise
        assert [net.launch_info(i, 1)[0].split(':')[0] for i in range(net.num_launches)][1] == 'dwconv3x3s1', net.describe()
        with pytest.raises(_lib.F8Error) as e:
            _g_net(grouped, C=16, groups=16, K=9, pad=4)
        assert e.value.status == F8_ERR_UNSUPPORTED and 'kernel 3, 5 or 7' in str(e.value)


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    for leg in gconv_cases.LEGS:
        g, _, ids = _planned(name, leg)
        lines = gconv_cases.g_lines(g.net)
        assert gconv_cases.lines_match(lines, gconv_cases.expect(case, leg)), (leg, g.net.describe())
        assert len(lines) == len(ids)                                # one launch per grouped conv, an int32 form next to int8 ones included
        hw = (case['H'], case['W'])
        for (i, _, _), s in zip(lines, gconv_cases._strides(case)):
            P, Q = gconv_cases.out_hw(case, hw, s)
            assert g.net.launch_info(i, case['N'])[2] == 2.0 * case['K'] ** 2 * case['cg'] * case['cout'] * P * Q * case['N'], (leg, i)
            hw = (P, Q)
        if case['join_i32']:                                         # the planner keeps the int32 form and the int8 form on the one launch
            assert 'out[i32=1 i8=1' in [ln for ln in g.net.describe().splitlines() if 'gconv' in ln][0], g.net.describe()


def test_requant_float_keeps_the_symbol():
    for s in (1, 2):
        (_, _, kern), = gconv_cases.g_lines(_planned(f'f_rq1_s{s}')[0].net)
        assert kern == gconv_cases.kernel(s)


def test_the_kernel_instances_are_exported_symbols():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    for s in (1, 2):
        assert f'void {gconv_cases.kernel(s)}(f8::GConvArgs)' in syms, s


def test_a_tap_on_a_grouped_conv_plans():
    """f8_net_output on the grouped conv's own result next to the readers' sum: the launch writes the int32 form, a copy-out launch follows."""
    case = gconv_cases.GEOMETRY['s1_9x11']
    x = gconv_cases.make_input('s1_9x11', case)
    for leg in gconv_cases.LEGS:
        g, out, ids = gconv_cases.build_graph(case, x, leg)
        assert g.net.output(ids[0], as_float=False) == 1
        g.net.finalize(3)
        assert g.net.outputs[1][:3] == (32, 9, 11)
        assert 'out[i32=1 i8=1' in [ln for ln in g.net.describe().splitlines() if 'gconv' in ln][0], g.net.describe()


# ---- the reference helper

def test_the_helper_equals_torchs_grouped_conv_in_float64():
    torch = pytest.importorskip('torch')
    for k, (C, cout, G, K, s, p, H, W) in enumerate([(32, 32, 8, 3, 1, 1, 9, 11), (48, 48, 2, 3, 2, 1, 8, 10), (32, 64, 8, 3, 1, 0, 9, 9), (40, 40, 5, 3, 2, 1, 7, 7),
                                                      (32, 32, 4, 1, 1, 0, 5, 6), (32, 32, 8, 5, 2, 2, 9, 11)]):
        x = synth.rand_uniform_int(21, f'hx{k}', (2, C, H, W), -127, 127).astype(np.int32)
        w = synth.rand_uniform_int(22, f'hw{k}', (cout, C // G, K, K), -127, 127).astype(np.int32)
        b = synth.rand_normal_int(23, f'hb{k}', (cout,), 3e5).astype(np.int32)
        want = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=s, padding=p, groups=G)
        got = grouped_conv2d(x, w, b, s, p, G)
        assert np.abs(want.numpy()).max() < 2 ** 31                     # small values: nothing wraps, float64 is exact
        np.testing.assert_array_equal(got, want.numpy().astype(np.int64))
    with pytest.raises(Exception):
        oracle.conv2d(x, w, b, s, p, G)                                 # the oracle itself refuses these groups
    plain = oracle.conv2d
    with gconv_cases.grouped_oracle():
        assert oracle.conv2d is grouped_conv2d
        np.testing.assert_array_equal(oracle.conv2d(x, w, b, s, p, G), got)
    assert oracle.conv2d is plain                                       # put back behind the block


# ---- liveness

@pytest.mark.parametrize('name', sorted(ALL))
def test_liveness_on_the_reference(name):
    """A dead signal hides a failure — conditions on the case table, not measurements: the final value has more than 8 distinct values and is not all
    at a clamp bound; every int8 tensor a reader (or the second grouped conv and the 1x1 in front of it) reads has at least 16 distinct values and
    fewer than half of its entries at a clamp bound; a case that aims at a wrap shows it; the cross-talk cases leave every channel outside the live
    group at its bias."""
    case = ALL[name]
    g, out, ids = _planned(name)
    y = g.v[out][0]
    assert np.unique(y).size > 8
    assert ((y == y.max()) | (y == y.min())).mean() < 0.5
    assert len(g.taps) == len(case['readers'] or []) + (2 if case.get('second') else 0)
    for label, xq, sgn in g.taps:
        lo, hi = (-127, 127) if sgn else (0, 255)
        assert np.unique(xq).size >= 16, label
        assert ((xq == lo) | (xq == hi)).mean() < 0.5, label
    raw = g.raw[ids[0]]
    if case['only_group'] is not None:
        cg, gi = case['cg'], case['only_group']
        inside = np.zeros(case['cout'], bool)
        inside[gi * cg:(gi + 1) * cg] = True
        b = gconv_cases.biases(case)
        assert (raw[:, ~inside] == b[~inside][None, :, None, None]).all()
        assert (raw[:, inside] != b[inside][None, :, None, None]).mean() > 0.9
    if case['aim'] == 'bias_big':
        (fl, _), = case['readers']
        n = case['in_fl'] + case['w_fl'] - fl
        r = raw.astype(np.int64)
        assert (r > 2 ** 31 - 2 ** 13).any(), 'no accumulator next to 2^31'
        # the accumulator itself wrapped past 2^31, or the rounding add `v + 2^(n-1)` of the requantisation does: the reference then clamps to 0
        wraps = (r < -2 ** 30) | (r + (1 << (n - 1)) > 2 ** 31 - 1)
        # (channel 3's bias, 2^31 - 50, wraps with any sum above 50; channel 17's, 2^31 - 2^12, only where its group's sum is above 2^12 - 2^(n-1))
        assert wraps[:, 3].any() and not wraps[:, [c for c in range(case['cout']) if c not in (3, 17)]].any(), 'nothing wraps'
        assert (g.taps[0][1][wraps] == 0).all()
    else:
        assert case['aim'] is None


def test_the_groups_matter_in_every_case():
    """The grouped result differs from what a kernel that mixed neighbouring groups would give: rolling the input channels by cg changes it."""
    for name, case in ALL.items():
        if case['only_group'] is not None:
            continue
        x = gconv_cases.make_input(name, case)
        w, b, G = gconv_cases.weights(case), gconv_cases.biases(case), case['C'] // case['cg']
        a = grouped_conv2d(x, w, b, case['stride'], case['pad'], G)
        r = grouped_conv2d(np.ascontiguousarray(np.roll(x, case['cg'], axis=1)), w, b, case['stride'], case['pad'], G)
        assert (a != r).mean() > 0.5, name


# ---- topology, entry points, exporter, ONNX

def test_resnext_topology_tables():
    want = {'resnext50_32x4d': (32, [128, 256, 512, 1024], [3, 4, 6, 3]), 'resnext101_32x8d': (32, [256, 512, 1024, 2048], [3, 4, 23, 3]),
            'resnext101_64x4d': (64, [256, 512, 1024, 2048], [3, 4, 23, 3])}
    for arch, (G, mids, depth) in want.items():
        spec = topology.get(arch)
        assert spec.arch == arch and len(spec.blocks) == sum(depth) and spec.fc_in == 2048
        ch, k = 64, 0
        for si, n in enumerate(depth):
            for li in range(n):
                b = spec.blocks[k]
                k += 1
                stride = 2 if (li == 0 and si) else 1
                outp, mid = 256 << si, mids[si]
                assert b.name == f'stage_{si}_layer_{li}' and [c.key for c in b.body] == [f'{b.name}.body.{j}' for j in (0, 2, 4)]
                assert [(c.cin, c.cout, c.k, c.stride, c.pad, c.groups, c.relu) for c in b.body] == \
                    [(ch, mid, 1, 1, 0, 1, True), (mid, mid, 3, stride, 1, G, True), (mid, outp, 1, 1, 0, 1, False)]
                assert (b.shortcut is not None) == (li == 0) and b.residual and b.post_relu
                if b.shortcut is not None:
                    assert (b.shortcut.cin, b.shortcut.cout, b.shortcut.k, b.shortcut.stride) == (ch, outp, 1, stride)
                ch = outp
    assert topology.get('resnet50').blocks[0].body[1].groups == 1       # (the plain ResNet table is not touched)


@functools.lru_cache(maxsize=None)
def _resnext50():
    spec = topology.get('resnext50_32x4d')
    return spec, synth.make_params(spec, seed=31)


def test_make_params_shapes_follow_the_table():
    spec, params = _resnext50()
    for c in spec.convs():
        assert params[c.key + '.weight'].shape == (c.cout, c.cin // c.groups, c.k, c.k) and params[c.key + '.bias'].shape == (c.cout,)
    assert params['stage_0_layer_0.body.2.weight'].shape == (128, 4, 3, 3) and params['stage_3_layer_2.body.2.weight'].shape == (1024, 32, 3, 3)


def test_build_net_accepts_grouped_convs_by_itself():
    """build_net sets grouped = 1 when the table holds a grouped conv and the caller gave no value: every body.2 of ResNeXt-50 is a launch of its
    own on the new kernel, between body.0 and body.4 with its join; with options={'grouped': 2} they are the expansion."""
    spec, params = _resnext50()
    net = build_net(spec, params, 2, hw=64)
    assert net.get_option('grouped') == 1
    toks = [net.launch_info(i, 1)[0] for i in range(net.num_launches)]
    g = [t for t in toks if t.startswith('gconv')]
    assert len(g) == 16 and sum(t.startswith('gconv3x3s2:') for t in g) == 3 and sum(t.startswith('gconv3x3s1:') for t in g) == 13, net.describe()
    assert all(t.endswith('.body.2') for t in g)
    i = toks.index('gconv3x3s1:stage_0_layer_1.body.2')
    assert toks[i - 1].endswith(':stage_0_layer_1.body.0') and toks[i + 1].endswith('_res:stage_0_layer_1.body.4'), net.describe()
    net2 = build_net(spec, params, 2, hw=64, options={'grouped': 2})
    g2 = [net2.launch_info(i, 1)[0] for i in range(net2.num_launches) if net2.launch_info(i, 1)[0].startswith('gconv')]
    assert len(g2) == 16 and all('_dense:' in t for t in g2)
    assert build_net(topology.get('resnet18'), synth.make_params(topology.get('resnet18'), seed=3), 2, hw=64).get_option('grouped') == 0


def test_the_exporter_refuses_a_grouped_layer_in_the_references_words():
    pytest.importorskip('torch')
    from f8net_amd import export
    spec = topology.get('resnext50_32x4d')
    with pytest.raises(NotImplementedError, match='Group-wise conv with groups != in_channels is not supported'):
        export.export_int_state(spec, synth.make_float_state(spec, seed=77), export.ExportConfig())


def _small_resnext():
    """head 3x3 / 2 -> max-pool -> an opening bottleneck around a grouped 3x3 -> classifier, as a topology table."""
    C = topology.ConvSpec
    blk = topology.BlockSpec('stage_0_layer_0', [C('stage_0_layer_0.body.0', 32, 32, 1, 1, 0, relu=True), C('stage_0_layer_0.body.2', 32, 32, 3, 1, 1, groups=8, relu=True),
                                                 C('stage_0_layer_0.body.4', 32, 64, 1, 1, 0)], C('stage_0_layer_0.shortcut.0', 32, 64, 1, 1, 0), residual=True, post_relu=True)
    return topology.NetSpec('small_resnext', C('head.0', 3, 32, 3, 2, 1, relu=True), True, [blk], None, 'classifier.0', 64, 10)


def test_onnx_round_trips_group():
    from f8net_amd import onnx_export, onnx_import
    spec = _small_resnext()
    params = synth.make_params(spec, seed=41)
    ig = onnx_export.graph_from_params(spec, params, hw=32)
    assert [o.groups for o in ig.ops if o.kind == 'conv'] == [1, 1, 8, 1, 1]
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert [(o.kind, o.groups if o.kind == 'conv' else None, o.stride if o.kind == 'conv' else None) for o in back.ops] == \
        [(o.kind, o.groups if o.kind == 'conv' else None, o.stride if o.kind == 'conv' else None) for o in ig.ops]
    for a, b in zip(ig.ops, back.ops):
        if a.kind == 'conv':
            np.testing.assert_array_equal(a.weight, b.weight)
    x, x_fl = synth.make_input(spec, params, 2, 32, seed=3)
    with gconv_cases.grouped_oracle():
        want = oracle.net_forward(spec, params, x, x_fl)
        np.testing.assert_array_equal(oracle.graph_forward(back, x, x_fl), want)
    assert np.unique(want).size > 8
    net = back.build_net(2)                                           # IntGraph.build_net accepts the grouped conv by itself
    assert net.get_option('grouped') == 1 and 'gconv3x3s1:' in net.describe()
