"""Depth-to-space and space-to-depth on the CPU: acceptance and refusals of f8_net_depth_to_space / f8_net_space_to_depth, the reference of
tests/pixmap_cases.py pinned to torch.nn.functional.pixel_shuffle / pixel_unshuffle, to the ONNX operators' definitions written out as reshape /
transpose and to the round trip, the data conditions of every case, the plan tokens and kernel instances every case plans on both legs of option
pixmap_i8 and with every fusing pass on — written by hand there —, launch_info / launch_valu by hand, where the ops cut ResNet-50's stage chain
(exactly where an output tap does), ONNX DepthToSpace / SpaceToDepth / the 6-D Reshape-Transpose-Reshape triple in both directions and the import
refusals, the torch ops' meta impls, the shipped nets' default plans against the recorded digests, and the host code under AddressSanitizer /
UndefinedBehaviorSanitizer as a stand-alone program.  tests/test_gpu_pixmap.py runs every case on the device."""
import numpy as np
import pytest
import torch

import pixmap_cases as pm
from f8net_amd import onnx_export, onnx_import, onnx_io, synth, topology
from f8net_amd._lib import F8Error
from f8net_amd.net import F8Net, build_net, record_net
from graph_cases import all_shipped_jobs, plan_digest_tool, same_ops, sanitized_host_program, shipped_digest_membership

INVALID, UNSUPPORTED, STATE = -1, -2, -5


def _w(cout, cin, k=1):
    return np.ones((cout, cin, k, k), np.int32)


def _src(C=36, H=8, W=6, fl=8, w_fl=5):
    """input (8 channels, H x W) -> a 1x1 conv to C channels; returns (net, input id, conv id)."""
    net = F8Net()
    x = net.input(8, H, W, fl)
    return net, x, net.conv(x, _w(C, 8), None, stride=1, pad=0, groups=1, weight_fl=w_fl, input_fl=fl, input_signed=False, quant_input=False)


# ---- the C ABI
def test_acceptance_shape_and_fraclen():
    net, x, a = _src(C=36)
    up = net.depth_to_space(a, 3, 'dcr', label='up')
    ps = net.pixel_shuffle(a, 2, label='ps')
    down = net.space_to_depth(a, 2, 'dcr', label='down')
    pu = net.pixel_unshuffle(x, 2)
    assert net.tensor_info(up) == (4, 24, 18, 13) and net.tensor_info(ps) == (9, 16, 12, 13)
    assert net.tensor_info(down) == (144, 4, 3, 13) and net.tensor_info(pu) == (32, 4, 3, 8)
    assert net.tensor_info(net.depth_to_space(a, 6)) == (1, 48, 36, 13)                    # order defaults to 'crd'
    r = net.conv(ps, _w(32, 9), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False)
    net.output(r, as_float=False)
    assert net.output(down, as_float=False) == 1
    net.finalize(2)
    assert net.output_info(1) == (144, 4, 3, 13, False)
    assert 's2d2dcr_i32:down' in net.describe() and 'd2s2crd_i8:ps' in net.describe()
    with pytest.raises(ValueError):
        F8Net().depth_to_space(0, 2, 'rcd')


@pytest.mark.parametrize('op', ['d2s', 's2d'])
@pytest.mark.parametrize('what, status', [('bad_id', INVALID), ('negative_id', INVALID), ('block1', INVALID), ('block0', INVALID), ('block_negative', INVALID),
                                          ('order2', INVALID), ('order_negative', INVALID), ('not_dividing', INVALID), ('block17', UNSUPPORTED),
                                          ('two_gib', UNSUPPORTED), ('finalized', STATE)])
def test_refusals(op, what, status):
    """Through the C symbols themselves (F8Net's methods take the order as a word).  36 channels on 8 x 6: 5^2 does not divide 36, 5 divides neither side."""
    from f8net_amd._lib import check
    net, x, a = _src(C=36)
    args = {'bad_id': (99, 2, 1), 'negative_id': (-1, 2, 1), 'block1': (a, 1, 1), 'block0': (a, 0, 0), 'block_negative': (a, -2, 1), 'order2': (a, 2, 2),
            'order_negative': (a, 2, -1), 'not_dividing': (a, 5, 1), 'block17': (a, 17, 0), 'two_gib': None, 'finalized': (a, 2, 1)}[what]
    if what == 'two_gib':                                          # [64, 4096, 4096] -> [16, 8192, 8192] / [256, 2048, 2048]: 2^30 values
        huge = F8Net()
        net, args = huge, (huge.input(64, 4096, 4096, 8), 2, 1)
    if what == 'finalized':
        net.output(a, as_float=False)
        net.finalize(1)
    fn = net._L.f8_net_depth_to_space if op == 'd2s' else net._L.f8_net_space_to_depth
    with pytest.raises(F8Error) as e:
        check(fn(net._h, *args))
    assert e.value.status == status, str(e.value)


def test_sixteen_is_the_largest_block_and_only_one_side_must_divide():
    net = F8Net()
    x = net.input(256, 16, 32, 8)
    assert net.tensor_info(net.depth_to_space(x, 16, 'crd')) == (1, 256, 512, 8)
    assert net.tensor_info(net.space_to_depth(x, 16, 'dcr')) == (65536, 1, 2, 8)
    net2 = F8Net()
    z = net2.input(12, 9, 6, 8)
    assert net2.tensor_info(net2.space_to_depth(z, 3, 'crd')) == (108, 3, 2, 8)               # 12 is no multiple of 9: space_to_depth does not ask
    assert net2.tensor_info(net2.depth_to_space(z, 2, 'crd')) == (3, 18, 12, 8)               # 9 x 6 is no multiple of 4: depth_to_space does not ask


def test_option_and_its_digest_entry():
    net = F8Net()
    assert net.get_option('pixmap_i8') == 1
    net.set_option('pixmap_i8', 0)
    assert net.get_option('pixmap_i8') == 0
    for bad in (-1, 2):
        with pytest.raises(F8Error):
            net.set_option('pixmap_i8', bad)
    tool = plan_digest_tool()
    assert tool.LATER['pixmap_i8'] == (0, 1)
    assert 'pixmap_cases' not in tool.CASE_MODULES                 # (tests/test_plan_digest_cases.py compares case_lines() with a recorded file)


def test_the_environment_seeds_the_option(monkeypatch):
    monkeypatch.setenv('F8_PIXMAP_I8', '0')
    assert F8Net().get_option('pixmap_i8') == 0


# ---- the reference
def _rand(shape, seed):
    return np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize('op, order, r, C', pm.SHAPES)
def test_reference_is_torchs_and_onnxs(op, order, r, C):
    """CRD against torch; both orders against the ONNX operators' definitions (DepthToSpace: the operator's own reshape / transpose of its
    documentation; SpaceToDepth: reshape [N, C, H / r, r, W / r, r], transpose [0, 3, 5, 1, 2, 4]); each order's pair is a round trip."""
    F = torch.nn.functional
    deep, wide = _rand((2, C * r * r, 3, 2), C * 100 + r), _rand((2, C, 3 * r, 2 * r), C * 100 + r + 1)
    up, down = pm.d2s_ref(deep, r, order), pm.s2d_ref(wide, r, order)
    if order == 'crd':
        np.testing.assert_array_equal(up, F.pixel_shuffle(torch.from_numpy(deep), r).numpy())
        np.testing.assert_array_equal(down, F.pixel_unshuffle(torch.from_numpy(wide), r).numpy())
        onnx_up = deep.reshape(2, C, r, r, 3, 2).transpose(0, 1, 4, 2, 5, 3).reshape(2, C, 3 * r, 2 * r)
    else:
        onnx_up = deep.reshape(2, r, r, C, 3, 2).transpose(0, 3, 4, 1, 5, 2).reshape(2, C, 3 * r, 2 * r)
        np.testing.assert_array_equal(down, wide.reshape(2, C, 3, r, 2, r).transpose(0, 3, 5, 1, 2, 4).reshape(2, C * r * r, 3, 2))
    np.testing.assert_array_equal(up, onnx_up)
    np.testing.assert_array_equal(pm.s2d_ref(up, r, order), deep)
    np.testing.assert_array_equal(pm.d2s_ref(down, r, order), wide)
    # the formulas of include/f8net.h on a few coordinates
    for (n, c, h, w, i, j) in ((0, 0, 0, 0, 0, 0), (1, C - 1, 2, 1, r - 1, 0), (1, C // 2, 1, 1, 0, r - 1), (0, C - 1, 2, 0, r - 1, r - 1)):
        sc = c * r * r + i * r + j if order == 'crd' else (i * r + j) * C + c
        assert up[n, c, h * r + i, w * r + j] == deep[n, sc, h, w]
        assert down[n, sc, h, w] == wide[n, c, h * r + i, w * r + j]


@pytest.mark.parametrize('name', sorted(pm.CASES))
def test_the_data_of_every_case_tells_a_wrong_kernel(name):
    """pixmap_cases.check_data (run by pm.reference): every op result differs from the other order, from i and j swapped and from nearest
    replication, and no two channels are equal; outputs carry values."""
    ref, outs, ops = pm.reference(name)
    assert all(np.unique(ref.v[o][0]).size > 50 for o in outs)
    assert ops and all(t in ref.srcv for t in ops)


# ---- tokens and kernels
@pytest.mark.parametrize('name', sorted(pm.CASES))
def test_tokens_and_kernels_of_every_case(name):
    c = pm.CASES[name]
    x = pm.make_input(name)
    for opts in ({}, pm.FUSE_ALL, dict(pixmap_i8=0)):
        g, _, _ = pm.plan(name, x, max_batch=c['N'] + 1, **opts)
        assert [(t, k) for _, t, k in pm.lines(g.net)] == pm.expected(name, **opts), (opts, g.net.describe())


def test_the_instance_rule_by_hand():
    """DESIGN 4.5q on the table: the run mover iff DCR and the small side's channels are a multiple of 16; the transposer iff CRD, r = 2 and a
    multiple of 4; else the general kernel."""
    for name, c in pm.CASES.items():
        for tok, sym in c['exp']:
            if tok.endswith('_i32:'):
                assert sym == pm.K32
                continue
            op, order, r, C = tok[:3], tok[-7:-4], int(tok[3:-7]), c['C']
            want = (pm.RUN if C % 16 == 0 else pm.GEN) if order == 'dcr' else ({'d2s': pm.TD, 's2d': pm.TS}[op] if r == 2 and C % 4 == 0 else pm.GEN)
            assert sym == want, (name, tok)


def test_the_third_int8_format_is_a_requant_step():
    g, _, _ = pm.plan('d2s_al_threeforms', pm.make_input('d2s_al_threeforms'))
    names = [g.net.launch_info(i, 1)[0] for i in range(g.net.num_launches)]
    assert [n for n in names if n.startswith(('d2s', 'requant:'))] == ['d2s2dcr_i32:op', 'requant:op']


@pytest.mark.parametrize('name', ['d2s2_crd_64', 's2d2_dcr_19', 'rt2_dcr_16', 'd2s2_crd_16_twoforms', 's2d2_crd_40'])
def test_an_i8_plan_holds_no_int32_form_up_to_its_last_op(name):
    g, _, _ = pm.plan(name, pm.make_input(name))
    last = pm.lines(g.net)[-1][0]
    rows = g.net.describe().splitlines()[:last + 1]
    assert all('i32=0' in r and 'requant:' not in r for r in rows), g.net.describe()


def test_the_round_trip_is_two_launches():
    g, _, _ = pm.plan('rt3_crd_3', pm.make_input('rt3_crd_3'))
    assert [t for _, t, _ in pm.lines(g.net)] == ['d2s3crd_i8:', 's2d3crd_i8:']


# (bytes / essential vector operations by hand: i8 — every real byte read once and written once, per form; i32 — the source's real int32 values read,
#  the padded output forms written, 3 operations per int8 value produced.  Pixels per image: depth_to_space 10 x 6 = 60 at r = 2; space_to_depth 5 x 3 = 15)
@pytest.mark.parametrize('name, per_image, valu', [
    ('d2s2_crd_19', 2 * 60 * 19, 0),
    ('d2s_al_twoforms', 2 * 60 * 16 * 2, 0),
    ('s2d_odd_to_out', 15 * (76 * 4 + 96 * 4), 0),                              # int32 in, the int32 form (96 padded channels) out
    ('s2d_al_threeforms', 15 * (64 * 4 + 64 * (4 + 2)), 15 * 64 * 3 * 2),       # int32 in; the int32 form and two int8 forms out
])
def test_launch_info_and_valu_by_hand(name, per_image, valu):
    g, _, _ = pm.plan(name, pm.make_input(name))
    (i, _, _), = pm.lines(g.net)
    for N in (1, 3):
        _, nbytes, ops = g.net.launch_info(i, N)
        assert (nbytes, ops) == (N * per_image, 0)
        assert g.net.launch_valu(i, N) == N * valu
        assert g.net.launch_grid(i, N) == g.net.launch_grid(pm.lines(g.net)[0][0], N)
    s, _, _ = pm.plan('d2s_al_to_out', pm.make_input('d2s_al_to_out'))            # ... and launch_grid answers as for a slice: no stage-chain geometry
    import chanmap_cases as cm
    sl, _, _ = cm.plan('sl_to_out', cm.make_input('sl_to_out'))
    assert s.net.launch_grid(pm.lines(s.net)[0][0], 3) == sl.net.launch_grid(cm.lines(sl.net)[0][0], 3)


# ---- the op cuts fused launches where a tap does
def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


def _backbone(net):
    return [n for n in _names(net) if not n.startswith(('tap:', 'd2s', 's2d'))]


@pytest.mark.parametrize('op', ['d2s', 's2d'])
def test_the_op_cuts_resnet50s_stage_chain_where_a_tap_does(op):
    name = 'stage_1_layer_1'                                        # 512 x 28 x 28 inside what the stage chain runs as one launch
    spec = topology.get('resnet50')
    params = synth.make_params(spec, seed=7)
    plain = build_net(spec, params, 8, options=pm.FUSE_ALL)
    tapped = build_net(spec, params, 8, options=pm.FUSE_ALL, taps=(name,))
    net = record_net(spec, params, options=pm.FUSE_ALL)
    t = net.depth_to_space(net.tap_ids[name], 2, 'crd', label='op') if op == 'd2s' else net.space_to_depth(net.tap_ids[name], 2, 'dcr', label='op')
    assert net.output(t, as_float=False) == 1
    for k, v in pm.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(8)
    assert _backbone(net) == _backbone(tapped)
    assert net.num_launches == tapped.num_launches + 1             # the tap there; here the op and the tap on it
    assert _backbone(plain) != _backbone(tapped), 'the tensor does not cut any fused launch: the comparison shows nothing'
    assert [n for n in _names(net) if n.startswith(('d2s', 's2d'))] == ['d2s2crd_i32:op' if op == 'd2s' else 's2d2dcr_i32:op']


# ---- ONNX
ONNX_CASES = ['d2s2_crd_19', 'd2s3_dcr_8', 's2d2_dcr_40', 's2d2_crd_12', 's2d3_crd_8', 'rt2_dcr_16', 'rt3_crd_3']


@pytest.mark.parametrize('name', ONNX_CASES)
def test_onnx_export_and_import_give_the_same_graph(name):
    """DepthToSpace(blocksize, mode) for both modes, SpaceToDepth(blocksize) for DCR, the 6-D Reshape / Transpose / Reshape triple for CRD
    space_to_depth.  same_ops does not know block / order: compared next to it.  The imported graph plans the case's launches."""
    c = pm.CASES[name]
    ig, g, out = pm.int_graph(name)
    ig.output_float = False
    data = onnx_export.export_graph(ig)
    nodes = onnx_io.load_graph(data).nodes
    kinds = [(o.kind, o.order) for o in ig.ops if o.kind in ('d2s', 's2d')]
    assert sum(n.op == 'DepthToSpace' for n in nodes) == sum(k == 'd2s' for k, _ in kinds)
    assert sum(n.op == 'SpaceToDepth' for n in nodes) == kinds.count(('s2d', 'dcr'))
    assert sum(n.op == 'Transpose' for n in nodes) == kinds.count(('s2d', 'crd'))
    for n in nodes:
        if n.op == 'DepthToSpace':
            assert n.attrs['mode'] == c['order'].upper().encode() and n.attrs['blocksize'] == c['r']
        if n.op == 'Transpose':
            assert list(n.attrs['perm']) == [0, 1, 3, 5, 2, 4]
    back = onnx_import.import_graph(data)
    same_ops(ig, back)
    assert [(o.block, o.order) for o in back.ops] == [(o.block, o.order) for o in ig.ops]
    assert back.solve_fraclens(c['x_fl']) == ig.solve_fraclens(c['x_fl'])
    net = back.build_net(c['N'], input_fraclen=c['x_fl'])
    assert [(t, k) for _, t, k in pm.lines(net)] == c['exp'], net.describe()


def _const_of(g, name):
    return next(n for n in g.nodes if n.op == 'Constant' and n.outputs[0] == name)


def _reshapes(g):
    """The Reshape nodes whose shape operand is a constant, in file order: [the 6-D view, the 4-D result]."""
    consts = {n.outputs[0] for n in g.nodes if n.op == 'Constant'}
    return [n for n in g.nodes if n.op == 'Reshape' and n.inputs[1] in consts]


def _triple_model(edit):
    ig, _, _ = pm.int_graph('s2d2_crd_12')                          # [12, 10, 6] -> view [N, 12, 5, 2, 3, 2] -> [48, 5, 3]
    g = onnx_io.load_graph(onnx_export.export_graph(ig))
    edit(g)
    return onnx_io.model_proto(g)


def test_the_six_d_triple_as_torch_writes_it():
    """torch names the batch as 0 or -1 in both Reshapes; the import takes either."""
    def edit(g):
        for n in _reshapes(g):
            c = _const_of(g, n.inputs[1])
            c.attrs['value'] = np.array([0] + list(c.attrs['value'][1:]), np.int64)
    ig, _, _ = pm.int_graph('s2d2_crd_12')
    back = onnx_import.import_graph(_triple_model(edit))
    same_ops(ig, back)
    assert [(o.kind, o.block, o.order) for o in back.ops if o.kind == 's2d'] == [('s2d', 2, 'crd')]


@pytest.mark.parametrize('what, match', [('perm', r'perm \[0, 1, 5, 3, 2, 4\]'), ('factor_c', 'must factor'), ('factor_r', 'must factor'), ('factor_map', 'must factor'),
                                         ('back', 'behind the space_to_depth Transpose to'), ('back_missing', 'missing or not a constant'),
                                         ('view_missing', 'Transpose of something other'), ('mode', 'mode'), ('blocksize', 'blocksize 17'),
                                         ('d2s_channels', 'no multiple of 9'), ('s2d_map', 'no multiple of 4')])
def test_onnx_import_refusals(what, match):
    def edit(g):
        tr = next((n for n in g.nodes if n.op == 'Transpose'), None)
        if what == 'perm':
            tr.attrs['perm'] = [0, 1, 5, 3, 2, 4]
        elif what.startswith('factor'):
            shape = {'factor_c': [-1, 6, 5, 2, 6, 2], 'factor_r': [-1, 12, 5, 2, 2, 3], 'factor_map': [-1, 12, 2, 5, 3, 2]}[what]
            _const_of(g, _reshapes(g)[0].inputs[1]).attrs['value'] = np.array(shape, np.int64)
        elif what == 'back':
            _const_of(g, _reshapes(g)[1].inputs[1]).attrs['value'] = np.array([-1, 48, 3, 5], np.int64)
        elif what in ('back_missing', 'view_missing'):              # the shape operand is no constant: another node's result
            n = _reshapes(g)[1 if what == 'back_missing' else 0]
            shape = _const_of(g, n.inputs[1])
            at = g.nodes.index(shape)
            g.nodes.insert(at + 1, onnx_io.Node('Concat', [shape.outputs[0]], ['/computed_shape'], name='/Concat_shape', attrs={'axis': 0}))
            n.inputs[1] = '/computed_shape'
    if what in ('mode', 'blocksize', 'd2s_channels', 's2d_map'):
        name = {'mode': 'd2s2_crd_19', 'blocksize': 'd2s2_crd_19', 'd2s_channels': 'd2s2_crd_19', 's2d_map': 's2d2_dcr_40'}[what]
        ig, _, _ = pm.int_graph(name)
        g = onnx_io.load_graph(onnx_export.export_graph(ig))
        n = next(n for n in g.nodes if n.op in ('DepthToSpace', 'SpaceToDepth'))
        if what == 'mode':
            n.attrs['mode'] = b'RCD'
        else:
            n.attrs['blocksize'] = {'blocksize': 17, 'd2s_channels': 3, 's2d_map': 4}[what]
        data = onnx_io.model_proto(g)
    else:
        data = _triple_model(edit)
    with pytest.raises(onnx_import.OnnxImportError, match=match):
        onnx_import.import_graph(data)


def test_a_shipped_net_and_the_shuffle_triple_import_as_before():
    import chanmap_cases as cm
    spec = topology.get('resnet18')
    ig = onnx_export.graph_from_params(spec, synth.make_params(spec, seed=5), 64)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert all(o.kind not in ('d2s', 's2d') for o in back.ops)
    same_ops(ig, back)
    ig, _, _ = cm.stage_int_graph()
    same_ops(ig, onnx_import.import_graph(onnx_export.export_graph(ig)))


# ---- the torch ops
def test_torch_ops_meta_impls():
    from f8net_amd import torch_ops  # noqa: F401  (registers the ops)
    x = torch.empty((3, 76, 5, 3), dtype=torch.int32, device='meta')
    assert torch.ops.f8net.depth_to_space(x, 2, 'crd').shape == (3, 19, 10, 6)
    assert torch.ops.f8net.depth_to_space(x, 2, 'dcr').dtype == torch.int32
    y = torch.empty((2, 3, 20, 12), dtype=torch.int32, device='meta')
    assert torch.ops.f8net.space_to_depth(y, 4, 'dcr').shape == (2, 48, 5, 3)
    assert torch.ops.f8net.space_to_depth(y, 2, 'crd').shape == torch.nn.functional.pixel_unshuffle(y, 2).shape
    for bad in (lambda: torch.ops.f8net.depth_to_space(x, 3, 'crd'), lambda: torch.ops.f8net.space_to_depth(y, 8, 'crd'),
                lambda: torch.ops.f8net.depth_to_space(x, 2, 'rcd'), lambda: torch.ops.f8net.depth_to_space(x, 1, 'crd')):
        with pytest.raises(Exception):
            bad()


# ---- the shipped nets plan as before
def test_plan_digests_of_the_shipped_nets_are_the_recorded_ones():
    shipped_digest_membership(all_shipped_jobs())


# ---- host code under the sanitizers
def test_host_code_under_asan_and_ubsan():
    """examples/pixshuffle_host.c records `espcn`, `edsr` and `stem` through the C ABI, finalizes, describes and destroys them.  f8_net.cpp's host side is
    compiled with AddressSanitizer and UndefinedBehaviorSanitizer and linked with the library's other objects into that stand-alone program."""
    out = sanitized_host_program('pixshuffle_host.c')
    assert out.rstrip().endswith('ok')
    assert out.count('d2s3crd_i32:') == 1 and out.count('d2s2crd_i8:') == 1 and out.count('s2d4dcr_i8:') == 1
