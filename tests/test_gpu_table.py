"""The 256-entry table op on the device, bit for bit against the reference of tests/table_cases.py (table[oracle.requant(x) + offset] in numpy):
every case on the default plan, with every fusing pass on, with table_i8 = 0 and with fuse_table = 0, each at N and N - 1 images from one handle
planned for N + 1; an EfficientNet MBConv block, recorded and imported from ONNX; a sigmoid SE branch inside ResNet-50's stage chain;
torch.ops.f8net.table_q / F8Table / F8Sigmoid / F8Swish against the same reference.
tests/test_table_plan.py checks on the CPU which tokens and kernel instances every case plans."""
import numpy as np
import pytest
import torch

import table_cases as tc
from f8net_amd import ops, tables  # (ops registers torch.ops.f8net)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _outputs(got, n, wants):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(wants)
    return [y.cpu().numpy().reshape((n,) + w.shape[1:]) for y, w in zip(got, wants)]


def _run(name, dev, **opts):
    c = tc.CASES[name]
    N = c['N']
    ref, routs, _ = tc.reference(name)                             # over N + 1 images
    wants = [ref.v[o][0] for o in routs]
    x = tc.make_input(name, N + 1)
    g, outs, _ = tc.plan(name, x, max_batch=N + 1, **opts)
    assert [(t, k) for _, t, k in tc.lines(g.net)] == tc.expected(name, **opts), g.net.describe()
    xt = torch.from_numpy(x).to(dev)
    for n in (N, N - 1):
        got = _outputs(g.net.run(xt[:n]), n, wants)
        for k, (y, w) in enumerate(zip(got, wants)):
            np.testing.assert_array_equal(y, w[:n], err_msg=f'{name} {opts} n={n} output {k}')
    g.net.check()


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_every_case_on_the_default_plan(name, dev):
    _run(name, dev)


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_every_case_with_all_fusions(name, dev):
    _run(name, dev, **tc.FUSE_ALL)


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_every_case_in_int32_mode(name, dev):
    _run(name, dev, table_i8=0)


@pytest.mark.parametrize('name', tc.FUSED)
def test_fused_gates_as_two_launches(name, dev):
    _run(name, dev, fuse_table=0)


# ---- an EfficientNet MBConv block, a sigmoid SE block on a ResNet-50 stage
LEGS = {'default': {}, 'all_fusions': tc.FUSE_ALL, 'int32_mode': dict(table_i8=0), 'two_launches': dict(fuse_table=0)}


@pytest.fixture(scope='module')
def mbconv_reference():
    g = tc._Graph(tc.mbconv_input(), tc.X_FL, record=False)
    out, ops = tc.mbconv_block(g, 0)
    assert np.unique(g.v[out][0]).size > 100 and all(np.unique(g.v[t][0]).size > 10 for t in ops)
    return g.v[out][0]


@pytest.mark.parametrize('leg', sorted(LEGS))
def test_efficientnet_mbconv_block(leg, mbconv_reference, dev):
    """1x1 expand + swish, depthwise 5x5 + swish, SE (pool, linear, swish, linear, sigmoid, channel gate), 1x1 project, join: the SE gate plans
    table+chmul_i8: (tc.MBCONV_TOKENS, by hand), two launches with fuse_table = 0."""
    x = tc.mbconv_input()
    g = tc._Graph(x, tc.X_FL)
    tc.mbconv_block(g, next(iter(g.v)))
    for k, v in LEGS[leg].items():
        g.net.set_option(k, v)
    g.net.finalize(2)
    assert [(t, k) for _, t, k in tc.lines(g.net)] == tc.expected_of(tc.MBCONV_TOKENS, tc.MBCONV_NOFUSE, **LEGS[leg]), g.net.describe()
    got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(mbconv_reference.shape)
    g.net.check()
    np.testing.assert_array_equal(got, mbconv_reference)


@pytest.mark.parametrize('leg', sorted(LEGS))
def test_onnx_imported_mbconv_block(leg, mbconv_reference, dev):
    """The same block written as an ONNX file (per table: requant, Add(128), Gather on a 256-entry initializer), imported, and planned through
    IntGraph.build_net."""
    from f8net_amd import onnx_export, onnx_import
    ig, g, out = tc.mbconv_int_graph()
    np.testing.assert_array_equal(g.v[out][0], mbconv_reference)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    net = back.build_net(2, input_fraclen=tc.X_FL, options=LEGS[leg])
    assert [(t, k) for _, t, k in tc.lines(net)] == tc.expected_of(tc.MBCONV_TOKENS, tc.MBCONV_NOFUSE, **LEGS[leg]), net.describe()
    got = net.run(torch.from_numpy(tc.mbconv_input()).to(dev)).cpu().numpy().reshape(mbconv_reference.shape)
    net.check()
    np.testing.assert_array_equal(got, mbconv_reference)


def test_sigmoid_se_branch_inside_a_stage_chain_on_resnet50(dev):
    """ResNet-50 at 64 x 64: stage_1_layer_1's output (512 x 8 x 8) sits in the middle of what the stage chain runs as one launch.  An SE branch with a
    sigmoid gate reads it — avgpool_sum, linear, sigmoid table, channel gate: the scaled map is output 1 — so the launch is cut there.  The logits stay
    the plain net's."""
    import dil_cases
    from f8net_amd import synth, tables, topology
    from f8net_amd.net import record_net
    from ir_cases import _b, _w
    from oracle import oracle
    name = 'stage_1_layer_1'
    spec = topology.get('resnet50')
    params = synth.make_params(spec, seed=17)
    x, x_fl = synth.make_input(spec, params, 2, 64, seed=3)
    seen = {}
    tspec, tparams = dil_cases.stuffed_twin(spec, params)
    logits = oracle.net_forward(tspec, tparams, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, (v.copy(), fl)) if k == name else None)
    assert seen[name][0].shape[1:] == (512, 8, 8)
    xt = torch.from_numpy(x).to(dev)
    for options in (None, tc.FUSE_ALL):
        net = record_net(spec, params, 64, options=options)
        g = tc._Graph(seen[name][0], seen[name][1], record=False)
        g.record, g.net = True, net
        src = net.tap_ids[name]
        g.v = {src: seen[name]}
        assert seen[name][1] == 10                                 # the map at fraclen 10, values up to 2^20: read at unsigned fraclen 0; its pool at fraclen 16
        v = g.linear(g.avgpool_sum(src), _w(71, (512, 512), 3.0), _b(72, 512, 2.0 ** 11), weight_fl=12, input_fl=0, input_signed=False, label='se.fc')
        gate = g.table(v, tables.sigmoid(4, True, 12), in_fl=4, in_signed=True, out_fl=12, label='se.gate')      # fraclen 12 read at +-8
        s = g.mul(src, gate, a_fl=0, a_signed=False, b_fl=8, label='se.scale')
        assert net.output(s, as_float=False) == 1
        for k, val in (options or {}).items():
            net.set_option(k, val)
        net.finalize(2)
        assert [(t, k) for _, t, k in tc.lines(net)] == [('table+chmul_i32:', tc.F32)], net.describe()
        want = g.v[s][0]
        assert np.unique(want).size > 100 and np.unique(g.v[gate][0]).size > 50
        got, scaled = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {options}')
        np.testing.assert_array_equal(scaled.cpu().numpy().reshape(want.shape), want, err_msg=f'scaled map {options}')


# ---- torch
def _rand(seed, shape, lo, hi, dev):
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, shape, dtype=np.int64).astype(np.int32)).to(dev)


@pytest.mark.parametrize('C, H, W, src_fl, in_fl, in_signed, kind', [
    (20, 7, 7, 13, 6, True, 'rnd'),
    (64, 9, 11, 12, 5, False, 'rnd'),
    (48, 1, 1, 9, 4, True, 'sigmoid'),
    (8, 7, 7, 5, 7, True, 'swish'),                                # a left shift by 2: 64 distinct indices
])
def test_torch_table_q_against_the_reference(C, H, W, src_fl, in_fl, in_signed, kind, dev):
    x = _rand(C * 7 + H, (3, C, H, W), -2 ** (src_fl - in_fl + 8), 2 ** (src_fl - in_fl + 8), dev)      # twice the format's range: both clamps act
    out_fl = 30 if kind == 'rnd' else 10
    table = (np.random.default_rng(C).integers(-2 ** 31, 2 ** 31, 256, dtype=np.int64).astype(np.int32) if kind == 'rnd'
             else getattr(tables, kind)(in_fl, in_signed, out_fl))
    want = tc.table_ref(x.cpu().numpy(), src_fl, table, in_fl=in_fl, in_signed=in_signed)
    got = torch.ops.f8net.table_q(x, torch.from_numpy(table), src_fl, in_fl, in_signed, out_fl)
    assert got.dtype == torch.int32 and got.shape == x.shape and np.unique(want).size > (50 if kind == 'rnd' else 10)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.ops.f8net.table_q(x.to('meta'), torch.from_numpy(table).to('meta'), src_fl, in_fl, in_signed, out_fl).shape == x.shape


def test_sigmoid_and_swish_modules(dev):
    fl = 11
    x = _rand(5, (3, 48, 7, 7), -9 * 2 ** fl, 9 * 2 ** fl, dev)
    x.output_fraclen = fl
    for mod, table, out_fl in ((ops.F8Sigmoid(4, True, 12).to(dev), tables.sigmoid(4, True, 12), 12), (ops.F8Swish(4, True, 8).to(dev), tables.swish(4, True, 8), 8),
                               (ops.F8Table(tables.tanh(5, True, 7), 5, True, 7).to(dev), tables.tanh(5, True, 7), 7)):
        y = mod(x)
        want = tc.table_ref(x.cpu().numpy(), fl, table, in_fl=mod.in_fl, in_signed=True)
        np.testing.assert_array_equal(y.cpu().numpy(), want)
        assert y.output_fraclen == out_fl and np.unique(want).size > 50
