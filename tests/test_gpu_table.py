"""The 256-entry table op on the device, bit for bit against the reference of tests/table_cases.py (table[oracle.requant(x) + offset] in numpy):
every case on the default plan, with every fusing pass on, with table_i8 = 0 and with fuse_table = 0, each at N and N - 1 images from one handle
planned for N + 1; an EfficientNet MBConv block, recorded and imported from ONNX; a sigmoid SE branch inside ResNet-50's stage chain;
torch.ops.f8net.table_q / F8Table / F8Sigmoid / F8Swish against the same reference.
tests/test_table_plan.py checks on the CPU which tokens and kernel instances every case plans."""
import numpy as np
import pytest
import torch

import ref_ops
import table_cases as tc
from f8net_amd import ops, tables  # (ops registers torch.ops.f8net)
from graph_cases import run_case, se_branch_on_resnet50_stage
from ir_cases import _b, _w
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    assert [(t, k) for _, t, k in tc.lines(net)] == tc.expected(name, **opts), net.describe()


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_every_case_on_the_default_plan(name, dev):
    run_case(tc, name, dev, _check_plan)


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_every_case_with_all_fusions(name, dev):
    run_case(tc, name, dev, _check_plan, **tc.FUSE_ALL)


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_every_case_in_int32_mode(name, dev):
    run_case(tc, name, dev, _check_plan, table_i8=0)


@pytest.mark.parametrize('name', tc.FUSED)
def test_fused_gates_as_two_launches(name, dev):
    run_case(tc, name, dev, _check_plan, fuse_table=0)


# ---- an EfficientNet MBConv block, a sigmoid SE block on a ResNet-50 stage
LEGS = {'default': {}, 'all_fusions': tc.FUSE_ALL, 'int32_mode': dict(table_i8=0), 'two_launches': dict(fuse_table=0)}


@pytest.fixture(scope='module')
def mbconv_reference():
    g = RefGraph(tc.mbconv_input(), tc.X_FL, record=False)
    out, ops = tc.mbconv_block(g, 0)
    assert np.unique(g.v[out][0]).size > 100 and all(np.unique(g.v[t][0]).size > 10 for t in ops)
    return g.v[out][0]


@pytest.mark.parametrize('leg', sorted(LEGS))
def test_efficientnet_mbconv_block(leg, mbconv_reference, dev):
    """1x1 expand + swish, depthwise 5x5 + swish, SE (pool, linear, swish, linear, sigmoid, channel gate), 1x1 project, join: the SE gate plans
    table+chmul_i8: (tc.MBCONV_TOKENS, by hand), two launches with fuse_table = 0."""
    x = tc.mbconv_input()
    g = RefGraph(x, tc.X_FL)
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
    def branch(g, src):                                            # the map is read at unsigned fraclen 0; its pool is at fraclen 16
        v = g.linear(g.avgpool_sum(src), _w(71, (512, 512), 3.0), _b(72, 512, 2.0 ** 11), weight_fl=12, input_fl=0, input_signed=False, label='se.fc')
        gate = g.table(v, tables.sigmoid(4, True, 12), in_fl=4, in_signed=True, out_fl=12, label='se.gate')      # fraclen 12 read at +-8
        assert np.unique(g.v[gate][0]).size > 50
        return g.mul(src, gate, a_fl=0, a_signed=False, b_fl=8, label='se.scale')
    se_branch_on_resnet50_stage(dev, branch, ('table+chmul_i32:', tc.F32), lines=tc.lines)


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
    want = ref_ops.table_ref(x.cpu().numpy(), src_fl, table, in_fl=in_fl, in_signed=in_signed)
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
        want = ref_ops.table_ref(x.cpu().numpy(), fl, table, in_fl=mod.in_fl, in_signed=True)
        np.testing.assert_array_equal(y.cpu().numpy(), want)
        assert y.output_fraclen == out_fl and np.unique(want).size > 50
