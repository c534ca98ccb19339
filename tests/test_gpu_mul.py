"""The fixed-point multiply and the hard gate on the device, bit for bit against the reference of tests/mul_cases.py (oracle.requant on each operand,
the product in numpy int64; np.clip + offset for the gate): every case on the default plan, with every fusing pass on, and — the cases whose gate runs
inside the mul launch — as two launches (fuse_hgate = 0), each at N and N - 1 images from one handle planned for N + 1; bench.py's pipelined schedule
on two cases; torch.ops.f8net.mul_q / F8HardSwish / F8ChannelGate against the same reference.
tests/test_mul_plan.py checks on the CPU which tokens and kernel instances every case plans."""
import numpy as np
import pytest
import torch

import mul_cases as mc
import ref_ops
from f8net_amd import ops  # (registers torch.ops.f8net)
from graph_cases import run_case, se_branch_on_resnet50_stage
from ir_cases import _b, _w
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    assert [(t, k) for _, t, k in mc.lines(net)] == mc.expected(name, **opts), net.describe()


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_every_case_on_the_default_plan(name, dev):
    run_case(mc, name, dev, _check_plan)


@pytest.mark.parametrize('name', sorted(mc.CASES))
def test_every_case_with_all_fusions(name, dev):
    run_case(mc, name, dev, _check_plan, **mc.FUSE_ALL)


@pytest.mark.parametrize('name', mc.FUSED)
def test_fused_gates_as_two_launches(name, dev):
    run_case(mc, name, dev, _check_plan, fuse_hgate=0)


@pytest.mark.parametrize('name', ['se_20', 'hsw_64'])
def test_pipelined_schedule(name, dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    c = mc.CASES[name]
    N = c['N']
    xs = [mc.make_input(name, N + 1)[:N]] + [mc.make_input(name, N + 1)[::-1][:N].copy(), np.roll(mc.make_input(name, N), 1, axis=2).copy()]
    g, outs, _ = mc.plan(name, xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    ref, routs, _ = mc.reference(name)
    wants = [ref.v[routs[0]][0][:N]]
    for x in xs[1:]:
        gi, oi, _ = mc.build_graph(name, x, record=False)
        wants.append(gi.v[oi[0]][0])
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    bufs = [torch.empty((N, wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=bufs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(bufs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    g.net.check()


# ---- the two small nets, the ONNX-imported SE graph, an SE block on a ResNet-50 stage
LEGS = {'default': {}, 'all_fusions': mc.FUSE_ALL, 'two_launches': dict(fuse_hgate=0)}


@pytest.fixture(scope='module')
def mbv3_reference():
    g = RefGraph(mc.mbv3_input(), mc.X_FL, record=False)
    out, ops = mc.mbv3_block(g, 0)
    assert np.unique(g.v[out][0]).size > 100 and all(np.unique(g.v[t][0]).size > 20 for t in ops)
    return g.v[out][0]


@pytest.mark.parametrize('leg', sorted(LEGS))
def test_mobilenet_v3_block(leg, mbv3_reference, dev):
    """1x1 expand + hard-swish, depthwise 5x5 + hard-swish, SE with a hard-sigmoid gate, 1x1 project, join: three fused gate launches by hand
    (mc.MBV3_TOKENS), six launches with fuse_hgate = 0."""
    x = mc.mbv3_input()
    g = RefGraph(x, mc.X_FL)
    mc.mbv3_block(g, next(iter(g.v)))
    for k, v in LEGS[leg].items():
        g.net.set_option(k, v)
    g.net.finalize(2)
    assert [(t, k) for _, t, k in mc.lines(g.net)] == (mc.MBV3_NOFUSE if leg == 'two_launches' else mc.MBV3_TOKENS), g.net.describe()
    got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(mbv3_reference.shape)
    g.net.check()
    np.testing.assert_array_equal(got, mbv3_reference)


@pytest.mark.parametrize('leg', sorted(LEGS))
def test_onnx_imported_se_net(leg, dev):
    """The SE graph written as an ONNX file (requant, Unsqueeze, Mul, Relu, Clip, Add), imported, and planned through IntGraph.build_net."""
    from f8net_amd import onnx_export, onnx_import
    ig, g, out = mc.se_int_graph()
    want = g.v[out][0]
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    net = back.build_net(3, input_fraclen=mc.X_FL, options=LEGS[leg])
    if leg != 'two_launches':
        assert [(t, k) for _, t, k in mc.lines(net)] == mc.SE_TOKENS, net.describe()
    got = net.run(torch.from_numpy(mc.se_input()).to(dev)).cpu().numpy().reshape(want.shape)
    net.check()
    np.testing.assert_array_equal(got, want)


def test_se_scale_of_a_block_output_inside_a_stage_chain_on_resnet50(dev):
    """ResNet-50 at 64 x 64: stage_1_layer_1's output (512 x 8 x 8) sits in the middle of what the stage chain runs as one launch.  An SE branch with a
    hard-sigmoid gate reads it — avgpool_sum, linear, hard gate, channel gate: the scaled map is output 1 — so the launch is cut there.  The logits
    stay the plain net's."""
    def branch(g, src):                                            # the map is read at unsigned fraclen 0; its pool is at fraclen 16
        v = g.linear(g.avgpool_sum(src), _w(71, (512, 512), 3.0), _b(72, 512, 2.0 ** 11), weight_fl=12, input_fl=0, input_signed=False, label='se.fc')
        assert np.unique(g.v[v][0]).size > 100
        return g.mul(src, g.hard_gate(v), a_fl=0, a_signed=False, b_fl=5, label='se.scale')
    se_branch_on_resnet50_stage(dev, branch, ('hgate+chmul_i32:', mc.W11), lines=mc.lines)


# ---- torch
def _rand(seed, shape, lo, hi, dev):
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, shape, dtype=np.int64).astype(np.int32)).to(dev)


@pytest.mark.parametrize('C, H, W, bcast, gate, a, b, relu', [
    (20, 7, 7, False, False, (4, True), (3, False), True),
    (64, 9, 11, False, False, (6, False), (6, True), False),
    (48, 7, 7, True, False, (4, True), (5, False), False),
    (64, 7, 7, True, True, (4, False), (5, False), False),
    (20, 9, 11, True, True, (4, True), (5, False), True),
    (20, 7, 7, False, True, (4, True), (5, False), False),
])
def test_torch_mul_q_against_the_reference(C, H, W, bcast, gate, a, b, relu, dev):
    fa, fb = 13, 12
    xa = _rand(C * 7 + H, (3, C, H, W), -2 ** 16, 2 ** 16, dev)
    xb = _rand(C * 11 + W, (3, C, 1, 1) if bcast else (3, C, H, W), -2 ** 15, 2 ** 15, dev)
    b_ref = ref_ops.hard_gate_ref(xb.cpu().numpy(), fb) if gate else xb.cpu().numpy()
    want, fl = ref_ops.mul_ref(xa.cpu().numpy(), fa, b_ref, fb, a_fl=a[0], a_signed=a[1], b_fl=b[0], b_signed=b[1], relu=relu)
    got = torch.ops.f8net.mul_q(xa, xb, fa, fb, a[0], a[1], b[0], b[1], gate, relu)
    assert got.dtype == torch.int32 and got.shape == xa.shape and np.unique(want).size > 50
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.ops.f8net.mul_q(xa.to('meta'), xb.to('meta'), fa, fb, a[0], a[1], b[0], b[1], gate, relu).shape == xa.shape


def test_hard_swish_and_channel_gate_modules(dev):
    fl = 11
    x = _rand(5, (3, 48, 7, 7), -6 * 2 ** fl, 6 * 2 ** fl, dev)
    x.output_fraclen = fl
    y = ops.F8HardSwish(x_fl=4, x_signed=True, g_fl=5)(x)
    want, out_fl = ref_ops.mul_ref(x.cpu().numpy(), fl, ref_ops.hard_gate_ref(x.cpu().numpy(), fl), fl, a_fl=4, a_signed=True, b_fl=5, b_signed=False)
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    assert y.output_fraclen == out_fl == 9
    s = _rand(6, (3, 48), -5 * 2 ** 9, 5 * 2 ** 9, dev)
    s.output_fraclen = 9
    z = ops.F8ChannelGate(x_fl=4, x_signed=True, g_fl=5)(x, s)
    gate = ref_ops.hard_gate_ref(s.cpu().numpy().reshape(3, 48, 1, 1), 9)
    want, out_fl = ref_ops.mul_ref(x.cpu().numpy(), fl, gate, 9, a_fl=4, a_signed=True, b_fl=5, b_signed=False)
    np.testing.assert_array_equal(z.cpu().numpy(), want)
    assert z.output_fraclen == out_fl
