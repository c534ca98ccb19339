"""Channel slice and channel shuffle on the device, bit for bit against the reference of tests/chanmap_cases.py (numpy fancy indexing on the graph
builder's int32 tensors): every case on both legs — option chanmap_i8 = 1 (bytes moved where the plan allows it, a concat in front of a shuffle read by
the shuffle launch itself) and 0 (the int32 launch everywhere) — at N and N - 1 images from one handle planned for N + 1, with every fusing pass on,
and the fused cases as two launches (fuse_shuffle = 0); bench.py's pipelined schedule on two cases; a ShuffleNet-V2 stage, also imported from ONNX;
torch.ops.f8net.channel_shuffle / F8ChannelShuffle against torch.nn.functional.channel_shuffle.
tests/test_chanmap_plan.py checks on the CPU which tokens and kernel instances every case plans."""
import numpy as np
import pytest
import torch

import chanmap_cases as cm
from f8net_amd import onnx_export, onnx_import, ops
from graph_cases import run_case
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    assert [(t, k) for _, t, k in cm.lines(net)] == cm.expected(name, **opts), net.describe()


@pytest.mark.parametrize('i8', [1, 0])
@pytest.mark.parametrize('name', sorted(cm.CASES))
def test_every_case_on_both_legs(name, i8, dev):
    run_case(cm, name, dev, _check_plan, chanmap_i8=i8)


@pytest.mark.parametrize('name', sorted(cm.CASES))
def test_every_case_with_all_fusions(name, dev):
    run_case(cm, name, dev, _check_plan, **cm.FUSE_ALL)


@pytest.mark.parametrize('name', cm.FUSED)
def test_fused_cases_as_two_launches(name, dev):
    run_case(cm, name, dev, _check_plan, fuse_shuffle=0)


@pytest.mark.parametrize('name', ['f_58_gap', 'sl_49_15'])
def test_pipelined_schedule(name, dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    c = cm.CASES[name]
    N = c['N']
    xs = [cm.make_input(name, N + 1)[:N]] + [cm.make_input(name, N + 1)[::-1][:N].copy(), np.roll(cm.make_input(name, N), 1, axis=2).copy()]
    g, outs, _ = cm.plan(name, xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    ref, routs, _ = cm.reference(name)
    wants = [ref.v[routs[0]][0][:N]]
    for x in xs[1:]:
        gi, oi, _ = cm.build_graph(name, x, record=False)
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


@pytest.mark.parametrize('name', ['sh2_352', 'sl_17_30', 'f_32'])
def test_profiled_run_times_the_launch(name, dev):
    x = cm.make_input(name)
    g, outs, _ = cm.plan(name, x)
    xt = torch.from_numpy(x).to(dev)
    y = g.net.run(xt)
    y2, ms = g.net.run_profiled(xt)
    assert torch.equal(y, y2) and len(ms) == g.net.num_launches
    (i, _, _), = cm.lines(g.net)
    assert ms[i] > 0.0
    g.net.check()


STAGE_FUSED = [('concat+shuffle2_i8:', cm.S2)]
STAGE_SPLIT = [('slice_i8:', cm.LT), ('slice_i8:', cm.LF)]                    # channels [0, 58) and [58, 116)
STAGE_I8 = STAGE_FUSED + (STAGE_SPLIT + STAGE_FUSED) * 2
STAGE_I32 = [('concat_i32:', cm.C32), ('shuffle2_i32:', cm.K32)] + ([('slice_i32:', cm.K32)] * 2 + [('concat_i32:', cm.C32), ('shuffle2_i32:', cm.K32)]) * 2


@pytest.fixture(scope='module')
def stage_reference():
    g = RefGraph(cm.stage_input(), cm.X_FL, record=False)
    out, shuffles = cm.shufflenet_stage(g, 0)
    assert np.unique(g.v[out][0]).size > 10 and all(np.unique(g.v[s][0]).size > 100 for s in shuffles)
    return g.v[out][0]


@pytest.mark.parametrize('leg', ['i8', 'i32', 'all_fusions'])
def test_shufflenet_v2_stage(leg, stage_reference, dev):
    """Every unit of the stage plans one concat+shuffle2_i8: launch (by hand: operands of 58 channels at offset 0 — the V = 2 instance)."""
    x = cm.stage_input()
    g = RefGraph(x, cm.X_FL)
    out, _ = cm.shufflenet_stage(g, next(iter(g.v)))
    for k, v in {'i8': {}, 'i32': dict(chanmap_i8=0), 'all_fusions': cm.FUSE_ALL}[leg].items():
        g.net.set_option(k, v)
    g.net.finalize(2)
    assert [(t, k) for _, t, k in cm.lines(g.net)] == (STAGE_I32 if leg == 'i32' else STAGE_I8), g.net.describe()
    got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(stage_reference.shape)
    g.net.check()
    np.testing.assert_array_equal(got, stage_reference)


def test_onnx_imported_shufflenet_v2_stage(stage_reference, dev):
    """The stage written as an ONNX file (Slice, Reshape / Transpose / Reshape), imported, and planned through IntGraph.build_net."""
    ig, g, out = cm.stage_int_graph()
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    net = back.build_net(2, input_fraclen=cm.X_FL)
    assert [(t, k) for _, t, k in cm.lines(net)] == STAGE_I8, net.describe()
    got = net.run(torch.from_numpy(cm.stage_input()).to(dev)).cpu().numpy().reshape(stage_reference.shape)
    net.check()
    np.testing.assert_array_equal(got, stage_reference)


@pytest.mark.parametrize('groups, C, H, W', [(2, 116, 7, 7), (3, 24, 9, 11), (8, 256, 1, 1)])
def test_torch_op_and_module_against_torch(groups, C, H, W, dev):
    x = torch.from_numpy(np.random.default_rng(groups * 1000 + C).integers(-2 ** 31, 2 ** 31, (3, C, H, W), dtype=np.int64).astype(np.int32)).to(dev)
    want = torch.nn.functional.channel_shuffle(x.cpu(), groups)
    got = torch.ops.f8net.channel_shuffle(x, groups)
    assert got.dtype == torch.int32 and got.shape == x.shape
    assert torch.equal(got.cpu(), want)
    x.output_fraclen = 5
    y = ops.F8ChannelShuffle(groups)(x)
    assert torch.equal(y.cpu(), want) and y.output_fraclen == 5
    assert torch.ops.f8net.channel_shuffle(x.to('meta'), groups).shape == x.shape
