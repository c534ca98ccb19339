"""Depth-to-space and space-to-depth on the device, bit for bit against the reference of tests/pixmap_cases.py (numpy reshape / transpose on the graph
builder's int32 tensors): every case on both legs — option pixmap_i8 = 1 (bytes moved where the plan allows it) and 0 (the int32 launch everywhere) —
at N and N - 1 images from one handle planned for N + 1, and with every fusing pass on; bench.py's pipelined schedule on two cases; an ESPCN tail, an
EDSR upsampler, a TResNet stem and a DUC head in front of an argmax output; the ESPCN tail imported from ONNX; torch.ops.f8net.depth_to_space /
space_to_depth and F8PixelShuffle / F8PixelUnshuffle against torch.nn.functional.pixel_shuffle / pixel_unshuffle.
tests/test_pixmap_plan.py checks on the CPU which tokens and kernel instances every case plans."""
import numpy as np
import pytest
import torch

import pixmap_cases as pm
from chanmap_cases import _cv
from f8net_amd import onnx_export, onnx_import, ops
from graph_cases import run_case
from ir_cases import _b, _w
from refgraph import RefGraph, record_int_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    assert [(t, k) for _, t, k in pm.lines(net)] == pm.expected(name, **opts), net.describe()


@pytest.mark.parametrize('i8', [1, 0])
@pytest.mark.parametrize('name', sorted(pm.CASES))
def test_every_case_on_both_legs(name, i8, dev):
    run_case(pm, name, dev, _check_plan, pixmap_i8=i8)


@pytest.mark.parametrize('name', sorted(pm.CASES))
def test_every_case_with_all_fusions(name, dev):
    run_case(pm, name, dev, _check_plan, **pm.FUSE_ALL)


@pytest.mark.parametrize('name', ['d2s2_crd_20', 's2d2_dcr_19'])
def test_pipelined_schedule(name, dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    c = pm.CASES[name]
    N = c['N']
    xs = [pm.make_input(name, N + 1)[:N]] + [pm.make_input(name, N + 1)[::-1][:N].copy(), np.roll(pm.make_input(name, N), 1, axis=2).copy()]
    g, outs, _ = pm.plan(name, xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    ref, routs, _ = pm.reference(name)
    wants = [ref.v[routs[0]][0][:N]]
    for x in xs[1:]:
        gi, oi, _ = pm.build_graph(name, x, record=False)
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


@pytest.mark.parametrize('name', ['d2s2_dcr_48', 'd2s8_crd_19', 's2d2_crd_12'])
def test_profiled_run_times_the_launch(name, dev):
    x = pm.make_input(name)
    g, outs, _ = pm.plan(name, x)
    xt = torch.from_numpy(x).to(dev)
    y = g.net.run(xt)
    y2, ms = g.net.run_profiled(xt)
    assert torch.equal(y, y2) and len(ms) == g.net.num_launches
    (i, _, _), = pm.lines(g.net)
    assert ms[i] > 0.0
    g.net.check()


# ---- small nets
def _input(tag, n, cin, H, W):
    return pm.synth.rand_uniform_int(5, f'pmnet{tag}', (n, cin, H, W), 0, 255).astype(np.int32)


def espcn_tail(g, x0):
    """conv 3x3 to 32 -> conv 3x3 to 27 -> pixel_shuffle 3: the int32 output [3, 3 H, 3 W]."""
    t = _cv(g, x0, 0, 32, 9, kernel=3, relu=True, in_fl=pm.X_FL, in_signed=False, quant_input=False)           # fraclen 13
    t = _cv(g, t, 1, 27, 5, kernel=3, relu=False, in_fl=4, in_signed=False)                                     # 9
    s = pm.d2s(g, t, 3, 'crd', label='sr')
    g.output(s)
    return s


def edsr_upsampler(g, x0):
    """Twice: conv 3x3 to 4 x 16 -> pixel_shuffle 2; then a 3x3 conv to 3 channels.  Each shuffle's only reader is a conv: the transposer moves bytes."""
    t = _cv(g, x0, 0, 16, 9, relu=True, in_fl=pm.X_FL, in_signed=False, quant_input=False)                      # fraclen 13
    shuffles = []
    for k in (1, 2):
        t = _cv(g, t, k, 64, 5, kernel=3, relu=True, in_fl=4, in_signed=False)                                  # 9
        t = pm.d2s(g, t, 2, 'crd', label=f'up{k}')
        shuffles.append(t)
        t = _cv(g, t, k + 2, 16, 5, kernel=3, relu=True, in_fl=4, in_signed=False)                              # 9
    out = _cv(g, t, 5, 3, 5, kernel=3, relu=False, in_fl=4, in_signed=False)
    g.output(out)
    return out, shuffles


def tresnet_stem(g, x0):
    """input (3 channels, 16 x 16) -> space_to_depth 4 in DCR order (48 x 4 x 4) -> conv 3x3 to 64 -> avgpool -> linear to 10."""
    s = pm.s2d(g, x0, 4, 'dcr', label='stem')
    t = _cv(g, s, 0, 64, 9, kernel=3, relu=True, in_fl=pm.X_FL, in_signed=False, quant_input=False)             # fraclen 13
    p = g.avgpool_sum(t)
    out = g.linear(p, _w(600, (10, 64), 8.0), _b(601, 10, 100.0), weight_fl=5, input_fl=4, input_signed=False, label='fc')
    g.output(out)
    return out, s


@pytest.mark.parametrize('leg', ['i8', 'i32', 'all_fusions'])
def test_espcn_tail(leg, dev):
    x = _input('espcn', 2, 8, 6, 5)
    g = RefGraph(x, pm.X_FL)
    s = espcn_tail(g, next(iter(g.v)))
    for k, v in {'i8': {}, 'i32': dict(pixmap_i8=0), 'all_fusions': pm.FUSE_ALL}[leg].items():
        g.net.set_option(k, v)
    g.net.finalize(2)
    assert [(t, k) for _, t, k in pm.lines(g.net)] == [('d2s3crd_i32:', pm.K32)], g.net.describe()        # the network output: int32 on every leg
    want = g.v[s][0]
    assert want.shape == (2, 3, 18, 15) and np.unique(want).size > 100
    got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
    g.net.check()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('leg', ['i8', 'i32', 'all_fusions'])
def test_edsr_upsampler(leg, dev):
    x = _input('edsr', 2, 8, 5, 3)
    g = RefGraph(x, pm.X_FL)
    out, shuffles = edsr_upsampler(g, next(iter(g.v)))
    for k, v in {'i8': {}, 'i32': dict(pixmap_i8=0), 'all_fusions': pm.FUSE_ALL}[leg].items():
        g.net.set_option(k, v)
    g.net.finalize(2)
    exp = [('d2s2crd_i32:', pm.K32)] * 2 if leg == 'i32' else [('d2s2crd_i8:', pm.TD)] * 2
    assert [(t, k) for _, t, k in pm.lines(g.net)] == exp, g.net.describe()
    want = g.v[out][0]
    assert want.shape == (2, 3, 20, 12) and np.unique(want).size > 100 and all(np.unique(g.v[s][0]).size > 50 for s in shuffles)
    got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
    g.net.check()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('leg', ['i8', 'i32', 'all_fusions'])
def test_tresnet_stem(leg, dev):
    x = _input('tresnet', 2, 3, 16, 16)
    g = RefGraph(x, pm.X_FL)
    out, s = tresnet_stem(g, next(iter(g.v)))
    for k, v in {'i8': {}, 'i32': dict(pixmap_i8=0), 'all_fusions': pm.FUSE_ALL}[leg].items():
        g.net.set_option(k, v)
    g.net.finalize(2)
    exp = [('s2d4dcr_i32:', pm.K32)] if leg == 'i32' else [('s2d4dcr_i8:', pm.GEN)]
    assert [(t, k) for _, t, k in pm.lines(g.net)] == exp, g.net.describe()
    want = g.v[out][0]
    assert g.v[s][0].shape == (2, 48, 4, 4) and np.unique(want).size > 10
    got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
    g.net.check()
    np.testing.assert_array_equal(got, want)


def test_duc_head_in_front_of_an_argmax_output(dev):
    """Dense Upsampling Convolution: a 1x1 conv to 19 x 64 channels on a 2 x 3 map, depth_to_space 8, the class map [16, 24] as the output."""
    from argmax_cases import argmax_ref
    name = 'd2s8_crd_19'
    x = pm.make_input(name)
    g = RefGraph(x, pm.X_FL)
    s = pm.d2s(g, pm._source(g, next(iter(g.v)), pm.CASES[name]), 8, 'crd', label='duc')
    g.net.output_argmax(s, 'u8')
    g.net.finalize(3)
    assert [(t, k) for _, t, k in pm.lines(g.net)] == [('d2s8crd_i32:', pm.K32)], g.net.describe()        # the argmax launch reads int32
    want = argmax_ref(g.v[s][0])
    assert want.shape == (3, 16, 24) and np.unique(want).size >= 5
    got = g.net.run(torch.from_numpy(x).to(dev))
    g.net.check()
    assert got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy().reshape(want.shape), want)


def test_onnx_imported_espcn_tail(dev):
    """The tail written as an ONNX file (DepthToSpace, mode CRD), imported, and planned through IntGraph.build_net."""
    x = _input('espcn', 2, 8, 6, 5)
    ig, g, out = record_int_graph(x, pm.X_FL, espcn_tail)
    ig.output_float = False
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert [(o.kind, o.block, o.order) for o in back.ops if o.kind == 'd2s'] == [('d2s', 3, 'crd')]
    net = back.build_net(2, input_fraclen=pm.X_FL)
    assert [(t, k) for _, t, k in pm.lines(net)] == [('d2s3crd_i32:', pm.K32)], net.describe()
    want = g.v[out][0]
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
    net.check()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('r, C, H, W', [(2, 19, 5, 3), (3, 3, 6, 5), (4, 16, 1, 1)])
def test_torch_ops_and_modules_against_torch(r, C, H, W, dev):
    """Full-range int32 data; C is the channel count of the small side."""
    F = torch.nn.functional
    rng = np.random.default_rng(r * 1000 + C)
    deep = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (3, C * r * r, H, W), dtype=np.int64).astype(np.int32)).to(dev)
    wide = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (3, C, H * r, W * r), dtype=np.int64).astype(np.int32)).to(dev)
    up, down = F.pixel_shuffle(deep.cpu(), r), F.pixel_unshuffle(wide.cpu(), r)
    got = torch.ops.f8net.depth_to_space(deep, r, 'crd')
    assert got.dtype == torch.int32 and got.shape == up.shape and torch.equal(got.cpu(), up)
    got = torch.ops.f8net.space_to_depth(wide, r, 'crd')
    assert got.dtype == torch.int32 and got.shape == down.shape and torch.equal(got.cpu(), down)
    for order in ('crd', 'dcr'):                                   # each order's pair is a round trip, and DCR is the numpy definition
        y = torch.ops.f8net.depth_to_space(deep, r, order)
        np.testing.assert_array_equal(y.cpu().numpy(), pm.d2s_ref(deep.cpu().numpy(), r, order))
        assert torch.equal(torch.ops.f8net.space_to_depth(y, r, order), deep)
    deep.output_fraclen = 5
    y = ops.F8PixelShuffle(r)(deep)
    assert torch.equal(y.cpu(), up) and y.output_fraclen == 5
    wide.output_fraclen = 7
    y = ops.F8PixelUnshuffle(r)(wide)
    assert torch.equal(y.cpu(), down) and y.output_fraclen == 7
    assert torch.ops.f8net.depth_to_space(deep.to('meta'), r, 'crd').shape == up.shape
    assert torch.ops.f8net.space_to_depth(wide.to('meta'), r, 'dcr').shape == down.shape
