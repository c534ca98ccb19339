"""Dilated convolutions on the device, bit for bit against the zero-stuffed reference of tests/dil_cases.py (the CPU oracle on the (2d + 1)-square kernel):
every plain case on conv_igemm_kernel, every depthwise case on dwconv3x3_dil_dot4_kernel and — `dwk_dot4 = 0` — on dwconvk_kernel, the two legs against
each other; igemm_tile 1 .. 4; one handle at several batch sizes; bench.py's pipelined schedule; a tap on a dilated result and the profiled run; the
op-level drop-in; an IntGraph with a dilated conv; resnet50_os16 and mobilenet_v2_os16 through build_net with taps, default plan and all fusions.
tests/test_dilated_plan.py checks on the CPU that every case is live on the reference's values."""
import numpy as np
import pytest
import torch

import dil_cases
from f8net_amd import onnx_export, synth, topology
from f8net_amd.net import build_net
from oracle import oracle
from ref_ops import stuffed
from refgraph import graph_forward

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _run(name, case, dev, batches=None, dot4=True, tile=None, **opts):
    """Plans the case, checks its dilated launches against the hand-written table and every batch against the shared reference; returns the last output."""
    n_max = case.get('max_batch') or case['N']
    x = dil_cases.make_input(name, case, n_max)
    g, out, _ = dil_cases.plan(name, case, x, **opts)
    assert dil_cases.d_lines(g.net) == dil_cases.expect(case, dot4=dot4, tile=tile), g.net.describe()
    ref, rout, _ = dil_cases.reference(name)
    want = ref.v[rout][0]
    xt = torch.from_numpy(x).to(dev)
    got = None
    for n in batches or [n_max]:
        got = g.net.run(xt[:n]).cpu().numpy().reshape((n,) + want.shape[1:])
        np.testing.assert_array_equal(got, want[:n], err_msg=f'{name} {opts} n={n}')
    g.net.check()
    return got


@pytest.mark.parametrize('name', sorted(dil_cases.PLAIN))
def test_plain_geometry(name, dev):
    _run(name, dil_cases.PLAIN[name], dev)


@pytest.mark.parametrize('name', sorted(dil_cases.PLAIN_FORMATS))
def test_plain_formats(name, dev):
    _run(name, dil_cases.PLAIN_FORMATS[name], dev)


@pytest.mark.parametrize('name', sorted(dil_cases.PLAIN_RES))
def test_plain_with_the_fused_residual_join(name, dev):
    _run(name, dil_cases.PLAIN_RES[name], dev)


@pytest.mark.parametrize('tile', sorted(dil_cases.TILES))
def test_every_igemm_tile(tile, dev):
    _run(dil_cases.TILE_CASE, dil_cases.ALL[dil_cases.TILE_CASE], dev, tile=dil_cases.TILES[tile], igemm_tile=tile)


@pytest.mark.parametrize('name', sorted(dil_cases.DW))
def test_depthwise_on_both_kernels(name, dev):
    """The dot4 kernel, then the generic kernel (dwk_dot4 = 0) on the same graph and input; both against the reference, hence against each other."""
    a = _run(name, dil_cases.DW[name], dev)
    b = _run(name, dil_cases.DW[name], dev, dot4=False, dwk_dot4=0)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('name', sorted(dil_cases.DW_GENERIC))
def test_depthwise_stride_2_and_the_int32_form_run_the_generic_kernel(name, dev):
    case = dil_cases.DW_GENERIC[name]
    assert all(k.startswith('f8::dwconvk_kernel<') for _, k in dil_cases.expect(case))      # (asserted by symbol against the plan in _run)
    _run(name, case, dev)


@pytest.mark.parametrize('name', sorted(dil_cases.GROUPED))
@pytest.mark.parametrize('grouped', [1, 2])
def test_grouped_is_the_dense_expansion(name, grouped, dev):
    _run(name, dil_cases.GROUPED[name], dev, grouped=grouped)


@pytest.mark.parametrize('name', sorted(dil_cases.MAX_BATCH))
def test_fewer_images_than_max_batch(name, dev):
    """Planned for 8 images; 3 images (sub-batches of 2 and 1), then 8 from the same handle."""
    _run(name, dil_cases.MAX_BATCH[name], dev, batches=[3, 8])


@pytest.mark.parametrize('name', sorted(dil_cases.PIPELINED))
def test_pipelined_schedule(name, dev):
    """bench.py's schedule on dilated conv d2 -> dilated conv d4: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three
    inputs rotating over nine runs; every output against the reference."""
    case = dil_cases.PIPELINED[name]
    xs = [dil_cases.make_input(name, case)] + [dil_cases.make_input(f'{name}{i}', case) for i in (1, 2)]
    g, out, _ = dil_cases.plan(name, case, xs[0])
    assert dil_cases.d_lines(g.net) == dil_cases.expect(case), g.net.describe()
    ref, rout, _ = dil_cases.reference(name)
    wants = [ref.v[rout][0]]
    for x in xs[1:]:
        gi, oi, _ = dil_cases.build_graph(case, x, record=False)
        wants.append(gi.v[oi][0])
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=outs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(outs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    g.net.check()


@pytest.mark.parametrize('name', ['p_9x11_d2_pad2_s2', 'd_c40_9x11_d3_pad3'])
def test_tap_on_the_dilated_result_and_the_profiled_run(name, dev):
    """f8_net_output on the dilated conv's own tensor (the launch then writes int32 next to its int8 form) and f8_net_run_profiled."""
    case = dil_cases.ALL[name]
    x = dil_cases.make_input(name, case)
    g, out, ids = dil_cases.build_graph(case, x)
    assert g.net.output(ids[0], as_float=False) == 1
    g.net.finalize(3)
    xt = torch.from_numpy(x).to(dev)
    y, tap = g.net.run(xt)
    np.testing.assert_array_equal(y.cpu().numpy().reshape(g.v[out][0].shape), g.v[out][0])
    np.testing.assert_array_equal(tap.cpu().numpy(), g.v[ids[0]][0])
    (y2, tap2), ms = g.net.run_profiled(xt)
    assert torch.equal(y2, y) and torch.equal(tap2, tap)
    assert len(ms) == g.net.num_launches and all(m >= 0.0 for m in ms)
    g.net.check()


@pytest.mark.parametrize('C, G, stride, d, pad', [(40, 1, 1, 2, 2), (64, 1, 2, 3, 1), (40, 40, 1, 2, 2), (32, 32, 2, 4, 4)])
def test_op_level_conv2d(dev, C, G, stride, d, pad):
    """F8Conv2d(dilation=) / torch.ops.f8net.conv2d on int32 NCHW device tensors; the meta function gives the same shape."""
    from f8net_amd import ops
    N, H, W = 3, 9, 11
    x = synth.rand_uniform_int(11, f'dop_x{C}', (N, C, H, W), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(12, f'dop_w{C}{G}', (C, C // G, 3, 3), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(13, f'dop_b{C}', (C,), 3e5).astype(np.int32)
    conv = ops.F8Conv2d(C, C, 3, stride=stride, padding=pad, groups=G, dilation=d)
    conv.weight.data, conv.bias.data = torch.from_numpy(w), torch.from_numpy(b)
    conv.input_fraclen.fill_(5)
    conv.weight_fraclen.fill_(6)
    xt = torch.from_numpy(x).to(dev)
    got = conv(xt).cpu().numpy()
    want = oracle.conv2d(x, stuffed(w, d), b, stride, pad, G)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    meta = torch.ops.f8net.conv2d(xt.to('meta'), conv.weight.to('meta'), conv.bias.to('meta'), stride, pad, G, 6, 5, False, d)
    assert tuple(meta.shape) == want.shape
    # the schema's default: a positional call without the dilation is the undilated conv
    plain = torch.ops.f8net.conv2d(xt, conv.weight.to(dev), conv.bias.to(dev), stride, 1, G, 6, 5, False).cpu().numpy()
    np.testing.assert_array_equal(plain, oracle.conv2d(x, w, b, stride, 1, G))


def _net_case(arch, dev, hw=64, seed=31):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=seed)
    x, x_fl = synth.make_input(spec, params, 2, hw, seed=3)
    return spec, params, x, x_fl


def test_an_intgraph_with_dilated_convs(dev):
    """mobilenet_v2_os16 recorded as an IntGraph (what the ONNX importer hands to build_net), against refgraph.graph_forward."""
    spec, params, x, _ = _net_case('mobilenet_v2_os16', dev)
    ig = onnx_export.graph_from_params(spec, params, 64)
    want = graph_forward(ig, x)
    assert np.unique(want).size > 8
    net = ig.build_net(2)
    assert 'dwconv3x3s1d2:' in net.describe()
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got.reshape(want.shape), want)
    net.check()


@pytest.mark.parametrize('arch', ['resnet50_os16', 'mobilenet_v2_os16'])
def test_dilated_backbones_through_build_net(arch, dev):
    """64 x 64 inputs, two images, `taps=` on the last two stage outputs; the default plan and the all-fusions plan against oracle.net_forward on the
    stuffed twin."""
    spec, params, x, x_fl = _net_case(arch, dev)
    stages = sorted({b.name.rsplit('_layer_', 1)[0] for b in spec.blocks})
    taps = [[b.name for b in spec.blocks if b.name.startswith(s + '_layer_')][-1] for s in stages[-2:]]
    seen = {}
    tspec, tparams = dil_cases.stuffed_twin(spec, params)
    want = oracle.net_forward(tspec, tparams, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, v.copy()) if k in taps else None)
    assert np.unique(want).size > 8 and all(np.unique(seen[t]).size > 8 for t in taps)
    xt = torch.from_numpy(x).to(dev)
    for options in (None, dil_cases.FUSE_ALL):
        net = build_net(spec, params, 2, hw=64, options=options, taps=taps)
        toks = [net.launch_info(i, 1)[0] for i in range(net.num_launches)]
        n_dil = sum(c.dilation > 1 for c in spec.convs())
        assert sum(t.split(':')[0].endswith('d2') or 'd2_t' in t.split(':')[0] for t in toks) == n_dil, net.describe()
        got = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got[0].cpu().numpy(), want, err_msg=str(options))
        for t, y in zip(taps, got[1:]):
            np.testing.assert_array_equal(y.cpu().numpy(), seen[t], err_msg=f'{t} {options}')
