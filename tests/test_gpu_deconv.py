"""Transposed convolutions on the device, bit for bit against the reference of tests/deconv_cases.py (the scatter form on int64, wrapped to int32):
every case on the default plan and with every fusing pass on, at N and N - 1 images; one handle planned for 8 run at 3 and then 8; bench.py's
pipelined schedule; a profiled run; requant_float = 1 (same symbol, same values); the op-level drop-in (ops.F8ConvTranspose2d /
torch.ops.f8net.conv_transpose2d); a small U-Net; an FCN-style head on tapped ResNet-18 stages next to the unchanged logits; an ONNX-imported graph.
tests/test_deconv_plan.py checks on the CPU what every case plans."""
import numpy as np
import pytest
import torch

import deconv_cases as dc
import ref_ops
from f8net_amd import onnx_export, onnx_import, ops, synth, topology
from f8net_amd.net import record_net
from graph_cases import run_case
from oracle import oracle
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    dc.check_lines(dc.CASES[name], dc.deconv_lines(net), net.describe())


def _run(name, dev, **opts):
    """(the reference runs over N images and the handle is planned for N: no spare image)"""
    run_case(dc, name, dev, _check_plan, spare_image=False, float_last_only=True, **opts)


@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_every_case_on_the_default_plan(name, dev):
    _run(name, dev)


@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_every_case_with_all_fusions(name, dev):
    _run(name, dev, **dc.FUSE_ALL)


@pytest.mark.parametrize('name', ['g_4210_9x11', 'e_2300'])
def test_one_handle_planned_for_8_runs_3_then_8(name, dev):
    x = dc.make_input(name, 8)
    g, outs, _ = dc.plan(name, x, max_batch=8)
    want = g.v[outs[0]][0]
    xt = torch.from_numpy(x).to(dev)
    for n in (3, 8):
        got = g.net.run(xt[:n]).cpu().numpy().reshape((n,) + want.shape[1:])
        np.testing.assert_array_equal(got, want[:n], err_msg=f'n={n}')
    g.net.check()


@pytest.mark.parametrize('name', ['g_4210', 'f_unet_i8'])
def test_pipelined_schedule(name, dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    c = dc.CASES[name]
    N = c['N']
    xs = [dc.make_input(name), dc.make_input(name)[::-1].copy(), np.roll(dc.make_input(name), 1, axis=2).copy()]
    g, outs, _ = dc.plan(name, xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    wants = [g.v[outs[0]][0]]
    for x in xs[1:]:
        gi, oi, _ = dc.build_graph(name, x, record=False)
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


def test_profiled_run_times_the_deconv_launch(dev):
    name = 'g_4210'
    x = dc.make_input(name)
    g, outs, _ = dc.plan(name, x)
    xt = torch.from_numpy(x).to(dev)
    y = g.net.run(xt)
    y2, ms = g.net.run_profiled(xt)
    assert torch.equal(y, y2) and len(ms) == g.net.num_launches
    (i, _, _), = dc.deconv_lines(g.net)
    assert ms[i] > 0.0
    g.net.check()


@pytest.mark.parametrize('name', ['g_4210', 'g_5321'])
def test_requant_float_changes_neither_symbol_nor_values(name, dev):
    """The transposed conv's epilogue is the integer requantisation whatever requant_float says."""
    _run(name, dev, requant_float=1)


@pytest.mark.parametrize('k, s, pad, op, cin, cout, hw, signed', [(2, 2, 0, 0, 8, 8, (3, 5), False), (4, 2, 1, 0, 40, 21, (7, 7), True),
                                                                   (3, 2, 1, 1, 64, 40, (3, 5), False), (3, 1, 1, 0, 8, 8, (3, 5), True)])
def test_op_level_drop_in(k, s, pad, op, cin, cout, hw, signed, dev):
    """ops.F8ConvTranspose2d (torch.ops.f8net.conv_transpose2d) on int32 NCHW against the reference; the module's parameters have nn.ConvTranspose2d's shapes."""
    m = ops.F8ConvTranspose2d(cin, cout, k, stride=s, padding=pad, output_padding=op, input_symmetric=signed)
    assert tuple(m.weight.shape) == (cin, cout, k, k)
    w = synth.rand_uniform_int(3, f'opw{k}{s}', (cin, cout, k, k), -127, 127).astype(np.int32)
    b = synth.rand_uniform_int(4, f'opb{k}{s}', (cout,), -2 ** 20, 2 ** 20).astype(np.int32)
    x = synth.rand_uniform_int(5, f'opx{k}{s}', (2, cin) + hw, -127 if signed else 0, 127 if signed else 255).astype(np.int32)
    m.weight.data = torch.from_numpy(w)
    m.bias.data = torch.from_numpy(b)
    m.weight_fraclen.fill_(6)
    m.input_fraclen.fill_(4)
    m = m.to(dev)
    got = m(torch.from_numpy(x).to(dev))
    want = ref_ops.deconv_ref(x, w, b, s, pad, op)
    assert tuple(got.shape) == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def _up(g, t, k, s, pad, cout, seed, label, relu=True, in_fl=4):
    """A transposed conv of tensor t (read at unsigned fraclen in_fl) to cout channels at fraclen in_fl + 6."""
    cin = g.v[t][0].shape[1]
    c = dict(k=k, s=s, cin=cin, cout=cout, src='conv', relu=relu, bias_big=False)
    w, b = dc.weights(c, seed)
    return g.conv_transpose(t, w, b, stride=s, pad=pad, output_padding=0, weight_fl=6, input_fl=in_fl, input_signed=False, relu=relu, label=label)


def test_small_unet(dev):
    """64 x 64 input -> enc1 (3x3 / 2, 32 channels, 32 x 32) -> enc2 (3x3 / 2, 64 channels, 16 x 16) -> mid (3x3) -> deconv 2x2 / 2 to 32 channels,
    concatenated with enc1 -> 3x3 -> deconv 2x2 / 2 to 16 channels, concatenated with a 3x3 of the input -> 1x1 to 5 classes: the output."""
    x = synth.rand_uniform_int(7, 'unetx', (2, 8, 64, 64), 0, 255).astype(np.int32)
    for options in (None, dc.FUSE_ALL):
        g = RefGraph(x, dc.X_FL)
        x0 = next(iter(g.v))

        def conv3(t, k, cout, stride, first=False, w_fl=5):
            cin = g.v[t][0].shape[1]
            w = dc._w(60 + k, (cout, cin, 3, 3), float(np.clip(5000.0 / ((90.0 if first else 40.0) * (9 * cin) ** 0.5), 0.7, 40.0)))
            return g.conv(t, w, dc._b(70 + k, cout, 2.0 ** 11, 2.0 ** 12), stride=stride, pad=1, groups=1, weight_fl=w_fl, input_fl=dc.X_FL if first else 4,
                          input_signed=False, relu=True, quant_input=not first)

        skip0 = conv3(x0, 0, 16, 1, first=True, w_fl=2)             # fraclen 10, the second deconv's
        enc1 = conv3(x0, 1, 32, 2, first=True, w_fl=2)              # fraclen 10, the first deconv's
        enc2 = conv3(enc1, 2, 64, 2, w_fl=6)
        mid = conv3(enc2, 3, 64, 1, w_fl=6)
        up1 = _up(g, mid, 2, 2, 0, 32, 80, 'up1')
        dec1 = conv3(g.concat([up1, enc1], label='cat1'), 4, 32, 1, w_fl=6)
        up0 = _up(g, dec1, 2, 2, 0, 16, 82, 'up0')
        dec0 = conv3(g.concat([up0, skip0], label='cat0'), 5, 16, 1, w_fl=6)
        out = g.conv(dec0, dc._w(66, (5, 16, 1, 1), 20.0), None, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
        g.output(out)
        for k, v in (options or {}).items():
            g.net.set_option(k, v)
        g.net.finalize(2)
        assert [(t, s) for lab in ('up1', 'up0') for _, t, s in dc.deconv_lines(g.net, lab)] == [('deconv2x2s2:', dc.symbol(32)), ('deconv2x2s2:', dc.symbol(16))], g.net.describe()
        want = g.v[out][0]
        assert want.shape == (2, 5, 64, 64) and np.unique(want).size > 1000 and np.unique(g.v[up0][0]).size > 100
        got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
        g.net.check()
        np.testing.assert_array_equal(got, want, err_msg=str(options))


def test_fcn_head_on_tapped_resnet18_stages(dev):
    """ResNet-18 at 64 x 64: the outputs of stage 1 (128 x 8 x 8), stage 2 (256 x 4 x 4) and stage 3 (512 x 2 x 2), tapped; a 1x1 score conv to 21 classes
    on each, the coarsest upsampled by a 4x4 / 2 / pad 1 transposed conv and joined with the next one's scores, twice (FCN-8s): output 1.  The
    logits stay the plain net's bit for bit; the default and the all-fusions plan."""
    spec = topology.get('resnet18')
    params = synth.make_params(spec, seed=19)
    x, x_fl = synth.make_input(spec, params, 2, 64, seed=5)
    names = [[b.name for b in spec.blocks if b.name.startswith(f'stage_{s}_')][-1] for s in (1, 2, 3)]
    seen = {}
    logits = oracle.net_forward(spec, params, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, (v.copy(), fl)) if k in names else None)
    assert [seen[n][0].shape[1:] for n in names] == [(128, 8, 8), (256, 4, 4), (512, 2, 2)]
    xt = torch.from_numpy(x).to(dev)
    for options in (None, dc.FUSE_ALL):
        net = record_net(spec, params, 64, options=options)
        g = RefGraph.on(net, {net.tap_ids[k]: v for k, v in seen.items()})
        # score convs first, so that each join's later producer is the transposed conv: the joins stay add: launches
        sc = [dc.producer(g, net.tap_ids[n], k, 21, 9, w_fl=6, relu=False, in_fl=4, quant_input=True) for k, n in enumerate(names)]      # fraclen 10
        up = _up(g, sc[2], 4, 2, 1, 21, 90, 'up32', relu=False, in_fl=4)
        f16 = g.add(up, sc[1])
        up = _up(g, f16, 4, 2, 1, 21, 92, 'up16', relu=False, in_fl=4)
        f8 = g.add(up, sc[0])
        assert net.output(f8, as_float=False) == 1
        for k, v in (options or {}).items():
            net.set_option(k, v)
        net.finalize(2)
        assert [(t, s) for lab in ('up32', 'up16') for _, t, s in dc.deconv_lines(net, lab)] == [('deconv4x4s2:', dc.symbol(21))] * 2, net.describe()
        assert sum(net.launch_info(i, 1)[0].startswith('add:') for i in range(net.num_launches)) >= 2, net.describe()
        assert net.output_info(1)[:3] == (21, 8, 8)
        want = g.v[f8][0]
        assert np.unique(want).size > 100
        got, head = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {options}')
        np.testing.assert_array_equal(head.cpu().numpy().reshape(want.shape), want, err_msg=f'head {options}')


@pytest.mark.parametrize('name', ['g_5321', 'f_unet_i8', 'f_fcn'])
def test_onnx_imported_graph_with_a_conv_transpose(name, dev):
    """The case written as an ONNX file (ConvTranspose), imported, and planned through IntGraph.build_net."""
    ig, g, out = dc.int_graph(name)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    x = dc.make_input(name)
    want = g.v[out][0]
    net = back.build_net(x.shape[0], input_fraclen=dc.X_FL)
    dc.check_lines(dc.CASES[name], dc.deconv_lines(net), net.describe())
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
    net.check()
    np.testing.assert_array_equal(got, want)
