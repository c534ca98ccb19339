"""Windowed average pooling on the device, bit for bit against the reference of tests/avgpool_cases.py (the window sums on int64, wrapped to int32):
every case on the three legs of option sumpool_wide — 0 (the block walker everywhere), 1 (the wide kernel from the measured crossover on), 2 (the wide
kernel for every kernel >= 2) — at N and N - 1 images from one handle planned for N + 1, and with every fusing pass on; bench.py's pipelined schedule
on two cases; a profiled run; torch.ops.f8net.avgpool2d_sum and ops.F8AvgPool2d; nets: a DenseNet block + transition + block imported from ONNX,
Inception-3a with its average-pool branch, a ResNet-D stride-2 opener, a pool on a ResNet-50 block output that a stage chain would keep on chip, a
PSP head on resnet50_os8 next to the unchanged logits.  tests/test_avgpool_plan.py checks on the CPU which token and kernel every case plans."""
import functools

import numpy as np
import pytest
import torch

import avgpool_cases as ac
import f8net_amd.torch_ops  # noqa: F401  (registers torch.ops.f8net)
import ref_ops
from avgpool_cases import producer
from f8net_amd import onnx_export, onnx_import, synth, topology
from f8net_amd.net import record_net
from graph_cases import run_case
from oracle import oracle
from refgraph import RefGraph, record_int_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _expect(name, leg):
    c = ac.CASES[name]
    return [] if c['forms'] is None else [(ac.token(c), ac.symbol(c, leg))]


def _check_plan(net, name, opts):
    assert [(t, k) for _, t, k in ac.pool_lines(net)] == _expect(name, opts.get('sumpool_wide', 1)), net.describe()


@pytest.mark.parametrize('leg', [0, 1, 2])
@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_every_case_on_every_leg(name, leg, dev):
    run_case(ac, name, dev, _check_plan, float_last_only=True, sumpool_wide=leg)


@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_every_case_with_all_fusions(name, dev):
    run_case(ac, name, dev, _check_plan, float_last_only=True, **ac.FUSE_ALL)


@pytest.mark.parametrize('name', ['g_3s1p1_5x7', 'g_15s15_15x30'])
def test_pipelined_schedule(name, dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    c = ac.CASES[name]
    N = c['N']
    xs = [ac.make_input(name, N + 1)[:N]] + [ac.make_input(name, N + 1)[::-1][:N].copy(), np.roll(ac.make_input(name, N), 1, axis=2).copy()]
    g, outs, _ = ac.plan(name, xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    ref, routs, _ = ac.reference(name)
    wants = [ref.v[routs[0]][0][:N]]
    for x in xs[1:]:
        gi, oi, _ = ac.build_graph(name, x, record=False)
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


def test_profiled_run_times_the_pool_launch(dev):
    name = 'g_3s2p1_7x9'
    x = ac.make_input(name)
    g, outs, _ = ac.plan(name, x)
    xt = torch.from_numpy(x).to(dev)
    y = g.net.run(xt)
    y2, ms = g.net.run_profiled(xt)
    assert torch.equal(y, y2) and len(ms) == g.net.num_launches
    (i, _, _), = ac.pool_lines(g.net)
    assert ms[i] > 0.0
    g.net.check()


# ---- the torch op and the module
@pytest.mark.parametrize('k, s, pad, hw', [(2, 2, 0, (7, 9)), (3, 1, 1, (5, 7)), (4, 2, 2, (8, 10)), (15, 15, 0, (15, 30)), (6, 6, 0, (6, 6))])
def test_torch_op_on_a_device_tensor(k, s, pad, hw, dev):
    x = synth.rand_uniform_int(21, f'op{k}{s}{pad}', (3, 40) + hw, -2 ** 27, 2 ** 27).astype(np.int32)
    want, _ = ref_ops.sumpool_ref(x, 0, k, s, pad)
    got = torch.ops.f8net.avgpool2d_sum(torch.from_numpy(x).to(dev), k, s, pad)
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_module_carries_the_output_fraclen(dev):
    from f8net_amd import ops
    x = synth.rand_uniform_int(22, 'mod', (2, 24, 7, 9), 0, 255).astype(np.int32)
    xt = torch.from_numpy(x).to(dev)
    xt.output_fraclen = 5
    for m, k, s, pad, sh in ((ops.F8AvgPool2d(2), 2, 2, 0, 2), (ops.F8AvgPool2d(3, stride=1, padding=1), 3, 1, 1, 3)):
        assert m.shiftnum == sh
        y = m(xt)
        assert y.output_fraclen == 5 + sh
        np.testing.assert_array_equal(y.cpu().numpy(), ref_ops.sumpool_ref(x, 0, k, s, pad)[0])


# ---- nets
def _check_graph(build, x, dev, option_sets=(None, ac.FUSE_ALL), pools=None):
    """build(g) -> output ids; records into a fresh net per option set, runs, compares every output with the graph's own reference."""
    xt = torch.from_numpy(x).to(dev)
    for options in option_sets:
        g = RefGraph(x, ac.X_FL)
        outs = build(g, next(iter(g.v)))
        for k, v in (options or {}).items():
            g.net.set_option(k, v)
        g.net.finalize(x.shape[0])
        if pools is not None:
            assert [t for _, t, _ in ac.pool_lines(g.net)] == pools, g.net.describe()
        wants = [g.v[o][0] for o in outs]
        assert all(np.unique(w).size > 50 for w in wants)
        got = g.net.run(xt)
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == len(wants)
        for y, w in zip(got, wants):
            np.testing.assert_array_equal(y.cpu().numpy().reshape(w.shape), w, err_msg=f'{options}')
        g.net.check()


def test_densenet_block_transition_block_imported_from_onnx(dev):
    x = ac.net_input('densenet')
    ig, g, out = record_int_graph(x, ac.X_FL, lambda g, x0: ac.net_densenet(g, x0)[0])
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert [(o.kernel, o.stride, o.pad, o.shift) for o in back.ops if o.kind == 'avgpool2d'] == [(2, 2, 0, 2)]
    want = g.v[out][0]
    assert np.unique(want).size > 100
    for options in (None, ac.FUSE_ALL):
        net = back.build_net(2, input_fraclen=ac.X_FL, options=options)
        assert [(t, k) for _, t, k in ac.pool_lines(net)] == [('sumpool2x2s2:', 'f8::sumpool_i32_kernel<2>')], net.describe()
        got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
        net.check()
        np.testing.assert_array_equal(got, want, err_msg=f'{options}')


@pytest.mark.parametrize('name', ['inception', 'resnet_d', 'densenet'])
def test_small_nets(name, dev):
    """Inception-3a with its average-pool branch, a ResNet-D stride-2 opener (pooled shortcut -> 1x1 -> join), the DenseNet graph recorded directly."""
    build, _, pools = ac.NETS[name]
    _check_graph(build, ac.net_input(name), dev, pools=pools)


@functools.lru_cache(maxsize=None)
def _walk(arch, hw, seed, names):
    """The oracle's walk of the net (dilated convs through their stuffed twins), once: (spec, params, x, x_fl, logits, {name: (values, fraclen)})."""
    import dil_cases
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=seed)
    x, x_fl = synth.make_input(spec, params, 2, hw, seed=3)
    names = names or (spec.blocks[-1].name,)
    seen = {}
    tspec, tparams = dil_cases.stuffed_twin(spec, params)
    logits = oracle.net_forward(tspec, tparams, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, (v.copy(), fl)) if k in names else None)
    return spec, params, x, x_fl, logits, seen


def test_pool_of_a_block_output_inside_a_stage_chain_on_resnet50(dev):
    """ResNet-50 at 64 x 64: stage_1_layer_1's output (512 x 8 x 8) sits in the middle of what the stage chain runs as one launch; a 2x2 / 2 pool
    reads it (output 1), so the launch is cut there.  The logits stay the plain net's."""
    name = 'stage_1_layer_1'
    spec, params, x, x_fl, logits, seen = _walk('resnet50', 64, 17, (name,))
    assert seen[name][0].shape[1:] == (512, 8, 8)
    xt = torch.from_numpy(x).to(dev)
    for options in (None, ac.FUSE_ALL):
        net = record_net(spec, params, 64, options=options)
        g = RefGraph.on(net, {net.tap_ids[k]: v for k, v in seen.items()})
        pl = g.avgpool(net.tap_ids[name], 2, label='pool')
        assert net.output(pl, as_float=False) == 1
        for k, v in (options or {}).items():
            net.set_option(k, v)
        net.finalize(2)
        assert [(t, k) for _, t, k in ac.pool_lines(net)] == [('sumpool2x2s2:', 'f8::sumpool_i32_kernel<2>')], net.describe()
        want = g.v[pl][0]
        assert np.unique(want).size > 100
        got, head = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {options}')
        np.testing.assert_array_equal(head.cpu().numpy().reshape(want.shape), want, err_msg=f'pool {options}')


def test_psp_head_on_resnet50_os8(dev):
    """resnet50_os8 at 96 x 96 (stage 3 on a 12 x 12 map) with a PSP head on the last block's output: bins 1 / 2 / 3 / 6 of the map (bin 1 is the
    global window: the avgpool_sum node), a 1x1 to 64 channels each, nearest upsample back to 12 x 12, concat with the stage output, a 1x1
    classifier to 5 classes: output 1.  The logits stay the plain net's bit for bit; the default and the all-fusions plan."""
    spec, params, x, x_fl, logits, seen = _walk('resnet50_os8', 96, 31, ())
    last = spec.blocks[-1].name
    assert seen[last][0].shape[2:] == (12, 12)
    xt = torch.from_numpy(x).to(dev)
    for options in (None, ac.FUSE_ALL):
        net = record_net(spec, params, 96, options=options)
        g = RefGraph.on(net, {net.tap_ids[k]: v for k, v in seen.items()})
        t = net.tap_ids[last]
        bs = [t]
        for b, bins in enumerate((1, 2, 3, 6)):
            pooled = g.adaptive_avgpool(t, bins, label=f'psp.pool{bins}')
            assert g.v[pooled][0].shape[2:] == (bins, bins)
            br = producer(g, pooled, b, 64, 5, w_fl=5, relu=True, in_fl=4, quant_input=True)
            bs.append(g.upsample(br, 12 // bins, 'nearest', label=f'psp.up{bins}'))
        cat = g.concat(bs, label='psp.cat')
        cls = producer(g, cat, 8, 5, 9, w_fl=5, relu=False, in_fl=4, quant_input=True)
        assert net.output(cls, as_float=False) == 1
        for k, v in (options or {}).items():
            net.set_option(k, v)
        net.finalize(2)
        assert [t for _, t, _ in ac.pool_lines(net)] == ['sumpool6x6s6:', 'sumpool4x4s4:', 'sumpool2x2s2:'], net.describe()
        assert sum(l.split()[1].startswith('avgpool_sum:psp.pool1') for l in net.describe().splitlines() if len(l.split()) > 1) == 1, net.describe()
        assert net.output_info(1)[:3] == (5, 12, 12)
        want = g.v[cls][0]
        assert np.unique(want).size > 100
        got, head = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {options}')
        np.testing.assert_array_equal(head.cpu().numpy().reshape(want.shape), want, err_msg=f'head {options}')
