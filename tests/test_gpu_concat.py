"""Channel concatenation on the device, bit for bit against the reference of tests/concat_cases.py (`oracle.add_align` next to a zero partner, then
np.concatenate): every case on both legs — option concat_i8 = 1 (the byte gather where the plan allows it) and 0 (the int32 launch everywhere) — at N
and N - 1 images from one handle planned for N + 1, and with every fusing pass on; bench.py's pipelined schedule on two cases; an ASPP head on
resnet50_os16's stage-3 output next to the unchanged logits; an ONNX-imported DenseNet graph through IntGraph.build_net.
tests/test_concat_plan.py checks on the CPU which mode and kernel instance every case plans."""
import numpy as np
import pytest
import torch

import concat_cases as cc
from f8net_amd import onnx_export, onnx_import, synth, topology
from f8net_amd.net import build_net, record_net
from graph_cases import run_case
from oracle import oracle
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    c = cc.CASES[name]
    i8 = opts.get('concat_i8', 1)
    assert all(tok == (c['mode'] if i8 else cc.I32) for _, tok, _ in cc.concat_lines(net)), net.describe()


@pytest.mark.parametrize('i8', [1, 0])
@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_every_case_on_both_legs(name, i8, dev):
    run_case(cc, name, dev, _check_plan, concat_i8=i8)


@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_every_case_with_all_fusions(name, dev):
    run_case(cc, name, dev, _check_plan, **cc.FUSE_ALL)


@pytest.mark.parametrize('name', ['straddle', 'nested'])
def test_pipelined_schedule(name, dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    c = cc.CASES[name]
    N = c['N']
    xs = [cc.make_input(name, N + 1)[:N]] + [cc.make_input(name, N + 1)[::-1][:N].copy(), np.roll(cc.make_input(name, N), 1, axis=2).copy()]
    g, outs, _ = cc.plan(name, xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    ref, routs, _ = cc.reference(name)
    wants = [ref.v[routs[0]][0][:N]]
    for x in xs[1:]:
        gi, oi, _ = cc.build_graph(name, x, record=False)
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


def test_profiled_run_times_the_concat_launch(dev):
    name = 'aligned2'
    x = cc.make_input(name)
    g, outs, _ = cc.plan(name, x)
    xt = torch.from_numpy(x).to(dev)
    y = g.net.run(xt)
    y2, ms = g.net.run_profiled(xt)
    assert torch.equal(y, y2) and len(ms) == g.net.num_launches
    (i, _, _), = cc.concat_lines(g.net)
    assert ms[i] > 0.0
    g.net.check()


def test_aspp_head_on_resnet50_os16(dev):
    """resnet50_os16 at 96 x 96 (stage 3 on a 6 x 6 map) with an ASPP head on the stage-3 output as output 1: the logits stay the plain net's bit for
    bit, the head matches the reference walk from the oracle's stage-3 tensor; the default plan and the all-fusions plan."""
    spec = topology.get('resnet50_os16')
    params = synth.make_params(spec, seed=31)
    x, x_fl = synth.make_input(spec, params, 2, 96, seed=3)
    last = spec.blocks[-1].name
    seen = {}
    import dil_cases
    tspec, tparams = dil_cases.stuffed_twin(spec, params)
    logits = oracle.net_forward(tspec, tparams, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, (v.copy(), fl)) if k == last else None)
    assert seen[last][0].shape[2:] == (6, 6)
    xt = torch.from_numpy(x).to(dev)
    for options in (None, cc.FUSE_ALL):
        plain = build_net(spec, params, 2, hw=96, options=options).run(xt).cpu().numpy()
        np.testing.assert_array_equal(plain, logits, err_msg=str(options))
        net = record_net(spec, params, 96, options=options)
        t = net.tap_ids[last]
        g = RefGraph.on(net, {t: seen[last]})
        proj, cat = cc.aspp_head(g, t)
        assert net.output(proj, as_float=False) == 1
        for k, v in (options or {}).items():
            net.set_option(k, v)
        net.finalize(2)
        (_, tok, sym), = cc.concat_lines(net)
        assert (tok, sym) == (cc.I8, 'f8::concat_i8_kernel<true>'), net.describe()
        want = g.v[proj][0]
        assert np.unique(want).size > 8 and np.unique(g.v[cat][0]).size > 8
        got, head = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {options}')
        np.testing.assert_array_equal(head.cpu().numpy(), want, err_msg=f'head {options}')


def test_onnx_imported_densenet_graph(dev):
    """The `nested` case written as an ONNX file, imported, and planned through IntGraph.build_net."""
    ig, g, out = cc.int_graph('nested')
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    x = cc.make_input('nested')
    want = g.v[out][0]
    net = back.build_net(x.shape[0], input_fraclen=cc.X_FL)
    assert len(cc.concat_lines(net)) == 4
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
    net.check()
    np.testing.assert_array_equal(got, want)
