"""Option fuse_se (f8_se.hip) on the device, bit for bit against tests/se_cases.py's reference graph: fused and as three launches, N and N - 1 of N + 1."""
import numpy as np
import pytest
import torch

import mul_cases as mc
import se_cases as sc
from graph_cases import run_case
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    assert sc.lines(net) == ([(sc.TOKEN, sc.CASES[name]['sym'])] if opts['fuse_se'] and sc.CASES[name]['sym'] else [('avgpool_sum:', 'f8::avgpool_kernel')]), net.describe()


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_every_case(name, fused, dev):
    run_case(sc, name, dev, _check_plan, fuse_se=sc.CASES[name]['key'] if fused else 0)


def _recorded(build, x, key):
    g = RefGraph(x, mc.X_FL)
    out = build(g, next(iter(g.v)))
    g.net.set_option('fuse_se', key)
    g.net.finalize(x.shape[0])
    return g.net, g.v[out[0] if isinstance(out, tuple) else out][0]


def _through_onnx(key):
    from f8net_amd import onnx_export, onnx_import
    ig, g, out = mc.se_int_graph()
    return onnx_import.import_graph(onnx_export.export_graph(ig)).build_net(3, input_fraclen=mc.X_FL, options={'fuse_se': key}), g.v[out][0]


@pytest.mark.parametrize('make, x, tokens', [(lambda key: _recorded(mc.mbv3_block, mc.mbv3_input(), key), mc.mbv3_input(), mc.MBV3_TOKENS),
                                             (lambda key: _recorded(mc.se_net, mc.se_input(), key), mc.se_input(), mc.SE_TOKENS),
                                             (_through_onnx, mc.se_input(), mc.SE_TOKENS)], ids=['mbv3_block', 'se_net', 'se_net_onnx'])
def test_whole_graph(make, x, tokens, dev):
    """One avgpool+fc+fc: launch, no avgpool_sum:, two launches fewer than with the key at 0, the gate tokens unchanged, the reference's values."""
    (off, _), (net, want) = make(0), make(1)
    assert sc.lines(off) == [('avgpool_sum:', 'f8::avgpool_kernel')] and sc.lines(net) == [(sc.TOKEN, sc.TF)], net.describe()
    assert net.num_launches == off.num_launches - 2 and [(t, k) for _, t, k in mc.lines(net)] == [(t, k) for _, t, k in mc.lines(off)] == tokens
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
    net.check()
    np.testing.assert_array_equal(got.reshape(want.shape), want)


def test_pipelined_schedule(dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    name, N = 'c72_m24', sc.CASES['c72_m24']['N']
    xs = [sc.make_input(name, N + 1)[:N], sc.make_input(name, N + 1)[::-1][:N].copy(), np.roll(sc.make_input(name, N), 1, axis=2).copy()]
    g, _, _ = sc.plan(name, xs[0], fuse_se=1, whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    assert sc.lines(g.net) == [(sc.TOKEN, sc.TF)]
    wants = [gi.v[oi[0]][0] for gi, oi, _ in (sc.build_graph(name, x, record=False) for x in xs)]
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
