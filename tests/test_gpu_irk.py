"""The fused inverted-residual launch around a depthwise 5x5 / 7x7 (f8_irk.hip, fuse_irk = 1) at op level: small graphs at the corners of its
geometry, channel counts and formats (tests/irk_cases.py), bit for bit against the CPU oracle's op-by-op value, next to the three-launch plan
(fuse_irk = 0) of the same graph.  tests/test_irk_plan.py checks on the CPU that every case is live on the oracle's values."""
import numpy as np
import pytest
import torch

import irk_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _both_legs(name, case, dev, batches=None):
    x = irk_cases.make_input(name, case)
    want = None
    for fuse_irk in (1, 0):
        g, out, _ = irk_cases.plan(name, case, x, fuse_irk)
        assert irk_cases.fused_lines(g.net) == (case['expect'] if fuse_irk else []), g.net.describe()
        want = g.v[out][0]
        for n in batches or [x.shape[0]]:
            got = g.net.run(torch.from_numpy(x[:n]).to(dev)).cpu().numpy().reshape((n,) + want.shape[1:])
            np.testing.assert_array_equal(got, want[:n], err_msg=f'{name} fuse_irk={fuse_irk} n={n}')
    return want


@pytest.mark.parametrize('name', sorted(irk_cases.GEOMETRY))
def test_geometry(name, dev):
    _both_legs(name, irk_cases.GEOMETRY[name], dev)


@pytest.mark.parametrize('name', sorted(irk_cases.CHANNELS))
def test_channels(name, dev):
    _both_legs(name, irk_cases.CHANNELS[name], dev)


@pytest.mark.parametrize('name', sorted(irk_cases.FORMATS))
def test_formats(name, dev):
    _both_legs(name, irk_cases.FORMATS[name], dev)


@pytest.mark.parametrize('suf', ['k5s1', 'k7s2'])
def test_requant_float_plans_run_the_integer_instance_with_the_same_values(suf, dev):
    """requant_float = 1: the same symbol (irk_cases: instance 2 on both) and, the inputs being the same, the same values as the plain case."""
    plain, rq1 = irk_cases.FORMATS[f'f_signed_in_{suf}'], irk_cases.FORMATS[f'f_rq1_{suf}']
    assert [k for _, k in plain['expect']] == [k for _, k in rq1['expect']]
    x = irk_cases.make_input('rq', plain)
    outs = []
    for case in (plain, rq1):
        g, out, _ = irk_cases.plan('rq', case, x, 1)
        assert irk_cases.fused_lines(g.net) == case['expect'], g.net.describe()
        outs.append(g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(g.v[out][0].shape))
        np.testing.assert_array_equal(outs[-1], g.v[out][0])
    np.testing.assert_array_equal(outs[0], outs[1])


def test_fewer_images_than_max_batch(dev):
    """Planned for 8 images; 3 images (one ragged group), then 8 (two groups) from the same handle."""
    _both_legs('max_batch', irk_cases.MAX_BATCH_CASE, dev, batches=[3, 8])


def test_pipelined_schedule(dev):
    """bench.py's schedule on a stride-2 opener and two joined blocks: whole-batch launches, three arena copies, runs in flight
    (set_pipelined(2)), three inputs rotating over nine runs; every output against the oracle."""
    case = irk_cases.PIPELINED_CASE
    xs = [irk_cases.make_input(f'pipelined{i}', case) for i in range(3)]
    g, out, _ = irk_cases.plan('pipelined', case, xs[0], 1)
    assert irk_cases.fused_lines(g.net) == case['expect'], g.net.describe()
    wants = [g.v[out][0]] + [irk_cases.build_graph(case, x)[0].v[out][0] for x in xs[1:]]
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=outs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(outs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
