"""The fused inverted-residual launch (f8_ir.hip, fuse_ir = 2) at op level: small graphs at the corners of its geometry and formats
(tests/ir_cases.py), bit for bit against the CPU oracle's op-by-op value, next to the three-launch plan (fuse_ir = 0) of the same graph.
tests/test_ir_plan.py checks on the CPU that every case is live on the oracle's values."""
import numpy as np
import pytest
import torch

import ir_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _both_legs(name, case, dev, batches=None):
    x = ir_cases.make_input(name, case)
    for fuse_ir in (2, 0):
        g, out, _ = ir_cases.plan(name, case, x, fuse_ir)
        assert ir_cases.fused_lines(g.net) == (case['expect'] if fuse_ir else []), g.net.describe()
        want = g.v[out][0]
        for n in batches or [x.shape[0]]:
            got = g.net.run(torch.from_numpy(x[:n]).to(dev)).cpu().numpy().reshape((n,) + want.shape[1:])
            np.testing.assert_array_equal(got, want[:n], err_msg=f'{name} fuse_ir={fuse_ir} n={n}')
        assert ir_cases.fused_lines(g.net) == (case['expect'] if fuse_ir else [])


@pytest.mark.parametrize('name', sorted(ir_cases.GEOMETRY))
def test_geometry(name, dev):
    _both_legs(name, ir_cases.GEOMETRY[name], dev)


@pytest.mark.parametrize('name', sorted(ir_cases.FORMATS))
def test_formats(name, dev):
    _both_legs(name, ir_cases.FORMATS[name], dev)


def test_fewer_images_than_max_batch(dev):
    """Planned for 8 images; 3 images (two workgroups: tiles of 2 and 1), then 8 from the same handle."""
    _both_legs('max_batch', ir_cases.MAX_BATCH_CASE, dev, batches=[3, 8])


def test_pipelined_schedule(dev):
    """bench.py's schedule on two stride-1 blocks and a stride-2 block: whole-batch launches, three arena copies, runs in flight
    (set_pipelined(2)), three inputs rotating over nine runs; every output against the oracle."""
    case = ir_cases.PIPELINED_CASE
    xs = [ir_cases.make_input(f'pipelined{i}', case) for i in range(3)]
    g, out, _ = ir_cases.plan('pipelined', case, xs[0], 2)
    assert ir_cases.fused_lines(g.net) == case['expect'], g.net.describe()
    wants = [g.v[out][0]] + [ir_cases.build_graph(case, x)[0].v[out][0] for x in xs[1:]]
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=outs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(outs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
