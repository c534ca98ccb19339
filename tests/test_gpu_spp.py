"""Stride-1 max pools on the LDS-tile kernel and the SPP / SPPF pyramid in one launch (f8_maxpool.hip) on the device, bit for bit against the reference
graph: every case of tests/spp_cases.py on the parent's plan, with maxpool_tile = 2 and with fuse_spp = 1 on top; one case imported from ONNX; the
op-level pool on a handle seeded with the option."""
import numpy as np
import pytest
import torch

import spp_cases as sc
from f8net_amd import onnx_export, onnx_import, ops, synth
from graph_cases import run_case
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_case(name, dev):
    for leg, opts in sc.LEGS.items():
        run_case(sc, name, dev, lambda net, name, opts: (sc.lines(net) == sc.want(name, leg)) or pytest.fail(net.describe()), **opts)


def test_sppf_from_onnx(dev):
    ig, g, out = sc.int_graph('sppf_555')
    want = g.v[out][0]
    net = onnx_import.import_graph(onnx_export.export_graph(ig)).build_net(2, input_fraclen=sc.X_FL, options=sc.LEGS['F'])
    assert sc.lines(net) == sc.want('sppf_555', 'F'), net.describe()
    got = net.run(torch.from_numpy(sc.make_input('sppf_555')).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got.reshape(want.shape), want)
    net.check()


def test_op_level_pool_on_a_seeded_handle(dev, monkeypatch):
    monkeypatch.setenv('F8_MAXPOOL_TILE', '2')                       # (the op returns int32, so its pool stays in the int32 mode: the key must not disturb it)
    x = synth.rand_uniform_int(7, 'spp_op', (2, 40, 13, 21), -2 ** 20, 2 ** 20).astype(np.int32)
    got = ops.F8MaxPool2d(5, 1, 2)(torch.from_numpy(x).to(dev))
    np.testing.assert_array_equal(got.cpu().numpy(), oracle.maxpool(x, 5, 1, 2))
