"""The standalone depthwise 3x3 launches at op level: small graphs at the corners of the geometry and formats of dwconv3x3_mma_kernel (f8_dwmma.hip),
dwconv3x3_dot4_kernel and dwconv3x3_kernel (f8_kernels.hip) — tests/dw_cases.py — bit for bit against the CPU oracle's op-by-op value.  Every case
runs with its own plan and, on the same graph and input, with dw_mma = 0 (the v_dot4 kernel) and dw_mma = 0, dw_dot4 = 0 (the generic kernel).
tests/test_dw_plan.py checks on the CPU that every case is live on the oracle's values."""
import numpy as np
import pytest
import torch

import dw_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _legs(case):
    """The legs that run a kernel no earlier leg of the case runs (an int32 output keeps the generic kernel on all three)."""
    seen, legs = [], []
    for leg in dw_cases.LEGS:
        k = dw_cases.leg_kernels(case, leg)
        if k not in seen:
            seen.append(k)
            legs.append(leg)
    return legs


def _all_legs(name, case, dev, batches=None, x=None):
    x = dw_cases.make_input(name, case) if x is None else x
    xt = torch.from_numpy(x).to(dev)
    outs = {}
    for leg in _legs(case):
        g, out, _ = dw_cases.plan(name, case, x, leg)
        assert [ln[1:] for ln in dw_cases.dw_lines(g.net)] == dw_cases.expect(case, leg), g.net.describe()
        want = g.v[out][0]
        for n in batches or [x.shape[0]]:
            got = g.net.run(xt[:n]).cpu().numpy().reshape((n,) + want.shape[1:])
            np.testing.assert_array_equal(got, want[:n], err_msg=f'{name} leg={leg} n={n}')
            outs[leg] = got
        g.net.check()
        assert [ln[1:] for ln in dw_cases.dw_lines(g.net)] == dw_cases.expect(case, leg)
    return outs


@pytest.mark.parametrize('name', sorted(dw_cases.GEOMETRY))
def test_geometry(name, dev):
    _all_legs(name, dw_cases.GEOMETRY[name], dev)


@pytest.mark.parametrize('name', sorted(dw_cases.FORMATS))
def test_formats(name, dev):
    _all_legs(name, dw_cases.FORMATS[name], dev)


def test_band_14(dev):
    """The only launch of the suite with 4096 wave items, where launch_dwconv_mma keeps bands of 14 rows: 32 images x (14 + 1 rows) x (28 + 1 columns)
    x 1024 channels in one launch (split = 1; test_dw_plan.py asserts the count)."""
    _all_legs('band14', dw_cases.BAND14_CASE, dev)


def test_mma_off_equals_mma(dev):
    """The 28 x 28 map on the matrix cores and, with dw_mma = 0 as the case's own option, on the v_dot4 kernel: one input, one value."""
    x = dw_cases.make_input('28x28', dw_cases.FORMATS['f_mma_28x28'])
    a = _all_legs('f_mma_28x28', dw_cases.FORMATS['f_mma_28x28'], dev, x=x)['own']
    b = _all_legs('f_dot4_mma_off_28x28', dw_cases.FORMATS['f_dot4_mma_off_28x28'], dev, x=x)['own']
    np.testing.assert_array_equal(a, b)


def test_fewer_images_than_max_batch(dev):
    """Planned for 8 images; 3 images (sub-batches of 2 and 1), then 8 from the same handle."""
    _all_legs('max_batch', dw_cases.MAX_BATCH_CASE, dev, batches=[3, 8])


def test_pipelined_schedule(dev):
    """bench.py's schedule on depthwise / 1 -> 1x1 -> depthwise / 2: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)),
    three inputs rotating over nine runs; every output against the oracle."""
    case = dw_cases.PIPELINED_CASE
    xs = [dw_cases.make_input(f'pipelined{i}', case) for i in range(3)]
    g, out, _ = dw_cases.plan('pipelined', case, xs[0])
    assert [ln[1:] for ln in dw_cases.dw_lines(g.net)] == dw_cases.expect(case), g.net.describe()
    wants = [g.v[out][0]] + [dw_cases.build_graph(case, x)[0].v[out][0] for x in xs[1:]]
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=outs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(outs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    assert [ln[1:] for ln in dw_cases.dw_lines(g.net)] == dw_cases.expect(case)
