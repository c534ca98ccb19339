"""The operand-stationary conv launches at op level: every instance of conv1x1_wstat_kernel (table A), its geometry (B), epilogues
(C) and ring schedules, conv1x1_wreg_kernel, conv3x3s2_wreg_kernel and conv3x3_patch_kernel — tests/ostat_cases.py — bit for bit against the CPU
oracle's op-by-op value.  tests/test_ostat_plan.py checks on the CPU that every case plans the instance the table names and is live on the
oracle's values."""
import numpy as np
import pytest
import torch

import igemm_cases as ic
import ostat_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _check_plan(case, net):
    assert ic.under_test(net) == [(case['token'], case['kernel'])], net.describe()


def _compare(got, wants, n, msg):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(wants)
    for k, (o, want) in enumerate(zip(got, wants)):
        np.testing.assert_array_equal(o.cpu().numpy().reshape((n,) + want.shape[1:]), want[:n], err_msg=f'{msg} output {k}')


def _run_case(name, case, dev, batches=None, repeats=1):
    x = ic.make_input(name, case)
    g, outs, _, _ = ic.plan(name, case, x)
    _check_plan(case, g.net)
    wants = [g.v[o][0] for o in outs]
    xt = torch.from_numpy(x).to(dev)
    for n in batches or case.get('batches') or [x.shape[0]]:
        for rep in range(repeats):
            _compare(g.net.run(xt[:n]), wants, n, f'{name} n={n} run {rep}')
    g.net.check()
    _check_plan(case, g.net)
    return g, wants


def _m(case, n=None):
    P, Q = ic.out_hw(case)
    return (n or case['N']) * P * Q


@pytest.mark.parametrize('name', sorted(oc.WSTAT_A))
def test_wstat_every_instance(name, dev):
    """Three images, three runs each: the counted waits of the tile ring are the subject, and a wrong wait shows sporadically."""
    _run_case(name, oc.WSTAT_A[name], dev, repeats=3)


@pytest.mark.parametrize('name', sorted(oc.WSTAT_B))
def test_wstat_geometry(name, dev):
    """The device has more compute units per channel group than the case has tiles: MG = T, one tile per pixel group (asserted: a device on which
    it is not so runs another schedule than the one the case is about)."""
    case = oc.WSTAT_B[name]
    T, MG, NG, grid, nts = oc.schedule(_m(case), (case['cout'] + 31) // 32 * 32, case['nw'], _cus(dev), 0)
    assert MG == T and set(nts) == {1}, f'{T} tiles on {MG} pixel groups: this device gives a pixel group more than one tile'
    _run_case(name, case, dev)


@pytest.mark.parametrize('name', sorted(oc.WSTAT_C))
def test_wstat_epilogue(name, dev):
    _run_case(name, oc.WSTAT_C[name], dev)


@pytest.mark.parametrize('name', sorted(oc.WSTAT_SCHED))
def test_wstat_ring_schedule(name, dev):
    """wstat_grid_div = 32: the pixel groups walk the tile counts the case names (the warm-up waits, the steady-state constant, the slot wrap-around,
    the uneven split), asserted from the device's compute units; three runs."""
    case = oc.WSTAT_SCHED[name]
    T, MG, NG, grid, nts = oc.schedule(_m(case), (case['cout'] + 31) // 32 * 32, case['nw'], _cus(dev), 32)
    assert T == case['T'] and set(nts) == oc.SCHED_NT[T], f'{T} tiles on {MG} pixel groups walk {sorted(set(nts))} tiles, not {sorted(oc.SCHED_NT[T])}, on this device'
    _run_case(name, case, dev, repeats=3)


def test_wstat_fewer_images_than_max_batch(dev):
    """The dual pair planned for 8 images; 1, 3 and 8 from the same handle (2, 6 and 16 tiles)."""
    _run_case('w_max_batch', oc.WSTAT_MAX_BATCH, dev, batches=[1, 3, 8])


def test_wstat_pipelined_schedule(dev):
    """bench.py's schedule on the residual join under wstat_grid_div = 32 (groups of 4 and 5 tiles): whole-batch launches, three arena copies, runs
    in flight (set_pipelined(2)), three inputs rotating over nine runs; every output against the oracle."""
    case = oc.WSTAT_PIPELINED
    T, MG, NG, grid, nts = oc.schedule(_m(case), 256, 8, _cus(dev), 32)
    assert T == case['T'] and set(nts) == oc.SCHED_NT[T], (T, MG, nts)
    xs = [ic.make_input(f'w_pipelined{i}', case) for i in range(3)]
    g, outs, _, _ = ic.plan('w_pipelined', case, xs[0])
    _check_plan(case, g.net)
    # (the output tensors' ids are the same in every build of the same case)
    wants = [[gg.v[o][0] for o in outs] for gg in [g] + [ic.build_graph(case, x)[0] for x in xs[1:]]]
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    g.net.set_pipelined(2)
    got = [g.net.run(xt[r % 3]) for r in range(9)]                # (every run writes buffers of its own)
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        _compare(got[r], wants[r % 3], case['N'], f'run {r}')
    g.net.check()
    _check_plan(case, g.net)


@pytest.mark.parametrize('name', sorted(oc.WREG))
def test_wreg(name, dev):
    _run_case(name, oc.WREG[name], dev, repeats=3)


@pytest.mark.parametrize('name', sorted(oc.S2WREG))
def test_s2wreg(name, dev):
    """1, 3, 4 and 5 images from a handle finalized for 5: a full group of four images, workgroups that return (n >= N), both halves."""
    _run_case(name, oc.S2WREG[name], dev)


@pytest.mark.parametrize('name', sorted(oc.PATCH))
def test_patch3x3(name, dev):
    _run_case(name, oc.PATCH[name], dev)
