"""The implicit-GEMM conv kernel (conv_igemm_kernel of f8_kernels.hip) at op level: every instance launch_conv dispatches (table A), the corners of
its geometry (table B) and the forms of its epilogue (table C) — tests/igemm_cases.py — bit for bit against the CPU oracle's op-by-op value.
tests/test_igemm_plan.py checks on the CPU that every case plans the instance the table names and is live on the oracle's values."""
import numpy as np
import pytest
import torch

import igemm_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _expect(case):
    return [(case['token'], case['kernel'])]


def _check_plan(case, net):
    assert ic.under_test(net) == _expect(case), net.describe()
    ls = ic.lines(net)
    for e in case['extra_tokens']:
        assert e in ls, net.describe()


def _compare(got, wants, n, msg):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(wants)
    for k, (o, want) in enumerate(zip(got, wants)):
        np.testing.assert_array_equal(o.cpu().numpy().reshape((n,) + want.shape[1:]), want[:n], err_msg=f'{msg} output {k}')


def _run_case(name, case, dev, batches=None, repeats=1, max_batch=None):
    x = ic.make_input(name, case)
    g, outs, _, _ = ic.plan(name, case, x, max_batch=max_batch)
    _check_plan(case, g.net)
    wants = [g.v[o][0] for o in outs]
    xt = torch.from_numpy(x).to(dev)
    for n in batches or [x.shape[0]]:
        for rep in range(repeats):
            _compare(g.net.run(xt[:n]), wants, n, f'{name} n={n} run {rep}')
    g.net.check()
    _check_plan(case, g.net)
    return g, wants


@pytest.mark.parametrize('name', sorted(ic.TABLE_A))
def test_every_instance(name, dev):
    """Three images on a handle finalized for the max_batch the tile needs, three runs each: the counted waits of the DMA ring are the subject, and a
    wrong wait shows sporadically."""
    _run_case(name, ic.TABLE_A[name], dev, repeats=3)


@pytest.mark.parametrize('name', sorted(ic.TABLE_B))
def test_geometry(name, dev):
    _run_case(name, ic.TABLE_B[name], dev)


@pytest.mark.parametrize('name', sorted(ic.TABLE_C))
def test_epilogue(name, dev):
    _run_case(name, ic.TABLE_C[name], dev)


def test_fewer_images_than_max_batch(dev):
    """Planned for 8 images (3x3 / pad 1 with a join on the ragged 9 x 7 map); 1, 3 and 8 images from the same handle."""
    case = dict(ic.TABLE_B['b_join_k3_p1'], N=8, max_batch=8)
    _run_case('max_batch', case, dev, batches=[1, 3, 8])


def test_pipelined_schedule(dev):
    """bench.py's schedule on the padded join: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating
    over nine runs; every output against the oracle."""
    base = ic.TABLE_C['c_join_pad']
    case = dict(base, opts=dict(base['opts'], whole_batch_launches=1, arena_copies=3, pipeline_depth=3))
    xs = [ic.make_input(f'pipelined{i}', case) for i in range(3)]
    g, outs, _, _ = ic.plan('pipelined', case, xs[0])
    _check_plan(case, g.net)
    (out,) = outs
    wants = [g.v[out][0]] + [(lambda gg: gg[0].v[gg[1][0]][0])(ic.build_graph(case, x)) for x in xs[1:]]
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    bufs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=bufs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(bufs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    g.net.check()
    _check_plan(case, g.net)


def test_autotune_keeps_token_kernel_and_value_together(dev):
    """f8_net_autotune may move the 5x5 conv over coutP 96 to any of its four tiles (the 128-wide ones skip their fourth column block): whichever it
    keeps, the plan token and the kernel name say the same tile, and the value is the oracle's as before."""
    name, case = 'b_k5_p2', ic.TABLE_B['b_k5_p2']
    g, wants = _run_case(name, case, dev)
    xt = torch.from_numpy(ic.make_input(name, case)).to(dev)
    g.net.autotune(case['N'], dev)
    (tok, kernel), = ic.under_test(g.net)
    f = kernel[kernel.index('<') + 1:-1].split(', ')
    assert tok == ic.token(case['k'], case['stride'], int(f[0]), int(f[1]), int(f[2])), (tok, kernel)
    assert f[5:] == ['true', 'false', '4', 'false'] and (int(f[0]), int(f[1])) in ((128, 128), (128, 64), (64, 128), (64, 64)) and int(f[2]) == 32
    for rep in range(3):
        _compare(g.net.run(xt), wants, case['N'], f'after autotune, run {rep}')
    g.net.check()
