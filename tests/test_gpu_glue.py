"""The pool, join and classifier launches on the device — maxpool_kernel, maxpool_i8x16_kernel, avgpool_kernel, add_kernel (`add:` and `requant:`),
fc_dense_kernel<512 | 1024 | 1280 | 2048> — bit for bit against the oracle's op-level functions: every case of tests/glue_cases.py at N and N - 1
images from one handle planned for N + 1, and with every fusing pass on; bench.py's pipelined schedule on pool -> join -> global pool -> classifier.
tests/test_glue_plan.py checks on the CPU what every case plans and that its data can show a wrong kernel.

No leg under requant_float = 1: bind_step's `out_formats` hands these kernels Requant::of(shift, signed) of each int8 output form, whatever that
option says, and they requantise with the integer requant_pack4 only; the option changes nothing they are given."""
import numpy as np
import pytest
import torch

import glue_cases as gc
from graph_cases import run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    assert gc.lines(net) == gc.expected(name, **opts), net.describe()


@pytest.mark.parametrize('name', sorted(gc.CASES))
def test_every_case(name, dev):
    run_case(gc, name, dev, _check_plan)


@pytest.mark.parametrize('name', sorted(gc.CASES))
def test_every_case_with_all_fusions(name, dev):
    run_case(gc, name, dev, _check_plan, **gc.FUSE_ALL)


def test_pipelined_schedule(dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs.  The
    classifier reads the run's chain error word and epoch on this path: clean, so no logit is poisoned and check() passes."""
    name = 'p_pool_join_gap_fc'
    N = gc.CASES[name]['N']
    xs = [gc.make_input(name, N + 1)[:N]] + [gc.make_input(name, N + 1)[::-1][:N].copy(), np.roll(gc.make_input(name, N), 1, axis=2).copy()]
    g, outs, _ = gc.plan(name, xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    _check_plan(g.net, name, {})
    ref, routs, _ = gc.reference(name)
    wants = [ref.v[routs[0]][0][:N]]
    for x in xs[1:]:
        gi, oi, _ = gc.build_graph(name, x, record=False)
        wants.append(gi.v[oi[0]][0])
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[1], wants[2])
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    bufs = [torch.empty((N, wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=bufs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        got = bufs[r].cpu().numpy()
        assert (got != -2 ** 31).all(), f'run {r}: poisoned logits'
        np.testing.assert_array_equal(got.reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    g.net.check()
