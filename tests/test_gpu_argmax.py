"""Channel argmax outputs on the device, bit for bit against the reference of tests/argmax_cases.py (np.argmax on int64 of the value the reference
graph holds; a fused case: ref_ops.upsample_ref, its int32 wrap included, then argmax): every case with every data kind of its own — all-negative
pixels, all-equal channels, ties across the lane halves / groups / channel blocks, INT32_MIN / INT32_MAX, sums that wrap, random — on three legs: the
default plan, every fusing pass on, and fuse_argmax = 0, each at N and N - 1 images from one handle planned for N + 1; bench.py's pipelined schedule
and a profiled run; a segmentation head on ResNet-18 (the class map next to the unchanged logits, the upsampled logits in no launch) and ResNet-18's
top-1 against argmax of the oracle's logits.  tests/test_argmax_plan.py checks on the CPU which token and kernel every case plans."""
import numpy as np
import pytest
import torch

import argmax_cases as ac
from f8net_amd import synth, topology
from f8net_amd.net import record_net
from oracle import oracle
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _compare(got, g, n, what):
    """The run's outputs against the graph's references over the first n images: value outputs as they are, class maps in their element type."""
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(g.outs)
    for k, (y, o) in enumerate(zip(got, g.outs)):
        want = o[1][:n]
        if o[0] == 'argmax':
            assert y.dtype == (torch.uint8 if o[2] == 'u8' else torch.int32) and y.numel() == want.size, (what, k, y.dtype, tuple(y.shape))
        np.testing.assert_array_equal(y.cpu().numpy().astype(np.int64).reshape(want.shape), want, err_msg=f'{what} n={n} output {k}')


def _run_case(name, leg, dev):
    c = ac.CASES[name]
    N, M = c['N'], c['N'] + 1
    opts = ac.LEGS[leg]
    tok = ac.expected_token(name, opts)
    for data in ac.data_kinds(name):
        ref, _, x = ac.reference(name, data)                       # (asserts what the data promises)
        g, _ = ac.plan(name, data, x, max_batch=M, **opts)
        assert [(t, k) for _, t, k in ac.argmax_lines(g.net)] == [(tok, ac.SYMBOL[tok])], g.net.describe()
        xt = torch.from_numpy(x).to(dev)
        for n in (N, N - 1):
            if n >= 1:
                _compare(g.net.run(xt[:n]), ref, n, f'{name} {data} {leg}')
        g.net.check()


@pytest.mark.parametrize('leg', sorted(ac.LEGS))
@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_every_case_and_data_kind_on_every_leg(name, leg, dev):
    _run_case(name, leg, dev)


@pytest.mark.parametrize('name', ['split2', 'split2_i32'])
def test_split_sub_batches_write_their_own_part_of_the_buffer(name, dev):
    """split = 2 at 4 and at 5 images of a 9-pixel map: the second sub-batch starts at byte 18 / 27 (uint8) of the caller's buffer — n0 * H * W elements of
    the index type, not of 4 bytes — and a guard region behind the map stays untouched."""
    c = ac.CASES[name]
    x = ac.make_input(name, 'random', 5)
    ref, _ = ac.build_graph(name, 'random', x, record=False)
    g, _ = ac.plan(name, 'random', x, max_batch=5)
    dt = torch.uint8 if c['dtype'] == 'u8' else torch.int32
    xt = torch.from_numpy(x).to(dev)
    for n in (4, 5):
        assert g.net.num_parts(n) == 2
        buf = torch.full((5 * 9 + 64,), 77, dtype=dt, device=dev)
        g.net.run(xt[:n], out=buf[:n * 9])
        got = buf.cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(got[:n * 9].reshape(n, 3, 3), ref.outs[0][1][:n], err_msg=f'{name} n={n}')
        assert (got[n * 9:] == 77).all(), 'the launch wrote behind its map'
    g.net.check()


@pytest.mark.parametrize('name', ['c21_7x7', 'b4_19x3x3_u8'])
def test_pipelined_schedule(name, dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    N = ac.CASES[name]['N']
    xs = [ac.make_input(name, d, N) for d in ('random', 'ties', 'neg')]
    wants = [ac.build_graph(name, d, x, record=False)[0].outs[0][1] for d, x in zip(('random', 'ties', 'neg'), xs)]
    g, _ = ac.plan(name, 'random', xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    bufs = [torch.empty((N, wants[0][0].size), dtype=torch.uint8, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=bufs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(bufs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    g.net.check()


def test_profiled_run_times_the_argmax_launch(dev):
    name = 'b2_21x5x3_u8'
    x = ac.make_input(name, 'random', 2)
    g, _ = ac.plan(name, 'random', x)
    xt = torch.from_numpy(x).to(dev)
    y = g.net.run(xt)
    y2, ms = g.net.run_profiled(xt)
    assert y.dtype == torch.uint8 and torch.equal(y, y2) and len(ms) == g.net.num_launches
    (i, _, _), = ac.argmax_lines(g.net)
    assert ms[i] > 0.0
    g.net.check()


def test_a_wrong_buffer_type_is_refused(dev):
    name = 'behind_value'
    x = ac.make_input(name, 'random', 2)
    g, _ = ac.plan(name, 'random', x)
    with pytest.raises(ValueError, match='uint8'):
        g.net.run(torch.from_numpy(x).to(dev), outs=[torch.empty((2, 5, 3), dtype=torch.int32, device=dev)])


# ---- whole graphs
def test_segmentation_head_on_resnet18(dev):
    """ResNet-18 at 64 x 64: a 1x1 classifier to 21 classes on the tapped stage-1 output (128 x 8 x 8), bilinear x8 back to 64 x 64, the class map as
    output 1 next to the unchanged logits of the net.  The default and the all-fusions plan hold `upsample_bilinear+argmax_u8:` and no upsample launch;
    fuse_argmax = 0 holds the two launches; the same class map on all three."""
    from concat_cases import producer
    spec = topology.get('resnet18')
    params = synth.make_params(spec, seed=17)
    x, x_fl = synth.make_input(spec, params, 2, 64, seed=3)
    stage = [b.name for b in spec.blocks if b.name.startswith('stage_1')][-1]
    seen = {}
    logits = oracle.net_forward(spec, params, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, (v.copy(), fl)) if k == stage else None)
    assert seen[stage][0].shape[2:] == (8, 8)
    xt = torch.from_numpy(x).to(dev)
    for leg, options in ac.LEGS.items():
        net = record_net(spec, params, 64, options=options)
        g = RefGraph.on(net, {net.tap_ids[stage]: seen[stage]})
        cls = producer(g, net.tap_ids[stage], 0, 21, 9, w_fl=5, relu=False, in_fl=4, quant_input=True)
        seg = g.upsample(cls, 8, 'bilinear', label='seg')
        assert net.output_argmax(seg, 'u8') == 1
        for k, v in options.items():
            net.set_option(k, v)
        net.finalize(2)
        tok = 'argmax_u8:' if leg == 'unfused' else 'upsample_bilinear+argmax_u8:'
        assert [(t, k) for _, t, k in ac.argmax_lines(net)] == [(tok, ac.SYMBOL[tok])], net.describe()
        assert len(ac.upsample_lines(net)) == (1 if leg == 'unfused' else 0), net.describe()
        assert net.outputs[1] == (1, 64, 64, 0, False) and net.output_kinds == [1, 2]
        want = ac.argmax_ref(g.v[seg][0])
        assert np.unique(want).size >= 5
        got, classes = net.run(xt)
        net.check()
        assert classes.dtype == torch.uint8 and tuple(classes.shape) == (2, 64, 64)
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {leg}')
        np.testing.assert_array_equal(classes.cpu().numpy(), want, err_msg=f'class map {leg}')


def test_top1_of_resnet18_is_argmax_of_the_oracles_logits(dev):
    """The predicted class of a classifier: the argmax of the linear's result as output 1, [N] int32, next to the float logits."""
    spec = topology.get('resnet18')
    params = synth.make_params(spec, seed=5)
    x, x_fl = synth.make_input(spec, params, 3, 64, seed=9)
    logits = oracle.net_forward(spec, params, x, x_fl)
    net = record_net(spec, params, 64)
    fc = net.tap_ids['avgpool'] + 1                                # the classifier's result: the tensor recorded right behind the pooled vector
    assert net.tensor_info(fc)[:3] == (logits.shape[1], 1, 1)
    assert net.output_argmax(fc, 'i32') == 1
    net.finalize(3)
    got, top1 = net.run(torch.from_numpy(x).to(dev))
    net.check()
    assert top1.dtype == torch.int32 and top1.numel() == 3
    np.testing.assert_array_equal(got.cpu().numpy(), logits)
    np.testing.assert_array_equal(top1.cpu().numpy().reshape(-1), np.argmax(logits.astype(np.int64), axis=1))


@pytest.mark.parametrize('name', ['c21_7x7', 'c33_6x6', 'c256_2x2_i32'])
def test_torch_op_and_module(name, dev):
    """torch.ops.f8net.argmax_channels and ops.F8ArgMax against the same reference, on the ties and the all-negative data."""
    from f8net_amd import ops, torch_ops  # noqa: F401  (registers the op)
    c = ac.CASES[name]
    u8 = c['dtype'] == 'u8'
    for data in ('ties', 'neg', 'extremes'):
        g, t, x = ac.reference(name, data)
        want = ac.argmax_ref(g.v[t][0])
        xt = torch.from_numpy(x).to(dev)
        y = torch.ops.f8net.argmax_channels(xt, u8)
        assert y.dtype == (torch.uint8 if u8 else torch.int32) and tuple(y.shape) == want.shape
        np.testing.assert_array_equal(y.cpu().numpy(), want, err_msg=f'{name} {data}')
        z = ops.F8ArgMax(c['dtype'])(xt[:1])                       # another batch: the cached plan is reused or rebuilt, the map is the first image's
        np.testing.assert_array_equal(z.cpu().numpy(), want[:1], err_msg=f'{name} {data} module')


@pytest.mark.parametrize('dtype', ['u8', 'i32'])
def test_onnx_imported_segmentation_tail(dtype, dev):
    """A 1x1 classifier, bilinear x4 and ArgMax written as an ONNX file, imported, and planned through IntGraph.build_net: the fused launch, the
    reference's class map."""
    from f8net_amd import onnx_export, onnx_import
    ig, x, want = ac.seg_tail_int_graph(dtype)
    net = onnx_import.import_graph(onnx_export.export_graph(ig)).build_net(x.shape[0], input_fraclen=ac.X_FL)
    tok = f'upsample_bilinear+argmax_{dtype}:'
    assert [(t, k) for _, t, k in ac.argmax_lines(net)] == [(tok, ac.SYMBOL[tok])], net.describe()
    got = net.run(torch.from_numpy(x).to(dev))
    net.check()
    assert got.dtype == (torch.uint8 if dtype == 'u8' else torch.int32)
    np.testing.assert_array_equal(got.cpu().numpy().reshape(want.shape), want)
