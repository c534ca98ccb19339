"""Upsampling on the device, bit for bit against the reference of tests/upsample_cases.py (np.repeat; the integer bilinear weights on int64, wrapped
to int32): every case on both legs — option upsample_i8 = 1 (the byte copy where the plan allows it) and 0 (the int32 launch everywhere) — at N and
N - 1 images from one handle planned for N + 1, and with every fusing pass on; bench.py's pipelined schedule on two cases; a profiled run; a whole
DeepLabV3 head on resnet50_os16 (ASPP with its image-pooling branch, projection, classifier, logits back at the input size) next to the unchanged
logits; an FPN top-down step on two tapped ResNet-50 stage outputs; ONNX-imported graphs with a Resize through IntGraph.build_net.
tests/test_upsample_plan.py checks on the CPU which mode and kernel every case plans."""
import numpy as np
import pytest
import torch

import concat_cases as cc
import upsample_cases as uc
from f8net_amd import onnx_export, onnx_import, synth, topology
from f8net_amd.net import record_net
from graph_cases import run_case
from oracle import oracle
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(net, name, opts):
    c = uc.CASES[name]
    tok = c['tok'] if opts.get('upsample_i8', 1) else c['tok_off']
    assert [(t, k) for _, t, k in uc.upsample_lines(net)] == [(tok, uc.SYMBOL[tok])], net.describe()


@pytest.mark.parametrize('i8', [1, 0])
@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_every_case_on_both_legs(name, i8, dev):
    run_case(uc, name, dev, _check_plan, upsample_i8=i8)


@pytest.mark.parametrize('name', sorted(uc.CASES))
def test_every_case_with_all_fusions(name, dev):
    run_case(uc, name, dev, _check_plan, **uc.FUSE_ALL)


@pytest.mark.parametrize('name', ['n_3x5_two', 'b_3x5_k1'])
def test_pipelined_schedule(name, dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine runs."""
    c = uc.CASES[name]
    N = c['N']
    xs = [uc.make_input(name, N + 1)[:N]] + [uc.make_input(name, N + 1)[::-1][:N].copy(), np.roll(uc.make_input(name, N), 1, axis=2).copy()]
    g, outs, _ = uc.plan(name, xs[0], whole_batch_launches=1, arena_copies=3, pipeline_depth=3)
    ref, routs, _ = uc.reference(name)
    wants = [ref.v[routs[0]][0][:N]]
    for x in xs[1:]:
        gi, oi, _ = uc.build_graph(name, x, record=False)
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


def test_profiled_run_times_the_upsample_launch(dev):
    name = 'n_3x5_s35'
    x = uc.make_input(name)
    g, outs, _ = uc.plan(name, x)
    xt = torch.from_numpy(x).to(dev)
    y = g.net.run(xt)
    y2, ms = g.net.run_profiled(xt)
    assert torch.equal(y, y2) and len(ms) == g.net.num_launches
    (i, _, _), = uc.upsample_lines(g.net)
    assert ms[i] > 0.0
    g.net.check()


def test_deeplabv3_head_on_resnet50_os16(dev):
    """resnet50_os16 at 96 x 96 (stage 3 on a 6 x 6 map) with a whole DeepLabV3 head on the stage-3 output: the four ASPP conv branches of
    concat_cases.aspp_head, the image-pooling branch (average pool -> 1x1 conv -> nearest (6, 6): the broadcast), concat, projection, a 1x1
    classifier to 5 classes, bilinear x16 back to 96 x 96 as output 1.  The logits stay the plain net's bit for bit; the default and the all-fusions plan."""
    import dil_cases
    spec = topology.get('resnet50_os16')
    params = synth.make_params(spec, seed=31)
    x, x_fl = synth.make_input(spec, params, 2, 96, seed=3)
    last = spec.blocks[-1].name
    seen = {}
    tspec, tparams = dil_cases.stuffed_twin(spec, params)
    logits = oracle.net_forward(tspec, tparams, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, (v.copy(), fl)) if k == last else None)
    assert seen[last][0].shape[2:] == (6, 6)
    xt = torch.from_numpy(x).to(dev)
    for options in (None, uc.FUSE_ALL):
        net = record_net(spec, params, 96, options=options)
        g = RefGraph.on(net, {net.tap_ids[k]: v for k, v in seen.items()})
        t = net.tap_ids[last]
        bs = [uc.producer(g, t, 0, 64, 5, w_fl=5, relu=True, in_fl=4, quant_input=True)]
        bs += [uc.producer(g, t, 1 + k, 64, 5, w_fl=5, relu=True, in_fl=4, quant_input=True, kernel=3, dilation=d) for k, d in enumerate((6, 12, 18))]
        pooled = uc.producer(g, g.avgpool_sum(t), 7, 64, 5, w_fl=5, relu=True, in_fl=4, quant_input=True)
        assert g.v[pooled][0].shape[2:] == (1, 1)
        bs.append(g.upsample(pooled, (6, 6), 'nearest', label='aspp.pool'))
        cat = g.concat(bs, label='aspp.cat')
        proj = uc.producer(g, cat, 6, 64, 9, w_fl=5, relu=True, in_fl=4, quant_input=True)
        cls = uc.producer(g, proj, 8, 5, 9, w_fl=5, relu=False, in_fl=4, quant_input=True)
        seg = g.upsample(cls, 16, 'bilinear', label='seg')
        assert net.output(seg, as_float=False) == 1
        for k, v in (options or {}).items():
            net.set_option(k, v)
        net.finalize(2)
        assert [(tok, sym) for _, tok, sym in uc.upsample_lines(net)] == [(uc.I8, uc.SYMBOL[uc.I8]), (uc.B32, uc.SYMBOL[uc.B32])], net.describe()
        assert [tok for _, tok, _ in cc.concat_lines(net)] == [cc.I8], net.describe()
        assert net.output_info(1)[:3] == (5, 96, 96)
        want = g.v[seg][0]
        assert np.unique(want).size > 100 and np.unique(g.v[pooled][0]).size > 8
        got, head = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {options}')
        np.testing.assert_array_equal(head.cpu().numpy().reshape(want.shape), want, err_msg=f'head {options}')


def test_fpn_top_down_step_on_resnet50(dev):
    """ResNet-50 at 64 x 64: the outputs of stage 1 (512 x 8 x 8) and stage 2 (1024 x 4 x 4), tapped; a 1x1 to 64 channels on each, the coarser one
    upsampled (nearest x2) and joined with the lateral: output 1.  The logits stay the plain net's."""
    spec = topology.get('resnet50')
    params = synth.make_params(spec, seed=17)
    x, x_fl = synth.make_input(spec, params, 2, 64, seed=5)
    c3, c4 = 'stage_1_layer_3', 'stage_2_layer_5'
    seen = {}
    logits = oracle.net_forward(spec, params, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, (v.copy(), fl)) if k in (c3, c4) else None)
    assert seen[c3][0].shape[1:] == (512, 8, 8) and seen[c4][0].shape[1:] == (1024, 4, 4)
    xt = torch.from_numpy(x).to(dev)
    for options in (None, uc.FUSE_ALL):
        net = record_net(spec, params, 64, options=options)
        g = RefGraph.on(net, {net.tap_ids[k]: v for k, v in seen.items()})
        top = uc.producer(g, net.tap_ids[c4], 0, 64, 9, w_fl=5, relu=False, in_fl=4, quant_input=True)
        up = g.upsample(top, 2, 'nearest', label='p4.up')
        lateral = uc.producer(g, net.tap_ids[c3], 1, 64, 8, w_fl=4, relu=False, in_fl=4, quant_input=True)
        p3 = g.add(up, lateral)
        assert net.output(p3, as_float=False) == 1
        for k, v in (options or {}).items():
            net.set_option(k, v)
        net.finalize(2)
        assert [(tok, sym) for _, tok, sym in uc.upsample_lines(net)] == [(uc.N32, uc.SYMBOL[uc.N32])], net.describe()
        want = g.v[p3][0]
        assert np.unique(want).size > 100
        got, head = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {options}')
        np.testing.assert_array_equal(head.cpu().numpy().reshape(want.shape), want, err_msg=f'p3 {options}')


@pytest.mark.parametrize('name', ['n_unet_i8', 'b_fpn'])
def test_onnx_imported_graph_with_a_resize(name, dev):
    """The case written as an ONNX file (Resize; bilinear: Resize + Mul), imported, and planned through IntGraph.build_net."""
    ig, g, out = uc.int_graph(name)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    x = uc.make_input(name)
    want = g.v[out][0]
    net = back.build_net(x.shape[0], input_fraclen=uc.X_FL)
    c = uc.CASES[name]
    assert [(t, k) for _, t, k in uc.upsample_lines(net)] == [(c['tok'], uc.SYMBOL[c['tok']])]
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
    net.check()
    np.testing.assert_array_equal(got, want)
