"""Rectangular convolutions on the device, bit for bit against the reference of tests/rect_cases.py (the CPU oracle behind an explicit zero pad): every
plain case on conv_igemm_kernel, every depthwise strip on dwstrip_dot4_kernel and — `dwk_dot4 = 0` — on dwconvk_kernel, the two legs against each other;
igemm_tile 1 .. 4; one handle at several batch sizes; bench.py's pipelined schedule; an Inception-v3 17x17 module (also through ONNX), an ERFNet
non-bottleneck-1D block, a SegNeXt MSCA block and a SAME-padded MobileNet stem, on the default plan and with every fusing pass on; the op-level drop-ins.
tests/test_rect_plan.py checks on the CPU that every case is live on the reference's values."""
import numpy as np
import pytest
import torch

import rect_cases
from f8net_amd import onnx_export, onnx_import, synth
from rect_cases import _b, _w

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _run(name, case, dev, batches=None, dot4=True, tile=None, **opts):
    """Plans the case, checks its rectangular launches against the hand-written table and every batch against the shared reference; returns the last output."""
    n_max = case.get('max_batch') or case['N']
    x = rect_cases.make_input(name, case, n_max)
    g, out, _ = rect_cases.plan(name, case, x, **opts)
    assert rect_cases.r_lines(g.net, case) == rect_cases.expect(case, dot4=dot4, tile=tile), g.net.describe()
    ref, rout, _ = rect_cases.reference(name)
    want = ref.v[rout][0]
    xt = torch.from_numpy(x).to(dev)
    got = None
    for n in batches or [n_max]:
        got = g.net.run(xt[:n]).cpu().numpy().reshape((n,) + want.shape[1:])
        np.testing.assert_array_equal(got, want[:n], err_msg=f'{name} {opts} n={n}')
    g.net.check()
    return got


@pytest.mark.parametrize('name', sorted(rect_cases.PLAIN))
def test_plain_geometry(name, dev):
    _run(name, rect_cases.PLAIN[name], dev)


@pytest.mark.parametrize('name', sorted(rect_cases.PLAIN_FORMATS))
def test_plain_formats(name, dev):
    _run(name, rect_cases.PLAIN_FORMATS[name], dev)


@pytest.mark.parametrize('name', sorted(rect_cases.PLAIN_RES))
def test_plain_with_the_fused_residual_join(name, dev):
    _run(name, rect_cases.PLAIN_RES[name], dev)


@pytest.mark.parametrize('tile', sorted(rect_cases.TILES))
def test_every_igemm_tile(tile, dev):
    _run(rect_cases.TILE_CASE, rect_cases.ALL[rect_cases.TILE_CASE], dev, tile=rect_cases.TILES[tile], igemm_tile=tile)


@pytest.mark.parametrize('name', sorted(rect_cases.DW))
def test_depthwise_strips_on_both_kernels(name, dev):
    """The dot4 kernel, then the scalar kernel (dwk_dot4 = 0) on the same graph and input; both against the reference, hence against each other."""
    a = _run(name, rect_cases.DW[name], dev)
    b = _run(name, rect_cases.DW[name], dev, dot4=False, dwk_dot4=0)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('name', sorted(rect_cases.DW_GENERIC))
def test_depthwise_stride_2_and_the_int32_form_run_the_scalar_kernel(name, dev):
    case = rect_cases.DW_GENERIC[name]
    assert all(k.startswith('f8::dwconvk_kernel<') for _, k in rect_cases.expect(case))      # (asserted by symbol against the plan in _run)
    _run(name, case, dev)


@pytest.mark.parametrize('name', sorted(rect_cases.MAX_BATCH))
def test_fewer_images_than_max_batch(name, dev):
    """Planned for 8 images; 3 images (sub-batches of 2 and 1), then 8 from the same handle."""
    _run(name, rect_cases.MAX_BATCH[name], dev, batches=[3, 8])


@pytest.mark.parametrize('name', sorted(rect_cases.PIPELINED))
def test_pipelined_schedule(name, dev):
    """bench.py's schedule on 1x7 -> 7x1: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating over nine
    runs; every output against the reference."""
    case = rect_cases.PIPELINED[name]
    xs = [rect_cases.make_input(name, case)] + [rect_cases.make_input(f'{name}{i}', case) for i in (1, 2)]
    g, out, _ = rect_cases.plan(name, case, xs[0])
    assert rect_cases.r_lines(g.net, case) == rect_cases.expect(case), g.net.describe()
    ref, rout, _ = rect_cases.reference(name)
    wants = [ref.v[rout][0]]
    for x in xs[1:]:
        gi, oi, _ = rect_cases.build_graph(case, x, record=False)
        wants.append(gi.v[oi][0])
    xt = [torch.from_numpy(x).to(dev) for x in xs]
    outs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=outs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(outs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    g.net.check()


# ---- graphs.  Conventions of the case table: weights 150 / sqrt(taps x cin_g), biases _b(., 2^9, 2^13).  A conv on the net input (fraclen 8, read as it
# is) has its weights at fraclen 5: its result is at 13.  Every inner conv reads its source at fraclen 4 (shift 9) with weights at 9: 13 again.
FIRST = dict(input_fl=8, quant_input=False, w_fl=5)


def _cv(g, t, seed, cout, cin, kh, kw, pads, *, groups=1, stride=1, d=1, relu=True, input_fl=4, quant_input=True, w_fl=9, b_mean=2.0 ** 13):
    w = _w(seed, (cout, cin // groups, kh, kw), 150.0 / (kh * kw * (cin // groups)) ** 0.5)
    return g.conv_rect(t, w, _b(seed + 100, cout, 2.0 ** 9, b_mean), stride=stride, pads=pads, groups=groups, weight_fl=w_fl, input_fl=input_fl,
                       input_signed=False, relu=relu, quant_input=quant_input, dilation=d)


def inception_17(g, x):
    """Inception-v3's 17 x 17 module on 64 channels: 1x1 | 1x1 -> 1x7 -> 7x1 | 1x1 -> 7x1 -> 1x7 -> 7x1 -> 1x7 | 3x3 / 1 / pad 1 sum-pool -> 1x1; concat."""
    b1 = _cv(g, x, 1, 64, 64, 1, 1, 0, **FIRST)
    b2 = _cv(g, x, 2, 64, 64, 1, 1, 0, **FIRST)
    b2 = _cv(g, _cv(g, b2, 3, 64, 64, 1, 7, (0, 3)), 4, 64, 64, 7, 1, (3, 0))
    b3 = _cv(g, x, 5, 64, 64, 1, 1, 0, **FIRST)
    for seed, (kh, kw) in zip((6, 7, 8, 9), ((7, 1), (1, 7), (7, 1), (1, 7))):
        b3 = _cv(g, b3, seed, 64, 64, kh, kw, (kh // 2, kw // 2))
    b4 = _cv(g, g.avgpool(x, 3, 1, 1), 10, 64, 64, 1, 1, 0, input_fl=8, w_fl=5)      # the window's sum is at fraclen 11: shift 3
    return g.concat([b1, b2, b3, b4])


def erfnet_nb1d(g, x):
    """ERFNet's non-bottleneck-1D block: 3x1 -> 1x3 -> 3x1 d2 -> 1x3 d2, joined with the block input (a 1x1's result at fraclen 13), ReLU."""
    pre = _cv(g, x, 1, 64, 64, 1, 1, 0, b_mean=2.0 ** 12, **FIRST)
    t = _cv(g, pre, 2, 64, 64, 3, 1, (1, 0))
    t = _cv(g, t, 3, 64, 64, 1, 3, (0, 1))
    t = _cv(g, t, 4, 64, 64, 3, 1, (2, 0), d=2)
    t = _cv(g, t, 5, 64, 64, 1, 3, (0, 2), d=2, relu=False)
    return g.add(t, pre, relu=True)


def segnext_msca(g, x):
    """SegNeXt's MSCA on 32 channels: depthwise 5x5; the strip pairs 1x7 -> 7x1, 1x11 -> 11x1, 1x21 -> 21x1 on its result; their sum with it (f8_net_add);
    a 1x1; f8_net_mul with the block input."""
    C = 32
    u = _cv(g, x, 1, C, C, 1, 1, 0, b_mean=2.0 ** 12, **FIRST)                                        # fraclen 13
    attn = _cv(g, u, 2, C, C, 5, 5, 2, groups=C, relu=False)
    s = attn
    for seed, k in ((3, 7), (5, 11), (7, 21)):
        b = _cv(g, attn, seed, C, C, 1, k, (0, k // 2), groups=C, relu=False)
        b = _cv(g, b, seed + 1, C, C, k, 1, (k // 2, 0), groups=C, relu=False)
        s = g.add(s, b)
    a = _cv(g, s, 9, C, C, 1, 1, 0, relu=False, input_fl=2, b_mean=0.0)                               # the sum of four: two more bits (shift 11); fraclen 11
    return g.mul(a, u, a_fl=2, a_signed=True, b_fl=4, b_signed=False)


def same_stem(g, x):
    """A TF-exported MobileNet head: 3x3 / 2 with SAME pads (0, 0, 1, 1) on 3 channels -> depthwise 3x3 -> 1x1."""
    t = _cv(g, x, 1, 32, 3, 3, 3, (0, 0, 1, 1), stride=2, **FIRST)
    t = _cv(g, t, 2, 32, 32, 3, 3, 1, groups=32)
    return _cv(g, t, 3, 64, 32, 1, 1, 0)


GRAPHS = {'inception_17': (inception_17, (64, 9, 9), ('conv1x7s1_t', 'conv7x1s1_t', 'concat')),
          'erfnet_nb1d': (erfnet_nb1d, (64, 10, 12), ('conv3x1s1_t', 'conv1x3s1_t', 'conv3x1s1d2_t', 'conv1x3s1d2_t64x64x64_res')),
          'segnext_msca': (segnext_msca, (32, 12, 12), ('dwconv1x7s1:', 'dwconv7x1s1:', 'dwconv1x11s1:', 'dwconv11x1s1:', 'dwconv1x21s1:', 'dwconv21x1s1:', 'mul')),
          'same_stem': (same_stem, (3, 16, 16), ('conv3x3s2_t',))}


@pytest.mark.parametrize('fuse', [False, True])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_graphs(name, fuse, dev):
    build, shape, tokens = GRAPHS[name]
    x = synth.rand_uniform_int(7, f'rect_g_{name}', (3,) + shape, 0, 255).astype(np.int32)
    g = rect_cases.RectGraph(x, 8)
    out = build(g, next(iter(g.v)))
    g.net.output(out, as_float=False)
    for k, v in (rect_cases.FUSE_ALL if fuse else {}).items():
        g.net.set_option(k, v)
    g.net.finalize(3)
    d = g.net.describe()
    assert all(t in d for t in tokens), d
    want = g.v[out][0]
    assert np.unique(want).size > 16 and (want != 0).mean() > 0.25, name
    got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
    np.testing.assert_array_equal(got, want, err_msg=f'{name} fuse={fuse}')
    g.net.check()


def test_the_inception_module_through_onnx(dev):
    """export -> import: equal describe(), equal IntOp fields, equal output."""
    x = synth.rand_uniform_int(7, 'rect_g_inception_17', (3, 64, 9, 9), 0, 255).astype(np.int32)
    ig, g, out = rect_cases.record_int_graph(x, 8, inception_17)
    want = g.v[out][0]
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    assert len(back.ops) == len(ig.ops)
    for a, b in zip(ig.ops, back.ops):
        assert (a.kind, a.src, a.rect, a.kernel, a.stride, a.pad, a.dilation, a.groups, a.shift, a.relu, a.srcs) == \
               (b.kind, b.src, b.rect, b.kernel, b.stride, b.pad, b.dilation, b.groups, b.shift, b.relu, b.srcs), (a, b)
        if a.kind == 'conv':
            np.testing.assert_array_equal(a.weight, b.weight)
            np.testing.assert_array_equal(a.bias, b.bias)
    na, nb = ig.build_net(3), back.build_net(3)
    assert na.describe() == nb.describe() and 'conv1x7s1_t' in na.describe() and 'conv7x1s1_t' in na.describe(), na.describe()
    xt = torch.from_numpy(x).to(dev)
    for net in (na, nb):
        np.testing.assert_array_equal(net.run(xt).cpu().numpy().reshape(want.shape), want)
        net.check()


@pytest.mark.parametrize('C, G, kh, kw, stride, pads, d', [(40, 1, 1, 7, (1, 1), (0, 3, 0, 3), 1), (64, 1, 3, 3, (2, 2), (0, 0, 1, 1), 1),
                                                           (32, 1, 3, 1, (2, 1), (2, 0, 2, 0), 2), (40, 40, 21, 1, (1, 1), (10, 0, 10, 0), 1)])
def test_op_level_conv2d_rect(dev, C, G, kh, kw, stride, pads, d):
    """torch.ops.f8net.conv2d_rect on int32 NCHW device tensors; the meta function gives the same shape."""
    x = synth.rand_uniform_int(11, f'rop_x{C}', (3, C, 9, 11), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(12, f'rop_w{C}{G}{kh}{kw}', (C, C // G, kh, kw), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(13, f'rop_b{C}', (C,), 3e5).astype(np.int32)
    from f8net_amd import torch_ops  # noqa: F401  (registers the ops)
    xt, wt, bt = (torch.from_numpy(a).to(dev) for a in (x, w, b))
    got = torch.ops.f8net.conv2d_rect(xt, wt, bt, list(stride), list(pads), G, 6, 5, False, d).cpu().numpy()
    want = rect_cases.rect_conv_ref(x, w, b, stride, pads, G, d)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    meta = torch.ops.f8net.conv2d_rect(xt.to('meta'), wt.to('meta'), bt.to('meta'), list(stride), list(pads), G, 6, 5, False, d)
    assert tuple(meta.shape) == want.shape


def test_f8conv2d_takes_tuple_arguments(dev):
    from f8net_amd import ops
    x = synth.rand_uniform_int(11, 'rop_x40', (3, 40, 9, 11), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(12, 'rmod_w', (72, 40, 1, 7), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(13, 'rmod_b', (72,), 3e5).astype(np.int32)
    conv = ops.F8Conv2d(40, 72, kernel_size=(1, 7), padding=(0, 3))
    conv.weight.data, conv.bias.data = torch.from_numpy(w), torch.from_numpy(b)
    conv.input_fraclen.fill_(5)
    conv.weight_fraclen.fill_(6)
    got = conv(torch.from_numpy(x).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got, rect_cases.rect_conv_ref(x, w, b, 1, (0, 3, 0, 3), 1))
    d2 = ops.F8Conv2d(40, 72, kernel_size=(3, 1), padding=(2, 0), dilation=(2, 1), stride=(2, 1))
    w2 = synth.rand_uniform_int(12, 'rmod_w2', (72, 40, 3, 1), -127, 127).astype(np.int32)
    d2.weight.data, d2.bias.data = torch.from_numpy(w2), torch.from_numpy(b)
    d2.input_fraclen.fill_(5)
    d2.weight_fraclen.fill_(6)
    got = d2(torch.from_numpy(x).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got, rect_cases.rect_conv_ref(x, w2, b, (2, 1), (2, 0, 2, 0), 1, 2))
