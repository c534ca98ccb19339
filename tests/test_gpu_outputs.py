"""Several network outputs on the GPU: the copy-out kernel of outputs 1 .. (f8_tap.hip) at its corners, taps next to and inside fused launches,
whole nets through IntModel.forward_features, and the run plumbing (sub-batches, the float / uint8 entries, pipelined runs, a run that was not
given its buffers).  Every comparison is bit-exact against the CPU oracle; float outputs against `.astype(np.float32)` of the oracle's int32."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from f8net_amd import int_model, synth, topology
from f8net_amd.net import F8Net, build_net
from oracle import oracle

import outputs_cases as oc
from refgraph import RefGraph


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------ the kernel's corners
# map side, N, C: input [N, 32, side, side] -> 1x1 conv to C channels (tapped) -> 1x1 conv to 32 channels = output 0
CORNERS = [(7, 3, 40),     # 147 pixels: pixel blocks straddle images, ragged last block, channels padded 40 -> 64
           (1, 9, 32),     # one pixel per image
           (8, 5, 64),     # full blocks, image boundaries on block boundaries
           (6, 1, 96),     # 36 pixels: a single image and one ragged block
           (14, 2, 33)]    # one live channel in the second channel block


@functools.lru_cache(maxsize=None)
def _corner(side, N, C):
    """Weights, input and the oracle's two tensors.  Biases near +-2^30 (odd low bits): the tapped values need 31 bits, so int32 -> float32 rounds."""
    x = synth.rand_uniform_int(3, f'cx{side}.{N}.{C}', (N, 32, side, side), -127, 127).astype(np.int32)
    w1 = np.clip(synth.rand_normal_int(4, f'cw1.{C}', (C, 32, 1, 1), 40.0), -127, 127).astype(np.int32)
    sign = np.where(np.arange(C) % 2 == 0, 1, -1)
    b1 = (sign * (2 ** 30 + synth.rand_uniform_int(5, f'cb1.{C}', (C,), 0, 2 ** 20))).astype(np.int32) | 1
    w2 = np.clip(synth.rand_normal_int(6, f'cw2.{C}', (32, C, 1, 1), 40.0), -127, 127).astype(np.int32)
    b2 = synth.rand_normal_int(7, f'cb2.{C}', (32,), 2.0 ** 12).astype(np.int32)
    y1 = oracle.conv2d(oracle.requant(x, 6, 6, True), w1, b1, 1, 0)                      # fraclen 6 + 6
    y2 = oracle.conv2d(oracle.requant(y1, 0, 12, True), w2, b2, 1, 0)
    assert np.abs(y1).min() > 2 ** 29 and (y1.astype(np.float32).astype(np.int64) != y1).any()      # the conversion rounds
    return x, w1, b1, w2, b2, y1, y2


@pytest.mark.parametrize('tap_tiled', [1, 0])
@pytest.mark.parametrize('as_float', [0, 1])
@pytest.mark.parametrize('side, N, C', CORNERS, ids=lambda v: str(v))
def test_tap_kernel_corners(dev, side, N, C, as_float, tap_tiled):
    x, w1, b1, w2, b2, y1, y2 = _corner(side, N, C)
    net = F8Net().set_option('tap_tiled', tap_tiled)
    t = net.input(32, side, side, 6)
    c1 = net.conv(t, w1, b1, stride=1, pad=0, groups=1, weight_fl=6, input_fl=6, input_signed=True, relu=False)
    c2 = net.conv(c1, w2, b2, stride=1, pad=0, groups=1, weight_fl=6, input_fl=0, input_signed=True, relu=False)
    assert (net.output(c2, as_float=False), net.output(c1, as_float=bool(as_float))) == (0, 1)
    net.finalize(N)
    tap = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith('tap:')]
    assert len(tap) == 1
    assert net.launch_kernel(tap[0]) == (f'f8::tap_kernel<{"true" if as_float else "false"}>' if tap_tiled else 'f8::output_kernel')
    # the buffer is pre-filled and one image longer than the output: nothing is written past the last image
    guard = -7.0 if as_float else -7
    buf = torch.full((N + 1, C, side, side), guard, dtype=torch.float32 if as_float else torch.int32, device=dev)
    out0, out1 = net.run(_t(x, dev), outs=[buf[:N]])
    assert out1.shape == (N, C, side, side) and out1.dtype == (torch.float32 if as_float else torch.int32)
    np.testing.assert_array_equal(_np(out1), y1.astype(np.float32) if as_float else y1)
    np.testing.assert_array_equal(_np(out0).reshape(y2.shape), y2)
    assert (_np(buf[N]) == guard).all()


# ------------------------------------------------------------------------------------------ several taps at once
def _residual_net(x, taps):
    """input -> 3x3 conv, ReLU -> two residual blocks (3x3, ReLU, 1x1, join, ReLU) -> average pool -> linear = output 0 (int32);
    taps: indices into [first block's 3x3 conv, second block's join, pooled vector]."""
    C = 64
    w = lambda k, shape, sig: np.clip(synth.rand_normal_int(20 + k, f'rw{k}', shape, sig), -127, 127).astype(np.int32)
    b = lambda k, n, sig: synth.rand_normal_int(40 + k, f'rb{k}', (n,), sig).astype(np.int32)
    g = RefGraph(x, 6)
    t = g.conv(next(iter(g.v)), w(0, (C, x.shape[1], 3, 3), 20.0), b(0, C, 2.0 ** 10), pad=1, groups=1, weight_fl=6, input_fl=6, input_signed=True, relu=True)
    cand = []
    for k in range(2):
        a = g.conv(t, w(1 + 2 * k, (C, C, 3, 3), 8.0), b(1 + 2 * k, C, 2.0 ** 10), pad=1, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=True)
        p = g.conv(a, w(2 + 2 * k, (C, C, 1, 1), 12.0), b(2 + 2 * k, C, 2.0 ** 10), pad=0, groups=1, weight_fl=7, input_fl=5, input_signed=False, relu=False)
        t = g.add(p, t, relu=True)
        cand.append((a, t))
    pooled = g.avgpool_sum(t)
    out = g.linear(pooled, w(9, (10, C), 30.0), b(9, 10, 2.0 ** 12), weight_fl=6, input_fl=3, input_signed=False)
    g.net.output(out, as_float=False)
    ids = [cand[0][0], cand[1][1], pooled]
    for k in taps:
        g.net.output(ids[k], as_float=False)
    return g, out, [ids[k] for k in taps]


def test_conv_join_and_pooled_taps_in_one_run(dev):
    N = 3
    x = synth.rand_uniform_int(9, 'resx', (N, 32, 7, 7), -127, 127).astype(np.int32)
    plain, out, _ = _residual_net(x, ())
    plain.net.finalize(N)
    want0 = plain.v[out][0].reshape(N, -1)
    got_plain = _np(plain.net.run(_t(x, dev)))
    np.testing.assert_array_equal(got_plain, want0)
    g, out, ids = _residual_net(x, (0, 1, 2))
    g.net.finalize(N)
    res = g.net.run(_t(x, dev))
    assert len(res) == 4
    np.testing.assert_array_equal(_np(res[0]), got_plain)                       # output 0: the net planned without taps, bit for bit
    for r, t, info in zip(res[1:], ids, g.net.outputs[1:]):
        want, fl = g.v[t]
        assert info[:4] == want.shape[1:] + (fl,)
        assert np.unique(want).size > 8
        np.testing.assert_array_equal(_np(r), want)


# ------------------------------------------------------------------------------------------ taps inside fused plans
def _run_block_case(dev, case, options, expect_in_plain, expect_in_tapped=None):
    params, x = oc.case_data(case)
    want0, seen = oc.oracle_blocks(case['blocks'], params, x, case['x_fl'], tail=case['tail'], pre=case['pre'])
    kw = dict(tail=case['tail'], pre=case['pre'], options=options)
    plain = oc.record_blocks(case['blocks'], params, case['cin'], case['hw'], case['x_fl'], **kw).finalize(case['N'])
    if expect_in_plain:
        assert expect_in_plain in plain.describe(), plain.describe()
    net = oc.record_blocks(case['blocks'], params, case['cin'], case['hw'], case['x_fl'], taps=case['taps'], **kw).finalize(case['N'])
    if expect_in_tapped:
        assert expect_in_tapped in net.describe(), net.describe()
    xt = _t(x, dev)
    got_plain = _np(plain.run(xt))
    res = net.run(xt)
    net.check()
    np.testing.assert_array_equal(got_plain.reshape(want0.shape), want0)
    np.testing.assert_array_equal(_np(res[0]), got_plain)                       # output 0 is unchanged by the taps
    for name, r, info in zip(case['taps'], res[1:], net.outputs[1:]):
        want, fl = seen[name]
        assert info[3] == fl and np.unique(want).size > 8
        np.testing.assert_array_equal(_np(r), want, err_msg=name)


def test_taps_in_and_behind_a_stage_chain(dev):
    """CHAINS[0] of tests/test_gpu_chain.py: a tap on block 0 cuts the three-block chain there, the tap on block 2 sits at the end of the rest."""
    _run_block_case(dev, oc.bottleneck_chain(), None, 'stage_chain_x3', 'stage_chain_x2:s.1.body.0..s.2.body.4')


@pytest.mark.parametrize('fuse_irchain', [0, 1])
def test_taps_on_two_inverted_residuals(dev, fuse_irchain):
    _run_block_case(dev, oc.inverted_residual_pair(), {'fuse_irchain': fuse_irchain}, 'ir_chain_x2' if fuse_irchain else None)


@pytest.mark.parametrize('fuse_dws, fuse_ir', [(0, 0), (1, 0), (0, 1)])
def test_taps_on_a_depthwise_separable_pair(dev, fuse_dws, fuse_ir):
    """fuse_ir = 1 (the default): without taps the inverted-residual launch takes 1x1 -> depthwise -> 1x1 ACROSS the two blocks, and the tap on the
    first block's output has to cut it; fuse_ir = 0 leaves the pair to fuse_dws."""
    expect = 'fused_dws:dws.1' if fuse_dws else ('fused_ir_s1_R7:dws.0.body.2+dws.1.body.0+dws.1.body.2' if fuse_ir else None)
    _run_block_case(dev, oc.depthwise_separable_pair(), {'fuse_dws': fuse_dws, 'fuse_ir': fuse_ir}, expect)


# ------------------------------------------------------------------------------------------ whole nets
def _oracle_features(spec, params, x, fl):
    """(logits, {name: (value behind the ReLU, fraclen)}) with the pooled vector as 'avgpool'."""
    relu_keys = {c.key for c in spec.convs() if c.relu}
    seen = {}

    def tap(name, v, f):
        seen[name] = (oracle.relu(v) if name in relu_keys else v.copy(), f)

    logits = oracle.net_forward(spec, params, x, fl, tap=tap)
    last, lfl = seen[spec.tail.key if spec.tail is not None else spec.blocks[-1].name]
    seen['avgpool'] = (oracle.avgpool_sum(last)[:, :, None, None], lfl + 6)
    return logits, seen


def _feature_names(spec):
    return (['head.maxpool'] if spec.head_maxpool else []) + oc.stage_taps(spec) + ['avgpool']


def _check_features(feats, seen, names):
    assert list(feats) == list(names)
    for name in names:
        want, fl = seen[name]
        assert feats[name].output_fraclen == fl and feats[name].dtype == torch.int32
        np.testing.assert_array_equal(_np(feats[name]), want, err_msg=name)


@pytest.mark.parametrize('arch', ['resnet18', 'resnet50', 'mobilenet_v1', 'mobilenet_v2'])
def test_whole_net_features(dev, arch):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=5)
    x, fl = synth.make_input(spec, params, 2, 64, seed=9)
    want, seen = _oracle_features(spec, params, x, fl)
    m = int_model.from_params(spec, params).to(dev)
    xt = _t(x, dev)
    setattr(xt, 'output_fraclen', fl)
    plain = _np(m(xt))
    np.testing.assert_array_equal(plain, want)
    names = _feature_names(spec)
    for k in range(0, len(names), 7):                       # a net has at most 7 further outputs (MobileNet-V2: 7 stages + the pooled vector)
        part = names[k:k + 7]
        logits, feats = m.forward_features(xt, part)
        np.testing.assert_array_equal(_np(logits), plain)   # the logits equal forward's
        _check_features(feats, seen, part)
    assert m.plan(64, 2, dev, taps=names[:7]) is m.plan(64, 2, dev, taps=tuple(names[:7])) and m.plan(64, 2, dev) is not m.plan(64, 2, dev, taps=names[:7])


def test_resnet50_stage_outputs_behind_the_stage_chains(dev):
    """224 x 224 is the only size at which the taps sit behind the stage-chain launches."""
    spec = topology.get('resnet50', normalize=True)
    params = synth.make_params(spec, seed=5, fraclens=topology.R50_NVIDIA_FRACLENS)
    x, fl = synth.make_input(spec, params, 1, 224, seed=9)
    want, seen = _oracle_features(spec, params, x, fl)
    m = int_model.from_params(spec, params).to(dev)
    names = oc.stage_taps(spec)
    plan = m.plan(224, 1, dev, taps=names).describe()
    assert plan.count('stage_chain_x') == 4 and plan.count(' tap:') == 4, plan
    xt = _t(x, dev)
    setattr(xt, 'output_fraclen', fl)
    logits, feats = m.forward_features(xt, names)
    np.testing.assert_array_equal(_np(logits), want)
    _check_features(feats, seen, names)


# ------------------------------------------------------------------------------------------ run plumbing
PLUMBING_TAPS = ('head.maxpool', 'stage_1_layer_1', 'avgpool')


@pytest.fixture(scope='module')
def r18():
    """ResNet-18 at 64 x 64, N = 5, on uint8 pixels: the oracle's logits and features, once."""
    spec = topology.get('resnet18')
    params = synth.make_params(spec, seed=5)
    u8 = synth.rand_uniform_int(13, 'pixels', (2, 5, 3, 64, 64), 0, 255).astype(np.uint8)
    ref = [_oracle_features(spec, params, u.astype(np.int32), 8) for u in u8]
    return spec, params, u8, ref


def _check_run(res, ref):
    want, seen = ref
    assert len(res) == 1 + len(PLUMBING_TAPS)
    np.testing.assert_array_equal(_np(res[0]), want)
    for name, r in zip(PLUMBING_TAPS, res[1:]):
        np.testing.assert_array_equal(_np(r), seen[name][0], err_msg=name)


@pytest.mark.parametrize('split', [2, 3])
def test_uneven_sub_batches(dev, r18, split):
    spec, params, u8, ref = r18
    net = build_net(spec, params, max_batch=5, hw=64, taps=PLUMBING_TAPS, options={'split': split})
    assert net.num_parts(5) == split
    _check_run(net.run(_t(u8[0].astype(np.int32), dev)), ref[0])
    res, ms = net.run_profiled(_t(u8[1].astype(np.int32), dev))
    assert len(ms) == net.num_launches
    _check_run(res, ref[1])


def test_float_and_uint8_entries_and_the_torch_op(dev, r18):
    spec, params, u8, ref = r18
    net = build_net(spec, params, max_batch=5, hw=64, taps=PLUMBING_TAPS)
    _check_run(net.run_u8(_t(u8[0], dev)), ref[0])
    img = u8[1].astype(np.float32) / np.float32(255.0)
    xi, fl = oracle.quantize_input_u8(img)
    assert fl == 8 and (xi == u8[1]).all()
    _check_run(net.run_f32(_t(img, dev), normalize=False), ref[1])
    from f8net_amd import torch_ops
    h = torch_ops.register_net(net)
    try:
        res = torch.ops.f8net.net_forward_taps(_t(u8[0].astype(np.int32), dev), h)
    finally:
        torch_ops.unregister_net(h)
    assert isinstance(res, (list, tuple))
    _check_run(res, ref[0])


def test_two_pipelined_runs_with_rotating_buffers(dev, r18):
    spec, params, u8, ref = r18
    net = build_net(spec, params, max_batch=5, hw=64, taps=PLUMBING_TAPS)
    xs = [_t(u.astype(np.int32), dev) for u in u8]
    outs0 = [torch.empty((5, spec.num_classes), dtype=torch.float32, device=dev) for _ in range(2)]
    outs = [[torch.empty((5,) + info[:3], dtype=torch.int32, device=dev) for info in net.outputs[1:]] for _ in range(2)]
    net.upload()
    torch.cuda.synchronize()                                # inputs and buffers are ready one call early
    net.set_pipelined(1)
    res = [net.run(xs[i], out=outs0[i], outs=outs[i]) for i in range(2)]
    torch.cuda.synchronize()
    net.set_pipelined(0)
    for i in range(2):
        assert res[i][1].data_ptr() == outs[i][0].data_ptr()
        _check_run(res[i], ref[i])


def test_a_run_without_its_buffers_is_refused(dev, r18):
    spec, params, u8, ref = r18
    net = build_net(spec, params, max_batch=5, hw=64, taps=PLUMBING_TAPS)
    x = _t(u8[0].astype(np.int32), dev)
    out = torch.full((5, spec.num_classes), -1.0, dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert net._L.f8_net_run(net._h, x.data_ptr(), out.data_ptr(), 5, stream) == -5       # F8_ERR_STATE
    torch.cuda.synchronize()
    assert (_np(out) == -1.0).all()                         # nothing was issued
    _check_run(net.run(x), ref[0])
    assert net._L.f8_net_run(net._h, x.data_ptr(), out.data_ptr(), 5, stream) == -5       # one-shot: the buffers of the run above are spent
    _check_run(net.run(x, out=out), ref[0])
