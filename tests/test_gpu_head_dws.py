"""fuse_head_dws: MobileNet-V1's head conv and first depthwise-separable block in one launch (f8_head_dws.hip), bit for bit against the CPU
oracle (op by op and whole nets), the reference goldens and the option-0 plan of the same parameters."""
import functools
import os

import numpy as np
import pytest
import torch

from f8net_amd import synth, topology
from ir_cases import _b, _w
from oracle import oracle
from refgraph import RefGraph

pytestmark = pytest.mark.gpu

FUSED = 'head3x3s2+dw3x3+1x1:'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _fused(net):
    return [i for i in range(net.num_launches) if net.launch_info(i, 1)[0].startswith(FUSED)]


# Formats: the input is fraclen 8 unsigned (pixel values 0 .. 255) or fraclen 6 signed; head weights fraclen 6 -> the depthwise conv's unsigned
# fraclen-6 input is a right shift by 8 (6); depthwise weights fraclen 6 -> the 1x1's unsigned fraclen-6 input: a shift by 6; 1x1 weights fraclen 6
# -> a reader of fraclen f shifts by 12 - f.  Weight and bias spreads keep the 8-bit values spread over their range without saturating everywhere.
def _graph(x, x_signed, cout, relu, readers, big):
    """raw input -> 3x3 / 2 head conv (ReLU) -> depthwise 3x3 (ReLU) -> 1x1 [ReLU] -> one 32-output 1x1 reader per (fl, signed), summed (int32)."""
    cin = x.shape[1]
    x_fl = 6 if x_signed else 8
    g = RefGraph(x, x_fl)
    t = next(iter(g.v))
    bd, bp = _b(40, 32, 2.0 ** 9), _b(60, cout, 2.0 ** 11)
    if big:                                                         # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
        bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
        bp[5], bp[min(20 + 32, cout - 1)] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
    h = g.conv(t, _w(20, (32, cin, 3, 3), 25.0 * (3.0 / cin) ** 0.5), _b(21, 32, 2.0 ** 11), stride=2, pad=1, groups=1, weight_fl=6, input_fl=x_fl,
               input_signed=x_signed, relu=True)
    d = g.conv(h, _w(30, (32, 1, 3, 3), 25.0), bd, stride=1, pad=1, groups=32, weight_fl=6, input_fl=6, input_signed=False, relu=True)
    p = g.conv(d, _w(50, (cout, 32, 1, 1), 10.0), bp, pad=0, groups=1, weight_fl=6, input_fl=6, input_signed=False, relu=relu)
    out = None
    for k, (fl, sgn) in enumerate(readers):
        c = g.conv(p, _w(90 + k, (32, cout, 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, relu=False)
        out = c if out is None else g.add(out, c)
    g.net.output(out, as_float=False)
    return g, out


def _input(H, W, N, cin=3, signed=False):
    lo, hi = (-127, 127) if signed else (0, 255)
    return synth.rand_uniform_int(5, f'x{H}x{W}', (N, cin, H, W), lo, hi).astype(np.int32)


def _run_case(dev, H, W, N, cout=64, relu=True, readers=((6, False),), opts=None, big=False, cin=3, signed=False, kinds=False):
    """Plans the graph with fuse_head_dws 1 and 0, checks the fused line (and its kernel) / its absence, compares both plans with the oracle."""
    x = _input(H, W, N, cin, signed)
    for on in (1, 0):
        g, out = _graph(x, signed, cout, relu, readers, big)
        g.net.set_option('fuse_head_dws', on)
        for k, v in (opts or {}).items():
            g.net.set_option(k, v)
        g.net.finalize(N)
        idx = _fused(g.net)
        assert len(idx) == on, g.net.describe()
        if on:
            assert g.net.launch_kernel(idx[0]) == 'f8::head_dws_kernel'
            assert (g.net.launch_info(0, 1)[0] == 'input(read by the stem launch)') == (cin == 3)
        want = g.v[out][0]
        assert np.unique(want).size > 8
        got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
        np.testing.assert_array_equal(got, want, err_msg=f'fuse_head_dws={on}')
        if kinds and on:
            # the other kinds of raw input: fp32 quantised by the loader waves, uint8 planes through the table, uint8 NHWC through the input launch
            # and the haloed form; the oracle ran on the quantised input
            u8 = x.astype(np.uint8)
            f = (u8.astype(np.float32) / np.float32(255.0)).astype(np.float32)
            xq, fl = oracle.quantize_input_u8(f)
            np.testing.assert_array_equal(xq, x)
            assert fl == 8
            got = g.net.run_f32(torch.from_numpy(f).to(dev), normalize=False).cpu().numpy().reshape(want.shape)
            np.testing.assert_array_equal(got, want, err_msg='run_f32')
            got = g.net.run_u8(torch.from_numpy(u8).to(dev)).cpu().numpy().reshape(want.shape)
            np.testing.assert_array_equal(got, want, err_msg='run_u8 NCHW')
            got = g.net.run_u8(torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).to(dev), nhwc=True).cpu().numpy().reshape(want.shape)
            np.testing.assert_array_equal(got, want, err_msg='run_u8 NHWC')


# input H x W, N (output map H / 2 x W / 2: bands of 14 rows split in two half-bands, strips of 28 columns)
SHAPES = {
    'minimal': (8, 8, 1),                # one strip, one band, rows and columns both at the border
    'ragged_band_two_strips': (32, 60, 2),   # P = 16: bands of 14 + 2 (an empty second half-band); Q = 30: a second strip with two live lanes
    'three_bands_three_strips': (60, 120, 3),   # persistent walk over 9 band tiles; strip seams under the DPP shifts
    'full_width': (8, 224, 1),           # four full strips
}


@pytest.mark.parametrize('case', sorted(SHAPES))
def test_shapes(case, dev):
    H, W, N = SHAPES[case]
    _run_case(dev, H, W, N)


def test_input_kinds(dev):
    _run_case(dev, 32, 60, 2, kinds=True)


def test_cout_48_pads_the_second_tile(dev):
    _run_case(dev, 32, 60, 1, cout=48)


def test_cout_32_with_relu(dev):
    _run_case(dev, 32, 60, 1, cout=32)


def test_no_relu_signed_reader(dev):
    _run_case(dev, 32, 60, 1, relu=False, readers=((5, True),))


def test_relu_signed_reader_floors_the_accumulators(dev):
    _run_case(dev, 32, 60, 1, relu=True, readers=((5, True),))


def test_two_reader_formats(dev):
    _run_case(dev, 32, 60, 1, readers=((6, False), (5, True)))


@pytest.mark.parametrize('cin,signed', [(1, False), (4, False), (4, True)], ids=['cin1', 'cin4', 'cin4_signed'])
def test_head_input_channels(cin, signed, dev):
    _run_case(dev, 16, 16, 1, cin=cin, signed=signed)


@pytest.mark.parametrize('rq', [0, 1])
def test_rounding_add_wraps(rq, dev):
    """Depthwise and 1x1 biases next to 2^31: the planner cannot bound the accumulators, the launch takes its integer form by itself."""
    _run_case(dev, 32, 60, 1, big=True, opts={'requant_float': rq})


def test_requant_float(dev):
    _run_case(dev, 32, 60, 1, opts={'requant_float': 1})


# ---- whole nets
def _build(spec, params, n, hw, **opts):
    from f8net_amd.net import build_net
    net = build_net(spec, params, max_batch=n, hw=hw, options=dict(opts, fuse_head_dws=1))
    assert len(_fused(net)) == 1, net.describe()
    return net


@pytest.mark.parametrize('more', [{}, {'fuse_dws': 1, 'fuse_dws7': 1}], ids=['alone', 'with_fuse_dws_and_dws7'])
def test_reference_goldens(more, golden_dir, dev):
    g = np.load(os.path.join(golden_dir, 'net_mobilenet_v1.npz'))
    spec = topology.get('mobilenet_v1', normalize=bool(g['normalize']))
    params = synth.reference_params(spec, seed=1234)
    for hw, n in ((64, 2), (224, 1)):
        x, _ = synth.make_input(spec, params, n, hw, seed=7)
        net = _build(spec, params, n, hw, **more)
        got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
        np.testing.assert_array_equal(got, g[f's1234_hw{hw}_n{n}/logits'], err_msg=f'hw{hw}')


def test_mobilenet_v2_unchanged(golden_dir, dev):
    from f8net_amd.net import build_net
    g = np.load(os.path.join(golden_dir, 'net_mobilenet_v2.npz'))
    spec = topology.get('mobilenet_v2', normalize=bool(g['normalize']))
    params = synth.reference_params(spec, seed=1234)
    x, _ = synth.make_input(spec, params, 2, 64, seed=7)
    net = build_net(spec, params, max_batch=2, hw=64, options={'fuse_head_dws': 1})
    idx = _fused(net)
    assert len(idx) == 1 and net.launch_kernel(idx[0]) == 'f8::stem_rows_kernel'
    np.testing.assert_array_equal(net.run(torch.from_numpy(x).to(dev)).cpu().numpy(), g['s1234_hw64_n2/logits'])


@functools.lru_cache(maxsize=None)
def _fresh(n):
    spec = topology.get('mobilenet_v1', normalize=True)
    params = synth.make_params(spec, seed=301)
    x, x_fl = synth.make_input(spec, params, n, 224, seed=3)
    want = oracle.net_forward(spec, params, x, x_fl)
    want.setflags(write=False)
    return spec, params, x, want


def test_fresh_seed_against_the_oracle(dev):
    """N = 5 at 224: 5 x 8 = 40 band tiles walked by fewer workgroups' XCD groups than a multiple of eight would give."""
    from f8net_amd.net import build_net
    spec, params, x, want = _fresh(5)
    net = _build(spec, params, 5, 224)
    xt = torch.from_numpy(x).to(dev)
    got = net.run(xt).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, build_net(spec, params, max_batch=5, hw=224, options={'fuse_head_dws': 0}).run(xt).cpu().numpy())


def test_pipelined_three_batches_in_flight(dev):
    from f8net_amd.net import build_net
    spec, params, x, want = _fresh(5)
    n = 3
    opts = {'whole_batch_launches': 1, 'arena_copies': 3, 'pipeline_depth': 3}
    net = _build(spec, params, n, 224, **opts)
    xs = [np.ascontiguousarray(x[i:i + n]) for i in range(3)]        # three overlapping windows of the five images
    xt = [torch.from_numpy(v).to(dev) for v in xs]
    outs = [torch.empty((n, spec.num_classes), dtype=torch.float32, device=dev) for _ in range(3)]
    net.set_pipelined(2)
    for r in range(9):
        net.run(xt[r % 3], out=outs[r % 3])
    torch.cuda.synchronize()
    net.set_pipelined(0)
    ref = build_net(spec, params, max_batch=n, hw=224, options={'fuse_head_dws': 0})
    for i in range(3):
        np.testing.assert_array_equal(outs[i].cpu().numpy(), want[i:i + n], err_msg=f'input {i}')
        np.testing.assert_array_equal(outs[i].cpu().numpy(), ref.run(xt[i]).cpu().numpy(), err_msg=f'input {i} vs option 0')
