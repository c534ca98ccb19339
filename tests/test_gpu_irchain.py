"""fuse_irchain: runs of stride-1 MobileNet-V2 inverted residuals in one launch (f8_irchain.hip), bit for bit against the reference goldens,
the CPU oracle, and the per-block launches of the option-off plan."""
import os

import numpy as np
import pytest
import torch

from f8net_amd import synth, topology
from ir_cases import _w
from oracle import oracle
from refgraph import RefGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _chains(net):
    return [ln for ln in net.describe().splitlines() if 'ir_chain_x' in ln]


def _symbols_stay(net, run):
    planned = [net.launch_kernel(i) for i in range(net.num_launches)]
    out = run()
    assert [net.launch_kernel(i) for i in range(net.num_launches)] == planned
    assert any(s.startswith('f8::irchain_kernel<') for s in planned)
    return out


def test_reference_goldens(golden_dir, dev):
    from f8net_amd.net import build_net
    g = np.load(os.path.join(golden_dir, 'net_mobilenet_v2.npz'))
    spec = topology.get('mobilenet_v2', normalize=bool(g['normalize']))
    params = synth.reference_params(spec, seed=1234)
    for hw, n in ((64, 2), (224, 1)):
        x, _ = synth.make_input(spec, params, n, hw, seed=7)
        net = build_net(spec, params, max_batch=n, hw=hw, options={'fuse_irchain': 1})
        assert len(_chains(net)) >= 2, net.describe()
        got = _symbols_stay(net, lambda: net.run(torch.from_numpy(x).to(dev)).cpu().numpy())
        np.testing.assert_array_equal(got, g[f's1234_hw{hw}_n{n}/logits'], err_msg=f'hw{hw}')


@pytest.mark.parametrize('hw', [96, 200, 320])
def test_fresh_seeds_against_the_oracle(hw, dev):
    from f8net_amd.net import build_net
    spec = topology.get('mobilenet_v2', normalize=True)
    params = synth.make_params(spec, seed=77 + hw)
    x, x_fl = synth.make_input(spec, params, 5, hw, seed=3)
    want = oracle.net_forward(spec, params, x, x_fl)
    for rq in (0, 1):
        net = build_net(spec, params, max_batch=8, hw=hw, options={'fuse_irchain': 1, 'requant_float': rq})
        assert _chains(net), net.describe()
        got = _symbols_stay(net, lambda: net.run(torch.from_numpy(x).to(dev)).cpu().numpy())
        np.testing.assert_array_equal(got, want, err_msg=f'hw{hw} requant_float={rq}')
        np.testing.assert_array_equal(net.run(torch.from_numpy(x[:2]).to(dev)).cpu().numpy(), want[:2])


def test_rounding_add_wraps(dev):
    """Biases next to 2^31 in expand / depthwise convs of chained blocks: the integer requantisation instance, oracle's values."""
    from f8net_amd.net import build_net
    spec = topology.get('mobilenet_v2')
    params = synth.make_params(spec, seed=55)
    for key, ch in (('stage_3_layer_2.body.0', 20), ('stage_3_layer_2.body.2', 9), ('stage_5_layer_1.body.0', 33), ('stage_5_layer_2.body.2', 5)):
        b = params[key + '.bias'].copy()
        b[ch], b[(ch + 13) % b.size] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
        params[key + '.bias'] = b
    for hw, n in ((64, 3), (224, 2)):
        x, fl = synth.make_input(spec, params, n, hw, seed=3)
        want = oracle.net_forward(spec, params, x, fl)
        for rq in (0, 1):
            net = build_net(spec, params, max_batch=n, hw=hw, options={'fuse_irchain': 1, 'requant_float': rq})
            assert len(_chains(net)) >= 2
            np.testing.assert_array_equal(net.run(torch.from_numpy(x).to(dev)).cpu().numpy(), want, err_msg=f'hw{hw} rq{rq}')


@pytest.mark.parametrize('split', [2, 4])
def test_split(split, dev):
    from f8net_amd.net import build_net
    spec = topology.get('mobilenet_v2', normalize=True)
    params = synth.make_params(spec, seed=9)
    x, fl = synth.make_input(spec, params, 9, 224, seed=4)
    net = build_net(spec, params, max_batch=9, hw=224, options={'fuse_irchain': 1, 'split': split})
    assert net.num_launches == 15
    np.testing.assert_array_equal(net.run(torch.from_numpy(x).to(dev)).cpu().numpy(), oracle.net_forward(spec, params, x, fl))


@pytest.mark.parametrize('rq', [0, 1])
def test_bench_schedule_and_ragged_batches(rq, dev):
    """bench.py's MobileNet-V2 schedule: whole-batch launches, three arena copies, three runs in flight (set_pipelined(2)), rotating inputs and
    outputs; picked images against the oracle.  Then ragged batches against the option-off plan."""
    from f8net_amd.net import build_net
    spec = topology.get('mobilenet_v2', normalize=True)
    params = synth.make_params(spec, seed=21)
    n = 128
    opts = {'fuse_irchain': 1, 'requant_float': rq, 'whole_batch_launches': 1, 'arena_copies': 3, 'pipeline_depth': 3}
    net = build_net(spec, params, max_batch=n, hw=224, options=opts)
    assert net.num_launches == 15
    xs = [synth.make_input(spec, params, n, 224, seed=300 + i) for i in range(3)]
    xt = [torch.from_numpy(x).to(dev) for x, _ in xs]
    outs = [torch.empty((n, spec.num_classes), dtype=torch.float32, device=dev) for _ in range(3)]
    net.set_pipelined(2)
    for r in range(12):
        net.run(xt[r % 3], out=outs[r % 3])
    torch.cuda.synchronize()
    pick = [0, n // 2, n - 1]
    for i, (x, fl) in enumerate(xs):
        want = oracle.net_forward(spec, params, x[pick], fl)
        np.testing.assert_array_equal(outs[i].cpu().numpy()[pick], want, err_msg=f'input {i}')
    net.set_pipelined(0)
    ref = build_net(spec, params, max_batch=n, hw=224, options={'requant_float': rq})
    for k in (1, 2, 3, 33, 127, 128):
        np.testing.assert_array_equal(net.run(xt[0][:k]).cpu().numpy(), ref.run(xt[0][:k]).cpu().numpy(), err_msg=f'k={k}')


# ---- F8Net graphs of chained blocks in corner formats, against the CPU oracle (op by op) and the same graph planned without the chain
def _block_graph(case, x):
    """case: (blocks, x_fl, tail_fls).  blocks: dicts cin, cout, E, in_fl / in_signed (expand input), w_fl (expand weights), dw_in_fl, dw_w_fl,
    pw_in_fl, pw_w_fl (default w_fl), res, join_relu, bias_big (expand biases next to 2^31), pw_sig (project weights), zero_ch {channel: project
    bias of an output channel whose project weights are zero}.  tail_fls: 1x1 convs that read the last block's output as int8 in these formats
    (a 32-channel output is also joined as int32)."""
    blocks, x_fl, tail_fls = case
    g = RefGraph(x, x_fl)
    t = next(iter(g.v))
    c0 = blocks[0]['cin']
    t = g.conv(t, _w(1, (c0, c0, 1, 1), 12.0), synth.rand_normal_int(2, 'pb', (c0,), 300.0).astype(np.int32), pad=0, groups=1,
               weight_fl=6, input_fl=min(x_fl, 7), input_signed=True, relu=False)
    for i, b in enumerate(blocks):
        E, wfl = b['E'], b['w_fl']
        be = synth.rand_normal_int(10 + i, 'be', (E,), 2.0 ** 10).astype(np.int32)
        if b.get('bias_big'):
            be[3], be[7] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
        e = g.conv(t, _w(20 + i, (E, b['cin'], 1, 1), 10.0), be, pad=0, groups=1, weight_fl=wfl, input_fl=b['in_fl'], input_signed=b['in_signed'], relu=True)
        d = g.conv(e, _w(30 + i, (E, 1, 3, 3), 25.0), synth.rand_normal_int(40 + i, 'bd', (E,), 2.0 ** 9).astype(np.int32), pad=1, groups=E,
                   weight_fl=b.get('dw_w_fl', wfl), input_fl=b['dw_in_fl'], input_signed=False, relu=True)
        wp = _w(50 + i, (b['cout'], E, 1, 1), b.get('pw_sig', 6.0))
        bp = synth.rand_normal_int(60 + i, 'bp', (b['cout'],), 2.0 ** 11).astype(np.int32)
        for ch, bias in b.get('zero_ch', {}).items():
            wp[ch] = 0
            bp[ch] = bias
        p = g.conv(d, wp, bp, pad=0, groups=1, weight_fl=b.get('pw_w_fl', wfl), input_fl=b['pw_in_fl'], input_signed=False, relu=False)
        t = g.add(p, t, relu=b.get('join_relu', False)) if b['res'] else p
    out = t
    if tail_fls:
        cs = [g.conv(t, _w(90 + k, (32, blocks[-1]['cout'], 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=True, relu=False)
              for k, fl in enumerate(tail_fls)]
        out = cs[0]
        for c in cs[1:]:
            out = g.add(out, c)
        if blocks[-1]['cout'] == 32:
            out = g.add(out, t)
    g.net.output(out, as_float=False)
    return g, out


CORNERS = {
    # MBV2_CORNERS' depthwise formats 8/6 -> 8, 8/1 -> 8, 8/0 -> 7 (shifts 6, 1, 1), on 64 / 96 channels
    'dw_formats': ([dict(cin=64, cout=64, E=384, in_fl=4, in_signed=True, w_fl=6, dw_in_fl=8, dw_w_fl=6, pw_in_fl=8, res=True),
                    dict(cin=64, cout=96, E=384, in_fl=4, in_signed=True, w_fl=6, dw_in_fl=8, dw_w_fl=1, pw_in_fl=8, res=False),
                    dict(cin=96, cout=96, E=576, in_fl=2, in_signed=True, w_fl=6, dw_in_fl=8, dw_w_fl=0, pw_in_fl=7, res=True)], 6, [3]),
    # block outputs at fraclen 14 / 15 requantised into SIGNED int8 at fraclen 0 / 1 (MBV2_CORNERS' project rows: shifts 14 and 15) — in LDS as the
    # next block's input, and as the last block's two int8 output forms next to its int32 one
    'shift14_15_into_signed': ([dict(cin=32, cout=32, E=192, in_fl=5, in_signed=True, w_fl=7, dw_in_fl=8, dw_w_fl=0, pw_in_fl=7, pw_w_fl=7, pw_sig=40.0, res=True),
                                dict(cin=32, cout=32, E=192, in_fl=0, in_signed=True, w_fl=7, dw_in_fl=6, dw_w_fl=6, pw_in_fl=8, pw_w_fl=7, pw_sig=40.0, res=True),
                                dict(cin=32, cout=32, E=192, in_fl=0, in_signed=True, w_fl=7, dw_in_fl=6, dw_w_fl=1, pw_in_fl=6, pw_w_fl=7, pw_sig=40.0, res=True)],
                               6, [1, 0]),
    # joins with the residual shifted left / the project result shifted left, a ReLU behind a join, an unsigned expand input
    'join_shifts': ([dict(cin=32, cout=32, E=96, in_fl=6, in_signed=True, dw_in_fl=5, pw_in_fl=4, w_fl=5, res=True),
                     dict(cin=32, cout=32, E=96, in_fl=1, in_signed=True, dw_in_fl=5, pw_in_fl=4, w_fl=7, res=True, join_relu=True),
                     dict(cin=32, cout=32, E=96, in_fl=3, in_signed=False, dw_in_fl=6, pw_in_fl=5, w_fl=2, res=True)], 5, [3]),
    # the int32 stream driven into the clamp: channel 5 of block 0 is exactly 0, block 1's project result there is 2^30 << 1 (acc_shl 1), which
    # wraps to -2^31 and is clamped to -(2^31 - 1); block 2 joins that stream (and channel 9's biases near 2^30 wrap in the joins)
    'stream_clamp': ([dict(cin=32, cout=32, E=96, in_fl=4, in_signed=True, w_fl=6, dw_in_fl=6, pw_in_fl=6, res=False, zero_ch={5: 0, 9: 2 ** 30 - 7}),
                      dict(cin=32, cout=32, E=96, in_fl=4, in_signed=True, w_fl=6, dw_in_fl=6, pw_in_fl=5, res=True, zero_ch={5: 2 ** 30, 9: 2 ** 30 + 3}),
                      dict(cin=32, cout=32, E=96, in_fl=4, in_signed=True, w_fl=6, dw_in_fl=6, pw_in_fl=6, res=True)], 5, [4]),
    # biases next to 2^31 in an expand conv (integer requantisation instance), 160 -> 320 channels on the 7x7 register shape
    'wrap_bias': ([dict(cin=160, cout=160, E=960, in_fl=4, in_signed=True, dw_in_fl=6, pw_in_fl=5, w_fl=6, res=True, bias_big=True),
                   dict(cin=160, cout=320, E=960, in_fl=3, in_signed=True, dw_in_fl=6, pw_in_fl=5, w_fl=6, res=False)], 5, [3]),
}
CORNER_H = {'dw_formats': 14, 'shift14_15_into_signed': 6, 'join_shifts': 5, 'stream_clamp': 6, 'wrap_bias': 7}


@pytest.mark.parametrize('tail', [False, True])
@pytest.mark.parametrize('case', sorted(CORNERS))
def test_corner_formats(case, tail, dev):
    blocks, x_fl, tail_fls = CORNERS[case]
    N, H = 3, CORNER_H[case]
    x = synth.rand_uniform_int(5, f'x{case}', (N, blocks[0]['cin'], H, H), -127, 127).astype(np.int32)
    for on in (1, 0):
        g, out = _block_graph((blocks, x_fl, tail_fls if tail else []), x)
        g.net.set_option('fuse_irchain', on)
        g.net.set_option('fuse_ir', 0)
        g.net.finalize(N)
        chains = _chains(g.net)
        if on:
            assert len(chains) == 1 and chains[0].split()[1].startswith(f'ir_chain_x{len(blocks)}:'), g.net.describe()
        else:
            assert not chains
        want = g.v[out][0]
        assert np.unique(want).size > 8
        got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
        np.testing.assert_array_equal(got, want, err_msg=f'{case} fuse_irchain={on}')
