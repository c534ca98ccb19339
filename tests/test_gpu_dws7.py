"""fuse_dws7: depthwise-separable blocks on 7x7 output maps in one launch, the average pool behind the last one summed in it (f8_dws7.hip), bit for
bit against the CPU oracle (op by op and whole nets), the reference goldens and the option-off plan of the same parameters.  The parameter
recipes are test_gpu_dws.py's."""
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


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _fused(net):
    return [ln for ln in net.describe().splitlines() if 'fused_dws7:' in ln]


def _dws7_symbols(net):
    return [net.launch_kernel(i) for i in range(net.num_launches) if net.launch_info(i, 1)[0].startswith('fused_dws7:')]


# A block: cin, cout, stride; dw_in_fl (the depthwise conv's unsigned input format), dw_w_fl / pw_in_fl: the mid requantisation shifts right by
# dw_in_fl + dw_w_fl - pw_in_fl; pw_w_fl and the readers' formats: the output shifts by pw_in_fl + pw_w_fl - reader fl.  *_sig / *_bsig: weight
# and bias spreads (small weights for a shift of 1, large biases for a shift of 16: the values stay inside 8 bits without saturating everywhere).
def _blk(cin, cout, stride=1, **kw):
    d = dict(cin=cin, cout=cout, stride=stride, dw_in_fl=6, dw_w_fl=6, pw_in_fl=6, pw_w_fl=6, dw_sig=25.0, dw_bsig=2.0 ** 9, pw_sig=None,
             pw_bsig=2.0 ** 11, pw_relu=True, big=False)
    d.update(kw)
    if d['pw_sig'] is None:
        d['pw_sig'] = 10.0 * (32.0 / cin) ** 0.5
    return d


def _graph(blocks, readers, x, pool):
    """input -> pre 1x1 (ReLU) -> blocks -> one 1x1 reader per (fl, signed) of `readers`, summed: the int32 net output.  pool: the block output
    goes through avgpool_sum(shift 6) and a linear layer that reads the pooled sums in the unsigned format `pool` instead."""
    g = RefGraph(x, 6)
    t = next(iter(g.v))
    c0 = blocks[0]['cin']
    t = g.conv(t, _w(1, (c0, c0, 1, 1), 12.0 * (32.0 / c0) ** 0.5), _b(2, c0, 300.0), pad=0, groups=1, weight_fl=blocks[0]['dw_in_fl'], input_fl=6,
               input_signed=True, relu=True)
    for i, b in enumerate(blocks):
        cin, cout = b['cin'], b['cout']
        bd, bp = _b(40 + i, cin, b['dw_bsig']), _b(60 + i, cout, b['pw_bsig'])
        if b['big']:                                              # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
            bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
            bp[5], bp[20] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
        d = g.conv(t, _w(30 + i, (cin, 1, 3, 3), b['dw_sig']), bd, stride=b['stride'], pad=1, groups=cin, weight_fl=b['dw_w_fl'],
                   input_fl=b['dw_in_fl'], input_signed=False, relu=True)
        t = g.conv(d, _w(50 + i, (cout, cin, 1, 1), b['pw_sig']), bp, pad=0, groups=1, weight_fl=b['pw_w_fl'], input_fl=b['pw_in_fl'],
                   input_signed=False, relu=b['pw_relu'])
    cl = blocks[-1]['cout']
    if pool is not None:
        p = g.avgpool_sum(t, 6)
        out = g.linear(p, _w(95, (40, cl), 8.0), _b(96, 40, 500.0), weight_fl=6, input_fl=pool, input_signed=False)
    else:
        out = None
        for k, (fl, sgn) in enumerate(readers):
            c = g.conv(t, _w(90 + k, (32, cl, 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, relu=False)
            out = c if out is None else g.add(out, c)
    g.net.output(out, as_float=False)
    return g, out


def _run_case(dev, blocks, H, N, readers=((6, False),), opts=None, inst=None, pool=None):
    """Plans the graph with fuse_dws7 1 and 0, checks the fused lines / their absence (the instance's FQ, `inst`; POOL on the last block exactly when
    `pool` is set), compares both plans with the oracle."""
    x = synth.rand_uniform_int(5, f'x{H}x{H}', (N, blocks[0]['cin'], H, H), -127, 127).astype(np.int32)
    for on in (1, 0):
        g, out = _graph(blocks, readers, x, pool)
        g.net.set_option('fuse_dws7', on)
        for k, v in (opts or {}).items():
            g.net.set_option(k, v)
        g.net.finalize(N)
        plan = g.net.describe()
        assert len(_fused(g.net)) == (len(blocks) if on else 0), plan
        if on:
            syms = _dws7_symbols(g.net)
            assert [s.endswith(', true>') for s in syms] == [False] * (len(blocks) - 1) + [pool is not None], syms
            assert 'avgpool_sum:' not in plan, plan
            if inst is not None:
                assert all(s.split(', ')[1] == str(inst) for s in syms), syms
        want = g.v[out][0]
        assert np.unique(want).size > 8
        got = g.net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(want.shape)
        np.testing.assert_array_equal(got, want, err_msg=f'fuse_dws7={on}')


# blocks, input map, images, pool format (None: a 1x1 reader)
SHAPES = {
    'k1_n1': ([_blk(32, 64)], 7, 1, None),                         # one K step, ONE image: 49 pixels, a ragged second pixel tile, one output tile per workgroup
    'group_ragged': ([_blk(32, 64)], 7, 5, None),                  # four images per workgroup: one full group + one image
    's2_14_to_7': ([_blk(64, 96, 2)], 14, 3, None),                # stride 2 (border rows and columns), Cout / 32 odd
    'lds_limit': ([_blk(1024, 64)], 7, 4, None),                   # Cin = 1024: three images fill the 160 KB exactly (groups of 3 + 1), 32 K steps
    'lds_limit_pool': ([_blk(1024, 64)], 7, 4, 3),                 # ... with the pool's sums beside the mid tile: two images per workgroup
    'wide_output': ([_blk(64, 1024)], 7, 9, None),                 # 32 output tiles in several slices, rotated tile walk, three groups (the last: one image)
    'cout48': ([_blk(64, 48)], 7, 2, None),                        # an output channel count padded to 64
    'pool_small': ([_blk(32, 64)], 7, 3, 3),                       # sums across pixel-tile boundaries (seams at pixels 49 and 98 of 147)
    'pool_ragged': ([_blk(32, 64)], 7, 5, 3),                      # ... one full group + one image
    'pool_1024': ([_blk(1024, 1024)], 7, 5, 4),                    # MobileNet-V1's last block: groups of 2 + 2 + 1 images
    # the second block reads the first one's int8 output (32 -> 64 -> 96: no fused_ir instance, which would claim 1x1 -> depthwise -> 1x1 first)
    'pair_pool': ([_blk(32, 64, 2), _blk(64, 96)], 14, 3, 3),
}


@pytest.mark.parametrize('case', sorted(SHAPES))
def test_shapes(case, dev):
    blocks, H, N, pool = SHAPES[case]
    _run_case(dev, blocks, H, N, inst=2, pool=pool)


def test_signed_reader_takes_the_general_instance(dev):
    _run_case(dev, [_blk(32, 64, pw_relu=False)], 7, 5, readers=((5, True),), inst=0)


def test_shift_1(dev):
    _run_case(dev, [_blk(32, 64, dw_in_fl=4, dw_w_fl=2, pw_in_fl=5, pw_w_fl=2, dw_sig=1.0, dw_bsig=40.0, pw_sig=0.7, pw_bsig=60.0)], 7, 5,
              readers=((6, False),), inst=2)


@pytest.mark.parametrize('rq', [0, 1])
def test_shift_16(rq, dev):
    _run_case(dev, [_blk(32, 64, dw_in_fl=8, dw_w_fl=8, pw_in_fl=0, pw_w_fl=16, dw_sig=60.0, pw_sig=60.0, dw_bsig=2.0 ** 21, pw_bsig=2.0 ** 21)], 7, 5,
              readers=((0, False),), opts={'requant_float': rq}, inst=2 - rq)


def test_shift_17_with_requant_float_takes_the_integer_instance(dev):
    _run_case(dev, [_blk(32, 64, dw_in_fl=8, dw_w_fl=9, pw_in_fl=0, pw_w_fl=17, dw_sig=60.0, pw_sig=60.0, dw_bsig=2.0 ** 22, pw_bsig=2.0 ** 22)], 7, 5,
              readers=((0, False),), opts={'requant_float': 1}, inst=2)


def test_two_output_formats(dev):
    _run_case(dev, [_blk(64, 64)], 7, 5, readers=((6, False), (7, False)), inst=2)
    _run_case(dev, [_blk(64, 64)], 7, 5, readers=((6, False), (5, True)), inst=0)


@pytest.mark.parametrize('rq', [0, 1])
def test_rounding_add_wraps(rq, dev):
    """Depthwise and 1x1 biases next to 2^31: the planner cannot bound the accumulators and picks the integer instance by itself."""
    _run_case(dev, [_blk(32, 64, big=True)], 7, 5, opts={'requant_float': rq}, inst=2)
    _run_case(dev, [_blk(64, 64, 2, big=True)], 14, 3, opts={'requant_float': rq}, inst=2)


@pytest.mark.parametrize('rq', [0, 1])
def test_pool_behind_the_float_requantisation(rq, dev):
    """With the pool only the depthwise requantisation decides the instance; the pooled sums take the general form."""
    _run_case(dev, [_blk(32, 64)], 7, 5, opts={'requant_float': rq}, inst=2 - rq, pool=3)


# ---- whole nets
def _symbols_stay(net, run):
    planned = [net.launch_kernel(i) for i in range(net.num_launches)]
    out = run()
    assert [net.launch_kernel(i) for i in range(net.num_launches)] == planned
    assert any(s.startswith('f8::dws7_kernel<') for s in planned)
    return out


@pytest.mark.parametrize('both', [0, 1], ids=['alone', 'with_fuse_dws'])
def test_reference_golden(golden_dir, both, dev):
    from f8net_amd.net import build_net
    g = np.load(os.path.join(golden_dir, 'net_mobilenet_v1.npz'))
    spec = topology.get('mobilenet_v1', normalize=bool(g['normalize']))
    params = synth.reference_params(spec, seed=1234)
    x, _ = synth.make_input(spec, params, 1, 224, seed=7)
    net = build_net(spec, params, max_batch=1, hw=224, options={'fuse_dws7': 1, 'fuse_dws': both})
    assert len(_fused(net)) == 2 and net.num_launches == (16 if both else 27), net.describe()
    got = _symbols_stay(net, lambda: net.run(torch.from_numpy(x).to(dev)).cpu().numpy())
    np.testing.assert_array_equal(got, g['s1234_hw224_n1/logits'])


@functools.lru_cache(maxsize=None)
def _fresh(hw, n):
    spec = topology.get('mobilenet_v1', normalize=True)
    params = synth.make_params(spec, seed=77 + hw)
    x, x_fl = synth.make_input(spec, params, n, hw, seed=3)
    want = oracle.net_forward(spec, params, x, x_fl)
    want.setflags(write=False)
    return spec, params, x, want


@pytest.mark.parametrize('opts', [{'requant_float': 0}, {'requant_float': 1}, {'split': 2}], ids=['rq0', 'rq1', 'split2'])
@pytest.mark.parametrize('hw,n,nf', [(112, 5, 6), (224, 3, 2)])
def test_fresh_seeds_against_the_oracle(hw, n, nf, opts, dev):
    from f8net_amd.net import build_net
    spec, params, x, want = _fresh(hw, n)
    net = build_net(spec, params, max_batch=8 if hw == 112 else n, hw=hw, options=dict(opts, fuse_dws7=1))
    assert len(_fused(net)) == nf, net.describe()
    got = _symbols_stay(net, lambda: net.run(torch.from_numpy(x).to(dev)).cpu().numpy())
    np.testing.assert_array_equal(got, want, err_msg=f'hw{hw} {opts}')
    if hw == 112:
        np.testing.assert_array_equal(net.run(torch.from_numpy(x[:2]).to(dev)).cpu().numpy(), want[:2])


def test_bench_schedule_and_ragged_batches(dev):
    """bench.py's schedule: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), rotating inputs and outputs; picked
    images against the oracle.  Then ragged batches against the option-off plan of the same parameters."""
    from f8net_amd.net import build_net
    spec = topology.get('mobilenet_v1', normalize=True)
    params = synth.make_params(spec, seed=21)
    n = 128
    opts = {'fuse_dws7': 1, 'fuse_dws': 1, 'whole_batch_launches': 1, 'arena_copies': 3, 'pipeline_depth': 3}
    net = build_net(spec, params, max_batch=n, hw=224, options=opts)
    assert net.num_launches == 16
    xs = [synth.make_input(spec, params, n, 224, seed=300 + i) for i in range(3)]
    xt = [torch.from_numpy(x).to(dev) for x, _ in xs]
    outs = [torch.empty((n, spec.num_classes), dtype=torch.float32, device=dev) for _ in range(3)]
    net.set_pipelined(2)
    for r in range(12):
        net.run(xt[r % 3], out=outs[r % 3])
    torch.cuda.synchronize()
    pick = [0, 64, 127]
    for i, (x, fl) in enumerate(xs):
        want = oracle.net_forward(spec, params, x[pick], fl)
        np.testing.assert_array_equal(outs[i].cpu().numpy()[pick], want, err_msg=f'input {i}')
    net.set_pipelined(0)
    ref = build_net(spec, params, max_batch=n, hw=224)
    for k in (1, 2, 3, 33, 127):
        np.testing.assert_array_equal(_symbols_stay(net, lambda: net.run(xt[0][:k]).cpu().numpy()), ref.run(xt[0][:k]).cpu().numpy(), err_msg=f'k={k}')
