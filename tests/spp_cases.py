"""Case table and graph builder of tests/test_spp_plan.py and tests/test_gpu_spp.py (options maxpool_tile and fuse_spp, f8_maxpool.hip).  No test functions.

A case is  input (8 channels, 0 .. 255, fraclen 8) -> a 1x1 producer conv to C channels at fraclen 13, x -> max pools of x and / or a concat -> one 32-output
1x1 reader in unsigned fraclen 4 behind the producer's ReLU or signed fraclen 3.  A tile is 24 - 2 (k / 2) pixels a side (12 at a window of 13, 20 at 5), a
workgroup takes 64 channels: the maps sit one pixel below and above a tile on either axis; 3 x 5 is smaller than the halo.  N = 2 of max_batch 3.
`want` is WRITTEN BY HAND per leg — P: the parent's plan, T: maxpool_tile = 2, F: maxpool_tile = 2 and fuse_spp = 1 — as the (token, kernel symbol) of every
max-pool / concat / pyramid launch in launch order; a leg that is not given plans as the leg before it."""
import sys

import numpy as np

import graph_cases
from concat_cases import X_FL, producer, readers
from f8net_amd import synth
from graph_cases import launch_lines
from oracle import oracle

U, S = (4, False), (3, True)
OLD, TILE, I32 = 'f8::maxpool_i8x16_kernel', 'f8::maxpool_tile_kernel<%d>', 'f8::maxpool_kernel'
LEGS = {'P': {}, 'T': {'maxpool_tile': 2}, 'F': {'maxpool_tile': 2, 'fuse_spp': 1}}


def _x(g, x0, c):
    # (scaled for two bits more than the reader's shift keeps: the requantisation saturates, so both ends of the format occur)
    return producer(g, x0, 0, c['C'], 12 if c['fmt'] == S else 11, w_fl=5, relu=c['fmt'] == U)


def _pyramid(g, x0, c):
    """x and its pools — ks side by side (SPP) or chained (SPPF) — concatenated in c['order'] (0 = x, j = pool j) -> the reader; `extra` draws one more
    reader: 'pool' of the first pool, 'avg' the concat's average (an int32 reader)."""
    x = _x(g, x0, c)
    ts = [x]
    for k in c['ks']:
        ts.append(g.maxpool(ts[-1] if c['chain'] else x, k, 1, k // 2))
    cat = g.concat([ts[j] for j in c['order']], label='cat')
    out = readers(g, cat, [c['fmt']])
    if c.get('extra') == 'pool':
        out = g.add(out, g.conv(ts[1], np.ones((32, c['C'], 1, 1), np.int32), None, pad=0, groups=1, weight_fl=6, input_fl=c['fmt'][0], input_signed=c['fmt'][1], relu=False))
    g.output(out)
    outs = [out]
    if c.get('extra') == 'avg':
        outs.append(g.avgpool_sum(cat))
        g.output(outs[-1])
    return outs, [cat]


def _alone(g, x0, c):
    """x -> one pool (k, stride, pad) -> the reader."""
    p = g.maxpool(_x(g, x0, c), *c['ks'])
    out = readers(g, p, [c['fmt']])
    g.output(out)
    return [out], [p]


def _case(C, H, W, ks, want, *, fmt=U, chain=False, order=None, build=_pyramid, **kw):
    return dict(C=C, H=H, W=W, N=2, ks=ks, want=want, fmt=fmt, chain=chain, order=order or list(range(len(ks) + 1)), build=build, **kw)


def _legs(n, fused, levels, cat='f8::concat_i8_kernel<true>'):
    """n stand-alone pools + the concat on P and T; on F the pyramid launch `fused`, or (None) what T plans."""
    w = {'P': [('maxpool_i8:', OLD)] * n + [('concat_i8:', cat)], 'T': [('maxpool_i8:', TILE % 1)] * n + [('concat_i8:', cat)]}
    if fused:
        w['F'] = [(fused, TILE % levels)]
    return w


SAME = {'P': [('maxpool_i8:', OLD)]}
CASES = {
    'spp_3x5': _case(32, 3, 5, (5, 9, 13), _legs(3, 'spp5_9_13+concat_i8:', 3)),                            # the map is smaller than the halo
    'spp_11x13_rev': _case(64, 11, 13, (5, 9, 13), _legs(3, 'spp5_9_13+concat_i8:', 3), fmt=S, order=[3, 2, 1, 0]),
    'spp_13x11_c96': _case(96, 13, 11, (5, 9, 13), _legs(3, 'spp5_9_13+concat_i8:', 3)),                    # a whole and a half channel block
    'sppf_555': _case(32, 13, 13, (5, 5, 5), _legs(3, 'spp5_9_13+concat_i8:', 3), chain=True),
    'sppf_33': _case(32, 19, 21, (3, 3), _legs(2, 'spp3_5+concat_i8:', 2), fmt=S, chain=True),
    'one_pool': _case(64, 21, 19, (5,), _legs(1, 'spp5+concat_i8:', 1), order=[1, 0]),
    'spp_7_11': _case(32, 13, 15, (7, 11), _legs(2, 'spp7_11+concat_i8:', 2)),                              # levels of 7 and 5: steps 1 2 2 1 and 1 2 1
    # ---- what the pyramid launch does not take: the parent's launches (on T: the tile kernel where the pool alone qualifies)
    'c40': _case(40, 13, 13, (5, 9, 13), _legs(3, None, 0, cat='f8::concat_i8_kernel<false>')),             # padded rows (Cs = 64): slices off the 16-byte grid
    'second_reader': _case(32, 13, 11, (5, 9), _legs(2, None, 0), extra='pool'),
    'int32_reader': _case(32, 13, 11, (5, 9, 13), {'P': [('maxpool_i32:', I32)] * 3 + [('concat_i32:', 'f8::concat_i32_kernel')]}, extra='avg'),
    'even_k': _case(32, 13, 11, (4, 1, 2), SAME, build=_alone),
    'stride2': _case(32, 13, 11, (3, 2, 1), SAME, build=_alone, fmt=S),
    'k15': _case(32, 13, 11, (15, 1, 7), SAME, build=_alone),                                               # a window above 13
}


def want(name, leg):
    w = CASES[name]['want']
    return w.get(leg) or w.get('T' if leg == 'F' else 'P') or w['P']


def lines(net):
    return [ln[1:] for ln in launch_lines(net, ('maxpool_', 'concat_', 'spp'))]


def make_input(name, n=None):
    c = CASES[name]
    return synth.rand_uniform_int(5, f'spp{name}', (n or c['N'], 8, c['H'], c['W']), 0, 255).astype(np.int32)


def _check_data(name, g, outs, ops):
    """The bytes the launches move fill the format: both extremes (a signed format clamps at +-127) and more than 100 distinct values."""
    fl, sgn = CASES[name]['fmt']
    q = oracle.requant(g.v[ops[0]][0], fl, g.v[ops[0]][1], sgn)
    assert (q.min(), q.max()) == ((-127, 127) if sgn else (0, 255)) and np.unique(q).size > 100, (name, q.min(), q.max(), np.unique(q).size)


graph_cases.bind_cases(sys.modules[__name__], check_data=_check_data)      # build_graph, reference, plan, int_graph
