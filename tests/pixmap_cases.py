"""Case table, reference and graph builders of the tests of depth-to-space and space-to-depth (f8_net_depth_to_space / f8_net_space_to_depth,
`F8Net.depth_to_space` / `space_to_depth` / `pixel_shuffle` / `pixel_unshuffle`, f8_pixmap.hip): tests/test_pixmap_plan.py (acceptance, refusals,
tokens, kernel symbols, launch_info, where the ops cut fused launches, ONNX, the torch ops' meta impls, the host code under the sanitizers; no GPU)
and tests/test_gpu_pixmap.py (every case on both legs, bit for bit on the device).  No test functions here.

The reference is numpy reshape / transpose on the int32 tensors the reference graph carries: `d2s_ref` / `s2d_ref` below, the definitions of
include/f8net.h; test_pixmap_plan.py pins them to torch.nn.functional.pixel_shuffle / pixel_unshuffle, to the ONNX operators' own definitions and to
the round trip for every (op, order, r, C) of the table.  `d2s(g, t, r, order)` / `s2d(...)` record the op on a RefGraph as its own methods do.

Unless a builder says otherwise a case is  input (8 channels, 0 .. 255, fraclen 8) -> one 1x1 producer conv, random weights (no two channels carry
the same values) -> the op -> readers: one 32-output 1x1 conv per (input_fl, signed), summed.  A depth_to_space source is 5 x 3 at N = 3 (r = 2: 180
output pixels, a ragged I32T block), a space_to_depth source 5 r x 3 r; one case is 4 x 6 at N = 2, one space_to_depth goes down to a 1 x 1 map,
the DUC head (r = 8) reads a 2 x 3 map.

The expected plan tokens and kernel symbols of every case — `exp`: option pixmap_i8 = 1 (the default plan, also with every fusing pass on), `exp0`:
pixmap_i8 = 0 — are WRITTEN BY HAND in launch order (the rule: DESIGN.md 4.5q — the run mover for the DCR order where the channel run, C of a
depth_to_space result or of a space_to_depth source, is a multiple of 16; the transposer for the CRD order at r = 2 where that count is a multiple of
4; the general byte kernel otherwise); nothing here asks the planner for them."""
import sys

import numpy as np

import graph_cases
from concat_cases import FUSE_ALL, X_FL, producer, readers  # noqa: F401  (the tests take FUSE_ALL from here)
from f8net_amd import synth


# ---- the reference
def d2s_ref(x, r, order, swap=False):
    """[N, C r^2, H, W] -> [N, C, H r, W r].  crd: out[c][h r + i][w r + j] = x[c r^2 + i r + j][h][w]; dcr: ... = x[(i r + j) C + c][h][w].
    swap: the (wrong) op with i and j exchanged, for the data checks."""
    N, CC, H, W = x.shape
    C = CC // (r * r)
    assert C * r * r == CC and order in ('crd', 'dcr')
    if order == 'crd':
        t = x.reshape(N, C, r, r, H, W)                            # [n, c, i, j, h, w]
        t = t.transpose(0, 1, 4, 3 if swap else 2, 5, 2 if swap else 3)
    else:
        t = x.reshape(N, r, r, C, H, W)                            # [n, i, j, c, h, w]
        t = t.transpose(0, 3, 4, 2 if swap else 1, 5, 1 if swap else 2)
    return np.ascontiguousarray(t).reshape(N, C, H * r, W * r)


def s2d_ref(x, r, order, swap=False):
    """[N, C, H r, W r] -> [N, C r^2, H, W], the inverse of d2s_ref for each order."""
    N, C, HH, WW = x.shape
    H, W = HH // r, WW // r
    assert H * r == HH and W * r == WW and order in ('crd', 'dcr')
    t = x.reshape(N, C, H, r, W, r)                                # [n, c, h, i, w, j]
    i, j = (5, 3) if swap else (3, 5)
    t = t.transpose(0, 1, i, j, 2, 4) if order == 'crd' else t.transpose(0, i, j, 1, 2, 4)
    return np.ascontiguousarray(t).reshape(N, C * r * r, H, W)


def d2s(g, t, r, order, label=None):
    o = g._id(lambda: g.net.depth_to_space(t, r, order, label=label))
    g.srcv[o] = ('d2s', g.v[t][0], r, order)
    return g._put(o, (d2s_ref(g.v[t][0], r, order), g.v[t][1]), 'd2s', src=g._src(t), block=r, order=order)


def s2d(g, t, r, order, label=None):
    o = g._id(lambda: g.net.space_to_depth(t, r, order, label=label))
    g.srcv[o] = ('s2d', g.v[t][0], r, order)
    return g._put(o, (s2d_ref(g.v[t][0], r, order), g.v[t][1]), 's2d', src=g._src(t), block=r, order=order)


OPS = {'d2s': d2s, 's2d': s2d}


# ---- the builders.  Each returns (output tensor ids in output order, [op tensor ids in launch order])
def _source(g, x0, c, k=0):
    """The op's source: a 1x1 conv of the input at fraclen 13, scaled for a reader at fraclen 4; depth_to_space: C r^2 channels, space_to_depth: C."""
    C = c['C'] * c['r'] ** 2 if c['op'] == 'd2s' else c['C']
    return producer(g, x0, k, C, 9, w_fl=5, relu=c['relu'])


def _tail(g, t, c):
    """Readers behind the op, or the op itself as the output (readers=None)."""
    if not c['readers']:
        g.output(t, as_float=c.get('as_float', False))
        return t
    out = readers(g, t, c['readers'])
    g.output(out)
    return out


def _op(g, x0, c):
    s = OPS[c['op']](g, _source(g, x0, c), c['r'], c['order'], label='op')
    return [_tail(g, s, c)], [s]


def _op_input(g, x0, c):
    """The net input itself (3 channels up to +-2^28 at fraclen 2): nothing bounds it, and the byte mode needs no bound."""
    s = OPS[c['op']](g, x0, c['r'], c['order'], label='op')
    return [_tail(g, s, c)], [s]


def _op_join(g, x0, c):
    """Two results of the op on two producers, joined: the join reads int32."""
    a = OPS[c['op']](g, _source(g, x0, c), c['r'], c['order'], label='op')
    b = OPS[c['op']](g, _source(g, x0, c, k=3), c['r'], c['order'], label='op2')
    out = readers(g, g.add(a, b, relu=True), [(4, False)])
    g.output(out)
    return [out], [a, b]


def _round_trip(g, x0, c):
    """depth_to_space, then space_to_depth of the same block and order: the source again, in two launches."""
    src = _source(g, x0, c)
    a = d2s(g, src, c['r'], c['order'], label='op')
    b = s2d(g, a, c['r'], c['order'], label='back')
    assert np.array_equal(g.v[b][0], g.v[src][0])
    return [_tail(g, b, c)], [a, b]


RUN, GEN, K32 = 'f8::pixmap_run_i8_kernel', 'f8::pixmap_i8_general_kernel', 'f8::pixmap_i32_kernel'
TD, TS = 'f8::pixmap_crd2_i8_kernel<false>', 'f8::pixmap_crd2_i8_kernel<true>'      # the r = 2 CRD transposer: depth_to_space / space_to_depth


def _case(build, exp, H=5, W=3, N=3, **kw):
    c = dict(build=build, exp=exp, exp0=[(t.replace('_i8:', '_i32:'), K32) for t, _ in exp], H=H, W=W, N=N, relu=True, readers=[(4, False)], cin=8, x_fl=X_FL)
    c.update(kw)
    if c['op'] == 's2d' and 'H' not in kw:                         # a space_to_depth source: 5 r x 3 r
        c['H'], c['W'] = H * c['r'], W * c['r']
    return c


def _c(op, order, r, C, sym, build=_op, mode='i8', **kw):
    """One op: C = the channels of a depth_to_space RESULT / of a space_to_depth SOURCE."""
    return _case(build, [(f'{op}{r}{order}_{mode}:', sym)], op=op, order=order, r=r, C=C, **kw)


def _variants(op, order, r, C, sym, tag):
    """The reader variants of one shape: two int8 forms; three (int32 mode + a requant step); read by a join; the int32 output; the float output."""
    tok = f'{op}{r}{order}'
    return {
        f'{tag}_twoforms': _c(op, order, r, C, sym, relu=False, readers=[(3, True), (4, False)]),
        f'{tag}_threeforms': _c(op, order, r, C, K32, mode='i32', relu=False, readers=[(3, True), (4, False), (5, False)]),
        f'{tag}_to_add': _case(_op_join, [(f'{tok}_i32:', K32)] * 2, op=op, order=order, r=r, C=C),
        f'{tag}_to_out': _c(op, order, r, C, K32, mode='i32', readers=None),
        f'{tag}_to_out_f32': _c(op, order, r, C, K32, mode='i32', readers=None, as_float=True),
    }


CASES = {
    # ---- depth_to_space, r = 2 (C of the result; the source has 4 C): 16-byte runs, multiples of 4 only, odd (sources 12 and 76 have pad channels),
    # 40 (Cs 64; the source's 160 channels span five channel blocks)
    'd2s2_dcr_64': _c('d2s', 'dcr', 2, 64, RUN), 'd2s2_crd_64': _c('d2s', 'crd', 2, 64, TD),
    'd2s2_dcr_16': _c('d2s', 'dcr', 2, 16, RUN), 'd2s2_crd_16': _c('d2s', 'crd', 2, 16, TD),
    'd2s2_dcr_48': _c('d2s', 'dcr', 2, 48, RUN), 'd2s2_crd_48': _c('d2s', 'crd', 2, 48, TD),
    'd2s2_dcr_12': _c('d2s', 'dcr', 2, 12, GEN), 'd2s2_crd_12': _c('d2s', 'crd', 2, 12, TD),
    'd2s2_dcr_20': _c('d2s', 'dcr', 2, 20, GEN), 'd2s2_crd_20': _c('d2s', 'crd', 2, 20, TD),
    'd2s2_dcr_3': _c('d2s', 'dcr', 2, 3, GEN), 'd2s2_crd_3': _c('d2s', 'crd', 2, 3, GEN),
    'd2s2_dcr_19': _c('d2s', 'dcr', 2, 19, GEN), 'd2s2_crd_19': _c('d2s', 'crd', 2, 19, GEN),
    'd2s2_dcr_40': _c('d2s', 'dcr', 2, 40, GEN), 'd2s2_crd_40': _c('d2s', 'crd', 2, 40, TD),
    'd2s2_crd_12_4x6': _c('d2s', 'crd', 2, 12, TD, H=4, W=6, N=2),
    # ---- other blocks: ESPCN's 27 -> 3, 72 -> 8, 256 -> 16, the DUC head's 1216 -> 19 on a 2 x 3 map
    'd2s3_crd_3': _c('d2s', 'crd', 3, 3, GEN), 'd2s3_dcr_3': _c('d2s', 'dcr', 3, 3, GEN),
    'd2s3_crd_8': _c('d2s', 'crd', 3, 8, GEN), 'd2s3_dcr_8': _c('d2s', 'dcr', 3, 8, GEN),
    'd2s4_crd_16': _c('d2s', 'crd', 4, 16, GEN), 'd2s4_dcr_16': _c('d2s', 'dcr', 4, 16, RUN),
    'd2s8_crd_19': _c('d2s', 'crd', 8, 19, GEN, H=2, W=3), 'd2s8_dcr_19': _c('d2s', 'dcr', 8, 19, GEN, H=2, W=3),
    # ---- space_to_depth (C of the source; the result has r^2 C).  From the net input: 3 channels, raw values up to +-2^28
    's2d4_dcr_input': _c('s2d', 'dcr', 4, 3, GEN, build=_op_input, cin=3, x_fl=2, raw=True, readers=[(4, True)]),
    's2d4_crd_input': _c('s2d', 'crd', 4, 3, GEN, build=_op_input, cin=3, x_fl=2, raw=True, readers=[(4, True)]),
    's2d2_dcr_input': _c('s2d', 'dcr', 2, 3, GEN, build=_op_input, cin=3, x_fl=2, raw=True, readers=[(4, True)]),
    's2d2_crd_input': _c('s2d', 'crd', 2, 3, GEN, build=_op_input, cin=3, x_fl=2, raw=True, readers=[(4, True)]),
    's2d2_dcr_16': _c('s2d', 'dcr', 2, 16, RUN), 's2d2_crd_16': _c('s2d', 'crd', 2, 16, TS),
    's2d2_dcr_32': _c('s2d', 'dcr', 2, 32, RUN), 's2d2_crd_32': _c('s2d', 'crd', 2, 32, TS),
    's2d2_dcr_12': _c('s2d', 'dcr', 2, 12, GEN), 's2d2_crd_12': _c('s2d', 'crd', 2, 12, TS),
    's2d2_dcr_19': _c('s2d', 'dcr', 2, 19, GEN), 's2d2_crd_19': _c('s2d', 'crd', 2, 19, GEN),
    's2d2_dcr_40': _c('s2d', 'dcr', 2, 40, GEN), 's2d2_crd_40': _c('s2d', 'crd', 2, 40, TS),
    's2d3_dcr_8': _c('s2d', 'dcr', 3, 8, GEN), 's2d3_crd_8': _c('s2d', 'crd', 3, 8, GEN),
    's2d2_crd_16_1x1': _c('s2d', 'crd', 2, 16, TS, H=2, W=2),              # a [64, 1, 1] result: M = 3
    's2d2_dcr_12_4x6': _c('s2d', 'dcr', 2, 12, GEN, H=8, W=12, N=2),
    # ---- depth_to_space, then space_to_depth of the same block and order
    'rt2_dcr_16': _case(_round_trip, [('d2s2dcr_i8:', RUN), ('s2d2dcr_i8:', RUN)], op='d2s', order='dcr', r=2, C=16),
    'rt3_crd_3': _case(_round_trip, [('d2s3crd_i8:', GEN), ('s2d3crd_i8:', GEN)], op='d2s', order='crd', r=3, C=3),
}
# ---- the reader variants on one aligned and one odd shape of each op
CASES['d2s2_crd_16_twoforms'] = _c('d2s', 'crd', 2, 16, TD, relu=False, readers=[(3, True), (4, False)])      # the transposer writing two forms
CASES['s2d2_crd_16_twoforms'] = _c('s2d', 'crd', 2, 16, TS, relu=False, readers=[(3, True), (4, False)])
CASES.update(_variants('d2s', 'dcr', 2, 16, RUN, 'd2s_al'))
CASES.update(_variants('d2s', 'crd', 2, 19, GEN, 'd2s_odd'))
CASES.update(_variants('s2d', 'dcr', 2, 16, RUN, 's2d_al'))
CASES.update(_variants('s2d', 'crd', 2, 19, GEN, 's2d_odd'))

SHAPES = sorted({(c['op'], c['order'], c['r'], c['C']) for c in CASES.values()})


def make_input(name, n=None):
    c = CASES[name]
    shape = (n or c['N'], c['cin'], c['H'], c['W'])
    if c.get('raw'):                                                           # up to +-2^28, and a band of small values (concat_cases' raw input)
        x = synth.rand_uniform_int(5, f'pmx{name}', shape, -2 ** 28, 2 ** 28).astype(np.int64)
        small = synth.rand_uniform_int(6, f'pms{name}', shape, -300, 300).astype(np.int64)
        x = np.where(small % 3 == 0, small, x)
        x.reshape(-1)[:4] = [2 ** 28, -2 ** 28, 2 ** 24, -2 ** 24]
        return x.astype(np.int32)
    return synth.rand_uniform_int(5, f'pmx{name}', shape, 0, 255).astype(np.int32)


def lines(net):
    """[(launch index, plan token, kernel symbol)] of the handle's depth_to_space and space_to_depth launches, in launch order."""
    return graph_cases.launch_lines(net, ('d2s', 's2d'))


def expected(name, **opts):
    """The hand-written (token, symbol) list of the case under these options."""
    return CASES[name]['exp' if opts.get('pixmap_i8', 1) else 'exp0']


def check_data(name, g, outs, ops):
    """What the table promises about every case's data, so that a wrong kernel cannot hide: every op result differs from the same op in the other
    order, from the op with i and j swapped and from nearest replication, and no two of its channels are equal."""
    for t in ops:
        kind, src, r, order = g.srcv[t]
        ref = d2s_ref if kind == 'd2s' else s2d_ref
        y = g.v[t][0]
        np.testing.assert_array_equal(y, ref(src, r, order))
        assert not np.array_equal(y, ref(src, r, 'dcr' if order == 'crd' else 'crd')), f'{name}: the other order gives the same values'
        assert not np.array_equal(y, ref(src, r, order, swap=True)), f'{name}: i and j swapped gives the same values'
        if kind == 'd2s':
            rep = np.repeat(np.repeat(src[:, :y.shape[1]], r, axis=2), r, axis=3)
        else:
            rep = np.tile(src[:, :, ::r, ::r], (1, r * r, 1, 1))
        assert rep.shape == y.shape and not np.array_equal(y, rep), f'{name}: nearest replication gives the same values'
        flat = y.transpose(1, 0, 2, 3).reshape(y.shape[1], -1)
        live = [row.tobytes() for row in flat if row.any()]                    # (a ReLU leaves a few channels of the wide producers at 0 throughout)
        assert len(set(live)) == len(live), f'{name}: two channels carry the same values'
        assert len(live) >= y.shape[1] - y.shape[1] // 16, f'{name}: {y.shape[1] - len(live)} of {y.shape[1]} channels are dead'


graph_cases.bind_cases(sys.modules[__name__], check_data=check_data)      # build_graph, reference, plan, int_graph
