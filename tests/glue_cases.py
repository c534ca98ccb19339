"""Case tables, graph builders and data assertions of the op-level tests of the oldest launch family — the pools, the join and the classifier that every
net and every later op leans on as readers and producers: maxpool_kernel / maxpool_i8x16_kernel, avgpool_kernel (the global sum), add_kernel (plan
tokens `add:` and `requant:`) of f8_kernels.hip and fc_dense_kernel<512 | 1024 | 1280 | 2048> of f8_fc.hip.  tests/test_glue_plan.py (tokens and kernel
symbols, the data conditions on the reference alone, the max-pool reference pinned to torch, ONNX; no GPU) and tests/test_gpu_glue.py (every case bit
for bit on the device).  No test functions here.

The references are the oracle's own: oracle.maxpool (-inf padding), avgpool_sum (int64 sum narrowed to int32), add_align, relu, requant, linear,
through RefGraph's methods.

Unless a builder says otherwise a case is  input (8 channels, 0 .. 255, fraclen 8) -> a 1x1 producer conv that reads it as it is, so that the op
under test does not read the network input -> the op -> readers: one 32-output 1x1 conv per (fraclen, signed), summed (concat_cases.readers), and /
or the op's result as an int32 network output.  The planner picks the forms from the readers: a max-pool with ONE int8 reader and nothing else runs
on bytes (`maxpool_i8:`), every other max-pool on the int32 form (`maxpool_i32:`); the first two int8 formats of a tensor are written by its
producer, a third by a `requant:` launch from the int32 form.

Five tables — A: max-pool geometry on the three forms (int32, signed int8, unsigned int8); B: what reads a max-pool on the int32 kernel; C: the
global sum pool; D: the join and the stand-alone requant; E: the classifier.  The expected plan tokens and kernel symbols of every case (`exp`, in
launch order) are WRITTEN BY HAND; nothing here asks the planner for them.

Padded channels (C = 8 and 40 leave 24 of 32 and 24 of 64 stored channels unused): no comparison here looks at them — a network output copies the C
real channels and a reader's weights cover only those.  Nothing is claimed about them."""
import sys

import numpy as np

import graph_cases
from concat_cases import FUSE_ALL, X_FL, producer, readers  # noqa: F401  (the tests take FUSE_ALL from here)
from f8net_amd import synth
from ir_cases import _b, _w
from oracle import oracle

MAXPOOL_I32, MAXPOOL_I8, AVGPOOL, ADD = 'f8::maxpool_kernel', 'f8::maxpool_i8x16_kernel', 'f8::avgpool_kernel', 'f8::add_kernel'
IGEMM_256 = 'f8::conv_igemm_kernel<128, 32, 64, 4, 1, false, false, 2, false>'      # 256 features -> 10 classes on a handle for a few images: the 128x32x64 tile
TOKENS = ('maxpool_i8', 'maxpool_i32', 'avgpool_sum', 'add', 'requant', 'linear_dense')      # (launch_lines matches the text in front of the colon)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def out_size(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def fc_symbol(features):
    return f'f8::fc_dense_kernel<{(features + 31) // 32 * 32}>'


def _tail(g, t, c):
    """What reads the op's result t: readers (output 0) and / or t itself as an int32 (or float) network output."""
    outs = []
    if c['readers']:
        outs.append(readers(g, t, c['readers']))
        g.output(outs[0])
    if c['out']:
        outs.append(t)
        g.output(t, as_float=c.get('as_float', False))
    return outs


# ---- tables A and B: max-pool
def _pool_source(g, x0, c):
    """The pool's source: C channels at fraclen 13 whose reader shift is 8.  Without a ReLU the biases are centred at -2^14 (-64 in a reader's
    units, the spread across channels as large): most channels are negative in most pixels, so that windows at the border have negative maxima.
    In front of an unsigned reader they are centred at +2^14 instead: negative maxima remain in the int32 values, and few channels are 0 throughout."""
    C = c['C']
    w = _w(300 + c['seed'], (C, 8, 1, 1), 40.0)
    b = _b(301 + c['seed'], C, 2.0 ** 12, 2.0 ** 13 if c['relu'] else 2.0 ** 14 if c.get('form') == 'u8' else -(2.0 ** 14))
    return g.conv(x0, w, b, pad=0, groups=1, weight_fl=5, input_fl=X_FL, input_signed=False, relu=c['relu'], quant_input=False)


def _maxpool(g, x0, c):
    src = _pool_source(g, x0, c)
    pl = g.maxpool(src, c['k'], c['s'], c['pad'])
    return _tail(g, pl, c), [pl]


S8, U8 = (5, True), (5, False)                                     # the int8 forms of table A: a right shift by 8


def _mp(k, s, pad, H, W, C, form, *, relu=False, seed=0, **kw):
    """form: 'i32' (the pool is the network output), 's8' / 'u8' (one int8 reader: the byte kernel)."""
    assert 2 * pad <= k and out_size(H, k, s, pad) >= 1 and out_size(W, k, s, pad) >= 1
    exp = [('maxpool_i32:', MAXPOOL_I32)] if form == 'i32' else [('maxpool_i8:', MAXPOOL_I8)]
    c = dict(table='A', build=_maxpool, exp=exp, k=k, s=s, pad=pad, H=H, W=W, C=C, N=3, relu=relu, seed=seed, form=form,
             readers={'i32': None, 's8': [S8], 'u8': [U8]}[form], out=form == 'i32')
    c.update(kw)
    return c


# (k, s, pad, H, W, C, relu).  H != W; 17 x 18 at C = 40 is 20 blocks of 256 lanes on the byte kernel, 77 on the int32 one; the last window is cut
# by the floor division (H + 2 pad - k no multiple of s) in 2s2, 3s2p1 (W), 3s3, 5s3p1 (H) and 3s2p1_cut (both)
GEOMETRY = {
    '1s1': (1, 1, 0, 7, 5, 40, False),
    '2s2': (2, 2, 0, 7, 5, 8, True),
    '2s1p1': (2, 1, 1, 7, 5, 96, False),
    '3s2p1': (3, 2, 1, 17, 18, 40, False),
    '3s1p1': (3, 1, 1, 7, 5, 96, False),
    '3s3': (3, 3, 0, 17, 18, 8, True),
    '4s2p2': (4, 2, 2, 7, 5, 40, False),
    '5s1p2': (5, 1, 2, 7, 5, 96, False),
    '5s3p1': (5, 3, 1, 17, 18, 8, False),
    'window': (3, 2, 0, 3, 3, 96, False),                          # the map is the window: P = Q = 1
    '3s2p1_cut': (3, 2, 1, 8, 6, 40, False),
    '2s2_96_relu': (2, 2, 0, 7, 5, 96, True),                      # signed bytes behind a ReLU
}
TABLE_A = {f'a_{tag}_{form}': _mp(*row[:6], form, relu=row[6], seed=7 * i) for i, (tag, row) in enumerate(GEOMETRY.items()) for form in ('i32', 's8', 'u8')}

def _rd(seed, readers, out, **kw):
    """3 / 2 / 1 over 40 channels on 7 x 5, always on the int32 kernel."""
    return _mp(3, 2, 1, 7, 5, 40, 'i32', seed=seed, table='B', readers=readers, out=out, **kw)


TABLE_B = {
    'b_i32': _rd(1, None, True),
    'b_i32_u8': _rd(2, [U8], True),
    'b_two_i8': _rd(3, [S8, (4, False)], False),                   # signed and unsigned, different fraclens
    'b_three': _rd(4, [S8, (4, False), (6, False)], False, exp=[('maxpool_i32:', MAXPOOL_I32), ('requant:', ADD)]),
    'b_saturating': _rd(5, [(7, True)], True),                     # a right shift by 6: both clamps
}


# ---- table C: the global sum pool
def _gap(g, x0, c):
    if c.get('wrap'):
        # 64 pixels of about +2^25 + 2^18 c (even channels) and -1.5 x 2^24 (odd ones): int64 sums in [2^31, 2^32) and around -1.5 x 2^30
        C = c['C']
        b = np.where(np.arange(C) % 2 == 0, 2 ** 25 + 2 ** 18 * np.arange(C), -3 * 2 ** 23).astype(np.int32)
        src = g.conv(x0, _w(330, (C, 8, 1, 1), 40.0), b, pad=0, groups=1, weight_fl=5, input_fl=X_FL, input_signed=False, relu=False, quant_input=False)
    else:
        src = producer(g, x0, 0, c['C'], 9, w_fl=5, relu=c['relu'], seed=c['seed'])
    pl = g.avgpool_sum(src, c['shift'])
    return _tail(g, pl, c), [pl]


def _gp(H, W, C, N, form, **kw):
    """form: 'i32' (the pooled vector is the output), 'i8' (one reader), 'two' (two readers).  The pool's shift is ceil(log2 HW): sums of about
    2^(13 + shift) at fraclen 13 + shift, a right shift by 8 in front of a reader at fraclen 5."""
    c = dict(table='C', build=_gap, exp=[('avgpool_sum:', AVGPOOL)], H=H, W=W, C=C, N=N, relu=False, seed=H * W, form=form, shift=int(np.ceil(np.log2(H * W))),
             readers={'i32': None, 'i8': [S8], 'two': [S8, (6, False)]}[form], out=form == 'i32')
    c.update(kw)
    return c


# eight lanes per (image, 4 channels): N Cs / 4 items of 8 lanes — 8 (C = 8, N = 1: one wave of a 256-lane workgroup), 16, 24, 48, 72 (partial last
# workgroups and waves) and, with the spare image and at N - 1, the counts between
TABLE_C = {
    'c_hw1': _gp(1, 1, 40, 3, 'i32'),
    'c_hw3': _gp(1, 3, 96, 1, 'i8'),
    'c_hw8': _gp(2, 4, 8, 3, 'two'),
    'c_hw9_8_n1': _gp(3, 3, 8, 1, 'i32'), 'c_hw9_8_n3': _gp(3, 3, 8, 3, 'i8'),
    'c_hw9_40_n1': _gp(3, 3, 40, 1, 'two', relu=True), 'c_hw9_40_n3': _gp(3, 3, 40, 3, 'i32'),
    'c_hw9_96_n1': _gp(1, 9, 96, 1, 'i8'), 'c_hw9_96_n3': _gp(1, 9, 96, 3, 'two'),
    'c_hw49': _gp(7, 7, 40, 3, 'i32', relu=True),
    'c_hw64': _gp(4, 16, 96, 3, 'i8'),
    'c_hw200': _gp(10, 20, 8, 1, 'two'),
    'c_hw200_96': _gp(10, 20, 96, 3, 'i32'),
    'c_wrap': _gp(4, 16, 40, 3, 'i32', wrap=True),
}


# ---- table D: the join and the stand-alone requant
def _operand(g, x0, k, C, fl, n, planted):
    """A 1x1 conv of the input at fraclen fl with values around +-2^n; planted {channel: (bias, live)}: the channel's bias is set by hand, its
    weights are zero (the channel is that value everywhere) unless live (the value plus about +-2^13 of weights x pixels)."""
    w = _w(340 + 5 * k, (C, 8, 1, 1), 12.0)
    b = _b(341 + 5 * k, C, 2.0 ** n)
    for ch, (v, live) in planted.items():
        b[ch] = v - (int(round(127.5 * w[ch].sum())) if live else 0)       # (live: the products of inputs 0 .. 255 are centred on 0)
        if not live:
            w[ch] = 0
    return g.conv(x0, w, b, pad=0, groups=1, weight_fl=fl - X_FL, input_fl=X_FL, input_signed=False, relu=False, quant_input=False)


def _join(g, x0, c):
    """Two 1x1 convs of the input at fraclens a and b, joined.  Both operands are network outputs too (behind the join's): a conv that nothing else
    reads would carry the join in its epilogue, and the stand-alone launch is what is under test."""
    d = c['d']
    lo, hi = 10, 10 + abs(d)
    fa, fb = (hi, lo) if d >= 0 else (lo, hi)
    pa, pb = c.get('plant', ({}, {}))
    a = _operand(g, x0, 0, c['C'], fa, 13 + (abs(d) if fa == hi else 0), pa)
    b = _operand(g, x0, 1, c['C'], fb, 13 + (abs(d) if fb == hi and d else 0), pb)
    t = g.add(a, b, relu=c['relu'])
    outs = _tail(g, t, c)
    g.output(a)
    g.output(b)
    return outs + [a, b], [t]


def _requant_behind(g, x0, c):
    """A third int8 format behind a conv ('conv') or behind a max-pool on the int32 kernel ('pool'): the stand-alone requant."""
    src = _pool_source(g, x0, c)
    t = g.maxpool(src, 3, 2, 1) if c['behind'] == 'pool' else src
    return _tail(g, t, c), [t]


def _jn(d, C, N, H, W, form, relu, **kw):
    """d = fraclen(a) - fraclen(b); the join's result is at fraclen 10 + |d| with values around 2^(13 + |d|): readers at fraclens 1 and 2."""
    rd = {'i32': None, 'i32_i8': [(1, True)], 'two': [(1, True), (2, False)], 'three': [(1, True), (2, False), (0, True)]}[form]
    exp = [('add:', ADD)] + ([('requant:', ADD)] if form == 'three' else [])
    c = dict(table='D', build=_join, exp=exp, d=d, C=C, N=N, H=H, W=W, relu=relu, form=form, readers=rd, out=form in ('i32', 'i32_i8'))
    c.update(kw)
    return c


def _extremes(d):
    """Channels 0 .. 5 of both operands by hand, for a join whose operand b shifts left by d (d >= 0): the aligned sums are
    2^31 - 1 + 0 (kept), -2^31 + 0 (the clamp's one victim), 2^30 + 2^30 = 2^31 -> wraps to -2^31 -> clamped, -2^30 - 2^30 -> clamped,
    and two live channels around +-2^31 whose sums fall on both sides of the wrap."""
    a = {0: (I32_MAX, False), 1: (I32_MIN, False), 2: (2 ** 30, False), 3: (-2 ** 30, False), 4: (2 ** 30, True), 5: (-2 ** 30, True)}
    b = {0: (0, False), 1: (0, False), 2: (2 ** 30 >> d, False), 3: (-(2 ** 30 >> d), False), 4: (2 ** 30 >> d, True), 5: (-(2 ** 30 >> d), True)}
    return a, b


# M = N H W: 1, 33 and 3 x 7 x 9 = 189 at N (and 2, 44, 252 on the handle's spare image)
TABLE_D = {
    'd_eq_i32': _jn(0, 8, 1, 1, 1, 'i32', False),
    'd_eq_relu_two': _jn(0, 96, 3, 7, 9, 'two', True),
    'd_p1_i32_i8': _jn(1, 96, 3, 1, 11, 'i32_i8', True),
    'd_m1_three': _jn(-1, 8, 3, 7, 9, 'three', False),
    'd_p5_two': _jn(5, 8, 3, 1, 11, 'two', False),
    'd_p5_relu_i32': _jn(5, 96, 1, 1, 1, 'i32', True),
    'd_m5_relu_three': _jn(-5, 96, 3, 7, 9, 'three', True),
    'd_m5_i32_i8': _jn(-5, 8, 1, 1, 1, 'i32_i8', False),
    'd_p12_relu_i32_i8': _jn(12, 8, 3, 7, 9, 'i32_i8', True),
    'd_p12_two': _jn(12, 96, 3, 1, 11, 'two', False),
    # the extremes: both clamps of clamp_sym31's range on the NHWC-tiled int32 path, with and without the ReLU, next to int8 forms
    'd_ext_eq_i32': _jn(0, 8, 3, 7, 9, 'i32', False, plant=_extremes(0)),
    'd_ext_p5_relu_i32_i8': _jn(5, 96, 3, 1, 11, 'i32_i8', True, plant=_extremes(5)),
    'd_ext_p12_three': _jn(12, 8, 3, 7, 9, 'three', False, plant=_extremes(12), out=True),      # int32 and three int8 formats
    # requant: alone (b == nullptr)
    'd_rq_conv_signed': dict(table='D', build=_requant_behind, behind='conv', exp=[('requant:', ADD)], C=40, N=3, H=7, W=9, relu=False, seed=11,
                             readers=[U8, (4, False), (6, True)], out=False),
    'd_rq_conv_unsigned': dict(table='D', build=_requant_behind, behind='conv', exp=[('requant:', ADD)], C=96, N=1, H=1, W=11, relu=False, seed=12,
                               readers=[S8, (4, True), (6, False)], out=False),
    'd_rq_pool_signed': dict(table='D', build=_requant_behind, behind='pool', exp=[('maxpool_i32:', MAXPOOL_I32), ('requant:', ADD)], C=8, N=3, H=7, W=9,
                             relu=False, seed=13, readers=[U8, (4, False), (6, True)], out=False),
    'd_rq_pool_unsigned': dict(table='D', build=_requant_behind, behind='pool', exp=[('maxpool_i32:', MAXPOOL_I32), ('requant:', ADD)], C=96, N=3, H=7, W=9,
                               relu=False, seed=14, readers=[S8, (4, True), (6, False)], out=False),
}


# ---- table E: the classifier
def _fc(g, x0, c):
    """input -> 1x1 producer to `features` channels (fraclen 13) -> [global sum pool of the H x W map, fraclen 19] -> linear to `classes`, the
    network output: the classifier writes the caller's buffer itself (`linear_dense:`) where the padded feature count has an instance."""
    F = c['features']
    t = producer(g, x0, 0, F, 9, w_fl=5, relu=not c['signed'], seed=c['seed'])
    fl = 13
    ops = []
    if c['H'] * c['W'] > 1:
        t = g.avgpool_sum(t)
        ops.append(t)
        fl = 19
    sh = 9 + int(np.ceil(np.log2(c['H'] * c['W'])))
    w = _w(350 + c['seed'], (c['classes'], F), c.get('w_sig', 30.0))
    b = _b(351 + c['seed'], c['classes'], 2.0 ** 16)
    for ch, v in c.get('bias', {}).items():
        b[ch] = v
    out = g.linear(t, w, b, weight_fl=6, input_fl=fl - sh, input_signed=c['signed'], label='fc')
    g.output(out, as_float=c.get('as_float', False))
    return [out], ops + [out]


def _cl(features, classes, N, *, H=1, W=1, signed=False, dense=True, **kw):
    exp = ([('avgpool_sum:', AVGPOOL)] if H * W > 1 else []) + ([('linear_dense:', fc_symbol(features))] if dense else [])
    c = dict(table='E', build=_fc, exp=exp, features=features, classes=classes, N=N, H=H, W=W, signed=signed, seed=features % 97 + classes, cin=8)
    c.update(kw)
    return c


# K = the padded features: 512 and 2048 are one and four MFMA steps per wave, 1024 and 1280 split NKW = 4 and 5 steps over each of the eight waves;
# 500 and 1250 pad up (the pad bytes and the pad weights are zeros).  Images: N and N - 1 from a handle for N + 1 — 33 and 32 images are two workgroups
# (the second with one live image) and one full one; classes 1 .. 33 either side of the 32-class tile, 1000 = 31 full tiles and one of 8
TABLE_E = {
    'e_512_10': _cl(512, 10, 3),
    'e_500_33_pooled_signed': _cl(500, 33, 3, H=2, W=3, signed=True),
    'e_1024_32_pooled': _cl(1024, 32, 1, H=3, W=3),
    'e_1024_1_signed': _cl(1024, 1, 3, signed=True),
    'e_1280_33': _cl(1280, 33, 3),
    'e_1250_10_pooled': _cl(1250, 10, 3, H=2, W=3),
    'e_2048_1000_pooled': _cl(2048, 1000, 3, H=2, W=3),
    'e_2048_32_signed': _cl(2048, 32, 1, signed=True),
    'e_512_33_n33': _cl(512, 33, 33),
    'e_1280_10_bias_wrap': _cl(1280, 10, 3, bias={k: I32_MAX if k < 4 else -I32_MAX for k in range(8)}),
    'e_1024_10_float': _cl(1024, 10, 3, as_float=True, w_sig=60.0, bias={0: 2 ** 30 + 1, 1: -(2 ** 30) - 3, 2: 2 ** 25 + 1}),
    'e_500_10_float_pooled': _cl(500, 10, 3, H=2, W=3, as_float=True),
    # 256 features have no fc_dense instance: the linear runs on conv_igemm_kernel and the output launch copies the logits
    'e_256_10_not_dense': _cl(256, 10, 3, dense=False, exp=[('conv1x1s1_t128x32x64:', IGEMM_256)]),
}


# ---- the four in a row (the pipelined test's graph): two max-pools on 512 channels, joined, summed over the map, classified
def _row(g, x0, c):
    """The join's sums are about 2^14 per pixel, 12 pixels: a right shift by 13 in front of the classifier at fraclen 6."""
    ps = [g.maxpool(producer(g, x0, k, 512, 9, w_fl=5, relu=bool(k), seed=c['seed']), 3, 2, 1) for k in range(2)]
    j = g.add(ps[0], ps[1], relu=True)
    pooled = g.avgpool_sum(j)
    out = g.linear(pooled, _w(360, (10, 512), 30.0), _b(361, 10, 2.0 ** 16), weight_fl=6, input_fl=6, input_signed=False, label='fc')
    g.output(out)
    return [out], ps + [j, pooled, out]


ROW = {'p_pool_join_gap_fc': dict(table='P', build=_row, N=3, H=7, W=5, seed=3, classes=10,
                                  exp=[('maxpool_i32:', MAXPOOL_I32)] * 2 + [('add:', ADD), ('avgpool_sum:', AVGPOOL), ('linear_dense:', fc_symbol(512))])}

CASES = dict(TABLE_A, **TABLE_B, **TABLE_C, **TABLE_D, **TABLE_E, **ROW)
TABLES = {t: sorted(k for k, c in CASES.items() if c['table'] == t) for t in 'ABCDEP'}


def make_input(name, n=None):
    c = CASES[name]
    return synth.rand_uniform_int(5, f'glue{name}', (n or c['N'], 8, c['H'], c['W']), 0, 255).astype(np.int32)


def lines(net):
    """[(plan token, kernel symbol)] of the handle's pool, join, requant and classifier launches, in launch order — and of the linear of the one
    case that must not take the classifier kernel."""
    return [(t, k) for _, t, k in sorted(graph_cases.launch_lines(net, TOKENS) + graph_cases.launch_lines(net, 'conv', label='fc'))]


def expected(name, **opts):
    """The hand-written (token, symbol) list of the case; no option the test files set moves it."""
    return CASES[name]['exp']


# ---- the data assertions
def _border(shape, c):
    """Mask [P, Q] of the outputs whose window reaches into the padding."""
    P, Q = shape
    rows = np.array([p * c['s'] - c['pad'] < 0 or p * c['s'] - c['pad'] + c['k'] > c['H'] for p in range(P)])
    cols = np.array([q * c['s'] - c['pad'] < 0 or q * c['s'] - c['pad'] + c['k'] > c['W'] for q in range(Q)])
    return rows[:, None] | cols[None, :]


def _check_maxpool(name, c, g, outs, ops):
    (pl,) = ops
    y, fl = g.v[pl]
    if c['pad'] > 0:
        # a border output below 0 has only negative in-image taps: a pool that pads with 0 answers 0 there
        m = _border(y.shape[2:], c)
        assert m.any() and (y[:, :, m] < 0).any(), f'{name}: no negative maximum in a border window'
        if c['readers'] and c['form'] != 'i32':
            rfl, sgn = c['readers'][0]
            q = oracle.requant(y, rfl, fl, sgn)[:, :, m]
            if sgn:                                                # (an unsigned form's 0 is its least value: padding with 0 is its -inf, nothing to see)
                assert (q < 0).mean() >= 0.25, f'{name}: {(q < 0).mean():.2f} of the signed border bytes are negative'
    if c['C'] == 96:
        # channels c, c + 16 (the other 16-byte half), c + 32 and c + 64 (the other 32-byte groups) carry different values, in every form compared
        v = y if c['form'] == 'i32' else oracle.requant(y, c['readers'][0][0], fl, c['readers'][0][1])
        distinct = 0
        for ch in range(16):
            four = [v[:, ch + o] for o in (0, 16, 32, 64)]
            distinct += all(not np.array_equal(four[i], four[j]) for i in range(4) for j in range(i))
        assert distinct >= 12, f'{name}: only {distinct} of 16 channels differ from those 16 / 32 / 64 channels on'
    if name == 'b_saturating':
        q = oracle.requant(y, c['readers'][0][0], fl, True)
        assert (q == 127).sum() > 10 and (q == -127).sum() > 10 and (np.abs(q) < 127).sum() > 10, f'{name}: a clamp is not reached'


def _check_gap(name, c, g, outs, ops):
    (pl,) = ops
    if c.get('wrap'):
        src = next(v for t, (v, fl) in g.v.items() if v.shape[2:] == (c['H'], c['W']) and v.shape[1] == c['C'])
        exact = src.astype(np.int64).sum(axis=(2, 3))
        assert (exact >= 2 ** 31).any() and (exact < 2 ** 32).all() and (exact <= -2 ** 30).any(), f'{name}: the exact sums do not leave the int32 range'
        assert (exact != g.v[pl][0].reshape(exact.shape)).any()


def _check_join(name, c, g, outs, ops):
    if c['build'] is not _join:
        return
    (t,) = ops
    a, b = outs[-2:]
    (xa, fa), (xb, fb) = g.v[a], g.v[b]
    raw = ((xa.astype(np.int64) << max(fb - fa, 0)) + (xb.astype(np.int64) << max(fa - fb, 0))).astype(np.uint64).astype(np.uint32).astype(np.int32)
    np.testing.assert_array_equal(g.v[t][0], np.maximum(np.maximum(raw, -I32_MAX), 0 if c['relu'] else I32_MIN))      # (the join restated: wrap, clamp, ReLU)
    if c['relu']:
        assert (raw < 0).mean() > 0.1, f'{name}: the ReLU has nothing to do'
    if 'plant' in c:
        exact = (xa.astype(np.int64) << max(fb - fa, 0)) + (xb.astype(np.int64) << max(fa - fb, 0))
        assert (raw == I32_MIN).sum() >= 3 and (raw != I32_MIN).sum() > 100, f'{name}: clamp_sym31 changes nothing, or everything'
        assert (xa == I32_MAX).any() and (xa == I32_MIN).any() and (np.abs(xa) == 2 ** 30).any()
        for ch in (4, 5):                                          # the live channels cross +-2^31 in some pixels and stay inside in others
            e = exact[:, ch]
            assert ((np.abs(e) >= 2 ** 31).any() and (np.abs(e) < 2 ** 31).any()), f'{name}: channel {ch} does not cross 2^31'


def _check_fc(name, c, g, outs, ops):
    y = g.v[outs[0]][0].reshape(-1, c['classes'])
    if c['N'] == 33:
        assert np.count_nonzero(y[32]) == c['classes'], f'{name}: the last image has zero logits'
    if c.get('as_float') and c.get('bias'):
        assert (np.abs(y) > 2 ** 24).any() and (y.astype(np.float32).astype(np.int64) != y).any(), f'{name}: every logit is a float32 value'
    if name == 'e_1280_10_bias_wrap':
        b = np.array([c['bias'][k] for k in range(8)], np.int64)   # +-(2^31 - 1): a product sum of the bias's sign wraps the logit to the other sign
        wrapped = np.sign(y[:, :8]) != np.sign(b)
        assert wrapped.any() and not wrapped.all(), f'{name}: {wrapped.sum()} of {wrapped.size} logits wrap past the bias'


def check_data(name, g, outs, ops):
    """What the tables promise about every case's data, on the reference alone, so that a wrong kernel cannot hide behind it."""
    c = CASES[name]
    {'A': _check_maxpool, 'B': _check_maxpool, 'C': _check_gap, 'D': _check_join, 'E': _check_fc, 'P': lambda *a: None}[c['table']](name, c, g, outs, ops)
    floor = 1 if c.get('classes') == 1 else 8                      # no case compares an all-equal output
    for o in outs:
        assert np.unique(g.v[o][0]).size > floor, f'{name}: output of {np.unique(g.v[o][0]).size} distinct values'


graph_cases.bind_cases(sys.modules[__name__], check_data=check_data)      # build_graph, reference (asserts check_data), plan, int_graph
