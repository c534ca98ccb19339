"""Case table, reference and graph builder of the tests of channel slice and channel shuffle (f8_net_slice / f8_net_channel_shuffle, `F8Net.slice` /
`split` / `channel_shuffle`, f8_chanmap.hip): tests/test_chanmap_plan.py (acceptance, refusals, tokens, kernel symbols, launch_info, where the ops cut
fused launches, ONNX, the host code under the sanitizers; no GPU) and tests/test_gpu_chanmap.py (every case on both legs, bit for bit on the device).
No test functions here.

The reference is numpy fancy indexing on the int32 tensors the reference graph carries (tests/ref_ops.py):
`channel_shuffle(x, g) = x[:, (c % g) * (C / g) + c / g]`, `channel_slice(x, a, n) = x[:, a : a + n]`; test_chanmap_plan.py pins both to
torch.nn.functional.channel_shuffle / torch.split for every (C, groups) and (first, channels) of the table.  A concat in front of a shuffle is
ref_ops.concat_align.

Unless a builder says otherwise a case is  input (8 channels, 0 .. 255, fraclen 8) -> one 1x1 producer conv per source, random weights (no two
channels carry the same values) -> the op -> readers: one 32-output 1x1 conv per (input_fl, signed), summed.  Maps are 7 x 7 at N = 3 (147 pixels:
a ragged I32T block), one 9 x 11, one [C, 1, 1] at N = 2.

The expected plan tokens and kernel symbols of every case — `exp`: option chanmap_i8 = 1 (the default plan, also with every fusing pass on), `exp0`:
chanmap_i8 = 0, `nofuse`: fuse_shuffle = 0 — are WRITTEN BY HAND in launch order, the concat launches among them (the rule: DESIGN.md 4.5m); nothing
here asks the planner for them."""
import sys

import numpy as np

import graph_cases
from concat_cases import FUSE_ALL, X_FL, producer, readers  # noqa: F401  (the tests take FUSE_ALL from here)
from f8net_amd import synth
from ir_cases import _b, _w
from refgraph import record_int_graph


# ---- the builders.  Each returns (output tensor ids in output order, [slice / shuffle tensor ids in launch order])
def _source(g, x0, c, C):
    """The op's source: a 1x1 conv of the input with C outputs at fraclen 13, scaled for a reader at fraclen 4 (c['vec']: of the input's average pool)."""
    if c.get('vec'):
        return producer(g, g.avgpool_sum(x0), 0, C, 9, w_fl=5, relu=c['relu'], quant_input=True)
    return producer(g, x0, 0, C, 9, w_fl=5, relu=c['relu'])


def _tail(g, t, c):
    """Readers behind the op, or the op itself as the output (readers=None)."""
    if not c['readers']:
        g.output(t, as_float=c.get('as_float', False))
        return t
    out = readers(g, t, c['readers'])
    g.output(out)
    return out


def _shuffle(g, x0, c):
    s = g.channel_shuffle(_source(g, x0, c, c['C']), c['groups'], label='op')
    return [_tail(g, s, c)], [s]


def _shuffle_join(g, x0, c):
    """The shuffle joined with another conv of the input: the join reads int32."""
    s = g.channel_shuffle(_source(g, x0, c, c['C']), c['groups'], label='op')
    other = producer(g, x0, 5, c['C'], 8, w_fl=4, relu=False)              # fraclen 12 against 13: the join shifts it by 1
    out = readers(g, g.add(s, other, relu=True), [(4, False)])
    g.output(out)
    return [out], [s]


def _shuffle_input(g, x0, c):
    """The net input itself (8 channels up to +-2^28 at fraclen 2): nothing bounds it, and the byte mode needs no bound."""
    s = g.channel_shuffle(x0, c['groups'], label='op')
    return [_tail(g, s, c)], [s]


def _shuffle_twice(g, x0, c):
    s1 = g.channel_shuffle(_source(g, x0, c, c['C']), 2, label='op1')
    s2 = g.channel_shuffle(s1, 3, label='op2')
    return [_tail(g, s2, c)], [s1, s2]


def _slice(g, x0, c):
    s = g.slice(_source(g, x0, c, c['C']), c['first'], c['first'] + c['channels'], label='op')
    return [_tail(g, s, c)], [s]


def _slice_two(g, x0, c):
    """Two slices of one tensor (torch.split(x, [32, 32])), read at unsigned fraclen 4 and at signed fraclen 3: the source is written in both formats."""
    a, b = g.split(_source(g, x0, c, 64), [32, 32])
    out = g.add(readers(g, a, [(4, False)]), readers(g, b, [(3, True)]))
    g.output(out)
    return [out], [a, b]


def _slice_input(g, x0, c):
    s = g.slice(x0, c['first'], c['first'] + c['channels'], label='op')
    return [_tail(g, s, c)], [s]


def _operands(g, x0, c):
    """The operands of a concat: cc._plain's producers (w_fl per operand), or cc._gapneg's (c['fmt']: (input_fl, weight_fl) per operand — operands whose
    own shift n_i = n - (cat.fl - fl_i) is NEGATIVE), or the raw input next to a conv of it (c['raw'])."""
    if c.get('raw'):
        return [x0, producer(g, x0, 0, c['Cs'][1], 5, w_fl=9, relu=False, in_fl=0, in_signed=True, quant_input=True)]
    if 'fmt' not in c:
        shift = (max(c['w_fl']) + X_FL) - c['readers'][0][0]
        return [producer(g, x0, k, ci, shift - (max(c['w_fl']) - wf), w_fl=wf, relu=c['relu']) for k, (ci, wf) in enumerate(zip(c['Cs'], c['w_fl']))]
    fls = [i + w for i, w in c['fmt']]
    n = max(fls) - c['readers'][0][0]
    ps = []
    for k, (ci, (i, w)) in enumerate(zip(c['Cs'], c['fmt'])):
        ni = n - (max(fls) - (i + w))
        wt = _w(300 + k, (ci, 8, 1, 1), float(np.clip(2.0 ** (ni + (8 - i)) * 0.3, 0.5, 20.0)))
        ps.append(g.conv(x0, wt, _b(310 + k, ci, 2.0 ** max(ni, 0) * 10, 2.0 ** max(ni, 0) * 20), pad=0, groups=1, weight_fl=w, input_fl=i, input_signed=False,
                         relu=c['relu'], quant_input=i != X_FL))
    return ps


def _cat_shuffle(g, x0, c):
    """concat -> shuffle -> readers (c['second']: the concat has a second reader, a conv in the shuffle's format)."""
    cat = g.concat(_operands(g, x0, c), label='cat')
    s = g.channel_shuffle(cat, c['groups'], label='op')
    out = readers(g, s, c['readers'])
    if c.get('second'):
        out = g.add(out, g.conv(cat, _w(97, (32, sum(c['Cs']), 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=c['readers'][0][0],
                                input_signed=c['readers'][0][1], relu=False))
    g.output(out)
    return [out], [s]


S16, S4, S2, SG = 'f8::shuffle_i8_kernel<16>', 'f8::shuffle_i8_kernel<4>', 'f8::shuffle_i8_kernel<2>', 'f8::shuffle_i8_general_kernel'
LT, LF, K32 = 'f8::slice_i8_kernel<true>', 'f8::slice_i8_kernel<false>', 'f8::chanmap_i32_kernel'
CT, CF, C32 = 'f8::concat_i8_kernel<true>', 'f8::concat_i8_kernel<false>', 'f8::concat_i32_kernel'


def _i32(exp):
    """The chanmap_i8 = 0 plan of a case without a concat: every launch in the int32 mode."""
    return [(t.replace('_i8:', '_i32:'), K32) for t, _ in exp]


def _case(build, exp, exp0=None, H=7, W=7, N=3, **kw):
    c = dict(build=build, exp=exp, exp0=_i32(exp) if exp0 is None else exp0, H=H, W=W, N=N, relu=True, readers=[(4, False)], cin=8, x_fl=X_FL)
    c.update(kw)
    return c


def _sh(groups, C, sym, **kw):
    return _case(_shuffle, [(f'shuffle{groups}_i8:', sym)], groups=groups, C=C, **kw)


def _sl(first, channels, C, sym, **kw):
    return _case(_slice, [('slice_i8:', sym)], first=first, channels=channels, C=C, **kw)


def _fused(Cs, groups, sym, cat_sym, alone_sym, **kw):
    """A concat + shuffle that plans as one launch; fuse_shuffle = 0: the concat in its byte mode (cat_sym), then the stand-alone shuffle (alone_sym)."""
    tok = f'shuffle{groups}'
    kw.setdefault('w_fl', [5] * len(Cs))
    return _case(_cat_shuffle, [(f'concat+{tok}_i8:', sym)], [('concat_i32:', C32), (f'{tok}_i32:', K32)], groups=groups, Cs=list(Cs),
                 nofuse=[('concat_i8:', cat_sym), (f'{tok}_i8:', alone_sym)], **kw)


def _two(Cs, groups, exp, **kw):
    """A concat + shuffle that plans as two launches whatever fuse_shuffle says."""
    return _case(_cat_shuffle, exp, [('concat_i32:', C32), (f'shuffle{groups}_i32:', K32)], groups=groups, Cs=list(Cs), w_fl=[5] * len(Cs), nofuse=exp, **kw)


CASES = {
    # ---- shuffles (groups, C): the instance by hand — V = the widest of 16 / 4 / 2 dividing C / 2 (two groups), else the general kernel
    'sh2_64': _sh(2, 64, S16),
    'sh2_352': _sh(2, 352, S16),                                               # 176 = 11 x 16: several vectors per group
    'sh2_24': _sh(2, 24, S4),
    'sh2_232': _sh(2, 232, S4),                                                # 116 = 29 x 4
    'sh2_116': _sh(2, 116, S2),                                                # 58 = 29 x 2; 12 pad channels
    'sh2_58': _sh(2, 58, SG),                                                  # an odd half
    'sh3_24': _sh(3, 24, SG, H=9, W=11, N=2),
    'sh4_16': _sh(4, 16, SG),                                                  # (groups == C / groups: this permutation is its own inverse)
    'sh4_48': _sh(4, 48, SG),
    'sh8_24': _sh(8, 24, SG, vec=True, N=2),                                   # a [C, 1, 1] map: M = 2
    'sh8_256': _sh(8, 256, SG),
    'sh_twoforms': _sh(2, 64, S16, relu=False, readers=[(3, True), (4, False)]),
    'sh_threeforms': _case(_shuffle, [('shuffle2_i32:', K32)], groups=2, C=64, relu=False, readers=[(3, True), (4, False), (5, False)]),
    'sh_to_add': _case(_shuffle_join, [('shuffle2_i32:', K32)], groups=2, C=64),
    'sh_to_out': _case(_shuffle, [('shuffle3_i32:', K32)], groups=3, C=24, readers=None),
    'sh_to_out_f32': _case(_shuffle, [('shuffle2_i32:', K32)], groups=2, C=116, readers=None, as_float=True),
    'sh_input': _case(_shuffle_input, [('shuffle2_i8:', S4)], groups=2, C=8, x_fl=2, raw=True, readers=[(4, True)]),
    'sh_twice': _case(_shuffle_twice, [('shuffle2_i8:', S4), ('shuffle3_i8:', SG)], C=24),
    # ---- slices (first, channels, C): ALIGNED where first is a multiple of 16
    'sl_0_58': _sl(0, 58, 116, LT),
    'sl_58_58': _sl(58, 58, 116, LF),
    'sl_16_32': _sl(16, 32, 64, LT),
    'sl_32_16': _sl(32, 16, 64, LT),
    'sl_17_30': _sl(17, 30, 64, LF),
    'sl_49_15': _sl(49, 15, 64, LF),                                           # straddles dwords
    'sl_29_29': _sl(29, 29, 58, LF),                                           # ends at the source's last real channel; unsigned form: the zero is 0x80
    'sl_0_1': _sl(0, 1, 8, LT),
    'sl_two': _case(_slice_two, [('slice_i8:', LT), ('slice_i8:', LT)]),
    'sl_to_out': _case(_slice, [('slice_i32:', K32)], first=17, channels=30, C=64, readers=None),
    'sl_input': _case(_slice_input, [('slice_i8:', LF)], first=2, channels=5, C=8, x_fl=2, raw=True, readers=[(4, True)]),
    # ---- concat -> shuffle in one launch: operand i is group i at offset 0
    'f_58': _fused((58, 58), 2, S2, CF, S2),
    'f_32': _fused((32, 32), 2, S16, CT, S16),
    'f_12': _fused((12, 12), 2, S4, CF, S4),
    # operand fraclens 13 / 11, the reader at unsigned fraclen 4: n = 9 and n_i = 9, 7
    'f_58_gap': _fused((58, 58), 2, S2, CF, S2, w_fl=[5, 3]),
    'f_32_gap': _fused((32, 32), 2, S16, CT, S16, w_fl=[3, 5]),
    # operand fraclens 11 / 7, the reader at unsigned fraclen 8: n = 3 and n_i = 3, -1 (that producer writes through the left-shift branch); no ReLU, so that
    # no channel is dead: the reader's clamp at 0 does what the ReLU did
    'f_12_neg': _fused((12, 12), 2, S4, CF, S4, fmt=[(8, 3), (5, 2)], readers=[(8, False)], relu=False),
    'f_32_neg': _fused((32, 32), 2, S16, CT, S16, fmt=[(5, 2), (8, 3)], readers=[(8, False)], relu=False),
    'f_16x4': _fused((16,) * 4, 4, SG, CT, SG),
    'f_twoforms': _fused((32, 32), 2, S16, CT, S16, relu=False, readers=[(3, True), (4, False)]),
    # ---- concat -> shuffle in two launches
    'u_unequal': _two((64, 32), 2, [('concat_i8:', CT), ('shuffle2_i8:', S16)]),               # 96 channels, groups of 48: group i is not operand i
    'u_second': _two((32, 32), 2, [('concat_i8:', CT), ('shuffle2_i8:', S16)], second=True),
    'u_raw': _two((8, 8), 2, [('concat_i32:', C32), ('shuffle2_i8:', S4)], x_fl=2, raw=True, readers=[(4, True)]),      # nothing bounds the input: (c) fails
}
SHUFFLES = sorted({(c['groups'], c['C']) for c in CASES.values() if c['build'] is _shuffle})
SLICES = sorted({(c['first'], c['channels'], c['C']) for c in CASES.values() if c['build'] is _slice})
FUSED = sorted(k for k, c in CASES.items() if c['exp'][0][0].startswith('concat+'))


def make_input(name, n=None):
    c = CASES[name]
    shape = (n or c['N'], c['cin'], c['H'], c['W'])
    if c.get('raw'):                                                           # up to +-2^28, and a band of small values (concat_cases' raw input)
        x = synth.rand_uniform_int(5, f'cmx{name}', shape, -2 ** 28, 2 ** 28).astype(np.int64)
        small = synth.rand_uniform_int(6, f'cms{name}', shape, -300, 300).astype(np.int64)
        x = np.where(small % 3 == 0, small, x)
        x.reshape(-1)[:4] = [2 ** 28, -2 ** 28, 2 ** 24, -2 ** 24]
        return x.astype(np.int32)
    return synth.rand_uniform_int(5, f'cmx{name}', shape, 0, 255).astype(np.int32)


def lines(net):
    """[(launch index, plan token, kernel symbol)] of the handle's slice, shuffle and concat launches, in launch order."""
    return graph_cases.launch_lines(net, ('slice_', 'shuffle', 'concat'))


def expected(name, **opts):
    """The hand-written (token, symbol) list of the case under these options."""
    c = CASES[name]
    if not opts.get('chanmap_i8', 1):
        return c['exp0']
    if not opts.get('fuse_shuffle', 1):
        return c.get('nofuse', c['exp'])
    return c['exp']


# ---- a ShuffleNet-V2 stage (1.0x: 24 -> 116 channels) in front of a small classifier
def _cv(g, t, k, cout, n, *, kernel=1, stride=1, depthwise=False, relu, in_fl, in_signed, w_fl=5, quant_input=True):
    """Conv number k of the stage, scaled so that a right shift by n (the next reader's) fills 8 bits."""
    cin = g.v[t][0].shape[1]
    groups = cin if depthwise else 1
    taps = kernel * kernel * (cin // groups)
    sig = float(np.clip(2.0 ** n * 100 / (128 * taps ** 0.5), 0.4, 40.0))
    w = _w(400 + 7 * k, (cout, cin // groups, kernel, kernel), sig)
    b = _b(500 + 7 * k, cout, 2.0 ** n * 20, 2.0 ** n * 40 if relu else 0.0)
    return g.conv(t, w, b, stride=stride, pad=kernel // 2, groups=groups, weight_fl=w_fl, input_fl=in_fl, input_signed=in_signed, relu=relu,
                  quant_input=quant_input, label=f'conv{k}')


STAGE = dict(cin=8, H=14, W=14, N=2, x_fl=X_FL, units=3)


def shufflenet_stage(g, x0):
    """input (8 channels, 14 x 14) -> 1x1 to 24 -> the stride-2 unit to 116 on 7 x 7 (branch 1: dw3x3 / 2 -> 1x1 to 58; branch 2: 1x1 -> dw3x3 / 2 -> 1x1
    to 58; concat; shuffle 2) -> two stride-1 units (split 58 / 58; the right half through 1x1 -> dw3x3 -> 1x1; concat; shuffle 2) -> 1x1 to 64 ->
    avgpool_sum -> linear to 10.  Activations behind a ReLU are read at unsigned fraclen 4, the depthwise results (no ReLU) at signed fraclen 3; the
    second stride-1 unit's last conv has weight fraclen 4, so its concat aligns operands of fraclens 8 and 7.
    (No layer geometry of it is refused by an existing rule: the stage is ShuffleNet-V2 1.0x's stage 2 cut to three units on a 14 x 14 input.)
    Returns (output id, [shuffle ids])."""
    t = _cv(g, x0, 0, 24, 9, relu=True, in_fl=X_FL, in_signed=False, quant_input=False)                       # fraclen 13
    b1 = _cv(g, t, 1, 24, 6, kernel=3, stride=2, depthwise=True, relu=False, in_fl=4, in_signed=False)          # 9
    b1 = _cv(g, b1, 2, 58, 4, relu=True, in_fl=3, in_signed=True)                                               # 8
    b2 = _cv(g, t, 3, 58, 5, relu=True, in_fl=4, in_signed=False)                                               # 9
    b2 = _cv(g, b2, 4, 58, 6, kernel=3, stride=2, depthwise=True, relu=False, in_fl=4, in_signed=False)         # 9
    b2 = _cv(g, b2, 5, 58, 4, relu=True, in_fl=3, in_signed=True)                                               # 8
    u = g.channel_shuffle(g.concat([b1, b2], label='unit0.cat'), 2, label='unit0')
    shuffles = [u]
    for k in (1, 2):
        left, right = g.split(u, [58, 58])
        r = _cv(g, right, 6 * k, 58, 5, relu=True, in_fl=4, in_signed=False)                                    # 9
        r = _cv(g, r, 6 * k + 1, 58, 6, kernel=3, depthwise=True, relu=False, in_fl=4, in_signed=False)         # 9
        r = _cv(g, r, 6 * k + 2, 58, 4 if k == 1 else 3, relu=True, in_fl=3, in_signed=True, w_fl=5 if k == 1 else 4)      # 8 / 7
        u = g.channel_shuffle(g.concat([left, r], label=f'unit{k}.cat'), 2, label=f'unit{k}')
        shuffles.append(u)
    t = _cv(g, u, 20, 64, 5, relu=True, in_fl=4, in_signed=False)                                               # 9
    p = g.avgpool_sum(t)                                                                                        # 15
    out = g.linear(p, _w(600, (10, 64), 8.0), _b(601, 10, 100.0), weight_fl=5, input_fl=4, input_signed=False, label='fc')
    g.output(out)
    return out, shuffles


def stage_input(n=None):
    return synth.rand_uniform_int(5, 'cmstage', (n or STAGE['N'], STAGE['cin'], STAGE['H'], STAGE['W']), 0, 255).astype(np.int32)


def stage_int_graph():
    """The stage as an IntGraph, op for op what shufflenet_stage records.  Returns (IntGraph, reference graph, output id)."""
    return record_int_graph(stage_input(), STAGE['x_fl'], lambda g, x0: shufflenet_stage(g, x0)[0])


graph_cases.bind_cases(sys.modules[__name__])      # build_graph, reference, plan, int_graph
