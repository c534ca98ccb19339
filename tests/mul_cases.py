"""Case table, reference and graph builder of the tests of the fixed-point multiply and the hard gate (f8_net_mul / f8_net_hard_gate, `F8Net.mul` /
`hard_gate` / `hard_swish`, f8_mul.hip): tests/test_mul_plan.py (the references pinned to torch in float64, acceptance, refusals, tokens, kernel
symbols, launch_info, where the ops cut fused launches, ONNX, the host code under the sanitizers; no GPU) and tests/test_gpu_mul.py (every case bit
for bit on the device, on the default plan, with every fusing pass on and with fuse_hgate = 0).  No test functions here.

The references (tests/ref_ops.py), in numpy int64 on the int32 tensors the reference graph carries:
    mul_ref       oracle.requant(a, a_fl, fl_a, a_signed) * oracle.requant(b, b_fl, fl_b, b_signed), b broadcast over H x W where it is [C, 1, 1],
                  max(., 0) where relu is set, wrapped to int32 (|product| <= 255 * 255: the wrap never acts)
    hard_gate_ref np.clip(x, -3 * 2^fl, 3 * 2^fl) + 3 * 2^fl

Unless a builder says otherwise a case is  input (8 channels, 0 .. 255, fraclen 8) -> one 1x1 producer conv per operand at fraclen 13, random weights
-> the op(s) -> readers: one 32-output 1x1 conv per (input_fl, signed), summed.  A gate vector is a linear on the input's avgpool_sum.  Maps are
7 x 7 at N = 3 (147 pixels: a ragged I32T block, and waves that span image boundaries for the broadcast), one 9 x 11 at N = 2, one [C, 1, 1] at
N = 2; C in {8, 20, 48, 64}: the 4-byte instance with its end mask, the 16-byte instance, a ragged 32-channel block.

The expected plan tokens and kernel symbols of every case — `exp`: the default plan (also with every fusing pass on), `nofuse`: fuse_hgate = 0 — are
WRITTEN BY HAND in launch order, the requant: steps of the op's result among them (the rule: DESIGN.md 4.5n); nothing here asks the planner for them."""
import sys

import numpy as np

import graph_cases
from concat_cases import FUSE_ALL, X_FL, producer, readers  # noqa: F401  (the tests take FUSE_ALL from here)
from f8net_amd import synth
from ir_cases import _b, _w
from refgraph import record_int_graph


# ---- the builders.  Each returns (output tensor ids in output order, [mul / hard-gate tensor ids in launch order])
def _source(g, x0, c, k=0):
    """Operand k: a 1x1 conv of the input with C outputs at fraclen 13, scaled for a reader at fraclen 4 (c['vec']: of the input's average pool)."""
    relu = c['src_relu'][k]
    if c.get('vec'):
        return producer(g, g.avgpool_sum(x0), 3 * k, c['C'], 9, w_fl=5, relu=relu, quant_input=True)
    return producer(g, x0, 3 * k, c['C'], 9, w_fl=5, relu=relu)


def _gate_vector(g, x0, c):
    """[C, 1, 1] at fraclen 13: a linear on the input's avgpool_sum (read at unsigned fraclen 8), values of both signs around 3 * 2^13."""
    C = c['C']
    return g.linear(g.avgpool_sum(x0), _w(41, (C, 8), 30.0), _b(42, C, 2.0 ** 13), weight_fl=5, input_fl=8, input_signed=False, label='fc')


def _fmt(c):
    return dict(a_fl=c['a'][0], a_signed=c['a'][1], b_fl=c['b'][0], b_signed=c['b'][1], relu=c['relu'])


def _tail(g, t, c):
    """Readers behind the op, or the op itself as the output (readers=None); c['join']: joined with another conv of the input first (an int32 reader);
    c['pool']: the result's average pool is a second output."""
    if c.get('join'):
        other = producer(g, next(iter(g.v)), 5, c['C'], 3, w_fl=3, relu=False, in_fl=4, in_signed=False, quant_input=True)      # fraclen 7, below the product's: the join shifts it
        t = g.add(t, other, relu=True)
    if not c['readers']:
        g.output(t)
        return [t]
    out = readers(g, t, c['readers'])
    g.output(out)
    if c.get('pool'):
        p = g.avgpool_sum(t)
        g.output(p)
        return [out, p]
    return [out]


def _mul(g, x0, c):
    m = g.mul(_source(g, x0, c, 0), _source(g, x0, c, 1), label='op', **_fmt(c))
    return _tail(g, m, c), [m]


def _square(g, x0, c):
    s = _source(g, x0, c, 0)
    m = g.mul(s, s, label='op', **_fmt(c))
    return _tail(g, m, c), [m]


def _chmul(g, x0, c):
    """a times a [C, 1, 1] vector that is NOT a hard gate: the linear's result read in b's format."""
    m = g.mul(_source(g, x0, c, 0), _gate_vector(g, x0, c), label='op', **_fmt(c))
    return _tail(g, m, c), [m]


def _se(g, x0, c):
    """The hard-sigmoid SE scale: chmul(x, hard_gate(fc)); c['second']: the gate has a second reader (a 32-output conv), so it is no part of the mul launch."""
    gate = g.hard_gate(_gate_vector(g, x0, c), label='gate')
    m = g.mul(_source(g, x0, c, 0), gate, label='op', **_fmt(c))
    outs = _tail(g, m, c)
    if c.get('second'):
        r = readers(g, gate, [(c['b'][0], False)])
        g.output(r)
        outs.append(r)
    return outs, [gate, m]


def _hswish(g, x0, c):
    """Hard-swish: mul(x, hard_gate(x)); c['second']: the gate is a network output too."""
    x = _source(g, x0, c, 0)
    gate = g.hard_gate(x, label='gate')
    m = g.mul(x, gate, label='op', **_fmt(c))
    outs = _tail(g, m, c)
    if c.get('second'):
        g.output(gate)
        outs.append(gate)
    return outs, [gate, m]


def _gate_input(g, x0, c):
    """The hard gate of the net input itself (any int32 value): the gate is the output, or read by one conv."""
    gate = g.hard_gate(x0, label='op')
    return _tail(g, gate, c), [gate]


I16, I4 = 'f8::mul_i8_kernel<false, false, 16>', 'f8::mul_i8_kernel<false, false, 4>'
B16, B4 = 'f8::mul_i8_kernel<true, false, 16>', 'f8::mul_i8_kernel<true, false, 4>'
G16, G4 = 'f8::mul_i8_kernel<true, true, 16>', 'f8::mul_i8_kernel<true, true, 4>'
W00, W01, W10, W11 = ('f8::mul_i32_kernel<false, false>', 'f8::mul_i32_kernel<false, true>', 'f8::mul_i32_kernel<true, false>',
                      'f8::mul_i32_kernel<true, true>')
HG, RQ = 'f8::hgate_kernel', 'f8::add_kernel'
U, S = False, True


def _case(build, exp, nofuse=None, H=7, W=7, N=3, **kw):
    c = dict(build=build, exp=exp, nofuse=exp if nofuse is None else nofuse, H=H, W=W, N=N, relu=False, src_relu=(True, True), readers=[(1, U)],
             cin=8, x_fl=X_FL, a=(4, U), b=(4, U))
    c.update(kw)
    return c


# fused gate cases: (fused token, its kernel, the stand-alone mul token, its kernel)
def _gated(build, tok, sym, tok2, sym2, **kw):
    kw.setdefault('b', (5, U))                                                 # the gate, 0 .. 6 at fraclen 5: 0 .. 192
    return _case(build, [(tok, sym)], [('hgate:', HG), (tok2, sym2)], **kw)


CASES = {
    # ---- element-wise, the four sign combinations.  Source fraclen 13 read at fraclen 6 (shift 7: the operands saturate, the extreme pairs occur —
    # asserted by reference()); the product at fraclen 12 read at fraclen 5: a right shift by 7 with exact ties in the data (asserted likewise)
    'mul_uu_64': _case(_mul, [('mul_i8:', I16)], C=64, a=(6, U), b=(6, U), readers=[(5, U)], extreme=(255, 255)),
    'mul_su_20': _case(_mul, [('mul_i8:', I4)], C=20, a=(6, S), b=(6, U), src_relu=(False, True), readers=[(5, S)], extreme=(-127, 255)),
    'mul_us_48': _case(_mul, [('mul_i8:', I16)], C=48, a=(6, U), b=(6, S), src_relu=(True, False), readers=[(5, S)], H=9, W=11, N=2, extreme=(255, -127)),
    'mul_ss_8': _case(_mul, [('mul_i8:', I4)], C=8, a=(6, S), b=(6, S), src_relu=(False, False), readers=[(5, S)], extreme=(-127, -127)),
    'mul_ss_relu': _case(_mul, [('mul_i8:', I4)], C=20, a=(3, S), b=(3, S), src_relu=(False, False), relu=True, readers=[(0, U)]),
    'mul_vec': _case(_mul, [('mul_i8:', I4)], C=20, vec=True, N=2, H=5, W=5),                # both operands [C, 1, 1]: element-wise on a one-pixel map, M = 2
    # ---- the readers: shift 0, a left shift, two formats, a third (requant:), int32 readers
    'mul_shift0': _case(_mul, [('mul_i8:', I4)], C=20, readers=[(8, U)]),
    'mul_shl': _case(_mul, [('mul_i8:', I4)], C=8, a=(2, U), b=(2, S), src_relu=(True, False), readers=[(5, S)]),      # fraclen 4 read at 5
    'mul_twoforms': _case(_mul, [('mul_i8:', I16)], C=64, b=(4, S), src_relu=(True, False), readers=[(1, S), (2, U)]),
    'mul_threeforms': _case(_mul, [('mul_i32:', W00), ('requant:', RQ)], C=64, b=(4, S), src_relu=(True, False), readers=[(1, S), (2, U), (0, S)]),
    'mul_to_add': _case(_mul, [('mul_i32:', W00)], C=48, join=True, readers=[(1, U)]),
    'mul_to_out': _case(_mul, [('mul_i32:', W00)], C=48, a=(4, S), src_relu=(False, True), readers=None),
    'mul_to_pool': _case(_mul, [('mul_i32:', W00)], C=20, pool=True),
    # ---- a == b: the square, in one format and in two (two forms of one tensor)
    'sq_one': _case(_square, [('mul_i8:', I16)], C=64, readers=[(1, U)]),
    'sq_two': _case(_square, [('mul_i8:', I4)], C=20, a=(4, S), b=(3, U), src_relu=(False, False), readers=[(2, S)]),
    # ---- the channel gate [C, 1, 1], no hard gate in front
    'ch_uu_64': _case(_chmul, [('chmul_i8:', B16)], C=64, b=(5, U)),
    'ch_su_20': _case(_chmul, [('chmul_i8:', B4)], C=20, a=(4, S), b=(5, U), src_relu=(False, True), readers=[(1, S)]),
    'ch_us_48': _case(_chmul, [('chmul_i8:', B16)], C=48, b=(4, S), readers=[(1, S)], H=9, W=11, N=2),
    'ch_ss_8': _case(_chmul, [('chmul_i8:', B4)], C=8, a=(4, S), b=(4, S), src_relu=(False, True), relu=True, readers=[(1, U)]),
    'ch_to_out': _case(_chmul, [('chmul_i32:', W10)], C=48, b=(4, S), readers=None),
    # ---- a hard gate fused into the launch, with fuse_hgate = 0, and with a second reader of the gate (not fusable)
    'se_64': _gated(_se, 'hgate+chmul_i8:', G16, 'chmul_i8:', B16, C=64),
    'se_20': _gated(_se, 'hgate+chmul_i8:', G4, 'chmul_i8:', B4, C=20, a=(4, S), src_relu=(False, True), readers=[(1, S)]),
    'se_48_9x11': _gated(_se, 'hgate+chmul_i8:', G16, 'chmul_i8:', B16, C=48, H=9, W=11, N=2),
    'se_to_out': _gated(_se, 'hgate+chmul_i32:', W11, 'chmul_i32:', W10, C=48, readers=None),
    'se_twoforms': _gated(_se, 'hgate+chmul_i8:', G16, 'chmul_i8:', B16, C=64, readers=[(1, U), (2, U)]),
    'se_second': _case(_se, [('hgate:', HG), ('chmul_i8:', B4)], C=20, b=(5, U), second=True),
    'hsw_64': _gated(_hswish, 'hgate+mul_i8:', W01, 'mul_i8:', I16, C=64, a=(4, S), src_relu=(False, True), readers=[(1, S)]),
    'hsw_20_9x11': _gated(_hswish, 'hgate+mul_i8:', W01, 'mul_i8:', I4, C=20, a=(4, S), src_relu=(False, True), readers=[(1, S)], H=9, W=11, N=2),
    'hsw_to_add': _gated(_hswish, 'hgate+mul_i32:', W01, 'mul_i32:', W00, C=48, a=(4, S), src_relu=(False, True), join=True),
    'hsw_second': _case(_hswish, [('hgate:', HG), ('mul_i8:', I4)], C=20, a=(4, S), b=(5, U), src_relu=(False, True), readers=[(1, S)], second=True),
    # ---- the hard gate of the raw net input: +-2^28 at fraclen 2, INT32_MIN / INT32_MAX, values exactly at +-3 * 2^fl; fraclens 0 and 28
    'hg_input_fl2': _case(_gate_input, [('hgate:', HG)], C=8, x_fl=2, raw=True, readers=None),
    'hg_input_fl0': _case(_gate_input, [('hgate:', HG)], C=8, x_fl=0, raw=True, readers=None),
    'hg_input_fl28': _case(_gate_input, [('hgate:', HG)], C=8, x_fl=28, raw=True, readers=None, H=9, W=11, N=2),
    'hg_input_read': _case(_gate_input, [('hgate:', HG)], C=8, x_fl=10, raw=True, readers=[(5, U), (3, U)]),
}
FUSED = sorted(k for k, c in CASES.items() if c['exp'] != c['nofuse'])
FORMATS = sorted({(c['a'], c['b']) for c in CASES.values() if c['build'] is not _gate_input})


def make_input(name, n=None):
    c = CASES[name]
    shape = (n or c['N'], c['cin'], c['H'], c['W'])
    if c.get('raw'):                                                           # any int32: a band around the clamp points, the extremes, the points themselves
        fl = c['x_fl']
        x = synth.rand_uniform_int(5, f'mx{name}', shape, -2 ** 28, 2 ** 28).astype(np.int64)
        near = synth.rand_uniform_int(6, f'mn{name}', shape, -4 * 2 ** fl - 4, 4 * 2 ** fl + 4).astype(np.int64)
        x = np.where(near % 3 != 0, near, x)
        x.reshape(-1)[:8] = [2 ** 28, -2 ** 28, -2 ** 31, 2 ** 31 - 1, 3 * 2 ** fl, -3 * 2 ** fl, 3 * 2 ** fl + 1, -3 * 2 ** fl - 1]
        return x.astype(np.int32)
    return synth.rand_uniform_int(5, f'mx{name}', shape, 0, 255).astype(np.int32)


def _has_ties(y, n):
    return n > 0 and bool(np.any((np.asarray(y, np.int64) & ((1 << n) - 1)) == (1 << (n - 1))))


def _check_data(name, g, outs, ops):
    """What the table promises about the DATA of reference(name): the extreme operand pairs occur, a right-shifting reader meets exact ties, values vary."""
    c = CASES[name]
    y, fl = g.v[ops[-1]]
    assert np.unique(y).size > 5, name
    for (A, B) in g.ops.values():
        if 'extreme' in c:
            assert np.any((A == c['extreme'][0]) & (np.broadcast_to(B, A.shape) == c['extreme'][1])), (name, A.min(), A.max(), B.min(), B.max())
    for rfl, _ in c['readers'] or []:
        if fl - rfl > 0 and not c.get('join'):
            assert _has_ties(y, fl - rfl), (name, fl, rfl)


graph_cases.bind_cases(sys.modules[__name__], check_data=_check_data)      # build_graph, reference (asserts _check_data), plan, int_graph


def lines(net):
    """[(launch index, plan token, kernel symbol)] of the handle's mul and hard-gate launches and of the requant: steps of their results, in launch order."""
    return [l for l in graph_cases.launch_lines(net, ('mul_', 'chmul_', 'hgate', 'requant'))
            if not l[1].startswith('requant') or net.launch_info(l[0], 1)[0].endswith(':op')]


def expected(name, **opts):
    """The hand-written (token, symbol) list of the case under these options."""
    c = CASES[name]
    return c['exp'] if opts.get('fuse_hgate', 1) else c['nofuse']


# ---- two small nets
def _cv(g, t, k, cout, n, *, kernel=1, depthwise=False, relu, in_fl, in_signed, w_fl=5, quant_input=True, label=None):
    """Conv number k, scaled so that a right shift by n (the next reader's) fills 8 bits."""
    cin = g.v[t][0].shape[1]
    groups = cin if depthwise else 1
    taps = kernel * kernel * (cin // groups)
    sig = float(np.clip(2.0 ** n * 100 / (128 * taps ** 0.5), 0.4, 40.0))
    return g.conv(t, _w(700 + 7 * k, (cout, cin // groups, kernel, kernel), sig), _b(800 + 7 * k, cout, 2.0 ** n * 20), pad=kernel // 2, groups=groups,
                  weight_fl=w_fl, input_fl=in_fl, input_signed=in_signed, relu=relu, quant_input=quant_input, label=label or f'conv{k}')


MBV3 = dict(cin=8, H=14, W=14, N=2, x_fl=X_FL)


def mbv3_block(g, x0):
    """A MobileNet-V3 block (bneck 5x5 with SE and hard-swish) between two 1x1 convs: input (8 channels, 14 x 14) -> 1x1 to 24 (the block input) ->
    1x1 expand to 72 + hard-swish -> depthwise 5x5 + hard-swish -> SE (avgpool_sum -> linear to 24 -> linear to 72 -> hard gate -> channel gate) ->
    1x1 project to 24 -> join with the block input -> 1x1 to 32 -> output.  Returns (output id, [mul / gate ids])."""
    t = _cv(g, x0, 0, 24, 9, relu=False, in_fl=X_FL, in_signed=False, quant_input=False, label='stem')                 # fraclen 13
    e = _cv(g, t, 1, 72, 8, relu=False, in_fl=4, in_signed=True, label='expand')                                       # 9; values around 3 * 2^9
    h1 = g.hard_swish(e, x_fl=3, x_signed=True, g_fl=5, label='hs1')                                                  # 8
    d = _cv(g, h1, 2, 72, 8, kernel=5, depthwise=True, relu=False, in_fl=2, in_signed=True, w_fl=7, label='dw')        # 9
    h2 = g.hard_swish(d, x_fl=3, x_signed=True, g_fl=5, label='hs2')                                                  # 8
    p = g.avgpool_sum(h2)                                                                                              # 14
    f1 = g.linear(p, _w(901, (24, 72), 6.0), _b(902, 24, 2.0 ** 8), weight_fl=5, input_fl=2, input_signed=True, label='se.fc1')       # 7
    f2 = g.linear(f1, _w(903, (72, 24), 10.0), _b(904, 72, 2.0 ** 9), weight_fl=6, input_fl=3, input_signed=True, label='se.fc2')     # 9
    gate = g.hard_gate(f2, label='se.gate')
    s = g.mul(h2, gate, a_fl=2, a_signed=True, b_fl=5, b_signed=False, label='se.scale')                               # 7
    pr = _cv(g, s, 3, 24, 6, relu=False, in_fl=1, in_signed=True, w_fl=6, label='project')                             # 7
    j = g.add(pr, t)
    out = _cv(g, j, 4, 32, 6, relu=True, in_fl=4, in_signed=True, label='tail')
    g.output(out)
    return out, [h1, h2, gate, s]


MBV3_TOKENS = [('hgate+mul_i8:', W01), ('hgate+mul_i32:', W01), ('hgate+chmul_i8:', G4)]      # hs2 is read by the pool in int32; 72 channels: V = 4
MBV3_NOFUSE = [('hgate:', HG), ('mul_i8:', I4), ('hgate:', HG), ('mul_i32:', W00), ('hgate:', HG), ('chmul_i8:', B4)]


def mbv3_input(n=None):
    return synth.rand_uniform_int(5, 'mbv3', (n or MBV3['N'], MBV3['cin'], MBV3['H'], MBV3['W']), 0, 255).astype(np.int32)


SE = dict(cin=8, H=7, W=7, N=3, x_fl=X_FL)


def se_net(g, x0, seen=None):
    """The graph the ONNX tests write, read back and plan: input -> 1x1 to 48 (ReLU) -> SE with a hard-sigmoid gate (avgpool_sum -> linear to 16 ->
    linear to 48 -> hard gate -> channel gate, ReLU on the product) -> hard-swish -> 1x1 to 32 -> output."""
    t = _cv(g, x0, 0, 48, 9, relu=True, in_fl=X_FL, in_signed=False, quant_input=False, label='stem')                  # 13
    p = g.avgpool_sum(t)                                                                                               # 19
    # (fc1's biases keep its results positive: the ONNX file's integer Div truncates where the reference's shift floors, so the file
    #  evaluated AS ONNX equals the reference only where no requantisation sees a negative value — oracle/onnx_eval.py)
    f1 = g.linear(p, _w(911, (16, 48), 2.0), _b(912, 16, 2.0 ** 8, 6000.0), weight_fl=5, input_fl=4, input_signed=False, label='fc1')  # 9
    f2 = g.linear(f1, _w(913, (48, 16), 12.0), _b(914, 48, 2.0 ** 9), weight_fl=6, input_fl=3, input_signed=True, label='fc2')         # 9
    if seen is not None:
        seen['fc1'] = g.v[f1][0]
    s = g.mul(t, g.hard_gate(f2), a_fl=4, a_signed=False, b_fl=5, b_signed=False, relu=True)                           # 9
    h = g.hard_swish(s, x_fl=2, x_signed=True, g_fl=5)                                                                 # 7
    out = _cv(g, h, 1, 32, 6, relu=False, in_fl=1, in_signed=True, label='tail')
    g.output(out)
    return out


SE_TOKENS = [('hgate+chmul_i32:', W11), ('hgate+mul_i8:', W01)]                               # the scaled map is the hard-swish's gate source: int32


def se_input(n=None):
    return synth.rand_uniform_int(5, 'senet', (n or SE['N'], SE['cin'], SE['H'], SE['W']), 0, 255).astype(np.int32)


def se_int_graph(seen=None):
    """se_net as an IntGraph, op for op what se_net records.  Returns (IntGraph, reference graph, output id)."""
    return record_int_graph(se_input(), SE['x_fl'], lambda g, x0: se_net(g, x0, seen))
