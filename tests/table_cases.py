"""Case table, reference and graph builder of the tests of the 256-entry table op (f8_net_table, `F8Net.table` / `sigmoid` / `swish` / `tanh`,
f8_table.hip): tests/test_table_plan.py (the tables against their definition, acceptance, refusals, tokens, kernel symbols, where the op cuts fused
launches, the host code under the sanitizers; no GPU) and tests/test_gpu_table.py (every case bit for bit on the device, on the default plan, with
every fusing pass on, with table_i8 = 0 and with fuse_table = 0).  No test functions here.

The reference (tests/ref_ops.py), in numpy on the int32 tensors the reference graph carries:
    table_ref     table[oracle.requant(x, in_fl, fl, in_signed) + (128 if in_signed else 0)]

Two families of cases.
  * The table alone (`_tab`).  The net input has C channels, 0 .. 255 at fraclen 8; the table's source is a 1x1 conv of it with a DIAGONAL weight
    matrix, so every source value is designed: even channels are the identity in the index format (weight 32 = 2^5 against a requant shift of 5; signed
    formats subtract 128), and the input's even channels walk a permutation of 0 .. 255 — EVERY reachable index (256 unsigned, 255 signed) occurs within
    the first N images, which reference() asserts: a case that reaches fewer cannot tell a wrong table order from a right one.  Odd channels have
    weights 41 .. 47 and small biases: exact ties of the round-half-even shift and both clamps occur (asserted likewise).
    Tables: uniformly random int32 (`rnd`); random with INT32_MIN, INT32_MAX and 0 at random places (`ext`); tables.sigmoid; tables.swish.  A random
    entry is read back at fraclen 30 by readers at fraclen 4 .. 6: a right shift by 24 .. 26 that fills the 8 bits, both clamps and ties included.
  * The sigmoid SE gate (`_se`): mul_cases' operands (8 input channels; a [C, 1, 1] vector from a linear on the input's average pool) with
    tables.sigmoid between the vector and the channel gate.
Maps are 7 x 7 at N = 3 (147 pixels: a ragged I32T block, waves that span images), 9 x 11 at N = 2, the [C, 1, 1] gate vector at N = 2 .. 3;
C in {8, 20, 48, 64}: the masked 4-byte instance, the 16-byte instance, a ragged 32-channel block.

The expected plan tokens and kernel symbols of every case — `exp`: the default plan (also with every fusing pass on), `nofuse`: fuse_table = 0; with
table_i8 = 0 every `table_i8:` of either list is `table_i32:` on f8::table_i32_kernel — are WRITTEN BY HAND in launch order."""
import sys

import numpy as np

import graph_cases
import mul_cases as mc
from concat_cases import FUSE_ALL, X_FL, readers  # noqa: F401  (the tests take FUSE_ALL from here)
from f8net_amd import synth, tables
from refgraph import record_int_graph

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the tables
def make_table(c):
    kind, (in_fl, sgn), out_fl = c['table'], c['in'], c['out_fl']
    if kind in ('rnd', 'ext'):
        t = synth.rand_uniform_int(7, f"tab{c['C']}{sgn}{kind}", (256,), INT32_MIN, INT32_MAX).astype(np.int64)
        if kind == 'ext':
            where = synth.rand_uniform_int(8, f"ext{c['C']}{sgn}", (256,), 0, 5)
            t = np.select([where == 0, where == 1, where == 2], [INT32_MIN, INT32_MAX, 0], t)
        return t.astype(np.int32)
    return getattr(tables, kind)(in_fl, sgn, out_fl)


# ---- the builders.  Each returns (output tensor ids in output order, [table / mul tensor ids in launch order])
def _designed_source(g, x0, c):
    """C -> C diagonal 1x1 conv at fraclen in_fl + 5: even channels give exactly the index x (unsigned) or x - 128 (signed) after the table's shift
    by 5; odd channels scale by 41 .. 47 / 32 and add a small bias: ties and both clamps."""
    C, (in_fl, sgn) = c['C'], c['in']
    w = np.zeros((C, C, 1, 1), np.int32)
    b = np.zeros(C, np.int32)
    for ch in range(C):
        w[ch, ch] = 32 if ch % 2 == 0 else 40 + ch % 8
        b[ch] = (-128 * w[ch, ch, 0, 0] if sgn else 0) + (0 if ch % 2 == 0 else 5 * ch - 200)
    return g.conv(x0, w, b, pad=0, groups=1, weight_fl=in_fl - 3, input_fl=X_FL, input_signed=False, relu=False, quant_input=False, label='src')


def _tab(g, x0, c):
    t = g.table(_designed_source(g, x0, c), make_table(c), in_fl=c['in'][0], in_signed=c['in'][1], out_fl=c['out_fl'], label='op')
    return mc._tail(g, t, c), [t]


def _se(g, x0, c):
    """The sigmoid SE scale: chmul(x, sigmoid(fc)); c['second']: the gate has a second reader (a 32-output conv), so it is no part of the mul launch."""
    gate = g.table(mc._gate_vector(g, x0, c), make_table(c), in_fl=c['in'][0], in_signed=c['in'][1], out_fl=c['out_fl'], label='gate')
    m = g.mul(mc._source(g, x0, c, 0), gate, label='op', **mc._fmt(c))
    outs = mc._tail(g, m, c)
    if c.get('second'):
        r = readers(g, gate, [(7, False)])
        g.output(r)
        outs.append(r)
    return outs, [gate, m]


T16, T4, T32 = 'f8::table_i8_kernel<16, 1>', 'f8::table_i8_kernel<4, 1>', 'f8::table_i32_kernel'
F16, F4, F32 = 'f8::table_chmul_i8_kernel<16>', 'f8::table_chmul_i8_kernel<4>', 'f8::table_chmul_i32_kernel'
RQ = mc.RQ
U, S = False, True


def _case(build, exp, nofuse=None, H=7, W=7, N=3, **kw):
    c = dict(build=build, exp=exp, nofuse=exp if nofuse is None else nofuse, H=H, W=W, N=N, relu=False, src_relu=(True, True), readers=[(6, S)],
             x_fl=X_FL, table='rnd', out_fl=30)
    c.update(kw)
    c.setdefault('cin', c['C'] if build is _tab else 8)
    return c


def _gated(tok, sym, tok2, sym2, tsym, **kw):
    """A fused sigmoid gate: [C, 1, 1] at fraclen 13 read at signed fraclen 4 (+-8), sigmoid at fraclen 12 read by the mul at unsigned fraclen 8."""
    kw.setdefault('readers', [(1, U)])
    return _case(_se, [(tok, sym)], [('table_i8:', tsym), (tok2, sym2)], table='sigmoid', out_fl=12, b=(8, U), a=kw.pop('a', (4, U)), **{'in': (4, S)}, **kw)


CASES = {
    # ---- the table alone, int8 readers: both input signs, V = 4 with its end mask and V = 16, one and two formats
    'rnd_u_8': _case(_tab, [('table_i8:', T4)], C=8, **{'in': (8, U)}),
    'rnd_s_20': _case(_tab, [('table_i8:', T4)], C=20, readers=[(6, U)], **{'in': (7, S)}),
    'rnd_u_48_9x11': _case(_tab, [('table_i8:', T16)], C=48, H=9, W=11, N=2, readers=[(6, S), (5, U)], **{'in': (5, U)}),
    'rnd_s_64': _case(_tab, [('table_i8:', T16)], C=64, readers=[(4, S)], **{'in': (4, S)}),
    'ext_u_20': _case(_tab, [('table_i8:', T4)], C=20, table='ext', readers=[(6, S), (6, U)], **{'in': (8, U)}),
    'ext_s_64_9x11': _case(_tab, [('table_i8:', T16)], C=64, H=9, W=11, N=2, table='ext', readers=[(5, S)], **{'in': (7, S)}),
    # ---- the int32 form: the result as an output, a third format (requant:), a join, a pool
    'rnd_u_64_out': _case(_tab, [('table_i32:', T32)], C=64, readers=None, **{'in': (8, U)}),
    'ext_s_48_out': _case(_tab, [('table_i32:', T32)], C=48, table='ext', readers=None, **{'in': (7, S)}),
    'rnd_s_8_three': _case(_tab, [('table_i32:', T32), ('requant:', RQ)], C=8, readers=[(6, S), (5, U), (4, S)], **{'in': (3, S)}),
    'rnd_u_20_three': _case(_tab, [('table_i32:', T32), ('requant:', RQ)], C=20, H=9, W=11, N=2, readers=[(6, S), (5, U), (4, S)], **{'in': (8, U)}),
    # ---- the functions: sigmoid of an unsigned and of a signed source, swish (signed); a join and a pool behind them
    'sig_u_64': _case(_tab, [('table_i8:', T16)], C=64, table='sigmoid', out_fl=12, readers=[(8, U)], **{'in': (5, U)}),
    'sig_s_20_9x11': _case(_tab, [('table_i8:', T4)], C=20, H=9, W=11, N=2, table='sigmoid', out_fl=12, readers=[(8, U), (7, U)], **{'in': (4, S)}),
    'swish_s_48': _case(_tab, [('table_i8:', T16)], C=48, table='swish', out_fl=10, readers=[(4, S)], **{'in': (4, S)}),
    'swish_s_20_add': _case(_tab, [('table_i32:', T32)], C=20, table='swish', out_fl=10, join=True, readers=[(3, U)], **{'in': (4, S)}),
    'sig_u_48_pool': _case(_tab, [('table_i32:', T32)], C=48, table='sigmoid', out_fl=12, pool=True, readers=[(8, U)], **{'in': (6, U)}),
    # ---- the sigmoid SE gate: fused into the broadcast mul, as two launches, with a second reader of the gate (not fusable)
    'se_64': _gated('table+chmul_i8:', F16, 'chmul_i8:', mc.B16, T16, C=64),
    'se_20': _gated('table+chmul_i8:', F4, 'chmul_i8:', mc.B4, T4, C=20, a=(4, S), src_relu=(False, True), readers=[(1, S)]),
    'se_48_9x11': _gated('table+chmul_i8:', F16, 'chmul_i8:', mc.B16, T16, C=48, H=9, W=11, N=2, readers=[(1, U), (2, U)]),
    'se_to_out': _gated('table+chmul_i32:', F32, 'chmul_i32:', mc.W10, T16, C=48, readers=None),
    'se_second': _case(_se, [('table_i8:', T4), ('chmul_i8:', mc.B4)], C=20, table='sigmoid', out_fl=12, a=(4, U), b=(8, U), readers=[(1, U)], second=True,
                       **{'in': (4, S)}),
}
FUSED = sorted(k for k, c in CASES.items() if c['exp'] != c['nofuse'])
ALONE = sorted(k for k, c in CASES.items() if c['build'] is _tab)


def make_input(name, n=None):
    c = CASES[name]
    shape = (n or c['N'], c['cin'], c['H'], c['W'])
    x = synth.rand_uniform_int(5, f'tx{name}', shape, 0, 255).astype(np.int32)
    if c['build'] is _tab:                                                     # the even channels walk a permutation of 0 .. 255, pixel by pixel
        ev = x[:, ::2]
        seq = (np.arange(ev.size, dtype=np.int64) * 97 + 13) % 256
        x[:, ::2] = seq.reshape(ev.shape[0], ev.shape[2], ev.shape[3], ev.shape[1]).transpose(0, 3, 1, 2)
    return x


def reachable(in_signed):
    return set(range(-127, 128)) if in_signed else set(range(256))


def _check_data(name, g, outs, ops):
    """What the module text promises about the DATA of reference(name) of a table-alone case: every reachable index occurs within the first N images
    AND within the first N - 1 (the two batch sizes the device runs), the source meets exact ties of the index shift and both clamps."""
    c = CASES[name]
    assert np.unique(g.v[ops[-1]][0]).size > 5, name
    if c['build'] is _tab:
        (q,) = g.idx.values()
        for n in (c['N'], c['N'] - 1):
            assert set(np.unique(q[:n]).tolist()) == reachable(c['in'][1]), (name, n, np.unique(q[:n]).size)
        src, fl = g.srcv[ops[0]]
        sh = fl - c['in'][0]
        assert sh == 5 and mc._has_ties(src, sh), name
        lo, hi = (-127, 127) if c['in'][1] else (0, 255)
        assert (np.asarray(src, np.int64) >> sh).max() > hi and ((np.asarray(src, np.int64) >> sh).min() < lo or not c['in'][1]), name


graph_cases.bind_cases(sys.modules[__name__], check_data=_check_data)      # build_graph, reference (asserts _check_data), plan, int_graph


def lines(net):
    """[(launch index, plan token, kernel symbol)] of the handle's table and mul launches and of the requant: steps of their results, in launch order."""
    return [l for l in graph_cases.launch_lines(net, ('table', 'mul_', 'chmul_', 'requant'))
            if not l[1].startswith('requant') or net.launch_info(l[0], 1)[0].endswith(':op')]


def expected_of(exp, nofuse, **opts):
    e = exp if opts.get('fuse_table', 1) else nofuse
    if not opts.get('table_i8', 1):
        e = [('table_i32:', T32) if t == 'table_i8:' else (t, k) for t, k in e]
    return e


def expected(name, **opts):
    """The hand-written (token, symbol) list of the case under these options."""
    c = CASES[name]
    return expected_of(c['exp'], c['nofuse'], **opts)


# ---- an EfficientNet MBConv block
MBCONV = dict(cin=8, H=14, W=14, N=2, x_fl=X_FL)


def _swish(g, t, label):
    """swish of a tensor at fraclen 9 read at signed fraclen 4 (+-8), the result at fraclen 8."""
    return g.table(t, tables.swish(4, True, 8), in_fl=4, in_signed=True, out_fl=8, label=label)


def mbconv_block(g, x0):
    """An EfficientNet MBConv block between two 1x1 convs: input (8 channels, 14 x 14) -> 1x1 to 24 (the block input) -> 1x1 expand to 72 -> swish ->
    depthwise 5x5 -> swish -> SE (avgpool_sum -> linear to 24 -> swish -> linear to 72 -> sigmoid table -> channel gate) -> 1x1 project to 24 -> join
    with the block input -> 1x1 to 32 -> output.  Returns (output id, [table / mul ids])."""
    _cv, _w, _b = mc._cv, mc._w, mc._b
    t = _cv(g, x0, 0, 24, 9, relu=False, in_fl=X_FL, in_signed=False, quant_input=False, label='stem')                  # fraclen 13
    e = _cv(g, t, 1, 72, 8, relu=False, in_fl=4, in_signed=True, label='expand')                                        # 9
    s1 = _swish(g, e, 'sw1')                                                                                            # 8
    d = _cv(g, s1, 2, 72, 8, kernel=5, depthwise=True, relu=False, in_fl=5, in_signed=True, w_fl=4, label='dw')          # 9
    s2 = _swish(g, d, 'sw2')                                                                                            # 8: read by the pool in int32 and by the gate in int8
    p = g.avgpool_sum(s2)                                                                                               # 14
    f1 = g.linear(p, _w(901, (24, 72), 12.0), _b(902, 24, 2.0 ** 8), weight_fl=5, input_fl=4, input_signed=True, label='se.fc1')       # 9
    s3 = _swish(g, f1, 'se.sw')                                                                                         # 8, a [24, 1, 1] table
    f2 = g.linear(s3, _w(903, (72, 24), 10.0), _b(904, 72, 2.0 ** 9), weight_fl=5, input_fl=4, input_signed=True, label='se.fc2')      # 9
    gate = g.table(f2, tables.sigmoid(4, True, 12), in_fl=4, in_signed=True, out_fl=12, label='se.gate')
    s = g.mul(s2, gate, a_fl=4, a_signed=True, b_fl=8, b_signed=False, label='se.scale')                                # 12
    pr = _cv(g, s, 3, 24, 6, relu=False, in_fl=4, in_signed=True, w_fl=3, label='project')                              # 7
    j = g.add(pr, t)
    out = _cv(g, j, 4, 32, 6, relu=True, in_fl=4, in_signed=True, label='tail')
    g.output(out)
    return out, [s1, s2, s3, gate, s]


# 72 and 24 channels: V = 4.  sw2 is read by the pool in int32.
MBCONV_TOKENS = [('table_i8:', T4), ('table_i32:', T32), ('table_i8:', T4), ('table+chmul_i8:', F4)]
MBCONV_NOFUSE = [('table_i8:', T4), ('table_i32:', T32), ('table_i8:', T4), ('table_i8:', T4), ('chmul_i8:', mc.B4)]


def mbconv_input(n=None):
    return synth.rand_uniform_int(5, 'mbconv', (n or MBCONV['N'], MBCONV['cin'], MBCONV['H'], MBCONV['W']), 0, 255).astype(np.int32)


def mbconv_int_graph():
    """mbconv_block as an IntGraph, op for op what mbconv_block records.  Returns (IntGraph, reference graph, output id)."""
    return record_int_graph(mbconv_input(), MBCONV['x_fl'], lambda g, x0: mbconv_block(g, x0)[0])


def unsigned_int_graph():
    """input -> 1x1 to 20 (ReLU) -> sigmoid table on an UNSIGNED index (no offset in the file), read by a left shift -> 1x1 to 32 -> output."""
    def build(g, x0):
        t = mc._cv(g, x0, 0, 20, 9, relu=True, in_fl=X_FL, in_signed=False, quant_input=False, label='stem')      # fraclen 13
        s = g.table(t, tables.sigmoid(5, False, 6), in_fl=5, in_signed=False, out_fl=6)
        out = mc._cv(g, s, 1, 32, 6, relu=False, in_fl=7, in_signed=False, label='tail')                          # fraclen 6 read at 7: a left shift
        g.output(out)
        return out
    return record_int_graph(mc.se_input(), X_FL, build)
