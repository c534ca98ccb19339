"""Cases of option fuse_se (f8_se.hip) for tests/test_se_plan.py and tests/test_gpu_se.py; the reference is refgraph.RefGraph.  No test functions here.
A case: input (8 channels, 0 .. 255, fraclen 8) -> 1x1 conv to C at fraclen 13 (the map x) -> avgpool_sum -> fc1 (to mid) -> fc2 (to C) -> gate -> channel
multiply of x -> a 32-output 1x1 reader -> output; the pool's shift and the layers' formats are scaled so that both requantisations fill 8 bits.  `sym`, the
fused launch's kernel instance, is WRITTEN BY HAND from the mapping rule (cout <= cin: K over lanes = true); sym None: the case matches no block.  `key`,
by hand too, is the lowest fuse_se at which the case fuses: 1 where C mid + mid C <= 2^17 (the planner's size rule), else 2."""
import math
import sys

import numpy as np

import graph_cases
from concat_cases import X_FL, readers
from f8net_amd import synth, tables
from ir_cases import _b, _w

TOKEN, TF, FT, TT = 'avgpool+fc+fc:', 'f8::se_kernel<true, false>', 'f8::se_kernel<false, true>', 'f8::se_kernel<true, true>'
U, S = False, True


def _fc(g, t, k, cout, *, w_sig, w_fl, b_sig, in_fl, signed, conv, relu, big, label):
    # Layer k: a linear, or (conv) the 1x1 conv ONNX import makes of it, with its ReLU; big: biases next to +-2^31 on two channels.
    cin = g.v[t][0].shape[1]
    w, b = _w(300 + k, (cout, cin), w_sig), _b(310 + k, cout, b_sig)
    if big:
        b[0], b[1 % cout] = 2 ** 31 - 1 - 900, -2 ** 31 + 700
    if conv:
        return g.conv(t, w.reshape(cout, cin, 1, 1), b, pad=0, groups=1, weight_fl=w_fl, input_fl=in_fl, input_signed=signed, relu=relu)
    return g.linear(t, w, b, weight_fl=w_fl, input_fl=in_fl, input_signed=signed, label=label)


def _se(g, x0, c):
    C, mid, hw = c['C'], c['mid'], c['H'] * c['W']
    xb = _b(12, C, 2.0 ** 11, 2.0 ** 11)
    if c['x'] == 'wrap':       # values next to -2^30 (the sum wraps several times) and +8e7 (49 of them pass 2^31; the reference asserts sum <= 2^32 - 1)
        xb = np.where(np.arange(C) % 2 == 0, -2 ** 30 + 5000, 80_000_000).astype(np.int32)
    xw = _w(11, (C, 8, 1, 1), 0.0 if c['x'] == 'zero' else 20.0)
    x = g.conv(x0, xw, xb * (c['x'] != 'zero'), pad=0, groups=1, weight_fl=5, input_fl=X_FL, input_signed=False, relu=c['x_relu'], quant_input=False)
    n1 = 6 + math.ceil(math.log2(hw))                                      # |x| ~ 2^13, its sum over hw pixels >> n1 fills 8 bits
    fl1 = 7 if c['s1'] else 8
    p = g.avgpool_sum(x, n1 + fl1 - 13)
    n2 = max(6, round(math.log2(10 * C ** 0.5)))                           # fc1's results ~ 10 * 100 * sqrt(C)
    fl2 = fl1 + 5 - n2
    f1 = _fc(g, p, 1, mid, w_sig=10.0, w_fl=5, b_sig=2.0 ** n2 * 20, in_fl=fl1, signed=c['s1'], conv=c['conv'], relu=c['conv'], big=c['big'], label='fc1')
    f2 = _fc(g, f1, 2, c.get('C2', C), w_sig=10.0, w_fl=10 - fl2, b_sig=2.0 ** 10, in_fl=fl2, signed=c['s2'], conv=c['conv'], relu=False, big=c['big'], label='fc2')
    if c['tail'] == 'table':                                               # fc2 read as one int8 form: the sigmoid table fused into the multiply
        gate, b_fl = g.table(f2, tables.sigmoid(4, True, 7), in_fl=4, in_signed=True, out_fl=7), 7
    else:                                                                  # ... as int32: the hard gate fused into the multiply
        gate, b_fl = g.hard_gate(f2), 5
    s = g.mul(x, gate, a_fl=6, a_signed=True, b_fl=b_fl, b_signed=False)
    outs = [f2] if c['tail'] == 'out0' else [readers(g, s, [(5, S)])]        # (fc2 is output 0: no match)
    if c['tail'] == 'both':                                                # ... as int32 AND int8: a second reader of fc2
        outs.append(g.linear(f2, _w(331, (16, c['C']), 10.0), None, weight_fl=5, input_fl=4, input_signed=True, label='second'))
    if c['tail'] == 'p_out':                                               # the pooled vector leaves the net: no match
        outs.append(p)
    if c['tail'] == 'fc1_two':                                             # fc1 has a second reader: no match
        outs.append(g.linear(f1, _w(332, (16, mid), 10.0), None, weight_fl=5, input_fl=fl2, input_signed=c['s2'], label='second'))
    for o in outs:
        g.output(o)
    return outs, [p, f1, f2]


def _case(C, mid, H=7, W=7, N=3, sym=TF, key=1, **kw):
    c = dict(build=_se, C=C, mid=mid, H=H, W=W, N=N, sym=sym, key=key, x='rand', x_relu=False, s1=S, s2=S, conv=False, big=False, tail='hgate', opts={})
    c.update(kw)
    return c


CASES = {
    # ---- geometry: one pixel; 49 pixels, N = 3: images straddle I32T blocks at 49 and 98; not square; 99 pixels, N = 2
    'px_1x1': _case(40, 12, H=1, W=1),
    'px_7x7': _case(40, 12),
    'px_5x9': _case(40, 12, H=5, W=9),
    'px_9x11': _case(40, 12, H=9, W=11, N=2),
    # ---- channels: Cs 96; mid 4; mid not a multiple of 4; an expanding pair (the mappings reversed); a second K pass and a third output pass
    'c72_m24': _case(72, 24),
    'c96_m4': _case(96, 4),
    'c144_m6': _case(144, 6),
    'c8_m40': _case(8, 40, sym=FT),
    'c1056_m264': _case(1056, 264, H=2, W=2, N=2, key=2),
    'rule_at': _case(256, 256, H=2, W=2, N=2, sym=TT),                     # ---- the size rule's two sides: 2 * 256 * 256 = 2^17 fuses with the key at 1 (both layers K over lanes); 2 * 256 * 260 only at 2
    'rule_over': _case(256, 260, H=2, W=2, N=2, sym=FT, key=2),
    'sum_wraps': _case(40, 12, x='wrap'),                                  # ---- values
    'bias_big': _case(40, 12, big=True),
    'zero_map': _case(40, 12, x='zero'),
    'fmt_us': _case(40, 12, s1=U, s2=S, x_relu=True),                      # ---- formats
    'fmt_su': _case(40, 12, s1=S, s2=U, conv=True),                        # (behind fc1's ReLU)
    'fc_convs': _case(72, 24, conv=True),                                  # both layers 1x1 convs, fc1 with ReLU
    'to_table': _case(40, 12, tail='table'),
    'to_both': _case(40, 12, tail='both'),
    'rq_float': _case(40, 12, s1=U, x_relu=True, opts=dict(requant_float=1)),
    'no_p_out': _case(40, 12, tail='p_out', sym=None),                     # ---- no match with the key on
    'no_fc1_two': _case(40, 12, tail='fc1_two', sym=None),
    'no_fc2_out0': _case(40, 12, tail='out0', sym=None),
    'no_mid_1032': _case(40, 1032, H=2, W=2, N=2, sym=None),
}


def make_input(name, n=None):
    c = CASES[name]
    return synth.rand_uniform_int(5, f'se{name}', (n or c['N'], 8, c['H'], c['W']), 0, 255).astype(np.int32)


graph_cases.bind_cases(sys.modules[__name__])                              # build_graph, reference, plan, int_graph


def lines(net):                                                            # [(plan token, kernel symbol)] of the pool launches, fused or not
    return [(t, k) for _, t, k in graph_cases.launch_lines(net, 'avgpool')]
