"""Case table and graph builder of tests/test_dwdeconv_plan.py and tests/test_gpu_dwdeconv.py: depthwise transposed convolutions (option dw_deconv,
f8_dwdeconv.hip).  No test functions here.

A case is  input (8 channels, 0 .. 255, fraclen 8) -> a 1x1 producer conv to C channels at fraclen 13 -> the depthwise transposed conv `up`, which
requantises them to unsigned fraclen 4 behind the producer's ReLU (shift 9) or to signed fraclen 3 (shift 10) -> one 32-output 1x1 reader per
(fraclen, signed), summed, and / or `up` itself as an int32 output.  Producer and readers are recorded through RefGraph; `up` is recorded on the handle
directly (RefGraph.conv_transpose knows no groups) and its reference value put into the graph: ref_ops.deconv_ref on the diagonal-expanded DENSE
weights [C, C, k, k].  The expected kernel symbol is WRITTEN BY HAND from f8_dwdeconv.hip: with dw_deconv = 1 the dot4 kernel of T = ceil(k / s) where
the launch writes int8 forms only and T <= 4, else — and with dw_deconv = 2 everywhere — the anchor kernel of the input's signedness."""
import numpy as np

from concat_cases import X_FL, producer, readers
from deconv_cases import deconv_lines, out_size  # noqa: F401  (the tests take them from here)
from f8net_amd import synth
from ir_cases import _b, _w
from oracle import oracle
from ref_ops import deconv_ref
from refgraph import RefGraph

U, S = (4, False), (3, True)
N = 2


def _case(k, s, pad, op, C, H, W, *, signed=False, relu=True, bias_big=False, fmts=(U,), out=False):
    assert 0 <= pad < k and 0 <= op < s and out_size(H, k, s, pad, op) >= 1 and out_size(W, k, s, pad, op) >= 1
    return dict(k=k, s=s, pad=pad, op=op, C=C, H=H, W=W, signed=signed, relu=relu, bias_big=bias_big, fmts=fmts, out=out)


CASES = {
    # ---- the geometries; maps 1 x 1, 3 x 5 and 2 x 9 (more than four anchor columns); C 4 (pad channels), 40, 64 (two 32-channel blocks)
    'g_4210': _case(4, 2, 1, 0, 40, 3, 5),                                 # T = 2 (DLA's 4x4 / 2)
    'g_4210_2x9': _case(4, 2, 1, 0, 64, 2, 9, signed=True, relu=False, fmts=(S,)),
    'g_8420': _case(8, 4, 2, 0, 4, 3, 5),                                  # T = 2 at s = 4 (DLA's 8x8 / 4)
    'g_3211': _case(3, 2, 1, 1, 40, 3, 5, fmts=(U, S), relu=False),        # T 2 / 1 mixed, output_padding, two int8 formats
    'g_2200': _case(2, 2, 0, 0, 64, 2, 9),                                 # T = 1
    'g_2301': _case(2, 3, 0, 1, 40, 3, 5, signed=True, relu=False, fmts=(S,)),      # phases without a tap store the bias
    'g_2301_1x1': _case(2, 3, 0, 1, 4, 1, 1),
    'g_5241': _case(5, 2, 4, 1, 40, 3, 5),                                 # pad = k - 1, T = 3
    'g_8230': _case(8, 2, 3, 0, 64, 3, 5),                                 # T = 4
    'g_8230_1x1': _case(8, 2, 3, 0, 40, 1, 1, signed=True, relu=False, fmts=(S,)),  # anchors past H and W
    'g_16840': _case(16, 8, 4, 0, 4, 2, 9),                                # FCN-8s' 16x16 / 8
    'g_16270': _case(16, 2, 7, 0, 40, 3, 5),                               # T = 8: the anchor kernel on every leg
    # ---- forms
    'f_out': _case(4, 2, 1, 0, 40, 3, 5, fmts=None, out=True),             # the int32 form alone
    'f_out_reader': _case(8, 4, 2, 0, 64, 2, 9, out=True),                 # both forms
    'f_out_signed': _case(3, 2, 1, 1, 4, 3, 5, signed=True, relu=False, fmts=None, out=True),
    'f_bias_big': _case(4, 2, 1, 0, 64, 3, 5, bias_big=True),              # biases near +-2^30
    'f_bias_big_out': _case(5, 2, 4, 1, 40, 3, 9, bias_big=True, relu=False, fmts=None, out=True),
}


def symbol(c, mode):
    T = -(-c['k'] // c['s'])
    if mode == 1 and not c['out'] and T <= 4:
        return f'f8::dwdeconv_dot4_kernel<{T}>'
    return 'f8::dwdeconv_kernel<%s>' % ('true' if c['signed'] else 'false')


def token(c):
    return 'dwdeconv%dx%ds%d:' % (c['k'], c['k'], c['s'])


def weights(c, seed=40):
    """[C, 1, k, k] and the bias: accumulators around 2^6 x 100, which a reader's shift of 6 turns into 8 bits."""
    taps = max(1.0, (c['k'] / c['s']) ** 2)
    w = _w(seed, (c['C'], 1, c['k'], c['k']), float(np.clip(6400.0 / (40.0 * taps ** 0.5), 0.7, 60.0)))
    b = _b(seed + 1, c['C'], 2.0 ** 11, 2.0 ** 12 if c['relu'] else 0.0)
    if c['bias_big']:
        b[0], b[3] = 2 ** 30 - 50, -(2 ** 30 - 50)
    return w, b


def dense(w):
    """[C, 1, k, k] -> the diagonal-expanded [C, C, k, k] of the same transposed conv at groups = 1."""
    C = w.shape[0]
    d = np.zeros((C, C) + w.shape[2:], w.dtype)
    d[np.arange(C), np.arange(C)] = w[:, 0]
    return d


def up(g, t, c, w, b, label='up'):
    """The depthwise transposed conv of tensor t, recorded on g.net directly; its reference value goes into g.v."""
    in_fl, sgn = S if c['signed'] else U
    o = g.net.conv_transpose(t, w, b, stride=c['s'], pad=c['pad'], output_padding=c['op'], weight_fl=6, input_fl=in_fl, input_signed=sgn, relu=c['relu'],
                             label=label, groups=w.shape[0])
    x, fl = g.v[t]
    y = deconv_ref(oracle.requant(x, in_fl, fl, sgn), dense(w), b, c['s'], c['pad'], c['op'])
    g.v[o] = (oracle.relu(y) if c['relu'] else y, in_fl + 6)
    return o


def make_input(name):
    c = CASES[name]
    return synth.rand_uniform_int(5, f'dwd{name}', (N, 8, c['H'], c['W']), 0, 255).astype(np.int32)


def plan(name, mode):
    """The case planned for N images under dw_deconv = mode.  Returns (graph, input, [output ids in output order])."""
    c = CASES[name]
    x = make_input(name)
    g = RefGraph(x, X_FL)
    g.net.set_option('dw_deconv', mode)
    t = producer(g, next(iter(g.v)), 0, c['C'], 10 if c['signed'] else 9, w_fl=5, relu=not c['signed'])
    u = up(g, t, c, *weights(c))
    outs = []
    if c['fmts']:
        outs.append(readers(g, u, c['fmts']))
    if c['out']:
        outs.append(u)
    for o in outs:
        g.output(o)
    g.net.finalize(N)
    return g, x, outs
