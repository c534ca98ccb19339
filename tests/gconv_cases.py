"""Case table, reference and graph builder of the tests of grouped convolutions (1 < groups < cin; option `grouped`): tests/test_gconv_plan.py
(acceptance, plan, symbols and liveness on the reference, no GPU) and tests/test_gpu_gconv.py (both legs against the reference on the device).  No
test functions here.

The reference.  `oracle.conv2d` refuses these groups (it is the reference's depthwise / plain conv) and stays as it is.  Wrapping int32 arithmetic
is order-free, so a grouped conv is the oracle applied per group and concatenated along the channels: `ref_ops.grouped_conv2d`, which RefGraph.conv
evaluates every conv with.  `grouped_oracle()` points `oracle.oracle.conv2d` at it for the time of an `oracle.graph_forward` / `net_forward`: the
whole-net walkers are the oracle's own and look the name up at call time.

Every op-level graph is  input -> grouped K x K (the conv under test; it reads the net input as it is, quant_input = False) -> output, where the
output is the grouped conv's int32 result itself (readers=None) or the sum of one 32-output 1x1 reader per (fraclen, signed) — plus the int32
result when `join_i32` is set (the launch then writes int32 next to its int8 forms).  The pipelined case chains two of them through a 1x1.

Two legs: `grouped = 1` (f8::gconv3x3_kernel<S> of f8_gconv.hip where the shape is in its set, plan token `gconv3x3s{S}:`) and `grouped = 2` (always
the dense expansion: conv_igemm_kernel over block-diagonal weights, plan token `gconv{k}x{k}s{S}_dense:`).  The expected tokens and symbols are
WRITTEN BY HAND from gconv_kernel_applies (f8_net.cpp) and gconv_kernel_name (f8_gconv.hip); nothing here asks the planner for them.  The kernel's
tile (gconv_tile): output columns in pieces of at most 64 (stride 2: 32), rows as the 48 KB patch allows, whole small images gathered up to 256
output pixels per workgroup; a workgroup covers four 32-channel slices."""
import contextlib

import numpy as np

from f8net_amd import synth
from ir_cases import PIPELINED_CASE as _IR_PIPELINED
from ir_cases import _b, _w
from oracle import oracle
from ref_ops import grouped_conv2d
from refgraph import RefGraph


@contextlib.contextmanager
def grouped_oracle():
    """`oracle.oracle.conv2d` = grouped_conv2d while the block runs (graph_forward / net_forward look the name up at call time)."""
    plain = oracle.conv2d
    oracle.conv2d = grouped_conv2d
    try:
        yield
    finally:
        oracle.conv2d = plain


def kernel(stride):
    return f'f8::gconv3x3_kernel<{stride}>'


DENSE_KERNEL = 'f8::conv_igemm_kernel<'                 # the dense expansion runs the implicit-GEMM kernel (an instance name starts like this)
LEGS = (1, 2)


# A case.  C channels in groups of cg; K / stride / pad of the grouped conv (cout = C unless given); formats: in_fl / in_signed (the net input's and
# the conv's), w_fl, relu; readers [(fraclen, signed)] — the shift of a reader is in_fl + w_fl - fraclen.  x_hi: the input is uniform in [0, x_hi]
# ([-x_hi, x_hi] signed).  w_sig is given FOR cg = 1 and scaled by 1 / sqrt(cg), so that a sum over 9 cg taps keeps the spread the formats were chosen
# for; bias_big: biases next to 2^31 on two channels; only_group: the input is zero outside that group.  on_kernel: the shape is in the new
# kernel's set (leg 1 then plans `gconv3x3s{S}:`, else the dense expansion on both legs).
def _case(H, W, stride=1, C=32, cg=4, N=3, pad=1, K=3, **kw):
    d = dict(H=H, W=W, stride=stride, C=C, cout=C, cg=cg, N=N, pad=pad, K=K, in_fl=8, in_signed=False, w_fl=5, relu=True, readers=[(4, False)],
             join_i32=False, x_hi=None, w_sig=40.0, b_sig=2.0 ** 9, b_mean=2.0 ** 13, bias_big=False, only_group=None, opts={}, aim=None, on_kernel=True)
    d.update(kw)
    if d['x_hi'] is None:
        d['x_hi'] = 127 if d['in_signed'] else 255
    return d


def out_hw(case, hw=None, stride=None):
    H, W = hw or (case['H'], case['W'])
    s = stride or case['stride']
    return (H + 2 * case['pad'] - case['K']) // s + 1, (W + 2 * case['pad'] - case['K']) // s + 1


def weights(case, seed=30):
    c = case
    return _w(seed, (c['cout'], c['cg'], c['K'], c['K']), c['w_sig'] * 3.0 / c['K'] / c['cg'] ** 0.5)


def biases(case, seed=40):
    c = case
    bd = _b(seed, c['cout'], c['b_sig'], c['b_mean'])
    if c['bias_big']:                                            # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
        bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
    return bd


def build_graph(case, x, leg=1):
    """Returns (graph, output tensor, [grouped conv tensor ids])."""
    c = case
    g = RefGraph(x, c['in_fl'], grouped=leg)
    t = next(iter(g.v))
    C, G = c['C'], c['C'] // c['cg']
    d = g.conv(t, weights(c), biases(c), stride=c['stride'], pad=c['pad'], groups=G, weight_fl=c['w_fl'], input_fl=c['in_fl'],
               input_signed=c['in_signed'], relu=c['relu'], quant_input=False)
    ids = [d]
    t = d
    if c.get('second'):                                          # -> 1x1 (ReLU) -> a second grouped conv, stride 2
        s = c['second']
        m = g.conv(t, _w(50, (C, C, 1, 1), s['m_sig']), _b(51, C, s['m_bsig'], s['m_bmean']), pad=0, groups=1, weight_fl=6, input_fl=s['m_in_fl'],
                   input_signed=False, relu=True, label='mid')
        t = g.conv(m, weights(c, 31), biases(c, 41), stride=s['stride'], pad=c['pad'], groups=G, weight_fl=s['w_fl'], input_fl=s['in_fl'],
                   input_signed=False, relu=True, label='g2_in')
        ids.append(t)
    out = t
    if c['readers']:
        out = None
        for k, (fl, sgn) in enumerate(c['readers']):
            r = g.conv(t, _w(90 + k, (32, c['cout'], 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, relu=False,
                       label=f'reader{k}')
            out = r if out is None else g.add(out, r)
        if c['join_i32']:
            out = g.add(out, t)
    g.net.output(out, as_float=False)
    return g, out, ids


def make_input(name, case, n=None):
    c = case
    x = synth.rand_uniform_int(5, f'gconvx{name}', (n or c['N'], c['C'], c['H'], c['W']), -c['x_hi'] if c['in_signed'] else 0, c['x_hi']).astype(np.int32)
    if c['only_group'] is not None:
        keep = np.zeros(c['C'], bool)
        keep[c['only_group'] * c['cg']:(c['only_group'] + 1) * c['cg']] = True
        x[:, ~keep] = 0
    return x


def plan(name, case, x, leg=1, max_batch=None):
    g, out, ids = build_graph(case, x, leg)
    for k, v in case['opts'].items():
        g.net.set_option(k, v)
    g.net.finalize(max_batch or case.get('max_batch') or x.shape[0])
    return g, out, ids


def _strides(case):
    return [case['stride']] + ([case['second']['stride']] if case.get('second') else [])


def g_lines(net):
    """[(launch index, plan token 'gconv3x3s1:', kernel name)] of the handle's grouped launches, in launch order."""
    return [(i, net.launch_info(i, 1)[0].split(':')[0] + ':', net.launch_kernel(i)) for i in range(net.num_launches)
            if net.launch_info(i, 1)[0].startswith('gconv')]


def expect(case, leg=1):
    """[(plan token, kernel symbol or its prefix)] of the case's grouped convs on a leg."""
    K = case['K']
    if leg == 1 and case['on_kernel']:
        return [(f'gconv3x3s{s}:', kernel(s)) for s in _strides(case)]
    return [(f'gconv{K}x{K}s{s}_dense:', DENSE_KERNEL) for s in _strides(case)]


def lines_match(lines, want):
    return len(lines) == len(want) and all(tok == wt and (kern == wk or (wk.endswith('<') and kern.startswith(wk))) for (_, tok, kern), (wt, wk) in zip(lines, want))


# ---- geometry at C = 32, cg = 4, pad 1, three images (sub-batches of 2 and 1): default formats (in 8 unsigned, w 5, ReLU, one unsigned reader at
#      fraclen 4: shift 9)
GEOMETRY = {}
for _S in (1, 2):
    GEOMETRY[f's{_S}_1x1'] = _case(1, 1, _S, w_sig=120.0)          # every tap but the centre is padding; eight images per workgroup, three live
    GEOMETRY[f's{_S}_3x3'] = _case(3, 3, _S)
    GEOMETRY[f's{_S}_9x11'] = _case(9, 11, _S)                     # odd both ways; stride 2: the last window hangs over the edge
    GEOMETRY[f's{_S}_8x10'] = _case(8, 10, _S)                     # even; stride 2: the last row and column are never a window centre
    GEOMETRY[f's{_S}_pad0_9x9'] = _case(9, 9, _S, pad=0)
GEOMETRY['s1_5x35'] = _case(5, 35)                                 # wider than one 32-pixel group, odd width
GEOMETRY['s2_5x69'] = _case(5, 69, 2)                              # -> 3 x 35: 35 output columns, more than a stride-2 tile's 32: two column tiles of 18
GEOMETRY['s1_3x70'] = _case(3, 70)                                 # 70 output columns, more than a tile's 64: two column tiles of 35
GEOMETRY['s1_41x33'] = _case(41, 33, N=2)                          # 35-pixel patch rows: 10 fit, 8 output rows at most -> 6 row tiles of 7, the last with 6 live
GEOMETRY['s2_37x63'] = _case(37, 63, 2, N=2)                       # -> 19 x 32: 65-pixel patch rows: 5 fit, 2 output rows per tile -> 10 tiles, the last with 1 live

# ---- channels and groups, 9 x 11 map (c_256: 7 x 7)
CHANNELS = {
    'c_64_cg32': _case(9, 11, C=64, cg=32),                        # G = 2: one group per slice
    'c_64_cg2': _case(9, 11, C=64, cg=2),
    'c_48_cg16': _case(9, 11, C=48, cg=16),                        # Cs 64: a half-live padded slice
    'c_160_cg8': _case(9, 11, 2, C=160, cg=8),                     # five slices: one more than a four-slice workgroup
    'c_256_cg16_7x7_n5': _case(7, 7, C=256, cg=16, N=5),           # four images per workgroup: a full workgroup and one with a single live image
    'c_40_cg8': _case(9, 11, C=40, cg=8),
}

# ---- outside the new kernel's set: the dense expansion on both legs
DENSE = {
    'd_cg24': _case(9, 11, C=48, cg=24, on_kernel=False),
    'd_cin_ne_cout': _case(9, 11, C=32, cg=4, cout=64, on_kernel=False),
    'd_k1': _case(9, 11, C=32, cg=8, K=1, pad=0, w_sig=120.0, on_kernel=False),
    'd_k5_s2': _case(9, 11, 2, C=32, cg=4, K=5, pad=2, on_kernel=False),
    'd_s3': _case(9, 11, 3, C=32, cg=4, on_kernel=False),
}

# ---- cross-talk: a signed input that is zero outside group 5; int32 out.  Every output channel outside the group is its bias path.
XTALK = {'x_s1': _case(9, 11, in_fl=7, in_signed=True, relu=False, readers=None, only_group=5, b_mean=0.0, b_sig=2.0 ** 11),
         'x_s2_c160': _case(9, 11, 2, C=160, cg=8, in_fl=7, in_signed=True, relu=False, readers=None, only_group=13, b_mean=0.0, b_sig=2.0 ** 11)}

# ---- formats, each at stride 1 and 2 on a 9 x 11 map
_SGN = dict(b_mean=0.0, b_sig=2.0 ** 11)
# shift 1: small inputs and weights; shift 17: the biases carry the values (weights of 8 bits cannot)
_S1 = dict(w_fl=0, readers=[(7, False)], x_hi=15, w_sig=1.5, b_sig=60.0, b_mean=150.0)
_S17 = dict(w_fl=9, readers=[(0, False)], w_sig=60.0, b_sig=2.0 ** 22, b_mean=2.0 ** 23)
FORMATS = {}


def _add(prefix, **kw):
    for s in (1, 2):
        FORMATS[f'{prefix}_s{s}'] = _case(9, 11, s, **kw)


# signed input: the pad value is a real 0, not the biased zero
_add('f_signed_in_signed_reader', in_fl=7, in_signed=True, relu=False, readers=[(4, True)], **_SGN)
_add('f_signed_in_unsigned_reader', in_fl=7, in_signed=True, readers=[(3, False)], b_mean=2.0 ** 12)
_add('f_no_relu', relu=False, readers=[(3, True)], b_mean=-2.0 ** 13, b_sig=2.0 ** 12)             # unsigned input: a bias below 0 centres the values
_add('f_two_unsigned', readers=[(4, False), (3, False)])                                          # shifts 9 and 10 in one launch
_add('f_mixed_forms', readers=[(4, False), (3, True)])
_add('f_shift1', **_S1)
_add('f_shift17', **_S17)
_add('f_bias_big', bias_big=True, aim='bias_big')
_add('f_i32', readers=None)                                                                       # int32 only
_add('f_i32_and_i8', join_i32=True)                                                               # one launch writes both
_add('f_rq1', opts={'requant_float': 1})                                                          # same kernel symbol, same values as s{S}_9x11

CASES = dict(GEOMETRY, **CHANNELS, **DENSE, **XTALK, **FORMATS)

# planned for 8 images, run with 3 (parts of 2 and 1) and then 8 from the same handle
MAX_BATCH_CASE = _case(9, 11, 2, N=8, max_batch=8)

# grouped 3x3 / 1 -> 1x1 (ReLU) -> grouped 3x3 / 2 on a 14 x 14 map, N = 3, bench.py's schedule
PIPELINED_CASE = _case(14, 14, readers=[(3, False)], opts=dict(_IR_PIPELINED['opts']),
                       second=dict(stride=2, m_in_fl=4, m_sig=8.0, m_bsig=2.0 ** 10, m_bmean=2.0 ** 11, in_fl=5, w_fl=5))
