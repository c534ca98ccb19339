"""Case table and graph builder of the op-level tests of the general depthwise launches — every accepted depthwise conv that is not 3x3 / pad 1:
kernel 3 / 5 / 7, stride 1 / 2, pad 0 .. kernel / 2 (dwconvk_dot4_kernel<K, S> and dwconvk_kernel<signed> of f8_dwk.hip): tests/test_dwk_plan.py
(acceptance, plan, symbols and liveness on the oracle, no GPU) and tests/test_gpu_dwk.py (both kernels against the oracle on the device).  No test
functions here.

Every graph is  input -> depthwise K x K (the conv under test; it reads the net input as it is, quant_input = False) -> output, where the output
is the depthwise int32 result itself (readers=None) or the sum of one 32-output 1x1 reader per (fraclen, signed) — plus the int32 result when
`join_i32` is set (the launch then writes int32 next to its int8 forms).  The pipelined case chains two of them through a 1x1.

The expected plan token and kernel symbol of every case are WRITTEN BY HAND from dwk_inst (f8_dwk.hip); nothing here asks the planner for them:
  dot4<K, S>        every int8-only launch with the default options
  generic<signed>   an int32 output, and every launch with dwk_dot4 = 0
dwconvk_dot4_kernel gives a thread PIX = 4 adjacent output pixels of a row and 4 channels."""
import numpy as np

from f8net_amd import synth
from ir_cases import PIPELINED_CASE as _IR_PIPELINED
from ir_cases import _b, _w
from refgraph import RefGraph

PIX = 4                                                 # f8_dwk.hip DWK_PIX: output pixels per thread of the dot4 kernel


def dot4(k, s):
    return f'f8::dwconvk_dot4_kernel<{k}, {s}>'


def generic(signed):
    return f'f8::dwconvk_kernel<{"true" if signed else "false"}>'


# A case.  K / stride / pad (None: K // 2) of the depthwise conv; formats: in_fl / in_signed (the net input's and the depthwise conv's), w_fl, relu;
# readers [(fraclen, signed)] — the shift of a reader is in_fl + w_fl - fraclen.  x_hi: the input is uniform in [0, x_hi] ([-x_hi, x_hi] signed).
# w_sig / b_sig / b_mean: spreads of the depthwise weights and biases — w_sig is given FOR A 3 x 3 and scaled by 3 / K, so that a sum over K * K taps
# keeps the spread the formats were chosen for; bias_big: biases next to 2^31 on two channels.  kernel: the expected symbol with the case's own
# options; the leg with dwk_dot4 = 0 runs generic<in_signed> whatever the shape.
def _case(K, stride, H, W, kernel=None, C=32, N=3, pad=None, **kw):
    d = dict(K=K, stride=stride, pad=K // 2 if pad is None else pad, H=H, W=W, C=C, N=N, in_fl=8, in_signed=False, w_fl=5, relu=True,
             readers=[(4, False)], join_i32=False, x_hi=None, w_sig=40.0, b_sig=2.0 ** 9, b_mean=2.0 ** 13, bias_big=False, opts={}, aim=None)
    d.update(kw)
    d['kernel'] = kernel or dot4(K, stride)
    if d['x_hi'] is None:
        d['x_hi'] = 127 if d['in_signed'] else 255
    return d


def out_hw(case, K=None, stride=None, pad=None, hw=None):
    K, s, p = K or case['K'], stride or case['stride'], case['pad'] if pad is None else pad
    H, W = hw or (case['H'], case['W'])
    return (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1


def _dw_weight(seed, C, K, sig):
    return _w(seed, (C, 1, K, K), sig * 3.0 / K)


def build_graph(case, x):
    """Returns (graph, output tensor, [depthwise tensor ids])."""
    c = case
    g = RefGraph(x, c['in_fl'])
    t = next(iter(g.v))
    C, K = c['C'], c['K']
    bd = _b(40, C, c['b_sig'], c['b_mean'])
    if c['bias_big']:                                            # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
        bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
    d = g.conv(t, _dw_weight(30, C, K, c['w_sig']), bd, stride=c['stride'], pad=c['pad'], groups=C, weight_fl=c['w_fl'], input_fl=c['in_fl'],
               input_signed=c['in_signed'], relu=c['relu'], quant_input=False)
    ids = [d]
    t = d
    if c.get('second'):                                          # -> 1x1 (ReLU) -> a second depthwise conv
        s = c['second']
        m = g.conv(t, _w(50, (C, C, 1, 1), s['m_sig']), _b(51, C, s['m_bsig'], s['m_bmean']), pad=0, groups=1, weight_fl=6, input_fl=s['m_in_fl'],
                   input_signed=False, relu=True, label='mid')
        t = g.conv(m, _dw_weight(31, C, s['K'], c['w_sig']), _b(41, C, c['b_sig'], c['b_mean']), stride=s['stride'], pad=s['K'] // 2, groups=C,
                   weight_fl=s['w_fl'], input_fl=s['in_fl'], input_signed=False, relu=True, label='dw2_in')
        ids.append(t)
    out = t
    if c['readers']:
        out = None
        for k, (fl, sgn) in enumerate(c['readers']):
            r = g.conv(t, _w(90 + k, (32, C, 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, relu=False, label=f'reader{k}')
            out = r if out is None else g.add(out, r)
        if c['join_i32']:
            out = g.add(out, t)
    g.net.output(out, as_float=False)
    return g, out, ids


def make_input(name, case, n=None):
    c = case
    return synth.rand_uniform_int(5, f'dwkx{name}', (n or c['N'], c['C'], c['H'], c['W']), -c['x_hi'] if c['in_signed'] else 0, c['x_hi']).astype(np.int32)


LEGS = {'own': {}, 'generic': {'dwk_dot4': 0}}


def _convs(case):
    """[(K, stride, input signed)] of the case's depthwise convs."""
    cs = [(case['K'], case['stride'], case['in_signed'])]
    if case.get('second'):
        cs.append((case['second']['K'], case['second']['stride'], False))
    return cs


def leg_kernels(case, leg):
    """The expected kernel of each depthwise conv of the case on a leg of LEGS."""
    if leg == 'own':
        return case['kernel'] if isinstance(case['kernel'], list) else [case['kernel']]
    return [generic(sgn) for _, _, sgn in _convs(case)]


def plan(name, case, x, leg='own', max_batch=None):
    g, out, ids = build_graph(case, x)
    for k, v in dict(case['opts'], **LEGS[leg]).items():
        g.net.set_option(k, v)
    g.net.finalize(max_batch or case.get('max_batch') or x.shape[0])
    return g, out, ids


def dw_lines(net):
    """[(launch index, plan token 'dwconv5x5s1:', kernel name)] of the handle's depthwise launches, in launch order."""
    return [(i, net.launch_info(i, 1)[0].split(':')[0] + ':', net.launch_kernel(i)) for i in range(net.num_launches)
            if net.launch_info(i, 1)[0].startswith('dwconv')]


def expect(case, leg='own'):
    return [(f'dwconv{k}x{k}s{s}:', kern) for (k, s, _), kern in zip(_convs(case), leg_kernels(case, leg))]


# ---- geometry, pad K // 2, three images (sub-batches of 2 and 1): default formats (in 8 unsigned, w 5, ReLU, one unsigned reader at fraclen 4: shift 9)
GEOMETRY = {}
for _K, _S in ((5, 1), (5, 2), (7, 1), (7, 2)):
    _n = f'k{_K}s{_S}'
    GEOMETRY[f'{_n}_1x1'] = _case(_K, _S, 1, 1, w_sig=120.0)       # every tap but the centre is padding (one tap: larger weights keep the values apart)
    GEOMETRY[f'{_n}_3x3'] = _case(_K, _S, 3, 3, w_sig=60.0)        # smaller than the kernel: no interior pixel
    GEOMETRY[f'{_n}_9x11'] = _case(_K, _S, 9, 11)                  # odd both ways; stride 2: the last window hangs over the edge
    GEOMETRY[f'{_n}_8x10'] = _case(_K, _S, 8, 10)                  # even; stride 2: the last row and column are never a window centre
    # output widths PIX + 1 and 2 PIX - 1: a thread with one live pixel, a thread with one dead pixel
    GEOMETRY[f'{_n}_q5'] = _case(_K, _S, 5, 5 if _S == 1 else 9)
    GEOMETRY[f'{_n}_q7'] = _case(_K, _S, 5, 7 if _S == 1 else 13)

# ---- pad below K // 2 (the kernels take pad at run time)
PADS = {
    'p_k5s1_pad0': _case(5, 1, 9, 9, pad=0), 'p_k5s2_pad0': _case(5, 2, 9, 9, pad=0),
    'p_k5s1_pad1': _case(5, 1, 9, 9, pad=1), 'p_k5s2_pad1': _case(5, 2, 9, 9, pad=1),
    'p_k7s1_pad0_7x7': _case(7, 1, 7, 7, pad=0),                  # -> 1 x 1: every tap in the image
    'p_k7s2_pad2_10x12': _case(7, 2, 10, 12, pad=2),
    # general depthwise with the smallest kernel: the token of the 3x3 / pad 1 path, the kernels of f8_dwk.hip
    'p_k3s1_pad0': _case(3, 1, 9, 11, pad=0), 'p_k3s2_pad0': _case(3, 2, 9, 11, pad=0),
}

# ---- channels
CHANNELS = {
    'c_24': _case(5, 1, 9, 11, C=24),                             # padded to 32
    'c_48_n5': _case(7, 1, 7, 7, C=48, N=5),                      # Cs 64: a 16-channel group that is all padding
    'c_160_7x7': _case(5, 2, 7, 7, C=160),
}

# ---- formats, each at K5 / S1 and K7 / S2 on a 9 x 11 map
# shift 8 for the signed / no-ReLU forms: biases around 0
_SGN = dict(b_mean=0.0, b_sig=2.0 ** 11)
# shift 1: small inputs and weights; shift 17: the biases carry the values (weights of 8 bits cannot)
_S1 = dict(w_fl=0, readers=[(7, False)], x_hi=15, w_sig=1.5, b_sig=60.0, b_mean=150.0)
_S17 = dict(w_fl=9, readers=[(0, False)], w_sig=60.0, b_sig=2.0 ** 22, b_mean=2.0 ** 23)
FORMATS = {}


def _add(prefix, kernel=None, **kw):
    for suf, K, S in (('k5s1', 5, 1), ('k7s2', 7, 2)):
        FORMATS[f'{prefix}_{suf}'] = _case(K, S, 9, 11, kernel(kw.get('in_signed', False)) if kernel else None, **kw)


# signed input: the pad value is a real 0, not the biased zero
_add('f_signed_in_signed_reader', in_fl=7, in_signed=True, relu=False, readers=[(4, True)], **_SGN)
_add('f_signed_in_unsigned_reader', in_fl=7, in_signed=True, readers=[(3, False)], b_mean=2.0 ** 12)
_add('f_no_relu', relu=False, readers=[(3, True)], b_mean=-2.0 ** 13, b_sig=2.0 ** 12)             # unsigned input: a bias below 0 centres the values
_add('f_relu_signed_reader', readers=[(3, True)])                                                 # shift 10 into [0, 127] behind the ReLU floor
_add('f_two_unsigned', readers=[(4, False), (3, False)])                                          # shifts 9 and 10 in one launch
_add('f_mixed_forms', readers=[(4, False), (3, True)])
_add('f_shift1', **_S1)
_add('f_shift17', **_S17)
_add('f_bias_big', bias_big=True, aim='bias_big')
_add('f_i32', generic, readers=None)                                                              # int32 only: the generic kernel on both legs
_add('f_i32_and_i8', generic, join_i32=True)                                                      # one launch writes both
FORMATS['f_rq1_k5s1'] = _case(5, 1, 9, 11, opts={'requant_float': 1})                             # same kernel symbol, same values as k5s1_9x11 (test_gpu_dwk.py compares them)

CASES = dict(GEOMETRY, **PADS, **CHANNELS, **FORMATS)

# planned for 8 images, run with 3 (parts of 2 and 1) and then 8 from the same handle
MAX_BATCH_CASE = _case(5, 2, 9, 11, N=8, max_batch=8)

# depthwise 5x5 / 1 -> 1x1 (ReLU) -> depthwise 7x7 / 2 on a 14 x 14 map, N = 3, bench.py's schedule
PIPELINED_CASE = _case(5, 1, 14, 14, [dot4(5, 1), dot4(7, 2)], readers=[(3, False)], opts=dict(_IR_PIPELINED['opts']),
                       second=dict(K=7, stride=2, m_in_fl=4, m_sig=8.0, m_bsig=2.0 ** 10, m_bmean=2.0 ** 11, in_fl=5, w_fl=5))
