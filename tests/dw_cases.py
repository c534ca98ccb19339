"""Case table and graph builder of the op-level tests of the standalone depthwise 3x3 launches (dwconv_inst -> launch_dwconv: dwconv3x3_mma_kernel
of f8_dwmma.hip, dwconv3x3_dot4_kernel and dwconv3x3_kernel of f8_kernels.hip): tests/test_dw_plan.py (plan, symbols and liveness on the oracle, no
GPU) and tests/test_gpu_dw.py (all three kernels against the oracle on the device).  No test functions here.

Every graph is  input -> depthwise 3x3, pad 1 (the conv under test; it reads the net input as it is, quant_input = False) -> output, where the
output is the depthwise int32 result itself (readers=None) or the sum of one 32-output 1x1 reader per (fraclen, signed) — plus the int32 result
when `join_i32` is set (the launch then writes int32 next to its int8 forms).  The pipelined case chains two of them through a 1x1.

The expected plan token and kernel instance of every case are WRITTEN BY HAND from dwconv_inst (f8_kernels.hip) and dwconv_mma_inst
(f8_dwmma.hip); nothing here asks the planner for them:
  mma<S, FQ, SUBS>  int8 outputs only, stride 1, or stride 2 on an even map; output width >= 28 (SUBS 1: strips of 28 columns) or == 14 (SUBS 2:
                    two rows of 14 per pixel tile).  FQ 0: the general epilogue (no ReLU, or a reader that is not an unsigned right shift of 1 .. 30);
                    else 1 with requant_float = 1, bounded accumulators and every shift <= 16 (kRequantU8MaxShift); else 2.
  dot4<S, 2>        every other int8-only launch (and every such launch with dw_mma = 0)
  generic<signed>   an int32 output (and every launch with dw_mma = 0, dw_dot4 = 0)"""
import numpy as np

from f8net_amd import synth
from ir_cases import PIPELINED_CASE as _IR_PIPELINED
from ir_cases import _b, _w
from refgraph import RefGraph

DW_SW = 28                                              # f8_dwmma.hip: output columns per strip, rows per band (8 below 4096 wave items)
DW_BAND = 14


def mma(s, fq, subs):
    return f'f8::dwconv3x3_mma_kernel<{s}, {fq}, {subs}>'


def dot4(s):
    return f'f8::dwconv3x3_dot4_kernel<{s}, 2>'


def generic(signed):
    return f'f8::dwconv3x3_kernel<{"true" if signed else "false"}>'


# A case.  Formats: in_fl / in_signed (the net input's and the depthwise conv's), w_fl, relu; readers [(fraclen, signed)] — the shift of a reader is
# in_fl + w_fl - fraclen.  x_hi: the input is uniform in [0, x_hi] ([-x_hi, x_hi] signed).  w_sig / b_sig / b_mean: spreads of the depthwise weights and
# biases; bias_big: biases next to 2^31 on two channels.  kernel: the expected instance with the case's own options; the legs of test_gpu_dw.py with
# dw_mma = 0 / dw_mma = 0, dw_dot4 = 0 run dot4<stride, 2> / generic<in_signed> whatever the shape.
def _case(H, W, kernel, C=32, N=3, stride=1, **kw):
    d = dict(H=H, W=W, C=C, N=N, stride=stride, in_fl=8, in_signed=False, w_fl=5, relu=True, readers=[(4, False)], join_i32=False, x_hi=None,
             w_sig=40.0, b_sig=2.0 ** 9, b_mean=2.0 ** 13, bias_big=False, opts={}, kernel=kernel, aim=None)
    d.update(kw)
    if d['x_hi'] is None:
        d['x_hi'] = 127 if d['in_signed'] else 255
    return d


def out_hw(case):
    return (case['H'] - 1) // case['stride'] + 1, (case['W'] - 1) // case['stride'] + 1


def build_graph(case, x):
    """Returns (graph, output tensor, [depthwise tensor ids])."""
    c = case
    g = RefGraph(x, c['in_fl'])
    t = next(iter(g.v))
    C = c['C']
    bd = _b(40, C, c['b_sig'], c['b_mean'])
    if c['bias_big']:                                            # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
        bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
    d = g.conv(t, _w(30, (C, 1, 3, 3), c['w_sig']), bd, stride=c['stride'], pad=1, groups=C, weight_fl=c['w_fl'], input_fl=c['in_fl'],
               input_signed=c['in_signed'], relu=c['relu'], quant_input=False)
    ids = [d]
    t = d
    if c.get('second'):                                          # -> 1x1 (ReLU) -> a second depthwise conv
        s = c['second']
        m = g.conv(t, _w(50, (C, C, 1, 1), s['m_sig']), _b(51, C, s['m_bsig'], s['m_bmean']), pad=0, groups=1, weight_fl=6, input_fl=s['m_in_fl'],
                   input_signed=False, relu=True, label='mid')
        t = g.conv(m, _w(31, (C, 1, 3, 3), c['w_sig']), _b(41, C, c['b_sig'], c['b_mean']), stride=s['stride'], pad=1, groups=C, weight_fl=s['w_fl'],
                   input_fl=s['in_fl'], input_signed=False, relu=True, label='dw2_in')
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
    return synth.rand_uniform_int(5, f'dwx{name}', (n or c['N'], c['C'], c['H'], c['W']), -c['x_hi'] if c['in_signed'] else 0, c['x_hi']).astype(np.int32)


LEGS = {'own': {}, 'dot4': {'dw_mma': 0}, 'generic': {'dw_mma': 0, 'dw_dot4': 0}}


def leg_kernels(case, leg):
    """The expected kernel of each depthwise conv of the case on a leg of LEGS."""
    strides = [case['stride']] + ([case['second']['stride']] if case.get('second') else [])
    own = case['kernel'] if isinstance(case['kernel'], list) else [case['kernel']]
    if leg == 'own':
        return own
    if leg == 'dot4':                                            # an int32 output keeps the generic kernel
        return [k if k.startswith('f8::dwconv3x3_kernel') else dot4(s) for k, s in zip(own, strides)]
    return [generic(case['in_signed'])] + [generic(False)] * (len(strides) - 1)


def plan(name, case, x, leg='own', max_batch=None):
    g, out, ids = build_graph(case, x)
    for k, v in dict(case['opts'], **LEGS[leg]).items():
        g.net.set_option(k, v)
    g.net.finalize(max_batch or case.get('max_batch') or x.shape[0])
    return g, out, ids


def dw_lines(net):
    """[(launch index, plan token 'dwconv3x3s1:', kernel name)] of the handle's depthwise launches, in launch order."""
    return [(i, net.launch_info(i, 1)[0].split(':')[0] + ':', net.launch_kernel(i)) for i in range(net.num_launches)
            if net.launch_info(i, 1)[0].startswith('dwconv3x3s')]


def expect(case, leg='own'):
    strides = [case['stride']] + ([case['second']['stride']] if case.get('second') else [])
    return [(f'dwconv3x3s{s}:', k) for s, k in zip(strides, leg_kernels(case, leg))]


def mma_tiling(case, n_launch):
    """(strip width, band height) of the case's MMA launch over n_launch images: launch_dwconv_mma's arithmetic."""
    P, Q = out_hw(case)
    vw = DW_SW if Q >= DW_SW else 14
    cts = (case['C'] + 31) // 32
    items = lambda band: n_launch * ((P + band - 1) // band) * ((Q + vw - 1) // vw) * cts
    band = DW_BAND
    if items(band) < 4096 and P > 8:
        band = 8
    return vw, band, items(band)


# ---- geometry, three images (sub-batches of 2 and 1): default formats (in 8 unsigned, w 5, ReLU, one unsigned reader at fraclen 4: shift 9 -> FQ 2)
GEOMETRY = {
    # strips of 28 output columns; lanes 28 .. 31 of a strip hold the first columns of the next one for the lane shifts
    's_12x28': _case(12, 28, mma(1, 2, 1)),                        # one exact strip; bands 8 + 4
    's_12x29': _case(12, 29, mma(1, 2, 1)),                        # a second strip of one column
    's_9x57': _case(9, 57, mma(1, 2, 1)),                          # three strips, the last of one column
    's_10x112': _case(10, 112, mma(1, 2, 1)),                      # four strips; bands 8 + 2
    # bands: a test-sized launch has < 4096 items -> band 8 when P > 8, else one band of 14
    'b_8x28': _case(8, 28, mma(1, 2, 1)),                          # band 14 holding 8 rows
    'b_9x28': _case(9, 28, mma(1, 2, 1)),                          # 8 + 1
    'b_16x28': _case(16, 28, mma(1, 2, 1)),                        # two exact bands
    'b_17x30': _case(17, 30, mma(1, 2, 1)),                        # 8 + 8 + 1 rows, strips of 28 + 2
    # two sub-rows of 14 columns per pixel tile
    'u_14x14': _case(14, 14, mma(1, 2, 2)),                        # bands 8 + 6
    'u_9x14': _case(9, 14, mma(1, 2, 2)),                          # 8 + 1: the last step's second sub-row is past the band
    'u_1x14': _case(1, 14, mma(1, 2, 2)),                          # one row: sub-row 1 never lives
    'u_15x14': _case(15, 14, mma(1, 2, 2)),                        # 8 + 7
    # stride 2 on the matrix cores (even maps only: H == 2 P, W == 2 Q)
    't_30x58': _case(30, 58, mma(2, 2, 1), stride=2),              # -> 15 x 29: strips 28 + 1, bands 8 + 7; input column 57 is colB's last
    't_56x56': _case(56, 56, mma(2, 2, 1), stride=2),              # -> 28 x 28
    't_28x28': _case(28, 28, mma(2, 2, 2), stride=2),              # -> 14 x 14
    't_18x28': _case(18, 28, mma(2, 2, 2), stride=2),              # -> 9 x 14: odd P with sub-rows
    't_2x56': _case(2, 56, mma(2, 2, 1), stride=2),                # -> 1 x 28
    # channels
    'c_24': _case(9, 28, mma(1, 2, 1), C=24),                      # padded to 32
    'c_96_n1': _case(8, 28, mma(1, 2, 1), C=96, N=1),              # 3 items in a 4-wave workgroup: the fourth wave returns
    'c_160_14x14': _case(14, 14, mma(1, 2, 2), C=160),             # 2 bands x 5 channel tiles = 10 items per image: 2.5 workgroups
    # the v_dot4 kernel: maps the MMA kernel has no instance for (output width < 28 and != 14, odd maps at stride 2)
    'd_7x7': _case(7, 7, dot4(1)),                                 # odd Q: pixel pairs 3 + a half
    'd_7x7_c48_n5': _case(7, 7, dot4(1), C=48, N=5),               # Cs 64: four 16-channel groups, one of them padding
    'd_5x9': _case(5, 9, dot4(1)),
    'd_29x29_s2': _case(29, 29, dot4(2), stride=2),                # -> 15 x 15; input row / column 29 is outside
    'd_7x13_s2': _case(7, 13, dot4(2), stride=2),                  # -> 4 x 7
    # the generic kernel with stride 2 on an odd map
    'g_9x11_s2': _case(9, 11, generic(False), stride=2, readers=None),
}

# ---- MMA band 14 for real: one launch of 32 images x 2 bands (14 + 1) x 2 strips (28 + 1) x 32 channel tiles = 4096 items; split = 1 keeps the
#      batch in one launch (the default 2 halves it: 2048 items, band 8)
BAND14_CASE = _case(15, 29, mma(1, 2, 1), C=1024, N=32, opts={'split': 1})

# ---- formats, each on a 28-wide map (9 x 29: SUBS 1, ragged strip and band) and a 14-wide one (9 x 14: SUBS 2, odd row count)
_M28 = ('29', dict(H=9, W=29), 1)
_M14 = ('14', dict(H=9, W=14), 2)
# shift 8 for the signed / no-ReLU forms: biases around 0
_SGN = dict(b_mean=0.0, b_sig=2.0 ** 11)
# shift 1: small inputs and weights; shifts 16 / 17: the biases carry the values (weights of 8 bits cannot)
_S1 = dict(w_fl=0, readers=[(7, False)], x_hi=15, w_sig=1.5, b_sig=60.0, b_mean=150.0)
_S16 = dict(w_fl=8, readers=[(0, False)], w_sig=60.0, b_sig=2.0 ** 21, b_mean=2.0 ** 22)
_S17 = dict(_S16, w_fl=9, b_sig=2.0 ** 22, b_mean=2.0 ** 23)
FORMATS = {}


def _add(prefix, fq, maps=(_M28, _M14), stride=1, **kw):
    for suf, geo, subs in maps:
        H, W = geo['H'] * stride, geo['W'] * stride
        FORMATS[f'{prefix}_{suf}'] = _case(H, W, mma(stride, fq, subs), stride=stride, **kw)


_add('f_rq1', 1, opts={'requant_float': 1})                                                    # the float-converter form
# signed input: the pad value is a real 0, not the biased zero
_add('f_signed_in_signed_reader', 0, in_fl=7, in_signed=True, relu=False, readers=[(4, True)], **_SGN)
_add('f_signed_in_unsigned_reader', 2, in_fl=7, in_signed=True, readers=[(3, False)], b_mean=2.0 ** 12)
_add('f_no_relu', 0, relu=False, readers=[(3, True)], b_mean=-2.0 ** 13, b_sig=2.0 ** 12)       # unsigned input: a bias below 0 centres the values
_add('f_relu_signed_reader', 0, readers=[(3, True)])                                           # shift 10 into [0, 127] behind the ReLU floor
_add('f_two_unsigned', 2, readers=[(4, False), (3, False)])                                    # shifts 9 and 10 in one launch
_add('f_mixed_forms', 0, readers=[(4, False), (3, True)])
_add('f_shift1', 2, **_S1)
_add('f_shift16_rq1', 1, opts={'requant_float': 1}, **_S16)
_add('f_shift17_rq1', 2, opts={'requant_float': 1}, **_S17)                                    # beyond kRequantU8MaxShift: the integer form
_add('f_shift16_rq0', 2, opts={'requant_float': 0}, **_S16)
_add('f_shift16_17_rq1', 2, opts={'requant_float': 1}, **dict(_S16, w_fl=9, readers=[(1, False), (0, False)]))   # one form beyond it takes both
for _rq in (0, 1):                                          # the accumulator is not bounded: the integer instance with either requant_float
    _add(f'f_bias_big_rq{_rq}', 2, opts={'requant_float': _rq}, bias_big=True, aim='bias_big')
# stride 2: the float-converter and the general epilogue, both SUBS forms (FQ 2: the geometry cases)
_add('f_s2_rq1', 1, stride=2, opts={'requant_float': 1})
_add('f_s2_signed', 0, stride=2, in_fl=7, in_signed=True, relu=False, readers=[(4, True)], **_SGN)
# the v_dot4 kernel's formats on its own shapes
FORMATS['f_dot4_signed_in'] = _case(7, 7, dot4(1), in_fl=7, in_signed=True, readers=[(3, False)], b_mean=2.0 ** 12)
FORMATS['f_dot4_no_relu_signed_reader'] = _case(5, 9, dot4(1), relu=False, readers=[(3, True)], b_mean=-2.0 ** 13, b_sig=2.0 ** 12)
FORMATS['f_dot4_two_forms'] = _case(7, 13, dot4(2), stride=2, readers=[(4, False), (3, True)])
FORMATS['f_dot4_mma_off_28x28'] = _case(28, 28, dot4(1), opts={'dw_mma': 0})                  # the map of f_mma_28x28: the two must agree (same oracle value)
FORMATS['f_mma_28x28'] = _case(28, 28, mma(1, 2, 1))
# the generic kernel: an int32 output (signed and unsigned input), int32 next to an int8 form, both other kernels off with two forms
FORMATS['f_gen_i32'] = _case(9, 14, generic(False), readers=None)
FORMATS['f_gen_i32_signed_in'] = _case(9, 29, generic(True), in_fl=7, in_signed=True, relu=False, readers=None, **_SGN)
FORMATS['f_gen_i32_and_i8'] = _case(9, 14, generic(False), join_i32=True)                      # one launch writes both (test_dw_plan.py asserts it)
FORMATS['f_gen_forced_two_forms'] = _case(14, 14, generic(False), readers=[(4, False), (3, True)], opts={'dw_mma': 0, 'dw_dot4': 0})

CASES = dict(GEOMETRY, **FORMATS)

# planned for 8 images, run with 3 (parts of 2 and 1) and then 8 from the same handle; 17 x 30: ragged band and strip
MAX_BATCH_CASE = _case(17, 30, mma(1, 2, 1), N=8, max_batch=8)

# depthwise 3x3 / 1 -> 1x1 (ReLU) -> depthwise 3x3 / 2 on a 28 x 28 map, N = 3, bench.py's schedule.  fuse_ir = 0: 1x1 (ReLU) -> depthwise -> 1x1 is
# an inverted residual, which the default plan may fuse into one launch
PIPELINED_CASE = _case(28, 28, [mma(1, 2, 1), mma(2, 2, 2)], readers=[(3, False)], opts=dict(_IR_PIPELINED['opts'], fuse_ir=0),
                       second=dict(stride=2, m_in_fl=4, m_sig=8.0, m_bsig=2.0 ** 10, m_bmean=2.0 ** 11, in_fl=5, w_fl=5))
