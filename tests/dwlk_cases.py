"""Case table and graph builder of the op-level tests of the large depthwise launches — square kernels 8 .. 31 under option dw_large (dwlk_kernel<TC> of
f8_dwlk.hip at stride 1 with int8 forms only, dwconvk_kernel<signed> of f8_dwk.hip elsewhere and under dw_large = 2): tests/test_dwlk_plan.py (no GPU)
and tests/test_gpu_dwlk.py.  No test functions here.

The graphs are dwk_cases': input -> depthwise K x K (reads the net input as it is) -> one 32-output 1x1 reader per (fraclen, signed), summed — or the
depthwise int32 result itself (readers=None); `second` chains two depthwise convs through a 1x1.  The handle's dw_large is set before the conv is added.

Expected tokens and symbols are WRITTEN BY HAND from dwk_inst / dwlk_geom: dwlk_kernel<TC>, TC = column tiles of 32 outputs a workgroup owns — 2 only
where the output is wider than 32 AND the tile (channel group x stacked rows + k - 1 x 32 (TC + 1) + 16 columns, plus the output tile) fits the LDS; dwlk_rule
keeps output maps of 8 and fewer rows or columns on the generic kernel."""
from dwk_cases import _case as _dwk_case
from dwk_cases import _dw_weight, dw_lines, generic, make_input, out_hw  # noqa: F401  (the tests read them from here)
from ir_cases import PIPELINED_CASE as _IR_PIPELINED
from ir_cases import _b, _w
from refgraph import RefGraph

LEGS = {'own': 1, 'generic': 2}                          # option dw_large


def dwlk(tc):
    return f'f8::dwlk_kernel<{tc}>'


# dwk_cases' case with biases that keep the ReLU'd values off the floor (mean 2^15 at shift 9: 64 of 255); kernel: the symbol on the 'own' leg
def _case(K, H, W, pad, kernel=None, stride=1, **kw):
    kw = dict(dict(b_mean=2.0 ** 15, b_sig=2.0 ** 11), **kw)
    return _dwk_case(K, stride, H, W, kernel or dwlk(1), pad=pad, **kw)


def build_graph(case, x, dw_large=1):
    """Returns (graph, output tensor, [depthwise tensor ids])."""
    c = case
    g = RefGraph(x, c['in_fl'])
    g.net.set_option('dw_large', dw_large)
    t = next(iter(g.v))
    C = c['C']
    bd = _b(40, C, c['b_sig'], c['b_mean'])
    if c['bias_big']:
        bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
    t = g.conv(t, _dw_weight(30, C, c['K'], c['w_sig']), bd, stride=c['stride'], pad=c['pad'], groups=C, weight_fl=c['w_fl'], input_fl=c['in_fl'],
               input_signed=c['in_signed'], relu=c['relu'], quant_input=False)
    ids = [t]
    if c.get('second'):                                          # -> 1x1 (ReLU) -> a second large depthwise conv
        s = c['second']
        m = g.conv(t, _w(50, (C, C, 1, 1), 8.0), _b(51, C, 2.0 ** 10, 2.0 ** 11), pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=True, label='mid')
        t = g.conv(m, _dw_weight(31, C, s['K'], c['w_sig']), _b(41, C, c['b_sig'], c['b_mean']), pad=s['K'] // 2, groups=C, weight_fl=5, input_fl=5,
                   input_signed=False, relu=True, label='dw2_in')
        ids.append(t)
    out = t
    for k, (fl, sgn) in enumerate(c['readers'] or []):
        r = g.conv(t, _w(90 + k, (32, C, 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, relu=False, label=f'reader{k}')
        out = r if k == 0 else g.add(out, r)
    g.net.output(out, as_float=False)
    return g, out, ids


def plan(case, x, leg='own', max_batch=None):
    g, out, ids = build_graph(case, x, LEGS[leg])
    for k, v in case['opts'].items():
        g.net.set_option(k, v)
    g.net.finalize(max_batch or case.get('max_batch') or x.shape[0])
    return g, out, ids


def expect(case, leg='own'):
    ks = [case['K']] + ([case['second']['K']] if case.get('second') else [])
    own = case['kernel'] if isinstance(case['kernel'], list) else [case['kernel']]
    sgn = [case['in_signed'], False]
    return [(f'dwconv{k}x{k}s{case["stride"]}:', own[i] if leg == 'own' else generic(sgn[i])) for i, k in enumerate(ks)]


_SGN = dict(b_mean=0.0, b_sig=2.0 ** 11)
CASES = {
    # ---- geometry, N = 3: the band inside one K chunk (9), across the chunk boundary (13 .. 17), the widest (31), an even kernel (8, 16)
    'k8_14x14_p4': _case(8, 14, 14, 4),                                   # -> 15 x 15: 2 images stacked, the last group has one
    'k9_14x14_p0': _case(9, 14, 14, 0, generic(False)),                   # -> 6 x 6: dwlk_rule keeps output maps of 8 and fewer rows or columns off dwlk_kernel
    'k9_12x33_p4_c40': _case(9, 12, 33, 4, C=40),                         # one column past a column tile; channels padded to 64
    'k13_33x12_p6': _case(13, 33, 12, 6),                                 # one row past a row tile
    'k13_7x7_p6_c40': _case(13, 7, 7, 6, generic(False), C=40),           # the kernel is larger than the map (RepLKNet's last stage): the rule again
    'k13_9x9_p6': _case(13, 9, 9, 6),                                     # ... and the smallest map past the rule
    'k16_26x24_p1': _case(16, 26, 24, 1),                                 # -> 13 x 11
    'k17_14x14_p8_c96': _case(17, 14, 14, 8, C=96),                       # three channel groups of 32
    'k31_40x40_p15': _case(31, 40, 40, 15, dwlk(2)),                      # two row tiles x one workgroup of two column tiles, 16 channels each
    'k31_40x40_p1': _case(31, 40, 40, 1),                                 # -> 12 x 12
    # ---- formats at k13 / pad 6 on 14 x 14
    'f_signed_in_no_relu': _case(13, 14, 14, 6, in_fl=7, in_signed=True, relu=False, readers=[(4, True)], **_SGN),      # the pad value is a real 0
    'f_no_relu_signed_reader': _case(13, 14, 14, 6, relu=False, readers=[(3, True)], **_SGN),
    'f_two_readers': _case(13, 14, 14, 6, readers=[(4, False), (3, True)]),                                              # two forms, one launch
    'f_two_readers_wide': _case(31, 40, 40, 15, readers=[(4, False), (3, False)]),                                       # ... whose output tiles leave room for one column tile
    'f_i32': _case(13, 14, 14, 6, generic(False), readers=None),                                                         # int32: the generic kernel on both legs
    'f_bias_big': _case(13, 14, 14, 6, bias_big=True),
    'f_stride2': _case(13, 14, 14, 6, generic(False), stride=2),
    'f_stride2_k8': _case(8, 15, 15, 0, generic(False), stride=2),
}

# planned for 8 images, run with 3 and then 8 from the same handle
MAX_BATCH_CASE = _case(9, 14, 14, 4, N=8, max_batch=8)

# depthwise 13x13 -> 1x1 (ReLU) -> depthwise 9x9 on a 14 x 14 map, N = 3, bench.py's schedule
PIPELINED_CASE = _case(13, 14, 14, 6, [dwlk(1), dwlk(1)], readers=[(1, False)], opts=dict(_IR_PIPELINED['opts']), second=dict(K=9))

ALL = dict(CASES, max_batch=MAX_BATCH_CASE, pipelined=PIPELINED_CASE)
