"""Case table and graph builder of the op-level tests of the fused inverted-residual launch around a depthwise 5x5 / 7x7 (f8_irk.hip, option
fuse_irk): tests/test_irk_plan.py (plan, symbols and liveness on the oracle, no GPU) and tests/test_gpu_irk.py (both legs against the oracle on
the device).  No test functions here.

Every graph is  input -> `pre` 1x1 (pass 1e3 refuses a block that reads the net input) -> block(s) -> output, where the output is the last
block's int32 result itself (readers=None) or the sum of one 32-output 1x1 reader per (fraclen, signed) — plus the int32 block result when
`join_i32` is set (the block then writes int32 next to its int8 forms).  Blocks are ir_cases._blk's with a kernel size K; the depthwise weight
spread is given for a 3x3 and scaled by 3 / K (as dwk_cases does), so that a sum over K * K taps keeps the spread the formats were chosen for.

The expected tile token (R# / G#) and kernel instance of every case are WRITTEN BY HAND from irk_config / irk_layout / irk_inst / irk_cap of
f8_irk.hip; nothing here asks the planner for them:
  tile      Ho * Wo <= 128: G = min(8, 128 // (Ho * Wo)) whole images (fewer while the LDS layout exceeds 160 KB) — token G#, or R<Ho> when G is 1;
            else rows: r = 128 // Wo, tiles = ceil(Ho / r), R = ceil(Ho / tiles) — token R#
  instance  fused_irk_kernel<K, cap, FQ>: cap = 96 / 192 / 320 by the padded output channels; FQ = 2 when both inner requantisations are right
            shifts into unsigned 8-bit behind a ReLU (whatever requant_float says), else 0"""
import numpy as np

from f8net_amd import synth
from ir_cases import PIPELINED_CASE as _IR_PIPELINED
from ir_cases import X_FL, _blk, _b, _w
from refgraph import RefGraph

INT32_MIN_CLAMP = -(2 ** 31 - 1)


def _kblk(K, cin, cout, E, stride=1, **kw):
    return dict(_blk(cin, cout, E, stride, **kw), K=K)


def build_graph(case, x):
    """Returns (graph, output tensor, per-block tensor ids [(expand, depthwise, project, block output)])."""
    blocks = case['blocks']
    g = RefGraph(x, X_FL)
    t = next(iter(g.v))
    c0 = blocks[0]['cin']
    bpre = _b(2, c0, 300.0)
    for ch, bias in case.get('pre_big', {}).items():
        bpre[ch] = bias
    t = g.conv(t, _w(1, (c0, c0, 1, 1), 12.0 * (32.0 / c0) ** 0.5), bpre, pad=0, groups=1, weight_fl=blocks[0]['in_fl'] + 2 + case.get('pre_fl', 0),
               input_fl=X_FL, input_signed=True, relu=False)
    ids = []
    for i, b in enumerate(blocks):
        E, cin, cout, K = b['E'], b['cin'], b['cout'], b['K']
        be, bd = _b(10 + i, E, b['e_bsig'], b['e_bmean']), _b(40 + i, E, b['d_bsig'], b['d_bmean'])
        if b['bias_big']:                                        # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
            be[3], be[7] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
            bd[5], bd[11] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
        e = g.conv(t, _w(20 + i, (E, cin, 1, 1), b['e_sig']), be, pad=0, groups=1, weight_fl=b['w_fl'], input_fl=b['in_fl'], input_signed=b['in_signed'],
                   relu=b['relu_a'], label=f'b{i}.in' if i else None)
        d = g.conv(e, _w(30 + i, (E, 1, K, K), b['d_sig'] * 3.0 / K), bd, stride=b['stride'], pad=K // 2, groups=E, weight_fl=b['dw_w_fl'],
                   input_fl=b['dw_in_fl'], input_signed=b['dw_signed'], relu=b['relu_b'], label=f'b{i}.dw_in')
        wp, bp = _w(50 + i, (cout, E, 1, 1), b['p_sig']), _b(60 + i, cout, b['p_bsig'], b['p_bmean'])
        for ch, bias in b['pw_big'].items():
            bp[ch] = bias
        p = g.conv(d, wp, bp, pad=0, groups=1, weight_fl=b['pw_w_fl'], input_fl=b['pw_in_fl'], input_signed=b['pw_signed'], relu=b['pw_relu'],
                   label=f'b{i}.pw_in')
        o = g.add(p, t, relu=b['join_relu']) if b['res'] else p
        ids.append((e, d, p, o))
        t = o
    out = t
    if case.get('readers'):
        out = None
        for k, (fl, sgn) in enumerate(case['readers']):
            c = g.conv(t, _w(90 + k, (32, blocks[-1]['cout'], 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, relu=False,
                       label=f'reader{k}')
            out = c if out is None else g.add(out, c)
        if case.get('join_i32'):
            out = g.add(out, t)
    g.net.output(out, as_float=False)
    return g, out, ids


def make_input(name, case, n=None):
    c = case
    return synth.rand_uniform_int(5, f'irkx{name}', (n or c['N'], c['blocks'][0]['cin'], c['H'], c['W']), -127, 127).astype(np.int32)


def plan(name, case, x, fuse_irk, max_batch=None):
    """The case's graph planned with the given fuse_irk (1: the leg under test, 0: the three-launch plan of today)."""
    g, out, ids = build_graph(case, x)
    g.net.set_option('fuse_irk', fuse_irk)
    for k, v in case.get('opts', {}).items():
        g.net.set_option(k, v)
    g.net.finalize(max_batch or case.get('max_batch') or x.shape[0])
    return g, out, ids


def fused_lines(net):
    """[(plan token 'fused_irk5_s1_R9:', kernel name)] of the handle's fused launches, in launch order."""
    return [(net.launch_info(i, 1)[0].split(':')[0] + ':', net.launch_kernel(i)) for i in range(net.num_launches)
            if net.launch_info(i, 1)[0].startswith('fused_irk')]


def tokens(net):
    """The plan token of every launch ('conv1x1s1_t..', 'dwconv5x5s1', 'fused_irk5_s1_R9', ..), in launch order."""
    return [net.launch_info(i, 1)[0].split(':')[0] for i in range(net.num_launches)]


def kernel(K, cap, inst):
    return f'f8::fused_irk_kernel<{K}, {cap}, {inst}>'


def _case(blocks, H, W, N, expect, readers=((4, True),), **kw):
    """expect: one (tile token, output-channel cap, instance) per block, by hand."""
    d = dict(blocks=blocks, H=H, W=W, N=N, readers=list(readers) if readers else None,
             expect=[(f'fused_irk{b["K"]}_s{b["stride"]}_{tok}:', kernel(b['K'], cap, inst)) for b, (tok, cap, inst) in zip(blocks, expect)])
    d.update(kw)
    return d


# ---- geometry: 32 -> 192 -> 32 (three chunks; joined with the block input at stride 1), default formats (in 4 signed, w 6, dw 6 / 6, pw 6 / 6,
#      ReLUs on: n1 = 4, n2 = 6, instance 2), three images
GEOMETRY = {}
for _K, _S in ((5, 1), (5, 2), (7, 1), (7, 2)):
    _n = f'k{_K}s{_S}'
    _one = lambda **kw: [_kblk(_K, 32, 32, 192, _S, res=_S == 1, **kw)]
    # 1 x 1 and 3 x 3: smaller than the kernel, every tap but a few is padding.  1, 9 (stride 2: 4) output pixels: G = 8, one ragged group of 3
    GEOMETRY[f'{_n}_1x1'] = _case(_one(d_sig=60.0), 1, 1, 3, [('G8', 96, 2)])
    GEOMETRY[f'{_n}_3x3'] = _case(_one(d_sig=40.0), 3, 3, 3, [('G8', 96, 2)])
    # 9 x 11: 99 output pixels, one image per tile; stride 2: 5 x 6 = 30 -> G = 4 (the last window hangs over the edge)
    GEOMETRY[f'{_n}_9x11'] = _case(_one(), 9, 11, 3, [('R9' if _S == 1 else 'G4', 96, 2)])
    # 8 x 10: 80 output pixels; stride 2: 4 x 5 = 20 -> G = 6, one ragged group of 3 (the last row and column are never a window centre)
    GEOMETRY[f'{_n}_8x10'] = _case(_one(), 8, 10, 3, [('R8' if _S == 1 else 'G6', 96, 2)])
    # 14 x 14: 196 pixels -> rows: 128 // 14 = 9, two tiles of 7; stride 2: 49 pixels -> G = 2 whole images, groups of 2 and 1
    GEOMETRY[f'{_n}_14x14'] = _case(_one(), 14, 14, 3, [('R7' if _S == 1 else 'G2', 96, 2)])
# row tiles with both halos in the middle and a ragged last tile.  22 x 30: 128 // 30 = 4 rows, 6 tiles, R = 4, the last tile has 2 rows;
# 37 x 30 / 2 -> 19 x 15: 128 // 15 = 8 rows, 3 tiles, R = ceil(19 / 3) = 7, the last tile has 5 rows
GEOMETRY['k5s1_22x30_rows'] = _case([_kblk(5, 32, 32, 64, res=True)], 22, 30, 2, [('R4', 96, 2)])
GEOMETRY['k7s1_22x30_rows'] = _case([_kblk(7, 32, 32, 64, res=True)], 22, 30, 2, [('R4', 96, 2)])
GEOMETRY['k5s2_37x30_rows'] = _case([_kblk(5, 32, 32, 64, 2)], 37, 30, 2, [('R7', 96, 2)])
GEOMETRY['k7s2_37x30_rows'] = _case([_kblk(7, 32, 32, 64, 2)], 37, 30, 2, [('R7', 96, 2)])

# ---- channels
CHANNELS = {
    # everything padded (24 -> 32, 72 -> 96: the second chunk is half and mostly empty, 40 -> 64)
    'c_24_72_40_k5s2': _case([_kblk(5, 24, 40, 72, 2)], 9, 11, 3, [('G4', 96, 2)]),
    'c_40_240_80_k7s2': _case([_kblk(7, 40, 80, 240, 2)], 14, 14, 3, [('G2', 96, 2)]),
    # E = 64: one chunk
    'c_E64_k7s1_3x3': _case([_kblk(7, 32, 32, 64, res=True, d_sig=40.0)], 3, 3, 3, [('G8', 96, 2)]),
    'c_E64_k5s1_1x1': _case([_kblk(5, 32, 32, 64, res=True, d_sig=60.0)], 1, 1, 3, [('G8', 96, 2)]),
    # E = 1152 on 7 x 7: 18 chunks; 49 pixels -> G = 2 (103 KB of LDS)
    'c_192_1152_192_k5s1_7x7': _case([_kblk(5, 192, 192, 1152, res=True)], 7, 7, 3, [('G2', 192, 2)]),
    'c_96_128_192_k7s2': _case([_kblk(7, 96, 192, 128, 2)], 9, 11, 3, [('G4', 192, 2)]),
    # the widest output: 320 channels, five accumulator tiles per wave.  7 x 7: G = 2 (128 KB of LDS); 8 x 10 / 2 -> 20 pixels: G = 6 (X 30 KB +
    # patch 6 x 11 x 14 x 64 B = 58 KB + mid2 8 KB + 2 x 27 KB of weights = 150 KB <= 160 KB)
    'c_192_256_320_k7s1_7x7': _case([_kblk(7, 192, 320, 256)], 7, 7, 3, [('G2', 320, 2)]),
    'c_64_128_320_k5s2': _case([_kblk(5, 64, 320, 128, 2)], 8, 10, 3, [('G6', 320, 2)]),
}

# ---- formats.  Without a join at K5 / S1 and K7 / S2, with a join at K5 / S1 and K7 / S1; 32 -> 192 -> 32 on 9 x 11, N = 2
FORMATS = {}
_TOK = {(5, 1): 'R9', (7, 1): 'R9', (7, 2): 'G4'}


def _add(prefix, inst, kw, sets=((5, 1), (7, 2)), cio=(32, 32, 192), cap=96, **ckw):
    for K, S in sets:
        FORMATS[f'{prefix}_k{K}s{S}'] = _case([_kblk(K, cio[0], cio[1], cio[2], S, **kw)], 9, 11, 2, [(_TOK[(K, S)], cap, inst)], **ckw)


_JOIN = ((5, 1), (7, 1))
# the default block input is signed (in_fl 4): the plain case, and the one the requant_float = 1 leg is compared with
_add('f_signed_in', 2, {})
_add('f_rq1', 2, {}, opts={'requant_float': 1})                  # same symbol, same values as f_signed_in (test_gpu_irk.py compares them)
# a missing ReLU feeds a signed format: the generic instance (a signed depthwise input: the patch border is a real zero)
_add('f_signed_dw_in', 0, dict(relu_a=False, dw_signed=True, dw_in_fl=5, e_bmean=0.0))
_add('f_signed_pw_in', 0, dict(relu_b=False, pw_signed=True, pw_in_fl=5, d_bmean=0.0))
_add('f_no_relu_both', 0, dict(relu_a=False, dw_signed=True, dw_in_fl=5, e_bmean=0.0, relu_b=False, pw_signed=True, pw_in_fl=4, d_bmean=0.0))
# ... at 192 and 320 output channels (the generic instances of the wider caps), small maps
for _K in (5, 7):
    FORMATS[f'f_signed_dw_in_cap192_k{_K}'] = _case([_kblk(_K, 64, 160, 64, relu_a=False, dw_signed=True, dw_in_fl=5, e_bmean=0.0, d_sig=40.0)], 3, 3, 3,
                                                    [('G8', 192, 0)])
    FORMATS[f'f_signed_dw_in_cap320_k{_K}'] = _case([_kblk(_K, 96, 320, 64, relu_a=False, dw_signed=True, dw_in_fl=5, e_bmean=0.0, d_sig=40.0)], 3, 3, 3,
                                                    [('G8', 320, 0)])
_add('f_out_pw_relu', 2, dict(pw_relu=True, p_bmean=2.0 ** 13), readers=((4, False),))
# joins.  The stream (pre's result) has fraclen X_FL + in_fl + 2 + pre_fl = 11; the project result pw_in_fl + pw_w_fl
_add('f_join_acc_shl', 2, dict(res=True, pw_in_fl=5, pw_w_fl=4, pw_big={3: 2 ** 28 + 11, 17: -(2 ** 28) - 5}), _JOIN, readers=((1, True),), aim='join')
_add('f_join_res_shl', 2, dict(res=True, dw_w_fl=8, pw_in_fl=8, pw_w_fl=6, e_bmean=2.0 ** 11), _JOIN, pre_big={4: 2 ** 27 + 9, 21: -(2 ** 27) - 3},
     readers=((4, True),), aim='join')
_add('f_join_relu', 2, dict(res=True, join_relu=True, pw_in_fl=5, pw_w_fl=5, p_bmean=2.0 ** 12, pw_big={3: 2 ** 29 + 11, 17: -(2 ** 29) - 5}), _JOIN,
     readers=((3, False),), aim='join')
# inner shifts of 1 (small weights) and 17 (biases carry the values: weights of 8 bits cannot)
_S1 = dict(in_fl=4, w_fl=2, dw_in_fl=5, dw_w_fl=2, pw_in_fl=6, e_sig=0.7, e_bsig=40.0, e_bmean=60.0, d_sig=1.0, d_bsig=40.0, d_bmean=60.0)
_S17 = dict(in_fl=7, w_fl=13, dw_in_fl=3, dw_w_fl=14, pw_in_fl=0, pw_w_fl=8, e_sig=60.0, e_bsig=2.0 ** 22, e_bmean=2.0 ** 22, d_sig=60.0,
            d_bsig=2.0 ** 22, d_bmean=2.0 ** 22)
_add('f_shift1', 2, _S1)
_add('f_shift17', 2, _S17, readers=((0, True),))
# biases next to 2^31 in the expand and depthwise convs, so that `v + 2^(n-1)` wraps
_add('f_bias_big', 2, dict(bias_big=True), aim='bias_big')
# output forms: two readers at signed fraclen 1 / 0 behind project formats 8 / 7 (shifts 14 and 15); int32 only; int32 + int8 from one launch
_P15 = dict(pw_in_fl=8, pw_w_fl=7, dw_in_fl=6, dw_w_fl=8, p_sig=40.0, p_bsig=2.0 ** 19)
_add('f_out_two_i8', 2, _P15, readers=((1, True), (0, True)))
_add('f_out_i32', 2, {}, readers=None)
_add('f_out_i32_res', 2, dict(res=True), _JOIN, readers=None)
_add('f_out_i32_and_i8', 2, _P15, readers=((1, True), (0, True)), join_i32=True)

CASES = dict(GEOMETRY, **CHANNELS, **FORMATS)

# 9 x 11 / 2 -> 30 pixels: G = 4; planned for 8 images, run with 3 (one ragged group) and then 8 (two groups) from the same handle
MAX_BATCH_CASE = _case([_kblk(5, 32, 32, 96, 2)], 9, 11, 8, [('G4', 96, 2)], max_batch=8)

# a stride-2 opener and two joined blocks, K = 5, on an 18 x 22 map (-> 9 x 11: 99 pixels, one image per tile), N = 3, bench.py's schedule
PIPELINED_CASE = _case([_kblk(5, 32, 32, 96, 2), _kblk(5, 32, 32, 192, res=True, e_sig=5.0), _kblk(5, 32, 32, 192, res=True, e_sig=5.0)], 18, 22, 3,
                       [('R9', 96, 2), ('R9', 96, 2), ('R9', 96, 2)], opts=dict(_IR_PIPELINED['opts']))
