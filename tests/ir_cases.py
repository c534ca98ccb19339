"""Case table and graph builder of the op-level tests of the fused inverted-residual launch (f8_ir.hip): tests/test_ir_plan.py (plan, symbols
and liveness on the oracle, no GPU) and tests/test_gpu_ir.py (both legs against the oracle on the device).  No test functions here.

Every graph is  input -> `pre` 1x1 (pass 1e refuses a block that reads the net input) -> block(s) -> output, where the output is the last
block's int32 result itself (readers=None) or the sum of one 32-output 1x1 reader per (fraclen, signed) — plus the int32 block result when
`join_i32` is set (the block then writes int32 next to its int8 forms).

The expected tile token (R# / G#) and kernel instance of every case are WRITTEN BY HAND from fused_ir_config / ir_layout / fused_ir_inst /
ir_nw of f8_ir.hip; nothing here asks the planner for them."""
import numpy as np

from f8net_amd import synth
from refgraph import RefGraph

INT32_MIN_CLAMP = -(2 ** 31 - 1)


def _w(seed, shape, sig):
    return np.clip(synth.rand_normal_int(seed, f'w{shape}', shape, sig), -127, 127).astype(np.int32)


def _b(seed, n, sig, mean=0.0):
    return np.clip(synth.rand_normal_int(seed, f'b{n}', (n,), sig) + int(mean), -2 ** 30, 2 ** 30).astype(np.int32)


# A block.  Formats: in_fl / in_signed (what the expand conv reads), w_fl (expand weights), dw_in_fl / dw_signed, dw_w_fl, pw_in_fl / pw_signed,
# pw_w_fl; the inner shifts are n1 = in_fl + w_fl - dw_in_fl and n2 = dw_in_fl + dw_w_fl - pw_in_fl.  relu_a / relu_b: behind the expand / the
# depthwise conv; pw_relu: behind the project conv (no join then); res / join_relu: the join with the block input and a ReLU behind it.
# bias_big: biases next to 2^31 in the expand and depthwise convs; zero_ch {channel: bias}: project output channels with zero weights;
# pw_big {channel: bias}: project biases set by hand (weights stay).  *_sig / *_bsig / *_bmean: spreads of weights and biases (None: scaled from
# the channel counts so that the requantised values fill their 8 bits; the bias means keep fewer than half of the values behind a ReLU at 0).
def _blk(cin, cout, E, stride=1, **kw):
    d = dict(cin=cin, cout=cout, E=E, stride=stride, in_fl=4, in_signed=True, w_fl=6, dw_in_fl=6, dw_signed=False, dw_w_fl=6, pw_in_fl=6,
             pw_signed=False, pw_w_fl=6, relu_a=True, relu_b=True, pw_relu=False, res=False, join_relu=False, bias_big=False, zero_ch={}, pw_big={},
             e_sig=None, e_bsig=2.0 ** 10, e_bmean=2.0 ** 10, d_sig=20.0, d_bsig=2.0 ** 9, d_bmean=2.0 ** 12, p_sig=None, p_bsig=2.0 ** 11, p_bmean=0.0)
    d.update(kw)
    if d['e_sig'] is None:
        d['e_sig'] = 8.0 * (32.0 / cin) ** 0.5
    if d['p_sig'] is None:
        d['p_sig'] = 6.0 * (192.0 / E) ** 0.5
    return d


X_FL = 5


def build_graph(case, x):
    """Returns (graph, output tensor, per-block tensor ids [(expand, depthwise, project, block output)])."""
    blocks = case['blocks']
    g = RefGraph(x, X_FL)
    t = next(iter(g.v))
    c0 = blocks[0]['cin']
    # the pre conv's result is requantised by a shift of 7 whatever the first block's input format is
    bpre = _b(2, c0, 300.0)
    for ch, bias in case.get('pre_big', {}).items():
        bpre[ch] = bias
    t = g.conv(t, _w(1, (c0, c0, 1, 1), 12.0 * (32.0 / c0) ** 0.5), bpre, pad=0, groups=1, weight_fl=blocks[0]['in_fl'] + 2 + case.get('pre_fl', 0),
               input_fl=X_FL, input_signed=True, relu=False)
    ids = []
    for i, b in enumerate(blocks):
        E, cin, cout = b['E'], b['cin'], b['cout']
        be, bd = _b(10 + i, E, b['e_bsig'], b['e_bmean']), _b(40 + i, E, b['d_bsig'], b['d_bmean'])
        if b['bias_big']:                                        # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
            be[3], be[7] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
            bd[5], bd[11] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
        e = g.conv(t, _w(20 + i, (E, cin, 1, 1), b['e_sig']), be, pad=0, groups=1, weight_fl=b['w_fl'], input_fl=b['in_fl'], input_signed=b['in_signed'],
                   relu=b['relu_a'], label=f'b{i}.in' if i else None)
        d = g.conv(e, _w(30 + i, (E, 1, 3, 3), b['d_sig']), bd, stride=b['stride'], pad=1, groups=E, weight_fl=b['dw_w_fl'], input_fl=b['dw_in_fl'],
                   input_signed=b['dw_signed'], relu=b['relu_b'], label=f'b{i}.dw_in')
        wp, bp = _w(50 + i, (cout, E, 1, 1), b['p_sig']), _b(60 + i, cout, b['p_bsig'], b['p_bmean'])
        for ch, bias in b['zero_ch'].items():
            wp[ch] = 0
            bp[ch] = bias
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
    return synth.rand_uniform_int(5, f'x{name}', (n or c['N'], c['blocks'][0]['cin'], c['H'], c['W']), -127, 127).astype(np.int32)


def plan(name, case, x, fuse_ir, max_batch=None):
    """The case's graph planned with fuse_irchain = 0 and the given fuse_ir (2: the leg under test, 0: the comparison leg)."""
    g, out, ids = build_graph(case, x)
    g.net.set_option('fuse_irchain', 0)
    g.net.set_option('fuse_ir', fuse_ir)
    for k, v in case.get('opts', {}).items():
        g.net.set_option(k, v)
    g.net.finalize(max_batch or case.get('max_batch') or x.shape[0])
    return g, out, ids


def fused_lines(net):
    """[(plan token 'fused_ir_s1_R7:', kernel name)] of the handle's fused inverted-residual launches, in launch order."""
    return [(net.launch_info(i, 1)[0].split(':')[0] + ':', net.launch_kernel(i)) for i in range(net.num_launches)
            if net.launch_info(i, 1)[0].startswith('fused_ir_s')]


def _k(cin, cout, inst):
    return f'f8::fused_ir_kernel<{cin}, {cout}, {inst}, {"true" if cout <= 96 else "false"}, {8 if cout <= 96 else 4}>'


def _case(blocks, H, W, N, expect, readers=((4, True),), **kw):
    """expect: one (tile token, channel pair, instance) per block, by hand."""
    d = dict(blocks=blocks, H=H, W=W, N=N, readers=list(readers) if readers else None,
             expect=[(f'fused_ir_s{b["stride"]}_{tok}:', _k(ci, co, inst)) for b, (tok, (ci, co), inst) in zip(blocks, expect)])
    d.update(kw)
    return d


# ---- geometry: default formats (in 4 signed, w 6, dw 6 / 6, pw 6 / 6, ReLUs on: n1 = 4, n2 = 6, instance 2; 1 with requant_float = 1)
# Tile tokens from fused_ir_config: R = largest divisor of Ho with R * Wo <= cap (256 for <32, 32>, else 128); R == Ho -> G = min(8, 128 / (Ho * Wo))
GEOMETRY = {
    # 256 / 28 = 9 -> 7 rows (28 % 7 == 0); 52 KB of LDS <= 80 KB keeps it
    'g_32_32_28x28': _case([_blk(32, 32, 192)], 28, 28, 2, [('R7', (32, 32), 2)]),
    # Wo = 112: 256 / 112 = 2, 9 % 2 != 0 -> one output row per tile, 9 tiles: grid 9, nwg & 7 == 1
    'g_32_32_9x112_wide': _case([_blk(32, 32, 96)], 9, 112, 1, [('R1', (32, 32), 1)], opts={'requant_float': 1}),
    # 29 -> 15: 128 / 15 = 8 -> 5 rows; patch rows reach input row 29 (outside) in the last tile, patch column 30 is the right border
    'g_32_64_29x29_s2': _case([_blk(32, 64, 192, 2)], 29, 29, 2, [('R5', (32, 64), 2)]),
    'g_64_64_28x28_s2': _case([_blk(64, 64, 384, 2)], 28, 28, 3, [('R7', (64, 64), 2)]),
    # 12 x 20: 128 / 20 = 6 rows, 120 pixels of 128; three output-channel tiles over the two wave halves (JSPLIT = 2)
    'g_64_96_12x20': _case([_blk(64, 96, 384)], 12, 20, 2, [('R6', (64, 96), 1)], opts={'requant_float': 1}),
    'g_96_96_14x14_res': _case([_blk(96, 96, 576, res=True)], 14, 14, 3, [('R7', (96, 96), 2)]),
    # 10 -> 5: 25 output pixels, G = 128 / 25 = 5 images (135 KB of LDS); 7 images: tiles of 5 and 2
    'g_96_160_10x10_s2': _case([_blk(96, 160, 576, 2)], 10, 10, 7, [('G5', (96, 160), 0)]),
    # 49 pixels: G = 2; 5 images: tiles of 2, 2, 1
    'g_160_160_7x7_res': _case([_blk(160, 160, 960, res=True)], 7, 7, 5, [('G2', (160, 160), 0)]),
    # 128 / 14 = 9 -> 7 rows; ir_layout: X 20 KB + patch 9 KB + mid2 8 KB + 2 x 31 KB of weights = 99 KB <= 160 KB
    'g_160_320_14x14': _case([_blk(160, 320, 960)], 14, 14, 2, [('R7', (160, 320), 0)]),
    # 16 pixels: G = 8; 11 images: tiles of 8 and 3.  E = 64: one full chunk
    'g_32_32_4x4_G8': _case([_blk(32, 32, 64)], 4, 4, 11, [('G8', (32, 32), 2)]),
    # 3 x 5 -> 2 x 3: 6 pixels, G = min(8, 21); 9 images: tiles of 8 and 1
    'g_32_32_3x5_s2_G8': _case([_blk(32, 32, 96, 2)], 3, 5, 9, [('G8', (32, 32), 2)]),
    # 196 pixels <= 256: R = Ho = 14, G = 128 / 196 -> 1.  E = 32: one half chunk alone; E = 48: padded to 64 inside the chunk
    'g_E32_half_chunk': _case([_blk(32, 32, 32)], 14, 14, 2, [('R14', (32, 32), 2)]),
    'g_E48_padded_chunk': _case([_blk(32, 32, 48)], 14, 14, 2, [('R14', (32, 32), 2)]),
    # channel counts padded to 32 (E = 144 -> 160: a half last chunk)
    'g_24_24_res': _case([_blk(24, 24, 144, res=True)], 14, 14, 2, [('R14', (32, 32), 2)]),
    'g_16_64': _case([_blk(16, 64, 96)], 14, 14, 2, [('R7', (32, 64), 2)]),
}
# 64 pixels: G = 2; planned for 8 images, run with 3 (grid 2: nwg < 8, tiles of 2 and 1) and with 8 from the same handle
MAX_BATCH_CASE = _case([_blk(32, 32, 96)], 8, 8, 8, [('G2', (32, 32), 2)], max_batch=8)

# ---- formats.  <32, 32> at 6 x 6 / N = 3: G = 128 / 36 = 3 (one tile); <64, 96>, <64, 64> and <96, 96> at 14 x 14 / N = 2: R7;
#      <96, 160> at 7 x 7 / N = 3: G2 (tiles of 2 and 1)
_A = dict(H=6, W=6, N=3)
_Bg = dict(H=14, W=14, N=2)
_V = dict(H=7, W=7, N=3)


def _fmt(sets, blocks_of, tok_inst, **kw):
    """The same blocks on each of `sets`: (suffix, geometry, channel pair, E, tile token)."""
    out = {}
    for suf, geo, (ci, co), E, tok in sets:
        blocks = blocks_of(ci, co, E)
        out[suf] = _case(blocks, geo['H'], geo['W'], geo['N'], [(tok, (ci, co), tok_inst if co <= 96 else 0)] * len(blocks), **kw)
    return out


_G3 = ('32_32', _A, (32, 32), 96, 'G3')
_R7 = ('64_96', _Bg, (64, 96), 384, 'R7')
_R7S = ('64_64', _Bg, (64, 64), 384, 'R7')
_VALU = ('96_160', _V, (96, 160), 576, 'G2')
FORMATS = {}


def _add(prefix, sets, blocks_of, inst, **kw):
    for suf, c in _fmt(sets, blocks_of, inst, **kw).items():
        FORMATS[f'{prefix}_{suf}'] = c


# general instance 0 on the MFMA depthwise path: a missing ReLU feeds a signed format (a signed depthwise input: the patch border is a real zero)
_add('f_signed_dw_in', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, relu_a=False, dw_signed=True, dw_in_fl=5, e_bmean=0.0)], 0)
_add('f_signed_pw_in', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, relu_b=False, pw_signed=True, pw_in_fl=5, d_bmean=0.0)], 0)
_add('f_signed_both', (_G3, _R7, _VALU), lambda ci, co, E: [_blk(ci, co, E, relu_a=False, dw_signed=True, dw_in_fl=5, e_bmean=0.0, relu_b=False, pw_signed=True,
                                                              pw_in_fl=4, d_bmean=0.0)], 0)
# inner shifts of 1 (small weights), 16 and 17 (biases carry the values: weights of 8 bits cannot), 0 (general instance)
_S1 = dict(in_fl=4, w_fl=2, dw_in_fl=5, dw_w_fl=2, pw_in_fl=6, e_sig=0.7, e_bsig=40.0, e_bmean=60.0, d_sig=1.0, d_bsig=40.0, d_bmean=60.0)
_S16 = dict(in_fl=7, w_fl=12, dw_in_fl=3, dw_w_fl=13, pw_in_fl=0, pw_w_fl=8, e_sig=60.0, e_bsig=2.0 ** 21, e_bmean=2.0 ** 21, d_sig=60.0,
            d_bsig=2.0 ** 21, d_bmean=2.0 ** 21)
_S17 = dict(_S16, w_fl=13, dw_w_fl=14, e_bsig=2.0 ** 22, e_bmean=2.0 ** 22, d_bsig=2.0 ** 22, d_bmean=2.0 ** 22)
_add('f_shift1', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, **_S1)], 2)
_add('f_shift16_rq0', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, **_S16)], 2, readers=((0, True),), opts={'requant_float': 0})
_add('f_shift16_rq1', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, **_S16)], 1, readers=((0, True),), opts={'requant_float': 1})
_add('f_shift17_rq1', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, **_S17)], 2, readers=((0, True),), opts={'requant_float': 1})
_add('f_shift0_n1', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, in_fl=2, w_fl=2, dw_in_fl=4, dw_w_fl=6, pw_in_fl=6, e_sig=0.45 * (32.0 / ci) ** 0.5, e_bsig=30.0,
                                                         e_bmean=60.0, d_sig=8.0, d_bsig=2.0 ** 7, d_bmean=2.0 ** 10)], 0)
_add('f_shift0_n2', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, dw_in_fl=6, dw_w_fl=0, pw_in_fl=6, d_sig=0.4, d_bsig=20.0, d_bmean=60.0)], 0)
# biases next to 2^31 in the expand and depthwise convs: the accumulators are not bounded, so the integer instance with either requant_float
for _rq in (0, 1):
    _add(f'f_bias_big_rq{_rq}', (_G3, _R7, _VALU), lambda ci, co, E: [_blk(ci, co, E, bias_big=True)], 2, opts={'requant_float': _rq}, aim='bias_big')
# joins.  The stream (pre's result) has fraclen X_FL + in_fl + 2 + pre_fl; the project result pw_in_fl + pw_w_fl
_JS = (_G3, _R7S)
_add('f_join_acc_shl', _JS, lambda ci, co, E: [_blk(ci, co, E, res=True, pw_in_fl=5, pw_w_fl=4, pw_big={3: 2 ** 28 + 11, 17: -(2 ** 28) - 5})], 2,
     readers=((1, True),), aim='join')                                   # 9 against 11: acc_shl = 2
_add('f_join_res_shl', _JS, lambda ci, co, E: [_blk(ci, co, E, res=True, dw_w_fl=8, pw_in_fl=8, pw_w_fl=6, e_bmean=2.0 ** 11)], 2, pre_big={4: 2 ** 27 + 9, 21: -(2 ** 27) - 3},
     readers=((4, True),), aim='join')                                   # 14 against 11: res_shl = 3
_add('f_join_equal', _JS, lambda ci, co, E: [_blk(ci, co, E, res=True, pw_in_fl=6, pw_w_fl=5, pw_big={3: 2 ** 30 + 11, 17: -(2 ** 30) - 5})], 2,
     readers=((3, True),), aim='join')                                   # 11 against 11
_add('f_join_relu', _JS, lambda ci, co, E: [_blk(ci, co, E, res=True, join_relu=True, pw_in_fl=5, pw_w_fl=5, p_bmean=2.0 ** 12, pw_big={3: 2 ** 29 + 11, 17: -(2 ** 29) - 5})], 2,
     readers=((3, False),), aim='join')                                  # 10 against 11: acc_shl = 1, ReLU behind the join
# the int32 stream driven into the clamp (the zero_ch construction of test_gpu_irchain.py): channel 5 of block 0 is exactly 0, block 1's project
# result there is 2^30 << 1 (acc_shl 1), which wraps to -2^31 and is clamped to -(2^31 - 1); block 2 joins that stream
for _suf, _c in _fmt(_JS, lambda ci, co, E: [_blk(ci, co, E, zero_ch={5: 0, 9: 2 ** 30 - 7}),
                                             _blk(ci, co, E, res=True, pw_in_fl=5, zero_ch={5: 2 ** 30, 9: 2 ** 30 + 3}),
                                             _blk(ci, co, E, res=True, e_sig=5.0 * (32.0 / ci) ** 0.5)], 2, readers=None, aim='stream_clamp').items():
    FORMATS[f'f_stream_clamp_{_suf}'] = _c
    FORMATS[f'f_stream_clamp_i8_{_suf}'] = dict(_c, readers=[(4, True)])
# output forms: int32 only; one int8 reader (every case above); two readers at signed fraclen 1 / 0 behind project formats 8 / 7 (15 -> shifts 14
# and 15) with and without the int32 form; a project conv with ReLU and no join
_add('f_out_i32', (_G3, _R7, _VALU), lambda ci, co, E: [_blk(ci, co, E)], 2, readers=None)
_add('f_out_i32_res', (_G3,), lambda ci, co, E: [_blk(ci, co, E, res=True)], 2, readers=None)
_P15 = dict(pw_in_fl=8, pw_w_fl=7, dw_in_fl=6, dw_w_fl=8, p_sig=40.0, p_bsig=2.0 ** 19)
_add('f_out_two_i8', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, **_P15)], 2, readers=((1, True), (0, True)))
_add('f_out_two_i8_i32', (_G3,), lambda ci, co, E: [_blk(ci, co, E, **_P15)], 2, readers=((1, True), (0, True)), join_i32=True)
_add('f_out_pw_relu', (_G3, _R7), lambda ci, co, E: [_blk(ci, co, E, pw_relu=True, p_bmean=2.0 ** 13)], 2, readers=((4, False),))

CASES = dict(GEOMETRY, **FORMATS)

# two stride-1 blocks and one stride-2 block on a 28 x 28 map, N = 3, bench.py's schedule
PIPELINED_CASE = _case([_blk(32, 32, 192, res=True), _blk(32, 32, 192, res=True, e_sig=5.0), _blk(32, 64, 192, 2, e_sig=4.0)], 28, 28, 3,
                       [('R7', (32, 32), 2), ('R7', (32, 32), 2), ('R7', (32, 64), 2)],
                       opts={'whole_batch_launches': 1, 'arena_copies': 3, 'pipeline_depth': 3})
