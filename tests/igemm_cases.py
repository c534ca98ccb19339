"""Case tables and graph builder of the op-level tests of the implicit-GEMM conv kernel (conv_igemm_kernel of f8_kernels.hip, every instance
launch_conv dispatches): tests/test_igemm_plan.py (plan, symbols and liveness on the oracle, no GPU) and tests/test_gpu_igemm.py (every case against
the oracle on the device).  No test functions here.

Every graph is  input -> [`pre`: a 1x1 producer, so that the conv under test reads a requantised int8 form] -> the conv under test -> [add with an
int32 tensor: the conv's own input (`join='in'`) or `other`, a 1x1 from the net input with the conv's cout channels (`join='other'`) | the dual
pair: body 1x1 -> 1x1 (under test) joined with a 1x1 shortcut] -> [max-pool | average pool] -> output, where output 0 is the result itself
(readers=None) or the sum of one 32-output 1x1 reader per (fraclen, signed); `out_i32` next to readers makes the int32 result output 1.

Every plan runs with wstat = wreg = s2wreg = patch3x3 = fuse_blocks = fuse_pool = 0 (BASE_OPTS): the plan the late-stage kernels are compared with.

The expected plan token and kernel instance of every case are WRITTEN BY HAND from pick_conv_tile, conv_inst, conv_deep_stages and conv_wpx
(f8_kernels.hip); nothing here asks the planner for them.  With M = P * Q * max_batch output pixels, coutP and ck the channel counts padded to 32:
  bk   64 where ck % 64 == 0, else 32; 128 with bk128 = 1, ck % 128 == 0 and coutP > 32
  bn   128 from coutP = 96 on, 64 above 32, else 32; a join takes 128 back to 64
  bm   128; fewer than 512 tiles and bn >= 64 -> bm 64; still fewer than 512 and bn 128 -> bn 64
  the dual pair: bk 64, bn 64 (128 with coutP >= dual_wide and bm 128)
  igemm_tile 1 .. 4: 128x128, 128x64, 64x128, 64x64 where bn <= 64 or coutP > 64 (the dual pair: bn 64 or 128x128)
  ring: 4 slots where 4 * (bm + bn) * bk <= 64 KB and the K loop has at least deep_nk steps, else 2
On an 8 x 8 map that is: max_batch 3 (the three images of a run) -> 128x32 (coutP 32) or 64x64; 512 -> 64x128 (coutP >= 96, no join); 1024 -> 128x64 (coutP 64) or 128x128."""
import numpy as np

from f8net_amd import synth
from ir_cases import _b, _w
from refgraph import RefGraph

BASE_OPTS = dict(wstat=0, wreg=0, s2wreg=0, patch3x3=0, fuse_blocks=0, fuse_pool=0)
SHALLOW, DEEP = 1 << 20, 1                                   # deep_nk: no K loop is long enough / every one is
ADD_KERNEL, MAXPOOL_I32, MAXPOOL_I8, AVGPOOL = 'f8::add_kernel', 'f8::maxpool_kernel', 'f8::maxpool_i8x16_kernel', 'f8::avgpool_kernel'


def _tf(v):
    return 'true' if v else 'false'


def kern(bm, bn, bk, pad, res, stages, dual=False):
    wpx = 4 if bm == 128 and bn <= 64 else 2                 # conv_wpx
    return f'f8::conv_igemm_kernel<{bm}, {bn}, {bk}, {wpx}, {4 // wpx}, {_tf(pad)}, {_tf(res or dual)}, {stages}, {_tf(dual)}>'


def token(k, stride, bm, bn, bk, res=False, dual=False):
    return f'conv{k}x{k}s{stride}_t{bm}x{bn}x{bk}{"_res" if res else "_dual" if dual else ""}:'


def deep_stages(bm, bn, bk):                                 # conv_deep_stages
    return 4 if 4 * (bm + bn) * bk <= 65536 else 3 if 3 * (bm + bn) * bk <= 65536 else 2


TILES = [(128, 128, 128), (128, 64, 128), (64, 128, 128), (64, 64, 128), (128, 128, 64), (128, 64, 64), (128, 32, 64), (64, 128, 64), (64, 64, 64),
         (128, 128, 32), (128, 64, 32), (128, 32, 32), (64, 128, 32), (64, 64, 32)]          # the F8_CASE table of launch_conv


def all_instances():
    """Every instance launch_conv / launch_conv_t can dispatch: 14 tiles x HAS_PAD x HAS_RES x {2 slots, the deep ring where it is deeper} and the
    dual pair (bk 64; bn 64 or 128x128) at both depths."""
    out = set()
    for bm, bn, bk in TILES:
        rings = sorted({2, deep_stages(bm, bn, bk)})
        for ring in rings:
            for pad in (False, True):
                for res in (False, True):
                    out.add(kern(bm, bn, bk, pad, res, ring))
            if bk == 64 and (bn == 64 or (bn == 128 and bm == 128)):
                out.add(kern(bm, bn, bk, False, True, ring, dual=True))
    return out


def uniform_ld(bm, bn, bk):                                  # UNIFORM_LD of conv_igemm_kernel: every wave owns the same number of DMA slots
    return (bm * bk // 16) % 256 == 0 and (bn * bk // 16) % 256 == 0


# A case.  The conv under test: k, stride, pad, cin -> cout on an H x W map, groups; in_fl / in_signed / w_fl its formats, relu its ReLU.  x_fl: the
# net input's fraclen (8 bits: [0, 255] unsigned, [-127, 127] signed).  pre: {w_fl, relu} a 1x1 c0 -> cin in front (the conv then requantises by
# x_fl + pre.w_fl - in_fl).  join: None | 'in' | 'other'; o_fl: fraclen of `other` (its weights' is o_fl - x_fl); join_relu.  clamp: channel 5 of
# the conv and of the other operand have zero weights and biases whose aligned sum is exactly 2^31, channel 9 biases that bring the sum above 2^30.
# dual: {mid, stride}: input -> 1x1 / stride (c0 -> mid, ReLU) -> the conv under test (1x1, mid -> cout) + shortcut 1x1 / stride (c0 -> cout).
# dual.host = 'shortcut': the shortcut behind the conv under test (it then hosts the pair's launch).  o_set {channel: value}: channels of `other`
# with zero weights and that bias.
# w_seed: another draw of the weights where the first left a liveness condition of test_igemm_plan.py unmet (eight output channels are few).
# pool: None | ('max', k, stride, pad) | ('avg',) behind the result; readers [(fraclen, signed)]; out_i32.  shift: the right shift the spreads aim
# at — weights' sigma and biases are scaled so that the accumulators spread over about 2^shift * [0, 255].
def _case(k, cin, cout, tok, kernel, H=8, W=8, N=3, max_batch=None, stride=1, pad=0, why='', **kw):
    d = dict(k=k, cin=cin, cout=cout, H=H, W=W, N=N, max_batch=max_batch or N, stride=stride, pad=pad, groups=1, c0=None, x_fl=8, x_signed=False,
             in_fl=8, in_signed=False, w_fl=None, relu=True, pre=None, join=None, o_fl=None, join_relu=False, clamp=True, dual=None, pool=None,
             readers=[(4, False)], out_i32=False, shift=9, opts={}, token=tok, kernel=kernel, extra_tokens=[], why=why, w_seed=0, w_mul=1.0, bias_big=False, spread=None, x_hi=None, bias_set={}, o_set={})
    d.update(kw)
    if d['x_hi'] is None:
        d['x_hi'] = 127 if d['x_signed'] else 255
    if d['join'] == 'other':                                      # a 1x1 joined with a 1x1 of the same input is the dual pair unless fuse_dual is off
        d['opts'] = dict({'fuse_dual': 0}, **d['opts'])
    if d['pre'] is None and d['dual'] is None:
        d['c0'] = cin
        d['in_fl'], d['in_signed'] = d['x_fl'], d['x_signed']
    elif d['c0'] is None:
        d['c0'] = 32
    if d['w_fl'] is None:
        # the first reader's right shift n = in_fl + w_fl - its fraclen: at most 9, and small enough that about 24 of the launch's values per form
        # are exact ties (one value in 2^n is), so that round-half-even is seen going both ways
        P, Q = out_hw(d)
        auto = d['readers'] and not d['pool'] and not d['pre'] and not d['dual'] and d['o_fl'] is None
        n = max(2, min(9, int(np.log2(d['N'] * P * Q * cout / 24.0)))) if auto else 9
        d['w_fl'] = n + (d['readers'][0][0] if d['readers'] else 4) - d['in_fl']
        assert d['w_fl'] >= 0, 'a smaller x_fl makes room for the shift'
    if d['join'] and d['o_fl'] is None:
        d['o_fl'] = d['in_fl'] + d['w_fl']
    return d


def out_hw(c):
    return (c['H'] + 2 * c['pad'] - c['k']) // c['stride'] + 1, (c['W'] + 2 * c['pad'] - c['k']) // c['stride'] + 1


def _sig(K, second_moment, shift):
    """Weights' sigma for accumulators of about 80 * 2^shift over K products with inputs of the given root second moment."""
    return min(60.0, 80.0 * 2.0 ** shift / (K ** 0.5 * second_moment))


def _lg(v):
    return float(np.log2(v))


def build_graph(case, x):
    """Returns (graph, [output tensors], tensor id of the conv under test, tensor id of what leaves the launch (the join's result))."""
    c = case
    g = RefGraph(x, c['x_fl'])
    for key, v in dict(BASE_OPTS, **c['opts']).items():           # (before the ops: `grouped` decides what the builder accepts)
        g.net.set_option(key, v)
    t0 = next(iter(g.v))
    c0, cin, cout, k = c['c0'], c['cin'], c['cout'], c['k']
    rms_x = c['x_hi'] / 3.0 ** 0.5
    s = c['w_seed']
    joined = bool(c['join'] or c['dual'])
    # formats: the conv's result, the join's other operand, the align shifts (join_shifts of f8_net.cpp: the smaller fraclen shifts left)
    fl = c['in_fl'] + c['w_fl']
    o_fl = (c['x_fl'] + c['pre']['w_fl'] if c['pre'] else c['x_fl']) if c['join'] == 'in' else c['o_fl'] if c['o_fl'] is not None else fl
    acc_shl, res_shl = (max(0, o_fl - fl), max(0, fl - o_fl)) if joined else (0, 0)
    # the spread of what leaves the launch: about 80 * 2^(first reader's shift); the conv's own and the other operand's are that before the alignment
    n_out = c['shift'] if c['spread'] is None else _lg(c['spread'] / 80.0)
    if c['spread'] is None and c['readers'] and not c['pool']:
        n_out = max(fl, o_fl if joined else fl) - c['readers'][0][0]
    n, no = n_out - acc_shl, n_out - res_shl
    big5, big9 = 2 ** 30, 2 ** 29 + 3                             # channel 5: the aligned sum is 2^30 + 2^30; channel 9: above 2^30
    src = t0
    if c['pre']:                                                  # its result spreads over about +-100 * 2^(requant shift) around 0
        npre = c['x_fl'] + c['pre']['w_fl'] - c['in_fl']
        wp = _w(s + 1, (cin, c0, 1, 1), _sig(c0, rms_x, npre) * (1.0 if c['in_signed'] else 0.7))
        bp = _b(s + 2, cin, 2.0 ** (npre + 4), 0.0 if c['in_signed'] else 2.0 ** (npre + 6.5))
        if c['join'] == 'in' and c['clamp']:
            wp[5] = 0
            bp[5], bp[9] = big5 >> res_shl, big9 >> res_shl
        src = g.conv(t0, wp, bp, pad=0, groups=1, weight_fl=c['pre']['w_fl'], input_fl=c['x_fl'], input_signed=c['x_signed'],
                     relu=c['pre'].get('relu', False), quant_input=False, label='pre')
    if c['dual']:
        mid, st = c['dual']['mid'], c['dual']['stride']
        n0 = c['x_fl'] + 5 - c['in_fl']
        src = g.conv(t0, _w(s + 1, (mid, c0, 1, 1), _sig(c0, rms_x, n0) * 0.7), _b(s + 2, mid, 2.0 ** (n0 + 4), 2.0 ** (n0 + 6.5)), stride=st, pad=0,
                     groups=1, weight_fl=5, input_fl=c['x_fl'], input_signed=c['x_signed'], relu=True, quant_input=False, label='body0')
    reads_input = src == t0
    rms_in = rms_x if reads_input else (75.0 if c['in_signed'] else 120.0)
    G = c['groups']
    K = k * k * (src_ch := (c['dual']['mid'] if c['dual'] else cin)) // G
    w = _w(s + 10, (cout, src_ch // G, k, k), _sig(K, rms_in, n) * c['w_mul'])
    # an unsigned first reader: the values it reads are centred above 0, with a tenth of them below (the ReLU's floor, or the clamp's, is live)
    up = bool(c['readers']) and not c['readers'][0][1]
    b = _b(s + 11, cout, 2.0 ** (n + 4), 0.0 if joined else 2.0 ** (n + 6.7) if up else 2.0 ** (n + 5.3) if c['relu'] else 0.0)
    if c['readers'] and not joined and not c['pool']:            # channels 3 and 4 reach the clamps of every form
        nmax = max(fl - rfl for rfl, _ in c['readers'])
        b[3] = 2 ** (max(nmax, 0) + 8) + 5
        if not c['relu']:
            b[4] = -b[3]
    for ch, v in c['bias_set'].items():
        b[ch] = v
    if c['bias_big']:                                             # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
        b[3], b[17] = 2 ** 31 - 50, -(2 ** 31) + 50
    other = src if c['join'] == 'in' else None
    if c['join'] == 'other' or c['dual']:
        wo = _w(s + 20, (cout, c0, 1, 1), _sig(c0, rms_x, no))
        bo = _b(s + 21, cout, 2.0 ** (no + 4), 2.0 ** (no + 6.7) if up else 0.0)
        if c['clamp']:
            wo[5] = 0
            bo[5], bo[9] = big5 >> res_shl, big9 >> res_shl
        for ch, v in c['o_set'].items():                           # channels of the other operand that are exactly v (zero weights)
            wo[ch] = 0
            bo[ch] = v
    if joined and c['clamp']:
        assert c['join'] != 'in' or c['pre'], 'the clamp construction needs a conv behind the other operand'
        w[5] = 0
        b[5], b[9] = big5 >> acc_shl, 2 ** 29 >> acc_shl
    def shortcut():
        return g.conv(t0, wo, bo, stride=c['dual']['stride'] if c['dual'] else 1, pad=0, groups=1, weight_fl=o_fl - c['x_fl'], input_fl=c['x_fl'],
                      input_signed=c['x_signed'], relu=False, quant_input=False, label='other')
    # dual['host'] = 'shortcut' (tests/ostat_cases.py): the shortcut is added behind the conv under test and carries the join, as in a ResNet
    host_sc = bool(c['dual']) and c['dual'].get('host') == 'shortcut'
    if (c['join'] == 'other' or c['dual']) and not host_sc:
        other = shortcut()
    y = g.conv(src, w, b, stride=c['stride'], pad=c['pad'], groups=G, weight_fl=c['w_fl'], input_fl=c['in_fl'], input_signed=c['in_signed'],
               relu=c['relu'], quant_input=not reads_input, label='under_test' if not reads_input else None)
    g.net._L.f8_net_set_label(g.net._h, y, b'ut')
    if host_sc:
        other = shortcut()
        t = g.add(other, y, relu=c['join_relu'])
    else:
        t = g.add(y, other, relu=c['join_relu']) if other is not None else y
    g.other, g.shl = other, (acc_shl, res_shl)                     # (for the liveness checks: the join's operand and align shifts)
    g.weights = dict(ut=w, other=wo if (c['join'] == 'other' or c['dual']) else None)      # (... and the K slices of both products)
    if c['pool']:
        if c['pool'][0] == 'max':
            pk, ps, pp = c['pool'][1:4]
            o = g.maxpool(t, pk, ps, pp)
        else:
            o = g.avgpool_sum(t)
        pooled = o
        if c['pool'][-1] == 'twice':                              # the sum of two max-pools: a join no conv epilogue can carry
            pooled = g.add(o, g.maxpool(t, pk, ps, pp))
    else:
        pooled = t
    outs = []
    if c['readers']:
        out = None
        for i, (rfl, sgn) in enumerate(c['readers']):
            r = g.conv(pooled, _w(90 + i, (32, cout, 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=rfl, input_signed=sgn, relu=False,
                       label=f'reader{i}')
            out = r if out is None else g.add(out, r)
        outs.append(out)
    if c['out_i32'] or not c['readers']:
        outs.append(pooled)
    for o in outs:
        g.net.output(o, as_float=False)
    return g, outs, y, t


def make_input(name, case, n=None):
    c = case
    lo, hi = (-c['x_hi'], c['x_hi']) if c['x_signed'] else (0, c['x_hi'])
    return synth.rand_uniform_int(5, f'igx{name}', (n or c['N'], c['c0'], c['H'], c['W']), lo, hi).astype(np.int32)


def plan(name, case, x, max_batch=None):
    g, outs, y, t = build_graph(case, x)
    g.net.finalize(max_batch or case['max_batch'])
    return g, outs, y, t


def lines(net):
    """[(plan token up to its colon, kernel name)] of every launch of the handle, in launch order."""
    return [(net.launch_info(i, 1)[0].split(':')[0] + ':', net.launch_kernel(i)) for i in range(net.num_launches)]


def under_test(net):
    """[(token, kernel)] of the launches that run the conv under test (build_graph labels its tensor 'ut'; the dual pair's launch is 'other+ut')."""
    out = []
    for i in range(net.num_launches):
        tok, _, key = net.launch_info(i, 1)[0].partition(':')
        if 'conv' in tok and 'ut' in key.split('+'):
            out.append((tok + ':', net.launch_kernel(i)))
    return out


# ================================================================================================================================================
# Table A: one case per dispatchable instance.  8 x 8 maps, three images on a handle finalized for the max_batch the tile needs.
# REACH: how each (bm, bn) is reached — (cout, max_batch without a join, with a join): a number is the max_batch under the default selection,
# 'T#' the igemm_tile value on a handle for 3 images where pick_conv_tile never gives the tile.
#   128x32   coutP 32: bn 32 keeps bm 128 whatever M is
#   64x64    coutP 64, 192 pixels: 2 tiles < 512 -> bm 64
#   128x64   coutP 64, 65536 pixels: 512 tiles of 128x64
#   64x128   coutP 128, 32768 pixels: 256 tiles of 128x128 -> bm 64: 512 tiles; a join has bn 64 -> igemm_tile 3
#   128x128  coutP 128, 65536 pixels: 512 tiles; a join has bn 64 -> igemm_tile 1
# bk: cin = bk * (K steps) [x 9 taps with padding]; bk 128 needs bk128 = 1.  The ring: deep_nk 1 (every loop deep) / 2^20 (none).
REACH = {(128, 32): (32, 3, 3), (64, 64): (64, 3, 3), (128, 64): (64, 1024, 1024), (64, 128): (128, 512, 'T3'), (128, 128): (128, 1024, 'T1')}
TABLE_A = {}
_nk_rot = 0
for _bm, _bn, _bk in TILES:
    _cout, _mb_plain, _mb_res = REACH[(_bm, _bn)]
    for _ring in sorted({2, deep_stages(_bm, _bn, _bk)}):
        for _pad in (False, True):
            for _res in (False, True):
                # K steps: padded forms 9 (3x3 over cin = bk); the others 1, 2, 3 in turn
                _nk = 9 if _pad else ((1, 3, 5) if _bk == 32 else (1, 2, 3))[_nk_rot % 3]       # (ck = 64 would be bk 64: a 32-byte step has odd counts only)
                _nk_rot += 0 if _pad else 1
                _cin = _bk * (1 if _pad else _nk)
                _reach = _mb_res if _res else _mb_plain
                _opts = {'deep_nk': DEEP if _ring > 2 else SHALLOW}
                if _bk == 128:
                    _opts['bk128'] = 1
                if isinstance(_reach, str):
                    _opts['igemm_tile'] = int(_reach[1])
                _k = 3 if _pad else 1
                TABLE_A[f'a_{_bm}x{_bn}x{_bk}_{"p" if _pad else "n"}{"r" if _res else "n"}{_ring}'] = _case(
                    _k, _cin, _cout, token(_k, 1, _bm, _bn, _bk, res=_res), kern(_bm, _bn, _bk, _pad, _res, _ring), pad=1 if _pad else 0,
                    max_batch=3 if isinstance(_reach, str) else _reach, join='other' if _res else None, join_relu=_res and _pad, opts=_opts,
                    readers=[(4, False)] if (_pad or not _res) else [(4, True)], nk=_nk,
                    why=f'{"igemm_tile " + _reach[1] if isinstance(_reach, str) else "default selection at max_batch " + str(_reach)}')
# the dual pair: 64 -> 64 -> 64 channels, K loop of 1 + 1 steps; 128x128 with dual_wide = 0 (coutP 64 >= 0) on a handle for 1024 images
for _bm, _bn, _mb, _extra in ((64, 64, 3, {}), (128, 64, 1024, {}), (128, 128, 1024, {'dual_wide': 0})):
    for _ring in (2, 4):
        TABLE_A[f'a_{_bm}x{_bn}x64_dual{_ring}'] = _case(
            1, 64, 64, token(1, 1, _bm, _bn, 64, dual=True), kern(_bm, _bn, 64, False, True, _ring, dual=True), max_batch=_mb, c0=64,
            dual=dict(mid=64, stride=1), join_relu=True, opts=dict(_extra, deep_nk=DEEP if _ring > 2 else SHALLOW), nk=2,
            why=f'dual pair at max_batch {_mb}' + (', dual_wide 0' if _extra else ''))
# K loops of 9 steps without padding (3x3 / pad 0 on the 8 x 8 map: 6 x 6 outputs) and of 1 .. 3 steps with it (1x1 / pad 1: 10 x 10 outputs, the
# border ring reads nothing), on a uniform and a ragged tile at both depths: with the rows above, every depth sees 1, 2, 3 and 9 steps in both forms
for _bm, _bn, _bk, _cout in ((64, 64, 64, 64), (64, 64, 32, 64), (128, 32, 64, 32)):
    for _ring in (2, 4):
        _o = {'deep_nk': DEEP if _ring > 2 else SHALLOW}
        TABLE_A[f'a_{_bm}x{_bn}x{_bk}_nn{_ring}_k9'] = _case(3, _bk, _cout, token(3, 1, _bm, _bn, _bk), kern(_bm, _bn, _bk, False, False, _ring), opts=_o, nk=9, max_batch=3,
                                                            why='3x3 without padding: 9 steps, HAS_PAD false')
        for _nk in ((1, 3) if _bk == 32 else (1, 2, 3)):
            TABLE_A[f'a_{_bm}x{_bn}x{_bk}_pn{_ring}_k{_nk}'] = _case(1, _bk * _nk, _cout, token(1, 1, _bm, _bn, _bk), kern(_bm, _bn, _bk, True, False, _ring), pad=1, max_batch=3,
                                                                     opts=_o, nk=_nk, why='1x1 with pad 1: short K loop, HAS_PAD true')


# ================================================================================================================================================
# Table B: geometry.  Handles for 3 images unless noted: 64x64 (coutP >= 64) or 128x32 (coutP 32) tiles; ring 4 from 7 K steps on (deep_nk's default).
def _geo(k, cin, cout, H, W, stride=1, pad=0, N=3, **kw):
    ck, coutP = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    bk = 64 if ck % 64 == 0 else 32
    bm, bn = (128, 32) if coutP == 32 else (64, 64)
    nk = k * k * ck // bk
    ring = 4 if nk >= 7 else 2
    res = kw.get('join') is not None
    kw.setdefault('x_fl', 4)                                      # (a label: room for right shifts below 4 in front of a reader at fraclen 4)
    c = _case(k, cin, cout, token(k, stride, bm, bn, bk, res=res), kern(bm, bn, bk, pad > 0, res, ring), H=H, W=W, N=N, stride=stride, pad=pad, nk=nk, **kw)
    if 'x_hi' not in kw and not c['pre']:                         # inputs small enough that weights of sigma 6 give accumulators of about 80 * 2^shift
        n = c['in_fl'] + c['w_fl'] - c['readers'][0][0]
        c['x_hi'] = int(max(1, min(127 if c['x_signed'] else 255, round(3.0 ** 0.5 * 80.0 * 2.0 ** n / (6.0 * (k * k * cin) ** 0.5)))))
    return c


TABLE_B = {
    # kernels, strides, pads
    'b_k1_s2': _geo(1, 40, 40, 9, 7, stride=2),
    'b_k1_s3': _geo(1, 24, 8, 9, 7, stride=3, w_seed=200),
    'b_k1_p1': _geo(1, 8, 40, 5, 6, pad=1),                              # one pad above k / 2: the border ring is bias alone
    'b_k3_p0': _geo(3, 24, 40, 9, 7),
    'b_k3_p1_s2': _geo(3, 40, 96, 9, 7, stride=2, pad=1),
    'b_k3_p2_s3': _geo(3, 8, 160, 9, 7, stride=3, pad=2),                 # pad above k / 2; 160: a partial third 64-wide tile
    'b_k5_p0': _geo(5, 8, 8, 9, 7),
    'b_k5_p1_s2': _geo(5, 24, 40, 9, 7, stride=2, pad=1),
    'b_k5_p2': _geo(5, 96, 96, 9, 7, pad=2),
    'b_k5_p3_s3': _geo(5, 8, 40, 9, 7, stride=3, pad=3),
    'b_k7_p0': _geo(7, 8, 8, 9, 7),
    'b_k7_p1_s3': _geo(7, 8, 40, 9, 9, stride=3, pad=1),
    'b_k7_p2_s2': _geo(7, 24, 8, 9, 7, stride=2, pad=2),
    'b_k7_p3': _geo(7, 40, 160, 9, 7, pad=3),
    # maps smaller than the kernel
    'b_2x2_under_7x7': _geo(7, 8, 40, 2, 2, pad=3, N=5, w_mul=3.5),       # every row's taps fall outside at both ends (4 of 49 inside: larger weights)
    'b_1xW': _geo(3, 24, 40, 1, 11, pad=1),
    'b_Hx1': _geo(3, 24, 40, 11, 1, pad=1),
    'b_1x1_under_3x3': _geo(3, 40, 8, 1, 1, pad=1, N=7, w_seed=1900),
    # signed input: a single class (the padding is a real 0)
    'b_signed_k3_p1': _geo(3, 24, 40, 9, 7, pad=1, x_signed=True),
    'b_signed_k7_p3_s2': _geo(7, 8, 96, 9, 7, stride=2, pad=3, x_signed=True),
    # M around multiples of 32 and of bm = 64: 3 x 21 = 63, 5 x 13 = 65, N x 31 / 33 pixels
    'b_M63': _geo(1, 40, 40, 3, 7, N=3),
    'b_M65': _geo(1, 40, 40, 5, 13, N=1),
    'b_M31': _geo(3, 24, 40, 31, 1, pad=1, N=1),
    'b_M33': _geo(3, 24, 40, 3, 11, pad=1, N=1),
    'b_M127_bm128': _geo(1, 40, 8, 127, 1, N=1, w_seed=100),
    'b_M129_bm128': _geo(1, 40, 8, 43, 3, N=1, w_seed=100),
    # grids: 1 (above), 7 and 9 (one either side of the eight XCDs), 17 workgroups
    'b_grid7': _geo(1, 24, 40, 8, 8, N=7),                                # 448 pixels: 7 x 1 tiles of 64x64
    'b_grid9': _geo(1, 24, 160, 8, 8, N=3),                               # 192 pixels: 3 x 3
    'b_grid17': _geo(3, 24, 40, 8, 17, N=8, pad=1),                       # 1088 pixels: 17 x 1
    # joins on ragged maps
    'b_join_k3_p1': _geo(3, 40, 40, 9, 7, pad=1, join='other', readers=[(4, True)]),
    'b_join_in_k3_p1_96': _geo(3, 96, 96, 9, 7, pad=1, join='in', pre=dict(w_fl=5, relu=True), in_fl=4, w_fl=9, c0=32, x_fl=8, readers=[(4, False)]),
}
# coutP 96 under a 128-wide tile (the fourth 32-column block is skipped) and 160 (a partial second tile): 64x128 at max_batch 512
TABLE_B['b_cout96_bn128'] = _case(1, 24, 96, token(1, 1, 64, 128, 32), kern(64, 128, 32, False, False, 2), H=8, W=8, max_batch=512, nk=1)
TABLE_B['b_cout160_bn128'] = _case(3, 24, 160, token(3, 1, 128, 128, 32), kern(128, 128, 32, True, False, 4), H=8, W=8, pad=1, max_batch=1024, nk=9)
# one grouped dense expansion on a non-default tile: block-diagonal weights, 64x128 by igemm_tile
TABLE_B['b_grouped_dense'] = _case(3, 96, 96, 'gconv3x3s1_dense:', kern(64, 128, 32, True, False, 4), H=9, W=7, pad=1, groups=4, nk=27,
                                   opts={'grouped': 2, 'igemm_tile': 3})


# ================================================================================================================================================
# Table C: the epilogue.  64 -> 64 channels on a 9 x 7 map unless noted (64x64x64, 1 K step at 1x1: ring 2), conv fraclen 13.
def _epi(readers, k=1, cin=64, cout=64, **kw):
    pad = kw.pop('pad', 0)
    ck = (cin + 31) // 32 * 32
    bk = 64 if ck % 64 == 0 else 32
    nk = k * k * ck // bk
    bm, bn = (128, 32) if cout <= 32 else (64, 64)
    res, dual = kw.get('join') is not None, kw.get('dual') is not None
    if dual:                                                      # both products: mid / 64 + c0 / 64 steps
        nk = kw['dual']['mid'] // 64 + kw['c0'] // 64
    kw.setdefault('H', 9)
    kw.setdefault('W', 7)
    return _case(k, cin, cout, token(k, 1, bm, bn, bk, res=res, dual=dual), kern(bm, bn, bk, pad > 0, res, 4 if nk >= 7 else 2, dual=dual), pad=pad,
                 readers=readers, nk=nk, **kw)


_U, _S = (4, False), (4, True)
TABLE_C = {
    # readers
    'c_u': _epi([_U]),
    'c_s': _epi([_S], relu=False),
    'c_s_behind_relu': _epi([(3, True)]),
    # fraclens 2 + 3 = 5, inputs in [0, 3]: q[0] right shift by 1 unsigned, q[1] left shift by 1 signed; channel 3 reaches 255 * 2
    'c_u_and_left': _epi([(4, False), (6, True)], x_fl=2, w_fl=3, x_hi=3, spread=25.0, bias_set={3: 600, 4: 505, 6: 2}),
    'c_left_shift0': _epi([(5, True)], x_fl=2, w_fl=3, x_hi=3, spread=50.0, relu=False),     # shift 0: requant_shl with nothing to shift
    'c_three_formats': _epi([_U, (3, True), (3, False)], extra_tokens=[('requant:', ADD_KERNEL)]),
    # int32 alone, next to one and two int8 forms
    'c_i32': _epi(None),
    'c_i32_u': _epi([_U], out_i32=True),
    'c_i32_u_s': _epi([_U, (3, True)], out_i32=True),
    'c_no_relu_u': _epi([_U], relu=False),
    # joins: the two align directions and none; ReLU behind the join on / off
    'c_join_acc_shl': _epi([(5, True)], join='other', o_fl=15),                     # 13 against 15: acc_shl 2
    'c_join_res_shl': _epi([_S], join='other', o_fl=10),                                     # 13 against 10: res_shl 3
    'c_join_equal': _epi([_S], join='other'),
    'c_join_relu1': _epi([_U], join='other', join_relu=True),
    'c_join_no_relu0': _epi([_S], join='other', relu=False, o_fl=12),
    'c_join_in_pre': _epi([_S], join='in', pre=dict(w_fl=5), in_fl=6, in_signed=True, w_fl=7, c0=32),     # the conv's own input, 13 against 13
    'c_join_i32_only': _epi(None, join='other', join_relu=True),
    'c_join_i32_two_i8': _epi([_U, (3, True)], join='other', out_i32=True),
    'c_join_pad': _epi([_S], k=3, pad=1, join='other', o_fl=12),
    'c_bias_big': _epi([_U, (3, True)], bias_big=True),                           # accumulators next to +-2^31: the rounding add wraps
    # the dual pair, equal strides and the shortcut (and body.0) at stride 2 against the 1x1's stride 1
    'c_dual': _epi([_U], dual=dict(mid=64, stride=1), c0=64, join_relu=True),
    'c_dual_s2': _epi([_S], dual=dict(mid=64, stride=2), c0=64, o_fl=12),
    'c_dual_acc_shl_i32': _epi([(7, False)], dual=dict(mid=64, stride=2), c0=64, o_fl=14, join_relu=True, out_i32=True),
    # requant_float once each (the integer form either way in this kernel; the plan must not move)
    'c_requant_float0': _epi([_U], opts={'requant_float': 0}),
    'c_requant_float1': _epi([_U], opts={'requant_float': 1}),
    # the element-wise launches behind the conv
    'c_maxpool_i32': _epi([_U], pool=('max', 3, 2, 1), out_i32=True, extra_tokens=[('maxpool_i32:', MAXPOOL_I32)]),
    'c_maxpool_i8': _epi([_U], pool=('max', 3, 2, 1), extra_tokens=[('maxpool_i8:', MAXPOOL_I8)]),
    'c_maxpool_i32_twice': _epi(None, pool=('max', 3, 2, 1, 'twice'), extra_tokens=[('maxpool_i32:', MAXPOOL_I32), ('add:', ADD_KERNEL)]),
    'c_avgpool_6px': _epi(None, pool=('avg',), H=2, W=3, extra_tokens=[('avgpool_sum:', AVGPOOL)]),
    'c_avgpool_49px': _epi(None, pool=('avg',), H=7, W=7, extra_tokens=[('avgpool_sum:', AVGPOOL)]),
}
CASES = dict(TABLE_A, **TABLE_B, **TABLE_C)
