"""Case table, reference and graph builder of the tests of dilated convolutions (f8_net_conv_dilated / `F8Net.conv(dilation=)`): tests/test_dilated_plan.py
(acceptance, refusals, plan tokens, kernel symbols, liveness on the reference, `topology.dilate`, the ONNX round trip; no GPU) and tests/test_gpu_dilated.py
(every case bit for bit on the device).  No test functions here.

The reference.  `oracle.conv2d` has no dilation and stays as it is, but it takes any kernel size: a dilated K x K conv equals the plain
(d (K - 1) + 1)-square conv whose weights are zero except at [::d, ::d], with the same stride, pad and groups — `ref_ops.stuffed(w, d)`, which
RefGraph.conv and refgraph.graph_forward evaluate a dilated conv with.  That is also what a
user of the library could do before this entry point existed.  test_dilated_plan.py pins the stuffed integer conv to
torch.nn.functional.conv2d(float64, dilation=d), which is exact here (|acc| << 2^53).

Every op-level graph is  input -> dilated conv (the conv under test; it reads the net input as it is, quant_input = False) -> output, where the output
is the conv's int32 result itself (readers=None) or the sum of one 32-output 1x1 reader per (fraclen, signed) — plus the int32 result when `join_i32`
is set (the launch then writes int32 next to its int8 forms).  `res` cases put a 1x1 in front and join the dilated conv with that 1x1's result, as a
BasicBlock does (the add rides in the dilated conv's epilogue); `second` chains two dilated convs through nothing but their requantisation.

Expected plan tokens and kernel symbols are WRITTEN BY HAND from label_conv_step / pick_conv_tile / conv_kernel_name / dwk_kernel_name; nothing here
asks the planner for them.  Small launches (fewer than 512 tiles, all of these): coutP 32 -> tile 128x32, else 64x64; bk 64 where the padded input
channels are a multiple of 64, else 32; nine K steps and more run the four-slot ring."""
import functools

import numpy as np

from f8net_amd import synth
from ir_cases import PIPELINED_CASE as _IR_PIPELINED
from ir_cases import _b, _w
from ref_ops import stuffed
from refgraph import RefGraph

# every fusing pass of the planner switched on (the options that are off by default among them)
FUSE_ALL = dict(fuse_blocks=1, fuse_ds=1, fuse_opener=1, fuse_chain=1, fuse_chain7=1, fuse_tail=1, fuse_p12=1, fuse_bchain=2, fuse_bchain7=2, fuse_ir=2,
                fuse_irchain=1, fuse_irk=1, fuse_dws=1, fuse_dws7=1, fuse_head2=1, fuse_head_dws=1, fuse_pool=1, fuse_dual=1, fuse_stem=1)


def out_size(n, k, stride, pad, d):
    return (n + 2 * pad - d * (k - 1) - 1) // stride + 1


# A case.  kind: 'plain' (groups 1), 'dw' (groups = C = cout) or 'grouped' (C in groups of cg).  Geometry of the dilated 3x3: H x W map, dilation d,
# pad, stride; N images.  Formats as gconv_cases: in_fl / in_signed (the net input's and the conv's), w_fl, relu, readers [(fraclen, signed)],
# join_i32, bias_big.  res: BasicBlock-style join (see the module text).  opts: planning options.  w_sig = None: 150 / sqrt(taps x input channels of
# one output), which fills the 8 bits behind the default shift of 9.
def _case(kind, C, cout, H, W, d, pad, stride=1, N=3, **kw):
    c = dict(kind=kind, C=C, cout=cout, H=H, W=W, d=d, pad=pad, stride=stride, N=N, K=3, cg=4, in_fl=8, in_signed=False, w_fl=5, relu=True,
             readers=[(4, False)], join_i32=False, res=False, second=None, bias_big=False, w_sig=None, b_sig=2.0 ** 9, b_mean=2.0 ** 13, opts={})
    c.update(kw)
    assert out_size(H, 3, stride, pad, d) >= 1 and out_size(W, 3, stride, pad, d) >= 1, (H, W, d, pad)
    assert kind != 'dw' or (C == cout and pad <= d)
    return c


def groups_of(c):
    return {'plain': 1, 'dw': c['C'], 'grouped': c['C'] // c['cg']}[c['kind']]


def weights(c, seed=30):
    cin_g = c['C'] // groups_of(c)
    sig = c['w_sig'] or 150.0 / (9 * cin_g) ** 0.5
    return _w(seed, (c['cout'], cin_g, 3, 3), sig)


def centre_only(w):
    z = np.zeros_like(w)
    z[:, :, 1, 1] = w[:, :, 1, 1]
    return z


def biases(c, seed=40):
    bd = _b(seed, c['cout'], c['b_sig'], c['b_mean'])
    if c['bias_big']:                                            # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
        bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
    return bd


def build_graph(case, x, record=True, centre=False):
    """Returns (graph, output tensor, [tensor ids of the dilated convs]).  centre: the reference runs with every tap but the centre zeroed."""
    c = case
    g = RefGraph(x, c['in_fl'], grouped=c['opts'].get('grouped', 1) if c['kind'] == 'grouped' else None, record=record)
    t = next(iter(g.v))
    G = groups_of(c)
    w = weights(c)
    ev = centre_only(w) if centre else None
    if c['res']:                                                 # 1x1 (ReLU, int32 + int8) -> dilated 3x3 / 1 at pad = d -> join with the 1x1's result, ReLU
        r = c['res']
        pre = g.conv(t, _w(20, (c['C'], c['C'], 1, 1), 150.0 / c['C'] ** 0.5), _b(21, c['C'], 2.0 ** 9, 2.0 ** 12), pad=0, groups=1, weight_fl=r['pre_w_fl'],
                     input_fl=c['in_fl'], input_signed=c['in_signed'], relu=True, quant_input=False)
        d = g.conv(pre, w, biases(c), stride=1, pad=c['pad'], groups=G, weight_fl=c['w_fl'], input_fl=r['in_fl'], input_signed=False, relu=False,
                   dilation=c['d'], w_eval=ev, label='res_in')
        ids = [d]
        t = g.add(d, pre, relu=True)
    else:
        d = g.conv(t, w, biases(c), stride=c['stride'], pad=c['pad'], groups=G, weight_fl=c['w_fl'], input_fl=c['in_fl'], input_signed=c['in_signed'],
                   relu=c['relu'], quant_input=False, dilation=c['d'], w_eval=ev)
        ids = [d]
        t = d
        if c['second']:                                          # -> a second dilated conv that requantises the first one's result
            s = c['second']
            w2 = weights(c, 31)
            t = g.conv(t, w2, biases(c, 41), stride=s['stride'], pad=s['pad'], groups=G, weight_fl=s['w_fl'], input_fl=s['in_fl'], input_signed=False,
                       relu=True, dilation=s['d'], w_eval=centre_only(w2) if centre else None, label='second_in')
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
    if record:
        g.net.output(out, as_float=False)
    return g, out, ids


def make_input(name, case, n=None):
    c = case
    hi = 127 if c['in_signed'] else 255
    return synth.rand_uniform_int(5, f'dilx{name}', (n or c['N'], c['C'], c['H'], c['W']), -hi if c['in_signed'] else 0, hi).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(name, centre):
    case = ALL[name]
    g, out, ids = build_graph(case, make_input(name, case, case.get('max_batch')), record=False, centre=centre)
    return g, out, ids


def reference(name, centre=False):
    """(graph, output id, conv ids) of the case evaluated on the reference alone, computed once per case (over max_batch images where the case has one);
    nothing may write into its arrays."""
    return _reference(name, centre)


def plan(name, case, x, max_batch=None, **opts):
    g, out, ids = build_graph(case, x)
    for k, v in dict(case['opts'], **opts).items():
        g.net.set_option(k, v)
    g.net.finalize(max_batch or case.get('max_batch') or x.shape[0])
    return g, out, ids


# ---- expected tokens and symbols, by hand
def _cs(c):
    return -(-c // 32) * 32


def igemm_tile(c):
    coutP, Cs = _cs(c['cout']), _cs(c['C'])
    bm, bn = (128, 32) if coutP == 32 else (64, 64)
    return bm, bn, 64 if Cs % 64 == 0 else 32


def igemm_symbol(bm, bn, bk, pad, res):
    wpx = 4 if bm == 128 and bn <= 64 else 2
    return f'f8::conv_igemm_kernel<{bm}, {bn}, {bk}, {wpx}, {4 // wpx}, {"true" if pad else "false"}, {"true" if res else "false"}, 4, false>'


def dw_symbol(dot4, stride, int8_only, signed):
    """dwconv3x3_dil_dot4_kernel exactly where dwconvk_dot4_kernel would run an undilated conv — option dwk_dot4, int8 forms only — and at stride 1."""
    if dot4 and stride == 1 and int8_only:
        return 'f8::dwconv3x3_dil_dot4_kernel'
    return f'f8::dwconvk_kernel<{"true" if signed else "false"}>'


def expect(case, dot4=True, tile=None):
    """[(plan token up to ':', kernel symbol)] of the case's dilated convs, in launch order."""
    c = case
    geo = [(c['stride'], c['d'], c['pad'])] + ([(c['second']['stride'], c['second']['d'], c['second']['pad'])] if c['second'] else [])
    out = []
    for i, (s, d, pad) in enumerate(geo):
        if c['kind'] == 'dw':
            feeds_second = i == 0 and c['second']                 # read by the second conv only: one int8 form
            int8_only = bool(feeds_second or (c['readers'] and not c['join_i32']))
            out.append((f'dwconv3x3s{s}d{d}:', dw_symbol(dot4, s, int8_only, c['in_signed'] and i == 0)))
            continue
        bm, bn, bk = tile or igemm_tile(c)
        res = bool(c['res'])
        if c['kind'] == 'grouped':
            out.append((f'gconv3x3s{s}d{d}_dense:', igemm_symbol(bm, bn, bk, pad > 0, False)))
        else:
            out.append((f'conv3x3s{s}d{d}_t{bm}x{bn}x{bk}{"_res" if res else ""}:', igemm_symbol(bm, bn, bk, pad > 0, res)))
    return out


def d_lines(net):
    """[(plan token, kernel symbol)] of the handle's dilated launches, in launch order: the conv tokens that carry d<D> behind the stride."""
    out = []
    for i in range(net.num_launches):
        tok = net.launch_info(i, 1)[0].split(':')[0] + ':'
        head = tok.split('_')[0].rstrip(':')
        if 'x3s' in head and 'd' in head.split('x3s')[1]:
            out.append((tok, net.launch_kernel(i)))
    return out


# ---- plain convs.  Defaults: unsigned fraclen-8 input, weights at 5, ReLU, one unsigned reader at fraclen 4 (shift 9); three images = sub-batches of 2 and 1
PLAIN = {
    # the must-haves
    'p_7x7_d4_pad4_rows_lose_both_outer_taps': _case('plain', 32, 32, 7, 7, 4, 4),            # H <= 2 d: masks 010, 011, 110 — nine classes a side
    'p_9x11_d6_pad6_most_taps_outside': _case('plain', 40, 72, 9, 11, 6, 6),
    'p_14x14_d2_pad1_pad_below_d': _case('plain', 64, 128, 14, 14, 2, 1),                      # unsigned, pad < d: -> 12 x 12
    'p_9x11_d3_pad1_pad_below_d': _case('plain', 32, 32, 9, 11, 3, 1),                         # -> 5 x 7
    # maps x dilations x pads x strides x channels
    'p_7x7_d2_pad2': _case('plain', 40, 72, 7, 7, 2, 2),
    'p_7x7_d2_pad0': _case('plain', 64, 128, 7, 7, 2, 0),                                      # -> 3 x 3, no padding instance
    'p_7x7_d3_pad3_s2': _case('plain', 32, 32, 7, 7, 3, 3, 2),
    'p_9x11_d2_pad2_s2': _case('plain', 64, 128, 9, 11, 2, 2, 2),                              # odd both ways, stride 2
    'p_9x11_d4_pad0': _case('plain', 32, 32, 9, 11, 4, 0),                                     # -> 1 x 3
    'p_9x11_d4_pad4': _case('plain', 64, 128, 9, 11, 4, 4),
    'p_5x35_d2_pad2': _case('plain', 32, 32, 5, 35, 2, 2),                                     # wider than one 32-pixel group
    'p_5x35_d3_pad3_s2': _case('plain', 40, 72, 5, 35, 3, 3, 2),
    'p_5x35_d6_pad6': _case('plain', 64, 128, 5, 35, 6, 6),                                    # H <= 2 d in rows only
    'p_5x35_d2_pad1': _case('plain', 40, 72, 5, 35, 2, 1),                                     # -> 3 x 33
    'p_14x14_d2_pad2': _case('plain', 32, 32, 14, 14, 2, 2),                                   # 588 pixels: five 128-pixel tiles
    'p_14x14_d3_pad3': _case('plain', 40, 72, 14, 14, 3, 3),
    'p_14x14_d4_pad4_s2': _case('plain', 64, 128, 14, 14, 4, 4, 2),
    'p_14x14_d6_pad6': _case('plain', 32, 32, 14, 14, 6, 6),
    'p_14x14_d6_pad1': _case('plain', 40, 72, 14, 14, 6, 1),                                   # -> 4 x 4
    'p_14x14_d4_pad0_s2': _case('plain', 64, 128, 14, 14, 4, 0, 2),                            # -> 3 x 3
}
_SGN = dict(in_fl=7, in_signed=True, b_mean=0.0, b_sig=2.0 ** 11)
PLAIN_FORMATS = {
    'pf_signed_in_d2': _case('plain', 40, 72, 9, 11, 2, 2, relu=False, readers=[(4, True)], **_SGN),      # signed input: the pad value is a real 0, one bias class
    'pf_signed_in_d4_s2': _case('plain', 32, 32, 9, 11, 4, 4, 2, readers=[(3, False)], **dict(_SGN, b_mean=2.0 ** 12)),
    'pf_no_relu': _case('plain', 64, 128, 9, 11, 2, 2, relu=False, readers=[(3, True)], b_mean=-2.0 ** 13, b_sig=2.0 ** 12),
    'pf_two_readers': _case('plain', 40, 72, 9, 11, 3, 3, readers=[(4, False), (3, False)]),               # shifts 9 and 10 in one launch
    'pf_mixed_readers_s2': _case('plain', 32, 32, 9, 11, 2, 1, 2, readers=[(4, False), (3, True)]),
    'pf_i32_only': _case('plain', 64, 128, 9, 11, 2, 2, readers=None),
    'pf_i32_only_d4_pad1': _case('plain', 32, 32, 9, 11, 4, 1, readers=None, relu=False),
    'pf_i32_and_i8': _case('plain', 32, 32, 9, 11, 2, 2, join_i32=True),                               # (the join with the readers' 32 channels: cout 32)
    'pf_bias_big': _case('plain', 32, 32, 9, 11, 2, 2, bias_big=True),
    'pf_bias_big_d3_s2': _case('plain', 64, 128, 7, 7, 3, 3, 2, bias_big=True),
    'pf_rq1': _case('plain', 40, 72, 9, 11, 2, 2, opts={'requant_float': 1}),
}
# the fused residual join: pre 1x1 at weight fraclen 5 (result at 13, ReLU) -> dilated conv reads it at fraclen 4 (shift 9), weights at 9 (result at 13
# too: the two operands weigh the same) -> conv + pre, ReLU; the reader takes the sum at fraclen 4 (shift 9)
_RES = dict(pre_w_fl=5, in_fl=4)
PLAIN_RES = {
    'pr_d2_14x14': _case('plain', 64, 64, 14, 14, 2, 2, res=_RES, w_fl=9),
    'pr_d4_7x7_unsigned_both_taps': _case('plain', 32, 32, 7, 7, 4, 4, res=_RES, w_fl=9),
    'pr_d3_9x11_i32_and_i8': _case('plain', 32, 32, 9, 11, 3, 3, res=_RES, w_fl=9, join_i32=True),
    'pr_d2_9x11_c40': _case('plain', 40, 40, 9, 11, 2, 2, res=_RES, w_fl=9),
}
# igemm_tile 1 .. 4 on one case: 128x128 / 128x64 / 64x128 / 64x64 (all admissible at coutP 128)
TILE_CASE = 'p_9x11_d4_pad4'
TILES = {1: (128, 128, 64), 2: (128, 64, 64), 3: (64, 128, 64), 4: (64, 64, 64)}

# ---- depthwise.  W < d (3), W no multiple of 4 d, an empty residue class (W = 3 at d = 4: residue 3 holds no pixel)
DW = {
    'd_c32_9x3_d4_pad4': _case('dw', 32, 32, 9, 3, 4, 4),                                       # W < d: one pixel per residue, residue 3 empty
    'd_c32_9x3_d2_pad2': _case('dw', 32, 32, 9, 3, 2, 2),
    'd_c40_9x9_d2_pad2': _case('dw', 40, 40, 9, 9, 2, 2),                                       # 9 = 8 + 1: a second group with one live pixel in one residue
    'd_c96_9x9_d3_pad3': _case('dw', 96, 96, 9, 9, 3, 3),
    'd_c32_9x9_d4_pad0': _case('dw', 32, 32, 9, 9, 4, 0),                                       # -> 1 x 1
    'd_c96_5x11_d2_pad1': _case('dw', 96, 96, 5, 11, 2, 1),                                     # pad < d: -> 3 x 9
    'd_c40_9x11_d3_pad3': _case('dw', 40, 40, 9, 11, 3, 3),
    'd_c32_9x11_d4_pad2': _case('dw', 32, 32, 9, 11, 4, 2),                                     # -> 5 x 7
    'd_c96_14x14_d2_pad2': _case('dw', 96, 96, 14, 14, 2, 2),                                   # MobileNet-V2 OS16's geometry
    'd_c40_14x14_d4_pad4': _case('dw', 40, 40, 14, 14, 4, 4),
    'd_c32_14x14_d3_pad0': _case('dw', 32, 32, 14, 14, 3, 0),                                   # -> 8 x 8
    'd_c32_5x35_d2_pad2': _case('dw', 32, 32, 5, 35, 2, 2),                                     # 35 = 4 groups of 8 + 3
    'd_c40_5x35_d3_pad3': _case('dw', 40, 40, 5, 35, 3, 3),
    'd_c96_5x35_d4_pad4': _case('dw', 96, 96, 5, 35, 4, 4),                                     # 35 = 2 groups of 16 + 3
    'd_signed_in': _case('dw', 40, 40, 9, 11, 2, 2, relu=False, readers=[(4, True)], **_SGN),
    'd_two_readers': _case('dw', 32, 32, 9, 11, 3, 3, readers=[(4, False), (3, True)]),
    'd_bias_big': _case('dw', 32, 32, 9, 11, 2, 2, bias_big=True),
    'd_rq1': _case('dw', 40, 40, 9, 11, 2, 2, opts={'requant_float': 1}),
}
# the generic kernel whatever dwk_dot4 says: stride 2, and the int32 form
DW_GENERIC = {
    'dg_s2_d2': _case('dw', 40, 40, 9, 11, 2, 2, 2),
    'dg_s2_d3_14x14_pad1': _case('dw', 96, 96, 14, 14, 3, 1, 2),
    'dg_s2_d4_signed': _case('dw', 32, 32, 9, 11, 4, 4, 2, relu=False, readers=[(4, True)], **_SGN),
    'dg_i32_only_d2': _case('dw', 32, 32, 9, 11, 2, 2, readers=None),
    'dg_i32_and_i8_d3': _case('dw', 32, 32, 9, 11, 3, 3, join_i32=True),
}

# ---- grouped: always the dense expansion, on both values of `grouped`
GROUPED = {'g_c32_cg4_d2': _case('grouped', 32, 32, 9, 11, 2, 2)}

# planned for 8 images, run with 3 (parts of 2 and 1) and then 8 from the same handle
MAX_BATCH = {'mb_plain': _case('plain', 40, 72, 9, 11, 2, 2, 2, N=8, max_batch=8), 'mb_dw': _case('dw', 40, 40, 9, 11, 2, 2, N=8, max_batch=8)}

# dilated 3x3 / 1 d2 -> dilated 3x3 d4 (it reads the first one's result at fraclen 4, shift 9) on a 14 x 14 map, N = 3, bench.py's schedule
PIPELINED = {'pl_plain': _case('plain', 64, 64, 14, 14, 2, 2, readers=[(3, False)], opts=dict(_IR_PIPELINED['opts']),
                               second=dict(stride=1, d=4, pad=4, in_fl=4, w_fl=5)),
             'pl_dw': _case('dw', 64, 64, 14, 14, 2, 2, readers=[(3, False)], opts=dict(_IR_PIPELINED['opts']),
                            second=dict(stride=1, d=4, pad=4, in_fl=4, w_fl=5))}

OP_CASES = dict(PLAIN, **PLAIN_FORMATS, **PLAIN_RES, **DW, **DW_GENERIC, **GROUPED)
ALL = dict(OP_CASES, **MAX_BATCH, **PIPELINED)


# ---- net level: the stuffed twins
def stuffed_twin(spec, params):
    """(spec, params) of the same net with every dilated conv replaced by its zero-stuffed plain twin, for oracle.net_forward."""
    import copy
    spec, params = copy.deepcopy(spec), dict(params)
    for c in spec.convs():
        if c.dilation > 1:
            params[c.key + '.weight'] = stuffed(np.asarray(params[c.key + '.weight']), c.dilation)
            c.k, c.dilation = c.dilation * (c.k - 1) + 1, 1
    return spec, params
