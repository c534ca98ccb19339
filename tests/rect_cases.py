"""Case table, reference and graph builder of the tests of rectangular convolutions (f8_net_conv_rect / `F8Net.conv` with a [.., kh, kw] weight, a stride
pair and two or four pads): tests/test_rect_plan.py (the reference pinned to torch, acceptance, refusals, plan tokens, kernel symbols, the bias classes,
liveness on the reference; no GPU) and tests/test_gpu_rect.py (every case bit for bit on the device).  No test functions here.

The reference.  `oracle.conv2d` takes any kh x kw kernel with ONE stride and ONE pad, and stays as it is.  A rectangular conv is built from it:
requantise the source as RefGraph.conv does; np.pad it with zeros by (top, bottom) and (left, right); apply ref_ops.grouped_conv2d(., stuffed, b, 1, 0,
groups); subsample [:, :, ::sh, ::sw].  `stuffed` is ref_ops.stuffed for a square kernel; that function spreads a kernel over a SQUARE of d (K - 1) + 1
taps from its height alone, so a rectangular kernel is stuffed per axis here (stuffed_rect: zeros except at [::d, ::d] of a (d (kh - 1) + 1) x
(d (kw - 1) + 1) kernel — the same thing, axis by axis).  test_rect_plan.py pins the result to torch.nn.functional.conv2d(float64) behind F.pad with tuple
stride and dilation, which is exact here (|acc| << 2^53), and — for odd k and symmetric pads — to the kernel zero-embedded in the max(kh, kw) square
through oracle.conv2d, which is what a user of the library could run before this entry point existed.

Every op-level graph is  input -> the conv under test (it reads the net input as it is, quant_input = False) -> output, where the output is the conv's
int32 result itself (readers=None) or the sum of one 32-output 1x1 reader per (fraclen, signed) — plus the int32 result when `join_i32` is set.  `res`
cases put a 1x1 in front and join the conv with that 1x1's result, as a BasicBlock does (the add rides in the conv's epilogue); `second` chains a second
rectangular conv behind the first through nothing but its requantisation (1x7 -> 7x1).

Expected plan tokens and kernel symbols are WRITTEN BY HAND from label_conv_step / pick_conv_tile / conv_kernel_name / dwk_kernel_name; nothing here
asks the planner for them.  Small launches (fewer than 512 tiles, all of these): coutP 32 -> tile 128x32, else 64x64; bk 64 where the padded input
channels are a multiple of 64, else 32; seven K steps (kh kw Cs / bk) and more run the four-slot ring, fewer the two-slot one; the padding instance
wherever one of the four pads is > 0."""
import functools

import numpy as np

import ref_ops
from dil_cases import FUSE_ALL  # noqa: F401  (the graphs of test_gpu_rect.py plan with it)
from f8net_amd import synth
from ir_cases import PIPELINED_CASE as _IR_PIPELINED
from ir_cases import _b, _w
from oracle import oracle
from refgraph import RefGraph, _i8_source


# ---- the reference
def pads4(pad):
    """An int, (ph, pw) or (top, left, bottom, right) as (top, left, bottom, right)."""
    if isinstance(pad, (tuple, list)):
        return (pad[0], pad[1], pad[0], pad[1]) if len(pad) == 2 else tuple(pad)
    return (pad,) * 4


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def stuffed_rect(w, d):
    """[cout, cin / groups, kh, kw] -> the zero-stuffed kernel of the same conv at dilation 1, each axis spread by itself."""
    w = np.asarray(w)
    kh, kw = w.shape[2:]
    if kh == kw:
        return ref_ops.stuffed(w, d)
    if d == 1:
        return w
    s = np.zeros(w.shape[:2] + (d * (kh - 1) + 1, d * (kw - 1) + 1), w.dtype)
    s[:, :, ::d, ::d] = w
    return s


def rect_conv_ref(xq, w, b, stride, pads, groups, d=1):
    """The int32 result of the conv on the already requantised source xq."""
    (sh, sw), (t, l, bo, r) = pair(stride), pads4(pads)
    xp = np.pad(np.asarray(xq, np.int32), ((0, 0), (0, 0), (t, bo), (l, r)))
    y = ref_ops.grouped_conv2d(np.ascontiguousarray(xp), np.ascontiguousarray(stuffed_rect(w, d)), b, 1, 0, groups)
    return np.ascontiguousarray(y[:, :, ::sh, ::sw])


def out_size(n, k, stride, p0, p1, d):
    return (n + p0 + p1 - d * (k - 1) - 1) // stride + 1


class RectGraph(RefGraph):
    """RefGraph with `conv_rect`: the builder call with tuple arguments, the reference above, and the IntOp onnx_import makes of it."""

    def conv_rect(self, t, w, b, *, stride=1, pads, groups, weight_fl, input_fl, input_signed, relu, label=None, quant_input=True, dilation=1, w_eval=None):
        st, pd = pair(stride), pads4(pads)
        o = self._id(lambda: self.net.conv(t, w, b, stride=st, pad=pd, groups=groups, weight_fl=weight_fl, input_fl=input_fl, input_signed=input_signed,
                                           quant_input=quant_input, relu=relu, dilation=dilation, label=label))
        x, fl = self.v[t]
        xq = _i8_source(x, fl, input_fl, input_signed, quant_input)
        if label:
            self.taps.append((label, xq, input_signed))
        y = rect_conv_ref(xq, w if w_eval is None else w_eval, b, st, pd, groups, dilation)
        self.raw[o] = y
        kh, kw = w.shape[2:]
        square = kh == kw and st[0] == st[1] and len(set(pd)) == 1
        geo = dict(stride=st[0], pad=pd[0], kernel=kh) if square else dict(stride=0, pad=0, kernel=0, rect=(kh, kw) + st + pd)
        return self._put(o, (oracle.relu(y) if relu else y, input_fl + weight_fl), 'conv', src=self._src(t), weight=np.asarray(w, np.int32),
                         bias=np.zeros(w.shape[0], np.int32) if b is None else np.asarray(b, np.int32), groups=groups,
                         shift=(fl - input_fl) if quant_input else None, signed=input_signed, relu=relu, key=label or self._key('layer'),
                         dilation=1 if kh == kw == 1 else dilation, **geo)


def record_int_graph(x, fl, build):
    """refgraph.record_int_graph on a RectGraph: the graph that build(g, input id) -> output id draws, as an IntGraph.  Returns (IntGraph, graph, output id)."""
    from f8net_amd.onnx_import import IntGraph, IntOp
    ig = IntGraph(input_signed=False)
    ig.ops.append(IntOp('input', shape=tuple(x.shape[1:])))
    g = RectGraph(x, fl, record=False, int_graph=ig)
    out = build(g, 0)
    ig.output = g.ids[out]
    ig.output_float = False
    return ig, g, out


# ---- a case.  kind: 'plain' (groups 1) or 'dw' (groups = C = cout).  Geometry: H x W map, kernel kh x kw, pads (top, left, bottom, right), stride
# (sh, sw), dilation d; N images.  Formats as dil_cases: in_fl / in_signed (the net input's and the conv's), w_fl, relu, readers [(fraclen, signed)],
# join_i32, bias_big.  res: BasicBlock-style join (see the module text).  opts: planning options.  w_sig = None: 150 / sqrt(taps x input channels of
# one output), which fills the 8 bits behind the default shift of 9.
def _case(kind, C, cout, H, W, kh, kw, pads, stride=(1, 1), d=1, N=3, **kw_):
    c = dict(kind=kind, C=C, cout=cout, H=H, W=W, kh=kh, kw=kw, pads=pads4(pads), stride=pair(stride), d=d, N=N, in_fl=8, in_signed=False, w_fl=5, relu=True,
             readers=[(4, False)], join_i32=False, res=False, second=None, bias_big=False, w_sig=None, b_sig=2.0 ** 9, b_mean=2.0 ** 13, opts={})
    c.update(kw_)
    t, l, b, r = c['pads']
    assert out_size(H, kh, c['stride'][0], t, b, d) >= 1 and out_size(W, kw, c['stride'][1], l, r, d) >= 1, (H, W, kh, kw, pads)
    assert kind != 'dw' or (C == cout and min(kh, kw) == 1 and d == 1 and c['stride'][0] == c['stride'][1])
    return c


def groups_of(c):
    return 1 if c['kind'] == 'plain' else c['C']


def weights(c, seed=30, shape=None):
    cin_g = c['C'] // groups_of(c)
    kh, kw = shape or (c['kh'], c['kw'])
    sig = c['w_sig'] or 150.0 / (kh * kw * cin_g) ** 0.5
    return _w(seed, (c['cout'], cin_g, kh, kw), sig)


def centre_only(w):
    z = np.zeros_like(w)
    z[:, :, w.shape[2] // 2, w.shape[3] // 2] = w[:, :, w.shape[2] // 2, w.shape[3] // 2]
    return z


def biases(c, seed=40):
    bd = _b(seed, c['cout'], c['b_sig'], c['b_mean'])
    if c['bias_big']:                                            # next to 2^31: `v + 2^(n-1)` wraps in the reference's int32 arithmetic
        bd[3], bd[17] = 2 ** 31 - 50, 2 ** 31 - 2 ** 12
    return bd


def build_graph(case, x, record=True, centre=False):
    """Returns (graph, output tensor, [tensor ids of the rectangular convs]).  centre: the reference runs with every tap but the central one zeroed."""
    c = case
    g = RectGraph(x, c['in_fl'], record=record)
    t = next(iter(g.v))
    G = groups_of(c)
    w = weights(c)
    ev = centre_only(w) if centre else None
    if c['res']:                                                 # 1x1 (ReLU, int32 + int8) -> the conv at 'same' pads -> join with the 1x1's result, ReLU
        r = c['res']
        pre = g.conv(t, _w(20, (c['C'], c['C'], 1, 1), 150.0 / c['C'] ** 0.5), _b(21, c['C'], 2.0 ** 9, 2.0 ** 12), pad=0, groups=1, weight_fl=r['pre_w_fl'],
                     input_fl=c['in_fl'], input_signed=c['in_signed'], relu=True, quant_input=False)
        d = g.conv_rect(pre, w, biases(c), stride=c['stride'], pads=c['pads'], groups=G, weight_fl=c['w_fl'], input_fl=r['in_fl'], input_signed=False,
                        relu=False, dilation=c['d'], w_eval=ev, label='res_in')
        ids = [d]
        t = g.add(d, pre, relu=True)
    else:
        d = g.conv_rect(t, w, biases(c), stride=c['stride'], pads=c['pads'], groups=G, weight_fl=c['w_fl'], input_fl=c['in_fl'],
                        input_signed=c['in_signed'], relu=c['relu'], quant_input=False, dilation=c['d'], w_eval=ev)
        ids = [d]
        t = d
        if c['second']:                                          # -> a second rectangular conv that requantises the first one's result
            s = c['second']
            w2 = weights(c, 31, (s['kh'], s['kw']))
            t = g.conv_rect(t, w2, biases(c, 41), stride=1, pads=s['pads'], groups=G, weight_fl=s['w_fl'], input_fl=s['in_fl'], input_signed=False,
                            relu=True, w_eval=centre_only(w2) if centre else None, label='second_in')
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
    return synth.rand_uniform_int(5, f'rectx{name}', (n or c['N'], c['C'], c['H'], c['W']), -hi if c['in_signed'] else 0, hi).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(name, centre):
    case = ALL[name]
    return build_graph(case, make_input(name, case, case.get('max_batch')), record=False, centre=centre)


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


def igemm_symbol(bm, bn, bk, pad, res, ksteps):
    wpx = 4 if bm == 128 and bn <= 64 else 2
    return (f'f8::conv_igemm_kernel<{bm}, {bn}, {bk}, {wpx}, {4 // wpx}, {"true" if pad else "false"}, {"true" if res else "false"}, '
            f'{4 if ksteps >= 7 else 2}, false>')


def dw_symbol(k, dot4, stride, int8_only, signed):
    """dwstrip_dot4_kernel<ceil((k + 3) / 4)> under option dwk_dot4 for int8 forms only at stride 1; else the scalar kernel."""
    if dot4 and stride == 1 and int8_only:
        return f'f8::dwstrip_dot4_kernel<{(k + 6) // 4}>'
    return f'f8::dwconvk_kernel<{"true" if signed else "false"}>'


def stride_token(st):
    return f'{st[0]}' if st[0] == st[1] else f'{st[0]}x{st[1]}'


def expect(case, dot4=True, tile=None):
    """[(plan token up to ':', kernel symbol)] of the case's rectangular convs, in launch order."""
    c = case
    geo = [(c['kh'], c['kw'], c['stride'], c['d'], c['pads'])]
    if c['second']:
        geo.append((c['second']['kh'], c['second']['kw'], (1, 1), 1, pads4(c['second']['pads'])))
    out = []
    for i, (kh, kw, st, d, pads) in enumerate(geo):
        if c['kind'] == 'dw':
            feeds_second = i == 0 and c['second']                 # read by the second conv only: one int8 form
            int8_only = bool(feeds_second or (c['readers'] and not c['join_i32']))
            out.append((f'dwconv{kh}x{kw}s{st[0]}:', dw_symbol(max(kh, kw), dot4, st[0], int8_only, c['in_signed'] and i == 0)))
            continue
        bm, bn, bk = tile or igemm_tile(c)
        res = bool(c['res'])
        dl = f'd{d}' if d > 1 else ''
        out.append((f'conv{kh}x{kw}s{stride_token(st)}{dl}_t{bm}x{bn}x{bk}{"_res" if res else ""}:',
                    igemm_symbol(bm, bn, bk, any(pads), res, kh * kw * _cs(c['C']) // bk)))
    return out


def r_lines(net, case):
    """[(plan token, kernel symbol)] of the handle's launches of the case's rectangular convs, in launch order: the conv tokens of its kernel sizes."""
    heads = {f'conv{case["kh"]}x{case["kw"]}s{stride_token(case["stride"])}'}
    if case['second']:
        heads.add(f'conv{case["second"]["kh"]}x{case["second"]["kw"]}s1')
    out = []
    for i in range(net.num_launches):
        tok = net.launch_info(i, 1)[0].split(':')[0] + ':'
        if any(tok.startswith(h) or tok.startswith('dw' + h) for h in heads):
            out.append((tok, net.launch_kernel(i)))
    return out


# ---- plain convs.  Defaults: unsigned fraclen-8 input, weights at 5, ReLU, one unsigned reader at fraclen 4 (shift 9); three images = sub-batches of 2 and 1
PLAIN = {
    'p_1x7_9x11': _case('plain', 32, 32, 9, 11, 1, 7, (0, 3, 0, 3)),
    'p_1x7_14x14_c40': _case('plain', 40, 72, 14, 14, 1, 7, (0, 3, 0, 3)),
    'p_7x1_9x11': _case('plain', 64, 128, 9, 11, 7, 1, (3, 0, 3, 0)),                           # 9 rows under 7 taps: every row class but one loses taps
    'p_7x1_5x35_rows_shorter_than_k': _case('plain', 40, 72, 5, 35, 7, 1, (3, 0, 3, 0)),           # H < kh: no row sees all taps
    'p_1x3_pad': _case('plain', 32, 32, 8, 8, 1, 3, (0, 1, 0, 1)),
    'p_1x3_nopad': _case('plain', 40, 72, 9, 11, 1, 3, 0),                                       # -> 9 x 9, no padding instance
    'p_3x1_pad': _case('plain', 64, 128, 14, 14, 3, 1, (1, 0, 1, 0)),
    'p_3x1_nopad': _case('plain', 32, 32, 5, 35, 3, 1, 0),                                       # -> 3 x 35
    'p_3x1_d2': _case('plain', 40, 72, 14, 14, 3, 1, (2, 0, 2, 0), d=2),
    'p_3x1_d6_9x11_rows_lose_both_outer_taps': _case('plain', 32, 32, 9, 11, 3, 1, (6, 0, 6, 0), d=6),      # H <= 2 d: masks 010, 011, 110
    'p_1x3_d2_5x35': _case('plain', 64, 128, 5, 35, 1, 3, (0, 2, 0, 2), d=2),
    'p_3x5_s2x1': _case('plain', 40, 72, 9, 11, 3, 5, (1, 2, 1, 2), stride=(2, 1)),              # -> 5 x 11
    'p_3x5_s1x2': _case('plain', 32, 32, 14, 14, 3, 5, (1, 2, 1, 2), stride=(1, 2)),             # -> 14 x 7
    'p_3x5_s1x2_5x35': _case('plain', 64, 128, 5, 35, 3, 5, (1, 2, 1, 2), stride=(1, 2)),        # -> 5 x 18
    'p_2x4_asymmetric': _case('plain', 40, 72, 9, 11, 2, 4, (0, 1, 1, 2)),                       # even sides, four different pads -> 9 x 11
    'p_3x3_s2_same_8x8': _case('plain', 32, 32, 8, 8, 3, 3, (0, 0, 1, 1), stride=2),             # TF 'SAME' at stride 2 on an even map -> 4 x 4
    'p_3x3_s2_same_9x11': _case('plain', 64, 128, 9, 11, 3, 3, (1, 1, 0, 0), stride=2),          # leading pads only -> 4 x 5
    'p_1x15_5x35': _case('plain', 32, 32, 5, 35, 1, 15, (0, 7, 0, 7)),
    'p_1x1_s2x1': _case('plain', 40, 72, 9, 11, 1, 1, 0, stride=(2, 1)),                         # CRNN-style: only the strides differ -> 5 x 11
}
_SGN = dict(in_fl=7, in_signed=True, b_mean=0.0, b_sig=2.0 ** 11)
PLAIN_FORMATS = {
    'pf_signed_in_1x7': _case('plain', 40, 72, 9, 11, 1, 7, (0, 3, 0, 3), relu=False, readers=[(4, True)], **_SGN),     # a real zero pad, one bias class
    'pf_signed_in_2x4': _case('plain', 32, 32, 9, 11, 2, 4, (0, 1, 1, 2), readers=[(3, False)], **dict(_SGN, b_mean=2.0 ** 12)),
    'pf_no_relu': _case('plain', 64, 128, 9, 11, 7, 1, (3, 0, 3, 0), relu=False, readers=[(3, True)], b_mean=-2.0 ** 13, b_sig=2.0 ** 12),
    'pf_two_readers': _case('plain', 40, 72, 9, 11, 3, 5, (1, 2, 1, 2), stride=(2, 1), readers=[(4, False), (3, False)]),
    'pf_mixed_readers': _case('plain', 32, 32, 8, 8, 3, 3, (0, 0, 1, 1), stride=2, readers=[(4, False), (3, True)]),
    'pf_i32_only': _case('plain', 64, 128, 9, 11, 1, 7, (0, 3, 0, 3), readers=None),
    'pf_i32_only_3x1_d2': _case('plain', 32, 32, 9, 11, 3, 1, (2, 0, 2, 0), d=2, readers=None, relu=False),
    'pf_i32_and_i8': _case('plain', 32, 32, 9, 11, 7, 1, (3, 0, 3, 0), join_i32=True),              # (the join with the readers' 32 channels: cout 32)
    'pf_bias_big': _case('plain', 32, 32, 9, 11, 1, 7, (0, 3, 0, 3), bias_big=True),
    'pf_bias_big_2x4': _case('plain', 64, 128, 9, 11, 2, 4, (0, 1, 1, 2), bias_big=True),
    'pf_rq1': _case('plain', 40, 72, 9, 11, 1, 7, (0, 3, 0, 3), opts={'requant_float': 1}),
}
# the fused residual join: pre 1x1 at weight fraclen 5 (result at 13, ReLU) -> the conv reads it at fraclen 4 (shift 9), weights at 9 (result at 13 too:
# the two operands weigh the same) -> conv + pre, ReLU; the reader takes the sum at fraclen 4 (shift 9)
_RES = dict(pre_w_fl=5, in_fl=4)
PLAIN_RES = {
    'pr_1x7_14x14': _case('plain', 64, 64, 14, 14, 1, 7, (0, 3, 0, 3), res=_RES, w_fl=9),
    'pr_1x7_9x11_c40_i32_and_i8': _case('plain', 32, 32, 9, 11, 1, 7, (0, 3, 0, 3), res=_RES, w_fl=9, join_i32=True),
    'pr_3x1_d2_9x11': _case('plain', 40, 40, 9, 11, 3, 1, (2, 0, 2, 0), d=2, res=_RES, w_fl=9),
}
# igemm_tile 1 .. 4 on one case: 128x128 / 128x64 / 64x128 / 64x64 (all admissible at coutP 128)
TILE_CASE = 'p_7x1_9x11'
TILES = {1: (128, 128, 64), 2: (128, 64, 64), 3: (64, 128, 64), 4: (64, 64, 64)}

# ---- depthwise strips: both orientations of k = 3, 7, 11, 21; C = 32, 40, 96.  The dot4 kernel gives a thread 8 consecutive outputs o0 .. o0 + 7 (o0 a
# multiple of 8); output o reads inputs o - pad .. o - pad + k - 1 and its alignment phase is o % 4.  Next to the LEADING border (outputs that lose taps
# there: o < pad) all four phases occur wherever pad >= 4: d_1x11_full_pad (pad 5), d_21x1_full_pad, d_1x21_5x35 (pad 10), d_7x1_pad3_1 only phases
# 0 .. 2.  Next to the TRAILING border (outputs o > L - 1 + pad - (k - 1), the last of them L_out - 1) the phases depend on L_out % 4: L_out = 11
# (d_1x11_full_pad, d_1x7_full_pad: phases 3, 0, 1, 2 of outputs 7 .. 10 — the last three in a second, partly empty run), 35 (d_1x21_5x35: outputs 25 .. 34,
# every phase), 9 (d_7x1_full_pad, d_21x1_full_pad: outputs 6 .. 8 and 0 .. 8), 14 (d_11x1_14x14: outputs 9 .. 13, every phase).
DW = {
    'd_1x3_full_pad': _case('dw', 32, 32, 9, 11, 1, 3, (0, 1, 0, 1)),
    'd_3x1_pad0': _case('dw', 40, 40, 9, 11, 3, 1, 0),                                          # -> 7 x 11
    'd_1x7_full_pad': _case('dw', 96, 96, 9, 11, 1, 7, (0, 3, 0, 3)),                             # 11 = 8 + 3: a second run with three live outputs
    'd_7x1_full_pad': _case('dw', 32, 32, 9, 11, 7, 1, (3, 0, 3, 0)),
    'd_1x7_9x3_axis_shorter_than_k': _case('dw', 32, 32, 9, 3, 1, 7, (0, 3, 0, 3)),               # W = 3 < 7: every output loses taps on both sides
    'd_7x1_pad3_1': _case('dw', 40, 40, 9, 11, 7, 1, (3, 0, 1, 0)),                               # unequal leading / trailing pads -> 7 x 11
    'd_1x7_pad1_3': _case('dw', 32, 32, 5, 35, 1, 7, (0, 1, 0, 3)),                               # -> 5 x 33
    'd_1x7_small_pad': _case('dw', 40, 40, 9, 11, 1, 7, (0, 1, 0, 1)),                            # the output shrinks -> 9 x 7
    'd_1x11_full_pad': _case('dw', 40, 40, 9, 11, 1, 11, (0, 5, 0, 5)),
    'd_11x1_14x14': _case('dw', 32, 32, 14, 14, 11, 1, (5, 0, 5, 0)),
    'd_11x1_pad0': _case('dw', 96, 96, 14, 14, 11, 1, 0),                                       # -> 4 x 14
    'd_1x21_5x35': _case('dw', 96, 96, 5, 35, 1, 21, (0, 10, 0, 10)),                             # 35 = 4 runs of 8 + 3
    'd_21x1_5x35_axis_shorter_than_k': _case('dw', 32, 32, 5, 35, 21, 1, (10, 0, 10, 0)),         # H = 5 < 21
    'd_21x1_full_pad': _case('dw', 40, 40, 9, 11, 21, 1, (10, 0, 10, 0)),
    'd_1x21_small_pad': _case('dw', 32, 32, 5, 35, 1, 21, (0, 4, 0, 2)),                          # -> 5 x 21
    'd_signed_in': _case('dw', 40, 40, 9, 11, 1, 7, (0, 3, 0, 3), relu=False, readers=[(4, True)], **_SGN),
    'd_two_readers': _case('dw', 32, 32, 9, 11, 11, 1, (5, 0, 5, 0), readers=[(4, False), (3, True)]),
    'd_bias_big': _case('dw', 32, 32, 9, 11, 1, 21, (0, 10, 0, 10), bias_big=True),
    'd_rq1': _case('dw', 40, 40, 9, 11, 7, 1, (3, 0, 3, 0), opts={'requant_float': 1}),
}
# the scalar kernel whatever dwk_dot4 says: stride 2, and the int32 form
DW_GENERIC = {
    'dg_s2_1x7': _case('dw', 40, 40, 9, 11, 1, 7, (0, 3, 0, 3), stride=2),                        # -> 5 x 6
    'dg_s2_21x1_14x14': _case('dw', 96, 96, 14, 14, 21, 1, (10, 0, 10, 0), stride=2),
    'dg_s2_11x1_signed': _case('dw', 32, 32, 9, 11, 11, 1, (5, 0, 3, 0), stride=2, relu=False, readers=[(4, True)], **_SGN),
    'dg_i32_only_1x11': _case('dw', 32, 32, 9, 11, 1, 11, (0, 5, 0, 5), readers=None),
    'dg_i32_and_i8_7x1': _case('dw', 32, 32, 9, 11, 7, 1, (3, 0, 3, 0), join_i32=True),
}

# planned for 8 images, run with 3 (parts of 2 and 1) and then 8 from the same handle
MAX_BATCH = {'mb_plain': _case('plain', 40, 72, 9, 11, 1, 7, (0, 3, 0, 3), N=8, max_batch=8),
             'mb_dw': _case('dw', 40, 40, 9, 11, 1, 11, (0, 5, 0, 5), N=8, max_batch=8)}

# 1x7 -> 7x1 (it reads the first one's result at fraclen 4, shift 9) on a 14 x 14 map, N = 3, bench.py's schedule
PIPELINED = {'pl_plain': _case('plain', 64, 64, 14, 14, 1, 7, (0, 3, 0, 3), readers=[(3, False)], opts=dict(_IR_PIPELINED['opts']),
                               second=dict(kh=7, kw=1, pads=(3, 0, 3, 0), in_fl=4, w_fl=5)),
             'pl_dw': _case('dw', 64, 64, 14, 14, 1, 7, (0, 3, 0, 3), readers=[(3, False)], opts=dict(_IR_PIPELINED['opts']),
                            second=dict(kh=7, kw=1, pads=(3, 0, 3, 0), in_fl=4, w_fl=5))}

OP_CASES = dict(PLAIN, **PLAIN_FORMATS, **PLAIN_RES, **DW, **DW_GENERIC)
ALL = dict(OP_CASES, **MAX_BATCH, **PIPELINED)

# every op case with more than one tap is held to the liveness caps of test_rect_plan.py (a 1x1 has no tap but the central one)
LIVENESS = sorted(k for k, c in OP_CASES.items() if c['kh'] * c['kw'] > 1)
