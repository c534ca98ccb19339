"""Importer for the reference's `int_op_only_model.onnx`.

`torch.onnx.export` of the reference IntModel (/root/reference/myutils/export.py:4-31, fix_train.py:948-954) traces
the integer forward into opset-11 primitives: the fraction lengths are Python ints at trace time, so what the file holds
is the *arithmetic* — every `int_op_only_fix_quant` (fix_quant_ops.py:90-114) appears as

    Add(S, 2^(n-1));  Mod(S, 2^n) == 2^(n-1);  Div(., 2^(n+1)) * 2;  Div(., 2^n);  Where;  Clip(lo, hi)     (n > 0)
    Mul(S, 2^-n);  Clip(lo, hi)                                                                              (n <= 0)

every residual join (fix_resnet.py:40-54) as `Clip(Add(Mul(A, 2^k), B), -(2^31-1), 2^31-1)`, the max-pool detour as
Cast-MaxPool-Cast, FXQAvgPool2d as two ReduceSums, the classifier as Gemm — with the int32 weights as initializers named
by their state_dict keys.  ONNX's integer `Div` truncates where the model's `>>` floors, so the file is a lossy picture
of the network for negative values; this importer does not execute it, it recognises the templates and rebuilds the
*PyTorch* semantics the file was traced from — the graph of conv / add / pool / linear nodes libf8net.so plans.

The absolute fraction lengths are not in the file (only their differences are: the shifts).  `IntGraph.solve_fraclens`
picks the least assignment that satisfies the reference's asserts (0 <= input_fraclen <= 8, resp. 7 signed;
fix_quant_ops.py:91-98) — any assignment with the same shifts computes the same integers, and the logits the
reference returns are raw integers (`.float()` without rescaling, fix_resnet.py:383).
"""
import re
from dataclasses import dataclass, field

import numpy as np

from . import onnx_io

I32_CLAMP = (1 << 31) - 1
AVGPOOL_SHIFT = 6      # FXQAvgPool2d(7).shiftnum, fix_quant_ops.py:121-122 (metadata only: absorbed by the next shift)


class OnnxImportError(ValueError):
    pass


# ------------------------------------------------------------------------------ the imported program

@dataclass
class IntOp:
    kind: str                      # input | conv | deconv | linear | add | maxpool | avgpool | avgpool2d | concat | upsample | slice | shuffle | d2s | s2d | mul | hgate | table
    src: int = -1                  # tensor id (index into IntGraph.ops)
    src2: int = -1                 # add: the operand that is NOT shifted; mul: operand b (of src's shape, or [C, 1, 1])
    weight: np.ndarray = None
    bias: np.ndarray = None
    stride: int = 1
    pad: int = 0
    groups: int = 1
    kernel: int = 0
    shift: int = None              # conv/linear: requant n (None = input already in format); add: k of `src << k`; avgpool2d: what the window's sum adds
                                   # to the fraction length (kernel, stride, pad: the window)
                                   # hgate: the source's fraction length fl itself (the file holds 3 * 2^fl); mul: unused (`shifts`)
    signed: bool = False           # conv/linear: clamp range of the requant (+-127 vs 0..255); mul: of operand a
    signed2: bool = False          # mul: clamp range of operand b's requant
    table: np.ndarray = None       # table: the 256 int32 entries (f8_net_table); `shift` is the requant n of the source, `signed` its clamp range
    in_fl: int = None              # table: the fraction length of the index format — with `shift` it pins the SOURCE's fraction length absolutely (in_fl + shift),
    out_fl: int = None             # table: ... and of the entries = of the result, pinned absolutely: the entries are constants of the graph, as a hard gate's 3 * 2^fl
    relu: bool = False
    swap: bool = False             # add: the shifted operand is the Add's second input (`res += x << k`) — cosmetic
    key: str = ''                  # state_dict key of the layer ('head.0', 'stage_0_layer_0.body.0', ...)
    shape: tuple = None            # input: (C, H, W)
    dilation: int = 1              # conv: spacing of the kernel's taps (ONNX `dilations`, both equal)
    srcs: list = None              # concat: the operands in channel order (tensor ids)
    shifts: list = None            # concat: k_i of `srcs[i] << k_i`, the alignment to the largest fraclen (the smallest is 0); mul: [n_a, n_b], the requant
                                   # shifts of the two operands
    mode: str = None               # upsample: 'nearest' | 'bilinear' (half-pixel centres; the result is the interpolated value times 4 scale^2)
    scale: tuple = None            # upsample: (scale_h, scale_w)
    first: int = 0                 # slice: the first channel
    channels: int = 0              # slice: how many; shuffle: the groups are in `groups`
    block: int = 0                 # d2s / s2d (depth_to_space / space_to_depth): the block size r
    order: str = None              # d2s / s2d: 'crd' | 'dcr' (include/f8net.h)
    output_padding: int = 0        # deconv (transposed conv; weight [cin, cout, k, k]): ONNX `output_padding`, both equal
    rect: tuple = None             # conv: None for a square kernel with one stride and one pad (`kernel`, `stride`, `pad`); else the rectangular geometry
                                   # (kh, kw, stride_h, stride_w, pad_top, pad_left, pad_bottom, pad_right) of f8_net_conv_rect, and those three are 0

    def conv_geometry(self):
        """(kh, kw, stride_h, stride_w, top, left, bottom, right) of a conv, rectangular or not."""
        return tuple(self.rect) if self.rect else (self.kernel, self.kernel, self.stride, self.stride) + (self.pad,) * 4


@dataclass
class IntGraph:
    ops: list = field(default_factory=list)
    output: int = -1
    output_float: bool = True
    input_signed: bool = False
    output_argmax: str = None      # None | 'u8' | 'i32': the graph's result is the channel argmax of tensor `output` (F8Net.output_argmax) in that index type

    def layer_keys(self):
        return [o.key for o in self.ops if o.kind in ('conv', 'deconv', 'linear')]

    # -- fraction lengths -------------------------------------------------------------------------------------------
    def solve_fraclens(self, input_fraclen=None):
        """Least fraction-length assignment consistent with the shifts.  Returns (V, layer) with V[t] = output_fraclen of
        tensor t and layer[t] = (input_fraclen, weight_fraclen) for conv / linear ops.

        Unknowns: V of every tensor.  With i_L = V[src_L] - n_L and w_L = V[out_L] - i_L the reference's invariants are
        difference constraints (0 <= i_L <= 8|7, 0 <= w_L <= 31, V[avgpool] <= 32, joins: V[b] = V[a] + k = V[out]);
        the least solution is the longest-path fixpoint from a zero node (Bellman-Ford)."""
        n = len(self.ops)
        ZERO = n
        edges = []                                   # (u, v, c): V[v] >= V[u] + c

        def ge(v, u, c):
            edges.append((u, v, c))

        def eq(v, u, c):                             # V[v] = V[u] + c
            ge(v, u, c)
            ge(u, v, -c)

        for t, o in enumerate(self.ops):
            if o.kind == 'input':
                if input_fraclen is None:
                    input_fraclen = 7 if self.input_signed else 8
                eq(t, ZERO, input_fraclen)
            elif o.kind in ('conv', 'deconv', 'linear'):
                lim = 7 if o.signed else 8
                if o.shift is None:                  # head conv: i = V[src]
                    ge(o.src, ZERO, 0)
                    ge(ZERO, o.src, -lim)
                    ge(t, o.src, 0)                  # w >= 0
                    ge(o.src, t, -31)                # w <= 31
                else:
                    ge(o.src, ZERO, o.shift)         # i >= 0
                    ge(ZERO, o.src, -(o.shift + lim))
                    ge(t, o.src, -o.shift)           # w = V[t] - V[src] + n >= 0
                    ge(o.src, t, o.shift - 31)
            elif o.kind == 'add':
                eq(o.src2, o.src, o.shift)
                eq(t, o.src2, 0)
            elif o.kind == 'concat':
                for s, k in zip(o.srcs, o.shifts):
                    eq(t, s, k)
            elif o.kind in ('maxpool', 'slice', 'shuffle', 'd2s', 's2d'):
                eq(t, o.src, 0)
            elif o.kind == 'hgate':                  # 3 * 2^fl is a constant of the graph: the source's fraction length is pinned absolutely
                if not 0 <= o.shift <= 28:
                    raise OnnxImportError(f'hard gate at fraction length {o.shift}: outside 0 .. 28 (f8_net_hard_gate)')
                eq(o.src, ZERO, o.shift)
                eq(t, o.src, 0)
            elif o.kind == 'table':                  # the entries are constants of the graph: both fraction lengths are pinned absolutely
                if not 0 <= o.in_fl <= (7 if o.signed else 8):
                    raise OnnxImportError(f'table: index format fraction length {o.in_fl} outside the 8-bit formats')
                if not 0 <= o.out_fl <= 38:
                    raise OnnxImportError(f'table: result fraction length {o.out_fl} outside 0 .. 38 (f8_net_table)')
                eq(o.src, ZERO, o.in_fl + o.shift)
                eq(t, ZERO, o.out_fl)
            elif o.kind == 'mul':
                # V[t] = a_fl + b_fl is a sum of two unknowns, no difference constraint — unless b's format is anchored: b is a hard gate's result, whose
                # fraction length is a constant, so b_fl is one and V[t] = V[a] - n_a + b_fl
                g = self.ops[o.src2]
                if g.kind not in ('hgate', 'table'):
                    raise OnnxImportError('Mul of two activations whose second operand is not a hard gate\'s result: its format is not anchored, so the '
                                          'product\'s fraction length (a sum of two unknowns) is no difference constraint')
                n_a, n_b = o.shifts
                b_fl = (g.shift if g.kind == 'hgate' else g.out_fl) - n_b      # (a table's result is anchored as a gate's: out_fl is a constant)
                if not 0 <= b_fl <= (7 if o.signed2 else 8):
                    raise OnnxImportError(f'Mul: the gate operand\'s format fraction length {b_fl} is outside the 8-bit formats')
                lim = 7 if o.signed else 8
                ge(o.src, ZERO, n_a)                 # a_fl = V[a] - n_a >= 0
                ge(ZERO, o.src, -(n_a + lim))
                eq(t, o.src, b_fl - n_a)
            elif o.kind == 'upsample':
                eq(t, o.src, 0 if o.mode == 'nearest' else upsample_fl_gain(o.scale))
                if o.mode != 'nearest':
                    ge(ZERO, t, -32)                 # f8_net_upsample: the bound of the average pool
            elif o.kind == 'avgpool2d':
                eq(t, o.src, o.shift)
                ge(ZERO, t, -32)                     # f8_net_avgpool_window: the same bound
            elif o.kind == 'avgpool':
                eq(t, o.src, AVGPOOL_SHIFT)
                ge(ZERO, t, -32)                     # fix_quant_ops.py:129
        V = [None] * (n + 1)
        V[ZERO] = 0
        for it in range(n + 2):
            changed = False
            for u, v, c in edges:
                if V[u] is not None and (V[v] is None or V[v] < V[u] + c):
                    V[v] = V[u] + c
                    changed = True
            if not changed:
                break
        else:
            raise OnnxImportError('no fraction-length assignment satisfies the shifts in this graph')
        if V[ZERO] != 0 or any(v is None for v in V):
            raise OnnxImportError('no fraction-length assignment satisfies the shifts in this graph')
        layer = {}
        for t, o in enumerate(self.ops):
            if o.kind in ('conv', 'deconv', 'linear'):
                i = V[o.src] - (o.shift or 0)
                layer[t] = (i, V[t] - i)
        return V[:n], layer

    def state_dict(self, input_fraclen=None):
        """Parameter dict keyed like the reference IntModel's state_dict (fix_quant_ops.py:705-713)."""
        _, layer = self.solve_fraclens(input_fraclen)
        sd = {}
        for t, o in enumerate(self.ops):
            if o.kind in ('conv', 'deconv', 'linear'):
                i, w = layer[t]
                sd[o.key + '.weight'] = o.weight
                sd[o.key + '.bias'] = o.bias
                sd[o.key + '.weight_fraclen'] = np.array(w, np.int32)
                sd[o.key + '.input_fraclen'] = np.array([i], np.int32)
        return sd

    # -- planning through the C ABI -----------------------------------------------------------------------------------
    def build_net(self, max_batch, hw=None, input_fraclen=None, options=None):
        """Record the graph through libf8net.so's builder and plan it (f8_net_finalize).
        options: {key: value} for f8_net_set_option, applied before planning (as net.build_net's)."""
        from .net import F8Net, accept_grouped
        V, layer = self.solve_fraclens(input_fraclen)
        net = F8Net()
        accept_grouped(net, [(o.weight.shape[1] * o.groups, o.groups) for o in self.ops if o.kind == 'conv'], options)
        ids = {}
        for t, o in enumerate(self.ops):
            if o.kind == 'input':
                C, H, W = o.shape
                if hw is not None:
                    H = W = hw
                ids[t] = net.input(C, H, W, V[t])
            elif o.kind == 'conv':
                i, w = layer[t]
                g = o.conv_geometry()
                ids[t] = net.conv(ids[o.src], o.weight, o.bias, stride=g[2:4] if o.rect else o.stride, pad=g[4:] if o.rect else o.pad, groups=o.groups,
                                  weight_fl=w, input_fl=i, input_signed=o.signed, quant_input=o.shift is not None,
                                  relu=o.relu, label=o.key, dilation=o.dilation)
            elif o.kind == 'deconv':
                i, w = layer[t]
                ids[t] = net.conv_transpose(ids[o.src], o.weight, o.bias, stride=o.stride, pad=o.pad, output_padding=o.output_padding,
                                            weight_fl=w, input_fl=i, input_signed=o.signed, quant_input=o.shift is not None,
                                            relu=o.relu, label=o.key)
            elif o.kind == 'linear':
                i, w = layer[t]
                ids[t] = net.linear(ids[o.src], o.weight, o.bias, weight_fl=w, input_fl=i, input_signed=o.signed,
                                    quant_input=o.shift is not None, label=o.key)
            elif o.kind == 'add':
                ids[t] = net.add(ids[o.src], ids[o.src2], relu=o.relu)
            elif o.kind == 'concat':                          # (the library aligns to the largest fraclen: V[t] = V[s] + k, min k = 0)
                ids[t] = net.concat([ids[s] for s in o.srcs])
            elif o.kind == 'maxpool':
                ids[t] = net.maxpool(ids[o.src], o.kernel, o.stride, o.pad)
            elif o.kind == 'upsample':
                ids[t] = net.upsample(ids[o.src], tuple(o.scale), o.mode)
            elif o.kind == 'slice':
                ids[t] = net.slice(ids[o.src], o.first, o.first + o.channels)
            elif o.kind == 'shuffle':
                ids[t] = net.channel_shuffle(ids[o.src], o.groups)
            elif o.kind == 'd2s':
                ids[t] = net.depth_to_space(ids[o.src], o.block, o.order)
            elif o.kind == 's2d':
                ids[t] = net.space_to_depth(ids[o.src], o.block, o.order)
            elif o.kind == 'hgate':
                ids[t] = net.hard_gate(ids[o.src])
            elif o.kind == 'table':
                ids[t] = net.table(ids[o.src], o.table, in_fl=o.in_fl, in_signed=o.signed, out_fl=o.out_fl)
            elif o.kind == 'mul':
                ids[t] = net.mul(ids[o.src], ids[o.src2], a_fl=V[o.src] - o.shifts[0], a_signed=o.signed, b_fl=V[o.src2] - o.shifts[1],
                                 b_signed=o.signed2, relu=o.relu)
            elif o.kind == 'avgpool2d':
                ids[t] = net.avgpool(ids[o.src], o.kernel, o.stride, o.pad, shift=o.shift)
            elif o.kind == 'avgpool':
                ids[t] = net.avgpool_sum(ids[o.src], AVGPOOL_SHIFT)
        if self.output_argmax:
            net.output_argmax(ids[self.output], self.output_argmax)
        else:
            net.output(ids[self.output], as_float=self.output_float)
        for k, v in (options or {}).items():
            net.set_option(k, v)
        return net.finalize(max_batch)


def _check_rect(wname, rect, dil, groups, cin):
    """What f8_net_conv_rect refuses, as an OnnxImportError that says which (include/f8net.h)."""
    kh, kw, sh, sw, pt, pl, pb, pr = rect
    what = f'kernel {kh}x{kw}, strides ({sh}, {sw}), pads [{pt}, {pl}, {pb}, {pr}], dilation {dil}'
    if not (1 <= kh <= 31 and 1 <= kw <= 31):
        raise OnnxImportError(f'Conv {wname}: rectangular kernel sides must be 1 .. 31 ({what})')
    if not 1 <= dil <= 64:
        raise OnnxImportError(f'Conv {wname}: dilation must be 1 .. 64 ({what})')
    eh, ew = dil * (kh - 1) + 1, dil * (kw - 1) + 1
    if pt >= eh or pb >= eh or pl >= ew or pr >= ew:
        raise OnnxImportError(f'Conv {wname}: a pad exceeds its axis\' extent - 1 = {eh - 1} rows / {ew - 1} columns ({what})')
    if 1 < groups < cin:
        raise OnnxImportError(f'Conv {wname}: grouped rectangular convs are not built (group {groups} of {cin} channels; {what})')
    if groups == cin and groups > 1:
        k = max(kh, kw)
        if not (min(kh, kw) == 1 and k >= 3 and dil == 1 and sh == sw and sh <= 2):
            raise OnnxImportError(f'Conv {wname}: rectangular depthwise convs are built for strips only: 1xk / kx1, 3 <= k <= 31, dilation 1, one '
                                  f'stride of 1 or 2 ({what})')


def tensor_shapes(ops):
    """[(C, H, W)] of every tensor of a list of IntOps (the shuffle's Reshape and an equal Split need the channel count and the map)."""
    out = []
    for o in ops:
        if o.kind == 'input':
            out.append(tuple(o.shape))
            continue
        C, H, W = out[o.src]
        if o.kind == 'conv':
            kh, kw, sh, sw, pt, pl, pb, pr = o.conv_geometry()
            out.append((o.weight.shape[0], (H + pt + pb - o.dilation * (kh - 1) - 1) // sh + 1, (W + pl + pr - o.dilation * (kw - 1) - 1) // sw + 1))
        elif o.kind == 'deconv':
            out.append((o.weight.shape[1], (H - 1) * o.stride - 2 * o.pad + o.kernel + o.output_padding, (W - 1) * o.stride - 2 * o.pad + o.kernel + o.output_padding))
        elif o.kind == 'linear':
            out.append((o.weight.shape[0], 1, 1))
        elif o.kind == 'concat':
            out.append((sum(out[s][0] for s in o.srcs), H, W))
        elif o.kind in ('maxpool', 'avgpool2d'):
            out.append((C, (H + 2 * o.pad - o.kernel) // o.stride + 1, (W + 2 * o.pad - o.kernel) // o.stride + 1))
        elif o.kind == 'upsample':
            out.append((C, H * o.scale[0], W * o.scale[1]))
        elif o.kind == 'avgpool':
            out.append((C, 1, 1))
        elif o.kind == 'slice':
            out.append((o.channels, H, W))
        elif o.kind == 'd2s':
            out.append((C // o.block ** 2, H * o.block, W * o.block))
        elif o.kind == 's2d':
            out.append((C * o.block ** 2, H // o.block, W // o.block))
        else:                                                        # add, shuffle, hgate, mul (operand a's shape)
            out.append((C, H, W))
    return out


def avgpool2d_shift(kernel):
    """FXQAvgPool2d(kernel).shiftnum = round(log2(kernel^2)) (fix_quant_ops.py:121-122): what a windowed average pool adds to the fraction length.
    Nothing in a file carries it (the consumer's shift absorbs it); any value computes the same integers."""
    import math
    return int(round(math.log2(kernel * kernel)))


def upsample_fl_gain(scale):
    """2k + 2 for a bilinear upsample by scale (2^k, 2^k): its integer weights sum to 4 scale^2 = 2^(2k + 2) (include/f8net.h)."""
    sh, sw = scale
    if sh != sw or sh not in (2, 4, 8, 16):
        raise OnnxImportError(f'bilinear upsample by {tuple(scale)}: only equal scales of 2, 4, 8 or 16')
    return 2 * (sh.bit_length() - 1) + 2


# ------------------------------------------------------------------------------ template recognition

def _pow2(c, what):
    c = int(c)
    if c <= 0 or c & (c - 1):
        raise OnnxImportError(f'{what}: {c} is not a power of two')
    return c.bit_length() - 1


def _match_requant(e):
    """expr -> (source tensor id, n, signed) for the int_op_only_fix_quant templates, or None for a bare tensor."""
    if e[0] == 'T':
        return None
    if e[0] != 'clip':
        raise OnnxImportError(f'conv input is not a requantised tensor: {e[0]}')
    _, body, lo, hi = e
    if (lo, hi) == (-127, 127):
        signed = True
    elif (lo, hi) == (0, 255):
        signed = False
    else:
        raise OnnxImportError(f'requant clamp [{lo},{hi}] is neither [-127,127] nor [0,255]')
    if body[0] == 'mul' and body[1][0] == 'T':                      # n <= 0: input << -n (fix_quant_ops.py:105-106)
        return body[1][1], -_pow2(body[2], 'left shift'), signed
    if body[0] != 'where':
        raise OnnxImportError(f'unrecognised requant body {body[0]}')
    _, cond, tie, reg = body
    try:
        (_, (_, src_m, M), h) = cond                                # eq(mod(S, 2^n), 2^(n-1))
        assert cond[0] == 'eq' and cond[1][0] == 'mod'
        (_, (_, (_, src_t, h1), D1), two) = tie                     # mul(div(addc(S, h), 2^(n+1)), 2)
        assert tie[0] == 'mul' and tie[1][0] == 'div' and tie[1][1][0] == 'addc'
        (_, (_, src_r, h2), D2) = reg                               # div(addc(S, h), 2^n)
        assert reg[0] == 'div' and reg[1][0] == 'addc'
    except (ValueError, AssertionError, TypeError, IndexError):
        raise OnnxImportError('unrecognised round-half-even template') from None
    n = _pow2(M, 'requant modulus')
    if not (src_m == src_t == src_r and src_m[0] == 'T'):
        raise OnnxImportError('round-half-even template reads different tensors')
    if n < 1 or not (h == h1 == h2 == 1 << (n - 1) and D1 == 1 << (n + 1) and D2 == 1 << n and two == 2):
        raise OnnxImportError(f'round-half-even constants inconsistent for n={n}')
    return src_m[1], n, signed


def _layer_key(weight_name):
    if not weight_name.endswith('.weight'):
        raise OnnxImportError(f'initializer {weight_name!r} is not named like a state_dict weight')
    return weight_name[:-len('.weight')]


def import_graph(model, input_signed=False) -> IntGraph:
    """model: path / bytes of an ONNX file exported from a reference IntModel.  input_signed: FLAGS.normalize of the run
    that exported it (the head conv's input is signed 8-bit then, fix_train.py:683-687; nothing in the file says so)."""
    g = model if isinstance(model, onnx_io.Graph) else onnx_io.load_graph(model)
    if len(g.inputs) != 1 or len(g.outputs) != 1:
        raise OnnxImportError('expected one graph input and one output')
    iname, _, idims = g.inputs[0]
    if len(idims) != 4 or not all(isinstance(d, int) for d in idims[1:]):
        raise OnnxImportError(f'graph input dims {idims}: expected [batch, C, H, W]')
    uses = {}
    for nd in g.nodes:
        for s in nd.inputs:
            uses[s] = uses.get(s, 0) + 1
    users = {}
    for nd in g.nodes:
        for s in nd.inputs:
            users.setdefault(s, []).append(nd)
    ig = IntGraph(input_signed=bool(input_signed))
    ig.ops.append(IntOp('input', shape=tuple(idims[1:])))
    val = {iname: ('T', 0)}                          # ONNX value name -> expr | ('const', python number | ndarray)
    for k, a in g.initializers.items():
        val[k] = ('init', k)

    def const(name, what):
        v = val.get(name)
        if v is None or v[0] != 'const':
            raise OnnxImportError(f'{what}: operand {name!r} is not a constant')
        c = v[1]
        if isinstance(c, np.ndarray):
            if c.size != 1:
                raise OnnxImportError(f'{what}: constant {name!r} is not a scalar')
            c = c.reshape(-1)[0]
        f = float(c)
        if f != int(f):
            raise OnnxImportError(f'{what}: constant {f} is not an integer')
        return int(f)

    def init(name, what):
        v = val.get(name)
        if v is None or v[0] != 'init':
            raise OnnxImportError(f'{what}: {name!r} is not an initializer')
        a = g.initializers[v[1]]
        if a is None:
            raise OnnxImportError(f'{what}: initializer {v[1]!r} has no payload (skeleton file: fill_initializers first)')
        return v[1], a

    def is_const(name):
        return val.get(name, ('?',))[0] == 'const'

    def int_list(name):
        """The integers of a constant or initializer operand, or None when it is neither (or absent)."""
        v = val.get(name) if name else None
        if v is None or v[0] not in ('const', 'init'):
            return None
        a = np.asarray(v[1] if v[0] == 'const' else g.initializers[v[1]]).reshape(-1)
        return [int(x) for x in a]

    def slice_op(src, first, channels, what):
        C = tensor_shapes(ig.ops)[src][0]
        if first < 0 or channels < 1 or first + channels > C:
            raise OnnxImportError(f'{what}: channels [{first}, {first + channels}) outside the tensor\'s {C}')
        ig.ops.append(IntOp('slice', src=src, first=first, channels=channels))
        return ('T', len(ig.ops) - 1)

    def requant_src(name, what):
        e = val.get(name)
        if e is None or e[0] in ('const', 'init', 'opaque'):
            raise OnnxImportError(f'{what}: input {name!r} is not an activation')
        m = _match_requant(e)
        return (e[1], None, False) if m is None else m

    for nd in g.nodes:
        op, out = nd.op, nd.outputs[0]
        a = nd.attrs
        if op == 'Constant':
            val[out] = ('const', a['value'])
        elif op == 'Identity':
            val[out] = val[nd.inputs[0]]
        elif op == 'ArgMax':
            # The class map: ArgMax over the channels as the graph's LAST node, alone (int64, returned as int32) or followed by one Cast to UINT8 / INT32 /
            # INT64 that is the output.  It is an output kind of the library, not a tensor: nothing else may read it.
            e = val.get(nd.inputs[0])
            if e is None or e[0] != 'T':
                raise OnnxImportError('ArgMax: its input is not a layer result')
            if a.get('axis', 0) != 1:
                raise OnnxImportError(f'ArgMax: axis {a.get("axis", 0)}; only the channel argmax (axis=1) is built')
            if a.get('select_last_index', 0) != 0:
                raise OnnxImportError('ArgMax: select_last_index=1; the smallest index wins a tie here')
            nxt = users.get(out, [])
            last = out == g.outputs[0][0] and not nxt
            cast = len(nxt) == 1 and nxt[0].op == 'Cast' and nxt[0].outputs[0] == g.outputs[0][0] and not users.get(nxt[0].outputs[0])
            if not (last or cast):
                raise OnnxImportError('ArgMax: its result feeds something other than the graph output (a class map is an output, not a tensor)')
            val[out] = ('argmax', e[1], 'i32')
        elif op in ('TopK', 'Softmax'):
            raise OnnxImportError(f'{op}: not built (top-k maps and softmax / confidence outputs; ArgMax(axis=1) is)')
        elif op == 'Cast' and val.get(nd.inputs[0], ('?',))[0] == 'argmax':
            if a['to'] not in (onnx_io.UINT8, onnx_io.INT32, onnx_io.INT64):
                raise OnnxImportError(f'Cast of an ArgMax to ONNX type {a["to"]}: UINT8, INT32 or INT64 (returned as int32)')
            val[out] = ('argmax', val[nd.inputs[0]][1], 'u8' if a['to'] == onnx_io.UINT8 else 'i32')
        elif op == 'Cast':
            v = val[nd.inputs[0]]
            val[out] = v                                           # integer-valued throughout: casts carry no arithmetic
            if out == g.outputs[0][0]:
                ig.output_float = a['to'] == onnx_io.FLOAT
        elif op == 'Pow':
            val[out] = ('const', float(const(nd.inputs[0], 'Pow')) ** const(nd.inputs[1], 'Pow'))
        elif op == 'Concat' and any(val.get(s, ('?',))[0] in ('T', 'mul') for s in nd.inputs):
            # torch.cat(dim=1) of activations; an operand at a smaller fraction length arrives as Mul(x, 2^k), the alignment of the residual join
            if a.get('axis') not in (1, -3):
                raise OnnxImportError(f'Concat of activations along axis {a.get("axis")}: only the channel axis (1)')
            srcs, shifts = [], []
            for s in nd.inputs:
                e = val.get(s, ('?',))
                if e[0] == 'T':
                    srcs.append(e[1])
                    shifts.append(0)
                elif e[0] == 'mul' and e[1][0] == 'T':
                    srcs.append(e[1][1])
                    shifts.append(_pow2(e[2], 'Concat operand scale'))
                else:
                    raise OnnxImportError(f'Concat operand {s!r} is neither a layer result nor one scaled by a power of two')
            if min(shifts) != 0:
                raise OnnxImportError('Concat: every operand is scaled (the result takes the largest operand fraction length)')
            ig.ops.append(IntOp('concat', src=srcs[0], srcs=srcs, shifts=shifts))
            val[out] = ('T', len(ig.ops) - 1)
        elif op == 'Resize':
            # nearest: Resize(x, roi, [1, 1, sh, sw]; nearest / asymmetric / floor).  bilinear: Resize(linear, half_pixel) and the Mul by 4 s^2 behind
            # it, which makes the values integers again — the pair is one op (the Mul branch below closes it)
            e = val.get(nd.inputs[0], ('?',))
            if e[0] != 'T':
                raise OnnxImportError('Resize: the input is not a layer result')
            if len(nd.inputs) > 3 and nd.inputs[3]:
                raise OnnxImportError('Resize with a `sizes` input: only constant integer scales')
            sc = val.get(nd.inputs[2]) if len(nd.inputs) > 2 else None
            if sc is None or sc[0] != 'const':
                raise OnnxImportError('Resize: the scales are not a constant')
            sc = np.asarray(sc[1], np.float64).reshape(-1)
            if sc.size != 4 or sc[0] != 1 or sc[1] != 1 or any(v != int(v) or v < 1 for v in sc[2:]):
                raise OnnxImportError(f'Resize scales {sc.tolist()}: expected [1, 1, sh, sw] with integer sh, sw >= 1')
            scale = (int(sc[2]), int(sc[3]))
            mode = a.get('mode', b'nearest').decode()
            ctm = a.get('coordinate_transformation_mode', b'half_pixel').decode()
            if mode == 'nearest':
                nm = a.get('nearest_mode', b'round_prefer_floor').decode()
                if ctm != 'asymmetric' or nm != 'floor':
                    raise OnnxImportError(f"Resize(nearest) with coordinate_transformation_mode {ctm!r}, nearest_mode {nm!r}: only 'asymmetric' / 'floor'")
                ig.ops.append(IntOp('upsample', src=e[1], mode='nearest', scale=scale))
                val[out] = ('T', len(ig.ops) - 1)
            elif mode == 'linear':
                if ctm not in ('half_pixel', 'pytorch_half_pixel'):
                    raise OnnxImportError(f"Resize(linear) with coordinate_transformation_mode {ctm!r}: only 'half_pixel' / 'pytorch_half_pixel'")
                gain = upsample_fl_gain(scale)
                nxt, name = users.get(out, []), out
                while len(nxt) == 1 and nxt[0].op == 'Cast':
                    name = nxt[0].outputs[0]
                    nxt = users.get(name, [])
                if len(nxt) != 1 or nxt[0].op != 'Mul':
                    raise OnnxImportError(f'Resize(linear) by {scale[0]} without the Mul by 2^{gain} behind it: its values are not integers')
                val[out] = ('resize_lin', e[1], scale, gain)
            else:
                raise OnnxImportError(f'Resize mode {mode!r}: only nearest and linear')
        elif op == 'Split' and val.get(nd.inputs[0], ('?',))[0] == 'T':
            # torch.split / torch.chunk along C: one slice per output.  Opset 11 carries the sizes as the attribute `split`, opset 13 as a second input
            src = val[nd.inputs[0]][1]
            if a.get('axis', 0) not in (1, -3):
                raise OnnxImportError(f'Split of an activation along axis {a.get("axis", 0)}: only the channel axis (1)')
            sizes = a.get('split') or (int_list(nd.inputs[1]) if len(nd.inputs) > 1 else None)
            C = tensor_shapes(ig.ops)[src][0]
            if not sizes:
                if C % len(nd.outputs):
                    raise OnnxImportError(f'Split of {C} channels into {len(nd.outputs)} equal parts')
                sizes = [C // len(nd.outputs)] * len(nd.outputs)
            if len(sizes) != len(nd.outputs) or sum(sizes) != C:
                raise OnnxImportError(f'Split sizes {list(sizes)} do not cover the {C} channels in {len(nd.outputs)} outputs')
            first = 0
            for o_name, n_ch in zip(nd.outputs, sizes):
                val[o_name] = slice_op(src, first, int(n_ch), 'Split')
                first += int(n_ch)
        elif op == 'Slice' and val.get(nd.inputs[0], ('?',))[0] == 'T':
            # x[:, a:b]: Slice(x, starts, ends, axes, steps) with constant operands, the channel axis, step 1
            src = val[nd.inputs[0]][1]
            starts, ends = int_list(nd.inputs[1]), int_list(nd.inputs[2])
            axes = int_list(nd.inputs[3]) if len(nd.inputs) > 3 else None
            steps = int_list(nd.inputs[4]) if len(nd.inputs) > 4 else [1]
            if starts is None or ends is None or (len(nd.inputs) > 3 and nd.inputs[3] and axes is None) or steps is None:
                raise OnnxImportError('Slice: starts / ends / axes / steps are not constants')
            if axes is None or len(axes) != 1 or axes[0] not in (1, -3) or len(starts) != 1 or len(ends) != 1:
                raise OnnxImportError(f'Slice of an activation along axes {axes}: only the channel axis (1)')
            if steps != [1]:
                raise OnnxImportError(f'Slice with steps {steps}: only step 1')
            C = tensor_shapes(ig.ops)[src][0]
            lo = starts[0] + C if starts[0] < 0 else starts[0]
            hi = min(ends[0] + C if ends[0] < 0 else ends[0], C)     # (torch writes `x[:, a:]` with ends = INT64_MAX)
            val[out] = slice_op(src, lo, hi - lo, 'Slice')
        elif op == 'Transpose':
            # the middle of torch's channel_shuffle: view(N, g, C / g, H, W).transpose(1, 2).reshape(N, C, H, W)
            e = val.get(nd.inputs[0], ('?',))
            if e[0] == 'reshape6':                                   # the middle of torch's pixel_unshuffle: view(N, C, H / r, r, W / r, r).permute(0, 1, 3, 5, 2, 4)
                if list(a.get('perm', [])) != [0, 1, 3, 5, 2, 4]:
                    raise OnnxImportError(f'Transpose of a 6-D view with perm {list(a.get("perm", []))}: only [0, 1, 3, 5, 2, 4] (space_to_depth in CRD order)')
                val[out] = ('s2d_t',) + e[1:]
            elif e[0] != 'reshape5':
                raise OnnxImportError('Transpose of something other than an activation reshaped to [N, groups, C / groups, H, W] or [N, C, H / r, r, W / r, r] '
                                      'by a Reshape with a constant shape')
            elif list(a.get('perm', [])) != [0, 2, 1, 3, 4]:
                raise OnnxImportError(f'Transpose with perm {list(a.get("perm", []))}: only [0, 2, 1, 3, 4] (the channel shuffle)')
            else:
                val[out] = ('shuffle_t',) + e[1:]
        elif op == 'Reshape' and val.get(nd.inputs[0], ('?',))[0] == 's2d_t':      # back to [N | 0 | -1, C r^2, H / r, W / r]
            e, shape = val[nd.inputs[0]], int_list(nd.inputs[1])
            C, H, W = tensor_shapes(ig.ops)[e[1]]
            r = e[2]
            if shape is None:
                raise OnnxImportError('Reshape behind the space_to_depth Transpose: its shape is missing or not a constant')
            if len(shape) != 4 or shape[1:] != [C * r * r, H // r, W // r]:
                raise OnnxImportError(f'Reshape behind the space_to_depth Transpose to {shape}: expected [N, {C * r * r}, {H // r}, {W // r}]')
            ig.ops.append(IntOp('s2d', src=e[1], block=r, order='crd'))
            val[out] = ('T', len(ig.ops) - 1)
        elif op == 'Reshape' and val.get(nd.inputs[0], ('?',))[0] == 'T' and int_list(nd.inputs[1]) is not None and len(int_list(nd.inputs[1])) == 6:
            # the head of torch's pixel_unshuffle: view(N, C, H / r, r, W / r, r)
            e, shape = val[nd.inputs[0]], int_list(nd.inputs[1])
            C, H, W = tensor_shapes(ig.ops)[e[1]]
            _, c6, h, ri, w_, rj = shape
            if c6 != C or ri < 2 or ri != rj or h * ri != H or w_ * rj != W:
                raise OnnxImportError(f'Reshape of a [{C}, {H}, {W}] activation to {shape}: a 6-D view must factor the map as [N, {C}, H / r, r, W / r, r]')
            val[out] = ('reshape6', e[1], ri)
        elif op == 'Reshape' and val.get(nd.inputs[0], ('?',))[0] in ('T', 'shuffle_t') and int_list(nd.inputs[1]) is not None and \
                len(int_list(nd.inputs[1])) in (4, 5):
            e, shape = val[nd.inputs[0]], int_list(nd.inputs[1])
            if e[0] == 'T':                                          # [N | 0 | -1, g, C / g, H, W]
                C, H, W = tensor_shapes(ig.ops)[e[1]]
                if len(shape) != 5:
                    raise OnnxImportError(f'Reshape of an activation to {shape}: only [N, groups, C / groups, H, W] (the channel shuffle)')
                _, gr, cg, h, w_ = shape
                if gr < 1 or cg < 1 or gr * cg != C or (h, w_) != (H, W):
                    raise OnnxImportError(f'Reshape of a [{C}, {H}, {W}] activation to {shape}: groups x (C / groups) must be {C} and the map {H} x {W}')
                val[out] = ('reshape5', e[1], gr)
            else:                                                    # back to [N | 0 | -1, C, H, W]
                C, H, W = tensor_shapes(ig.ops)[e[1]]
                if len(shape) != 4 or shape[1:] != [C, H, W]:
                    raise OnnxImportError(f'Reshape behind the shuffle\'s Transpose to {shape}: expected [N, {C}, {H}, {W}]')
                ig.ops.append(IntOp('shuffle', src=e[1], groups=e[2]))
                val[out] = ('T', len(ig.ops) - 1)
        elif op in ('DepthToSpace', 'SpaceToDepth') and val.get(nd.inputs[0], ('?',))[0] == 'T':
            src = val[nd.inputs[0]][1]
            C, H, W = tensor_shapes(ig.ops)[src]
            r = int(a.get('blocksize', 0))
            mode = a.get('mode', b'DCR')
            mode = (mode.decode() if isinstance(mode, bytes) else str(mode)) if op == 'DepthToSpace' else 'DCR'
            if mode not in ('DCR', 'CRD'):
                raise OnnxImportError(f'DepthToSpace mode {mode!r}: only DCR and CRD')
            if r < 2 or r > 16:
                raise OnnxImportError(f'{op} blocksize {r}: outside 2 .. 16 (f8_net_depth_to_space)')
            if op == 'DepthToSpace' and C % (r * r):
                raise OnnxImportError(f'DepthToSpace blocksize {r} on {C} channels: no multiple of {r * r}')
            if op == 'SpaceToDepth' and (H % r or W % r):
                raise OnnxImportError(f'SpaceToDepth blocksize {r} on a {H} x {W} map: no multiple of {r}')
            ig.ops.append(IntOp('d2s' if op == 'DepthToSpace' else 's2d', src=src, block=r, order=mode.lower()))
            val[out] = ('T', len(ig.ops) - 1)
        elif op == 'Unsqueeze' and val.get(nd.inputs[0], ('?',))[0] in ('T', 'clip'):
            val[out] = val[nd.inputs[0]]                           # a [N, C] gate vector lifted to [N, C, 1, 1] in front of a Mul: no arithmetic
        elif op == 'Gather' and val.get(nd.inputs[0], ('?',))[0] in ('init', 'T', 'clip'):
            # the table op: Gather(axis = 0) on a 256-entry int32 initializer, indexed by a requantised activation (+ 128 for a signed format).  The
            # initializer's NAME carries the two fraction lengths nothing else in the file states: `<any>.in_fl_<i>.out_fl_<o>` (onnx_export writes it)
            axis = a.get('axis', 0)
            if val[nd.inputs[0]][0] != 'init':
                raise OnnxImportError(f'Gather of an activation (axis {axis}): only a table lookup, Gather(table initializer, index), is imported')
            key, arr = init(nd.inputs[0], 'Gather')
            arr = np.asarray(arr)
            if axis != 0:
                raise OnnxImportError(f'Gather on initializer {key!r} along axis {axis}: a table lookup gathers along axis 0')
            if arr.shape != (256,) or arr.dtype != np.int32:
                raise OnnxImportError(f'Gather on initializer {key!r} of shape {tuple(arr.shape)} and type {arr.dtype}: a table is 256 int32 entries')
            m = re.fullmatch(r'.*\.in_fl_(\d+)\.out_fl_(\d+)', key)
            if not m:
                raise OnnxImportError(f'Gather on initializer {key!r}: the name does not end in .in_fl_<i>.out_fl_<o>, so the table\'s fraction lengths are unknown')
            e = val.get(nd.inputs[1], ('?',))
            offset = 0
            if e[0] == 'addc':
                offset, e = e[2], e[1]
            if e[0] != 'clip':
                raise OnnxImportError('Gather index is not a requantised activation (Clip to an 8-bit format [, Add 128])')
            src, n, signed = _match_requant(e)
            if offset != (128 if signed else 0):
                raise OnnxImportError(f'Gather index offset {offset} on a {"signed" if signed else "unsigned"} index: expected {128 if signed else 0}')
            ig.ops.append(IntOp('table', src=src, shift=n, signed=signed, table=arr.copy(), in_fl=int(m.group(1)), out_fl=int(m.group(2))))
            val[out] = ('T', len(ig.ops) - 1)
        elif op in ('Shape', 'Gather', 'Unsqueeze', 'Concat'):
            val[out] = ('opaque',)                                 # the `x.view(x.size(0), -1)` plumbing before the FC
        elif op == 'Reshape':
            val[out] = val[nd.inputs[0]]
        elif op in ('Add', 'Mul', 'Div', 'Mod', 'Equal'):
            x, y = nd.inputs
            if op in ('Add', 'Mul') and is_const(x) and not is_const(y):
                x, y = y, x
            if is_const(x) and is_const(y):
                cx, cy = const(x, op), const(y, op)
                val[out] = ('const', {'Add': cx + cy, 'Mul': cx * cy}.get(op))
                if val[out][1] is None:
                    raise OnnxImportError(f'{op} of two constants')
            elif is_const(y) and val.get(x, ('?',))[0] == 'avgpool_win':
                _, src, k, st, pad = val[x]
                if op != 'Mul' or const(y, op) != k * k:
                    raise OnnxImportError(f'AveragePool {k} x {k} must be followed by a Mul by {k}^2 = {k * k} (the window\'s sum)')
                ig.ops.append(IntOp('avgpool2d', src=src, kernel=k, stride=st, pad=pad, shift=avgpool2d_shift(k)))
                val[out] = ('T', len(ig.ops) - 1)
            elif is_const(y) and val.get(x, ('?',))[0] == 'resize_lin':
                _, src, scale, gain = val[x]
                if op != 'Mul' or const(y, op) != 1 << gain:
                    raise OnnxImportError(f'Resize(linear) by {scale[0]} must be followed by a Mul by 2^{gain} = {1 << gain}')
                ig.ops.append(IntOp('upsample', src=src, mode='bilinear', scale=scale))
                val[out] = ('T', len(ig.ops) - 1)
            elif is_const(y) and op == 'Add' and val.get(x, ('?',))[0] == 'clip' and val[x][1][0] == 'T':
                # the hard gate relu6(x + 3) in fixed point: Clip(x, -3 * 2^fl, 3 * 2^fl) then Add(3 * 2^fl)
                _, e, lo, hi = val[x]
                c = const(y, 'Add')
                if not (-lo == hi == c):
                    raise OnnxImportError(f'Clip [{lo}, {hi}] + {c} of an activation: a hard gate needs equal constants (Clip(x, -L, L) + L)')
                if hi <= 0 or hi % 3 or (hi // 3) & (hi // 3 - 1):
                    raise OnnxImportError(f'Clip(x, -{hi}, {hi}) + {hi} of an activation: a hard gate\'s constant is 3 * 2^fl, {hi} is not')
                ig.ops.append(IntOp('hgate', src=e[1], shift=(hi // 3).bit_length() - 1))
                val[out] = ('T', len(ig.ops) - 1)
            elif is_const(y):
                tag = {'Add': 'addc', 'Mul': 'mul', 'Div': 'div', 'Mod': 'mod', 'Equal': 'eq'}[op]
                val[out] = (tag, val[x], const(y, op))
            elif op == 'Add':
                val[out] = ('add', val[x], val[y])
            elif op == 'Mul':
                # the product of two activations, each behind its requantisation; the one that reads a hard gate's result is operand b
                ra, rb = requant_src(x, 'Mul'), requant_src(y, 'Mul')
                if ra[1] is None or rb[1] is None:
                    raise OnnxImportError('Mul of two activations that are not both requantised to 8-bit formats')
                if ig.ops[rb[0]].kind not in ('hgate', 'table') and ig.ops[ra[0]].kind in ('hgate', 'table'):
                    ra, rb = rb, ra
                if ig.ops[rb[0]].kind not in ('hgate', 'table'):
                    raise OnnxImportError('Mul of two activations of which none is a hard gate\'s result: no operand format is anchored, so the '
                                          'product\'s fraction length cannot be solved (only x * hard_gate(.) is imported)')
                ig.ops.append(IntOp('mul', src=ra[0], src2=rb[0], shifts=[ra[1], rb[1]], signed=ra[2], signed2=rb[2]))
                val[out] = ('T', len(ig.ops) - 1)
            else:
                raise OnnxImportError(f'{op} of two activations')
        elif op == 'Where':
            val[out] = ('where', val[nd.inputs[0]], val[nd.inputs[1]], val[nd.inputs[2]])
        elif op == 'Clip':
            lo, hi = const(nd.inputs[1], 'Clip'), const(nd.inputs[2], 'Clip')
            e = val[nd.inputs[0]]
            if e[0] == 'add':                                      # residual join, fix_resnet.py:40-54
                # the exporter stores clamp_(min=-(2^31-1), max=2^31-1) as float32 constants, which round to -+2^31
                if -lo not in (I32_CLAMP, I32_CLAMP + 1) or hi not in (I32_CLAMP, I32_CLAMP + 1):
                    raise OnnxImportError(f'residual clamp [{lo},{hi}]')
                l, r = e[1], e[2]
                swap = l[0] != 'mul'
                if swap:
                    l, r = r, l
                if l[0] != 'mul' or l[1][0] != 'T' or r[0] != 'T':
                    raise OnnxImportError('residual join is not Add(Mul(A, 2^k), B)')
                ig.ops.append(IntOp('add', src=l[1][1], src2=r[1], shift=_pow2(l[2], 'residual shift'), swap=swap))
                val[out] = ('T', len(ig.ops) - 1)
            else:
                val[out] = ('clip', e, lo, hi)
        elif op == 'Relu':
            e = val[nd.inputs[0]]
            if e[0] != 'T' or ig.ops[e[1]].kind not in ('conv', 'deconv', 'add', 'mul') or uses.get(nd.inputs[0], 0) != 1:
                raise OnnxImportError('Relu on something other than a single-use conv / join result')
            ig.ops[e[1]].relu = True                               # nn.ReLU(inplace=True) on the producer's tensor
            val[out] = e
        elif op == 'Conv':
            src, n, signed = requant_src(nd.inputs[0], 'Conv')
            wname, w = init(nd.inputs[1], 'Conv weight')
            b = init(nd.inputs[2], 'Conv bias')[1] if len(nd.inputs) > 2 else None
            w = np.array(w, np.int32)
            ap = a.get('auto_pad', b'NOTSET')
            if ap not in (b'NOTSET', 'NOTSET'):
                raise OnnxImportError(f'Conv {wname}: auto_pad {ap!r}: only explicit pads')
            k = [int(v) for v in a.get('kernel_shape', w.shape[2:])]
            pads, st = [int(v) for v in a.get('pads', [0, 0, 0, 0])], [int(v) for v in a.get('strides', [1, 1])]
            dil = [int(v) for v in a.get('dilations', [1, 1])]
            if len(k) != 2 or len(pads) != 4 or len(st) != 2 or len(dil) != 2:
                raise OnnxImportError(f'Conv {wname}: only 2-D convs (kernel_shape {k}, pads {pads}, strides {st}, dilations {dil})')
            # one dilation for both axes (f8_net_conv_rect): the axes whose kernel is > 1 must agree; an axis of one tap has no spacing ([d, 1] on a 3x1 is d)
            live = sorted({d for d, kk in zip(dil, k) if kk > 1})
            if len(live) > 1 or min(dil) < 1:
                raise OnnxImportError(f'Conv {wname}: only equal dilations on the axes with more than one tap (got dilations {dil}, kernel {k})')
            d1 = live[0] if live else 1
            groups = int(a.get('group', 1))
            if k[0] == k[1] and len(set(pads)) == 1 and st[0] == st[1]:
                geo = dict(stride=st[0], pad=pads[0], kernel=k[0])
            else:                                                   # ONNX pads: [top, left, bottom, right]
                geo = dict(stride=0, pad=0, kernel=0, rect=(k[0], k[1], st[0], st[1], pads[0], pads[1], pads[2], pads[3]))
                _check_rect(wname, geo['rect'], d1, groups, w.shape[1] * groups)
            ig.ops.append(IntOp('conv', src=src, weight=w,
                                bias=None if b is None else np.array(b, np.int32), groups=groups, shift=n, signed=signed,
                                key=_layer_key(wname), dilation=d1, **geo))
            if n is None:
                ig.ops[-1].signed = ig.input_signed
            val[out] = ('T', len(ig.ops) - 1)
        elif op == 'ConvTranspose':
            # nn.ConvTranspose2d on int32: W [cin, cout, k, k]; one stride, one pad and one output_padding for both axes.  What f8_net_conv_transpose
            # does not build is named, one error each
            src, n, signed = requant_src(nd.inputs[0], 'ConvTranspose')
            wname, w = init(nd.inputs[1], 'ConvTranspose weight')
            b = init(nd.inputs[2], 'ConvTranspose bias')[1] if len(nd.inputs) > 2 else None
            w = np.array(w, np.int32)
            if w.ndim != 4:
                raise OnnxImportError(f'ConvTranspose {wname}: weight of rank {w.ndim}, expected [cin, cout, k, k]')
            k = list(a.get('kernel_shape', w.shape[2:]))
            if len(k) != 2 or k[0] != k[1] or w.shape[2] != w.shape[3] or k[0] != w.shape[2]:
                raise OnnxImportError(f'ConvTranspose {wname}: non-square kernel {k} (weight {tuple(w.shape)})')
            ap = a.get('auto_pad', b'NOTSET')
            if (ap.decode() if isinstance(ap, bytes) else ap) != 'NOTSET':
                raise OnnxImportError(f'ConvTranspose {wname}: auto_pad {ap!r}: only explicit pads')
            if 'output_shape' in a:
                raise OnnxImportError(f'ConvTranspose {wname}: output_shape {list(a["output_shape"])}: only pads + output_padding')
            if a.get('group', 1) != 1:
                raise OnnxImportError(f'ConvTranspose {wname}: group {a.get("group")}: only group = 1')
            dil = list(a.get('dilations', [1, 1]))
            if any(d != 1 for d in dil):
                raise OnnxImportError(f'ConvTranspose {wname}: dilations {dil}: only 1')
            pads, st, opad = list(a.get('pads', [0, 0, 0, 0])), list(a.get('strides', [1, 1])), list(a.get('output_padding', [0, 0]))
            if len(set(pads)) != 1:
                raise OnnxImportError(f'ConvTranspose {wname}: asymmetric pads {pads}')
            if st[0] != st[1] or opad[0] != opad[1]:
                raise OnnxImportError(f'ConvTranspose {wname}: unequal strides {st} / output_padding {opad}')
            ig.ops.append(IntOp('deconv', src=src, weight=w, bias=None if b is None else np.array(b, np.int32), stride=int(st[0]),
                                pad=int(pads[0]), kernel=int(k[0]), shift=n, signed=signed, key=_layer_key(wname), output_padding=int(opad[0])))
            if n is None:
                ig.ops[-1].signed = ig.input_signed
            val[out] = ('T', len(ig.ops) - 1)
        elif op == 'Gemm':
            if a.get('transB', 0) != 1 or a.get('alpha', 1.0) != 1.0 or a.get('beta', 1.0) != 1.0:
                raise OnnxImportError('Gemm: expected x @ W^T + b')
            src, n, signed = requant_src(nd.inputs[0], 'Gemm')
            wname, w = init(nd.inputs[1], 'Gemm weight')
            b = init(nd.inputs[2], 'Gemm bias')[1] if len(nd.inputs) > 2 else None
            ig.ops.append(IntOp('linear', src=src, weight=np.array(w, np.int32),
                                bias=None if b is None else np.array(b, np.int32), shift=n, signed=signed,
                                key=_layer_key(wname)))
            val[out] = ('T', len(ig.ops) - 1)
        elif op == 'MaxPool':
            e = val[nd.inputs[0]]
            k, st, pads = a['kernel_shape'], a.get('strides', [1, 1]), a.get('pads', [0, 0, 0, 0])
            if e[0] != 'T' or k[0] != k[1] or st[0] != st[1] or len(set(pads)) != 1 or a.get('ceil_mode', 0):
                raise OnnxImportError('MaxPool: unsupported form')
            ig.ops.append(IntOp('maxpool', src=e[1], kernel=k[0], stride=st[0], pad=pads[0]))
            val[out] = ('T', len(ig.ops) - 1)
        elif op == 'AveragePool':
            # AveragePool(count_include_pad=1) and the Mul by k^2 behind it, which makes the values integers again (the window's sum): the pair is one
            # op (the Mul branch above closes it).  What f8_net_avgpool_window does not build is named, one error each
            e = val[nd.inputs[0]]
            if e[0] != 'T':
                raise OnnxImportError('AveragePool: the input is not a layer result')
            ap = a.get('auto_pad', b'NOTSET')
            if (ap.decode() if isinstance(ap, bytes) else ap) != 'NOTSET':
                raise OnnxImportError(f'AveragePool: auto_pad {ap!r}: only explicit pads')
            if a.get('ceil_mode', 0):
                raise OnnxImportError('AveragePool: ceil_mode=1 is not built (only floor)')
            k = list(a['kernel_shape'])
            st, pads = list(a.get('strides', [1] * len(k))), list(a.get('pads', [0] * 2 * len(k)))
            if len(k) != 2 or k[0] != k[1]:
                raise OnnxImportError(f'AveragePool: non-square kernel {k}')
            if len(st) != 2 or st[0] != st[1]:
                raise OnnxImportError(f'AveragePool: non-square strides {st}')
            if len(set(pads)) != 1:
                raise OnnxImportError(f'AveragePool: asymmetric pads {pads}')
            if not a.get('count_include_pad', 0) and pads[0] > 0:
                raise OnnxImportError(f'AveragePool: count_include_pad=0 with pad {pads[0]} > 0: the divisor would vary over the border')
            nxt, name = users.get(out, []), out
            while len(nxt) == 1 and nxt[0].op == 'Cast':
                name = nxt[0].outputs[0]
                nxt = users.get(name, [])
            if len(nxt) != 1 or nxt[0].op != 'Mul':
                raise OnnxImportError(f'AveragePool {k[0]} x {k[0]} without the Mul by {k[0] * k[0]} behind it: its values are not integers')
            val[out] = ('avgpool_win', e[1], int(k[0]), int(st[0]), int(pads[0]))
        elif op == 'ReduceSum':                                    # x.sum(-1).sum(-1), fix_quant_ops.py:130
            e = val[nd.inputs[0]]
            if a.get('axes') != [-1] or a.get('keepdims', 1) != 0:
                raise OnnxImportError('ReduceSum: expected axes=[-1], keepdims=0')
            if e[0] == 'T':
                val[out] = ('rsum', e)
            elif e[0] == 'rsum':
                ig.ops.append(IntOp('avgpool', src=e[1][1]))
                val[out] = ('T', len(ig.ops) - 1)
            else:
                raise OnnxImportError('ReduceSum: unsupported operand')
        else:
            raise OnnxImportError(f'unsupported ONNX op {op}')
    e = val.get(g.outputs[0][0])
    if e is not None and e[0] == 'argmax':
        ig.output, ig.output_argmax, ig.output_float = e[1], e[2], False
        return ig
    if e is None or e[0] != 'T':
        raise OnnxImportError('graph output is not a layer result')
    ig.output = e[1]
    return ig


def detect_arch(ig: IntGraph):
    """Name of the topology table entry whose layer keys this graph carries, or None.  A graph with dilated convs is the `_os16` / `_os8` form of
    that entry (topology.dilate) whose strides, pads and dilations it has — or none."""
    from . import topology
    keys = sorted(ig.layer_keys())
    geo = {o.key: (o.stride, o.pad, o.dilation) for o in ig.ops if o.kind == 'conv'}
    for arch in ('resnet18', 'resnet50', 'mobilenet_v1', 'mobilenet_v2'):
        if sorted(topology.get(arch).layer_keys()) != keys:
            continue
        if all(d == 1 for _, _, d in geo.values()):
            return arch
        for name in (f'{arch}_os16', f'{arch}_os8'):
            if all(geo[c.key] == (c.stride, c.pad, c.dilation) for c in topology.get(name).convs()):
                return name
    return None


def int_model_from_onnx(model, normalize=False, input_fraclen=None):
    """ONNX file -> our IntModel (the module tree with the reference's state_dict keys) for one of the four nets.
    normalize / input_fraclen: FLAGS.normalize of the exporting run and its head.input_fraclen — with normalize the
    float image is scaled by 2^head.input_fraclen before it enters the net (fix_train.py:683-687), and that scale is
    not in the file (default 7; without normalize the input is u8 at fraclen 8, fix_train.py:689-692)."""
    from . import topology
    from .int_model import from_params
    ig = import_graph(model, input_signed=normalize)
    arch = detect_arch(ig)
    if arch is None:
        raise OnnxImportError('layer keys match none of resnet18 / resnet50 / mobilenet_v1 / mobilenet_v2; use '
                              'import_graph(...).build_net(...) for a free-form graph')
    return from_params(topology.get(arch, normalize=normalize), ig.state_dict(input_fraclen))
