"""The one reference graph of the op-level tests, and the one walker of an IntGraph.  No test functions here.

`RefGraph` has one method per builder method of F8Net.  Every method evaluates the op on the CPU — the oracle's op-level functions where the oracle
has the op, tests/ref_ops.py where it has not — and keeps (value, fraclen) in `v[id]`; with record=True it also records the op into `net` (an F8Net),
with int_graph=ig it also appends the op's IntOp to ig, field for field what f8net_amd.onnx_import makes of the exported op.  What the case builders'
own data checks read: `taps` [(label, the int8 tensor a labelled conv reads, signed)], `raw[id]` (a conv's result before its ReLU), `ops[id]` (the
two operands of a mul in its formats), `idx[id]` / `srcv[id]` (a table's index tensor and its source).

`graph_forward` evaluates an IntGraph (every op kind onnx_import can produce) with the same references and holds the fraclen solver against them.
`oracle/` stays as it is."""
import numpy as np

import ref_ops
from f8net_amd.onnx_import import IntGraph, IntOp
from oracle import oracle


def _i8_source(x, fl, input_fl, input_signed, quant_input):
    """What a conv-like op reads: the source requantised to its input format, or — quant_input=False — as it is, already 8 bits in that format."""
    if quant_input:
        return oracle.requant(x, input_fl, fl, input_signed)
    assert fl == input_fl and x.min() >= (-127 if input_signed else 0) and x.max() <= (127 if input_signed else 255)
    return x


def _vec(y):
    return y.reshape(y.shape[0], y.shape[1], 1, 1)


class RefGraph:
    def __init__(self, x, x_fl, *, record=True, grouped=None, int_graph=None):
        """record=False: only the reference is evaluated, no handle is touched (tensor ids are counted here, the input is 0).  grouped: the handle's
        option of that name (which launch a grouped conv plans)."""
        self.record, self.ig = record, int_graph
        self.taps, self.raw, self.ops, self.idx, self.srcv = [], {}, {}, {}, {}
        self.net, t0, self._n = None, 0, 0
        if record:
            from f8net_amd.net import F8Net
            self.net = F8Net()
            t0 = self.net.input(x.shape[1], x.shape[2], x.shape[3], x_fl)
            if grouped is not None:
                self.net.set_option('grouped', grouped)
        self.v = {t0: (x, x_fl)}
        self.ids = {t0: 0}                                         # tensor id -> index of its op in the IntGraph

    @classmethod
    def on(cls, net, values):
        """A graph that goes on recording into an existing handle `net`, from its tensors {id: (reference value, fraclen)}."""
        g = cls(*next(iter(values.values())), record=False)
        g.record, g.net, g.v = True, net, dict(values)
        return g

    def _id(self, make):
        if self.record:
            return make()
        self._n += 1
        return self._n

    def _put(self, o, value, kind, **fields):
        """The op's result and, with an IntGraph, its IntOp (the fields' tensor ids are `_src`'s: indices into ig.ops)."""
        self.v[o] = value
        if self.ig is not None:
            self.ig.ops.append(IntOp(kind, **fields))
            self.ids[o] = len(self.ig.ops) - 1
        return o

    def _src(self, t):
        return self.ids[t] if self.ig is not None else None

    def _key(self, prefix):
        return f'{prefix}{len(self.ig.ops)}' if self.ig is not None else None

    # ---- convs
    def conv(self, t, w, b, *, stride=1, pad, groups, weight_fl, input_fl, input_signed, relu, label=None, quant_input=True, dilation=1, w_eval=None):
        """w_eval: other weights for the reference only (the liveness checks zero taps).  label: the conv's int8 source goes into `taps`."""
        o = self._id(lambda: self.net.conv(t, w, b, stride=stride, pad=pad, groups=groups, weight_fl=weight_fl, input_fl=input_fl,
                                           input_signed=input_signed, quant_input=quant_input, relu=relu, dilation=dilation))
        x, fl = self.v[t]
        xq = _i8_source(x, fl, input_fl, input_signed, quant_input)
        if label:
            self.taps.append((label, xq, input_signed))
        ws = ref_ops.stuffed(w if w_eval is None else w_eval, dilation)
        d, m = dilation, max(x.shape[2], x.shape[3]) - 1
        if d > 1 and w.shape[2] == 3 and pad == d and stride == 1 and m < d and groups == 1 and quant_input:
            # A 3x3 at dilation d, pad d, stride 1 on a map of at most m + 1 pixels a side, m < d: the taps further than m from the centre only ever
            # meet padding, so the stuffed (2d + 1)-square kernel cropped to its central (2m + 1) square, at pad m, is the same conv (ASPP's d = 18
            # on a 6 x 6 map: 11 x 11 taps instead of 37 x 37 for the reference to walk)
            y = oracle.conv2d(xq, np.ascontiguousarray(ws[:, :, d - m:d + m + 1, d - m:d + m + 1]), b, 1, m, 1)
        else:
            y = ref_ops.grouped_conv2d(xq, ws, b, stride, pad, groups)
        self.raw[o] = y
        return self._put(o, (oracle.relu(y) if relu else y, input_fl + weight_fl), 'conv', src=self._src(t), weight=np.asarray(w, np.int32),
                         bias=np.zeros(w.shape[0], np.int32) if b is None else np.asarray(b, np.int32), stride=stride, pad=pad, groups=groups,
                         kernel=w.shape[2], shift=(fl - input_fl) if quant_input else None, signed=input_signed, relu=relu,
                         key=self._key('layer'), dilation=dilation)

    def conv_transpose(self, t, w, b, *, stride, pad, output_padding=0, weight_fl, input_fl, input_signed, relu, quant_input=True, label=None, w_eval=None):
        o = self._id(lambda: self.net.conv_transpose(t, w, b, stride=stride, pad=pad, output_padding=output_padding, weight_fl=weight_fl, input_fl=input_fl,
                                                     input_signed=input_signed, quant_input=quant_input, relu=relu, label=label))
        x, fl = self.v[t]
        xq = _i8_source(x, fl, input_fl, input_signed, quant_input)
        y = ref_ops.deconv_ref(xq, w if w_eval is None else w_eval, b, stride, pad, output_padding)
        self.raw[o] = y
        return self._put(o, (oracle.relu(y) if relu else y, input_fl + weight_fl), 'deconv', src=self._src(t), weight=np.asarray(w, np.int32),
                         bias=np.zeros(w.shape[1], np.int32) if b is None else np.asarray(b, np.int32), stride=stride, pad=pad, kernel=w.shape[2],
                         shift=(fl - input_fl) if quant_input else None,
                         signed=input_signed, relu=relu, key=label or self._key('layer'),
                         output_padding=output_padding)

    def linear(self, t, w, b, *, weight_fl, input_fl, input_signed, label=None):
        o = self._id(lambda: self.net.linear(t, w, b, weight_fl=weight_fl, input_fl=input_fl, input_signed=input_signed, quant_input=True, label=label))
        x, fl = self.v[t]
        y = oracle.linear(oracle.requant(x.reshape(x.shape[0], -1), input_fl, fl, input_signed), w, b)
        return self._put(o, (_vec(y), input_fl + weight_fl), 'linear', src=self._src(t), weight=np.asarray(w, np.int32),
                         bias=np.zeros(w.shape[0], np.int32) if b is None else np.asarray(b, np.int32), shift=fl - input_fl, signed=input_signed, key=label or self._key('fc'))

    # ---- joins
    def add(self, a, b, relu=False):
        o = self._id(lambda: self.net.add(a, b, relu=relu))
        (xa, fa), (xb, fb) = self.v[a], self.v[b]
        y, fl = oracle.add_align(xa, xb, fa, fb)
        s, s2 = (a, b) if fa <= fb else (b, a)                    # src is the operand that shifts
        return self._put(o, (oracle.relu(y) if relu else y, fl), 'add', src=self._src(s), src2=self._src(s2), shift=abs(fa - fb), relu=relu, swap=s == b)

    def concat(self, ts, label=None):
        o = self._id(lambda: self.net.concat(ts, label=label))
        y, fl = ref_ops.concat_align([self.v[t][0] for t in ts], [self.v[t][1] for t in ts])
        return self._put(o, (y, fl), 'concat', src=self._src(ts[0]), srcs=[self._src(t) for t in ts], shifts=[fl - self.v[t][1] for t in ts])

    # ---- pools and upsample
    def maxpool(self, t, k, stride, pad):
        o = self._id(lambda: self.net.maxpool(t, k, stride, pad))
        return self._put(o, (oracle.maxpool(self.v[t][0], k, stride, pad), self.v[t][1]), 'maxpool', src=self._src(t), kernel=k, stride=stride, pad=pad)

    def avgpool_sum(self, t, shift=oracle.AVGPOOL_SHIFT):
        o = self._id(lambda: self.net.avgpool_sum(t, shift))
        return self._put(o, (_vec(oracle.avgpool_sum(self.v[t][0])), self.v[t][1] + shift), 'avgpool', src=self._src(t))

    def avgpool(self, t, k, stride=None, pad=0, shift=None, label=None):
        stride = k if stride is None else stride
        o = self._id(lambda: self.net.avgpool(t, k, stride, pad, shift, label=label))
        return self._put(o, ref_ops.sumpool_ref(self.v[t][0], self.v[t][1], k, stride, pad, shift), 'avgpool2d', src=self._src(t), kernel=k, stride=stride,
                         pad=pad, shift=ref_ops.default_shift(k) if shift is None else shift)

    def adaptive_avgpool(self, t, bins, label=None):
        k = self.v[t][0].shape[2] // bins
        o = self._id(lambda: self.net.adaptive_avgpool(t, bins, label=label))
        return self._put(o, ref_ops.sumpool_ref(self.v[t][0], self.v[t][1], k, k, 0), 'avgpool2d', src=self._src(t), kernel=k, stride=k, pad=0,
                         shift=ref_ops.default_shift(k))

    def upsample(self, t, scale, mode='nearest', label=None):
        o = self._id(lambda: self.net.upsample(t, scale, mode, label=label))
        return self._put(o, ref_ops.upsample_ref(self.v[t][0], self.v[t][1], scale, mode), 'upsample', src=self._src(t), mode=mode,
                         scale=(scale, scale) if isinstance(scale, int) else tuple(scale))

    # ---- channel maps
    def slice(self, t, start, stop, label=None):
        o = self._id(lambda: self.net.slice(t, start, stop, label=label))
        return self._put(o, (ref_ops.channel_slice(self.v[t][0], start, stop - start), self.v[t][1]), 'slice', src=self._src(t), first=start,
                         channels=stop - start)

    def split(self, t, sizes):
        firsts = np.cumsum([0] + list(sizes))
        return [self.slice(t, int(a), int(a + n)) for a, n in zip(firsts, sizes)]

    def channel_shuffle(self, t, groups, label=None):
        o = self._id(lambda: self.net.channel_shuffle(t, groups, label=label))
        return self._put(o, (ref_ops.channel_shuffle(self.v[t][0], groups), self.v[t][1]), 'shuffle', src=self._src(t), groups=groups)

    # ---- pointwise
    def mul(self, a, b, *, a_fl, a_signed, b_fl, b_signed=False, relu=False, label=None):
        o = self._id(lambda: self.net.mul(a, b, a_fl=a_fl, a_signed=a_signed, b_fl=b_fl, b_signed=b_signed, relu=relu, label=label))
        (xa, fa), (xb, fb) = self.v[a], self.v[b]
        self.ops[o] = ref_ops.mul_operands(xa, fa, xb, fb, a_fl, a_signed, b_fl, b_signed)
        return self._put(o, ref_ops.mul_ref(xa, fa, xb, fb, a_fl=a_fl, a_signed=a_signed, b_fl=b_fl, b_signed=b_signed, relu=relu), 'mul',
                         src=self._src(a), src2=self._src(b), shifts=[fa - a_fl, fb - b_fl], signed=a_signed, signed2=b_signed, relu=relu)

    def hard_gate(self, t, label=None):
        o = self._id(lambda: self.net.hard_gate(t, label=label))
        x, fl = self.v[t]
        return self._put(o, (ref_ops.hard_gate_ref(x, fl), fl), 'hgate', src=self._src(t), shift=fl)

    def hard_swish(self, t, *, x_fl, x_signed, g_fl, label=None):
        return self.mul(t, self.hard_gate(t), a_fl=x_fl, a_signed=x_signed, b_fl=g_fl, b_signed=False, label=label)

    def table(self, t, table, *, in_fl, in_signed, out_fl, label=None):
        o = self._id(lambda: self.net.table(t, table, in_fl=in_fl, in_signed=in_signed, out_fl=out_fl, label=label))
        x, fl = self.srcv[o] = self.v[t]
        self.idx[o] = ref_ops.table_index(x, fl, in_fl=in_fl, in_signed=in_signed)
        return self._put(o, (ref_ops.table_ref(x, fl, table, in_fl=in_fl, in_signed=in_signed), out_fl), 'table', src=self._src(t), shift=fl - in_fl,
                         signed=in_signed, table=np.asarray(table, np.int32).copy(), in_fl=in_fl, out_fl=out_fl)

    def output(self, t, as_float=False):
        if self.record:
            self.net.output(t, as_float=as_float)


def record_int_graph(x, fl, build):
    """The graph that build(g, input id) -> output id draws on a RefGraph over input x, as an IntGraph.  Returns (IntGraph, the graph, output id)."""
    ig = IntGraph(input_signed=False)
    ig.ops.append(IntOp('input', shape=tuple(x.shape[1:])))
    g = RefGraph(x, fl, record=False, int_graph=ig)
    out = build(g, 0)
    ig.output = g.ids[out]
    ig.output_float = False
    return ig, g, out


def graph_forward(ig, x, input_fraclen=None):
    """The integer result of an IntGraph on input x, every op kind onnx_import can produce, each with the reference RefGraph uses; the fraclen the
    solver gives an op is held against the reference's at every op."""
    V, layer = ig.solve_fraclens(input_fraclen)
    t = {}
    for i, o in enumerate(ig.ops):
        fl = V[i]
        if o.kind == 'input':
            t[i] = np.ascontiguousarray(x, dtype=np.int32)
        elif o.kind in ('conv', 'deconv', 'linear'):
            s = t[o.src]
            if o.shift is not None:
                s = oracle.requant(s, layer[i][0], V[o.src], o.signed)
            if o.kind == 'conv':
                y = ref_ops.grouped_conv2d(s, ref_ops.stuffed(o.weight, o.dilation), o.bias, o.stride, o.pad, o.groups)
            elif o.kind == 'deconv':
                y = ref_ops.deconv_ref(s, o.weight, o.bias, o.stride, o.pad, o.output_padding)
            else:
                y = _vec(oracle.linear(s.reshape(s.shape[0], -1), o.weight, o.bias))
            t[i] = oracle.relu(y) if o.relu else y
            fl = sum(layer[i])
        elif o.kind == 'add':
            y, fl = oracle.add_align(t[o.src], t[o.src2], V[o.src], V[o.src2])
            t[i] = oracle.relu(y) if o.relu else y
        elif o.kind == 'maxpool':
            t[i], fl = oracle.maxpool(t[o.src], o.kernel, o.stride, o.pad), V[o.src]
        elif o.kind == 'avgpool':
            t[i], fl = _vec(oracle.avgpool_sum(t[o.src])), V[o.src] + oracle.AVGPOOL_SHIFT
        elif o.kind == 'avgpool2d':
            t[i], fl = ref_ops.sumpool_ref(t[o.src], V[o.src], o.kernel, o.stride, o.pad, o.shift)
        elif o.kind == 'concat':
            t[i], fl = ref_ops.concat_align([t[s] for s in o.srcs], [V[s] for s in o.srcs])
            assert [V[i] - V[s] for s in o.srcs] == list(o.shifts)
        elif o.kind == 'upsample':
            t[i], fl = ref_ops.upsample_ref(t[o.src], V[o.src], tuple(o.scale), o.mode)
        elif o.kind == 'slice':
            t[i], fl = ref_ops.channel_slice(t[o.src], o.first, o.channels), V[o.src]
        elif o.kind == 'shuffle':
            t[i], fl = ref_ops.channel_shuffle(t[o.src], o.groups), V[o.src]
        elif o.kind == 'mul':
            t[i], fl = ref_ops.mul_ref(t[o.src], V[o.src], t[o.src2], V[o.src2], a_fl=V[o.src] - o.shifts[0], a_signed=o.signed,
                                       b_fl=V[o.src2] - o.shifts[1], b_signed=o.signed2, relu=o.relu)
        elif o.kind == 'hgate':
            assert V[o.src] == o.shift
            t[i], fl = ref_ops.hard_gate_ref(t[o.src], o.shift), o.shift
        elif o.kind == 'table':
            assert V[o.src] - o.in_fl == o.shift
            t[i], fl = ref_ops.table_ref(t[o.src], V[o.src], o.table, in_fl=o.in_fl, in_signed=o.signed), o.out_fl
        else:
            raise ValueError(o.kind)
        assert fl == V[i], (i, o.kind, fl, V[i])
    y = t[ig.output]
    return y.astype(np.float32) if ig.output_float else y
