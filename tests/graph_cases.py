"""What the op-case modules share (concat_cases, upsample_cases, deconv_cases, avgpool_cases, chanmap_cases): the launches of a plan by token, the
walker of an imported IntGraph, and the recorder that writes a module's `_Graph` into an IntGraph.  No test functions here.

`oracle/` stays as it is: `graph_forward` handles the ops the oracle's own walker does not know with the case modules' references (imported when
the walker runs: those modules import this one) and hands every other op kind to the oracle's op-level functions."""
import numpy as np

from f8net_amd.onnx_import import IntGraph, IntOp
from oracle import oracle


def launch_lines(net, prefix='', label=None):
    """[(launch index, plan token 'xyz:', kernel symbol)] of the handle's launches whose token starts with `prefix` (a string or a tuple of them)
    and, if given, whose tensor is labelled `label`, in launch order."""
    out = []
    for i in range(net.num_launches):
        tok, _, what = net.launch_info(i, 1)[0].partition(':')
        if tok.startswith(prefix) and label in (None, what):
            out.append((i, tok + ':', net.launch_kernel(i)))
    return out


def graph_forward(ig, x, input_fraclen=None):
    import avgpool_cases
    import concat_cases
    import deconv_cases
    import dil_cases
    import upsample_cases
    V, layer = ig.solve_fraclens(input_fraclen)
    t = {}
    for i, o in enumerate(ig.ops):
        fl = V[i]
        if o.kind == 'input':
            t[i] = np.ascontiguousarray(x, dtype=np.int32)
        elif o.kind in ('conv', 'deconv'):
            s = t[o.src]
            if o.shift is not None:
                s = oracle.requant(s, layer[i][0], V[o.src], o.signed)
            if o.kind == 'conv':
                y = oracle.conv2d(s, dil_cases.stuffed(o.weight, o.dilation), o.bias, o.stride, o.pad, o.groups)
            else:
                y = deconv_cases.deconv_ref(s, o.weight, o.bias, o.stride, o.pad, o.output_padding)
            t[i] = oracle.relu(y) if o.relu else y
        elif o.kind == 'add':
            y, fl = oracle.add_align(t[o.src], t[o.src2], V[o.src], V[o.src2])
            t[i] = oracle.relu(y) if o.relu else y
        elif o.kind == 'maxpool':
            t[i] = oracle.maxpool(t[o.src], o.kernel, o.stride, o.pad)
        elif o.kind == 'concat':
            t[i], fl = concat_cases.concat_align([t[s] for s in o.srcs], [V[s] for s in o.srcs])
            assert [V[i] - V[s] for s in o.srcs] == list(o.shifts)
        elif o.kind == 'upsample':
            t[i], fl = upsample_cases.upsample_ref(t[o.src], V[o.src], tuple(o.scale), o.mode)
        elif o.kind == 'avgpool2d':
            t[i], fl = avgpool_cases.sumpool_ref(t[o.src], V[o.src], o.kernel, o.stride, o.pad, o.shift)
        else:
            raise ValueError(o.kind)
        assert fl == V[i]
    return t[ig.output]


class Recorder:
    """In front of a module's `_Graph` (class Recorder(graph_cases.Recorder, _Graph)): a graph that evaluates the reference and writes every op into
    an IntGraph, op for op what the recording graph hands the library.  A module adds the methods of its own ops."""

    def __init__(self, x, fl, ig):
        super().__init__(x, fl, record=False)
        self.ig = ig
        self.ids = {0: 0}

    def _put(self, o, op):
        self.ig.ops.append(op)
        self.ids[o] = len(self.ig.ops) - 1
        return o

    def conv(self, t, w, b, *, stride=1, pad, groups, weight_fl, input_fl, input_signed, relu, label=None, quant_input=True, dilation=1, w_eval=None):
        o = super().conv(t, w, b, stride=stride, pad=pad, groups=groups, weight_fl=weight_fl, input_fl=input_fl, input_signed=input_signed, relu=relu,
                         quant_input=quant_input, dilation=dilation)
        return self._put(o, IntOp('conv', src=self.ids[t], weight=np.asarray(w, np.int32),
                                  bias=np.zeros(w.shape[0], np.int32) if b is None else np.asarray(b, np.int32), stride=stride, pad=pad, groups=groups,
                                  kernel=w.shape[2], shift=(self.v[t][1] - input_fl) if quant_input else None, signed=input_signed, relu=relu,
                                  key=f'layer{len(self.ig.ops)}', dilation=dilation))

    def add(self, a, b, relu=False):
        o = super().add(a, b, relu=relu)
        fa, fb = self.v[a][1], self.v[b][1]
        s, s2 = (a, b) if fa <= fb else (b, a)                    # src is the operand that shifts
        return self._put(o, IntOp('add', src=self.ids[s], src2=self.ids[s2], shift=abs(fa - fb), relu=relu, swap=s == b))

    def maxpool(self, t, k, stride, pad):
        return self._put(super().maxpool(t, k, stride, pad), IntOp('maxpool', src=self.ids[t], kernel=k, stride=stride, pad=pad))

    def concat(self, ts, label=None):
        o = super().concat(ts)
        fl = self.v[o][1]
        return self._put(o, IntOp('concat', src=self.ids[ts[0]], srcs=[self.ids[t] for t in ts], shifts=[fl - self.v[t][1] for t in ts]))

    def upsample(self, t, scale, mode='nearest', label=None):
        sc = (scale, scale) if isinstance(scale, int) else tuple(scale)
        return self._put(super().upsample(t, scale, mode), IntOp('upsample', src=self.ids[t], mode=mode, scale=sc))


def record_int_graph(recorder, x, fl, build):
    """The graph that build(g, input id) -> output id draws on a `recorder` over input x, as an IntGraph.  Returns (IntGraph, the graph, output id)."""
    ig = IntGraph(input_signed=False)
    ig.ops.append(IntOp('input', shape=tuple(x.shape[1:])))
    g = recorder(x, fl, ig)
    out = build(g, 0)
    ig.output = g.ids[out]
    ig.output_float = False
    return ig, g, out
