"""Writer for `int_op_only_model.onnx` files, the counterpart of the reference's
`onnx_export` (/root/reference/myutils/export.py:4-31, called from fix_train.py:948-954).

The reference gets its file by tracing the PyTorch IntModel with `torch.onnx.export(opset_version=11)`; here the same
opset-11 vocabulary is written directly from the integer graph — per op the node sequence the tracer produces:

    int_op_only_fix_quant, n > 0   Add, Mod(fmod=0), Cast(i64), Equal, Pow/Cast/Div, Pow/Cast/Mul, Pow/Cast/Div, Where,
                                   Clip(f32 bounds), Cast(i32)                      (fix_quant_ops.py:99-112)
    int_op_only_fix_quant, n <= 0  Pow/Cast/Mul, Clip, Cast(i32)                    (fix_quant_ops.py:105-112)
    conv / ReLU                    Conv(int32 W, B initializers), Relu, Cast(i32)
    transposed conv / ReLU         ConvTranspose(int32 W [cin, cout, k, k], B; strides, pads, output_padding), Relu, Cast(i32)
    residual join                  Pow/Cast/Mul, Add, Clip(-+2^31 as f32), Cast(i32) [, Relu, Cast]   (fix_resnet.py:40-54,77)
    head max-pool                  Cast(f32), MaxPool, Cast(i32)                     (fix_resnet.py:358-359)
    FXQAvgPool2d                   Cast(i64), ReduceSum(-1) x2, Cast(i32)            (fix_quant_ops.py:130-133)
    windowed average pool          Cast(f32), AveragePool(count_include_pad=1, ceil_mode=0), Mul(k^2), Cast(i32)
    channel concatenation          [Pow/Cast/Mul per operand at a smaller fraction length,] Concat(axis=1)
    channel slice                  Slice(starts [a], ends [b], axes [1], steps [1])
    channel shuffle                Reshape([-1, g, C / g, H, W]), Transpose(perm [0, 2, 1, 3, 4]), Reshape([-1, C, H, W])
    depth_to_space                 DepthToSpace(blocksize, mode DCR | CRD)
    space_to_depth, DCR            SpaceToDepth(blocksize)
    space_to_depth, CRD            Reshape([-1, C, H / r, r, W / r, r]), Transpose(perm [0, 1, 3, 5, 2, 4]), Reshape([-1, C r^2, H / r, W / r])  (torch's pixel_unshuffle)
    fixed-point product            the requant of each operand as in front of a conv, [Unsqueeze(axes [2, 3]) of a [N, C] gate vector,] Mul [, Relu]
    hard gate relu6(x + 3)         Clip(x, -3 * 2^fl, 3 * 2^fl), Add(3 * 2^fl)
    256-entry table                the requant of the source as in front of a conv, [Add(128) for a signed index,] Gather(axis=0) on a 256-entry int32
                                   initializer named `table_<t>.in_fl_<i>.out_fl_<o>` (the name carries the two fraction lengths)
    upsampling, nearest            Resize(nearest, asymmetric, floor; scales [1, 1, sh, sw])
    upsampling, bilinear           Cast(f32), Resize(linear, half_pixel; scales [1, 1, s, s]), Mul(4 s^2), Cast(i32)
    x.view(x.size(0), -1)          Shape, Gather, Unsqueeze, Concat, Reshape         (fix_resnet.py:371)
    classifier                     Gemm(transB=1), Cast(f32)                         (fix_resnet.py:383)
    class map (output_argmax)      ArgMax(axis=1, keepdims=0, select_last_index=0), Cast(u8 | i32): the graph's last nodes, in place of the output's Cast

Input `input` int32 [batch_size, C, H, W], output `output` float32 [batch_size, classes], dynamic batch axis, initializers
named by state_dict key — as in the reference's files, including the tracer's merging of the identical arithmetic when
two requants of the max-pool result share a shift (ResNet-50 `stage_0_layer_0`: body.0 and shortcut.0).  Node names differ.
"""
import numpy as np

from . import onnx_io, topology
from .onnx_import import AVGPOOL_SHIFT, IntGraph, IntOp, tensor_shapes
from .onnx_io import Node


def _fl(params, key, name):
    return int(np.asarray(params[f'{key}.{name}']).reshape(-1)[0])


def graph_from_params(spec: topology.NetSpec, params: dict, hw: int = 224) -> IntGraph:
    """The walk IntModel.forward does (fix_resnet.py:354-383, fix_mobilenet_v2.py:209-241, fix_mobilenet_v1.py:122-147)
    recorded as an IntGraph: shifts from the exported fraction lengths."""
    params = {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in params.items()}
    ig = IntGraph(input_signed=spec.normalize)
    ig.ops.append(IntOp('input', shape=(3, hw, hw)))
    fl = {0: _fl(params, spec.head.key, 'input_fraclen')}

    def conv(src, c, quant=True):
        i, w = _fl(params, c.key, 'input_fraclen'), _fl(params, c.key, 'weight_fraclen')
        ig.ops.append(IntOp('conv', src=src, weight=params[c.key + '.weight'].astype(np.int32),
                            bias=params[c.key + '.bias'].astype(np.int32), stride=c.stride, pad=c.pad, groups=c.groups,
                            kernel=c.k, shift=(fl[src] - i) if quant else None, signed=c.signed_in, relu=c.relu,
                            key=c.key, dilation=c.dilation))
        fl[len(ig.ops) - 1] = i + w
        return len(ig.ops) - 1

    def join(res, x, relu, ge):
        a, b = fl[res], fl[x]
        if a > b or (ge and a == b):                                # x << (a - b)   fix_resnet.py:43-44 / mbv2 :37-38
            op = IntOp('add', src=x, src2=res, shift=a - b, relu=relu, swap=True)
        else:                                                       # res << (b - a)
            op = IntOp('add', src=res, src2=x, shift=b - a, relu=relu)
        ig.ops.append(op)
        fl[len(ig.ops) - 1] = max(a, b)
        return len(ig.ops) - 1

    t = conv(0, spec.head, quant=False)
    if spec.head_maxpool:
        ig.ops.append(IntOp('maxpool', src=t, kernel=3, stride=2, pad=1))
        fl[len(ig.ops) - 1] = fl[t]
        t = len(ig.ops) - 1
    ge = spec.arch.startswith('mobilenet')
    for b in spec.blocks:
        x = r = t
        for c in b.body:
            r = conv(r, c)
        if b.shortcut is not None:
            r = join(r, conv(x, b.shortcut), b.post_relu, ge)
        elif b.residual:
            r = join(r, x, b.post_relu, ge)
        t = r
    if spec.tail is not None:
        t = conv(t, spec.tail)
    ig.ops.append(IntOp('avgpool', src=t))
    fl[len(ig.ops) - 1] = fl[t] + AVGPOOL_SHIFT
    t = len(ig.ops) - 1
    k = spec.fc_key
    ig.ops.append(IntOp('linear', src=t, weight=params[k + '.weight'].astype(np.int32),
                        bias=params[k + '.bias'].astype(np.int32), shift=fl[t] - _fl(params, k, 'input_fraclen'),
                        signed=spec.fc_signed_in, key=k))
    ig.output = len(ig.ops) - 1
    ig.output_float = True
    return ig


class _Writer:
    def __init__(self):
        self.nodes = []
        self.n = 0

    def emit(self, op, inputs, attrs=None):
        self.n += 1
        out = f'/{op}_{self.n}_output_0'
        self.nodes.append(Node(op, list(inputs), [out], name=f'/{op}_{self.n}', attrs=dict(attrs or {})))
        return out

    def const(self, value, dtype):
        return self.emit('Constant', [], {'value': np.array(value, dtype)})

    def cast(self, x, to):
        return self.emit('Cast', [x], {'to': to})

    def pow2(self, e):                                               # `1 << e` traced as int(2.0 ** e)
        e = self.const(float(e), np.float32)
        return self.cast(self.emit('Pow', [self.const(2.0, np.float32), e]), onnx_io.INT32)


def _requant(w, s, n, signed):
    """int_op_only_fix_quant of value s by shift n as the tracer writes it (the conv branch of export_graph keeps its own copy: it merges two
    requants of a max-pool result).  Returns the int32 value."""
    lo, hi = (-127.0, 127.0) if signed else (0.0, 255.0)
    if n > 0:
        h = 1 << (n - 1)
        a = w.emit('Add', [s, w.const(h, np.int32)])
        m = w.emit('Mod', [s, w.const(1 << n, np.int32)], {'fmod': 0})
        e = w.emit('Equal', [w.cast(m, onnx_io.INT64), w.const(h, np.int64)])
        v = w.emit('Where', [e, w.emit('Mul', [w.emit('Div', [a, w.pow2(n + 1)]), w.pow2(1)]), w.emit('Div', [a, w.pow2(n)])])
    else:
        v = w.emit('Mul', [s, w.pow2(-n)])
    return w.cast(w.emit('Clip', [v, w.const(lo, np.float32), w.const(hi, np.float32)]), onnx_io.INT32)


def export_graph(ig: IntGraph) -> bytes:
    """IntGraph -> serialized ModelProto."""
    w = _Writer()
    inits = {}
    name = {}
    shared = {}
    flat = set()                                                     # tensors the file holds as [N, C]: a Gemm's result and what follows it element-wise
    for t, o in enumerate(ig.ops):
        if o.kind == 'input':
            name[t] = 'input'
            in_dims = ['batch_size'] + list(o.shape)
            continue
        if o.kind in ('conv', 'deconv', 'linear'):
            s = name[o.src]
            if o.kind == 'linear':                                   # x.view(x.size(0), -1), fix_resnet.py:371
                b0 = w.emit('Gather', [w.emit('Shape', [s]), w.const(0, np.int64)], {'axis': 0})
                cat = w.emit('Concat', [w.emit('Unsqueeze', [b0], {'axes': [0]}), w.const([-1], np.int64)], {'axis': 0})
                s = w.emit('Reshape', [s, cat])
            if o.shift is not None:
                n = o.shift
                lo, hi = (-127.0, 127.0) if o.signed else (0.0, 255.0)
                if (s, n) in shared and ig.ops[o.src].kind == 'maxpool':
                    # the tracer merges the identical arithmetic of two requants of one tensor (body.0 / shortcut.0 at
                    # equal input_fraclen) — but only where the tensor has no in-place writers: the `.int()` of the
                    # max-pool detour, not the clamp_/ReLU(inplace) results that open later stages.  Where / Clip stay.
                    e, tie, reg = shared[(s, n)]
                    v = w.emit('Where', [e, tie, reg]) if n > 0 else tie
                elif n > 0:
                    h = 1 << (n - 1)
                    a = w.emit('Add', [s, w.const(h, np.int32)])
                    m = w.emit('Mod', [s, w.const(1 << n, np.int32)], {'fmod': 0})
                    e = w.emit('Equal', [w.cast(m, onnx_io.INT64), w.const(h, np.int64)])
                    tie = w.emit('Mul', [w.emit('Div', [a, w.pow2(n + 1)]), w.pow2(1)])
                    reg = w.emit('Div', [a, w.pow2(n)])
                    shared[(s, n)] = (e, tie, reg)
                    v = w.emit('Where', [e, tie, reg])
                else:
                    v = w.emit('Mul', [s, w.pow2(-n)])
                    shared[(s, n)] = (None, v, None)
                v = w.emit('Clip', [v, w.const(lo, np.float32), w.const(hi, np.float32)])
                s = w.cast(v, onnx_io.INT32)
            inits[o.key + '.weight'] = o.weight
            ins = [s, o.key + '.weight']
            if o.bias is not None:
                inits[o.key + '.bias'] = o.bias
                ins.append(o.key + '.bias')
            if o.kind == 'conv':
                kh, kw, sh, sw, pt, pl, pb, pr = o.conv_geometry()     # (pads: [top, left, bottom, right]; an axis of one tap has dilation 1)
                y = w.emit('Conv', ins, {'dilations': [int(o.dilation) if kh > 1 else 1, int(o.dilation) if kw > 1 else 1], 'group': int(o.groups),
                                         'kernel_shape': [kh, kw], 'pads': [pt, pl, pb, pr], 'strides': [sh, sw]})
            elif o.kind == 'deconv':
                y = w.emit('ConvTranspose', ins, {'dilations': [1, 1], 'group': 1, 'kernel_shape': [o.kernel] * 2, 'output_padding': [int(o.output_padding)] * 2,
                                                  'pads': [o.pad] * 4, 'strides': [o.stride] * 2})
            else:
                y = w.emit('Gemm', ins, {'alpha': 1.0, 'beta': 1.0, 'transB': 1})
                flat.add(t)
        elif o.kind == 'add':
            m = w.emit('Mul', [name[o.src], w.pow2(o.shift)])
            v = w.emit('Add', [name[o.src2], m] if o.swap else [m, name[o.src2]])   # `res += x`: res first
            v = w.emit('Clip', [v, w.const(-2147483647.0, np.float32), w.const(2147483647.0, np.float32)])
            y = w.cast(v, onnx_io.INT32)
        elif o.kind == 'hgate':                                      # relu6(x + 3) at fraction length fl = o.shift: clamp first, then the offset
            lim = 3 << o.shift
            v = w.emit('Clip', [name[o.src], w.const(float(-lim), np.float32), w.const(float(lim), np.float32)])
            y = w.emit('Add', [w.cast(v, onnx_io.INT32), w.const(lim, np.int32)])
            if o.src in flat:
                flat.add(t)
        elif o.kind == 'table':
            A = _requant(w, name[o.src], o.shift, o.signed)
            if o.signed:
                A = w.emit('Add', [A, w.const(128, np.int32)])
            key = f'table_{t}.in_fl_{int(o.in_fl)}.out_fl_{int(o.out_fl)}'
            inits[key] = np.ascontiguousarray(np.asarray(o.table).reshape(256), dtype=np.int32)
            y = w.emit('Gather', [key, A], {'axis': 0})
            if o.src in flat:
                flat.add(t)
        elif o.kind == 'mul':
            A = _requant(w, name[o.src], o.shifts[0], o.signed)
            B = _requant(w, name[o.src2], o.shifts[1], o.signed2)
            if o.src2 in flat and o.src not in flat:
                B = w.emit('Unsqueeze', [B], {'axes': [2, 3]})
            y = w.emit('Mul', [A, B])
            if o.src in flat:
                flat.add(t)
        elif o.kind == 'concat':                                     # torch.cat(dim=1); `x << k` as in the residual join
            y = w.emit('Concat', [name[s] if k == 0 else w.emit('Mul', [name[s], w.pow2(k)]) for s, k in zip(o.srcs, o.shifts)], {'axis': 1})
        elif o.kind == 'slice':                                      # x[:, a:b]
            y = w.emit('Slice', [name[o.src], w.const([o.first], np.int64), w.const([o.first + o.channels], np.int64), w.const([1], np.int64),
                                 w.const([1], np.int64)])
        elif o.kind == 'shuffle':                                    # x.view(N, g, C / g, H, W).transpose(1, 2).reshape(N, C, H, W)
            C, H, W = tensor_shapes(ig.ops[:t + 1])[t]
            v = w.emit('Reshape', [name[o.src], w.const([-1, o.groups, C // o.groups, H, W], np.int64)])
            v = w.emit('Transpose', [v], {'perm': [0, 2, 1, 3, 4]})
            y = w.emit('Reshape', [v, w.const([-1, C, H, W], np.int64)])
        elif o.kind == 'd2s':
            y = w.emit('DepthToSpace', [name[o.src]], {'blocksize': int(o.block), 'mode': o.order.upper().encode()})
        elif o.kind == 's2d' and o.order == 'dcr':
            y = w.emit('SpaceToDepth', [name[o.src]], {'blocksize': int(o.block)})
        elif o.kind == 's2d':                                        # x.view(N, C, H / r, r, W / r, r).permute(0, 1, 3, 5, 2, 4).reshape(N, C r^2, H / r, W / r)
            C, H, W = tensor_shapes(ig.ops[:t + 1])[t]
            r = int(o.block)
            v = w.emit('Reshape', [name[o.src], w.const([-1, C // (r * r), H, r, W, r], np.int64)])
            v = w.emit('Transpose', [v], {'perm': [0, 1, 3, 5, 2, 4]})
            y = w.emit('Reshape', [v, w.const([-1, C, H, W], np.int64)])
        elif o.kind == 'upsample':
            roi, sc = w.const(np.zeros(0, np.float32), np.float32), w.const([1.0, 1.0, float(o.scale[0]), float(o.scale[1])], np.float32)
            if o.mode == 'nearest':
                y = w.emit('Resize', [name[o.src], roi, sc], {'coordinate_transformation_mode': b'asymmetric', 'mode': b'nearest', 'nearest_mode': b'floor'})
            else:                                                    # the interpolated value times 4 s^2: integers again behind the Mul
                v = w.emit('Resize', [w.cast(name[o.src], onnx_io.FLOAT), roi, sc], {'coordinate_transformation_mode': b'half_pixel', 'mode': b'linear'})
                y = w.cast(w.emit('Mul', [v, w.const(float(4 * o.scale[0] * o.scale[1]), np.float32)]), onnx_io.INT32)
        elif o.kind == 'maxpool':
            v = w.emit('MaxPool', [w.cast(name[o.src], onnx_io.FLOAT)],
                       {'ceil_mode': 0, 'dilations': [1, 1], 'kernel_shape': [o.kernel] * 2, 'pads': [o.pad] * 4,
                        'strides': [o.stride] * 2})
            y = w.cast(v, onnx_io.INT32)
        elif o.kind == 'avgpool2d':                                  # the window's sum: the average times k^2, integers again behind the Mul
            v = w.emit('AveragePool', [w.cast(name[o.src], onnx_io.FLOAT)],
                       {'ceil_mode': 0, 'count_include_pad': 1, 'kernel_shape': [o.kernel] * 2, 'pads': [o.pad] * 4, 'strides': [o.stride] * 2})
            y = w.cast(w.emit('Mul', [v, w.const(float(o.kernel * o.kernel), np.float32)]), onnx_io.INT32)
        elif o.kind == 'avgpool':
            v = w.cast(name[o.src], onnx_io.INT64)
            v = w.emit('ReduceSum', [v], {'axes': [-1], 'keepdims': 0})
            v = w.emit('ReduceSum', [v], {'axes': [-1], 'keepdims': 0})
            y = w.cast(v, onnx_io.INT32)
            flat.add(t)
        else:
            raise ValueError(o.kind)
        if o.relu:
            y = w.cast(w.emit('Relu', [y]), onnx_io.INT32)
        name[t] = y
    if ig.output_argmax:                                             # the class map: ArgMax over the channels (int64), cast to the index type
        if ig.output_argmax not in ('u8', 'i32'):
            raise ValueError(f"IntGraph.output_argmax {ig.output_argmax!r}: None, 'u8' or 'i32'")
        out_type = onnx_io.UINT8 if ig.output_argmax == 'u8' else onnx_io.INT32
        w.cast(w.emit('ArgMax', [name[ig.output]], {'axis': 1, 'keepdims': 0, 'select_last_index': 0}), out_type)
    else:
        out_type = onnx_io.FLOAT if ig.output_float else onnx_io.INT32
        w.cast(name[ig.output], out_type)
    w.nodes[-1].outputs[0] = 'output'
    classes = ig.ops[ig.output].weight.shape[0] if ig.ops[ig.output].kind == 'linear' and not ig.output_argmax else '?'
    g = onnx_io.Graph(w.nodes, inits, [('input', onnx_io.INT32, in_dims)],
                      [('output', out_type, ['batch_size', classes])],
                      opset=11, producer='f8net_amd', name='main_graph')
    return onnx_io.model_proto(g)


def onnx_export(model, data_shape, output_file):
    """Same call shape as the reference's `onnx_export(model, data_shape, data_dtype, device, output_file)`
    (myutils/export.py:4) minus what a tracer needs: `model` is our IntModel, data_shape = [1, 3, H, W]."""
    ig = graph_from_params(model.spec, model.state_dict(), hw=int(data_shape[2]))
    data = export_graph(ig)
    with open(output_file, 'wb') as fh:
        fh.write(data)
    return len(data)
