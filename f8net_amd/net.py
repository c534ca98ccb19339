"""Host-side mirror of the reference's IntModel on top of libf8net.so.

`F8Net` walks a topology table + an exported-IntModel parameter dict and records the same integer
graph the reference's `IntModel.forward` executes (/root/reference/models/fix_resnet.py:352-383,
fix_mobilenet_v2.py:207-241, fix_mobilenet_v1.py:120-147) through the C ABI; the library plans it
into fused HIP launches.  torch is used for device memory and streams only.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib, tables, topology
from ._lib import ConvDesc, ConvGeom, LinearDesc, MulDesc, TableDesc, check

AVGPOOL_SHIFT = 6   # FXQAvgPool2d(7).shiftnum = round(log2(49)), fix_quant_ops.py:121-122


def _np_i32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)


def accept_grouped(net, convs, options=None):
    """The raw builder refuses grouped convs (1 < groups < cin) unless the handle's option `grouped` says otherwise, and the option must be set
    before the conv is added.  The high-level entry points call this before they record: a value the caller gave (options, or F8_GROUPED in the
    environment) is applied as it is; with none, `grouped` becomes 1 when one of `convs` — (cin, groups) pairs — is grouped."""
    if options and 'grouped' in options:
        net.set_option('grouped', options['grouped'])
    elif 'F8_GROUPED' not in os.environ and any(1 < g < cin for cin, g in convs):
        net.set_option('grouped', 1)


def conv_pair(v):
    """An int or a pair as (h, w)."""
    if isinstance(v, (tuple, list)):
        h, w = v
        return int(h), int(w)
    return int(v), int(v)


def conv_pads(pad):
    """An int, (ph, pw) or (top, left, bottom, right) as (top, left, bottom, right) — the order of ONNX `pads`."""
    if isinstance(pad, (tuple, list)):
        if len(pad) == 2:
            return int(pad[0]), int(pad[1]), int(pad[0]), int(pad[1])
        t, l, b, r = pad
        return int(t), int(l), int(b), int(r)
    return (int(pad),) * 4


class F8Net:
    """One planned integer network (or single op) living in libf8net.so."""

    def __init__(self):
        self._L = _lib.lib()
        self._h = self._L.f8_net_create()
        if not self._h:
            raise MemoryError('f8_net_create failed')
        self.max_batch = 0
        self.out_elems = 0
        self.out_float = True
        self.in_shape = None
        self.outputs = []       # after finalize: (C, H, W, fraclen, as_float) of every output, in the order of the output() calls
        self.output_kinds = []  # after finalize, parallel to `outputs`: 0 int32 values, 1 float32 values, 2 argmax as uint8, 3 argmax as int32 (f8_net_output_kind)
        self.tap_ids = {}       # record_net: name -> tensor id of everything `taps=` accepts
        self.taps = ()          # record_net: the names marked as outputs 1 .., in that order

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self._L.f8_net_destroy(h)

    # ---- builder (thin wrappers over the C ABI) ------------------------------------------
    def input(self, C, H, W, fraclen):
        self.in_shape = (C, H, W)
        return check(self._L.f8_net_input(self._h, C, H, W, fraclen))

    def conv(self, src, weight, bias, *, stride, pad, groups, weight_fl, input_fl, input_signed,
             quant_input=True, relu=False, label=None, dilation=1):
        """dilation: the spacing of the kernel's taps (f8_net_conv_dilated); the weights stay the real taps.
        weight may be [cout, cin_g, kh, kw]; stride an int or (sh, sw); pad an int, (ph, pw) or (top, left, bottom, right).  Anything square and symmetric
        goes through f8_net_conv / f8_net_conv_dilated as ever; everything else is f8_net_conv_rect."""
        w = _np_i32(weight)
        cout, cin_g, kh, kw = w.shape
        sh, sw = conv_pair(stride)
        pads = conv_pads(pad)
        square = kh == kw and sh == sw and len(set(pads)) == 1
        d = ConvDesc(cin=cin_g * groups, cout=cout, kernel=kh if square else 0, stride=sh if square else 0, pad=pads[0] if square else 0, groups=groups,
                     weight_fl=int(weight_fl), input_fl=int(input_fl), input_signed=int(bool(input_signed)),
                     quant_input=int(bool(quant_input)), relu=int(bool(relu)))
        b = None if bias is None else _np_i32(bias)
        if not square:
            g = ConvGeom(kh=kh, kw=kw, stride_h=sh, stride_w=sw, pad_top=pads[0], pad_left=pads[1], pad_bottom=pads[2], pad_right=pads[3],
                         dilation=int(dilation))
            t = check(self._L.f8_net_conv_rect(self._h, src, ctypes.byref(d), ctypes.byref(g), w.ctypes.data,
                                               None if b is None else b.ctypes.data))
        elif dilation != 1:
            t = check(self._L.f8_net_conv_dilated(self._h, src, ctypes.byref(d), int(dilation), w.ctypes.data,
                                                  None if b is None else b.ctypes.data))
        else:
            t = check(self._L.f8_net_conv(self._h, src, ctypes.byref(d), w.ctypes.data,
                                          None if b is None else b.ctypes.data))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def conv_transpose(self, src, weight, bias, *, stride, pad, output_padding=0, weight_fl, input_fl, input_signed,
                       quant_input=True, relu=False, label=None):
        """Transposed convolution (f8_net_conv_transpose): weight [cin, cout, k, k] as nn.ConvTranspose2d.weight; the result is
        [(H - 1) stride - 2 pad + k + output_padding]^2 at fraclen weight_fl + input_fl.  stride 1 is recorded as the equivalent plain conv."""
        w = _np_i32(weight)
        cin, cout, k, k2 = w.shape
        assert k == k2
        d = ConvDesc(cin=cin, cout=cout, kernel=k, stride=stride, pad=pad, groups=1,
                     weight_fl=int(weight_fl), input_fl=int(input_fl), input_signed=int(bool(input_signed)),
                     quant_input=int(bool(quant_input)), relu=int(bool(relu)))
        b = None if bias is None else _np_i32(bias)
        t = check(self._L.f8_net_conv_transpose(self._h, src, ctypes.byref(d), int(output_padding), w.ctypes.data,
                                                None if b is None else b.ctypes.data))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def linear(self, src, weight, bias, *, weight_fl, input_fl, input_signed, quant_input=True, label=None):
        w = _np_i32(weight)
        d = LinearDesc(in_features=w.shape[1], out_features=w.shape[0], weight_fl=int(weight_fl),
                       input_fl=int(input_fl), input_signed=int(bool(input_signed)),
                       quant_input=int(bool(quant_input)))
        b = None if bias is None else _np_i32(bias)
        t = check(self._L.f8_net_linear(self._h, src, ctypes.byref(d), w.ctypes.data,
                                        None if b is None else b.ctypes.data))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def add(self, a, b, relu=False, label=None):
        t = check(self._L.f8_net_add(self._h, a, b, int(bool(relu))))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def concat(self, srcs, label=None):
        """Channel concatenation of 2 .. 8 tensors of one map size, in order (f8_net_concat); fraclen = the largest operand fraclen."""
        ids = (ctypes.c_int * len(srcs))(*[int(t) for t in srcs])
        t = check(self._L.f8_net_concat(self._h, ids, len(srcs)))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def upsample(self, src, scale, mode='nearest', label=None):
        """Upsampling by integer scales (f8_net_upsample): `scale` is an int or (scale_h, scale_w); mode 'nearest' keeps the fraclen, 'bilinear'
        (half-pixel centres, scale 2 / 4 / 8 / 16) yields the exact interpolated value times 4 scale^2 at fraclen + 2 log2(scale) + 2."""
        sh, sw = (scale, scale) if isinstance(scale, int) else scale
        modes = {'nearest': 0, 'bilinear': 1}
        if mode not in modes:
            raise ValueError(f"upsample mode {mode!r}: 'nearest' or 'bilinear'")
        t = check(self._L.f8_net_upsample(self._h, src, modes[mode], int(sh), int(sw)))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def slice(self, src, start, stop, label=None):
        """Channels [start, stop) of a tensor, `x[:, start:stop]` (f8_net_slice); map size and fraclen are the source's."""
        t = check(self._L.f8_net_slice(self._h, src, int(start), int(stop) - int(start)))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def split(self, src, sizes, labels=None):
        """torch.split(x, sizes, dim=1): one slice per entry of `sizes`, in channel order."""
        out, first = [], 0
        for k, n in enumerate(sizes):
            out.append(self.slice(src, first, first + int(n), label=labels[k] if labels else None))
            first += int(n)
        return out

    def channel_shuffle(self, src, groups, label=None):
        """torch.nn.functional.channel_shuffle(x, groups) (f8_net_channel_shuffle); map size and fraclen are the source's."""
        t = check(self._L.f8_net_channel_shuffle(self._h, src, int(groups)))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def _pixmap(self, fn, src, block, order, label):
        orders = {'dcr': 0, 'crd': 1}
        if order not in orders:
            raise ValueError(f"order {order!r}: 'crd' or 'dcr'")
        t = check(fn(self._h, src, int(block), orders[order]))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def depth_to_space(self, src, block, order='crd', label=None):
        """[C r^2, H, W] -> [C, H r, W r], r = block (f8_net_depth_to_space).  order 'crd': torch.nn.functional.pixel_shuffle / ONNX DepthToSpace
        mode="CRD"; 'dcr': ONNX DepthToSpace's default mode.  The fraclen is the source's."""
        return self._pixmap(self._L.f8_net_depth_to_space, src, block, order, label)

    def space_to_depth(self, src, block, order='crd', label=None):
        """[C, H r, W r] -> [C r^2, H, W], r = block, the inverse of depth_to_space for each order (f8_net_space_to_depth).  order 'crd':
        torch.nn.functional.pixel_unshuffle; 'dcr': ONNX SpaceToDepth, TResNet's stem.  The fraclen is the source's."""
        return self._pixmap(self._L.f8_net_space_to_depth, src, block, order, label)

    def pixel_shuffle(self, src, r, label=None):
        """torch.nn.functional.pixel_shuffle(x, r): depth_to_space in CRD order."""
        return self.depth_to_space(src, r, 'crd', label)

    def pixel_unshuffle(self, src, r, label=None):
        """torch.nn.functional.pixel_unshuffle(x, r): space_to_depth in CRD order."""
        return self.space_to_depth(src, r, 'crd', label)

    def mul(self, a, b, *, a_fl, a_signed, b_fl, b_signed=False, relu=False, label=None):
        """Fixed-point product of two activations (f8_net_mul): a requantised to (a_fl, a_signed) times b requantised to (b_fl, b_signed), at fraclen
        a_fl + b_fl.  b has a's shape (element-wise) or is [C, 1, 1] (a per-image channel gate: the scale of a squeeze-and-excitation block)."""
        d = MulDesc(a_fl=int(a_fl), a_signed=int(bool(a_signed)), b_fl=int(b_fl), b_signed=int(bool(b_signed)), relu=int(bool(relu)))
        t = check(self._L.f8_net_mul(self._h, a, b, ctypes.byref(d)))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def hard_gate(self, src, label=None):
        """relu6(x + 3) in fixed point (f8_net_hard_gate): clamp(x, -3 * 2^fl, 3 * 2^fl) + 3 * 2^fl at the source's fraclen — the numerator of
        hard-sigmoid; its 1 / 6 is a constant real scale for the exporter to fold into the next conv's weights."""
        t = check(self._L.f8_net_hard_gate(self._h, src))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def hard_swish(self, src, *, x_fl, x_signed, g_fl, label=None):
        """x * relu6(x + 3) (six times hard-swish): mul(src, hard_gate(src)) with x read at (x_fl, x_signed) and the gate, 0 .. 6, at unsigned g_fl."""
        return self.mul(src, self.hard_gate(src), a_fl=x_fl, a_signed=x_signed, b_fl=g_fl, b_signed=False, label=label)

    def table(self, src, table, *, in_fl, in_signed, out_fl, label=None):
        """Any pointwise function as a 256-entry table (f8_net_table): src requantised to (in_fl, in_signed) gives q; the result is table[q] (unsigned)
        or table[q + 128] (signed), int32 at fraclen out_fl.  `table`: 256 int32 entries (f8net_amd.tables builds them)."""
        tab = np.ascontiguousarray(np.asarray(table).reshape(-1), dtype=np.int32)
        if tab.size != 256 or not np.array_equal(tab, np.asarray(table).reshape(-1)):
            raise ValueError('table: 256 int32 entries')
        d = TableDesc(in_fl=int(in_fl), in_signed=int(bool(in_signed)), out_fl=int(out_fl))
        t = check(self._L.f8_net_table(self._h, src, ctypes.byref(d), tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def sigmoid(self, src, *, in_fl, in_signed, out_fl, label=None):
        return self.table(src, tables.sigmoid(in_fl, in_signed, out_fl), in_fl=in_fl, in_signed=in_signed, out_fl=out_fl, label=label)

    def swish(self, src, *, in_fl, in_signed, out_fl, label=None):
        return self.table(src, tables.swish(in_fl, in_signed, out_fl), in_fl=in_fl, in_signed=in_signed, out_fl=out_fl, label=label)

    def tanh(self, src, *, in_fl, in_signed, out_fl, label=None):
        return self.table(src, tables.tanh(in_fl, in_signed, out_fl), in_fl=in_fl, in_signed=in_signed, out_fl=out_fl, label=label)

    def maxpool(self, src, k=3, stride=2, pad=1, label=None):
        t = check(self._L.f8_net_maxpool(self._h, src, k, stride, pad))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def avgpool(self, src, kernel, stride=None, pad=0, shift=None, label=None):
        """Windowed average pooling (f8_net_avgpool_window): the wrapping int32 SUM of each kernel x kernel window's in-image taps at fraclen + shift;
        `stride` defaults to `kernel`, `shift` to the reference's round(log2(kernel^2)).  The global window (kernel == H == W, pad 0) is avgpool_sum."""
        kernel = int(kernel)
        stride = kernel if stride is None else int(stride)
        if shift is None:
            shift = int(round(math.log2(kernel * kernel))) if kernel >= 1 else 0
        t = check(self._L.f8_net_avgpool_window(self._h, src, kernel, stride, int(pad), int(shift)))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def adaptive_avgpool(self, src, bins, shift=None, label=None):
        """nn.AdaptiveAvgPool2d(bins) on a map whose sides are multiples of `bins` (kernel = stride = side / bins, which must be the same for both
        sides: windows are square); any other map raises ValueError (uneven bins are not built)."""
        _, h, w, _ = self.tensor_info(src)
        bins = int(bins)
        if bins < 1 or h % bins or w % bins or h // bins != w // bins:
            raise ValueError(f'adaptive_avgpool: a {h} x {w} map does not split into {bins} x {bins} equal square windows')
        k = h // bins
        if k == 1:
            raise ValueError(f'adaptive_avgpool: {bins} bins of a {h} x {w} map is the identity')
        return self.avgpool(src, k, k, 0, shift, label)

    def avgpool_sum(self, src, shift=AVGPOOL_SHIFT, label=None):
        t = check(self._L.f8_net_avgpool_sum(self._h, src, shift))
        if label:
            self._L.f8_net_set_label(self._h, t, label.encode())
        return t

    def output(self, src, as_float=True):
        """Marks tensor `src` as a network output (f8_net_output) and returns its index.  The first call names output 0, which the
        run methods return as today; every further call adds an output that they return behind it, shaped [N, C, H, W]."""
        k = check(self._L.f8_net_output(self._h, src, int(bool(as_float))))
        if k == 0:
            self.out_float = bool(as_float)
        return k

    def output_argmax(self, src, dtype='u8'):
        """Marks the channel argmax of tensor `src` as a network output (f8_net_output_argmax) and returns its index: the class map [N, H, W] of a
        segmentation head ([N] for a [C, 1, 1] tensor: the predicted class), the smallest index winning a tie.  dtype 'u8' (at most 255 channels;
        255 is the poison value) or 'i32'.  The tensor may be a value output as well (output())."""
        sizes = {'u8': 1, 'i32': 4}
        if dtype not in sizes:
            raise ValueError(f"output_argmax dtype {dtype!r}: 'u8' or 'i32'")
        k = check(self._L.f8_net_output_argmax(self._h, src, sizes[dtype]))
        if k == 0:
            self.out_float = False
        return k

    def finalize(self, max_batch):
        check(self._L.f8_net_finalize(self._h, int(max_batch)))
        self.max_batch = int(max_batch)
        self.out_elems = int(self._L.f8_net_output_elems(self._h))
        self.outputs = [self.output_info(k) for k in range(check(self._L.f8_net_num_outputs(self._h)))]
        self.output_kinds = [check(self._L.f8_net_output_kind(self._h, k)) for k in range(len(self.outputs))]
        return self

    def _out_dtype(self, k):
        """torch dtype of output k's buffer."""
        import torch
        return (torch.int32, torch.float32, torch.uint8, torch.int32)[self.output_kinds[k]]

    def _output0(self, N, device, out):
        """Output 0's buffer [N, out_elems] (a class map as output 0: [N, H * W]); allocated when `out` is None, checked when it is a class map."""
        import torch
        dt = self._out_dtype(0)
        if out is None:
            return torch.empty((N, self.out_elems), dtype=dt, device=device)
        if self.output_kinds[0] >= 2 and (out.device != device or out.dtype != dt or not out.is_contiguous() or out.numel() != N * self.out_elems):
            raise ValueError(f'F8Net: out= must be a contiguous {dt} tensor of [{N},{self.out_elems}] on {device} (output 0 is a class map)')
        return out

    def output_info(self, k):
        """(C, H, W, fraclen, as_float) of output k (f8_net_output_info)."""
        v = [ctypes.c_int(0) for _ in range(5)]
        check(self._L.f8_net_output_info(self._h, int(k), *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v[:4]) + (bool(v[4].value),)

    def tensor_info(self, t):
        """(C, H, W, fraclen) of any recorded tensor (f8_net_tensor_info)."""
        v = [ctypes.c_int(0) for _ in range(4)]
        check(self._L.f8_net_tensor_info(self._h, int(t), *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # ---- introspection ----------------------------------------------------------------------
    def describe(self) -> str:
        n = self._L.f8_net_describe(self._h, None, 0)
        buf = ctypes.create_string_buffer(n)
        self._L.f8_net_describe(self._h, buf, n)
        return buf.value.decode()

    @property
    def num_launches(self):
        return check(self._L.f8_net_num_launches(self._h))

    @property
    def arena_bytes(self):
        return int(self._L.f8_net_arena_bytes(self._h))

    @property
    def weight_bytes(self):
        return int(self._L.f8_net_weight_bytes(self._h))

    @property
    def output_fraclen(self):
        return check(self._L.f8_net_output_fraclen(self._h))

    def launch_info(self, i, N):
        name = ctypes.create_string_buffer(256)
        b, o = ctypes.c_double(), ctypes.c_double()
        check(self._L.f8_net_launch_info(self._h, i, N, name, 256, ctypes.byref(b), ctypes.byref(o)))
        return name.value.decode(), b.value, o.value

    def num_parts(self, N):
        return check(self._L.f8_net_num_parts(self._h, int(N)))

    def step_launches(self, i, N):
        """Kernel launches planned launch i issues per run of N images (sub-batches / chunks), f8_net_step_launches."""
        return check(self._L.f8_net_step_launches(self._h, i, int(N)))

    def launch_valu(self, i, N):
        """Essential vector lane-operations of planned launch i for N images (f8_net_launch_valu)."""
        v = ctypes.c_double(0.0)
        check(self._L.f8_net_launch_valu(self._h, i, int(N), ctypes.byref(v)))
        return v.value

    def launch_kernel(self, i):
        buf = ctypes.create_string_buffer(256)
        check(self._L.f8_net_launch_kernel(self._h, i, buf, 256))
        return buf.value.decode()

    def launch_grid(self, i, N, num_cu=0):
        """Stage-chain geometry of planned launch i for N images on num_cu compute units (0: 256), f8_net_launch_grid:
        (workgroups per tile column, groups, grid, images per tile column); zeros for other launches."""
        v = [ctypes.c_int(0) for _ in range(4)]
        check(self._L.f8_net_launch_grid(self._h, i, int(N), int(num_cu), *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # ---- execution (torch = device memory + stream plumbing) ---------------------------------
    def upload(self):
        check(self._L.f8_net_upload(self._h))

    def _check_input(self, x):
        import torch
        if not x.is_cuda:
            raise ValueError('F8Net.run: input must be a CUDA/HIP tensor (there is no CPU path)')
        if x.dtype != torch.int32 or not x.is_contiguous():
            raise ValueError('F8Net.run: input must be contiguous int32 NCHW')
        if tuple(x.shape[1:]) != tuple(self.in_shape):
            raise ValueError(f'F8Net.run: input shape {tuple(x.shape)} != [N,{self.in_shape}]')
        if not (1 <= x.shape[0] <= self.max_batch):
            raise ValueError(f'F8Net.run: batch {x.shape[0]} outside [1,{self.max_batch}]')

    def set_option(self, key, value):
        """Per-handle tuning option (f8_net_set_option; keys in include/f8net.h).  Planning keys before finalize()."""
        check(self._L.f8_net_set_option(self._h, key.encode(), int(value)))
        return self

    def get_option(self, key):
        v = ctypes.c_int(0)
        check(self._L.f8_net_get_option(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def _input_ready(self, ev):
        """One-shot: the next run also waits for `ev` (a torch.cuda.Event recorded behind the producer of its input)."""
        if ev is not None:
            check(self._L.f8_net_set_input_ready(self._h, ctypes.c_void_p(ev.cuda_event)))

    def _output_buffers(self, N, device, outs):
        """Hands the buffers of outputs 1 .. to the next run (f8_net_set_output_buffers; allocated when `outs` is None) and returns them
        shaped [N, C, H, W] — a class map (output_argmax): [N, H, W], uint8 or int32.  A single-output net has none."""
        import torch
        extra = self.outputs[1:]
        if not extra:
            if outs:
                raise ValueError('F8Net: outs= given, but the net has a single output')
            return []
        shapes = [(N, H, W) if kind >= 2 else (N, C, H, W) for (C, H, W, _, _), kind in zip(extra, self.output_kinds[1:])]
        dtypes = [self._out_dtype(k) for k in range(1, len(self.outputs))]
        if outs is None:
            outs = [torch.empty(shape, dtype=dt, device=device) for shape, dt in zip(shapes, dtypes)]
        if len(outs) != len(extra):
            raise ValueError(f'F8Net: {len(outs)} buffers for outputs 1 .. {len(extra)}')
        res = []
        for o, shape, dt in zip(outs, shapes, dtypes):
            if o.device != device or o.dtype != dt or not o.is_contiguous() or o.numel() != math.prod(shape):
                raise ValueError(f'F8Net: an output buffer must be a contiguous {str(dt).replace("torch.", "")} tensor of {list(shape)} on {device}')
            res.append(o.view(shape))
        ptrs = (ctypes.c_void_p * len(res))(*[o.data_ptr() for o in res])
        check(self._L.f8_net_set_output_buffers(self._h, ptrs, len(res)))
        return res

    def run(self, x, out=None, input_ready=None, outs=None):
        """x: int32 CUDA tensor [N,C,H,W] (reference input format).  Returns [N, out_elems]; a net with more than one output returns the
        tuple (output 0, output 1, ...), the further ones shaped [N,C,H,W] (outs: their buffers, allocated when None).
        input_ready: torch.cuda.Event recorded behind the producer of `x` when that is another stream (pipelined callers)."""
        import torch
        self._check_input(x)
        N = x.shape[0]
        out = self._output0(N, x.device, out)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        with torch.cuda.device(x.device):
            outs = self._output_buffers(N, x.device, outs)      # (may raise: before the one-shot event is armed)
            self._input_ready(input_ready)
            check(self._L.f8_net_run(self._h, x.data_ptr(), out.data_ptr(), N, ctypes.c_void_p(stream)))
        return (out, *outs) if outs else out

    def check(self):
        """Synchronise the device and raise if a kernel of an earlier run reported a failure (f8_net_check)."""
        check(self._L.f8_net_check(self._h))
        return self

    def autotune(self, N, device=None):
        """Measured tile selection for runs of N images (f8_net_autotune).  Returns the number of launches re-tiled."""
        import torch
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            return check(self._L.f8_net_autotune(self._h, int(N), ctypes.c_void_p(stream)))

    def set_pipelined(self, on=True):
        """Let consecutive runs overlap (f8_net_set_pipelined): the caller keeps inputs / outputs of consecutive runs in
        buffers that were ready one call earlier (static input, double-buffered outputs).  on=2 / 'alternate': whole
        batches of consecutive runs alternate between two internal streams instead of splitting every run in two."""
        mode = 2 if on in (2, 'alternate') else int(bool(on))
        check(self._L.f8_net_set_pipelined(self._h, mode))

    def run_f32(self, images, normalize, out=None, input_ready=None, outs=None):
        """images: float32 CUDA tensor [N,C,H,W] as forward_loss receives them (fix_train.py:676-692); the input
        quantisation runs inside the input kernel.  normalize: FLAGS.normalize of the reference."""
        import torch
        if not images.is_cuda:
            raise ValueError('F8Net.run_f32: input must be a CUDA/HIP tensor (there is no CPU path)')
        if images.dtype != torch.float32 or not images.is_contiguous():
            raise ValueError('F8Net.run_f32: input must be contiguous float32 NCHW')
        if tuple(images.shape[1:]) != tuple(self.in_shape):
            raise ValueError(f'F8Net.run_f32: input shape {tuple(images.shape)} != [N,{self.in_shape}]')
        N = images.shape[0]
        if not (1 <= N <= self.max_batch):
            raise ValueError(f'F8Net.run_f32: batch {N} outside [1,{self.max_batch}]')
        out = self._output0(N, images.device, out)
        stream = torch.cuda.current_stream(images.device).cuda_stream
        with torch.cuda.device(images.device):
            outs = self._output_buffers(N, images.device, outs)
            self._input_ready(input_ready)
            check(self._L.f8_net_run_f32(self._h, images.data_ptr(), int(bool(normalize)), out.data_ptr(), N,
                                         ctypes.c_void_p(stream)))
        return (out, *outs) if outs else out

    def run_u8(self, images, normalize=False, mean=None, std=None, nhwc=False, out=None, input_ready=None, outs=None):
        """images: uint8 CUDA tensor, NCHW [N,3,H,W] (or NHWC [N,H,W,3] with nhwc=True) as a decoder yields them; ToTensor /
        Normalize(mean, std) / the input quantisation of forward_loss are a table lookup inside the input kernel (f8_net_run_u8)."""
        import torch
        if not images.is_cuda:
            raise ValueError('F8Net.run_u8: input must be a CUDA/HIP tensor (there is no CPU path)')
        if images.dtype != torch.uint8 or not images.is_contiguous():
            raise ValueError('F8Net.run_u8: input must be contiguous uint8')
        C, H, W = self.in_shape
        want = (H, W, C) if nhwc else (C, H, W)
        if tuple(images.shape[1:]) != want:
            raise ValueError(f'F8Net.run_u8: input shape {tuple(images.shape)} != [N,{want}]')
        N = images.shape[0]
        if not (1 <= N <= self.max_batch):
            raise ValueError(f'F8Net.run_u8: batch {N} outside [1,{self.max_batch}]')
        out = self._output0(N, images.device, out)
        m = (ctypes.c_float * 3)(*[float(v) for v in mean]) if mean is not None else None
        s = (ctypes.c_float * 3)(*[float(v) for v in std]) if std is not None else None
        stream = torch.cuda.current_stream(images.device).cuda_stream
        with torch.cuda.device(images.device):
            outs = self._output_buffers(N, images.device, outs)
            self._input_ready(input_ready)
            check(self._L.f8_net_run_u8(self._h, images.data_ptr(), int(bool(nhwc)), int(bool(normalize)), m, s, out.data_ptr(), N,
                                        ctypes.c_void_p(stream)))
        return (out, *outs) if outs else out

    def run_profiled(self, x, out=None, outs=None):
        """Like run(); also returns per-launch milliseconds (HIP events on the launch stream)."""
        import torch
        self._check_input(x)
        N = x.shape[0]
        out = self._output0(N, x.device, out)
        n = self.num_launches
        ms = (ctypes.c_float * n)()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        with torch.cuda.device(x.device):
            outs = self._output_buffers(N, x.device, outs)
            check(self._L.f8_net_run_profiled(self._h, x.data_ptr(), out.data_ptr(), N,
                                              ctypes.c_void_p(stream), ms, n))
        return ((out, *outs) if outs else out), [float(v) for v in ms]


def _fl(params, key, name):
    return int(np.asarray(params[f'{key}.{name}']).reshape(-1)[0])


def build_net(spec: topology.NetSpec, params: dict, max_batch: int, hw: int = 224,
              input_fraclen=None, options=None, taps=()) -> F8Net:
    """Record IntModel.forward for `spec` with exported parameters `params` (numpy or torch-cpu
    tensors keyed like the reference state_dict) and plan it for batches up to max_batch.
    options: {key: value} for f8_net_set_option, applied before planning.  taps: see record_net."""
    net = record_net(spec, params, hw, input_fraclen, taps=taps, options=options)
    for k, v in (options or {}).items():
        net.set_option(k, v)
    return net.finalize(max_batch)


def record_net(spec: topology.NetSpec, params: dict, hw: int = 224, input_fraclen=None, taps=(), options=None) -> F8Net:
    """The recording half of build_net: the graph is in the handle, not yet planned (set planning options, then finalize).
    options: only its `grouped` key is read here — grouped convs are accepted while they are recorded (accept_grouped).

    taps: names of further tensors to return, marked as int32 outputs 1, 2, ... in the order given (output 0 stays the float
    logits).  A name is a block name (`stage_1_layer_3`: the block's output tensor, whether or not the block ends in a join), a
    conv key (`stage_1_layer_3.body.0`, `head.0`, `tail.0`), 'head.maxpool' or 'avgpool' (the pooled vector in front of the
    classifier, at the last map's fraclen + 6).  A conv key names the tensor BEHIND that conv's ReLU, as a tensor id does everywhere
    in the C ABI; the CPU oracle's `tap=` callback reports a conv before its in-place ReLU, so a comparison applies `oracle.relu`
    where `ConvSpec.relu` is set.  An unknown name raises ValueError with the valid ones; the name -> tensor id map of everything
    that can be tapped is kept as `net.tap_ids`, the names given as `net.taps`."""
    params = {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in params.items()}
    net = F8Net()
    accept_grouped(net, [(c.cin, c.groups) for c in spec.convs()], options)
    head_in_fl = _fl(params, spec.head.key, 'input_fraclen')
    if input_fraclen is None:
        input_fraclen = head_in_fl if spec.normalize else 8     # fix_train.py:683-692
    if input_fraclen != head_in_fl:
        raise ValueError(f'network input fraclen {input_fraclen} != head.input_fraclen {head_in_fl}: the reference '
                         f'feeds the head conv head-format integers without requantising (fix_resnet.py:356-358)')

    ids = net.tap_ids

    def conv(src, c: topology.ConvSpec, quant_input=True):
        ids[c.key] = net.conv(src, params[c.key + '.weight'], params[c.key + '.bias'], stride=c.stride, pad=c.pad,
                              groups=c.groups, weight_fl=_fl(params, c.key, 'weight_fraclen'),
                              input_fl=_fl(params, c.key, 'input_fraclen'), input_signed=c.signed_in,
                              quant_input=quant_input, relu=c.relu, label=c.key, dilation=c.dilation)
        return ids[c.key]

    t = net.input(3, hw, hw, input_fraclen)
    t = conv(t, spec.head, quant_input=False)                    # fix_resnet.py:356-358
    if spec.head_maxpool:
        t = ids['head.maxpool'] = net.maxpool(t, 3, 2, 1, label='head.maxpool')        # fix_resnet.py:359
    for b in spec.blocks:                                        # IntBlock.forward, fix_resnet.py:26-77
        x = t
        r = x
        for c in b.body:
            r = conv(r, c)
        if b.shortcut is not None:
            sx = conv(x, b.shortcut)
            r = net.add(r, sx, relu=b.post_relu, label=b.name)
        elif b.residual:
            r = net.add(r, x, relu=b.post_relu, label=b.name)
        t = ids[b.name] = r
    if spec.tail is not None:                                    # fix_mobilenet_v2.py:218-224
        t = conv(t, spec.tail)
    t = ids['avgpool'] = net.avgpool_sum(t, AVGPOOL_SHIFT, label='avgpool')       # fix_quant_ops.py:126-134
    k = spec.fc_key
    t = net.linear(t, params[k + '.weight'], params[k + '.bias'], weight_fl=_fl(params, k, 'weight_fraclen'),
                   input_fl=_fl(params, k, 'input_fraclen'), input_signed=spec.fc_signed_in, label=k)
    net.output(t, as_float=True)                                 # `.float()`, fix_resnet.py:383
    taps = tuple(taps)
    unknown = [n for n in taps if n not in ids]
    if unknown:
        raise ValueError(f'record_net: unknown tap name(s) {unknown}; valid names: {", ".join(ids)}')
    for n in taps:
        net.output(ids[n], as_float=False)
    net.taps = taps
    return net
