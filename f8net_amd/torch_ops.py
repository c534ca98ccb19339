"""`torch.ops.f8net.*`: the C ABI of libf8net.so registered with the PyTorch dispatcher (torch.library).

The reference has no operator registry — its integer path is plain `nn.Module` composition — so these are the
"CUDAExtension-style" ops BASELINE.json's north_star asks for: each schema names one reference call site and its CUDA (HIP)
implementation ends in one `f8_*` entry point of include/f8net.h; `Meta` implementations give shapes, so the ops trace under
`torch.compile` / FakeTensor.  There is no CPU implementation: calling an op on CPU tensors raises NotImplementedError from
the dispatcher.

    f8net::requant(x, fl, input_fl, signed)          int_op_only_fix_quant            fix_quant_ops.py:90-114
    f8net::relu_(x)                                  nn.ReLU(inplace) on int32        fix_resnet.py:39,77
    f8net::add_align_(res, x, res_fl, x_fl)          residual align-add-clamp         fix_resnet.py:40-54
    f8net::conv2d(x, w, b, stride, pad, groups, weight_fl, input_fl, input_signed, dilation=1)    `layer_(res)`, int nn.Conv2d of int_conv :680-714
    f8net::conv2d_rect(x, w, b, stride[2], pads[4], groups, weight_fl, input_fl, input_signed, dilation=1)    the same with a kh x kw kernel, (sh, sw), (top, left, bottom, right)
    f8net::linear(x, w, b, weight_fl, input_fl, input_signed)                         `self.classifier(x)`, int_fc :1165-1195
    f8net::avgpool_sum(x)                            FXQAvgPool2d int branch          fix_quant_ops.py:126-134
    f8net::maxpool(x, k, stride, pad)                head max-pool                    fix_resnet.py:358-359
    f8net::channel_shuffle(x, groups)                torch.nn.functional.channel_shuffle on int32 (f8_net_channel_shuffle; no reference call site)
    f8net::depth_to_space(x, block, order)           [N, C r^2, H, W] -> [N, C, H r, W r]; order 'crd' = torch.nn.functional.pixel_shuffle, 'dcr' = ONNX
                                                     DepthToSpace's default (f8_net_depth_to_space; no reference call site)
    f8net::space_to_depth(x, block, order)           the inverse; 'crd' = pixel_unshuffle, 'dcr' = ONNX SpaceToDepth (f8_net_space_to_depth)
    f8net::mul_q(a, b, a_src_fl, b_src_fl, a_fl, a_signed, b_fl, b_signed, hard_gate_b, relu)
                                                     requant(a) * requant(b), b of a's shape or [N, C, 1, 1]; hard_gate_b: b is relu6(b + 3) in fixed point
                                                     first (f8_net_mul, f8_net_hard_gate; no reference call site)
    f8net::table_q(x, table, src_fl, in_fl, in_signed, out_fl)
                                                     table[requant(x) (+ 128 signed)]: any pointwise function as 256 int32 entries (f8_net_table;
                                                     f8net_amd.tables builds sigmoid, swish, tanh, ...; no reference call site)
    f8net::argmax_channels(x, u8)                    the smallest channel index of the largest value per pixel, [N, C, H, W] -> [N, H, W] uint8 (u8, at most
                                                     255 channels) or int32 (f8_net_output_argmax; the reference's forward_loss takes topk of the logits)
    f8net::net_forward(x, handle)                    IntModel.forward                 fix_resnet.py:352-383 (handle: register_net)
    f8net::net_forward_taps(x, handle)               ... of a net with further outputs (F8Net.output called more than once): all of them
    f8net::net_forward_f32(images, handle, normalize)  forward_loss input quantisation + IntModel.forward, fix_train.py:683-692

conv2d / linear plan a one-node net per (weight tensor, its in-place version, geometry, input shape, device) and cache it
(LRU); `F8Conv2d` / `F8Linear` / the pool modules in ops.py call these ops, so everything above the C ABI goes through the
dispatcher.
"""
import collections
import os
import ctypes
import weakref

import torch
from torch.library import Library

from . import _lib
from ._lib import check
from .net import F8Net, accept_grouped

_DEF = Library('f8net', 'DEF')
_DEF.define('requant(Tensor x, int fl, int input_fl, bool signed) -> Tensor')
_DEF.define('relu_(Tensor(a!) x) -> Tensor(a!)')
_DEF.define('add_align_(Tensor(a!) res, Tensor x, int res_fl, int x_fl) -> Tensor(a!)')
_DEF.define('conv2d(Tensor x, Tensor weight, Tensor? bias, int stride, int pad, int groups, int weight_fl, int input_fl, bool input_signed, int dilation=1) -> Tensor')
_DEF.define('conv2d_rect(Tensor x, Tensor weight, Tensor? bias, int[2] stride, int[4] pads, int groups, int weight_fl, int input_fl, bool input_signed, int dilation=1) -> Tensor')
_DEF.define('conv_transpose2d(Tensor x, Tensor weight, Tensor? bias, int stride, int pad, int output_padding, int weight_fl, int input_fl, bool input_signed) -> Tensor')
_DEF.define('linear(Tensor x, Tensor weight, Tensor? bias, int weight_fl, int input_fl, bool input_signed) -> Tensor')
_DEF.define('avgpool_sum(Tensor x) -> Tensor')
_DEF.define('avgpool2d_sum(Tensor x, int k, int stride, int pad) -> Tensor')
_DEF.define('maxpool(Tensor x, int k, int stride, int pad) -> Tensor')
_DEF.define('channel_shuffle(Tensor x, int groups) -> Tensor')
_DEF.define('depth_to_space(Tensor x, int block, str order) -> Tensor')
_DEF.define('space_to_depth(Tensor x, int block, str order) -> Tensor')
_DEF.define('mul_q(Tensor a, Tensor b, int a_src_fl, int b_src_fl, int a_fl, bool a_signed, int b_fl, bool b_signed, bool hard_gate_b, bool relu) -> Tensor')
_DEF.define('table_q(Tensor x, Tensor table, int src_fl, int in_fl, bool in_signed, int out_fl) -> Tensor')
_DEF.define('argmax_channels(Tensor x, bool u8) -> Tensor')
_DEF.define('net_forward(Tensor x, int handle) -> Tensor')
_DEF.define('net_forward_taps(Tensor x, int handle) -> Tensor[]')
_DEF.define('net_forward_f32(Tensor images, int handle, bool normalize) -> Tensor')


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _i32(t, who):
    if t.dtype != torch.int32:
        raise TypeError(f'f8net::{who}: expects int32, got {t.dtype}')


# ------------------------------------------------------------------------------------------ element-wise ops
def _requant(x, fl, input_fl, signed):
    _i32(x, 'requant')
    x = x.contiguous()
    res = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(_lib.lib().f8_requant_i32(x.data_ptr(), res.data_ptr(), x.numel(), int(input_fl), int(fl), int(bool(signed)), _stream(x)))
    return res


def _relu_(x):
    _i32(x, 'relu_')
    assert x.is_contiguous()
    with torch.cuda.device(x.device):
        check(_lib.lib().f8_relu_i32(x.data_ptr(), x.numel(), _stream(x)))
    return x


def _add_align_(res, x, res_fl, x_fl):
    _i32(res, 'add_align_')
    _i32(x, 'add_align_')
    assert res.shape == x.shape and res.is_contiguous() and x.is_contiguous()
    with torch.cuda.device(res.device):
        check(_lib.lib().f8_add_align_i32(res.data_ptr(), x.data_ptr(), res.numel(), int(res_fl), int(x_fl), None, _stream(res)))
    return res


# ------------------------------------------------------------------------------------------ one-node nets (LRU)
_DETECT_DATA_EDITS = os.environ.get('F8NET_DETECT_DATA_EDITS', '0') == '1'


def set_detect_data_edits(on: bool):
    """Opt into content fingerprints of the op-level plans' parameters.  In-place edits through the parameter itself
    (`weight.copy_()`, `weight[...] = v` under no_grad) bump `Tensor._version` and re-plan by themselves; `weight.data[...] = v`
    has a private version counter and is only seen with this switch on (two reductions and a host sync per parameter tensor and
    call), or after `invalidate_plans()`.  Off by default: the per-call sync serialised the stream on every op-level forward."""
    global _DETECT_DATA_EDITS
    _DETECT_DATA_EDITS = bool(on)


def invalidate_plans():
    """Drop every cached op-level plan (after edits the version counters cannot see, e.g. through `.data`)."""
    _plans.d.clear()


_AUDIT_PERIOD = max(1, int(os.environ.get('F8NET_PLAN_AUDIT_PERIOD', '64')))      # default guard: every N-th reuse of a plan re-reads its parameters
_warned = [False]


def _fingerprint(t, force=False):
    """(sum, position-weighted sum) of an integer tensor; computed on every call only when set_detect_data_edits(True), and on every
    F8NET_PLAN_AUDIT_PERIOD-th reuse of a plan otherwise (`force`)."""
    if not (_DETECT_DATA_EDITS or force):
        return ()
    v = t.detach().reshape(-1).to(torch.int64)
    if v.numel() == 0:
        return (0, 0)
    wgt = torch.arange(1, v.numel() + 1, device=v.device, dtype=torch.int64) % 65521
    return (int(v.sum().item()), int((v * wgt).sum().item()))


class _PlanCache:
    def __init__(self, cap=512):
        self.cap = cap
        self.d = collections.OrderedDict()

    def get(self, key, tensors, n, build):
        """key: hashable geometry; tensors: the parameter tensors the plan snapshots (identity + in-place version checked)."""
        ent = self.d.get(key)
        ver = tuple(None if t is None else (t._version, t.data_ptr()) + _fingerprint(t) for t in tensors)
        if ent is not None:
            refs, ever, net, audit = ent
            same = all((r is None and t is None) or (r is not None and r() is t) for r, t in zip(refs, tensors))
            if same and ever == ver and net.max_batch >= n:
                # default guard against edits no version counter sees (`weight.data[...] = v`): every _AUDIT_PERIOD-th reuse the
                # parameters are re-read (two reductions + one host sync per tensor) and compared with what the plan was built from
                audit[0] += 1
                stale = False
                if not _DETECT_DATA_EDITS and audit[0] % _AUDIT_PERIOD == 0:
                    stale = tuple(None if t is None else _fingerprint(t, True) for t in tensors) != audit[1]
                    if stale and not _warned[0]:
                        _warned[0] = True
                        import warnings
                        warnings.warn('f8net: a parameter of an op-level module was edited through `.data` (no version counter sees that); the plan was rebuilt '
                                      f'at the periodic audit (every {_AUDIT_PERIOD} calls).  Call f8net_amd.torch_ops.invalidate_plans() after such edits, or '
                                      'set_detect_data_edits(True) to check on every call.')
                if not stale:
                    self.d.move_to_end(key)
                    return net
        net = build(max(n, 1))
        self.d[key] = (tuple(None if t is None else weakref.ref(t) for t in tensors), ver, net,
                       [0, tuple(None if t is None else _fingerprint(t, True) for t in tensors)])
        self.d.move_to_end(key)
        while len(self.d) > self.cap:
            self.d.popitem(last=False)
        return net


_plans = _PlanCache()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _conv_out(n, k, stride, pad, dilation):
    return (n + 2 * pad - dilation * (k - 1) - 1) // stride + 1


def _conv2d(x, weight, bias, stride, pad, groups, weight_fl, input_fl, input_signed, dilation=1):
    _i32(x, 'conv2d')
    x = x.contiguous()
    N, C, H, W = x.shape
    key = ('conv', x.device.index, C, H, W, id(weight), tuple(weight.shape), None if bias is None else id(bias), stride, pad, groups, weight_fl, input_fl,
           bool(input_signed), dilation)

    def build(n):
        net = F8Net()
        accept_grouped(net, [(C, groups)])
        t = net.input(C, H, W, input_fl)
        t = net.conv(t, _np(weight), _np(bias), stride=stride, pad=pad, groups=groups, weight_fl=weight_fl, input_fl=input_fl,
                     input_signed=input_signed, quant_input=False, relu=False, dilation=dilation)
        net.output(t, as_float=False)
        return net.finalize(n)

    net = _plans.get(key, (weight, bias), N, build)
    k = weight.shape[2]
    P, Q = _conv_out(H, k, stride, pad, dilation), _conv_out(W, k, stride, pad, dilation)
    return net.run(x).view(N, weight.shape[0], P, Q)


def _rect_out(n, k, stride, pad0, pad1, dilation):
    return (n + pad0 + pad1 - dilation * (k - 1) - 1) // stride + 1


def _conv2d_rect(x, weight, bias, stride, pads, groups, weight_fl, input_fl, input_signed, dilation=1):
    """nn.Conv2d with tuple arguments behind an explicit zero pad (f8_net_conv_rect): stride (sh, sw), pads (top, left, bottom, right)."""
    _i32(x, 'conv2d_rect')
    x = x.contiguous()
    N, C, H, W = x.shape
    stride, pads = tuple(int(v) for v in stride), tuple(int(v) for v in pads)
    key = ('conv_rect', x.device.index, C, H, W, id(weight), tuple(weight.shape), None if bias is None else id(bias), stride, pads, groups, weight_fl, input_fl,
           bool(input_signed), dilation)

    def build(n):
        net = F8Net()
        t = net.input(C, H, W, input_fl)
        t = net.conv(t, _np(weight), _np(bias), stride=stride, pad=pads, groups=groups, weight_fl=weight_fl, input_fl=input_fl,
                     input_signed=input_signed, quant_input=False, relu=False, dilation=dilation)
        net.output(t, as_float=False)
        return net.finalize(n)

    net = _plans.get(key, (weight, bias), N, build)
    P, Q = _rect_out(H, weight.shape[2], stride[0], pads[0], pads[2], dilation), _rect_out(W, weight.shape[3], stride[1], pads[1], pads[3], dilation)
    return net.run(x).view(N, weight.shape[0], P, Q)


def _deconv_out(n, k, stride, pad, output_padding):
    return (n - 1) * stride - 2 * pad + k + output_padding


def _conv_transpose2d(x, weight, bias, stride, pad, output_padding, weight_fl, input_fl, input_signed):
    """nn.ConvTranspose2d on int32 (weight [cin, cout, k, k]): one f8_net_conv_transpose launch behind the input launch."""
    _i32(x, 'conv_transpose2d')
    x = x.contiguous()
    N, C, H, W = x.shape
    key = ('deconv', x.device.index, C, H, W, id(weight), tuple(weight.shape), None if bias is None else id(bias), stride, pad, output_padding, weight_fl,
           input_fl, bool(input_signed))

    def build(n):
        net = F8Net()
        t = net.input(C, H, W, input_fl)
        t = net.conv_transpose(t, _np(weight), _np(bias), stride=stride, pad=pad, output_padding=output_padding, weight_fl=weight_fl,
                               input_fl=input_fl, input_signed=input_signed, quant_input=False, relu=False)
        net.output(t, as_float=False)
        return net.finalize(n)

    net = _plans.get(key, (weight, bias), N, build)
    k = weight.shape[2]
    return net.run(x).view(N, weight.shape[1], _deconv_out(H, k, stride, pad, output_padding), _deconv_out(W, k, stride, pad, output_padding))


def _linear(x, weight, bias, weight_fl, input_fl, input_signed):
    _i32(x, 'linear')
    N, C = x.shape[0], weight.shape[1]
    x4 = x.contiguous().view(N, C, 1, 1)
    key = ('fc', x.device.index, C, id(weight), None if bias is None else id(bias), weight_fl, input_fl, bool(input_signed))

    def build(n):
        net = F8Net()
        t = net.input(C, 1, 1, input_fl)
        t = net.linear(t, _np(weight), _np(bias), weight_fl=weight_fl, input_fl=input_fl, input_signed=input_signed, quant_input=False)
        net.output(t, as_float=False)
        return net.finalize(n)

    return _plans.get(key, (weight, bias), N, build).run(x4)


def _avgpool_sum(x):
    _i32(x, 'avgpool_sum')
    x = x.contiguous()
    N, C, H, W = x.shape

    def build(n):
        net = F8Net()
        t = net.input(C, H, W, 0)
        t = net.avgpool_sum(t, 0)
        net.output(t, as_float=False)
        return net.finalize(n)

    return _plans.get(('avg', x.device.index, C, H, W), (), N, build).run(x)


def _avgpool2d_sum(x, k, stride, pad):
    """The wrapping int32 sum of every k x k window (f8_net_avgpool_window, shift 0): [N, C, H, W] -> [N, C, P, Q]."""
    _i32(x, 'avgpool2d_sum')
    x = x.contiguous()
    N, C, H, W = x.shape

    def build(n):
        net = F8Net()
        t = net.input(C, H, W, 0)
        t = net.avgpool(t, k, stride, pad, shift=0)
        net.output(t, as_float=False)
        return net.finalize(n)

    P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return _plans.get(('avg2d', x.device.index, C, H, W, k, stride, pad), (), N, build).run(x).view(N, C, P, Q)


def _maxpool(x, k, stride, pad):
    _i32(x, 'maxpool')
    x = x.contiguous()
    N, C, H, W = x.shape

    def build(n):
        net = F8Net()
        t = net.input(C, H, W, 0)
        t = net.maxpool(t, k, stride, pad)
        net.output(t, as_float=False)
        return net.finalize(n)

    P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return _plans.get(('max', x.device.index, C, H, W, k, stride, pad), (), N, build).run(x).view(N, C, P, Q)


def _channel_shuffle(x, groups):
    """out[:, c] = x[:, (c % groups) * (C / groups) + c / groups] (f8_net_channel_shuffle): [N, C, H, W] -> [N, C, H, W]."""
    _i32(x, 'channel_shuffle')
    x = x.contiguous()
    N, C, H, W = x.shape

    def build(n):
        net = F8Net()
        t = net.input(C, H, W, 0)
        t = net.channel_shuffle(t, groups)
        net.output(t, as_float=False)
        return net.finalize(n)

    return _plans.get(('shuffle', x.device.index, C, H, W, groups), (), N, build).run(x).view(N, C, H, W)


def _pixmap_shape(x, block, order, s2d):
    """The result's [N, C, H, W]; the refusals of f8_net_depth_to_space / f8_net_space_to_depth as ValueError (the meta impl has no handle to ask)."""
    N, C, H, W = x.shape
    r = int(block)
    if order not in ('crd', 'dcr'):
        raise ValueError(f"order {order!r}: 'crd' or 'dcr'")
    if r < 2 or r > 16:
        raise ValueError(f'block {r}: 2 .. 16')
    if s2d:
        if H % r or W % r:
            raise ValueError(f'space_to_depth: the {H} x {W} map is no multiple of block {r}')
        return N, C * r * r, H // r, W // r
    if C % (r * r):
        raise ValueError(f'depth_to_space: the {C} channels are no multiple of block^2 = {r * r}')
    return N, C // (r * r), H * r, W * r


def _pixmap(x, block, order, s2d):
    who = 'space_to_depth' if s2d else 'depth_to_space'
    _i32(x, who)
    x = x.contiguous()
    N, C, H, W = x.shape
    shape = _pixmap_shape(x, block, order, s2d)

    def build(n):
        net = F8Net()
        t = net.input(C, H, W, 0)
        t = net.space_to_depth(t, block, order) if s2d else net.depth_to_space(t, block, order)
        net.output(t, as_float=False)
        return net.finalize(n)

    return _plans.get((who, x.device.index, C, H, W, int(block), order), (), N, build).run(x).view(shape)


def _depth_to_space(x, block, order):
    """f8_net_depth_to_space: [N, C r^2, H, W] -> [N, C, H r, W r]; order 'crd' is torch.nn.functional.pixel_shuffle."""
    return _pixmap(x, block, order, False)


def _space_to_depth(x, block, order):
    """f8_net_space_to_depth: [N, C, H r, W r] -> [N, C r^2, H, W]; order 'crd' is torch.nn.functional.pixel_unshuffle."""
    return _pixmap(x, block, order, True)


def _mul_q(a, b, a_src_fl, b_src_fl, a_fl, a_signed, b_fl, b_signed, hard_gate_b, relu):
    """int_op_only_fix_quant(a, 8, a_fl, a_src_fl, a_signed) * int_op_only_fix_quant(b', 8, b_fl, b_src_fl, b_signed) with b' = b, or
    clamp(b, -3 * 2^b_src_fl, 3 * 2^b_src_fl) + 3 * 2^b_src_fl when hard_gate_b (f8_net_mul / f8_net_hard_gate): [N, C, H, W] x ([N, C, H, W] |
    [N, C, 1, 1]) -> [N, C, H, W] at fraclen a_fl + b_fl.  `b is a` with hard_gate_b is hard-swish times 6.
    A planned net has one input, so the two operands enter as the channels of one tensor at one fraction length F and leave it through two slices
    (a gate vector: through a 1 x 1 window at stride max(H, W), which also lifts its fraction length).  Only the SHIFTS a_src_fl - a_fl and
    b_src_fl - b_fl and the gate's 3 * 2^b_src_fl enter the values, so the formats are declared relative to F; operand fraction lengths so far apart
    that no F keeps both declared formats inside 0 .. 8 (7 signed) raise ValueError, as do gate vectors on maps wider than 64."""
    _i32(a, 'mul_q')
    _i32(b, 'mul_q')
    same = b is a or (b.data_ptr() == a.data_ptr() and b.shape == a.shape)
    a = a.contiguous()
    N, C, H, W = a.shape
    bcast = tuple(b.shape[2:]) == (1, 1) and (H, W) != (1, 1)
    if tuple(b.shape) != ((N, C, 1, 1) if bcast else (N, C, H, W)):
        raise ValueError(f'mul_q: b is {tuple(b.shape)}: neither a\'s shape {tuple(a.shape)} nor [{N}, {C}, 1, 1]')
    n_a, n_b = a_src_fl - a_fl, b_src_fl - b_fl
    lim_a, lim_b = (7 if a_signed else 8), (7 if b_signed else 8)
    lift = 0                                                        # what the gate vector's window adds to F
    if hard_gate_b and not bcast:
        F = b_src_fl
    elif hard_gate_b:
        F = max(n_a, 0)
        lift = b_src_fl - F
    else:
        F = max(n_a, 0) if bcast else max(n_a, n_b, 0)
        lift = max(0, n_b - F) if bcast else 0
    fa, fb = F - n_a, F + lift - n_b
    if not (0 <= fa <= lim_a and 0 <= fb <= lim_b and lift >= 0 and 0 <= F <= 28) or (bcast and max(H, W) > 64):
        raise ValueError(f'mul_q: shifts {n_a} / {n_b} (hard_gate_b={bool(hard_gate_b)}) on a {H} x {W} map fit no common input fraction length')
    fmt = dict(a_fl=fa, a_signed=a_signed, b_fl=fb, b_signed=b_signed, relu=relu)

    def build(n):
        net = F8Net()
        if same:
            t = net.input(C, H, W, F)
            ta = tb = t
        else:
            t = net.input(2 * C, H, W, F)
            ta, tb = net.slice(t, 0, C), net.slice(t, C, 2 * C)
            if bcast:                                               # pixel (0, 0) of b's channels is the vector
                tb = net.avgpool(tb, 1, max(H, W), 0, shift=lift)
        if hard_gate_b:
            tb = net.hard_gate(tb)
        net.output(net.mul(ta, tb, **fmt), as_float=False)
        return net.finalize(n)

    if same:
        x = a
    elif bcast:
        x = a.new_zeros((N, 2 * C, H, W))
        x[:, :C] = a
        x[:, C:, 0, 0] = b.reshape(N, C)
    else:
        x = torch.cat([a, b.contiguous()], dim=1)
    key = ('mul', a.device.index, C, H, W, same, bcast, F, lift, fa, bool(a_signed), fb, bool(b_signed), bool(hard_gate_b), bool(relu))
    return _plans.get(key, (), N, build).run(x).view(N, C, H, W)


def _table_q(x, table, src_fl, in_fl, in_signed, out_fl):
    """table[int_op_only_fix_quant(x, 8, in_fl, src_fl, in_signed) (+ 128 for a signed format)] (f8_net_table): x int32 [N, C, H, W] at fraction length
    src_fl, `table` 256 int32 entries (any device), the result int32 of x's shape at fraction length out_fl.  Only the SHIFT src_fl - in_fl enters the
    values, so the planned net declares its input at max(shift, 0) and the index format relative to it; a shift below -8 (-7 signed) fits no 8-bit
    format and raises ValueError.  The plan is cached per shape and formats and snapshots the table as a conv's plan snapshots its weights: one plan per
    key, rebuilt when another table tensor arrives or this one is edited in place (identity and version are checked; the plan cache is an LRU of bounded
    size), and the table is read back from the device only when a plan is built.  Keep the table tensor alive between calls (ops.F8Table does)."""
    _i32(x, 'table_q')
    _i32(table, 'table_q')
    if table.numel() != 256:
        raise ValueError(f'table_q: the table has {table.numel()} entries, not 256')
    x = x.contiguous()
    N, C, H, W = x.shape
    n = src_fl - in_fl
    F = max(n, 0)
    if not (0 <= F - n <= (7 if in_signed else 8) and n <= 30):
        raise ValueError(f'table_q: shift {n} ({"signed" if in_signed else "unsigned"}) fits no 8-bit index format')
    def build(k):
        tab = table.detach().cpu().numpy().reshape(256).copy()
        net = F8Net()
        t = net.input(C, H, W, F)
        net.output(net.table(t, tab, in_fl=F - n, in_signed=in_signed, out_fl=out_fl), as_float=False)
        return net.finalize(k)

    key = ('table', x.device.index, C, H, W, n, bool(in_signed), int(out_fl))
    return _plans.get(key, (table,), N, build).run(x).view(N, C, H, W)


def _argmax_channels(x, u8):
    """The class map of int32 logits (f8_net_output_argmax on the input of a one-launch net): out[n, h, w] = the smallest c with the largest
    x[n, c, h, w], signed compare.  [N, C, H, W] -> [N, H, W], uint8 (u8: C <= 255, else the library's F8_ERR_UNSUPPORTED) or int32; C >= 2."""
    _i32(x, 'argmax_channels')
    x = x.contiguous()
    N, C, H, W = x.shape

    def build(n):
        net = F8Net()
        net.output_argmax(net.input(C, H, W, 0), 'u8' if u8 else 'i32')
        return net.finalize(n)

    return _plans.get(('argmax', x.device.index, C, H, W, bool(u8)), (), N, build).run(x).view(N, H, W)


# ------------------------------------------------------------------------------------------ whole nets
_nets = {}


def register_net(net: F8Net) -> int:
    """Make a planned F8Net callable as torch.ops.f8net.net_forward(x, handle).  The registry holds a strong reference until
    unregister_net(handle)."""
    h = id(net)
    _nets[h] = net
    return h


def unregister_net(handle: int):
    _nets.pop(handle, None)


def _net_forward(x, handle):
    return _nets[handle].run(x.contiguous())


def _net_forward_taps(x, handle):
    res = _nets[handle].run(x.contiguous())
    return list(res) if isinstance(res, tuple) else [res]


def _net_forward_f32(images, handle, normalize):
    return _nets[handle].run_f32(images.contiguous(), normalize)


# ------------------------------------------------------------------------------------------ registration
_CUDA = Library('f8net', 'IMPL', 'CUDA')
for _n, _f in (('requant', _requant), ('relu_', _relu_), ('add_align_', _add_align_), ('conv2d', _conv2d), ('conv2d_rect', _conv2d_rect), ('conv_transpose2d', _conv_transpose2d), ('linear', _linear),
               ('avgpool_sum', _avgpool_sum), ('avgpool2d_sum', _avgpool2d_sum), ('maxpool', _maxpool), ('channel_shuffle', _channel_shuffle), ('depth_to_space', _depth_to_space), ('space_to_depth', _space_to_depth), ('mul_q', _mul_q), ('table_q', _table_q), ('argmax_channels', _argmax_channels), ('net_forward', _net_forward), ('net_forward_taps', _net_forward_taps),
               ('net_forward_f32', _net_forward_f32)):
    _CUDA.impl(_n, _f)

_META = Library('f8net', 'IMPL', 'Meta')
_META.impl('requant', lambda x, fl, input_fl, signed: torch.empty_like(x))
_META.impl('relu_', lambda x: x)
_META.impl('add_align_', lambda res, x, res_fl, x_fl: res)
_META.impl('conv2d', lambda x, w, b, stride, pad, groups, wfl, ifl, sgn, dilation=1: x.new_empty(
    (x.shape[0], w.shape[0], _conv_out(x.shape[2], w.shape[2], stride, pad, dilation), _conv_out(x.shape[3], w.shape[3], stride, pad, dilation))))
_META.impl('conv2d_rect', lambda x, w, b, stride, pads, groups, wfl, ifl, sgn, dilation=1: x.new_empty(
    (x.shape[0], w.shape[0], _rect_out(x.shape[2], w.shape[2], stride[0], pads[0], pads[2], dilation),
     _rect_out(x.shape[3], w.shape[3], stride[1], pads[1], pads[3], dilation))))
_META.impl('conv_transpose2d', lambda x, w, b, stride, pad, opad, wfl, ifl, sgn: x.new_empty(
    (x.shape[0], w.shape[1], _deconv_out(x.shape[2], w.shape[2], stride, pad, opad), _deconv_out(x.shape[3], w.shape[3], stride, pad, opad))))
_META.impl('linear', lambda x, w, b, wfl, ifl, sgn: x.new_empty((x.shape[0], w.shape[0])))
_META.impl('avgpool_sum', lambda x: x.new_empty((x.shape[0], x.shape[1])))
_META.impl('avgpool2d_sum', lambda x, k, stride, pad: x.new_empty(
    (x.shape[0], x.shape[1], (x.shape[2] + 2 * pad - k) // stride + 1, (x.shape[3] + 2 * pad - k) // stride + 1)))
_META.impl('maxpool', lambda x, k, stride, pad: x.new_empty(
    (x.shape[0], x.shape[1], (x.shape[2] + 2 * pad - k) // stride + 1, (x.shape[3] + 2 * pad - k) // stride + 1)))
_META.impl('channel_shuffle', lambda x, groups: torch.empty_like(x))
_META.impl('depth_to_space', lambda x, block, order: x.new_empty(_pixmap_shape(x, block, order, False)))
_META.impl('space_to_depth', lambda x, block, order: x.new_empty(_pixmap_shape(x, block, order, True)))
_META.impl('mul_q', lambda a, b, a_src_fl, b_src_fl, a_fl, a_signed, b_fl, b_signed, hard_gate_b, relu: torch.empty_like(a))
_META.impl('table_q', lambda x, table, src_fl, in_fl, in_signed, out_fl: torch.empty_like(x))
_META.impl('argmax_channels', lambda x, u8: x.new_empty((x.shape[0], x.shape[2], x.shape[3]), dtype=torch.uint8 if u8 else torch.int32))
_KIND_DTYPE = (torch.int32, torch.float32, torch.uint8, torch.int32)      # F8Net.output_kinds: int32 / float32 values, a class map as uint8 / int32 ([N, H, W])
_META.impl('net_forward', lambda x, handle: x.new_empty((x.shape[0], _nets[handle].out_elems), dtype=_KIND_DTYPE[_nets[handle].output_kinds[0]]))
_META.impl('net_forward_taps', lambda x, handle: [x.new_empty((x.shape[0], _nets[handle].out_elems), dtype=_KIND_DTYPE[_nets[handle].output_kinds[0]])] + [
    x.new_empty((x.shape[0], H, W) if kind >= 2 else (x.shape[0], C, H, W), dtype=_KIND_DTYPE[kind])
    for (C, H, W, _, _), kind in zip(_nets[handle].outputs[1:], _nets[handle].output_kinds[1:])])
_META.impl('net_forward_f32', lambda x, handle, normalize: x.new_empty((x.shape[0], _nets[handle].out_elems),
                                                                      dtype=torch.float32 if _nets[handle].out_float else torch.int32))
