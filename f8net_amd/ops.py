"""Op-level seam: drop-in replacements for the pieces `IntBlock.forward` / `IntModel.forward` call.

Same names, argument meaning and error behaviour as the reference
(/root/reference/models/fix_quant_ops.py:90-134 and the int `nn.Conv2d` / `nn.Linear` built by
`int_conv` :680-714 / `int_fc` :1165-1195), operating on int32 tensors that live in HBM.  Every
function here ends in a HIP kernel of libf8net.so — through `torch.ops.f8net.*` (torch_ops.py), i.e. the PyTorch dispatcher
over the C ABI; there is no CPU path.

This is the parity granularity (one launch chain per reference op, NCHW int32 at every seam).  The
performance path is the fused whole-net plan in `f8net_amd.net` / `f8net_amd.int_model`.
"""
import torch
import torch.nn as nn

from . import tables
from . import torch_ops  # noqa: F401  (registers torch.ops.f8net.*; every function below goes through the dispatcher)


def _require_dev_i32(t, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f'{who}: expects a CUDA/HIP tensor (no CPU path)')
    if t.dtype != torch.int32:
        raise TypeError(f'{who}: expects int32, got {t.dtype}')


def int_op_only_fix_quant(input, wl=8, fl=0, input_fl=0, signed=True):
    """fix_quant_ops.py:90-114.  Returns a new int32 tensor tagged with `.output_fraclen = fl`."""
    assert wl >= 0
    assert fl >= 0
    if signed:
        assert fl <= wl - 1
    else:
        assert fl <= wl
    assert type(wl) == int
    assert type(fl) == int
    if wl != 8:
        raise NotImplementedError('only the 8-bit word length the reference nets use is built')
    _require_dev_i32(input, 'int_op_only_fix_quant')
    res = torch.ops.f8net.requant(input, int(fl), int(input_fl), bool(signed))
    setattr(res, 'output_fraclen', fl)
    return res


def relu_(x):
    """nn.ReLU(inplace=True) on an int32 tensor (fix_resnet.py:39,77)."""
    _require_dev_i32(x, 'relu_')
    return torch.ops.f8net.relu_(x)


def add_align_(res, x, res_fraclen, x_fraclen):
    """Residual join of fix_resnet.py:40-54: res (+)= x after aligning fraclens, clamp; in place on
    `res`.  Returns (res, output_fraclen)."""
    _require_dev_i32(res, 'add_align_')
    _require_dev_i32(x, 'add_align_')
    torch.ops.f8net.add_align_(res, x, int(res_fraclen), int(x_fraclen))
    out_fl = max(int(res_fraclen), int(x_fraclen))
    setattr(res, 'output_fraclen', out_fl)
    return res, out_fl


class _Scalars:
    """(weight_fraclen, input_fraclen) of a module as Python ints, re-read only when the buffers were edited (an `.item()`
    on a device-resident buffer is a synchronisation: not once per forward)."""

    def __init__(self):
        self.ver, self.val = None, None

    def get(self, m):
        ver = (m.weight_fraclen._version, m.weight_fraclen.data_ptr(), m.input_fraclen._version, m.input_fraclen.data_ptr())
        if ver != self.ver:
            self.val = (int(m.weight_fraclen.reshape(-1)[0].item()), int(m.input_fraclen.reshape(-1)[0].item()))
            self.ver = ver
        return self.val


class F8Conv2d(nn.Conv2d):
    """The integer `nn.Conv2d` of `int_conv` (fix_quant_ops.py:680-714) with a HIP forward (`torch.ops.f8net.conv2d`).

    Same parameters / buffers / attributes as the reference export: int32 `weight`, `bias`, buffers
    `weight_fraclen` (0-dim) and `input_fraclen` ([1]), attribute `input_symmetric`, `int_op_only`.
    forward(x): x int32 NCHW holding input_fraclen-format 8-bit integers -> int32 NCHW.  The op plans per (weight tensor,
    its in-place version, input shape, device): editing `weight` / `bias` in place re-plans on the next forward."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, groups=1,
                 input_symmetric=False, dilation=1):
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                         dilation=dilation, groups=groups, bias=True)
        self.weight.requires_grad_(False)
        self.bias.requires_grad_(False)
        self.weight.data = torch.zeros(self.weight.shape, dtype=torch.int32)
        self.bias.data = torch.zeros(self.bias.shape, dtype=torch.int32)
        self.register_buffer('weight_fraclen', torch.zeros((), dtype=torch.int32))
        self.register_buffer('input_fraclen', torch.zeros(1, dtype=torch.int32))
        self.input_symmetric = bool(input_symmetric)
        self.int_op_only = True
        self._fl = _Scalars()

    def forward(self, x):
        _require_dev_i32(x, 'F8Conv2d')
        w_fl, in_fl = self._fl.get(self)
        kh, kw = self.kernel_size
        if kh == kw and self.stride[0] == self.stride[1] and self.padding[0] == self.padding[1] and self.dilation[0] == self.dilation[1]:
            return torch.ops.f8net.conv2d(x, self.weight, self.bias, self.stride[0], self.padding[0], self.groups, w_fl, in_fl,
                                          self.input_symmetric, self.dilation[0])
        # nn.Conv2d's tuple kernel_size / stride / padding / dilation (f8_net_conv_rect): one dilation for the axes with more than one tap
        dil = {d for d, k in zip(self.dilation, self.kernel_size) if k > 1}
        if len(dil) > 1:
            raise ValueError(f'F8Conv2d: dilation {self.dilation} on kernel {self.kernel_size}: only equal dilations on the axes with more than one tap')
        ph, pw = self.padding
        return torch.ops.f8net.conv2d_rect(x, self.weight, self.bias, list(self.stride), [ph, pw, ph, pw], self.groups, w_fl, in_fl,
                                           self.input_symmetric, dil.pop() if dil else 1)


class F8ConvTranspose2d(nn.ConvTranspose2d):
    """An integer `nn.ConvTranspose2d` in the manner of `int_conv` (the reference names a ReLUClipFXQConvTransposeBN, fix_quant_ops.py:9, and defines none)
    with a HIP forward (`torch.ops.f8net.conv_transpose2d`): int32 `weight` [cin, cout, k, k], `bias`, buffers `weight_fraclen` / `input_fraclen`,
    attribute `input_symmetric`, as F8Conv2d.  forward(x): x int32 NCHW holding input_fraclen-format 8-bit integers -> int32 NCHW."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0, input_symmetric=False):
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, output_padding=output_padding, bias=True)
        self.weight.requires_grad_(False)
        self.bias.requires_grad_(False)
        self.weight.data = torch.zeros(self.weight.shape, dtype=torch.int32)
        self.bias.data = torch.zeros(self.bias.shape, dtype=torch.int32)
        self.register_buffer('weight_fraclen', torch.zeros((), dtype=torch.int32))
        self.register_buffer('input_fraclen', torch.zeros(1, dtype=torch.int32))
        self.input_symmetric = bool(input_symmetric)
        self.int_op_only = True
        self._fl = _Scalars()

    def forward(self, x):
        _require_dev_i32(x, 'F8ConvTranspose2d')
        w_fl, in_fl = self._fl.get(self)
        return torch.ops.f8net.conv_transpose2d(x, self.weight, self.bias, self.stride[0], self.padding[0], self.output_padding[0], w_fl, in_fl,
                                                self.input_symmetric)


class F8Linear(nn.Linear):
    """The integer `nn.Linear` of `int_fc` (fix_quant_ops.py:1165-1195) with a HIP forward (`torch.ops.f8net.linear`)."""

    def __init__(self, in_features, out_features, input_symmetric=False):
        super().__init__(in_features, out_features, bias=True)
        self.weight.requires_grad_(False)
        self.bias.requires_grad_(False)
        self.weight.data = torch.zeros(self.weight.shape, dtype=torch.int32)
        self.bias.data = torch.zeros(self.bias.shape, dtype=torch.int32)
        self.register_buffer('weight_fraclen', torch.zeros((), dtype=torch.int32))
        self.register_buffer('input_fraclen', torch.zeros(1, dtype=torch.int32))
        self.input_symmetric = bool(input_symmetric)
        self.int_op_only = True
        self._fl = _Scalars()

    def forward(self, x):
        _require_dev_i32(x, 'F8Linear')
        w_fl, in_fl = self._fl.get(self)
        return torch.ops.f8net.linear(x, self.weight, self.bias, w_fl, in_fl, self.input_symmetric)


class FXQAvgPool2d(nn.Module):
    """fix_quant_ops.py:117-134, int branch: int64 sum over H,W, truncate, fraclen += shiftnum."""

    def __init__(self, kernel_size):
        super().__init__()
        self.kernel_size = kernel_size
        self.shiftnum = int(torch.round(torch.log2(torch.tensor(float(kernel_size ** 2)))).item())
        self.int_op_only = True

    def forward(self, x):
        _require_dev_i32(x, 'FXQAvgPool2d')
        output_fraclen = x.output_fraclen + self.shiftnum
        assert output_fraclen <= 32
        res = torch.ops.f8net.avgpool_sum(x)
        setattr(res, 'output_fraclen', output_fraclen)
        return res


class F8AvgPool2d(nn.Module):
    """Windowed average pooling in FXQAvgPool2d's manner (fix_quant_ops.py:117-138, int branch, per window): the integer SUM of each kernel_size x
    kernel_size window (a tap in the padding adds 0; count_include_pad=True's constant divisor is left to the next layer's weights) with a HIP forward
    (`torch.ops.f8net.avgpool2d_sum`), fraclen += shiftnum = round(log2(kernel_size^2)).  `stride` defaults to `kernel_size`."""

    def __init__(self, kernel_size, stride=None, padding=0):
        super().__init__()
        self.kernel_size, self.stride, self.padding = int(kernel_size), int(kernel_size if stride is None else stride), int(padding)
        self.shiftnum = int(torch.round(torch.log2(torch.tensor(float(self.kernel_size ** 2)))).item())
        self.int_op_only = True

    def forward(self, x):
        _require_dev_i32(x, 'F8AvgPool2d')
        output_fraclen = x.output_fraclen + self.shiftnum
        assert output_fraclen <= 32
        res = torch.ops.f8net.avgpool2d_sum(x, self.kernel_size, self.stride, self.padding)
        setattr(res, 'output_fraclen', output_fraclen)
        return res


class F8ArgMax(nn.Module):
    """torch.argmax(x, dim=1) on int32 device tensors with a HIP forward (`torch.ops.f8net.argmax_channels`): the class map [N, H, W] of logits
    [N, C, H, W], the smallest index winning a tie.  dtype 'u8' (at most 255 channels) or 'i32'."""

    def __init__(self, dtype='u8'):
        super().__init__()
        if dtype not in ('u8', 'i32'):
            raise ValueError(f"F8ArgMax dtype {dtype!r}: 'u8' or 'i32'")
        self.u8 = dtype == 'u8'
        self.int_op_only = True

    def forward(self, x):
        _require_dev_i32(x, 'F8ArgMax')
        return torch.ops.f8net.argmax_channels(x, self.u8)


class F8ChannelShuffle(nn.Module):
    """nn.ChannelShuffle(groups) on int32 device tensors with a HIP forward (`torch.ops.f8net.channel_shuffle`): out[:, c] = x[:, (c % groups) *
    (C / groups) + c / groups].  A permutation of channels: the fraclen is the input's."""

    def __init__(self, groups):
        super().__init__()
        self.groups = int(groups)
        self.int_op_only = True

    def forward(self, x):
        _require_dev_i32(x, 'F8ChannelShuffle')
        res = torch.ops.f8net.channel_shuffle(x, self.groups)
        if hasattr(x, 'output_fraclen'):
            setattr(res, 'output_fraclen', x.output_fraclen)
        return res


class F8PixelShuffle(nn.Module):
    """nn.PixelShuffle(r) on int32 device tensors with a HIP forward (`torch.ops.f8net.depth_to_space`, order 'crd'): [N, C r^2, H, W] ->
    [N, C, H r, W r].  A rearrangement of values: the fraclen is the input's."""

    def __init__(self, upscale_factor):
        super().__init__()
        self.upscale_factor = int(upscale_factor)
        self.int_op_only = True

    def forward(self, x):
        _require_dev_i32(x, 'F8PixelShuffle')
        res = torch.ops.f8net.depth_to_space(x, self.upscale_factor, 'crd')
        if hasattr(x, 'output_fraclen'):
            setattr(res, 'output_fraclen', x.output_fraclen)
        return res


class F8PixelUnshuffle(nn.Module):
    """nn.PixelUnshuffle(r) on int32 device tensors with a HIP forward (`torch.ops.f8net.space_to_depth`, order 'crd'): [N, C, H r, W r] ->
    [N, C r^2, H, W].  A rearrangement of values: the fraclen is the input's."""

    def __init__(self, downscale_factor):
        super().__init__()
        self.downscale_factor = int(downscale_factor)
        self.int_op_only = True

    def forward(self, x):
        _require_dev_i32(x, 'F8PixelUnshuffle')
        res = torch.ops.f8net.space_to_depth(x, self.downscale_factor, 'crd')
        if hasattr(x, 'output_fraclen'):
            setattr(res, 'output_fraclen', x.output_fraclen)
        return res


class F8HardSwish(nn.Module):
    """Six times nn.Hardswish on int32 device tensors with a HIP forward (`torch.ops.f8net.mul_q` with the hard gate on its own operand):
    x_q * relu6(x + 3) with x_q = x requantised to (x_fl, x_signed) and the gate, 0 .. 6, requantised to unsigned g_fl; the result's fraclen is
    x_fl + g_fl.  The 1 / 6 is a constant real scale: fold it into the next layer's weights."""

    def __init__(self, x_fl, x_signed=True, g_fl=5):
        super().__init__()
        self.x_fl, self.x_signed, self.g_fl = int(x_fl), bool(x_signed), int(g_fl)
        self.int_op_only = True

    def forward(self, x):
        _require_dev_i32(x, 'F8HardSwish')
        fl = x.output_fraclen
        res = torch.ops.f8net.mul_q(x, x, fl, fl, self.x_fl, self.x_signed, self.g_fl, False, True, False)
        setattr(res, 'output_fraclen', self.x_fl + self.g_fl)
        return res


class F8ChannelGate(nn.Module):
    """The scale of a squeeze-and-excitation block with a hard-sigmoid gate, times 6: x_q * relu6(s + 3) broadcast over H x W, x [N, C, H, W]
    requantised to (x_fl, x_signed), s [N, C, 1, 1] the second FC's result, its gate requantised to unsigned g_fl (`torch.ops.f8net.mul_q`).
    The result's fraclen is x_fl + g_fl; the 1 / 6 is left to the next layer's weights."""

    def __init__(self, x_fl, x_signed=False, g_fl=5):
        super().__init__()
        self.x_fl, self.x_signed, self.g_fl = int(x_fl), bool(x_signed), int(g_fl)
        self.int_op_only = True

    def forward(self, x, s):
        _require_dev_i32(x, 'F8ChannelGate')
        _require_dev_i32(s, 'F8ChannelGate')
        s4 = s.reshape(s.shape[0], s.shape[1], 1, 1)
        res = torch.ops.f8net.mul_q(x, s4, x.output_fraclen, s.output_fraclen, self.x_fl, self.x_signed, self.g_fl, False, True, False)
        setattr(res, 'output_fraclen', self.x_fl + self.g_fl)
        return res


class F8Table(nn.Module):
    """Any pointwise function on int32 device tensors with a HIP forward (`torch.ops.f8net.table_q`, f8_net_table): x requantised to
    (in_fl, in_signed) indexes `table` (256 int32 entries: f8net_amd.tables.from_function and friends); the result's fraclen is out_fl."""

    def __init__(self, table, in_fl, in_signed, out_fl):
        super().__init__()
        self.register_buffer('table', torch.as_tensor(table, dtype=torch.int32).reshape(256).clone())
        self.in_fl, self.in_signed, self.out_fl = int(in_fl), bool(in_signed), int(out_fl)
        self.int_op_only = True

    def forward(self, x):
        _require_dev_i32(x, type(self).__name__)
        res = torch.ops.f8net.table_q(x, self.table, x.output_fraclen, self.in_fl, self.in_signed, self.out_fl)
        setattr(res, 'output_fraclen', self.out_fl)
        return res


class F8Sigmoid(F8Table):
    """nn.Sigmoid of x read at (in_fl, in_signed), rounded half to even to fraclen out_fl."""

    def __init__(self, in_fl, in_signed=True, out_fl=12):
        super().__init__(tables.sigmoid(in_fl, in_signed, out_fl), in_fl, in_signed, out_fl)


class F8Swish(F8Table):
    """nn.SiLU of x read at (in_fl, in_signed), rounded half to even to fraclen out_fl."""

    def __init__(self, in_fl, in_signed=True, out_fl=8):
        super().__init__(tables.swish(in_fl, in_signed, out_fl), in_fl, in_signed, out_fl)


class F8MaxPool2d(nn.Module):
    """Head max-pool (fix_resnet.py:358-359 float detour / FXQMaxPool2d): exact integer max."""

    def __init__(self, kernel_size=3, stride=2, padding=1):
        super().__init__()
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding

    def forward(self, x):
        _require_dev_i32(x, 'F8MaxPool2d')
        return torch.ops.f8net.maxpool(x, self.kernel_size, self.stride, self.padding)


class IntReLU(nn.Module):
    def forward(self, x):
        return relu_(x)
