"""The entries of the 256-entry table op (f8_net_table, `F8Net.table`): a pointwise function sampled on the 8-bit fixed-point grid.

`from_function(fn, in_fl, in_signed, out_fl)` -> int32[256].  Index i stands for the source value q = i (unsigned format, 0 .. 255) or q = i - 128
(signed, -127 .. 127; entry 0 is never read and holds the value of q = -128).  Entry = fn(q / 2^in_fl) * 2^out_fl, evaluated by torch in float64,
rounded half to even and clamped to int32: where the clamp does not act, |entry / 2^out_fl - fn| <= 2^-(out_fl + 1)."""
import numpy as np
import torch

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def grid(in_fl, in_signed):
    """The 256 real arguments in table order (float64)."""
    q = torch.arange(256, dtype=torch.float64) - (128 if in_signed else 0)
    return q / 2.0 ** in_fl


def from_function(fn, in_fl, in_signed, out_fl):
    y = fn(grid(in_fl, in_signed)).to(torch.float64) * 2.0 ** out_fl
    y = torch.clamp(torch.round(y), INT32_MIN, INT32_MAX)          # torch.round: half to even
    return y.numpy().astype(np.int64).astype(np.int32)


def sigmoid(in_fl, in_signed, out_fl):
    return from_function(torch.sigmoid, in_fl, in_signed, out_fl)


def tanh(in_fl, in_signed, out_fl):
    return from_function(torch.tanh, in_fl, in_signed, out_fl)


def swish(in_fl, in_signed, out_fl):
    """x * sigmoid(x) (SiLU)."""
    return from_function(torch.nn.functional.silu, in_fl, in_signed, out_fl)


def mish(in_fl, in_signed, out_fl):
    return from_function(torch.nn.functional.mish, in_fl, in_signed, out_fl)


def gelu(in_fl, in_signed, out_fl):
    return from_function(torch.nn.functional.gelu, in_fl, in_signed, out_fl)


def leaky_relu(slope, in_fl, in_signed, out_fl):
    return from_function(lambda x: torch.nn.functional.leaky_relu(x, slope), in_fl, in_signed, out_fl)


def hard_sigmoid(in_fl, in_signed, out_fl):
    """relu6(x + 3) / 6: the true one, with the 1 / 6 inside (f8_net_hard_gate leaves it to the next conv's weights)."""
    return from_function(torch.nn.functional.hardsigmoid, in_fl, in_signed, out_fl)
