"""The CPU reference of every op the oracle does not have, one function per op, in numpy on the int32 tensors a graph carries.  refgraph.RefGraph and
refgraph.graph_forward evaluate with these and nothing else; the case modules and tests take them from here.  `oracle/` stays as it is: requant,
conv2d (groups 1 or cin), linear, add_align, relu, maxpool and avgpool_sum are the oracle's own.  No test functions here.

Where a reference is pinned against torch or the oracle (`pin_to_torch` / `pin_to_oracle`), the pin stands in the op's case module and the op's
_plan test calls it."""
import math

import numpy as np

from f8net_amd.onnx_import import upsample_fl_gain
from oracle import oracle

_oracle_conv2d = oracle.conv2d


def wrap32(y):
    return ((np.asarray(y, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


# ---- convs: any groups (the oracle per group), any dilation (zero-stuffed weights)
def grouped_conv2d(x, w, b, stride, pad, groups=1):
    """oracle.conv2d for any groups: 1 < groups < cin is the oracle per group, concatenated along the channels (wrapping int32 arithmetic is
    order-free)."""
    cin = x.shape[1]
    if groups == 1 or groups == cin:
        return _oracle_conv2d(x, w, b, stride, pad, groups)
    cg, kg = cin // groups, w.shape[0] // groups
    assert cg * groups == cin and kg * groups == w.shape[0] and w.shape[1] == cg
    x, w = np.asarray(x), np.asarray(w)
    return np.concatenate([_oracle_conv2d(np.ascontiguousarray(x[:, g * cg:(g + 1) * cg]), np.ascontiguousarray(w[g * kg:(g + 1) * kg]),
                                          None if b is None else np.ascontiguousarray(np.asarray(b)[g * kg:(g + 1) * kg]), stride, pad, 1)
                           for g in range(groups)], axis=1)


def stuffed(w, d):
    """[cout, cin / groups, K, K] -> the zero-stuffed [cout, cin / groups, d (K - 1) + 1, ...] kernel of the same conv at dilation 1."""
    w = np.asarray(w)
    if d == 1 or w.shape[2] == 1:
        return w
    K = w.shape[2]
    E = d * (K - 1) + 1
    s = np.zeros(w.shape[:2] + (E, E), w.dtype)
    s[:, :, ::d, ::d] = w
    return s


# ---- transposed conv: the scatter form on int64
def deconv_exact(x, w, b, s, pad, op):
    """(N, cin, H, W) integers, w [cin, cout, k, k], b [cout] or None -> int64 (N, cout, P, Q), not wrapped: every input pixel (ih, iw) adds
    x[ci] * w[ci, co, kh, kw] at (s ih + kh, s iw + kw) of the full (H - 1) s + k + op square, of which the output is the window [pad, pad + P)."""
    x, w = np.asarray(x, np.int64), np.asarray(w, np.int64)
    N, cin, H, W = x.shape
    cout, k = w.shape[1], w.shape[2]
    full = np.zeros((N, cout, (H - 1) * s + k + op, (W - 1) * s + k + op), np.int64)
    for kh in range(k):
        for kw in range(k):
            full[:, :, kh:kh + (H - 1) * s + 1:s, kw:kw + (W - 1) * s + 1:s] += np.einsum('nchw,cd->ndhw', x, w[:, :, kh, kw])
    P, Q = (H - 1) * s - 2 * pad + k + op, (W - 1) * s - 2 * pad + k + op
    y = full[:, :, pad:pad + P, pad:pad + Q]
    assert y.shape[2:] == (P, Q)
    if b is not None:
        y = y + np.asarray(b, np.int64).reshape(1, -1, 1, 1)
    return y


def deconv_ref(x, w, b, s, pad, op):
    return wrap32(deconv_exact(x, w, b, s, pad, op))


# ---- concat: the residual join's alignment next to a zero partner
def concat_align(xs, fls):
    """[(N, C_i, H, W) int32], [fraclen_i] -> (concatenation at the largest fraclen, that fraclen)."""
    fl = max(fls)
    parts = []
    for x, f in zip(xs, fls):
        y, got = oracle.add_align(np.zeros_like(x), x, fl, f)
        assert got == fl
        parts.append(y)
    return np.concatenate(parts, axis=1), fl


# ---- upsample: nearest is np.repeat; bilinear the integer weights of include/f8net.h, per axis
def nearest_exact(x, sh, sw):
    return np.repeat(np.repeat(np.asarray(x, np.int64), sh, axis=2), sw, axis=3)


def _bilinear_axis(x, s, axis):
    n = x.shape[axis]
    i0, i1, wl, wu = [], [], [], []
    for o in range(s * n):
        i, j = divmod(o, s)
        if j < s // 2:
            i0.append(max(i - 1, 0)), i1.append(i), wl.append(s - 2 * j - 1), wu.append(s + 2 * j + 1)
        else:
            i0.append(i), i1.append(min(i + 1, n - 1)), wl.append(3 * s - 2 * j - 1), wu.append(2 * j + 1 - s)
    shape = [1] * x.ndim
    shape[axis] = s * n
    wl, wu = np.array(wl, np.int64).reshape(shape), np.array(wu, np.int64).reshape(shape)
    assert ((wl + wu) == 2 * s).all() and (wl > 0).all() and (wu > 0).all()
    return wl * np.take(x, i0, axis=axis) + wu * np.take(x, i1, axis=axis)


def bilinear_exact(x, k):
    """(N, C, H, W) integers -> the exact half-pixel interpolation times 2^(2k + 2), int64, not wrapped."""
    x = np.asarray(x, np.int64)
    return _bilinear_axis(_bilinear_axis(x, 1 << k, 2), 1 << k, 3)


def upsample_ref(x, fl, scale, mode):
    """-> (int32 values, fraclen)."""
    sh, sw = (scale, scale) if isinstance(scale, int) else scale
    if mode == 'nearest':
        return wrap32(nearest_exact(x, sh, sw)), fl
    k = sh.bit_length() - 1
    assert mode == 'bilinear' and sh == sw == 1 << k and 1 <= k <= 4
    assert upsample_fl_gain((sh, sw)) == 2 * k + 2
    return wrap32(bilinear_exact(x, k)), fl + 2 * k + 2


# ---- windowed average pool: the window sums over the zero-padded map
def default_shift(k):
    """The reference's round(log2(k^2)): what the fraclen grows by."""
    return int(round(math.log2(k * k)))


def sumpool_exact(x, k, stride, pad):
    """(N, C, H, W) integers -> the window sums over the zero-padded map, int64, not wrapped."""
    x = np.asarray(x, np.int64)
    N, C, H, W = x.shape
    P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    assert P >= 1 and Q >= 1
    xp = np.zeros((N, C, H + 2 * pad, W + 2 * pad), np.int64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    y = np.zeros((N, C, P, Q), np.int64)
    for r in range(k):
        for s in range(k):
            y += xp[:, :, r:r + (P - 1) * stride + 1:stride, s:s + (Q - 1) * stride + 1:stride]
    return y


def sumpool_ref(x, fl, k, stride, pad, shift=None):
    """-> (int32 values, fraclen)."""
    return wrap32(sumpool_exact(x, k, stride, pad)), fl + (default_shift(k) if shift is None else shift)


# ---- channel slice and shuffle: fancy indexing
def shuffle_index(C, groups):
    c = np.arange(C)
    return (c % groups) * (C // groups) + c // groups


def channel_shuffle(x, groups):
    return x[:, shuffle_index(x.shape[1], groups)]


def channel_slice(x, first, channels):
    return x[:, np.arange(first, first + channels)]


# ---- fixed-point multiply and hard gate
def mul_operands(a, fl_a, b, fl_b, a_fl, a_signed, b_fl, b_signed):
    """(A, B): the two operands in the mul's formats, int64."""
    return (oracle.requant(a, a_fl, fl_a, a_signed).astype(np.int64), oracle.requant(b, b_fl, fl_b, b_signed).astype(np.int64))


def mul_ref(a, fl_a, b, fl_b, *, a_fl, a_signed, b_fl, b_signed=False, relu=False):
    """-> (product int32 in a's shape, fraclen a_fl + b_fl); b has a's shape or is [N, C, 1, 1].  |product| <= 255 * 255: the wrap never acts."""
    A, B = mul_operands(a, fl_a, b, fl_b, a_fl, a_signed, b_fl, b_signed)
    y = A * B                                                     # (numpy broadcasts [N, C, 1, 1] over H x W)
    if relu:
        y = np.maximum(y, 0)
    return wrap32(y), a_fl + b_fl


def hard_gate_ref(x, fl):
    lim = 3 * 2 ** fl
    return wrap32(np.clip(np.asarray(x, np.int64), -lim, lim) + lim)


# ---- the 256-entry table
def table_index(x, fl, *, in_fl, in_signed):
    """q: the source in the table's index format, int64."""
    return oracle.requant(x, in_fl, fl, in_signed).astype(np.int64)


def table_ref(x, fl, table, *, in_fl, in_signed):
    return np.asarray(table, np.int32)[table_index(x, fl, in_fl=in_fl, in_signed=in_signed) + (128 if in_signed else 0)]
