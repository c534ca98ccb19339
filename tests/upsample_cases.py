"""Case table, reference and graph builder of the tests of upsampling (f8_net_upsample / `F8Net.upsample`, f8_upsample.hip):
tests/test_upsample_plan.py (acceptance, refusals, mode tokens, kernel symbols, forms, launch_info, fused nets, the ONNX round trip; no GPU) and
tests/test_gpu_upsample.py (every case on both legs, bit for bit on the device).  No test functions here.

The reference (ref_ops.upsample_ref) is numpy on int64, wrapped to int32 at the end: nearest is `np.repeat` along H and W; bilinear applies, per axis of n values and for
output index o = s i + j (0 <= j < s), the integer weights of include/f8net.h
    j <  s / 2:  (s - 2j - 1) x[max(i - 1, 0)] + (s + 2j + 1) x[i]
    j >= s / 2:  (3s - 2j - 1) x[i] + (2j + 1 - s) x[min(i + 1, n - 1)]
over H and then over W: the exact half-pixel interpolation times 4 s^2 = 2^(2k + 2), fraclen + 2k + 2.  `pin_to_torch` holds it against
torch.nn.functional.interpolate in float64 with exact equality (tests/test_upsample_plan.py runs it on non-wrapping inputs).

Unless a builder says otherwise a case is  input (8 channels, 0 .. 255, fraclen 8) -> a 1x1 producer conv that reads it as it is, C outputs at
fraclen 13 -> upsample -> readers: one 32-output 1x1 conv per (input_fl, signed), summed (concat_cases.readers).

The expected plan token of every case, on both legs of option upsample_i8, and the forms its launch writes are WRITTEN BY HAND (the rule:
DESIGN.md 4.5j); nothing here asks the planner for them."""
import sys

import numpy as np

import graph_cases
from concat_cases import FUSE_ALL, X_FL, producer, readers  # noqa: F401  (the tests take them from here)
from f8net_amd import synth
from graph_cases import launch_lines
from ref_ops import bilinear_exact

I8, N32, B32 = 'upsample_nearest_i8:', 'upsample_nearest_i32:', 'upsample_bilinear_i32:'
SYMBOL = {I8: 'f8::upsample_i8_kernel', N32: 'f8::upsample_i32_kernel<false>', B32: 'f8::upsample_i32_kernel<true>'}


def pin_to_torch(x, k):
    """bilinear_exact against torch in float64: exact equality (|x| 2^(2k + 2) stays far below 2^53)."""
    import torch
    import torch.nn.functional as F
    want = F.interpolate(torch.from_numpy(np.asarray(x, np.float64)), scale_factor=1 << k, mode='bilinear', align_corners=False) * 2.0 ** (2 * k + 2)
    got = bilinear_exact(x, k)
    assert np.abs(got).max() < 2 ** 52
    np.testing.assert_array_equal(got.astype(np.float64), want.numpy())


# ---- the builders.  Each returns (output tensor ids in output order, [upsample tensor ids])
def _shift(c):
    """The first reader's requant shift of the upsampled tensor, less what a bilinear upsample adds: what fills 8 bits at the producer."""
    return 13 - (c['readers'][0][0] if c['readers'] else 4)


def _plain(g, x0, c):
    """producer -> upsample -> readers (or the upsample itself as an output, alone or next to a reader)."""
    p = producer(g, x0, 0, c['C'], _shift(c), w_fl=5, relu=c['relu'])
    up = g.upsample(p, c['scale'], c['mode'], label='up')
    outs = []
    if c['readers']:
        outs.append(readers(g, up, c['readers']))
        g.output(outs[0])
    if c['out']:
        outs.append(up)
        g.output(up, as_float=c.get('as_float', False))
    return outs, [up]


def _coarse(g, x0, c):
    """The coarse level of a two-level case: the input max-pooled by the case's scale (the fine map is the input's)."""
    s = c['scale'] if isinstance(c['scale'], int) else c['scale'][0]
    return g.maxpool(x0, s, s, 0)


def _fpn(g, x0, c):
    """FPN top-down step: a producer on the coarse level, upsampled, joined with a lateral 1x1 conv of the fine level (fraclen 12 against 13: the
    join shifts it by 1), one int8 reader behind the join."""
    top = producer(g, _coarse(g, x0, c), 0, c['C'], 9, w_fl=5, relu=True)
    up = g.upsample(top, c['scale'], c['mode'], label='up')
    lateral = producer(g, x0, 1, c['C'], 8, w_fl=4, relu=False)
    out = readers(g, g.add(up, lateral, relu=False), [(4, False)])
    g.output(out)
    return [out], [up]


def _unet(g, x0, c):
    """U-Net decoder step: the upsampled coarse level concatenated with a skip (a producer on the fine level at the upsample's fraclen), one int8
    reader behind the concat.  c['opts'] chooses the concat's mode; the byte-gather mode asks the upsample for the concat's int8 format."""
    top = producer(g, _coarse(g, x0, c), 0, c['C'], 9, w_fl=5, relu=True)
    up = g.upsample(top, c['scale'], c['mode'], label='up')
    gain = g.v[up][1] - g.v[top][1]
    skip = producer(g, x0, 1, 24, 9 + gain, w_fl=5 + gain, relu=True)
    out = readers(g, g.concat([up, skip], label='cat'), [(4, False)])
    g.output(out)
    return [out], [up]


def _wrap(g, x0, c):
    """A 3x3 conv over 32 channels (0 .. 255) with weights 64 .. 127: accumulators around 2^22, interpolated at 16x = times 2^10: the exact sums
    pass 2^31 and the result is their int32 wrap.  The result is the output."""
    w = synth.rand_uniform_int(11, 'upwrapw', (c['C'], 32, 3, 3), 64, 127).astype(np.int32)
    p = g.conv(x0, w, None, pad=1, groups=1, weight_fl=0, input_fl=X_FL, input_signed=False, relu=False, quant_input=False)
    up = g.upsample(p, c['scale'], c['mode'], label='up')
    g.output(up)
    exact = bilinear_exact(g.v[p][0], 4)
    assert (np.abs(exact) >= 2 ** 31).mean() > 0.25, 'the exact sums stay inside int32: the case shows nothing'
    return [up], [up]


def _case(C, H, W, mode, scale, tok, *, tok_off=None, forms=(0, 1), build=_plain, **kw):
    """H x W: the SOURCE map.  tok / tok_off: the expected plan token with option upsample_i8 = 1 / 0; forms: (int32 forms, int8 forms) the launch
    writes with upsample_i8 = 1 — all by hand."""
    c = dict(C=C, H=H, W=W, N=2, mode=mode, scale=scale, tok=tok, tok_off=tok_off or (N32 if mode == 'nearest' else B32), forms=forms, build=build,
             readers=[(4, False)], out=False, relu=True, cin=8, opts={})
    c.update(kw)
    return c


U, S = (4, False), (3, True)
CASES = {
    # ---- nearest
    'n_bcast7': _case(40, 1, 1, 'nearest', (7, 7), I8),                               # the ASPP broadcast; 49 pixels per image, two channel blocks
    'n_bcast33': _case(32, 1, 1, 'nearest', (33, 33), I8),
    'n_1x3': _case(8, 1, 3, 'nearest', (2, 2), I8),
    'n_3x1_w4': _case(8, 3, 1, 'nearest', (1, 4), I8),
    'n_2x2_h4': _case(64, 2, 2, 'nearest', (4, 1), I8),
    'n_3x5_s35': _case(40, 3, 5, 'nearest', (3, 5), I8),
    'n_3x5_two': _case(40, 3, 5, 'nearest', (2, 2), I8, forms=(0, 2), readers=[U, S], relu=False),     # 60 pixels per image
    'n_7x7_three': _case(64, 7, 7, 'nearest', (2, 2), N32, forms=(1, 2), readers=[U, S, (5, False)], relu=False),      # a third format: int32 + `requant:`
    'n_fpn': _case(40, 3, 5, 'nearest', (2, 2), N32, forms=(1, 0), build=_fpn),
    'n_unet_i8': _case(40, 3, 5, 'nearest', (2, 2), I8, build=_unet),
    'n_unet_i32': _case(40, 3, 5, 'nearest', (2, 2), N32, forms=(1, 0), build=_unet, opts={'concat_i8': 0}),
    'n_out': _case(40, 3, 5, 'nearest', (2, 2), N32, forms=(1, 0), readers=None, out=True),
    'n_out_f32': _case(8, 7, 7, 'nearest', (2, 2), N32, forms=(1, 0), readers=None, out=True, as_float=True),
    'n_out_reader': _case(64, 2, 2, 'nearest', (2, 2), N32, forms=(1, 1), out=True),
    # ---- bilinear (always the int32 mode)
    'b_1x1_k1': _case(8, 1, 1, 'bilinear', 2, B32),                                    # a constant
    'b_1x3_k2': _case(40, 1, 3, 'bilinear', 4, B32),
    'b_3x1_k1': _case(8, 3, 1, 'bilinear', 2, B32),
    'b_2x2_k3': _case(64, 2, 2, 'bilinear', 8, B32),
    'b_3x5_k1': _case(40, 3, 5, 'bilinear', 2, B32),
    'b_3x5_k4': _case(8, 3, 5, 'bilinear', 16, B32),
    'b_7x7_two': _case(64, 7, 7, 'bilinear', 2, B32, forms=(0, 2), readers=[U, S], relu=False),
    'b_7x7_three': _case(40, 7, 7, 'bilinear', 2, B32, forms=(1, 2), readers=[U, S, (5, False)], relu=False),
    'b_fpn': _case(40, 3, 5, 'bilinear', 2, B32, forms=(1, 0), build=_fpn),
    'b_unet_i8': _case(40, 3, 5, 'bilinear', 2, B32, build=_unet),
    'b_unet_i32': _case(40, 3, 5, 'bilinear', 2, B32, forms=(1, 0), build=_unet, opts={'concat_i8': 0}),
    'b_out': _case(40, 7, 7, 'bilinear', 4, B32, forms=(1, 0), readers=None, out=True),
    'b_out_f32': _case(8, 3, 5, 'bilinear', 2, B32, forms=(1, 0), readers=None, out=True, as_float=True),
    'b_out_reader': _case(64, 3, 5, 'bilinear', 2, B32, forms=(1, 1), out=True),
    'b_wrap': _case(40, 3, 3, 'bilinear', 16, B32, forms=(1, 0), build=_wrap, cin=32),
}


def input_hw(c):
    """The input's map: the source map, except where the case pools the input down to its coarse level first."""
    if c['build'] in (_fpn, _unet):
        s = c['scale'] if isinstance(c['scale'], int) else c['scale'][0]
        return c['H'] * s, c['W'] * s
    return c['H'], c['W']


def make_input(name, n=None):
    c = CASES[name]
    return synth.rand_uniform_int(5, f'upx{name}', (n or c['N'], c['cin']) + input_hw(c), 0, 255).astype(np.int32)


def upsample_lines(net):
    """[(launch index, plan token, kernel symbol)] of the handle's upsample launches, in launch order."""
    return launch_lines(net, 'upsample_')


graph_cases.bind_cases(sys.modules[__name__])      # build_graph, reference, plan, int_graph
